"""The shared ragged front end (probpose_pytorch_amd/_ragged.py) through its three consumers on the GPU: the batch of
tests/ragged_fixture.py (11 detections, three interleaved groups, K = 3, scores tied inside a group and across groups,
one group of a single detection), given once as it is and once shuffled so that both ties arrive the other way round,
through PoseNMS, PoseTracker.update (max_tracks = 4: the tie decides who finds no slot) and CocoKeypointEval
(max_dets = 4: the tie decides who is cut).  Each must agree with its own gauge on the batch as given, exactly as its
own tests demand; the bounds are theirs (tests/test_posenms_gpu.py, test_track_gpu.py, test_cocoeval_gpu.py: u = 2^-53,
|d OKS| <= (2 K + 2) u, keep / ids / born / flags exact, hard-mode scores and filtered keypoints the same bits, soft
scores within 1.001 n ((2 c + 4) / oks_thr + 6) u relative with c = 2 K + 2 and n = 5 picks per image at most,
precision and recall within 2^-52, stats within 1011 * 2^-52).  The fixture conditions those bounds rest on are
asserted on the gauges' values first.
"""
import numpy as np
import pytest
import torch

from tests import cocoeval_reference as CR
from tests import posenms_reference as PR
from tests import ragged_fixture as F
from tests import track_reference as TR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
K, SIGMAS = F.K, np.full(F.K, F.SIGMA)
OKS_THR, VIS_THR, MATCH_THR, MAX_AGE, MAX_TRACKS, MAX_DETS, SMOOTH = 0.9, 0.2, 0.3, 30, 4, 4, (1.0, 0.05, 1.0)
ORDERS = {"given": np.arange(F.M), "shuffled": F.SHUFFLE}
pytest_orders = pytest.mark.parametrize("order", list(ORDERS.values()), ids=list(ORDERS))


def device(order, kpts="kpts"):
    """The batch in ``order`` on the device: (group ids (host), keypoints [M, K, 3] with the visibility as the third
    column, scores, areas)."""
    b = F.batch()
    kp3 = np.concatenate([b[kpts], b["vis"][..., None]], axis=2)[order]
    return (b["pos"][order], torch.from_numpy(kp3).cuda(), torch.from_numpy(b["score"][order]).cuda(),
            torch.from_numpy(b["area"][order]).cuda())


def given(order, idx):
    """Where the batch indices ``idx`` stand in the batch given in ``order``."""
    where = np.empty(F.M, dtype=np.int64)
    where[order] = np.arange(F.M)
    return where[idx]


@pytest_orders
@pytest.mark.parametrize("mode", ["hard", "soft_gaussian"])
def test_posenms(order, mode):
    from probpose_pytorch_amd import PoseNMS
    b, groups = F.batch(), F.groups(order)
    images = [PR.make_image(b["kpts"][idx], b["score"][idx], b["area"][idx], b["vis"][idx]) for _, idx in groups]
    want = PR.run(images, SIGMAS, mode, OKS_THR, VIS_THR, 20)
    for r in want["per_image"]:                         # the fixture conditions of tests/test_posenms_gpu.py
        seen = np.asarray(r["oks_seen"], dtype=np.float64)
        assert seen.size == 0 or np.abs(seen - OKS_THR).min() > 1e-9
        assert all(runner is None or (top == runner and untouched) or top - runner > 1e-9 * abs(top)
                   for top, runner, untouched, _, _ in r["gaps"])
    assert 0 < want["keep"].sum() < F.M or mode != "hard"
    ids, kp3, sc, ar = device(order)
    res = PoseNMS(SIGMAS, mode=mode, oks_thr=OKS_THR, vis_thr=VIS_THR)(ids, kp3, sc, ar)
    assert list(res.image_ids) == [g for g, _ in groups]
    assert res.counts.cpu().numpy().tolist() == want["counts"].tolist()
    keep, scores = res.keep.cpu().numpy(), res.scores.cpu().numpy()
    at = np.concatenate([given(order, idx) for _, idx in groups])       # the gauge's rows in the batch as given
    assert np.array_equal(keep[at], want["keep"])
    if mode == "hard":
        assert scores.tobytes() == F.SCORE[order].tobytes()
    else:
        bound = 1.001 * 5 * ((2 * (2 * K + 2) + 4) / OKS_THR + 6) * U
        worst = float((np.abs(scores[at] - want["scores"]) / (bound * np.abs(want["scores"]))).max())
        print(f"soft_gaussian: worst |d score| / bound = {worst:.4f} (bound {bound:.3e})")
        assert worst <= 1.0


@pytest_orders
def test_tracker_update(order):
    from probpose_pytorch_amd import OneEuro, PoseTracker
    b, groups = F.batch(), F.groups(order)
    gauge = TR.Tracker(SIGMAS, MATCH_THR, MAX_AGE, MAX_TRACKS, VIS_THR, SMOOTH)
    tracker = PoseTracker(SIGMAS, match_thr=MATCH_THR, max_age=MAX_AGE, max_tracks=MAX_TRACKS, vis_thr=VIS_THR,
                          smooth=OneEuro(*SMOOTH))
    bound, events = (2 * K + 2) * U, {}
    for kpts in ("kpts", "kpts2"):
        want = gauge.update({g: TR.make_frame(b[kpts][idx], b["score"][idx], b["area"][idx], b["vis"][idx])
                             for g, idx in groups})
        for r in want.values():                         # the fixture conditions of tests/test_track_gpu.py
            seen = np.asarray(r["oks_seen"], dtype=np.float64)
            assert seen.size == 0 or np.abs(seen - MATCH_THR).min() > 1e-9
            assert all(not best > MATCH_THR or second is None or best - second > 1e-9
                       for best, second, _, _ in r["gaps"])
            for k, v in r["events"].items():
                events[k] = events.get(k, 0) + v
        ids, kp3, sc, ar = device(order, kpts)
        res = tracker.update(kp3, ar, sc, stream_ids=ids)
        assert res.stream_ids == [g for g, _ in groups]
        got = {k: getattr(res, k).cpu().numpy() for k in ("ids", "born", "oks", "keypoints")}
        assert not res.dropped.any()
        for g, idx in groups:
            at, w = given(order, idx), want[g]
            assert np.array_equal(got["ids"][at], w["ids"]) and np.array_equal(got["born"][at], w["born"]), (kpts, g)
            assert np.abs(got["oks"][at] - w["oks"]).max() <= bound, (kpts, g)
            assert got["keypoints"][at].tobytes() == w["keypoints"].tobytes(), (kpts, g)
        assert tracker.overflow.cpu().numpy().tolist() == [gauge.streams[g].overflow for g, _ in groups]
    assert events["birth"] == 9 and events["match"] == 9 and events["overflow"] == 4, events


@pytest_orders
def test_cocoeval(order):
    from probpose_pytorch_amd import CocoKeypointEval
    b = F.batch()
    ev, images = CocoKeypointEval(SIGMAS, max_dets=MAX_DETS), []
    for g in range(3):                                  # the images in the order of their ground truth
        gt = [p for p in b["people"] if p["group"] == g]
        idx = dict(F.groups(order))[g]
        images.append(CR.make_image(np.stack([p["kpts"] for p in gt]), np.stack([p["bbox"] for p in gt]),
                                    [p["area"] for p in gt], None, b["kpts"][idx], b["score"][idx], b["area"][idx],
                                    K=K))
        ev.add_ground_truth(g, images[-1]["gt_kpts"], images[-1]["gt_bbox"], images[-1]["gt_area"])
    want = CR.evaluate(images, SIGMAS, max_dets=MAX_DETS)
    thr = np.minimum(CR.OKS_THRESHOLDS, 1 - 1e-10)
    for r in want["per_image"][0]:                      # the fixture condition of tests/test_cocoeval_gpu.py
        assert r["dt_index"].size <= MAX_DETS
        for row in r["oks"]:
            cand = np.sort(row[row > thr[0] - 1e-9])
            assert all(np.abs(v - thr).min() > 1e-9 for v in cand) and (np.diff(cand) > 1e-9).all()
    assert [r["dt_index"].size for r in want["per_image"][0]] == [4, 4, 1] and 0.05 < want["AP"] < 0.95
    ids, kp3, sc, ar = device(order)
    ev.add_detections(ids, kp3, sc, ar)
    got = ev.evaluate()
    assert np.abs(got["precision"] - want["precision"]).max() <= 2.0 ** -52
    assert np.abs(got["recall"] - want["recall"]).max() <= 2.0 ** -52
    assert max(abs(got[k] - want[k]) for k in CR.STATS) <= 1011 * 2.0 ** -52
