"""PoseTrackEval on the GPU against its gauge (tests/trackeval_reference.py): every integer exactly, the OKS sum within
relative 1e-12 (more than TP * 2^-53, the bound on adding TP values in [0, 1] in any order, plus exp()'s last-bit
differences).  The scenes are drawn so that no OKS lies within 1e-9 of a threshold, which is asserted on the gauge's
matrices, except where an OKS of exactly 1.0 meets the threshold 1.0 on purpose.

Shapes, the smallest at which each mechanism can go wrong: frames without ground truths, without predictions and
without either; G > D and D > G; 1, 63, 64, 65 and 256 people in a frame (the lane boundary, a second column per lane,
the limit); 1, 4 and 5 sequences (the workgroup boundary); 1 and 3 thresholds; K = 1 and 17; a sequence of one frame;
1, 65, 256, 257 and 1024 identities in the identity stage (257: the first use of the 16-column form)."""
import math

import numpy as np
import pytest

from tests import trackeval_reference as R
from tests.cocoeval_reference import default_sigmas

pytestmark = pytest.mark.gpu


def _device(seqs, sig, thresholds, on_device=False):
    import torch
    from probpose_pytorch_amd import PoseTrackEval
    ev = PoseTrackEval(sig, thresholds=thresholds)
    for name, frames in seqs.items():
        for f in frames:
            pk = torch.from_numpy(f["pred_kpts"]).cuda() if on_device else f["pred_kpts"]
            ev.add_frame(name, f["gt_ids"], f["gt_kpts"], f["gt_bbox"], f["gt_area"], f["pred_ids"], pk)
    return ev, ev.evaluate()


def _same(got, ref):
    assert got["thresholds"] == ref["thresholds"]
    assert list(got["per_sequence"]) == list(ref["per_sequence"])
    for name in ref["per_sequence"]:
        for t, (g, r) in enumerate(zip(got["per_sequence"][name], ref["per_sequence"][name])):
            ints = {k: g[k] for k in R.INT_KEYS}
            print(name, ref["thresholds"][t], ints, g["oks_sum"], r["oks_sum"])
            assert ints == {k: r[k] for k in R.INT_KEYS}, (name, t)
            assert all(type(v) is int for v in ints.values())
            assert abs(g["oks_sum"] - r["oks_sum"]) <= 1e-12 * abs(r["oks_sum"]), (name, t)
    for g, r in zip(got["metrics"], ref["metrics"]):
        assert {k: g[k] for k in R.INT_KEYS} == {k: r[k] for k in R.INT_KEYS}
        for k in R.RATIO_KEYS:
            assert (math.isnan(g[k]) and math.isnan(r[k])) or abs(g[k] - r[k]) <= 1e-12 * abs(r[k]), k


def _first_ground_truths(f, n, K):
    return R.make_frame(f["gt_ids"][:n], f["gt_kpts"][:n], f["gt_bbox"][:n], f["gt_area"][:n], f["pred_ids"],
                        f["pred_kpts"], K=K)


def _check(seqs, sig, thresholds, gap=True, best_total=None, **kw):
    ref = R.evaluate(seqs, sig, thresholds, best_total=best_total)
    if gap:
        assert R.min_threshold_gap(ref) > 1e-9
    ev, got = _device(seqs, sig, thresholds, **kw)
    _same(got, ref)
    return ev, got, ref


@pytest.mark.parametrize("n_seq,n_thr,K", [(1, 1, 17), (4, 3, 1), (5, 1, 3), (5, 3, 17)])
def test_random_sequences_equal_the_gauge(n_seq, n_thr, K):
    rng = np.random.default_rng(100 * n_seq + 10 * n_thr + K)
    seqs = {}
    for s in range(n_seq):                                  # odd ones crowded: the assignment has to choose
        seqs[("cam", s)] = R.random_sequence(rng, K, int(rng.integers(1, 10)), int(rng.integers(1, 9)),
                                             extent=40.0 if s % 2 else 600.0, blind_p=0.1)
    seqs["one frame"] = R.random_sequence(rng, K, 1, 3, always=True)
    thresholds = (0.5,) if n_thr == 1 else (0.3, 0.5, 0.75)
    _, got, ref = _check(seqs, default_sigmas(K), thresholds, on_device=bool(n_seq % 2))
    assert sum(m["TP"] for m in got["metrics"]) > 0


@pytest.mark.parametrize("people", [1, 63, 64, 65, 256])
def test_people_per_frame(people):
    """The lane boundary, a second column per lane and the limit, crowded so that augmenting paths go beyond their first
    step; two or three frames, so that the continuation bonus and the switches are in play at these sizes too.  The
    second sequence has G > D in every frame, the third D > G.  At 256 the crowd is thinner, there are two frames and
    one threshold: the gauge's solver is plain Python."""
    rng = np.random.default_rng(people)
    K, big = 1, people > 65
    crowd = R.random_sequence(rng, K, 2 if big else 3, people, extent=(100.0 if big else 40.0) * math.sqrt(people),
                              always=True, stray_p=0.0, miss_p=0.0, switch_p=0.05)
    fewer = R.random_sequence(rng, K, 2, min(people, 65), extent=100.0, always=True, stray_p=0.0, miss_p=0.3)
    more = [_first_ground_truths(f, max(1, len(f["gt_ids"]) // 2), K)
            for f in R.random_sequence(rng, K, 2, min(people, 65), extent=100.0, always=True, miss_p=0.0, stray_p=1.0)]
    assert all(len(f["gt_ids"]) == people and len(f["pred_ids"]) == people for f in crowd)
    if big:                                                 # the limit on both sides in frame 0; then half the rows
        crowd[1] = _first_ground_truths(crowd[1], people // 2, K)
    assert all(len(f["gt_ids"]) < len(f["pred_ids"]) for f in more)
    assert people < 8 or all(len(f["gt_ids"]) > len(f["pred_ids"]) for f in fewer)
    _, got, ref = _check(dict(crowd=crowd, fewer=fewer, more=more), default_sigmas(K), (0.3,) if big else (0.3, 0.6))
    frames = ref["details"]["crowd"][0]["clear"]["frames"]
    print("steps", [fr["steps"] for fr in frames])
    assert people == 1 or sum(fr["steps"] for fr in frames) > sum(len(fr["q"]) for fr in frames) * (1.02 if big else 1.25)


def test_empty_frames_and_empty_sides():
    K = 3
    walk = R.scene(K, [dict(gt=4, pred=9, at=(0, 0)), dict(gt=None, pred=2, at=(300, 0), frames=(1, 2)),
                       dict(gt=8, pred=None, at=(600, 0), frames=(2, 3))], 4)
    none = R.make_frame(K=K)
    seqs = {"gaps": [none, walk[0], none, none, walk[1], walk[2], none, walk[3]],       # both sides empty, repeatedly
            "no gt": R.scene(K, [dict(gt=None, pred=1, at=(0, 0))], 3),
            "no pred": R.scene(K, [dict(gt=1, pred=None, at=(0, 0))], 3),
            "nothing": [none, none]}
    _, got, _ = _check(seqs, np.full(K, 0.05), (0.5,))
    # person 4 is matched in frames 1, 4, 5 and 7 of 8: three runs
    assert got["per_sequence"]["gaps"][0]["Frag"] == 2 and got["per_sequence"]["gaps"][0]["TP"] == 4


def test_the_hand_made_scenes():
    K = 3
    sig = np.full(K, 0.05)
    _, got, _ = _check({"kept": R.continued_pair_frames(K), "gap": R.scene(K, R.ONE_FRAME_GAP, 5)}, sig, (0.5,))
    kept, gap = got["per_sequence"]["kept"][0], got["per_sequence"]["gap"][0]
    assert (kept["TP"], kept["IDSW"]) == (4, 0)             # the rule keeps the pair; without the bonus IDSW would be 2
    assert (gap["TP"], gap["FN"], gap["IDSW"], gap["Frag"], gap["PT"]) == (4, 1, 1, 1, 1)
    # a prediction equal to the ground truth has OKS 1.0 exactly: admissible at the threshold 1.0
    _, got, _ = _check({"exact": R.scene(K, [dict(gt=1, pred=1, at=(0, 0))], 3)}, sig, (0.5, 1.0), gap=False)
    assert [m["TP"] for m in got["metrics"]] == [3, 3]


def test_ground_truths_without_a_visible_keypoint():
    rng = np.random.default_rng(5)
    K = 17
    seqs = {"blind": R.random_sequence(rng, K, 6, 4, blind_p=0.5, always=True)}
    blind = sum(int((~(f["gt_kpts"][:, :, 2] > 0).any(axis=1)).sum()) for f in seqs["blind"])
    assert blind >= 4
    _check(seqs, default_sigmas(K), (0.2, 0.5))


def _scipy_total(c):
    from scipy.optimize import linear_sum_assignment
    c = np.asarray(c, dtype=np.float64)
    rows, cols = linear_sum_assignment(c, maximize=True)
    return int(c[rows, cols].sum())


@pytest.mark.parametrize("sizes", [(1, 65), (256, 257, 1024)])
def test_the_identity_stage_sizes(sizes):
    """1, 65, 256, 257 and 1024 identities on either side, from many short tracks that contend for one another: the
    4-column form up to 256, the 16-column form from 257.  The gauge's own solver gives IDTP up to 65; from 256 on its
    plain loops take from seconds to minutes, and scipy's gives the same unique total."""
    rng = np.random.default_rng(sum(sizes))
    seqs = {n: R.many_identities(rng, n) for n in sizes}
    _, got, ref = _check(seqs, np.full(1, 0.05), (0.5,), best_total=_scipy_total if max(sizes) > 65 else None)
    for n in seqs:
        c = ref["details"][n][0]["identity"]["c"]
        assert (len(c), len(c[0])) == (n, n)
        assert n == 1 or 0 < got["per_sequence"][n][0]["IDTP"] < got["per_sequence"][n][0]["TP"]


def test_twice_the_same_and_reset():
    rng = np.random.default_rng(3)
    seqs = {s: R.random_sequence(rng, 3, 6, 5, extent=60.0) for s in range(3)}
    ev, first, _ = _check(seqs, np.full(3, 0.05), (0.4, 0.6))
    second = ev.evaluate()
    assert second["per_sequence"] == first["per_sequence"]
    assert [{k: m[k] for k in R.INT_KEYS + ("oks_sum",)} for m in second["metrics"]] == \
           [{k: m[k] for k in R.INT_KEYS + ("oks_sum",)} for m in first["metrics"]]
    ev.reset()
    empty = ev.evaluate()
    assert empty["per_sequence"] == {} and all(m[k] == 0 for m in empty["metrics"] for k in R.INT_KEYS)
    assert all(math.isnan(m[k]) for m in empty["metrics"] for k in R.RATIO_KEYS)


def test_four_launches_and_nothing_waits_before_the_readback(monkeypatch):
    import torch
    from probpose_pytorch_amd import _lib
    rng = np.random.default_rng(4)
    seqs = {s: R.random_sequence(rng, 3, 5, 4) for s in range(6)}
    ev, first = _device(seqs, np.full(3, 0.05), (0.4, 0.6), on_device=True)     # warm
    names, launch = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a: (names.append(name), launch(name, *a))[1])
    b = ev._tables()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, sizes, keep = ev._enqueue(b)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert names == ["pp_cocoeval_oks", "pp_trackeval_clear", "pp_trackeval_overlap", "pp_trackeval_identity"]
    assert ev._finish(b, out.cpu().numpy(), *sizes)["per_sequence"] == first["per_sequence"]
    del names[:]
    assert ev.evaluate()["per_sequence"] == first["per_sequence"] and len(names) == 4


def test_a_clean_clip_through_the_tracker_scores_one():
    """Two people walk past each other at a distance; PoseTracker's ids and keypoints go back in as predictions against
    the poses it was given."""
    import torch
    from probpose_pytorch_amd import PoseTrackEval, PoseTracker
    K = 17
    sig = default_sigmas(K)
    tracker = PoseTracker(sig)
    ev = PoseTrackEval(sig, thresholds=(0.5, 0.9))
    base = R.person(K, 0.0, 0.0, spread=40.0)
    for f in range(8):
        pts = np.stack([base + (3.0 * f, 0.0), base + (500.0 - 3.0 * f, 200.0)])
        kp, bb, ar = R.gt_of(pts)
        res = tracker.update(torch.from_numpy(pts).cuda(), torch.from_numpy(ar).cuda(),
                             torch.tensor([0.9, 0.8], dtype=torch.float64).cuda())
        ev.add_frame("clip", [11, 22], kp, bb, ar, res.ids.cpu().numpy(), res.keypoints)
    got = ev.evaluate()
    for m in got["metrics"]:
        assert (m["TP"], m["FN"], m["FP"], m["IDSW"], m["MT"], m["Frag"], m["IDTP"]) == (16, 0, 0, 0, 2, 0, 16)
        assert m["MOTA"] == 1.0 and m["IDF1"] == 1.0 and m["MOTP"] == 1.0


def test_the_command_line_scores_what_inference_track_writes(tmp_path, capsys):
    """inference.py --frames --track writes tracks.json; its own poses, annotated with one identity per box position,
    are the ground truth: the command line reports a perfect score at both thresholds."""
    import json
    from probpose_pytorch_amd import inference, trackeval
    from tests.test_track_inference import ARGS, BOXES, write_frames
    names, table = write_frames(tmp_path / "frames")
    out = tmp_path / "out"
    record = inference.main(ARGS + ["--frames", str(tmp_path / "frames"), "--boxes-json", str(table), "--track",
                                    "--output", str(out)])
    gt = []
    for f, r in enumerate(record):
        boxes = BOXES if f % 2 == 0 else BOXES[::-1]
        gt.append(dict(frame=r["frame"], persons=[
            dict(id=100 + (i if f % 2 == 0 else 1 - i), keypoints=[[x, y, 2.0] for x, y in d["keypoints"]],
                 bbox=box[:4], area=box[2] * box[3]) for i, (d, box) in enumerate(zip(r["detections"], boxes))]))
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    capsys.readouterr()
    assert trackeval.main([str(tmp_path / "gt.json"), str(out / "tracks.json"), "--thr", "0.5,0.9", "--sigmas", "0.05",
                           "--seq", "clip"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0] == "clip: 4 frames; 0 detections without a slot scored as one-frame tracks"
    rows = [json.loads(line) for line in lines[1:]]
    assert [r["thr"] for r in rows] == [0.5, 0.9]
    for r in rows:
        assert (r["TP"], r["FN"], r["FP"], r["IDSW"], r["MT"], r["Frag"], r["IDTP"]) == (8, 0, 0, 0, 2, 0, 8)
        assert r["MOTA"] == 1.0 and r["IDF1"] == 1.0 and r["MOTP"] == 1.0
