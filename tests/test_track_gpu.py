"""PoseTracker on the GPU against the plain-loop float64 gauge of tests/track_reference.py, call by call.

Bounds (u = 2^-53, the unit roundoff of float64; every OKS lies in [0, 1]):

OKS.  As in tests/test_posenms_gpu.py: the exponent e is the same bits on both sides; exp (1 ulp each side), the sum of
n <= K terms and the division differ: |OKS_kernel - OKS_gauge| <= (2 K + 2) u.

ids, born, (id, age) of every slot, overflow.  Exact equality.  The association compares OKS values with match_thr and
with each other.  The fixture conditions, asserted on the gauge's values before anything touches the device: (1) no
pair OKS the gauge evaluates lies within 1e-9 of match_thr; (2) for every detection whose best OKS exceeds match_thr,
the best exceeds the second best by more than 1e-9: 1e-9 is 10^5 times the OKS bound, so both sides decide alike, and by
induction over the detections and the calls both sides hold the same state; (3) scores are pairwise distinct within a
stream and call except one deliberate tie, which the stable rule decides; (4) over each scene at least 20 % of the
detections are matched and there is at least one birth, expiry and re-identification after a gap; overflow happens in
its scene and in no other; with vis_thr at least one keypoint filter is re-initialised.

keypoints, xhat, dxhat, init.  Bit equality: every operation of the filter is an IEEE basic operation (+, -, *, /, abs)
on the same operands in the same order on both sides (the kernels are compiled -ffp-contract=off).
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import posenms_reference as PR
from tests import track_reference as TR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MATCH_THR, MAX_AGE, SMOOTH, N_FRAMES = 0.3, 2, (1.0, 0.05, 1.0), 12
# K 1 and 17; vis_thr None and 0.2; 16, 65 and 130 slots: a lane owns one, two and three slots, the scenes of 65 and
# 130 people fill every slot, so the 64-slot edge is crossed; 20 people on 8 slots overflow; near-duplicate pairs
CASES = {
    "one_slot_per_lane": dict(K=17, T=16, P=12, vis_thr=None, leavers=2, entrants=2),
    "two_slots_per_lane": dict(K=17, T=65, P=65, vis_thr=0.2, leavers=3, entrants=3),
    "three_slots_per_lane": dict(K=1, T=130, P=130, vis_thr=None, leavers=4, entrants=4),
    "overflow": dict(K=17, T=8, P=20, vis_thr=None),
    "near_duplicates": dict(K=17, T=16, P=12, vis_thr=0.2, duplicates=True),
}
STREAMS = ["empty", "main", "solo"]                     # 0, many and 1 detections; "solo" is absent from some calls


def _freeze(frames):
    for f in frames:
        for a in f.values():
            if a is not None:
                a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def scene(name):
    """The calls of a case: a list of (t, {stream: frame}).  "main" is the case's scene, "solo" one drifting person,
    named in two calls of three, "empty" a stream that never has a detection.  Read-only."""
    c = dict(CASES[name])
    K, P = c.pop("K"), c.pop("P")
    c.pop("T"), c.pop("vis_thr")
    main, times, _ = TR.make_scene(5, K, N_FRAMES, P, MAX_AGE, **c)
    solo, _, _ = TR.make_scene(6, K, N_FRAMES, 1, MAX_AGE)
    empty = TR.make_frame(np.zeros((0, K, 2)), [], [], np.zeros((0, K)))
    _freeze(main + solo + [empty])
    calls = []
    for f, t in enumerate(times):
        frames = {"empty": empty, "main": main[f]}
        if f % 3 != 1:
            frames["solo"] = solo[f]
        calls.append((float(t), frames))
    return tuple(calls)


def _snapshot(tr):
    return {s: {k: np.array(getattr(st, k)) for k in ("id", "age", "t_last", "area", "kp", "xhat", "dxhat", "init")}
            | dict(overflow=st.overflow, next_id=st.next_id) for s, st in tr.streams.items()}


@functools.lru_cache(maxsize=None)
def gauge(name, smooth=True):
    """Per call: ({stream: result}, the state of every stream after the call)."""
    c = CASES[name]
    tr = TR.Tracker(PR.default_sigmas(c["K"]), MATCH_THR, MAX_AGE, c["T"], c["vis_thr"], SMOOTH if smooth else None)
    return tuple((tr.update(frames, t), _snapshot(tr)) for t, frames in scene(name))


def check_fixture(name):
    """Conditions (1) - (4) of the module docstring on the gauge's values."""
    c, events, n_det, ties = CASES[name], {}, 0, 0
    for (t, frames), (results, _) in zip(scene(name), gauge(name)):
        for s, r in results.items():
            seen = np.asarray(r["oks_seen"], dtype=np.float64)
            assert seen.size == 0 or np.abs(seen - MATCH_THR).min() > 1e-9, "a pair OKS sits on the threshold"
            for best, second, _, _ in r["gaps"]:
                assert not best > MATCH_THR or second is None or best - second > 1e-9, ("two slots tie", best, second)
            sc = np.sort(frames[s]["score"])
            ties += int((np.diff(sc) == 0).sum())
            if s == "main":
                n_det += r["ids"].size
                for k, v in r["events"].items():
                    events[k] = events.get(k, 0) + v
    assert ties == 1, ties
    assert events["match"] >= 0.2 * n_det and events["birth"] and events["expiry"] and events["reid"], events
    assert (events["overflow"] > 0) == (name == "overflow"), events
    assert (events["reinit"] > 0) == (c["vis_thr"] is not None), events
    last = gauge(name)[-1][1]["main"]
    if c["T"] > 64:
        assert any(snap["main"]["id"][64:].max() >= 0 for _, snap in gauge(name)), "the 64-slot edge is not crossed"
    assert last["overflow"] == events["overflow"]
    return events


def flat(frames, order=STREAMS):
    """The frames of one call as one batch in the streams' order: stream ids, keypoints [M, K, 3] (the third column the
    visibility), areas, scores."""
    names = [s for s in order if s in frames]
    ids = [s for s in names for _ in range(frames[s]["kpts"].shape[0])]
    kp = np.concatenate([np.concatenate([frames[s]["kpts"], frames[s]["vis"][..., None]], axis=2) for s in names])
    return ids, kp, np.concatenate([frames[s]["area"] for s in names]), np.concatenate([frames[s]["score"]
                                                                                          for s in names])


def make_tracker(name, smooth=True, **kw):
    from probpose_pytorch_amd import OneEuro, PoseTracker
    c = CASES[name]
    return PoseTracker(PR.default_sigmas(c["K"]), match_thr=MATCH_THR, max_age=MAX_AGE, max_tracks=c["T"],
                       vis_thr=c["vis_thr"], smooth=OneEuro(*SMOOTH) if smooth else None, **kw)


def run_device(name, smooth=True, tracker=None, dtype=torch.float64):
    """Every call of the case on the device: per call (the result's tensors as host arrays, tracks() of every stream
    seen, overflow)."""
    tr = tracker or make_tracker(name, smooth)
    out = []
    for t, frames in scene(name):
        ids, kp, ar, sc = flat(frames)
        res = tr.update(torch.from_numpy(kp).to("cuda", dtype), torch.from_numpy(ar).to("cuda", dtype),
                        torch.from_numpy(sc).to("cuda", dtype), stream_ids=ids, t=t, streams=[s for s in STREAMS
                                                                                              if s in frames])
        assert res.stream_ids == [s for s in STREAMS if s in frames]
        host = {k: getattr(res, k).cpu().numpy() for k in ("ids", "keypoints", "oks", "born")}
        seen = list(tr._index)
        out.append((host, {s: tr.tracks(s) for s in seen}, dict(zip(seen, tr.overflow.cpu().numpy().tolist()))))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_scenes_are_the_gauges_call_by_call(name):
    events = check_fixture(name)
    K, worst = CASES[name]["K"], 0.0
    bound = (2 * K + 2) * U
    for n, ((t, frames), (want, snap), (got, tracks, overflow)) in enumerate(zip(scene(name), gauge(name),
                                                                                 run_device(name))):
        names = [s for s in STREAMS if s in frames]
        cat = lambda key: np.concatenate([want[s][key] for s in names])
        assert got["ids"].dtype == np.int64 and got["born"].dtype == np.bool_ and got["oks"].dtype == np.float64
        assert got["keypoints"].dtype == np.float64 and got["keypoints"].shape == cat("keypoints").shape
        assert np.array_equal(got["ids"], cat("ids")), (n, np.nonzero(got["ids"] != cat("ids"))[0])
        assert np.array_equal(got["born"], cat("born")), n
        worst = max(worst, float(np.abs(got["oks"] - cat("oks")).max(initial=0.0)))
        assert np.abs(got["oks"] - cat("oks")).max(initial=0.0) <= bound, n
        assert got["keypoints"].tobytes() == cat("keypoints").tobytes(), (
            n, np.abs(got["keypoints"] - cat("keypoints")).max())
        assert set(tracks) == set(snap)
        for s, w in snap.items():
            g = tracks[s]
            assert np.array_equal(g["id"], w["id"]) and np.array_equal(g["age"], w["age"]), (n, s)
            assert g["age"].dtype == np.int32 and g["init"].dtype == np.uint8
            for mine, theirs in (("t_last", "t_last"), ("area", "area"), ("keypoints", "kp"), ("xhat", "xhat"),
                                 ("dxhat", "dxhat"), ("init", "init")):
                assert g[mine].tobytes() == w[theirs].tobytes(), (n, s, mine)
            assert overflow[s] == w["overflow"], (n, s)
    print(f"{name}: events {events}; worst |d OKS| = {worst / bound:.4f} of the bound {bound:.3e}")


def test_float32_inputs_are_widened_exactly():
    """float32 device tensors give what the gauge gives on the same values widened to float64."""
    name = "one_slot_per_lane"
    c = CASES[name]
    tr_g = TR.Tracker(PR.default_sigmas(c["K"]), MATCH_THR, MAX_AGE, c["T"], c["vis_thr"], SMOOTH)
    tr_d = make_tracker(name)
    for t, frames in scene(name)[:4]:
        f = frames["main"]
        f32 = {k: v.astype(np.float32) for k, v in f.items()}
        want = tr_g.update({0: TR.make_frame(*(f32[k].astype(np.float64) for k in ("kpts", "score", "area", "vis")))},
                           t)[0]
        res = tr_d.update(torch.from_numpy(f32["kpts"]).cuda(), torch.from_numpy(f32["area"]).cuda(),
                          torch.from_numpy(f32["score"]).cuda(), t=t)
        assert res.stream_ids == [0] and np.array_equal(res.ids.cpu().numpy(), want["ids"])
        assert res.keypoints.cpu().numpy().tobytes() == want["keypoints"].tobytes()


def test_without_a_filter_the_input_bits_come_back():
    name = "near_duplicates"
    for (t, frames), (want, _), (got, _, _) in zip(scene(name), gauge(name, smooth=False),
                                                   run_device(name, smooth=False)):
        _, kp, _, _ = flat(frames)
        assert got["keypoints"].tobytes() == np.ascontiguousarray(kp[..., :2]).tobytes()
        names = [s for s in STREAMS if s in frames]
        assert np.array_equal(got["ids"], np.concatenate([want[s]["ids"] for s in names]))


def test_two_runs_give_the_same_bits():
    name = "two_slots_per_lane"
    a, b = run_device(name), run_device(name)
    for (ga, ta, oa), (gb, tb, ob) in zip(a, b):
        assert all(ga[k].tobytes() == gb[k].tobytes() for k in ga) and oa == ob
        assert all(ta[s][k].tobytes() == tb[s][k].tobytes() for s in ta for k in ta[s])


def test_reset_restarts_one_stream_and_leaves_the_others():
    name = "one_slot_per_lane"
    tr = make_tracker(name)
    calls = scene(name)

    def call(n, t):
        ids, kp, ar, sc = flat(calls[n][1])
        res = tr.update(torch.from_numpy(kp).cuda(), torch.from_numpy(ar).cuda(), torch.from_numpy(sc).cuda(),
                        stream_ids=ids, t=t)
        return np.asarray(ids), res.ids.cpu().numpy(), res.born.cpu().numpy()

    call(0, 1.0)
    before = tr.tracks("solo")
    tr.reset("main")
    assert (tr.tracks("main")["id"] == -1).all() and tr.tracks("solo")["id"].tolist() == before["id"].tolist()
    ids, got, born = call(2, 2.0)                       # both streams are in calls 0 and 2
    main = ids == "main"
    assert sorted(got[main].tolist()) == list(range(int(main.sum()))) and born[main].all()      # ids restart at 0
    assert got[~main].tolist() == [0] and not born[~main].any()                                 # solo goes on
    tr.reset()
    assert all((tr.tracks(s)["id"] == -1).all() for s in ("main", "solo")) and int(tr.overflow.sum()) == 0
    ids, got, born = call(3, 3.0)
    assert born.all() and got[ids == "solo"].tolist() == [0]


def test_update_reads_back_the_finiteness_booleans_and_nothing_else():
    name = "one_slot_per_lane"
    tr = make_tracker(name)
    calls = scene(name)
    inputs = []
    for t, frames in calls[:3]:
        ids, kp, ar, sc = flat(frames)
        inputs.append((ids, t, [torch.from_numpy(a).cuda() for a in (kp, ar, sc)]))
    ids, t, dev = inputs[0]
    tr.update(*dev, stream_ids=ids, t=t)                # allocates the state
    torch.cuda.synchronize()
    sync_mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            for ids, t, dev in inputs[1:]:
                res = tr.update(*dev, stream_ids=ids, t=t)
            overflow = tr.overflow
            syncs = [w for w in seen if "synchroniz" in str(w.message).lower()]
    finally:
        torch.cuda.set_sync_debug_mode(sync_mode)
    print(f"PoseTracker.update x 2: {len(syncs)} synchronising call(s)")
    assert len(syncs) == 2, [str(w.message) for w in syncs]
    want = gauge(name)[2][0]
    assert np.array_equal(res.ids.cpu().numpy(), np.concatenate([want[s]["ids"] for s in STREAMS if s in calls[2][1]]))
    assert overflow.cpu().numpy().tolist() == [0, 0]
    bad = dev[1].clone()
    bad[0] = float("nan")
    with pytest.raises(ValueError, match="areas: non-finite values"):
        tr.update(dev[0], bad, dev[2], stream_ids=ids, t=t + 1)
    with pytest.raises(ValueError, match="either all device tensors or all host arrays"):
        tr.update(dev[0], dev[1].cpu(), dev[2], stream_ids=ids, t=t + 1)
    with pytest.raises(ValueError, match="t: "):
        tr.update(*dev, stream_ids=ids, t=t)


def test_end_to_end_from_decode_through_nms():
    """Three frames of four people, each frame with a duplicate box of person 0: Codec.decode_device -> frame
    coordinates -> PoseNMS -> boolean index -> PoseTracker.  Each person keeps one id across the frames."""
    from probpose_pytorch_amd import Codec, OneEuro, PoseNMS, PoseTracker, ProbMap
    K, H, W = 17, 64, 48
    sig = PR.default_sigmas(K)
    codec = Codec(ProbMap((192, 256), (W, H), sig))
    rng = np.random.default_rng(3)
    peaks = np.stack([rng.uniform(8, W - 8, (4, K)), rng.uniform(8, H - 8, (4, K))], axis=2)
    boxes = np.array([[100.0 + 300.0 * p, 50.0, 192.0, 256.0] for p in range(4)])
    yy, xx = np.mgrid[0:H, 0:W]
    nms = PoseNMS(sig, mode="hard", oks_thr=0.9, kpt_thr=0.0)
    tracker = PoseTracker(sig, smooth=OneEuro(), max_tracks=8)
    seen = []
    for f in range(3):
        order = rng.permutation(5)                      # 4 is the duplicate of person 0
        person = np.where(order == 4, 0, order)
        c = peaks[person] + f * np.array([0.7, -0.5])
        hm = np.exp(-((xx[None, None] - c[..., 0, None, None]) ** 2 + (yy[None, None] - c[..., 1, None, None]) ** 2)
                    / 8.0).astype(np.float32)
        aux = [torch.from_numpy(rng.random((5, K, 1, 1), dtype=np.float32)).cuda() for _ in range(4)]
        out = codec.decode_device((torch.from_numpy(hm).cuda(), *aux))
        box = torch.from_numpy(boxes[person]).cuda()
        kp = out["kpts"] + box[:, None, :2]             # crops at scale 1: input pixels + the box corner
        box_scores = torch.from_numpy(np.where(order == 4, 0.3, 0.9 - 0.1 * order)).cuda()
        res = nms(np.zeros(5, dtype=np.int64), kp, box_scores, box[:, 2] * box[:, 3], kpt_scores=out["scores"])
        keep = res.keep
        assert keep.cpu().numpy().tolist() == (order != 4).tolist()
        tr = tracker.update(kp[keep], (box[:, 2] * box[:, 3])[keep], res.scores[keep], out["scores"][keep])
        ids = tr.ids.cpu().numpy()
        assert tr.born.cpu().numpy().tolist() == [f == 0] * 4 and (tr.oks.cpu().numpy() > 0.5).all() == (f > 0)
        seen.append(dict(zip(person[order != 4].tolist(), ids.tolist())))
    assert seen[0] == seen[1] == seen[2] and sorted(seen[0].values()) == [0, 1, 2, 3]
