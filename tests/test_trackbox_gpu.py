"""PoseTracker.propose_boxes and PoseFollower on the GPU against the plain-loop float64 gauge of
tests/trackbox_reference.py.

The state is built by real ``update`` calls on ``track_reference.make_scene`` scenes, mirrored on the gauge tracker;
tests/test_track_gpu.py shows those states to be the same bits (the scenes here keep its fixture conditions: people a
420-pixel grid apart, so a pair OKS is either far above or far below match_thr).

Bound: equality, byte for byte.  Every step of the rule is one IEEE basic operation (+, -, *, /, comparisons) on the
same operands in the same order on both sides (the kernels are compiled -ffp-contract=off).

Shapes (K, max_tracks, streams): (1, 1, 1); (17, 8, 3); (133, 70, 17), which crosses the 16-stream chunk of the state
and, with 66 people in its first stream, the 64-slot edge.
"""
import functools

import numpy as np
import pytest
import torch

from tests import posenms_reference as PR
from tests import track_reference as TR
from tests import trackbox_reference as BR

pytestmark = pytest.mark.gpu

MATCH_THR, MAX_AGE, SMOOTH, VIS_THR, N_FRAMES = 0.3, 2, (1.0, 0.05, 1.0), 0.3, 4
# people per stream; min_keypoints at the mean count of keypoints above VIS_THR, so that FEW and PROPOSED both occur
SHAPES = {
    "one": dict(K=1, T=1, people=[1], few=1, seed=43),
    "mid": dict(K=17, T=8, people=[6, 8, 2], few=12),
    "big": dict(K=133, T=70, people=[66] + [2] * 16, few=93),
}


@functools.lru_cache(maxsize=None)
def calls(name):
    """The update calls of a shape: a tuple of (t, {stream: frame}).  After frame 0 the big first stream keeps only the
    people of its slots 0, 1 and 58 .. 65 (the gauge's OKS loops stay short); the others follow make_scene, whose third
    people are absent for a while.  Read-only."""
    c = SHAPES[name]
    scenes = [TR.make_scene(c.get("seed", 40) + s, c["K"], N_FRAMES, P, MAX_AGE) for s, P in enumerate(c["people"])]
    times = scenes[0][1]
    out = []
    for f in range(N_FRAMES):
        frames = {}
        for s, (fr, _, who) in enumerate(scenes):
            keep = np.ones(who[f].size, dtype=bool)
            if f > 0 and c["people"][s] > 8:                # frame 0 fills the slots in descending score order
                by_slot = who[0][np.argsort(-fr[0]["score"], kind="stable")]
                keep = np.isin(who[f], np.concatenate([by_slot[:2], by_slot[58:]]))
            frames[s] = {k: (None if v is None else np.ascontiguousarray(v[keep])) for k, v in fr[f].items()}
            for a in frames[s].values():
                a.setflags(write=False)
        out.append((float(times[f]), frames))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gauge_tracker(name, smooth):
    c = SHAPES[name]
    tr = TR.Tracker(PR.default_sigmas(c["K"]), MATCH_THR, MAX_AGE, c["T"], VIS_THR, SMOOTH if smooth else None)
    for t, frames in calls(name):
        tr.update(frames, t)
    return tr


def device_tracker(name, smooth):
    from probpose_pytorch_amd import OneEuro, PoseTracker
    c = SHAPES[name]
    tr = PoseTracker(PR.default_sigmas(c["K"]), match_thr=MATCH_THR, max_age=MAX_AGE, max_tracks=c["T"],
                     vis_thr=VIS_THR, smooth=OneEuro(*SMOOTH) if smooth else None)
    for t, frames in calls(name):
        streams = list(frames)
        ids = [s for s in streams for _ in range(frames[s]["kpts"].shape[0])]
        cat = lambda key: torch.from_numpy(np.concatenate([frames[s][key] for s in streams])).cuda()
        tr.update(cat("kpts"), cat("area"), cat("score"), cat("vis"), stream_ids=ids, streams=streams, t=t)
    return tr


def frame_sizes(name):
    """Per-stream frames that cut the people's 420-pixel grid; every third stream is not named: no clamp."""
    return {s: (700.0 + 37.0 * s, 500.0 + 29.0 * s) for s in range(len(SHAPES[name]["people"])) if s % 3 != 2}


@functools.lru_cache(maxsize=None)
def variant(name, smooth, extrapolate, rich):
    """(options of propose_boxes, the gauge's per-stream results).  ``rich``: max_age 2, the FEW threshold, an aspect,
    max_dt, per-stream frames and suppression boxes made from the gauge's own unsuppressed proposals."""
    c, tr = SHAPES[name], gauge_tracker(name, smooth)
    t = calls(name)[-1][0] + 0.04
    streams = list(range(len(c["people"])))
    if not rich:
        opts = dict(extrapolate=extrapolate, min_keypoints=1)
        frames, given = {}, {}
    else:
        opts = dict(extrapolate=extrapolate, min_keypoints=c["few"], max_age=2, aspect=0.75, max_dt=0.02, iou_thr=0.4,
                    pad=1.3, min_side=3.0)
        frames, given = frame_sizes(name), {}
        for s in streams[::2]:                              # the odd streams get no given box
            boxes, _, _, status = ref_propose(tr, s, t, opts, frames.get(s), ())
            mine = boxes[status == BR.PROPOSED][::2].copy()
            mine[:, 0] += 0.1 * mine[:, 2]                  # IoU 0.9 / 1.1 with its proposal
            given[s] = np.concatenate([mine, [[-500.0, -500.0, 10.0, 10.0], [5.0, 5.0, 0.0, 40.0]]])
    want = [ref_propose(tr, s, t, opts, frames.get(s), given.get(s, ())) for s in streams]
    return t, opts, frames, given, want


def ref_propose(tr, s, t, opts, frame_wh, given):
    o = dict(opts)
    o["aspect"] = o.get("aspect") or 0.0
    o["max_dt"] = np.inf if o.get("max_dt") is None else o["max_dt"]
    return BR.propose(tr.streams[s], t, vis_thr=tr.vis_thr, smooth=tr.smooth is not None, frame_wh=frame_wh,
                      sup_boxes=given, **o)


def run_device(tr, name, t, opts, frames, given):
    suppress = None
    if given:
        rows = [(s, b) for s, bs in given.items() for b in bs]
        order = np.random.default_rng(1).permutation(len(rows))            # streams interleaved
        suppress = (np.array([rows[i][1] for i in order]), [rows[i][0] for i in order])
    return tr.propose_boxes(t, frame_size=frames or None, suppress=suppress, **opts)


@pytest.mark.parametrize("name", list(SHAPES))
def test_proposals_are_the_gauges_byte_for_byte(name):
    seen = set()
    cases = [(sm, ex, rich) for sm in (False, True) for ex in (False, True) for rich in (False, True)]
    for sm, ex, rich in cases:                              # the fixture, on the gauge's side first
        seen |= {int(v) for _, _, _, status in variant(name, sm, ex, rich)[4] for v in status}
    assert seen == set(range(6)) if name != "one" else BR.PROPOSED in seen, seen
    last = gauge_tracker(name, True).streams[0]
    assert name != "big" or (last.id[64:] >= 0).any(), "the 64-slot edge is not crossed"
    trackers = {sm: device_tracker(name, sm) for sm in (False, True)}
    for sm, ex, rich in cases:
        t, opts, frames, given, want = variant(name, sm, ex, rich)
        tr = trackers[sm]
        state = [c.clone() for c in tr._chunks]
        calls_before = (tr._calls, tr._t_prev)
        got = run_device(tr, name, t, opts, frames, given)
        again = run_device(tr, name, t, opts, frames, given)
        assert all(torch.equal(a, b) for a, b in zip(state, tr._chunks)), "propose_boxes wrote state"
        assert (tr._calls, tr._t_prev) == calls_before and got.stream_ids == list(range(len(want)))
        S, T = len(want), SHAPES[name]["T"]
        assert got.boxes.shape == (S, T, 4) and got.boxes.dtype == torch.float64 and got.status.dtype == torch.uint8
        assert got.ids.shape == got.scores.shape == got.status.shape == (S, T) and got.ids.dtype == torch.int64
        host = {k: getattr(got, k).cpu().numpy() for k in ("boxes", "ids", "scores", "status")}
        for k, i in (("boxes", 0), ("ids", 1), ("scores", 2), ("status", 3)):
            ref = np.stack([w[i] for w in want])
            assert host[k].tobytes() == ref.tobytes(), (sm, ex, rich, k, np.argwhere(host[k] != ref)[:4])
            assert getattr(again, k).cpu().numpy().tobytes() == host[k].tobytes(), (k, "two calls differ")
        boxes, ids, scores, index = got.compact()
        ref = [BR.compact(*w) for w in want]
        assert boxes.tobytes() == np.concatenate([r[0] for r in ref]).tobytes()
        assert ids.tolist() == np.concatenate([r[1] for r in ref]).tolist()
        assert scores.tobytes() == np.concatenate([r[2] for r in ref]).tobytes()
        assert index.tolist() == [s for s, r in enumerate(ref) for _ in range(r[1].size)]
    print(f"{name}: status codes seen {sorted(seen)}")


def test_streams_are_chosen_and_nothing_synchronises():
    name = "mid"
    tr = device_tracker(name, True)
    t, opts, frames, given, want = variant(name, True, True, True)
    run_device(tr, name, t, opts, frames, given)            # warm
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run_device(tr, name, t, opts, frames, given)
        pick = tr.propose_boxes(t, streams=[2, 0], frame_size=frames[0], **opts)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert got.status.cpu().numpy().tobytes() == np.stack([w[3] for w in want]).tobytes()
    assert pick.stream_ids == [2, 0]
    for row, s in enumerate(pick.stream_ids):
        ref = ref_propose(gauge_tracker(name, True), s, t, opts, frames[0], ())
        assert pick.boxes[row].cpu().numpy().tobytes() == ref[0].tobytes()
    # suppression boxes that are already on the device, for the only stream named
    one = tr.propose_boxes(t, streams=[0], frame_size=frames[0], suppress=(torch.from_numpy(given[0]).cuda(), None), **opts)
    assert one.status.cpu().numpy().tobytes() == want[0][3].tobytes()
    with pytest.raises(ValueError, match="t: "):
        tr.propose_boxes(calls(name)[-1][0])
    from probpose_pytorch_amd import PoseTracker
    assert PoseTracker(np.full(3, 0.05)).propose_boxes().compact()[0].shape == (0, 4)       # no stream: no launch


# ------------------------------------------------------------------------------------------------ the closed loop
def device_estimate(scene):
    """Scene.estimate in torch operations on the device (comparisons, one product and sum per centre: the same bits)."""
    def estimate(f, boxes):
        kp_all, mean = (torch.from_numpy(a).cuda() for a in scene.people(f))
        b = torch.from_numpy(np.asarray(boxes, dtype=np.float64).reshape(-1, 4)).cuda()
        x, y, w, h = (b[:, i, None] for i in range(4))
        ex, ey, cx, cy = x + w, y + h, x + w * 0.5, y + h * 0.5
        mx, my = mean[None, :, 0], mean[None, :, 1]
        holds = (x <= mx) & (mx <= ex) & (y <= my) & (my <= ey)
        d = torch.where(holds, (mx - cx).abs() + (my - cy).abs(), torch.inf)
        c = kp_all[d.argmin(dim=1)]
        inside = (c[..., 0] >= x) & (c[..., 0] <= ex) & (c[..., 1] >= y) & (c[..., 1] <= ey) & holds.any(dim=1, keepdim=True)
        centre = torch.stack([cx, cy], dim=2).expand(-1, scene.K, -1)
        scores = torch.full(inside.shape, 0.05, dtype=torch.float64, device="cuda").masked_fill(inside, 0.9)
        return torch.where(inside[..., None], c, centre), scores
    return estimate


LOOPS = [dict(v=2, smooth=sm, extrapolate=ex) for sm in (False, True) for ex in (False, True)] + [
    dict(v=3, smooth=True, extrapolate=True), dict(v=3, smooth=True, extrapolate=False),
    dict(v=3, smooth=True, extrapolate=True, aspect=0.75), dict(v=3, smooth=True, extrapolate=True, gone=(2, 15))]


@pytest.mark.parametrize("case", LOOPS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_the_follower_is_the_gauges_loop(case):
    from probpose_pytorch_amd import OneEuro, PoseFollower, PoseTracker
    case = dict(case)
    v, smooth, gone = case.pop("v"), case.pop("smooth"), case.pop("gone", None)
    scene = BR.Scene(v, gone)
    want = scene.run(BR.Follower(scene.tracker(SMOOTH if smooth else None), scene.estimate, **case))
    tracker = PoseTracker(np.full(scene.K, 0.05), match_thr=0.3, max_age=5, max_tracks=8, vis_thr=0.3,
                          smooth=OneEuro(*SMOOTH) if smooth else None, fps=scene.FPS)
    follower = PoseFollower(tracker, device_estimate(scene), **case)
    for f, w in enumerate(want):
        got = follower.step(f, scene.first_boxes if f == 0 else None, frame_size=scene.SIZE)
        assert got.boxes.tobytes() == w["boxes"].tobytes(), (f, got.boxes, w["boxes"])
        assert got.source.tolist() == w["source"].tolist()
        assert got.tracks.ids.cpu().numpy().tolist() == w["result"]["ids"].tolist(), f
        assert got.tracks.keypoints.cpu().numpy().tobytes() == w["result"]["keypoints"].tobytes(), f
        assert got.kpt_scores.cpu().numpy().tobytes() == w["kpt_scores"].tobytes(), f
    if gone is not None:
        slots = tracker.tracks(0)
        assert slots["id"].tolist() == [0, 1] + [-1] * 6
