"""The optimal track association on the GPU against the integer gauge of tests/trackopt_reference.py.

(a) pp_track_assign_optimal on its own, on hand-made state blocks and a hand-made float64 OKS workspace.  Both sides
read the same bits and every later step is integer arithmetic, so everything is compared by exact equality, ties
included: slot_of, ids, born, total, match_oks, te and the id / age / t_last / area fields and counters of the state.

(b) PoseTracker(assign="optimal") against trackopt_reference.Tracker call by call.  The device's pair OKS differs from
the gauge's by at most (2 K + 2) u (tests/test_track_gpu.py), u = 2^-53; times 2^40 that is below 0.005, so each weight
q differs by at most 1 and the total of any matching by at most min(D, T).  The fixture conditions, asserted on the
gauge's values before the device is touched: no evaluated OKS within 1e-9 of match_thr (both sides agree on which pairs
are admissible) and margin(q) > 2 min(D, T) for every stream and call (a matching that lacks a pair of the gauge's
optimum stays below it on the device too): both sides hold the same matching, and by induction the same state.  ids,
born and slot ids / ages are then equal, keypoints and filter state bit-equal (IEEE basic operations on the same
operands), oks within (2 K + 2) u.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import posenms_reference as PR
from tests import track_reference as TR
from tests import trackopt_reference as OR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MATCH_THR, MAX_AGE, SMOOTH, N_FRAMES = 0.3, 2, (1.0, 0.05, 1.0), 10

# ------------------------------------------------------------------------------------------------ (a) the entry alone
N_STREAMS, EMPTY = 6, 2                                 # two workgroups of four waves; stream 2 has no detection


def _matrix(kind, rng, D, T):
    if kind == "dense":
        return rng.uniform(0.0, 1.0, (D, T))
    if kind == "quarter":
        return rng.integers(0, 5, (D, T)) / 4.0
    if kind == "tracker":                               # one strong pair per row, the rest below the threshold
        oks = rng.uniform(0.0, 0.25, (D, T))
        cols = rng.permutation(T)[:D]
        oks[np.arange(cols.size), cols] = rng.uniform(0.5, 1.0, cols.size)
        return oks
    if kind == "example":
        return np.array(OR.EXAMPLE)
    if kind == "none":
        return rng.uniform(0.0, 0.3, (D, T))
    raise KeyError(kind)


ENTRY_CASES = {
    "no_detection": ("dense", 0, 5), "one_by_one": ("dense", 1, 1), "wide": ("dense", 3, 5), "tall": ("dense", 5, 3),
    "one_column_per_lane": ("dense", 64, 64), "two_columns_virtual": ("dense", 70, 65),
    "three_columns": ("dense", 65, 130), "tracker_like_at_the_limit": ("tracker", 256, 256),
    "quarter_steps_full_of_ties": ("quarter", 40, 40), "the_example": ("example", 2, 2),
    "nothing_admissible": ("none", 4, 6),
}


def entry_problem(name):
    """Six streams of one launch: per stream the OKS rows [D_s, T], areas, and the hand-made state fields."""
    kind, D, T = ENTRY_CASES[name]
    rng = np.random.default_rng(sorted(ENTRY_CASES).index(name))
    streams = []
    for s in range(N_STREAMS):
        Ds = 0 if s == EMPTY else (max(D - 1, 0) if s == 4 else D)
        oks = _matrix(kind, rng, D, T)[:Ds]
        all_live = kind in ("tracker", "example") or s == 1
        live = np.ones(T, dtype=bool) if all_live else rng.uniform(size=T) < 0.8
        if kind != "none":
            oks[:, ~live] = 0.99                        # a slot that is not live attracts nobody
        if kind == "dense" and Ds and s == 3:
            oks[0, 0] = np.nan
        streams.append(dict(oks=oks, live=live, area=rng.uniform(100.0, 200.0, Ds),
                            id=np.where(live, 100 + np.arange(T), -1).astype(np.int64),
                            age=rng.integers(0, MAX_AGE + 1, T).astype(np.int32), t_last=rng.uniform(0.1, 0.5, T),
                            slot_area=rng.uniform(100.0, 200.0, T), next_id=1000 + s, overflow=s))
    return T, streams


def entry_expected(T, st, t):
    """The rule after ``solve``: what the entry writes for one stream."""
    oks, D = st["oks"], st["oks"].shape[0]
    q = OR.quantise(oks, st["live"], MATCH_THR) if D else []
    slots, steps = OR.solve(q) if D else ([], 0)
    ids, born, slot_of = np.full(D, -1, dtype=np.int64), np.zeros(D, dtype=np.uint8), np.full(D, -1, dtype=np.int32)
    match_oks, te = np.zeros(D), np.zeros(D)
    sid, age, t_last, area = st["id"].copy(), st["age"].copy(), st["t_last"].copy(), st["slot_area"].copy()
    next_id, overflow = st["next_id"], st["overflow"]
    taken = np.zeros(T, dtype=bool)
    for i, j in enumerate(slots):
        if j >= 0:
            ids[i], slot_of[i], match_oks[i], te[i] = sid[j], j, oks[i, j], np.float64(t) - t_last[j]
            taken[j], age[j], t_last[j], area[j] = True, 0, t, st["area"][i]
    for j in range(T):
        if st["live"][j] and not taken[j]:
            age[j] += 1
            if age[j] > MAX_AGE:
                sid[j] = -1
    for i, j in enumerate(slots):
        if j < 0:
            free = np.flatnonzero(sid < 0)
            if free.size:
                k = int(free[0])
                sid[k], age[k], t_last[k], area[k] = next_id, 0, t, st["area"][i]
                ids[i], born[i], slot_of[i] = next_id, 1, k
                next_id += 1
            else:
                overflow += 1
    return dict(ids=ids, born=born, slot_of=slot_of, match_oks=match_oks, te=te, total=OR.total(q, slots), id=sid,
                age=age, t_last=t_last, area=area, next_id=next_id, overflow=overflow, steps=steps)


@pytest.mark.parametrize("name", list(ENTRY_CASES))
def test_the_entry_alone_is_the_gauge_exactly(name):
    from probpose_pytorch_amd import _lib, tracker
    K, t, t_prev = 1, 1.0, 0.5
    T, streams = entry_problem(name)
    want = [entry_expected(T, st, t) for st in streams]
    lay = tracker.state_layout(T, K)
    raw = np.zeros((N_STREAMS, lay["bytes"]), dtype=np.uint8)

    def field(s, key):
        at, dtype, shape = lay[key]
        return raw[s, at:at + int(np.prod(shape)) * dtype.itemsize].view(dtype)

    for s, st in enumerate(streams):
        field(s, "id")[:], field(s, "age")[:], field(s, "t_last")[:] = st["id"], st["age"], st["t_last"]
        field(s, "area")[:], field(s, "next_id")[:], field(s, "overflow")[:] = st["slot_area"], st["next_id"], \
            st["overflow"]
    off = np.zeros(N_STREAMS + 1, dtype=np.int64)
    off[1:] = np.cumsum([st["oks"].shape[0] for st in streams])
    M = int(off[-1])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    state = dev(raw)
    blocks = dev(state.data_ptr() + lay["bytes"] * np.arange(N_STREAMS, dtype=np.int64))
    oks = dev(np.concatenate([st["oks"].reshape(-1) for st in streams] + [np.zeros(1)]))
    area = dev(np.concatenate([st["area"] for st in streams] + [np.zeros(1)]))
    new = lambda dtype, n=M + 1: torch.full((n,), 77, dtype=dtype, device="cuda")
    ids, match_oks, born, slot_of, te = (new(torch.int64), new(torch.float64), new(torch.uint8), new(torch.int32),
                                         new(torch.float64))
    total = new(torch.int64, N_STREAMS)
    _lib.launch("pp_track_assign_optimal", N_STREAMS, K, T, M, off, dev(off), blocks, oks, area, MATCH_THR, MAX_AGE, t,
                t_prev, ids, match_oks, born, slot_of, te, total)
    got = {k: v.cpu().numpy() for k, v in dict(ids=ids, match_oks=match_oks, born=born, slot_of=slot_of, te=te,
                                               total=total).items()}
    raw = state.cpu().numpy()
    steps = 0
    for s, w in enumerate(want):
        lo, hi = off[s], off[s + 1]
        for k in ("slot_of", "ids", "born", "match_oks", "te"):
            assert got[k][lo:hi].tobytes() == w[k].tobytes(), (name, s, k, got[k][lo:hi], w[k])
        assert got["total"][s] == w["total"], (name, s)
        for k in ("id", "age", "t_last", "area"):
            assert field(s, k).tobytes() == w[k].tobytes(), (name, s, k)
        assert field(s, "next_id")[0] == w["next_id"] and field(s, "overflow")[0] == w["overflow"], (name, s)
        steps += w["steps"]
    assert all(int(got[k][M]) == 77 for k in got if k != "total"), "a write past the last detection"
    matched = sum(int((w["slot_of"] >= 0).sum() - w["born"].sum()) for w in want)
    print(f"{name}: {M} detections on {T} slots, {matched} matched, {steps} inner steps in the gauge")
    if name == "the_example":
        assert want[0]["slot_of"].tolist() == [1, 0] and not want[0]["born"].any()
    if name == "nothing_admissible":
        assert matched == 0 and all(w["total"] == 0 for w in want)
    if name in ("tall", "two_columns_virtual"):
        assert any(w["overflow"] > st["overflow"] or w["born"].any() for w, st in zip(want, streams))


# ------------------------------------------------------------------------------------------------ (b) end to end
CASES = {
    "one_slot_per_lane": dict(K=17, T=16, P=12, vis_thr=None, leavers=2, entrants=2),
    "two_slots_per_lane": dict(K=17, T=65, P=65, vis_thr=0.2, leavers=3, entrants=3),
}
STREAMS = ["empty", "main", "cross"]                    # "cross" is the crossing pair, named in the first two calls


@functools.lru_cache(maxsize=None)
def scene(name):
    c = dict(CASES[name])
    K, P = c.pop("K"), c.pop("P")
    c.pop("T"), c.pop("vis_thr")
    main, times, _ = TR.make_scene(5, K, N_FRAMES, P, MAX_AGE, **c)
    cross = OR.crossing_pair(PR.default_sigmas(K))
    empty = TR.make_frame(np.zeros((0, K, 2)), [], [], np.zeros((0, K)))
    for f in [*main, *cross, empty]:
        for a in f.values():
            if a is not None:
                a.setflags(write=False)
    calls = []
    for f, t in enumerate(times):
        frames = {"empty": empty, "main": main[f]}
        if f < 2:
            frames["cross"] = cross[f]
        calls.append((float(t), frames))
    return tuple(calls)


def _snapshot(tr):
    return {s: {k: np.array(getattr(st, k)) for k in ("id", "age", "t_last", "area", "kp", "xhat", "dxhat", "init")}
            | dict(overflow=st.overflow) for s, st in tr.streams.items()}


@functools.lru_cache(maxsize=None)
def gauge(name):
    c = CASES[name]
    tr = OR.Tracker(PR.default_sigmas(c["K"]), MATCH_THR, MAX_AGE, c["T"], c["vis_thr"], SMOOTH)
    return tuple((tr.update(frames, t), _snapshot(tr)) for t, frames in scene(name))


@functools.lru_cache(maxsize=None)
def greedy_ids(name):
    c = CASES[name]
    tr = TR.Tracker(PR.default_sigmas(c["K"]), MATCH_THR, MAX_AGE, c["T"], c["vis_thr"], SMOOTH)
    return tuple({s: r["ids"] for s, r in tr.update(frames, t).items()} for t, frames in scene(name))


@functools.lru_cache(maxsize=None)
def check_fixture(name):
    """The conditions of the module docstring, on the gauge's values."""
    events, differ, least = {}, 0, None
    for (results, _), greedy in zip(gauge(name), greedy_ids(name)):
        for s, r in results.items():
            seen = np.asarray(r["oks_seen"], dtype=np.float64)
            assert seen.size == 0 or np.abs(seen - MATCH_THR).min() > 1e-9, "a pair OKS sits on the threshold"
            D = r["ids"].size
            if D and r["n_live"]:
                mg = OR.margin(r["q"])
                assert mg > 2 * min(D, CASES[name]["T"]), (name, s, mg)
                least = mg if least is None else min(least, mg)
            differ += int(not np.array_equal(r["ids"], greedy[s]))
            for k, v in r["events"].items():
                events[k] = events.get(k, 0) + v
    assert differ >= 1, "the greedy and the optimal gauge never disagree"
    assert events["match"] and events["birth"] and events["expiry"] and events["reid"], events
    return events, differ, least


def flat(frames):
    names = [s for s in STREAMS if s in frames]
    ids = [s for s in names for _ in range(frames[s]["kpts"].shape[0])]
    kp = np.concatenate([np.concatenate([frames[s]["kpts"], frames[s]["vis"][..., None]], axis=2) for s in names])
    return names, ids, kp, np.concatenate([frames[s]["area"] for s in names]), np.concatenate(
        [frames[s]["score"] for s in names])


def make_tracker(name, **kw):
    from probpose_pytorch_amd import OneEuro, PoseTracker
    c = CASES[name]
    return PoseTracker(PR.default_sigmas(c["K"]), match_thr=MATCH_THR, max_age=MAX_AGE, max_tracks=c["T"],
                       vis_thr=c["vis_thr"], smooth=OneEuro(*SMOOTH), **kw)


def run_device(name, **kw):
    tr = make_tracker(name, **kw)
    out = []
    for t, frames in scene(name):
        names, ids, kp, ar, sc = flat(frames)
        res = tr.update(torch.from_numpy(kp).cuda(), torch.from_numpy(ar).cuda(), torch.from_numpy(sc).cuda(),
                        stream_ids=ids, t=t, streams=names)
        host = {k: getattr(res, k).cpu().numpy() for k in ("ids", "keypoints", "oks", "born")}
        seen = list(tr._index)
        out.append((host, {s: tr.tracks(s) for s in seen}, dict(zip(seen, tr.overflow.cpu().numpy().tolist()))))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_the_optimal_tracker_is_the_gauge_call_by_call(name):
    events, differ, least = check_fixture(name)
    K = CASES[name]["K"]
    bound, worst = (2 * K + 2) * U, 0.0
    assert make_tracker(name, assign="optimal").assign == "optimal"
    for n, ((t, frames), (want, snap), (got, tracks, overflow)) in enumerate(
            zip(scene(name), gauge(name), run_device(name, assign="optimal"))):
        names = [s for s in STREAMS if s in frames]
        cat = lambda key: np.concatenate([want[s][key] for s in names])
        assert np.array_equal(got["ids"], cat("ids")), (n, np.nonzero(got["ids"] != cat("ids"))[0])
        assert np.array_equal(got["born"], cat("born")), n
        err = float(np.abs(got["oks"] - cat("oks")).max(initial=0.0))
        worst = max(worst, err)
        assert err <= bound, (n, err)
        assert got["keypoints"].tobytes() == cat("keypoints").tobytes(), n
        assert set(tracks) == set(snap)
        for s, w in snap.items():
            g = tracks[s]
            assert np.array_equal(g["id"], w["id"]) and np.array_equal(g["age"], w["age"]), (n, s)
            for mine, theirs in (("t_last", "t_last"), ("area", "area"), ("keypoints", "kp"), ("xhat", "xhat"),
                                 ("dxhat", "dxhat"), ("init", "init")):
                assert g[mine].tobytes() == w[theirs].tobytes(), (n, s, mine)
            assert overflow[s] == w["overflow"], (n, s)
    print(f"{name}: events {events}; greedy differs in {differ} stream-calls; least margin {least}; worst |d OKS| = "
          f"{worst / bound:.4f} of the bound {bound:.3e}")


# ------------------------------------------------------------------------------------------------ (c) other checks
def test_two_runs_give_the_same_bits():
    name = "two_slots_per_lane"
    a, b = run_device(name, assign="optimal"), run_device(name, assign="optimal")
    for (ga, ta, oa), (gb, tb, ob) in zip(a, b):
        assert all(ga[k].tobytes() == gb[k].tobytes() for k in ga) and oa == ob
        assert all(ta[s][k].tobytes() == tb[s][k].tobytes() for s in ta for k in ta[s])


def test_the_optimal_update_synchronises_no_more_than_the_greedy_one():
    name = "one_slot_per_lane"
    counts = {}
    for mode in ("greedy", "optimal"):
        tr = make_tracker(name, assign=mode)
        inputs = []
        for t, frames in scene(name)[:3]:
            names, ids, kp, ar, sc = flat(frames)
            inputs.append((ids, names, t, [torch.from_numpy(a).cuda() for a in (kp, ar, sc)]))
        ids, names, t, dev = inputs[0]
        tr.update(*dev, stream_ids=ids, t=t, streams=names)         # allocates the state
        torch.cuda.synchronize()
        sync_mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                for ids, names, t, dev in inputs[1:]:
                    res = tr.update(*dev, stream_ids=ids, t=t, streams=names)
                counts[mode] = len([w for w in seen if "synchroniz" in str(w.message).lower()])
        finally:
            torch.cuda.set_sync_debug_mode(sync_mode)
        if mode == "optimal":
            want = gauge(name)[2][0]
            assert np.array_equal(res.ids.cpu().numpy(), np.concatenate([want[s]["ids"] for s in names]))
    print(f"PoseTracker.update x 2: {counts} synchronising call(s)")
    assert counts["optimal"] == counts["greedy"] == 2, counts


def test_the_command_line_runs_the_optimal_launch(tmp_path, monkeypatch):
    """inference --track --assign optimal: the frames of tests/test_track_inference.py keep one id per box position, and
    every update went through pp_track_assign_optimal, none through pp_track_assign."""
    from probpose_pytorch_amd import _lib, inference
    from tests.test_track_inference import ARGS, write_frames
    names, table = write_frames(tmp_path / "frames")
    launched, launch = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a: (launched.append(name), launch(name, *a))[1])
    record = inference.main(ARGS + ["--frames", str(tmp_path / "frames"), "--boxes-json", str(table), "--track",
                                    "--assign", "optimal", "--smooth", "--output", str(tmp_path / "out")])
    assert [[d["id"] for d in r["detections"]] for r in record] == [[0, 1], [1, 0], [0, 1], [1, 0]]
    assert launched.count("pp_track_assign_optimal") == len(names) and "pp_track_assign" not in launched


def test_greedy_named_explicitly_is_the_default_tracker():
    name = "one_slot_per_lane"
    a, b = run_device(name), run_device(name, assign="greedy")
    for (ga, ta, oa), (gb, tb, ob) in zip(a, b):
        assert all(ga[k].tobytes() == gb[k].tobytes() for k in ga) and oa == ob
        assert all(ta[s][k].tobytes() == tb[s][k].tobytes() for s in ta for k in ta[s])
    greedy = greedy_ids(name)
    for n, ((t, frames), (got, _, _)) in enumerate(zip(scene(name), a)):
        assert np.array_equal(got["ids"], np.concatenate([greedy[n][s] for s in STREAMS if s in frames])), n
