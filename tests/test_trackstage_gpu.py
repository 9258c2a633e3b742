"""PoseTracker's motion prediction, two-stage association and gated births on the GPU against the plain-loop gauge of
tests/trackstage_reference.py, call by call, under the conventions of tests/test_track_gpu.py.

Bounds (u = 2^-53; every OKS lies in [0, 1]).
OKS: the predicted pose is one product and one sum per coordinate on the same operands on both sides (the kernels are
compiled -ffp-contract=off), so it is the same bits, and with it the exponent argument; exp (1 ulp each side), the sum
of n <= K terms and the division differ: |OKS_kernel - OKS_gauge| <= (2 K + 2) u, the bound of test_track_gpu.py.
ids, born, dropped, (id, age) of every slot, overflow: exact.  keypoints, xhat, dxhat, init: bit-equal.

The fixture conditions, asserted on the gauge's values before anything touches the device: (1) no pair OKS the gauge
evaluates lies within 1e-9 of match_thr or of low_match_thr; (2) greedy: wherever a row's best OKS exceeds its stage's
threshold it exceeds the second best by more than 1e-9 (1e-9 is 10^5 times the OKS bound: both sides decide alike, and
by induction hold the same state); (3) optimal: margin(q) > 2 min(rows, T) for every stage, the condition of
test_trackopt_gpu.py (where every row and every column of q has at most one admissible pair the matching is forced and
the margin is the least such q, which (1) puts above 2^40 * 1e-9 > 1000); (4) the "main" stream of every scene has at
least one stage-2 match, one dropped detection, one birth refused to a stage-1 row by birth_thr and one slot kept out
of stage 2 by its age while a row of stage 2 would have taken it; (5) in the predicted scenes at least one match that
the same gauge without ``predict`` does not make, and where predict_max_dt is set at least one update in which a live
slot's t - t_last exceeds it; (6) the stream "high" is all stage 1, "low" all stage 2 after its first frame, and in
"three_slots_per_lane" the main stream has 63, 64 and 65 stage-1 rows in three of its calls.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import posenms_reference as PR
from tests import track_reference as TR
from tests import trackopt_reference as OR
from tests import trackstage_reference as SR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MATCH_THR, LOW_MATCH_THR, HIGH_THR, BIRTH_THR, MAX_AGE, SMOOTH = 0.3, 0.2, 0.5, 0.6, 2, (1.0, 0.05, 1.0)
FAST = (10.0, 0.05, 5.0)            # One-Euro constants of the predicted scenes: cutoffs that follow the runner's speed
# K 1 and 17; vis_thr None and 0.2; 16, 65 and 130 slots (a lane owns one, two, three); five streams in the calls that
# name "solo" / "cross": a second workgroup of the four-wave launch; optimal at T = D = 65 and at 256 x 256
CASES = {
    "one_slot_per_lane": dict(K=17, T=16, P=12, vis_thr=None, leavers=2, entrants=2, frames=12, assign="greedy",
                              predict=False, low_max_age=0),
    "two_slots_per_lane": dict(K=17, T=65, P=65, vis_thr=0.2, leavers=3, entrants=3, frames=12, assign="greedy",
                               predict=True, predict_max_dt=0.05, low_max_age=1, all_high_first=True, smooth=FAST),
    "three_slots_per_lane": dict(K=1, T=130, P=130, vis_thr=None, leavers=4, entrants=4, frames=12, assign="greedy",
                                 predict=True, low_max_age=0, n_high={4: 63, 5: 64, 6: 65}, all_high_first=True,
                                 smooth=FAST),
    "optimal_two_columns": dict(K=17, T=65, P=65, vis_thr=0.2, leavers=3, entrants=3, frames=10, assign="optimal",
                                predict=True, low_max_age=0, all_high_first=True, smooth=FAST),
    "optimal_at_the_limit": dict(K=1, T=256, P=256, vis_thr=None, frames=5, assign="optimal", predict=False,
                                 low_max_age=0),
}
STREAMS = ["empty", "main", "solo", "cross", "high", "low"]
OPTIONS = ("assign", "predict", "predict_max_dt", "low_max_age")


def _rescored(frame, score):
    return TR.make_frame(frame["kpts"], score, frame["area"], frame["vis"])


def _runner(K, times, seed=3):
    """One person of side 60 accelerating from rest along x (x = 500 t^2), score 0.9: the filter's speed grows with the
    person's while the steps are small; from the fifth frame on a step is 10 units and more, which the stored pose
    does not follow and, with the cutoffs of FAST, the predicted one does."""
    rng = np.random.default_rng(seed)
    shape = rng.uniform(0, 1, (K, 2)) * 60.0
    frames = []
    for t in times:
        kp = shape + np.array([500.0 * t * t, 0.0]) + rng.uniform(-0.5, 0.5, (K, 2))
        frames.append(TR.make_frame(kp[None], [0.9], [2160.0], rng.uniform(0.3, 1.0, (1, K))))
    return frames


@functools.lru_cache(maxsize=None)
def scene(name):
    """The calls of a case: a tuple of (t, {stream: frame}), read-only.  "main" is the case's make_scene, with the
    scores of the frames in ``n_high`` remapped (order kept) so that exactly that many reach HIGH_THR, and with
    ``all_high_first`` those of the first frame raised to BIRTH_THR and above; "solo" is the runner,
    named in every call but the second; "cross" the crossing pair of trackopt_reference in the first two calls
    (optimal cases); "high" five people whose scores are all >= BIRTH_THR; "low" five people born in the first frame
    and below HIGH_THR ever after; "empty" never has a detection."""
    c = CASES[name]
    K, P, F = c["K"], c["P"], c["frames"]
    main, times, _ = TR.make_scene(5, K, F, P, MAX_AGE, leavers=c.get("leavers", 0), entrants=c.get("entrants", 0))
    if c.get("all_high_first"):                         # everybody is born in the first frame: every slot is used
        main[0] = _rescored(main[0], BIRTH_THR + 0.4 * main[0]["score"])
    for f, n in c.get("n_high", {}).items():
        s = main[f]["score"]
        top = np.argsort(-s, kind="stable")[:n]
        new = s * 0.5
        new[top] = HIGH_THR + s[top] * 0.4
        main[f] = _rescored(main[f], new)
    high = [_rescored(f, BIRTH_THR + 0.4 * f["score"]) for f in TR.make_scene(8, K, F, 5, MAX_AGE)[0]]
    low = [_rescored(f, BIRTH_THR + 0.4 * f["score"] if n == 0 else 0.5 * f["score"])
           for n, f in enumerate(TR.make_scene(9, K, F, 5, MAX_AGE)[0])]
    solo = _runner(K, times)
    cross = OR.crossing_pair(PR.default_sigmas(K))
    empty = TR.make_frame(np.zeros((0, K, 2)), [], [], np.zeros((0, K)))
    for f in [*main, *high, *low, *solo, *cross, empty]:
        for a in f.values():
            if a is not None:
                a.setflags(write=False)
    calls = []
    for f, t in enumerate(times):
        frames = {"empty": empty, "main": main[f], "high": high[f], "low": low[f]}
        if f != 1:
            frames["solo"] = solo[f]
        if c["assign"] == "optimal" and f < 2:
            frames["cross"] = cross[f]
        calls.append((float(t), {s: frames[s] for s in STREAMS if s in frames}))
    return tuple(calls)


def _snapshot(tr):
    return {s: {k: np.array(getattr(st, k)) for k in ("id", "age", "t_last", "area", "kp", "xhat", "dxhat", "init")}
            | dict(overflow=st.overflow) for s, st in tr.streams.items()}


@functools.lru_cache(maxsize=None)
def gauge(name, predict=None):
    """Per call: ({stream: result}, the state of every stream after the call)."""
    c = CASES[name]
    opts = {k: c[k] for k in OPTIONS if k in c}
    if predict is not None:
        opts["predict"] = predict
        opts.pop("predict_max_dt", None)
    tr = SR.Tracker(PR.default_sigmas(c["K"]), MATCH_THR, MAX_AGE, c["T"], c["vis_thr"], c.get("smooth", SMOOTH),
                    high_thr=HIGH_THR, low_match_thr=LOW_MATCH_THR, birth_thr=BIRTH_THR, **opts)
    return tuple((tr.update(frames, t), _snapshot(tr)) for t, frames in scene(name))


def _margin_holds(q, rows, T):
    admissible = np.array(q) > 0
    if admissible.size == 0 or not admissible.any():
        return True
    if admissible.sum(axis=0).max() <= 1 and admissible.sum(axis=1).max() <= 1:       # the matching is forced
        return int(np.array(q)[admissible].min()) > 2 * min(rows, T)
    return OR.margin(q) > 2 * min(rows, T)


@functools.lru_cache(maxsize=None)
def check_fixture(name):
    """Conditions (1) - (6) of the module docstring on the gauge's values."""
    c, events, n_high, late = CASES[name], {}, [], 0
    before = None
    for n, ((t, frames), (results, snap)) in enumerate(zip(scene(name), gauge(name))):
        for s, r in results.items():
            seen = np.asarray(r["oks_seen"], dtype=np.float64)
            for thr in (MATCH_THR, LOW_MATCH_THR):
                assert seen.size == 0 or np.abs(seen - thr).min() > 1e-9, "a pair OKS sits on a threshold"
            for best, second, thr in r["gaps"]:
                assert not best > thr or second is None or best - second > 1e-9, ("two slots tie", best, second)
            for st in r["stages"]:
                assert _margin_holds(st["q"], st["rows"], c["T"]), (name, n, s)
            D = r["ids"].size
            if s == "main":
                n_high.append(r["n_high"])
                for k, v in r["events"].items():
                    events[k] = events.get(k, 0) + v
            if s == "high":
                assert r["n_high"] == D and D and not r["dropped"].any()
            if s == "low":
                assert r["n_high"] == (D if n == 0 else 0) and D
            if before is not None and s in before and c.get("predict_max_dt") is not None:
                live = before[s]["id"] >= 0
                late += int((t - before[s]["t_last"][live] > c["predict_max_dt"]).any())
        before = snap
    assert events["low_match"] and events["dropped"] and events["refused"] and events["kept_out"], events
    assert events["match"] and events["birth"] and events["expiry"], events
    assert sum(sum(r["events"]["low_match"] for s, r in res.items() if s == "low") for res, _ in gauge(name)), "low"
    if "n_high" in c:
        assert {63, 64, 65} <= set(n_high), n_high
    for edge in (64, 128):
        if c["T"] > edge:
            assert any(snap["main"]["id"][edge:].max() >= 0 for _, snap in gauge(name)), f"no slot from {edge} on"
    differ = 0
    if c["predict"]:
        assert c.get("predict_max_dt") is None or late, "no update with a gap longer than predict_max_dt"
        for (with_p, _), (without, _) in zip(gauge(name), gauge(name, predict=False)):
            for s, r in with_p.items():
                matched = (r["ids"] >= 0) & ~r["born"]
                differ += int((matched & (without[s]["ids"] != r["ids"])).sum())
            if differ:
                break                                       # after the first difference the two states part
        assert differ, "prediction changes no match in this scene"
    if c["assign"] == "optimal":
        assert max(max((st["rows"] for st in r["stages"]), default=0) for res, _ in gauge(name)
                   for r in res.values()) > 1
    return events, differ


def flat(frames):
    names = [s for s in STREAMS if s in frames]
    ids = [s for s in names for _ in range(frames[s]["kpts"].shape[0])]
    kp = np.concatenate([np.concatenate([frames[s]["kpts"], frames[s]["vis"][..., None]], axis=2) for s in names])
    return names, ids, kp, np.concatenate([frames[s]["area"] for s in names]), np.concatenate(
        [frames[s]["score"] for s in names])


def make_tracker(name, **kw):
    from probpose_pytorch_amd import OneEuro, PoseTracker
    c = CASES[name]
    opts = dict(high_thr=HIGH_THR, low_match_thr=LOW_MATCH_THR, birth_thr=BIRTH_THR) | {k: c[k] for k in OPTIONS
                                                                                         if k in c} | kw
    return PoseTracker(PR.default_sigmas(c["K"]), match_thr=MATCH_THR, max_age=MAX_AGE, max_tracks=c["T"],
                       vis_thr=c["vis_thr"], smooth=OneEuro(*c.get("smooth", SMOOTH)), **opts)


def run_device(name, calls=None, **kw):
    tr = make_tracker(name, **kw)
    out = []
    for t, frames in (scene(name) if calls is None else calls):
        names, ids, kp, ar, sc = flat(frames)
        res = tr.update(torch.from_numpy(kp).cuda(), torch.from_numpy(ar).cuda(), torch.from_numpy(sc).cuda(),
                        stream_ids=ids, t=t, streams=names)
        assert res.stream_ids == names
        host = {k: getattr(res, k).cpu().numpy() for k in ("ids", "keypoints", "oks", "born", "dropped")}
        seen = list(tr._index)
        out.append((host, {s: tr.tracks(s) for s in seen}, dict(zip(seen, tr.overflow.cpu().numpy().tolist()))))
    return out


def compare_with_gauge(calls, want_calls, got_calls, K):
    bound, worst = (2 * K + 2) * U, 0.0
    for n, ((t, frames), (want, snap), (got, tracks, overflow)) in enumerate(zip(calls, want_calls, got_calls)):
        names = [s for s in STREAMS if s in frames]
        cat = lambda key: np.concatenate([want[s][key] for s in names])
        assert got["ids"].dtype == np.int64 and got["born"].dtype == np.bool_ and got["dropped"].dtype == np.bool_
        assert np.array_equal(got["ids"], cat("ids")), (n, np.nonzero(got["ids"] != cat("ids"))[0])
        assert np.array_equal(got["born"], cat("born")), n
        assert np.array_equal(got["dropped"], cat("dropped")), n
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
    return worst / bound


@pytest.mark.parametrize("name", list(CASES))
def test_scenes_are_the_gauges_call_by_call(name):
    events, differ = check_fixture(name)
    worst = compare_with_gauge(scene(name), gauge(name), run_device(name), CASES[name]["K"])
    print(f"{name}: events {events}; prediction changes {differ} match(es) of the first call that differs; worst "
          f"|d OKS| = {worst:.4f} of the bound")


def test_two_runs_give_the_same_bits():
    name = "two_slots_per_lane"
    a, b = run_device(name), run_device(name)
    for (ga, ta, oa), (gb, tb, ob) in zip(a, b):
        assert all(ga[k].tobytes() == gb[k].tobytes() for k in ga) and oa == ob
        assert all(ta[s][k].tobytes() == tb[s][k].tobytes() for s in ta for k in ta[s])


# ---------------------------------------------------------------------------------------------- equivalences
def _same(a, b):
    for (ga, ta, oa), (gb, tb, ob) in zip(a, b):
        assert all(ga[k].tobytes() == gb[k].tobytes() for k in ga if k in gb) and oa == ob
        assert set(ta) == set(tb) and all(ta[s][k].tobytes() == tb[s][k].tobytes() for s in ta for k in ta[s])


def _staged_at_minus_inf(module, name, monkeypatch, **kw):
    """``module``'s tracker of case ``name`` through pp_track_assign_staged with high_thr = birth_thr = -inf (which the
    constructor, asking for finite thresholds, does not take: they are set on the object)."""
    from probpose_pytorch_amd import _lib
    tr = module.make_tracker(name, high_thr=0.0, **kw)
    tr.high_thr = tr.birth_thr = -np.inf
    launched, launch = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda entry, *a: (launched.append(entry), launch(entry, *a))[1])
    return tr, launched


@pytest.mark.parametrize("name", ["two_slots_per_lane", "three_slots_per_lane", "overflow", "near_duplicates"])
def test_the_staged_entry_at_minus_inf_is_pp_track_assign(name, monkeypatch):
    from tests import test_track_gpu as TG
    want = TG.run_device(name)
    tr, launched = _staged_at_minus_inf(TG, name, monkeypatch)
    got = TG.run_device(name, tracker=tr)
    assert launched.count("pp_track_assign_staged") == len(want) and "pp_track_assign" not in launched
    _same(want, got)


@pytest.mark.parametrize("name", ["one_slot_per_lane", "two_slots_per_lane"])
def test_the_staged_entry_at_minus_inf_is_pp_track_assign_optimal(name, monkeypatch):
    from tests import test_trackopt_gpu as OG
    want = OG.run_device(name, assign="optimal")
    tr, launched = _staged_at_minus_inf(OG, name, monkeypatch, assign="optimal")
    monkeypatch.setattr(OG, "make_tracker", lambda *a, **k: tr)
    got = OG.run_device(name, assign="optimal")
    assert launched.count("pp_track_assign_staged") == len(want) and "pp_track_assign_optimal" not in launched
    _same(want, got)


def test_the_predicted_entry_with_no_filter_state_and_max_dt_0_is_pp_track_oks(monkeypatch):
    """An unsmoothed tracker never initialises a filter (init all 0): on every call of its scene, the predicted entry
    on the arguments of pp_track_oks, with max_dt = 0, writes the workspace pp_track_oks writes."""
    from probpose_pytorch_amd import _lib
    from tests import test_track_gpu as TG
    name = "two_slots_per_lane"
    pairs, launch = [], _lib.launch

    def spy(entry, *a):
        rc = launch(entry, *a)
        if entry == "pp_track_oks":
            other = torch.full_like(a[-1], 7.0)
            launch("pp_track_oks_predicted", *a[:-1], 123.0, 0.0, other)
            pairs.append((a[-1].clone(), other))
        return rc

    monkeypatch.setattr(_lib, "launch", spy)
    tr = TG.make_tracker(name, smooth=False)
    TG.run_device(name, smooth=False, tracker=tr)
    assert all(int(tr.tracks(s)["init"].max()) == 0 for s in tr._index)
    assert len(pairs) == len(TG.scene(name)) and sum(a.numel() for a, _ in pairs) > 10000
    for a, b in pairs:
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert any(float(a.max()) > MATCH_THR for a, _ in pairs)


# ---------------------------------------------------------------------------------------------- the default path
@pytest.mark.parametrize("assign", ["greedy", "optimal"])
def test_the_default_tracker_launches_the_three_old_entries_and_nothing_else(assign, monkeypatch):
    from probpose_pytorch_amd import _lib
    from tests import test_track_gpu as TG
    name = "one_slot_per_lane"
    launched, launch = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda entry, *a: (launched.append((entry, len(a))), launch(entry, *a))[1])
    tr = TG.make_tracker(name, assign=assign)
    calls = TG.scene(name)[:3]
    for t, frames in calls:
        ids, kp, ar, sc = TG.flat(frames)
        res = tr.update(torch.from_numpy(kp).cuda(), torch.from_numpy(ar).cuda(), torch.from_numpy(sc).cuda(),
                        stream_ids=ids, t=t)
        assert res.dropped.dtype == torch.bool and res.dropped.shape == res.ids.shape and not bool(res.dropped.any())
    middle = ("pp_track_assign", 18) if assign == "greedy" else ("pp_track_assign_optimal", 19)
    assert launched == [("pp_track_oks", 13), middle, ("pp_track_filter", 16)] * len(calls), launched


def test_a_staged_predicted_update_synchronises_no_more_than_the_default_one():
    name = "one_slot_per_lane"
    tr = make_tracker(name, predict=True)
    inputs = []
    for t, frames in scene(name)[:3]:
        names, ids, kp, ar, sc = flat(frames)
        inputs.append((ids, names, t, [torch.from_numpy(a).cuda() for a in (kp, ar, sc)]))
    ids, names, t, dev = inputs[0]
    tr.update(*dev, stream_ids=ids, t=t, streams=names)             # allocates the state
    torch.cuda.synchronize()
    sync_mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            for ids, names, t, dev in inputs[1:]:
                tr.update(*dev, stream_ids=ids, t=t, streams=names)
            syncs = [w for w in seen if "synchroniz" in str(w.message).lower()]
    finally:
        torch.cuda.set_sync_debug_mode(sync_mode)
    assert len(syncs) == 2, [str(w.message) for w in syncs]          # the finiteness booleans of the two updates


# ---------------------------------------------------------------------------------------------- scored scenarios
EVAL_K, EVAL_FPS = 3, 25.0
EVAL_SHAPE = np.array([[0.0, 0.0], [30.0, 10.0], [10.0, 40.0]])
EVAL_AREA = 2160.0


def _person(x, y):
    return EVAL_SHAPE + np.array([x, y])


def _frame(people):
    """people: (x, y, score)."""
    kp = np.array([_person(x, y) for x, y, _ in people]).reshape(len(people), EVAL_K, 2)
    return TR.make_frame(kp, [s for _, _, s in people], [EVAL_AREA] * len(people), np.ones((len(people), EVAL_K)))


def _run_both(frames, keep=None, **opts):
    """The frames through the gauge (first, on the CPU) and through PoseTracker: per frame the ids of both, asserted
    equal.  ``keep(frame)``: the detections the caller hands on (a bool mask), None: all."""
    from probpose_pytorch_amd import OneEuro, PoseTracker
    sig = PR.default_sigmas(EVAL_K)
    smooth = opts.pop("smooth", None)
    g = SR.Tracker(sig, MATCH_THR, MAX_AGE, 8, None, smooth, EVAL_FPS, **opts)
    handed = []
    for f in frames:
        m = np.ones(f["score"].size, dtype=bool) if keep is None else keep(f)
        handed.append((m, TR.make_frame(f["kpts"][m], f["score"][m], f["area"][m], f["vis"][m])))
    want = [g.update({0: f})[0]["ids"] for _, f in handed]
    d = PoseTracker(sig, match_thr=MATCH_THR, max_age=MAX_AGE, max_tracks=8, fps=EVAL_FPS,
                    smooth=None if smooth is None else OneEuro(*smooth), **opts)
    got = []
    for _, f in handed:
        res = d.update(torch.from_numpy(f["kpts"]).cuda(), torch.from_numpy(f["area"]).cuda(),
                       torch.from_numpy(f["score"]).cuda())
        got.append(res.ids.cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(want, got)), (want, got)
    ids = []
    for (m, _), a in zip(handed, got):
        full = np.full(m.size, -1, dtype=np.int64)
        full[m] = a
        ids.append(full)
    return ids


def _score(frames, who, ids):
    """IDSW and Frag of PoseTrackEval: the ground truth is every detection with who >= 0 (its person), the predictions
    every detection with an id."""
    from probpose_pytorch_amd import PoseTrackEval
    ev = PoseTrackEval(PR.default_sigmas(EVAL_K), thresholds=(0.5,))
    for f, w, i in zip(frames, who, ids):
        w = np.asarray(w)
        gt = w >= 0
        kp = np.concatenate([f["kpts"][gt], np.full((int(gt.sum()), EVAL_K, 1), 2.0)], axis=2)
        box = np.concatenate([f["kpts"][gt].min(axis=1), np.ptp(f["kpts"][gt], axis=1)], axis=1).reshape(-1, 4)
        ev.add_frame("s", w[gt].astype(np.int64), kp, box, f["area"][gt], i[i >= 0], f["kpts"][i >= 0])
    m = ev.evaluate()["metrics"][0]
    return m["IDSW"], m["Frag"]


def test_prediction_carries_an_accelerating_person_across_another():
    """Person 0 accelerates along x from rest (x = 600 t^2 at 25 frames per second: 3 units in the second frame, 57 in
    the 30th), passing person 1, who stands 6 units above the path at x = 300 (OKS 0.43 with a pose on the path).
    Without ``predict`` the steps outgrow the OKS of the last position and the track breaks; with it, and a filter
    quick enough to follow the speed (FAST), the run has no switch and no fragment."""
    frames, who = [], []
    for n in range(1, 31):
        t = n / EVAL_FPS
        frames.append(_frame([(600.0 * t * t, 0.0, 0.9), (300.0, 6.0, 0.8)]))
        who.append([0, 1])
    smooth = FAST
    plain = _run_both(frames, smooth=smooth)
    moved = _run_both(frames, smooth=smooth, predict=True)
    assert len({int(i[0]) for i in plain}) > 1, "the gauge without predict already keeps the track"
    assert {int(i[0]) for i in moved} == {0} and {int(i[1]) for i in moved} == {1}
    idsw, frag = _score(frames, who, plain)
    assert idsw + frag >= 1, (idsw, frag)
    assert _score(frames, who, moved) == (0, 0)


def test_the_cascade_keeps_a_dimmed_person_and_gives_clutter_no_id():
    """Person 0 walks slowly; its score is 0.9, except 0.3 in frames 6 - 10 (MAX_AGE + 3 frames).  Clutter (person -1)
    of score 0.25 - 0.4 appears far away in frames 4 - 13, every piece for two consecutive frames."""
    frames, who = [], []
    for n in range(18):
        people, w = [(100.0 + 2.0 * n, 50.0, 0.3 if 6 <= n <= 10 else 0.9)], [0]
        if 4 <= n <= 13:
            c = (n - 4) // 2
            people.append((1000.0 + 500.0 * c, 900.0, 0.25 + 0.03 * c))
            w.append(-1)
        frames.append(_frame(people))
        who.append(w)
    clutter = [np.asarray(w) < 0 for w in who]
    cascade = _run_both(frames, high_thr=0.5)
    assert all((i[c] == -1).all() for i, c in zip(cascade, clutter)) and {int(i[0]) for i in cascade} == {0}
    assert _score(frames, who, cascade) == (0, 0)
    by_caller = _run_both(frames, keep=lambda f: f["score"] >= 0.5)
    idsw, frag = _score(frames, who, by_caller)
    assert frag >= 1 and len({int(i[0]) for i in by_caller} - {-1}) == 2, (idsw, frag)
    neither = _run_both(frames)
    assert any((i[c] >= 0).any() for i, c in zip(neither, clutter)) and {int(i[0]) for i in neither} == {0}


# ---------------------------------------------------------------------------------------------- the command line
def test_the_command_line_runs_the_predicted_and_the_staged_launch(tmp_path, monkeypatch):
    """inference --track --smooth --predict --high-thr --birth-thr on the frames of tests/test_track_inference.py: the
    box of score 0.9 keeps id 0; the box of score 0.8 is a row of stage 1 but below --birth-thr, so it is never born
    and is dropped in every frame; every update went through the two new entries."""
    from probpose_pytorch_amd import _lib, inference
    from tests.test_track_inference import ARGS, write_frames
    names, table = write_frames(tmp_path / "frames")
    launched, launch = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a: (launched.append(name), launch(name, *a))[1])
    record = inference.main(ARGS + ["--frames", str(tmp_path / "frames"), "--boxes-json", str(table), "--track",
                                    "--smooth", "--predict", "0.5", "--high-thr", "0.5", "--low-match-thr", "0.2",
                                    "--birth-thr", "0.85", "--output", str(tmp_path / "out")])
    assert [[d["id"] for d in r["detections"]] for r in record] == [[0, -1], [-1, 0], [0, -1], [-1, 0]]
    assert launched.count("pp_track_oks_predicted") == launched.count("pp_track_assign_staged") == len(names)
    assert not {"pp_track_oks", "pp_track_assign", "pp_track_assign_optimal"} & set(launched)
