"""CPU tests of the optimal track association: the gauge tests/trackopt_reference.py against scipy's
linear_sum_assignment and against exhaustive search, the gauge against its planted faults, the 2 x 2 example on which
the greedy walk switches an identity, and the refusals of PoseTracker(assign="optimal"), of pp_track_assign_optimal
(through ctypes, made-up device addresses: nothing is launched) and of the --assign flag.  None of this needs a GPU."""
import itertools

import numpy as np
import pytest

from tests import posenms_reference as PR
from tests import track_reference as TR
from tests import trackopt_reference as OR

THRESHOLDS = (0.0, 0.3, 0.6)


def random_oks(rng, D, T, quarter):
    if quarter:
        return rng.integers(0, 5, (D, T)) / 4.0
    return rng.uniform(0.0, 1.0, (D, T))


def exhaustive(q):
    """The largest total over every assignment of the D rows to distinct columns of 0 .. max(D, T) - 1."""
    D, T = len(q), len(q[0])
    m = max(D, T)
    return max(sum(q[i][j] for i, j in enumerate(cols) if j < T) for cols in itertools.permutations(range(m), D))


def check_matching(q, slots):
    D, T = len(q), len(q[0])
    got = [j for j in slots if j >= 0]
    assert len(slots) == D and len(set(got)) == len(got) and all(0 <= j < T for j in got)
    assert all(q[i][j] > 0 for i, j in enumerate(slots) if j >= 0), "an inadmissible pair is matched"
    free = set(range(T)) - set(got)
    assert not any(q[i][j] > 0 for i, j0 in enumerate(slots) if j0 < 0 for j in free), "an admissible pair is left out"


def cases():
    """(q, oks, live, thr): every shape D, T in 1 .. 6, three thresholds, continuous and quarter-step OKS, some columns
    not live with large OKS; then the special matrices."""
    rng = np.random.default_rng(11)
    for D, T, thr, quarter in itertools.product(range(1, 7), range(1, 7), THRESHOLDS, (False, True)):
        oks = random_oks(rng, D, T, quarter)
        live = rng.uniform(size=T) < 0.8
        oks[:, ~live] = 0.99                            # a dead column must not attract anybody
        yield OR.quantise(oks, live, thr), oks, live, thr
    ones = np.ones(3, dtype=bool)
    yield OR.quantise(np.full((4, 3), 0.2), ones, 0.3), np.full((4, 3), 0.2), ones, 0.3         # nothing admissible
    nan = np.array([[np.nan, 0.5, 0.4], [0.9, np.nan, 0.4]])
    yield OR.quantise(nan, ones, 0.3), nan, ones, 0.3
    dead = np.array([[0.99, 0.4], [0.99, 0.5], [0.99, 0.45]])
    yield OR.quantise(dead, np.array([False, True]), 0.3), dead, np.array([False, True]), 0.3


def test_solve_reaches_the_optimum_of_scipy_and_of_exhaustive_search():
    from scipy.optimize import linear_sum_assignment
    n, shapes = 0, set()
    for q, oks, live, thr in cases():
        D, T = len(q), len(q[0])
        slots, steps = OR.solve(q)
        check_matching(q, slots)
        assert 1 <= steps <= D * (max(D, T) + 1)
        got = OR.total(q, slots)
        qa = np.array(q, dtype=np.int64)
        rows, cols = linear_sum_assignment(qa, maximize=True)
        assert got == int(qa[rows, cols].sum()), (q, slots)
        assert got == exhaustive(q), (q, slots)
        for i, j in enumerate(slots):
            assert j < 0 or (live[j] and oks[i, j] > thr)
        shapes.add((D, T))
        n += 1
    assert n == 6 * 6 * 3 * 2 + 3 and any(D < T for D, T in shapes) and any(D > T for D, T in shapes)


def test_special_matrices():
    ones = np.ones(3, dtype=bool)
    assert OR.solve(OR.quantise(np.full((4, 3), 0.2), ones, 0.3))[0] == [-1] * 4
    q = OR.quantise(np.array([[np.nan, 0.5, 0.4], [0.9, np.nan, 0.4]]), ones, 0.3)
    assert q[0][0] == 0 and q[1][1] == 0 and OR.solve(q)[0] == [1, 0]
    q = OR.quantise(np.array([[0.99, 0.4], [0.99, 0.5], [0.99, 0.45]]), np.array([False, True]), 0.3)
    assert [r[0] for r in q] == [0, 0, 0] and OR.solve(q)[0] == [-1, 1, -1]
    assert OR.solve([])[0] == [] and OR.solve([[], []])[0] == [-1, -1]
    # the weight itself: 1 above the threshold by the least bit, 1 + 2^40 at the cap
    assert OR.weight(np.nextafter(0.3, 1.0), 0.3) == 1 and OR.weight(0.3, 0.3) == 0 and OR.weight(np.nan, 0.0) == 0
    assert OR.weight(1.0, 0.0) == 1 + 2 ** 40 and OR.weight(np.inf, 0.5) == 1 + 2 ** 40
    assert OR.weight(0.55, 0.3) == 1 + int(np.floor((np.float64(0.55) - np.float64(0.3)) * 2.0 ** 40))


def greedy_on_matrix(oks, thr):
    """track_reference's rule 3 on a ready matrix, every column live."""
    taken, slots = set(), []
    for row in oks:
        best = max((j for j in range(len(row)) if j not in taken), key=lambda j: (row[j], -j), default=None)
        if best is not None and row[best] > thr:
            taken.add(best)
            slots.append(best)
        else:
            slots.append(-1)
    return slots


def test_the_example_greedy_switches_an_identity_and_optimal_does_not():
    oks = np.array(OR.EXAMPLE)
    q = OR.quantise(oks, np.ones(2, dtype=bool), 0.3)
    assert greedy_on_matrix(oks, 0.3) == [0, -1] and OR.solve(q)[0] == [1, 0]
    assert OR.margin(q) == OR.total(q, [1, 0]) - q[0][0] > 2 ** 38
    # the same through both trackers, on a scene whose second frame has these pair OKS
    sig = PR.default_sigmas(1)
    first, second = OR.crossing_pair(sig)
    greedy, optimal = TR.Tracker(sig, 0.3, 30, 4), OR.Tracker(sig, 0.3, 30, 4)
    for tr in (greedy, optimal):
        assert tr.update({0: first})[0]["ids"].tolist() == [0, 1]
    g, o = greedy.update({0: second})[0], optimal.update({0: second})[0]
    seen = np.array(o["oks_seen"]).reshape(2, 2)
    assert np.abs(seen - oks).max() < 1e-12, seen
    assert g["ids"].tolist() == [0, 2] and g["born"].tolist() == [False, True]          # B's track ages, a new id
    assert o["ids"].tolist() == [1, 0] and not o["born"].any() and o["slots"] == [1, 0]
    assert np.array_equal(o["oks"], seen[[0, 1], [1, 0]])
    assert greedy.streams[0].age.tolist()[:3] == [0, 1, 0] and optimal.streams[0].age.tolist()[:2] == [0, 0]


def test_the_optimal_tracker_is_the_greedy_one_where_nobody_competes():
    """People far apart: one candidate per detection, so both associations, and everything after them, agree."""
    K = 3
    sig = PR.default_sigmas(K)
    frames, times, _ = TR.make_scene(5, K, 10, 6, 2, leavers=1, entrants=1)
    greedy, optimal = TR.Tracker(sig, 0.3, 2, 8, 0.2, (1.0, 0.05, 1.0)), OR.Tracker(sig, 0.3, 2, 8, 0.2,
                                                                                     (1.0, 0.05, 1.0))
    events = {}
    for f, t in zip(frames, times):
        g, o = greedy.update({0: f}, t)[0], optimal.update({0: f}, t)[0]
        for k in ("ids", "keypoints", "oks", "born"):
            assert g[k].tobytes() == o[k].tobytes(), k
        for k, v in o["events"].items():
            events[k] = events.get(k, 0) + v
    assert events["match"] and events["birth"] and events["expiry"] and events["reid"], events
    a, b = greedy.streams[0], optimal.streams[0]
    assert all(np.array(getattr(a, k)).tobytes() == np.array(getattr(b, k)).tobytes()
               for k in ("id", "age", "t_last", "area", "kp", "vis", "xhat", "dxhat", "init"))


def test_planted_faults_are_told_from_the_rule():
    ones = np.ones(2, dtype=bool)
    # >= instead of > at the threshold
    on_thr = np.array([[0.5, 0.2]])
    assert OR.solve(OR.quantise(on_thr, ones, 0.5))[0] == [-1]
    assert OR.solve(OR.quantise(on_thr, ones, 0.5, ge=True))[0] == [0]
    # the highest instead of the lowest column on equal minv
    assert OR.solve([[5, 5]])[0] == [0] and OR.solve([[5, 5]], highest=True)[0] == [1]
    tie = OR.quantise(np.array([[0.75, 0.75], [0.75, 0.75]]), ones, 0.3)
    assert OR.solve(tie)[0] == [0, 1] and OR.solve(tie, highest=True)[0] != [0, 1]
    # forgetting the q > 0 filter at the end
    nothing = OR.quantise(np.full((2, 2), 0.1), ones, 0.3)
    assert OR.solve(nothing)[0] == [-1, -1] and OR.solve(nothing, keep_zero=True)[0] != [-1, -1]
    # and over the random cases each fault changes at least one answer, the rule none
    changed = dict(ge=0, highest=0, keep_zero=0)
    for q, oks, live, thr in cases():
        want = OR.solve(q)[0]
        changed["ge"] += OR.solve(OR.quantise(oks, live, thr, ge=True))[0] != want
        changed["highest"] += OR.solve(q, highest=True)[0] != want
        changed["keep_zero"] += OR.solve(q, keep_zero=True)[0] != want
    assert all(changed.values()), changed


def test_margin():
    assert OR.margin([[10, 9], [9, 1]]) == 18 - 11          # without (0, 1): 10 + 1; without (1, 0): 10 + 1
    assert OR.margin([[7]]) == 7 and OR.margin([[0, 0]]) == OR.INF and OR.margin([[4, 4]]) == 0


def test_python_refusals():
    from probpose_pytorch_amd import PoseTracker, _lib, tracker
    sig = np.full(3, 0.05)
    assert tracker.OPT_MAX == _lib.PP_TRACK_OPT_MAX == 256
    assert PoseTracker(sig).assign == "greedy" and PoseTracker(sig, assign="greedy").assign == "greedy"
    tr = PoseTracker(sig, assign="optimal", max_tracks=_lib.PP_TRACK_OPT_MAX)
    assert tr.assign == "optimal"
    for word in ("hungarian", "", None, "Optimal"):
        with pytest.raises(ValueError, match="assign"):
            PoseTracker(sig, assign=word)
    with pytest.raises(TypeError):
        PoseTracker(sig, 0.3, 30, 64, None, None, 30.0, "optimal")      # keyword-only
    with pytest.raises(ValueError, match="max_tracks: 257 is above the 256"):
        PoseTracker(sig, assign="optimal", max_tracks=257)
    PoseTracker(sig, assign="greedy", max_tracks=257)
    M = _lib.PP_TRACK_OPT_MAX + 1
    kp, ones = np.zeros((M + 2, 3, 2)), np.ones(M + 2)
    ids = ["a", "a"] + ["cam"] * M
    with pytest.raises(ValueError, match=f"stream_ids: stream 'cam' has {M} detections, more than the 256"):
        tr.update(kp, ones, ones, stream_ids=ids)
    with pytest.raises(_lib.HipExtensionError):             # 256 are taken: the device is needed now
        tr.update(kp[:-1], ones[:-1], ones[:-1], stream_ids=ids[:-1])
    with pytest.raises(_lib.HipExtensionError):             # and greedy takes the 257
        PoseTracker(sig, max_tracks=300).update(kp, ones, ones, stream_ids=ids)


DEV = dict(off=0x80000, blocks=0x20000, oks=0x70000, area=0x50000, ids=0x90000, match_oks=0xa0000, born=0xb0000,
           slot_of=0xc0000, te=0xd0000, total=0xf0000)


def _assign(lib, host_off=(0, 3, 3, 10), n_str=None, K=17, T=64, Dtot=None, match_thr=0.3, max_age=30, t=1.0,
            t_prev=0.5, null=(), no_host=False):
    off = np.asarray(host_off, dtype=np.int64)
    p = {k: (None if k in null else v) for k, v in DEV.items()}
    return lib.pp_track_assign_optimal(len(off) - 1 if n_str is None else n_str, K, T,
                                       int(off[-1]) if Dtot is None else Dtot, None if no_host else off.ctypes.data,
                                       p["off"], p["blocks"], p["oks"], p["area"], match_thr, max_age, t, t_prev,
                                       p["ids"], p["match_oks"], p["born"], p["slot_of"], p["te"], p["total"], None)


def test_the_entry_refuses_bad_arguments_before_any_launch(built_lib):
    L = built_lib
    for kwargs, word in ((dict(host_off=(1, 3, 10)), b"do not start at 0"),
                         (dict(host_off=(0, 5, 3, 10)), b"not monotone at stream 1"),
                         (dict(host_off=(0, 3, 10), Dtot=11), b"the arrays hold 11"),
                         (dict(host_off=(0, 3, 10), n_str=-1), b"n_str"),
                         (dict(host_off=(0, 2, 4099, 4100)), b"stream 1 has 4097 detections"),
                         (dict(no_host=True), b"null host offsets"),
                         (dict(K=0), b"K=0"), (dict(T=0), b"max_tracks=0"), (dict(T=4097), b"max_tracks=4097"),
                         (dict(match_thr=1.0), b"match_thr"), (dict(match_thr=float("nan")), b"match_thr"),
                         (dict(max_age=-1), b"max_age=-1"),
                         (dict(t=0.5, t_prev=0.5), b"te <= 0"), (dict(t=float("inf")), b"te <= 0"),
                         *[(dict(null=(k,)), b"null argument")
                           for k in ("off", "blocks", "oks", "area", "ids", "match_oks", "born", "slot_of", "te")],
                         # the two limits of this entry
                         (dict(T=257), b"max_tracks=257 is above PP_TRACK_OPT_MAX = 256"),
                         (dict(T=4096), b"PP_TRACK_OPT_MAX = 256"),
                         (dict(host_off=(0, 2, 259, 300)), b"stream 1 has 257 detections, more than PP_TRACK_OPT_MAX"),
                         (dict(host_off=(0, 257), T=256), b"stream 0 has 257 detections")):
        rc = _assign(L, **kwargs)
        assert rc < 0 and word in L.pp_last_error() and b"pp_track_assign_optimal" in L.pp_last_error(), (
            kwargs, rc, L.pp_last_error())
    # what launches nothing returns 0, with or without a total
    assert _assign(L, host_off=(0,), T=256, t_prev=float("-inf")) == 0, L.pp_last_error()
    assert _assign(L, host_off=(0,), null=("total",), match_thr=0.0, max_age=0) == 0, L.pp_last_error()
    assert _assign(L, host_off=(0,), T=257) < 0             # checked even when nothing would launch


def test_the_constant_and_the_symbol_are_in_the_header_and_the_binding():
    from probpose_pytorch_amd import _lib
    header = open(_lib.LIB_PATH.replace("probpose_pytorch_amd/lib/libprobpose_hip.so", "include/probpose_hip.h")).read()
    assert f"#define PP_TRACK_OPT_MAX {_lib.PP_TRACK_OPT_MAX}\n" in header and _lib.PP_TRACK_OPT_MAX == 256
    assert "int pp_track_assign_optimal(" in header and "pp_track_assign_optimal" in _lib.EXPORTS
    assign, optimal = _lib._SIGNATURES["pp_track_assign"], _lib._SIGNATURES["pp_track_assign_optimal"]
    assert optimal[0] is assign[0] and optimal[1][:-1] == assign[1] and optimal[1][-1] is optimal[1][-2]
    assert _lib.PP_TRACK_OPT_MAX <= _lib.PP_TRACK_MAX_TRACKS and _lib.PP_TRACK_OPT_MAX % 64 == 0


def test_the_assign_flag(capsys):
    from probpose_pytorch_amd import inference
    with pytest.raises(SystemExit):
        inference.main(["--assign", "hungarian"])
    assert "--assign" in capsys.readouterr().err
    with pytest.raises(SystemExit):                         # accepted by the parser, refused for what it lacks
        inference.main(["--assign", "optimal"])
    assert "--assign needs --track" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        inference.main(["--track", "--assign", "optimal"])
    err = capsys.readouterr().err
    assert "error: --track needs --frames" in err
