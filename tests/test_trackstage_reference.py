"""CPU tests of the gauge tests/trackstage_reference.py (motion prediction, two-stage association, gated births): with
every option off it is the single-stage gauges call by call; with both thresholds at -inf likewise; and small
hand-worked frames for each rule.  None of this needs a GPU."""
import numpy as np
import pytest

from tests import posenms_reference as PR
from tests import track_reference as TR
from tests import trackopt_reference as OR
from tests import trackstage_reference as SR

SMOOTH = (1.0, 0.05, 1.0)
STATE = ("id", "age", "t_last", "area", "kp", "vis", "xhat", "dxhat", "init")


def same_state(a, b):
    return all(np.array(getattr(a, k)).tobytes() == np.array(getattr(b, k)).tobytes() for k in STATE) and \
        (a.next_id, a.overflow) == (b.next_id, b.overflow)


def scenes():
    """(name, K, T, max_age, vis_thr, frames, times): the single-stage gauges' own scenes, small."""
    yield ("plain", 3, 8, 2, 0.2) + TR.make_scene(5, 3, 10, 6, 2, leavers=1, entrants=1)[:2]
    yield ("overflow", 2, 4, 2, None) + TR.make_scene(5, 2, 8, 9, 2)[:2]
    yield ("duplicates", 3, 8, 2, 0.2) + TR.make_scene(7, 3, 10, 6, 2, duplicates=True)[:2]
    first, second = OR.crossing_pair(PR.default_sigmas(1))
    yield ("crossing", 1, 4, 30, None, [first, second], np.array([0.1, 0.2]))


@pytest.mark.parametrize("assign", ["greedy", "optimal"])
@pytest.mark.parametrize("options", [{}, dict(high_thr=-np.inf, birth_thr=-np.inf),
                                     dict(high_thr=-np.inf, birth_thr=-np.inf, low_match_thr=0.1, low_max_age=5)])
def test_without_its_options_the_gauge_is_the_single_stage_gauge_call_by_call(assign, options):
    single = TR.Tracker if assign == "greedy" else OR.Tracker
    events, differ = {}, 0
    for name, K, T, max_age, vis_thr, frames, times in scenes():
        sig = PR.default_sigmas(K)
        want = single(sig, 0.3, max_age, T, vis_thr, SMOOTH)
        got = SR.Tracker(sig, 0.3, max_age, T, vis_thr, SMOOTH, assign=assign, **options)
        other = (OR.Tracker if assign == "greedy" else TR.Tracker)(sig, 0.3, max_age, T, vis_thr, SMOOTH)
        for f, t in zip(frames, times):
            w, g, o = want.update({0: f}, t)[0], got.update({0: f}, t)[0], other.update({0: f}, t)[0]
            for k in ("ids", "keypoints", "oks", "born"):
                assert g[k].tobytes() == w[k].tobytes(), (name, k)
            assert not g["dropped"].any() and g["n_high"] == f["kpts"].shape[0]
            assert same_state(got.streams[0], want.streams[0]), name
            differ += int(not np.array_equal(w["ids"], o["ids"]))
            for k in w["events"]:
                events[k] = events.get(k, 0) + g["events"][k]
                assert g["events"][k] == w["events"][k], (name, k)
    assert differ, "greedy and optimal never disagree on these scenes: the comparison would not tell them apart"
    assert all(events[k] for k in ("match", "birth", "expiry", "reid", "overflow", "reinit")), events


# ---------------------------------------------------------------------------------------------- hand-worked frames
# K = 1, sigma 0.05, area 10000: a detection d away from a track has OKS exp(-d^2 / 200) (up to DBL_EPSILON in the
# area): 1 at 0, 0.88 at 5, 0.61 at 10, 0.14 at 20, 0 at 100
SIG, AREA = np.array([0.05]), 10000.0


def frame(*people):
    """people: (x, score)."""
    return TR.make_frame(np.array([[[x, 0.0]] for x, _ in people]).reshape(len(people), 1, 2),
                         [s for _, s in people], [AREA] * len(people), np.ones((len(people), 1)))


def tracker(**kw):
    kw.setdefault("max_tracks", 4)
    return SR.Tracker(SIG, match_thr=0.3, max_age=30, **kw)


def test_a_score_equal_to_high_thr_is_high():
    """A track unseen for one frame is invisible to stage 2 (low_max_age 0); the detection that returns to it scores
    exactly high_thr, so it is a row of stage 1 and continues the track; one ulp below it would be dropped."""
    for score, ids, dropped in ((0.5, [0], [False]), (np.nextafter(0.5, 0.0), [-1], [True])):
        tr = tracker(high_thr=0.5, birth_thr=0.6)
        assert tr.update({0: frame((0.0, 0.9))})[0]["ids"].tolist() == [0]
        tr.update({0: frame()})
        assert tr.streams[0].age[0] == 1
        r = tr.update({0: frame((1.0, score))})[0]
        assert r["ids"].tolist() == ids and r["dropped"].tolist() == dropped and r["n_high"] == int(not dropped[0])
        assert not r["born"].any() and tr.streams[0].overflow == 0


def test_a_slot_aged_past_low_max_age_is_invisible_to_stage_two_but_still_ages():
    for low_max_age, ids, age in ((0, [-1], 2), (1, [0], 0)):
        tr = tracker(high_thr=0.5, low_max_age=low_max_age)
        tr.update({0: frame((0.0, 0.9))})
        tr.update({0: frame()})
        r = tr.update({0: frame((1.0, 0.4))})[0]
        assert r["ids"].tolist() == ids and r["dropped"].tolist() == [ids[0] < 0] and r["n_high"] == 0
        assert tr.streams[0].age[0] == age and tr.streams[0].id[0] == 0
        assert r["events"]["kept_out"] == int(low_max_age == 0) and r["events"]["low_match"] == int(low_max_age == 1)
        assert r["oks"][0] == (0.0 if ids[0] < 0 else r["oks_seen"][0]) and 0.99 < r["oks_seen"][0] < 1.0
    # a high detection reaches the old slot in stage 1 whatever its age
    tr = tracker(high_thr=0.5, low_max_age=0)
    tr.update({0: frame((0.0, 0.9))})
    tr.update({0: frame()})
    assert tr.update({0: frame((1.0, 0.7))})[0]["ids"].tolist() == [0]


def test_stage_two_takes_what_stage_one_left_at_its_own_threshold():
    """Two tracks; the low detection sits nearer to track 0 than the high one does, but the high one chooses first;
    the low one continues track 1 at OKS 0.14 only under low_match_thr 0.1."""
    for low_match_thr, ids in ((None, [0, -1]), (0.1, [0, 1])):
        tr = tracker(high_thr=0.5, low_match_thr=low_match_thr)
        assert tr.update({0: frame((0.0, 0.9), (25.0, 0.8))})[0]["ids"].tolist() == [0, 1]
        r = tr.update({0: frame((3.0, 0.7), (5.0, 0.2))})[0]
        assert r["ids"].tolist() == ids and r["n_high"] == 1 and r["dropped"].tolist() == [False, ids[1] < 0]
        assert tr.streams[0].age[:2].tolist() == [0, int(ids[1] < 0)]
    # the low detection comes first in the input: stage order is by score, not by position
    tr = tracker(high_thr=0.5, low_match_thr=0.1)
    tr.update({0: frame((0.0, 0.9), (25.0, 0.8))})
    assert tr.update({0: frame((5.0, 0.2), (3.0, 0.7))})[0]["ids"].tolist() == [1, 0]


def test_a_dropped_detection_does_not_touch_overflow():
    for birth_thr, overflow, dropped in ((0.5, 0, [False, True]), (-np.inf, 1, [False, False])):
        tr = tracker(max_tracks=1, high_thr=0.5, birth_thr=birth_thr)
        tr.update({0: frame((0.0, 0.9))})
        r = tr.update({0: frame((1.0, 0.9), (100.0, 0.3))})[0]
        assert r["ids"].tolist() == [0, -1] and r["dropped"].tolist() == dropped and not r["born"].any()
        assert tr.streams[0].overflow == overflow and r["events"]["overflow"] == overflow
    # birth_thr alone: one stage, gated births; a low detection still continues a track of any age
    tr = tracker(birth_thr=0.5)
    tr.update({0: frame((0.0, 0.9), (50.0, 0.3))})
    assert tr.streams[0].id.tolist() == [0, -1, -1, -1]
    tr.update({0: frame()})
    r = tr.update({0: frame((1.0, 0.2), (50.0, 0.5))})[0]
    assert r["ids"].tolist() == [0, 1] and r["born"].tolist() == [False, True] and r["n_high"] == 2


def test_an_optimal_stage_one_beats_the_greedy_walk_on_a_near_duplicate_pair():
    sig = PR.default_sigmas(1)
    first, second = OR.crossing_pair(sig)
    got = {}
    for assign in ("greedy", "optimal"):
        tr = SR.Tracker(sig, 0.3, 30, 4, assign=assign, high_thr=0.5)
        assert tr.update({0: first})[0]["ids"].tolist() == [0, 1]
        got[assign] = tr.update({0: second})[0]
    assert got["greedy"]["ids"].tolist() == [0, 2] and got["greedy"]["born"].tolist() == [False, True]
    assert got["optimal"]["ids"].tolist() == [1, 0] and not got["optimal"]["born"].any()
    assert got["optimal"]["stages"][0]["rows"] == 2 and len(got["optimal"]["stages"]) == 1
    # with the second detection low, the optimal stage 1 has one row and takes its best column: the greedy outcome
    low = TR.make_frame(second["kpts"], [0.9, 0.4], second["area"], second["vis"])
    tr = SR.Tracker(sig, 0.3, 30, 4, assign="optimal", high_thr=0.5)
    tr.update({0: first})
    r = tr.update({0: low})[0]
    assert r["ids"].tolist() == [0, -1] and r["dropped"].tolist() == [False, True] and len(r["stages"]) == 2


# ---------------------------------------------------------------------------------------------- prediction
def test_the_predicted_pose_is_one_product_and_one_sum_per_coordinate():
    st = TR.Stream(2, 2)
    st.kp[1], st.xhat[1] = [[1.0, 2.0], [3.0, 4.0]], [[10.0, 20.0], [30.0, 40.0]]
    st.dxhat[1] = [[0.1, -0.2], [7.0, 7.0]]
    st.init[1], st.t_last[1] = [1, 0], 0.7
    dt = np.float64(1.0) - np.float64(0.7)
    want = [[np.float64(10.0) + np.float64(0.1) * dt, np.float64(20.0) + np.float64(-0.2) * dt], [3.0, 4.0]]
    assert SR.predicted_pose(st, 1, 1.0, np.inf).tolist() == want
    assert SR.predicted_pose(st, 1, 1.0, 0.25).tolist() == [[10.025, 19.95], [3.0, 4.0]]      # dt clamped to max_dt
    assert SR.predicted_pose(st, 1, 1.0, 0.0).tolist() == [[10.0, 20.0], [3.0, 4.0]]
    assert SR.predicted_pose(st, 0, 1.0, np.inf).tolist() == [[0.0, 0.0], [0.0, 0.0]]          # nothing initialised


def test_lag_and_overshoot_cancel_on_a_constant_velocity_track():
    """With a constant cutoff (beta 0) and a constant frame time, xhat lags a constant-velocity track by (1 - a) v te /
    a and dxhat settles at v / a: xhat + dxhat * te is the next true position."""
    te, v, smooth = 0.04, 250.0, (1.0, 0.0, 1.0)
    a = TR.alpha(te, 1.0)
    xhat, dxhat = np.float64(0.0), np.float64(0.0)
    for n in range(1, 400):
        xhat, dxhat = TR.one_euro_step(v * te * n, xhat, dxhat, te, smooth)
    x = v * te * 399
    assert abs((x - xhat) - (1 - a) * v * te / a) < 1e-6 and abs(dxhat - v / a) < 1e-6
    assert abs(xhat + dxhat * te - (x + v * te)) < 1e-6


def test_prediction_keeps_a_fast_track_that_the_last_position_loses():
    """One person at a constant 12 units per frame (OKS 0.49 against the last position) and then a gap of three
    frames: the stored pose is 48 away (OKS 1e-5), the predicted one is where the person is.  The cutoff is high
    (a = 0.96): dxhat settles at v / a, so over a gap of n frames the prediction overshoots by about (n - 1) (1 / a - 1)
    frames' worth of motion, here 1.5 units."""
    ids = {}
    for predict in (False, True):
        tr = tracker(smooth=(100.0, 0.0, 1.0), fps=25.0, predict=predict)
        seen = []
        for n in range(40):
            seen += tr.update({0: frame((12.0 * n, 0.9))})[0]["ids"].tolist()
        for _ in range(3):
            tr.update({0: frame()})
        r = tr.update({0: frame((12.0 * 43, 0.9))})[0]
        ids[predict] = seen + r["ids"].tolist()
        assert (r["oks"][0] > 0.95) == predict
    assert set(ids[True]) == {0} and ids[False][-1] == 1 and set(ids[False][:-1]) == {0}
    # with predict_max_dt below the gap the track is moved by less and lost again
    tr = tracker(smooth=(100.0, 0.0, 1.0), fps=25.0, predict=True, predict_max_dt=0.04)
    for n in range(40):
        tr.update({0: frame((12.0 * n, 0.9))})
    for _ in range(3):
        tr.update({0: frame()})
    assert tr.update({0: frame((12.0 * 43, 0.9))})[0]["born"].tolist() == [True]
