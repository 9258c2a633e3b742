"""The gauge of PoseTracker (tests/track_reference.py) on hand-computed cases, and each rule told from its mutation.

The hand cases use one keypoint with sigma 0.05 and areas of 100: e = d^2 / 0.01 / (100 + eps) / 2 = d^2 / 2, so two
poses a distance d apart have OKS exp(-d^2 / 2): 0.8825 at 0.5, 0.6065 at 1, 0.1353 at 2, 0 (underflow) at 100.
"""
import math

import numpy as np
import pytest

from tests import posenms_reference as PR
from tests import track_reference as TR

SIG1 = np.array([0.05])


def frame(xs, scores=None, areas=None, vis=None, K=1):
    """Detections on the x axis: every keypoint of detection i at (xs[i], 0)."""
    xs = np.asarray(xs, dtype=np.float64).reshape(-1)
    kp = np.zeros((xs.size, K, 2))
    kp[:, :, 0] = xs[:, None]
    scores = np.linspace(0.9, 0.5, xs.size) if scores is None else scores
    return TR.make_frame(kp, scores, np.full(xs.size, 100.0) if areas is None else areas, vis)


def tracker(**kw):
    kw.setdefault("max_age", 2)
    kw.setdefault("max_tracks", 4)
    return TR.Tracker(kw.pop("sigmas", SIG1), **kw)


def step(tr, fr, t=None):
    return tr.update({0: fr}, t)[0]


def test_pair_oks_of_the_hand_cases():
    for d, want in ((0.5, math.exp(-0.125)), (1.0, math.exp(-0.5)), (2.0, math.exp(-2.0)), (100.0, 0.0)):
        got = PR.pair_oks([[d, 0.0]], [[0.0, 0.0]], 100.0, 100.0, SIG1)
        assert got == pytest.approx(want, rel=1e-12, abs=0.0)


@pytest.mark.parametrize("given_order", [False, True])
def test_two_detections_prefer_one_track_the_higher_score_gets_it(given_order):
    tr = tracker(given_order=given_order)
    first = step(tr, frame([0.0]))
    assert first["ids"].tolist() == [0] and first["born"].tolist() == [True] and first["oks"].tolist() == [0.0]
    r = step(tr, frame([0.5, 0.2], scores=[0.5, 0.9]))          # both within the track's reach; the second scores higher
    if given_order:                                             # the mutation: the first one given takes the track
        assert r["ids"].tolist() == [0, 1] and r["born"].tolist() == [False, True]
    else:
        assert r["ids"].tolist() == [1, 0] and r["born"].tolist() == [True, False]
        assert r["oks"][1] == pytest.approx(math.exp(-0.02), rel=1e-12) and r["oks"][0] == 0.0
        assert tr.streams[0].id.tolist() == [0, 1, -1, -1] and tr.streams[0].next_id == 2


def test_equal_scores_are_visited_in_the_order_given():
    tr = tracker()
    step(tr, frame([0.0]))
    r = step(tr, frame([0.5, 0.2], scores=[0.7, 0.7]))
    assert r["ids"].tolist() == [0, 1]


@pytest.mark.parametrize("unseen, same", [(2, True), (3, False)])
def test_a_track_survives_max_age_unseen_frames_and_no_more(unseen, same):
    tr = tracker(max_age=2)
    assert step(tr, frame([0.0]))["ids"].tolist() == [0]
    for n in range(unseen):
        r = step(tr, frame([]))
        assert r["ids"].size == 0
        assert tr.streams[0].age[0] == n + 1
    assert (tr.streams[0].id[0] == 0) == same
    r = step(tr, frame([0.1]))
    assert r["ids"].tolist() == [0 if same else 1] and r["born"].tolist() == [not same]
    assert r["events"]["reid"] == int(same) and tr.streams[0].age[0] == 0
    assert tr.streams[0].id.tolist() == [0 if same else 1, -1, -1, -1]          # the freed slot is the lowest free one


@pytest.mark.parametrize("births_first", [False, True])
def test_a_slot_freed_in_a_call_is_reused_by_a_birth_of_that_call(births_first):
    tr = tracker(max_age=0, max_tracks=1, births_first=births_first)
    step(tr, frame([0.0]))
    r = step(tr, frame([100.0]))                                # nobody continues track 0: it expires in this call
    assert r["events"]["expiry"] == 1
    if births_first:                                            # the mutation: the birth came too early for the slot
        assert r["ids"].tolist() == [-1] and tr.streams[0].overflow == 1 and tr.streams[0].id.tolist() == [-1]
    else:
        assert r["ids"].tolist() == [1] and r["born"].tolist() == [True] and tr.streams[0].overflow == 0
        assert tr.streams[0].id.tolist() == [1]


def test_overflow_gives_minus_one_and_counts():
    tr = tracker(max_tracks=1, max_age=5)
    r = step(tr, frame([0.0, 100.0, 200.0]))
    assert r["ids"].tolist() == [0, -1, -1] and r["born"].tolist() == [True, False, False]
    assert tr.streams[0].overflow == 2 and r["events"]["overflow"] == 2
    assert np.array_equal(r["keypoints"], frame([0.0, 100.0, 200.0])["kpts"])
    r = step(tr, frame([100.0, 0.3]))                           # the track goes on; the stranger still finds no slot
    assert r["ids"].tolist() == [-1, 0] and tr.streams[0].overflow == 3 and tr.streams[0].next_id == 1


def test_one_euro_sequence_of_four_samples_by_hand():
    """x = 0, 1, 1, 3 at t = 0.5, 1, 1.5, 2.5 with min_cutoff 1, beta 0.5, d_cutoff 1.
    Sample 1 initialises: xhat = 0, dxhat = 0.
    Sample 2, te = 0.5: a_d = pi / (pi + 1) = 0.758547; dx = 2, dxhat = 1.517094; fc = 1.758547, r = 5.524638,
      a = 0.846735; xhat = 0.846735.
    Sample 3, te = 0.5: dx = 0.306530, dxhat = 0.758547 * 0.306530 + 0.241453 * 1.517094 = 0.598825; fc = 1.299412,
      r = 4.082224, a = 0.803236; xhat = 0.803236 + 0.196764 * 0.846735 = 0.969843.
    Sample 4, te = 1: a_d = 2 pi / (2 pi + 1) = 0.862697; dx = 2.030157, dxhat = 1.751410 + 0.137303 * 0.598825 =
      1.833631; fc = 1.916816, r = 12.043709, a = 0.923335; xhat = 2.770004 + 0.076665 * 0.969843 = 2.844357."""
    smooth = (1.0, 0.5, 1.0)
    assert float(TR.alpha(0.5, 1.0)) == pytest.approx(math.pi / (math.pi + 1), rel=1e-15)
    tr = tracker(smooth=smooth, match_thr=0.0)
    want = [0.0, 0.8467347994101125, 0.9698428885458034, 2.84435736924633]
    want6 = [0.0, 0.846735, 0.969843, 2.844357]
    for x, t, w, w6 in zip([0.0, 1.0, 1.0, 3.0], [0.5, 1.0, 1.5, 2.5], want, want6):
        r = step(tr, frame([x]), t)
        assert r["ids"].tolist() == [0]
        assert r["keypoints"][0, 0, 0] == pytest.approx(w, rel=1e-14, abs=0.0)
        assert abs(r["keypoints"][0, 0, 0] - w6) < 1e-6
        assert r["keypoints"][0, 0, 1] == 0.0
    st = tr.streams[0]
    assert st.xhat[0, 0, 0] == r["keypoints"][0, 0, 0] and st.dxhat[0, 0, 0] == pytest.approx(1.833631493584759)
    assert st.kp[0, 0, 0] == 3.0 and st.t_last[0] == 2.5 and st.init[0, 0] == 1
    # without a filter the output is the input and no filter state is kept
    raw = tracker(smooth=None, match_thr=0.0)
    for x, t in zip([0.0, 1.0, 1.0, 3.0], [0.5, 1.0, 1.5, 2.5]):
        assert step(raw, frame([x]), t)["keypoints"][0, 0, 0] == x
    assert not raw.streams[0].init.any() and not raw.streams[0].xhat.any()


def test_default_times_come_from_fps_and_must_increase():
    tr = tracker(fps=20.0)
    step(tr, frame([0.0]))
    step(tr, frame([0.0]))
    assert tr.streams[0].t_last[0] == 2 / 20.0
    with pytest.raises(ValueError, match="t:"):
        step(tr, frame([0.0]), 0.1)


def test_match_needs_more_than_the_threshold():
    """OKS exactly at match_thr (0, by underflow) does not continue a track; the mutation >= does."""
    for ge, ids in ((False, [1]), (True, [0])):
        tr = tracker(match_thr=0.0, ge_match=ge)
        step(tr, frame([0.0]))
        r = step(tr, frame([100.0]))
        assert r["oks_seen"] == [0.0] and r["ids"].tolist() == ids


def test_the_areas_are_averaged():
    """A pose 1.5 from its track, areas 400 and 100: e = 2.25 / 0.01 / 250 / 2 = 0.45, OKS 0.6376 > 0.5; with the
    track's area alone e = 1.125, OKS 0.3247: no match."""
    for mutant, ids, oks in ((False, [0], math.exp(-0.45)), (True, [1], 0.0)):
        tr = tracker(match_thr=0.5, track_area=mutant)
        step(tr, frame([0.0], areas=[100.0]))
        r = step(tr, frame([1.5], areas=[400.0]))
        assert r["ids"].tolist() == ids and r["oks"][0] == pytest.approx(oks, rel=1e-12)
        assert r["oks_seen"][0] == pytest.approx(math.exp(-1.125 if mutant else -0.45), rel=1e-12)


def test_te_is_the_time_since_the_track_was_seen():
    """Uneven times, and one frame without the person: te = t - t_last = 0.25, not (age + 1) / fps = 2 / 30."""
    outs = []
    for mutant in (False, True):
        tr = tracker(smooth=(1.0, 0.0, 1.0), te_from_age=mutant, fps=30.0)
        step(tr, frame([0.0]), 0.1)
        step(tr, frame([]), 0.15)
        outs.append(step(tr, frame([1.0]), 0.35)["keypoints"][0, 0, 0])
    r = 2 * math.pi * 0.25
    assert outs[0] == pytest.approx(r / (r + 1), rel=1e-14)
    r = 2 * math.pi * (2 / 30.0)
    assert outs[1] == pytest.approx(r / (r + 1), rel=1e-14) and abs(outs[0] - outs[1]) > 0.3


def test_an_uncounted_keypoint_loses_its_filter_state():
    """Two keypoints, the second hidden in the second frame: in the third it starts afresh (raw output); the mutation
    filters it from the state of the first frame."""
    sig = np.array([0.05, 0.05])
    outs = []
    for mutant in (False, True):
        tr = tracker(sigmas=sig, smooth=(1.0, 0.0, 1.0), vis_thr=0.5, keep_uncounted=mutant)
        step(tr, frame([0.0], vis=[[0.9, 0.9]], K=2), 1.0)
        r = step(tr, frame([0.5], vis=[[0.9, 0.5]], K=2), 2.0)          # 0.5 is not above the threshold
        assert r["ids"].tolist() == [0] and r["keypoints"][0, 1, 0] == 0.5 and r["keypoints"][0, 0, 0] < 0.5
        assert tr.streams[0].init[0].tolist() == [1, 1 if mutant else 0]
        r = step(tr, frame([1.0], vis=[[0.9, 0.9]], K=2), 3.0)
        assert r["ids"].tolist() == [0] and r["events"]["reinit"] == (0 if mutant else 1)
        outs.append(r["keypoints"][0, 1, 0])
    assert outs[0] == 1.0 and outs[1] < 0.99


def test_streams_are_independent_and_reset_forgets():
    tr = tracker()
    r = tr.update({"a": frame([0.0, 50.0]), "b": frame([0.0])})
    assert r["a"]["ids"].tolist() == [0, 1] and r["b"]["ids"].tolist() == [0]
    tr.update({"a": frame([])})                                         # b is not named: it does not age
    assert tr.streams["a"].age[:2].tolist() == [1, 1] and tr.streams["b"].age[0] == 0
    tr.reset("a")
    r = tr.update({"a": frame([0.0]), "b": frame([0.1, 70.0])})
    assert r["a"]["ids"].tolist() == [0] and r["a"]["born"].tolist() == [True]
    assert r["b"]["ids"].tolist() == [0, 1] and r["b"]["born"].tolist() == [False, True]


def test_the_scenes_produce_every_event():
    """The seeded scenes of tests/test_track_gpu.py, on the gauge alone: matches, births, expiries and
    re-identifications in each; overflow in its scene only."""
    for K, T, P, vis_thr, kw in ((17, 16, 12, None, dict(leavers=2, entrants=2)), (1, 16, 12, None, {}),
                                 (17, 8, 20, None, {}), (17, 16, 12, 0.2, dict(duplicates=True))):
        frames, times, _ = TR.make_scene(5, K, 12, P, 2, **kw)
        tr = TR.Tracker(PR.default_sigmas(K), 0.3, 2, T, vis_thr, (1.0, 0.05, 1.0))
        events, n = {}, 0
        for f, t in zip(frames, times):
            r = step(tr, f, t)
            n += r["ids"].size
            for k, v in r["events"].items():
                events[k] = events.get(k, 0) + v
        assert events["match"] >= 0.2 * n and events["birth"] and events["expiry"] and events["reid"], events
        assert (events["overflow"] > 0) == (P > T) and (events["reinit"] > 0) == (vis_thr is not None)
