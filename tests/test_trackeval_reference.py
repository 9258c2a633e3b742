"""CPU tests of the gauge of PoseTrackEval (tests/trackeval_reference.py): hand-computed scenes whose counts are written
out here, a scene on which only the continuation bonus keeps an identity, each planted switch shown to change a count,
and, on random small scenes, every frame's total weight and every IDTP against scipy's assignment solver on the same
integer matrix (exact: every total is below 2^53)."""
import math

import numpy as np
import pytest

from tests import trackeval_reference as R
from tests.cocoeval_reference import default_sigmas

K = 3
SIG = np.full(K, 0.05)


def _one(frames, thresholds=(0.5,), **switches):
    res = R.evaluate({"s": frames}, SIG, thresholds, **switches)
    return res["metrics"][0], res


def test_a_perfect_tracker_scores_one():
    frames = R.scene(K, [dict(gt=7, pred=70, at=(0, 0)), dict(gt=3, pred=30, at=(300, 0))], 5)
    m, _ = _one(frames)
    assert {k: m[k] for k in R.INT_KEYS} == dict(TP=10, FN=0, FP=0, IDSW=0, MT=2, PT=0, ML=0, Frag=0, IDTP=10, IDFN=0,
                                                 IDFP=0)
    assert m["MOTA"] == 1.0 and m["IDF1"] == 1.0 and m["IDP"] == 1.0 and m["IDR"] == 1.0 and m["MOTP"] == 1.0


def test_two_people_whose_ids_swap_once():
    # 7 frames; the tracker's ids 1 and 2 trade places from frame 4 on
    a = {f: (1 if f < 4 else 2) for f in range(7)}
    b = {f: (2 if f < 4 else 1) for f in range(7)}
    frames = R.scene(K, [dict(gt=10, pred=a, at=(0, 0)), dict(gt=20, pred=b, at=(300, 0))], 7)
    m, res = _one(frames)
    # every instance is matched: TP 14.  Both people change their predicted identity once: IDSW 2.
    # c = [[4, 3], [3, 4]]: IDTP 8, IDFN = IDFP = 14 - 8 = 6, IDF1 = 16 / (16 + 12) = 4 / 7, MOTA = 1 - 2 / 14
    assert res["details"]["s"][0]["identity"]["c"] == [[4, 3], [3, 4]]
    assert {k: m[k] for k in R.INT_KEYS} == dict(TP=14, FN=0, FP=0, IDSW=2, MT=2, PT=0, ML=0, Frag=0, IDTP=8, IDFN=6,
                                                 IDFP=6)
    assert m["IDF1"] == 16 / 28 and m["MOTA"] == 1 - 2 / 14 and m["IDP"] == 8 / 14 and m["IDR"] == 8 / 14


def test_a_gap_of_one_frame_then_another_id():
    m, _ = _one(R.scene(K, R.ONE_FRAME_GAP, 5))
    # matched in 4 of 5 frames (5 * 4 > 4 * 5 is false: PT), two runs: Frag 1; last = 1 when 2 arrives: IDSW 1
    # c = [[2, 2]]: IDTP 2, IDFN = 5 - 2, IDFP = 4 - 2
    assert {k: m[k] for k in R.INT_KEYS} == dict(TP=4, FN=1, FP=0, IDSW=1, MT=0, PT=1, ML=0, Frag=1, IDTP=2, IDFN=3,
                                                 IDFP=2)
    assert m["MOTA"] == 1 - 2 / 5 and m["IDF1"] == 4 / 9
    # judged against prev (none after the gap) the change of identity goes unseen
    assert _one(R.scene(K, R.ONE_FRAME_GAP, 5), switch_from_prev=True)[0]["IDSW"] == 0


def test_the_continued_pair_is_kept_at_the_lower_oks():
    frames = R.continued_pair_frames(K)
    s = R.frame_oks(frames[1], SIG)
    assert 0.5 + 1e-3 < s[0, 0] < s[0, 1] - 1e-3 and 0.5 + 1e-3 < s[1, 1] < s[1, 0] - 1e-3
    s0 = R.frame_oks(frames[0], SIG)
    assert s0[0, 0] == 1.0 and s0[1, 1] == 1.0 and s0[0, 1] < 0.4 and s0[1, 0] < 0.4
    m, res = _one(frames)
    assert (m["TP"], m["IDSW"]) == (4, 0) and res["details"]["s"][0]["clear"]["frames"][1]["slots"] == [0, 1]
    assert res["details"]["s"][0]["clear"]["frames"][1]["total"] > 2 * R.BONUS
    m, res = _one(frames, no_bonus=True)
    assert (m["TP"], m["IDSW"]) == (4, 2) and res["details"]["s"][0]["clear"]["frames"][1]["slots"] == [1, 0]


def test_equal_to_the_threshold_is_admissible():
    frames = R.scene(K, [dict(gt=1, pred=1, at=(0, 0))], 3)
    assert _one(frames, thresholds=(1.0,))[0]["TP"] == 3
    m = _one(frames, thresholds=(1.0,), gt=True)[0]
    assert (m["TP"], m["FN"], m["FP"], m["IDTP"]) == (0, 3, 3, 0)
    assert math.isnan(m["MOTP"]) and m["MOTA"] == -1.0 and m["IDF1"] == 0.0


def test_runs_are_counted_over_the_frames_of_the_sequence():
    # the person (and the prediction) are away in frame 2; a bystander keeps the sequence going
    tracks = [dict(gt=1, pred=1, at=(0, 0), frames=(0, 1, 3, 4)), dict(gt=2, pred=2, at=(300, 0))]
    m, res = _one(R.scene(K, tracks, 5))
    assert res["details"]["s"][0]["clear"]["runs"] == {1: 2, 2: 1} and (m["Frag"], m["MT"], m["IDSW"]) == (1, 2, 0)
    assert _one(R.scene(K, tracks, 5), runs_over_present=True)[0]["Frag"] == 0


def test_ratios_without_a_denominator_are_nan():
    m, _ = _one([R.make_frame(K=K), R.make_frame(K=K)])
    assert all(m[k] == 0 for k in R.INT_KEYS) and all(math.isnan(m[k]) for k in R.RATIO_KEYS)
    # predictions only: MOTA has no ground truth, IDP is 0 / FP
    m, _ = _one([R.cloud_frame(K, (), (0.0,), (), (4,))])
    assert (m["FP"], m["IDFP"]) == (1, 1) and math.isnan(m["MOTA"]) and math.isnan(m["IDR"]) and m["IDP"] == 0.0
    assert m["IDF1"] == 0.0


def test_mostly_tracked_and_mostly_lost_thresholds():
    # 10 frames: matched in 9 (MT: 45 > 40), in 8 (PT: 40 > 40 is false), in 2 (PT: 10 < 10 is false), in 1 (ML)
    def seen(n):
        return {f: 1 for f in range(n)}
    for n, want in ((9, "MT"), (8, "PT"), (2, "PT"), (1, "ML")):
        m, _ = _one(R.scene(K, [dict(gt=1, pred=seen(n), at=(0, 0))], 10))
        assert {k: m[k] for k in ("MT", "PT", "ML")} == {k: int(k == want) for k in ("MT", "PT", "ML")}, n


@pytest.mark.parametrize("seed", range(6))
def test_random_scenes_against_scipy(seed):
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(seed)
    k = int(rng.choice([1, 3, 17]))
    sig = default_sigmas(k)
    # "b" is crowded: neighbours are admissible for one another and the assignment has to choose
    seqs = {n: R.random_sequence(rng, k, int(rng.integers(1, 9)), int(rng.integers(1, 7)), extent=extent)
            for n, extent in (("a", 600.0), ("b", 40.0))}
    thresholds = (0.3, 0.5, 0.75)
    res = R.evaluate(seqs, sig, thresholds)
    assert R.min_threshold_gap(res) > 1e-9

    def best(q):
        q = np.asarray(q, dtype=np.float64)
        if q.size == 0:
            return 0
        r, c = linear_sum_assignment(q, maximize=True)
        return int(q[r, c].sum())

    checked = matched = 0
    for name in seqs:
        for t in range(len(thresholds)):
            d = res["details"][name][t]
            for fr in d["clear"]["frames"]:
                assert fr["total"] < 2 ** 53 and fr["total"] == best(fr["q"])
                checked += 1
                matched += sum(j >= 0 for j in fr["slots"])
            assert d["identity"]["IDTP"] == best(d["identity"]["c"])
            rec = res["per_sequence"][name][t]
            assert rec["TP"] + rec["FN"] == rec["IDTP"] + rec["IDFN"]       # both count the ground-truth instances
            assert rec["TP"] + rec["FP"] == rec["IDTP"] + rec["IDFP"]
            assert rec["MT"] + rec["PT"] + rec["ML"] == len(d["clear"]["present"])
    assert checked and matched
    for t in range(len(thresholds)):
        for key in R.INT_KEYS:
            assert res["metrics"][t][key] == sum(res["per_sequence"][n][t][key] for n in seqs)


def test_the_last_identity_matters_on_random_scenes():
    """switch_from_prev also loses switches on drawn scenes, not only on the hand-made one above: the drawn tracker
    misses people for a frame and comes back with another id."""
    rng = np.random.default_rng(11)
    seqs = {n: R.random_sequence(rng, 3, 12, 5, switch_p=0.2, miss_p=0.25) for n in range(4)}
    rule = R.evaluate(seqs, SIG, (0.5,))["metrics"][0]
    other = R.evaluate(seqs, SIG, (0.5,), switch_from_prev=True)["metrics"][0]
    assert other["IDSW"] < rule["IDSW"] and all(other[k] == rule[k] for k in R.INT_KEYS if k != "IDSW")
