"""The HOTA gauge (tests/hota_reference.py) on hand-computed scenes, against each of its planted faults, and against an
independent float restatement of the paper that uses scipy's assignment.  CPU only.

Scene ONE.  One annotated track over 4 frames, perfectly localised (s = 1); it carries predicted id 1 in frames 0 - 1
and id 2 in frames 2 - 3.  Every frame: R = C = 1, x = 1 / (2 - 1) = 1.  pmc[g][1] = pmc[g][2] = 2, ng = 4, np = 2:
A = 2 / (4 + 2 - 2) = 0.5 for both.  Every frame matches its only pair; at every alpha TP = 4, FN = FP = 0, loc = 4,
mc = 2 and 2: assA = 2 * 4 / (4 + 2 - 2) = 2, assRe = 2 * 4 / 4 = 2, assPr = 2 * 4 / 2 = 4.  DetA = 1, AssA = 2 / 4 =
0.5, AssRe = 0.5, AssPr = 1, LocA = 1, HOTA = sqrt(0.5).

Scene TWO, alphas 0.25, 0.5, 0.75.  Ground truths 1 and 2, predictions 7, 8 and 9; OKS rows are ground truths:
  frame 0   gt 1, 2   pred 7, 8   s = [[0, 0], [0.4, 0.8]]
  frame 1   gt 1, 2   pred 7, 8   s = 0: two misses, two false positives
  frame 2   gt 1, 2   pred 7, 8   s = [[0.8, 0], [0.6, 0]]
  frame 3   gt 1      no prediction: a miss
  frame 4   no ground truth, pred 9: a stray
ng[1] = 4, ng[2] = 3; np[7] = np[8] = 3, np[9] = 1; 7 annotated and 7 predicted instances.
Step 1.  Frame 0: R_2 = 1.2, C_7 = 0.4, C_8 = 0.8: x(2,7) = 0.4 / (1.2 + 0.4 - 0.4) = 1/3, x(2,8) = 0.8 / (1.2 + 0.8 -
0.8) = 2/3.  Frame 2: R_1 = 0.8, R_2 = 0.6, C_7 = 1.4: x(1,7) = 0.8 / 1.4 = 4/7, x(2,7) = 0.6 / 1.4 = 3/7.  In units of
2^32: pmc[1][7] = 4/7, pmc[2][7] = 1/3 + 3/7 = 16/21, pmc[2][8] = 2/3.
Step 2.  A[1][7] = (4/7) / (7 - 4/7) = 4/45, A[2][7] = (16/21) / (6 - 16/21) = 8/55, A[2][8] = (2/3) / (6 - 2/3) = 1/8.
Step 3.  Frame 0, ground truth 2: A s = 8/55 * 0.4 = 0.058 with 7, 1/8 * 0.8 = 0.1 with 8: it takes 8 (s = 0.8).
Frame 2, prediction 7: 4/45 * 0.8 = 0.071 with 1, 8/55 * 0.6 = 0.087 with 2: it goes to 2 (s = 0.6) and 1 is missed,
though s alone would have given it to 1.
Steps 4 - 6.  alpha 0.25 and 0.5: both pairs count.  TP = 2, FN = FP = 5, loc = 1.4, mc[2][8] = mc[2][7] = 1: assA =
1 / (3 + 3 - 1) + 1 / (3 + 3 - 1) = 0.4, assRe = assPr = 1/3 + 1/3.  DetA = 2 / 12, DetRe = DetPr = 2 / 7, AssA = 0.2,
AssRe = AssPr = 1/3, LocA = 0.7, HOTA = sqrt(1 / 30).  alpha 0.75: only (2, 8).  TP = 1, FN = FP = 6, loc = 0.8, assA =
0.2, assRe = assPr = 1/3; DetA = 1 / 13, AssA = 0.2, LocA = 0.8, HOTA = sqrt(1 / 65).

What each fault does to scene TWO:
  match_on_s          frame 2 gives prediction 7 to ground truth 1 (0.8 > 0.6): loc = 1.6 at 0.25, TP = 2 at 0.75
  hard_pmc            pmc = 1, 2, 1: A[2][7] = 2 / (6 - 2) = 1/2, A[2][8] = 1 / (6 - 1) = 1/5; frame 0: 1/2 * 0.4 = 0.2 >
                      1/5 * 0.8 = 0.16, ground truth 2 takes 7 (s = 0.4): loc = 1.0 at 0.25, TP = 1 at 0.5, 0 at 0.75
  no_col_sum          x = s / R_g: pmc[2][7] = 1/3 + 1 = 4/3, A[2][7] = (4/3) / (6 - 4/3) = 2/7; frame 0: 2/7 * 0.4 =
                      0.114 > 0.1: ground truth 2 takes 7 again
  assa_no_minus_m     assA = 1/6 + 1/6 at 0.25 (and 8 / 6 instead of 2 on scene ONE)
  per_alpha_matching  at 0.75 the pair (2, 7) of frame 2 is struck out before the matching, so 7 goes to ground truth 1
                      (s = 0.8): TP = 2 at 0.75
"""
import math

import numpy as np
import pytest

from tests import hota_reference as H
from tests.trackeval_reference import make_frame

FAULTS = ("match_on_s", "hard_pmc", "no_col_sum", "assa_no_minus_m", "per_alpha_matching")
THIRD = 1.0 / 3.0


def scene(spec):
    """[(gt ids, pred ids, OKS rows)] -> (sequences, oks) of one sequence "s"."""
    frames = [make_frame(g, pred_ids=p, K=1) for g, p, _ in spec]
    return {"s": frames}, {"s": [np.asarray(m, dtype=np.float64).reshape(len(g), len(p)) for g, p, m in spec]}


ONE = [([5], [1], [[1.0]]), ([5], [1], [[1.0]]), ([5], [2], [[1.0]]), ([5], [2], [[1.0]])]
TWO = [([1, 2], [7, 8], [[0.0, 0.0], [0.4, 0.8]]), ([1, 2], [7, 8], [[0.0, 0.0], [0.0, 0.0]]),
       ([1, 2], [7, 8], [[0.8, 0.0], [0.6, 0.0]]), ([1], [], []), ([], [9], [])]
TWO_ALPHAS = (0.25, 0.5, 0.75)


def _close(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * max(abs(w), 1e-300), (got, want)


def test_scene_one_by_hand():
    seqs, oks = scene(ONE)
    r = H.evaluate(seqs, oks=oks)
    h, rec, d = r["hota"], r["per_sequence_hota"]["s"], r["details"]["s"]
    n = len(H.DEFAULT_ALPHAS)
    assert n == 19 and h["alphas"] == [i / 20.0 for i in range(1, 20)]
    assert d["pmc"] == [[2 << 32, 2 << 32]] and d["ng"] == [4] and d["np"] == [2, 2]
    assert d["q"] == [[[1 + (1 << 31)]]] * 4 and d["held"] == [[0]] * 4
    assert h["TP"] == [4] * n and h["FN"] == [0] * n and h["FP"] == [0] * n
    assert rec["loc_sum"] == [4.0] * n and rec["assa_sum"] == [2.0] * n
    assert rec["assre_sum"] == [2.0] * n and rec["asspr_sum"] == [4.0] * n
    for k, v in (("DetA", 1.0), ("AssA", 0.5), ("HOTA", math.sqrt(0.5)), ("LocA", 1.0), ("DetRe", 1.0),
                 ("DetPr", 1.0), ("AssRe", 0.5), ("AssPr", 1.0)):
        assert h["curves"][k] == [v] * n and h[k] == pytest.approx(v, abs=1e-15), k


def test_scene_two_by_hand():
    seqs, oks = scene(TWO)
    r = H.evaluate(seqs, oks=oks, alphas=TWO_ALPHAS)
    h, rec, d = r["hota"], r["per_sequence_hota"]["s"], r["details"]["s"]
    assert d["ng"] == [4, 3] and d["np"] == [3, 3, 1]
    want_pmc = [[4 / 7, 0, 0], [16 / 21, 2 / 3, 0]]
    for a in range(2):
        for b in range(3):                                   # each of at most two floors loses less than one unit
            assert 0 <= want_pmc[a][b] * 2 ** 32 - d["pmc"][a][b] < 2.001, (a, b)
    assert d["held"] == [[-1, 1], [-1, -1], [1, -1], [], [-1]]
    assert h["TP"] == [2, 2, 1] and h["FN"] == [5, 5, 6] and h["FP"] == [5, 5, 6]
    _close(rec["loc_sum"], [1.4, 1.4, 0.8])
    _close(rec["assa_sum"], [0.4, 0.4, 0.2])
    _close(rec["assre_sum"], [2 * THIRD, 2 * THIRD, THIRD])
    _close(rec["asspr_sum"], [2 * THIRD, 2 * THIRD, THIRD])
    assert d["mc"][0] == [[0, 0, 0], [1, 1, 0]] and d["mc"][2] == [[0, 0, 0], [0, 1, 0]]
    c = h["curves"]
    _close(c["DetA"], [2 / 12, 2 / 12, 1 / 13])
    _close(c["DetRe"], [2 / 7, 2 / 7, 1 / 7])
    _close(c["DetPr"], [2 / 7, 2 / 7, 1 / 7])
    _close(c["AssA"], [0.2, 0.2, 0.2])
    _close(c["AssRe"], [THIRD] * 3)
    _close(c["AssPr"], [THIRD] * 3)
    _close(c["LocA"], [0.7, 0.7, 0.8])
    _close(c["HOTA"], [math.sqrt(1 / 30), math.sqrt(1 / 30), math.sqrt(1 / 65)])
    _close([h["HOTA"]], [(2 * math.sqrt(1 / 30) + math.sqrt(1 / 65)) / 3])
    # above every OKS of the scene nothing is left: the ratios are 0, LocA is 1
    top = H.evaluate(seqs, oks=oks, alphas=(0.9,))["hota"]
    assert top["TP"] == [0] and top["FN"] == [7] and top["FP"] == [7]
    assert all(top[k] == 0.0 for k in H.CURVES if k != "LocA") and top["LocA"] == 1.0


@pytest.mark.parametrize("fault", FAULTS)
def test_every_planted_fault_changes_a_number(fault):
    seqs, oks = scene(TWO)
    rule = H.evaluate(seqs, oks=oks, alphas=TWO_ALPHAS)["per_sequence_hota"]["s"]
    bad = H.evaluate(seqs, oks=oks, alphas=TWO_ALPHAS, **{fault: True})["per_sequence_hota"]["s"]
    assert bad != rule
    if fault == "match_on_s":
        assert bad["TP"] == [2, 2, 2] and bad["loc_sum"][0] == pytest.approx(1.6)
    elif fault in ("hard_pmc", "no_col_sum"):
        assert bad["TP"] == [2, 1, 0] and bad["loc_sum"][0] == pytest.approx(1.0)
    elif fault == "assa_no_minus_m":
        assert bad["TP"] == rule["TP"] and bad["assa_sum"][0] == pytest.approx(THIRD)
        seqs, oks = scene(ONE)
        assert H.evaluate(seqs, oks=oks, assa_no_minus_m=True)["per_sequence_hota"]["s"]["assa_sum"][0] == \
            pytest.approx(8 / 6)
    else:
        assert bad["TP"] == [2, 2, 2] and bad["loc_sum"][:2] == rule["loc_sum"][:2]


# ------------------------------------------------------------------------------------------------ the paper, in floats
def paper_hota(frames, oks, alphas):
    """HOTA as the paper gives it, float64 throughout, the per-frame assignment by scipy on A * s.  Returns the record
    of hota_reference.hota_sequence (without details) and the smallest lead of a frame's optimum over every matching
    that lacks one of its pairs."""
    from scipy.optimize import linear_sum_assignment
    gids = sorted({int(g) for f in frames for g in f["gt_ids"]})
    pids = sorted({int(p) for f in frames for p in f["pred_ids"]})
    gi, pi = {g: i for i, g in enumerate(gids)}, {p: i for i, p in enumerate(pids)}
    pot = np.zeros((len(gids), len(pids)))
    ng, npr = np.zeros(len(gids)), np.zeros(len(pids))
    clean = [np.where(s > 0, s, 0.0) for s in oks]
    for f, s in zip(frames, clean):
        rows, cols = [gi[int(g)] for g in f["gt_ids"]], [pi[int(p)] for p in f["pred_ids"]]
        ng[rows] += 1
        npr[cols] += 1
        if s.size:
            den = s.sum(axis=1, keepdims=True) + s.sum(axis=0, keepdims=True) - s
            pot[np.ix_(rows, cols)] += np.divide(s, den, out=np.zeros_like(s), where=s > 0)
    align = pot / (ng[:, None] + npr[None, :] - pot)
    n = len(alphas)
    counts = np.zeros((n, len(gids), len(pids)))
    tp, loc, lead = [0] * n, [0.0] * n, float("inf")
    for f, s in zip(frames, clean):
        if not s.size:
            continue
        rows, cols = [gi[int(g)] for g in f["gt_ids"]], [pi[int(p)] for p in f["pred_ids"]]
        score = align[np.ix_(rows, cols)] * s
        r, c = linear_sum_assignment(score, maximize=True)
        best = score[r, c].sum()
        for i, j in zip(r, c):
            if s[i, j] > 0:
                without = score.copy()
                without[i, j] = 0.0
                r2, c2 = linear_sum_assignment(without, maximize=True)
                lead = min(lead, best - without[r2, c2].sum())
                for k, alpha in enumerate(alphas):
                    if s[i, j] >= alpha:
                        tp[k] += 1
                        loc[k] += s[i, j]
                        counts[k, rows[i], cols[j]] += 1
    n_gt, n_pred = sum(len(f["gt_ids"]) for f in frames), sum(len(f["pred_ids"]) for f in frames)
    either = ng[:, None] + npr[None, :]
    return dict(TP=tp, FN=[n_gt - t for t in tp], FP=[n_pred - t for t in tp], loc_sum=loc,
                assa_sum=[float((m * m / (either - m)).sum()) for m in counts],
                assre_sum=[float((m * m / ng[:, None]).sum()) for m in counts],
                asspr_sum=[float((m * m / npr[None, :]).sum()) for m in counts]), lead


def drawn_sequence(rng, n_frames, n_gt, n_pred):
    """Similarities drawn directly: persistent ids, about a third of the pairs at 0, people coming and going."""
    frames, oks = [], []
    for _ in range(n_frames):
        g = sorted(rng.choice(n_gt, size=int(rng.integers(0, n_gt + 1)), replace=False) + 100)
        p = sorted(rng.choice(n_pred, size=int(rng.integers(0, n_pred + 1)), replace=False) + 900)
        s = rng.uniform(0.02, 1.0, (len(g), len(p))) * (rng.random((len(g), len(p))) > 0.35)
        frames.append(make_frame(g, pred_ids=p, K=1))
        oks.append(s)
    return frames, oks


def test_the_gauge_equals_the_paper_in_floats():
    """Where every frame's optimum leads by more than 1e-6 (the quantisation moves a matching's total by less than
    2^-23 = 1.2e-7, so two totals by less than 2.4e-7), the integer rule and the float rule pick the same pairs."""
    rng = np.random.default_rng(11)
    alphas = H.DEFAULT_ALPHAS
    seqs, oks, ref = {}, {}, {}
    while len(seqs) < 6:
        frames, mats = drawn_sequence(rng, int(rng.integers(3, 9)), int(rng.integers(1, 6)), int(rng.integers(1, 7)))
        rec, lead = paper_hota(frames, mats, alphas)
        if lead > 1e-6:                                     # the margin: asserted by construction, and again below
            name = len(seqs)
            seqs[name], oks[name], ref[name] = frames, mats, (rec, lead)
    got = H.evaluate(seqs, oks=oks, alphas=alphas)
    assert sum(got["hota"]["TP"]) > 50
    for name, (rec, lead) in ref.items():
        assert lead > 1e-6
        mine = got["per_sequence_hota"][name]
        for k in ("TP", "FN", "FP"):
            assert mine[k] == rec[k], (name, k)
        for k in H.SUM_KEYS:
            for a, b in zip(mine[k], rec[k]):
                assert abs(a - b) <= 1e-9 * max(abs(b), 1.0), (name, k)
    paper = H.finish([rec for rec, _ in ref.values()], alphas)
    for k in H.CURVES:
        assert abs(got["hota"][k] - paper[k]) <= 1e-9, k
        for a, b in zip(got["hota"]["curves"][k], paper["curves"][k]):
            assert abs(a - b) <= 1e-9, k
    assert 0.0 < got["hota"]["HOTA"] < 1.0


def test_nan_and_zero_count_as_nothing():
    spec = [([1, 2], [7, 8], [[0.9, float("nan")], [0.0, 0.5]])]
    seqs, oks = scene(spec)
    r = H.evaluate(seqs, oks=oks, alphas=(0.5, 0.9))
    assert r["details"]["s"]["pmc"] == [[1 << 32, 0], [0, 1 << 32]] and r["details"]["s"]["held"] == [[0, 1]]
    assert r["hota"]["TP"] == [2, 1]                        # an OKS equal to an alpha counts
    assert H.min_alpha_gap(r) == 0.0


def test_a_sequence_may_have_two_to_the_twenty_frames():
    with pytest.raises(ValueError, match="1048577 frames, more than 1048576"):
        H.hota_sequence([None] * (H.MAX_FRAMES + 1), [None] * (H.MAX_FRAMES + 1))
