"""The gauge of PoseTrackEval(hota=True): HOTA (Luiten et al., IJCV 2021) with OKS as the similarity, restated in plain
loops on Python ints and numpy float64.  Written from the rule (include/probpose_hip.h), not from the
kernels and not from any evaluation package.

  potential(frames, oks) -> pmc, ng, np, gpos, ppos    step 1: the soft-Jaccard potential matches and the presences
  alignment(pmc, ng_a, np_b) -> A                      step 2
  frame_weights(frame, s, ...) -> q [G][D]             step 3's integer weights
  hota_sequence(frames, oks, alphas) -> record         steps 1 - 5 for one sequence: TP FN FP loc_sum assa_sum assre_sum
                                                       asspr_sum (lists per alpha) and the details (pmc, q, slots, mc)
  finish(records, alphas) -> dict                      step 6: what ``res["hota"]`` holds
  evaluate(sequences, sigmas, alphas, oks=None)        {"hota", "per_sequence_hota", "details"}

Frames and sequences are those of tests/trackeval_reference.py; ``oks`` (name -> list of [G, D] float64 matrices) stands
in for frame_oks where a test draws the similarities itself.  The solver is tests/trackopt_reference.solve, imported.

The rule.  s[g][d] is the frame's OKS; an s that is not > 0 (a NaN is not) counts as 0 everywhere.  Every float step is
one IEEE float64 operation.
 1. Per frame R_g = sum_d s[g][d], C_d = sum_g s[g][d], sequential from 0.0 in ascending index.  For every pair with
    s > 0: x = s / ((R_g + C_d) - s), pmc[a][b] += floor(x * 2^32), a and b the identities of g and d (dense, in order
    of first appearance).  ng[a], np[b]: the frames an identity appears in.
 2. A[a][b] = float64(pmc) / float64(2^32 (ng[a] + np[b]) - pmc), the denominator an integer.
 3. q[g][d] = 0 unless s > 0, else 1 + floor((A * s) * 2^32); slots = solve(q): one matching per frame for all alphas.
 4. Per alpha: a matched pair counts iff s >= alpha; TP, FN = ground-truth instances - TP, FP = predicted instances -
    TP, loc = the sum of s over the counted pairs, mc[a][b] += 1.
 5. Per alpha over the entries m of mc: assA = sum m m / (ng + np - m), assRe = sum m m / ng, assPr = sum m m / np.
 6. Summed over the sequences: DetA = TP / (TP + FN + FP), DetRe = TP / (TP + FN), DetPr = TP / (TP + FP), AssA = assA /
    TP, AssRe = assRe / TP, AssPr = assPr / TP, LocA = loc / TP, HOTA = sqrt(DetA AssA); a ratio whose denominator is 0
    is 0, LocA is then 1.  The headline numbers are the means over the alphas.

The switches (``match_on_s``, ``hard_pmc``, ``no_col_sum``, ``assa_no_minus_m``, ``per_alpha_matching``) are planted
faults: tests/test_hota_reference.py shows that the gauge tells the rule from each of them; their defaults are the rule.
"""
import math

import numpy as np

from tests.trackeval_reference import frame_oks
from tests.trackopt_reference import solve

SCALE = np.float64(2.0 ** 32)
ONE = 1 << 32
MAX_FRAMES = 1 << 20
DEFAULT_ALPHAS = tuple(i / 20.0 for i in range(1, 20))
CURVES = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")
SUM_KEYS = ("loc_sum", "assa_sum", "assre_sum", "asspr_sum")


def sim(s):
    """An OKS as the rule reads it: float64, 0 for whatever is not > 0."""
    s = np.float64(s)
    return s if s > 0 else np.float64(0.0)


def potential(frames, oks, hard_pmc=False, no_col_sum=False):
    """-> pmc [NG][NP] ints, ng [NG], np [NP], gpos, ppos (id -> dense index in order of first appearance)."""
    gpos, ppos = {}, {}
    for frame in frames:
        for g in frame["gt_ids"]:
            gpos.setdefault(int(g), len(gpos))
        for p in frame["pred_ids"]:
            ppos.setdefault(int(p), len(ppos))
    pmc = [[0] * len(ppos) for _ in range(len(gpos))]
    ng, npr = [0] * len(gpos), [0] * len(ppos)
    for frame, s in zip(frames, oks):
        gids, pids = [int(g) for g in frame["gt_ids"]], [int(p) for p in frame["pred_ids"]]
        G, D = len(gids), len(pids)
        for g in gids:
            ng[gpos[g]] += 1
        for p in pids:
            npr[ppos[p]] += 1
        R, C = [np.float64(0.0)] * G, [np.float64(0.0)] * D
        clean = [[sim(s[i, j]) for j in range(D)] for i in range(G)]
        for i in range(G):
            for j in range(D):
                R[i] = R[i] + clean[i][j]
        for j in range(D):
            for i in range(G):
                C[j] = C[j] + clean[i][j]
        for i in range(G):
            for j in range(D):
                v = clean[i][j]
                if v > 0:
                    if hard_pmc:
                        w = ONE
                    else:
                        x = v / R[i] if no_col_sum else v / ((R[i] + C[j]) - v)
                        w = int(np.floor(x * SCALE))
                    pmc[gpos[gids[i]]][ppos[pids[j]]] += w
    return pmc, ng, npr, gpos, ppos


def alignment(pmc, ng_a, np_b):
    den = ONE * (ng_a + np_b) - pmc
    return np.float64(pmc) / np.float64(den) if den > 0 else np.float64(0.0)


def frame_weights(frame, s, pmc, ng, npr, gpos, ppos, match_on_s=False):
    G, D = len(frame["gt_ids"]), len(frame["pred_ids"])
    q = [[0] * D for _ in range(G)]
    for i in range(G):
        a = gpos[int(frame["gt_ids"][i])]
        for j in range(D):
            b = ppos[int(frame["pred_ids"][j])]
            v = sim(s[i, j])
            if v > 0:
                A = np.float64(1.0) if match_on_s else alignment(pmc[a][b], ng[a], npr[b])
                q[i][j] = 1 + int(np.floor((A * v) * SCALE))
    return q


def hota_sequence(frames, oks, alphas=DEFAULT_ALPHAS, match_on_s=False, hard_pmc=False, no_col_sum=False,
                  assa_no_minus_m=False, per_alpha_matching=False):
    if len(frames) > MAX_FRAMES:
        raise ValueError(f"a sequence has {len(frames)} frames, more than {MAX_FRAMES}")
    alphas = [np.float64(a) for a in alphas]
    n = len(alphas)
    pmc, ng, npr, gpos, ppos = potential(frames, oks, hard_pmc=hard_pmc, no_col_sum=no_col_sum)
    NG, NP = len(gpos), len(ppos)
    mc = [[[0] * NP for _ in range(NG)] for _ in range(n)]
    tp, loc = [0] * n, [np.float64(0.0)] * n
    n_gt = n_pred = 0
    qs, held, steps = [], [], 0
    for frame, s in zip(frames, oks):
        G, D = len(frame["gt_ids"]), len(frame["pred_ids"])
        n_gt, n_pred = n_gt + G, n_pred + D
        q = frame_weights(frame, s, pmc, ng, npr, gpos, ppos, match_on_s=match_on_s)
        slots, st = solve(q) if G and D else ([-1] * G, 0)
        steps += st
        qs.append(q)
        row_of = [-1] * D                                   # per prediction the row it is matched to
        for i, j in enumerate(slots):
            if j >= 0:
                row_of[j] = i
        held.append(row_of)
        for k, alpha in enumerate(alphas):
            if per_alpha_matching and G and D:              # the fault: pairs below alpha leave the matching
                qa = [[q[i][j] if sim(s[i, j]) >= alpha else 0 for j in range(D)] for i in range(G)]
                use = solve(qa)[0]
            else:
                use = slots
            for i, j in enumerate(use):
                if j >= 0 and sim(s[i, j]) >= alpha:
                    tp[k] += 1
                    loc[k] = loc[k] + sim(s[i, j])
                    mc[k][gpos[int(frame["gt_ids"][i])]][ppos[int(frame["pred_ids"][j])]] += 1
    assa, assre, asspr = [np.float64(0.0)] * n, [np.float64(0.0)] * n, [np.float64(0.0)] * n
    for k in range(n):
        for a in range(NG):
            for b in range(NP):
                m = mc[k][a][b]
                if m > 0:
                    mm = np.float64(m * m)
                    assa[k] = assa[k] + mm / np.float64(ng[a] + npr[b] - (0 if assa_no_minus_m else m))
                    assre[k] = assre[k] + mm / np.float64(ng[a])
                    asspr[k] = asspr[k] + mm / np.float64(npr[b])
    return dict(TP=tp, FN=[n_gt - t for t in tp], FP=[n_pred - t for t in tp], loc_sum=[float(x) for x in loc],
                assa_sum=[float(x) for x in assa], assre_sum=[float(x) for x in assre],
                asspr_sum=[float(x) for x in asspr],
                details=dict(pmc=pmc, ng=ng, np=npr, q=qs, held=held, mc=mc, steps=steps))


def _ratio(num, den, empty=0.0):
    return float(np.float64(num) / np.float64(den)) if den else empty


def finish(records, alphas):
    """records: the per-sequence dicts -> what ``res["hota"]`` holds."""
    alphas = [float(a) for a in alphas]
    n = len(alphas)
    tot = {k: [sum(r[k][i] for r in records) for i in range(n)] for k in ("TP", "FN", "FP")}
    for k in SUM_KEYS:
        tot[k] = [float(sum(np.float64(r[k][i]) for r in records)) for i in range(n)]
    curves = {k: [] for k in CURVES}
    for i in range(n):
        tp, fn, fp = tot["TP"][i], tot["FN"][i], tot["FP"][i]
        det_a, ass_a = _ratio(tp, tp + fn + fp), _ratio(tot["assa_sum"][i], tp)
        curves["DetA"].append(det_a)
        curves["DetRe"].append(_ratio(tp, tp + fn))
        curves["DetPr"].append(_ratio(tp, tp + fp))
        curves["AssA"].append(ass_a)
        curves["AssRe"].append(_ratio(tot["assre_sum"][i], tp))
        curves["AssPr"].append(_ratio(tot["asspr_sum"][i], tp))
        curves["LocA"].append(_ratio(tot["loc_sum"][i], tp, empty=1.0))
        curves["HOTA"].append(math.sqrt(det_a * ass_a))
    out = dict(alphas=alphas, TP=tot["TP"], FN=tot["FN"], FP=tot["FP"], curves=curves)
    for k in CURVES:
        out[k] = float(np.mean(np.asarray(curves[k], dtype=np.float64)))
    return out


def evaluate(sequences, sigmas=None, alphas=DEFAULT_ALPHAS, oks=None, **switches):
    """{"hota": finish(...), "per_sequence_hota": name -> the record's lists, "details": name -> the record's details
    and its OKS matrices}."""
    per_sequence, details = {}, {}
    for name, frames in sequences.items():
        mats = [np.asarray(m, dtype=np.float64) for m in oks[name]] if oks is not None else \
            [frame_oks(f, sigmas) for f in frames]
        rec = hota_sequence(frames, mats, alphas, **switches)
        details[name] = dict(rec.pop("details"), oks=mats)
        per_sequence[name] = rec
    return dict(hota=finish(list(per_sequence.values()), alphas), per_sequence_hota=per_sequence, details=details)


def min_alpha_gap(result):
    """The smallest |s - alpha| over every OKS of the result's details and every alpha (inf without any)."""
    gap = float("inf")
    for d in result["details"].values():
        for s in d["oks"]:
            if s.size:
                for alpha in result["hota"]["alphas"]:
                    gap = min(gap, float(np.nanmin(np.abs(s - alpha))))
    return gap


def integers(result):
    """Everything of a result that is an integer: TP per sequence and alpha, the held rows, mc."""
    return {name: (result["per_sequence_hota"][name]["TP"], d["held"], d["mc"])
            for name, d in result["details"].items()}
