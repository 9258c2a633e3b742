"""The gauge of HeadCalibration: the fit in Python integers, the apply in numpy float32, the score in
``fractions.Fraction`` (include/probpose_hip.h, "HeadCalibration").

``isotonic_blocks`` is a stack pool-adjacent-violators over the non-empty bins: a new block pools with the block under
it while value(under) >= value(new), compared as ``P_l * N_r >= P_r * N_l`` in unbounded integers.  ``mul`` stands for
that product, so a test can run the same code under masked 64-bit arithmetic and see what wraps.  The table is formed
with the roundings the header states: ``float(int)``, float64 division and ``np.float32`` each round to nearest even.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests import valmeter_reference as vr

BINS = vr.BINS
Q30 = vr.Q30
HEADS = ("probability", "visibility", "oks")
BINARY = ("n", "skipped", "brier", "mean_conf", "ece", "mce")
OKS = ("n", "skipped", "ece")
NAN = float("nan")


def exact_mul(a: int, b: int) -> int:
    return a * b


def wrapped_mul(a: int, b: int) -> int:
    """The product as int64 arithmetic gives it: the low 64 bits, read as a signed number."""
    v = (a * b) & (2 ** 64 - 1)
    return v - 2 ** 64 if v >= 2 ** 63 else v


def isotonic_blocks(P, n, mul=exact_mul):
    """(P, N) of the block that covers each bin, as a list of pairs of Python ints, and the list of the blocks as
    (first bin, end bin, P, N).  An empty bin (n == 0) carries the block of the nearest non-empty bin to its left, the
    leading empty bins the first block; no sample at all gives (0, 0) everywhere and no block."""
    P, n = [int(v) for v in P], [int(v) for v in n]
    stack = []                                  # [first non-empty bin, P, N]
    for b, (p, w) in enumerate(zip(P, n)):
        if w == 0:
            continue
        cur = [b, p, w]
        while stack and mul(stack[-1][1], cur[2]) >= mul(cur[1], stack[-1][2]):
            top = stack.pop()
            cur = [top[0], top[1] + cur[1], top[2] + cur[2]]
        stack.append(cur)
    if not stack:
        return [(0, 0)] * len(P), []
    blocks = []
    for i, (first, p, w) in enumerate(stack):
        start = 0 if i == 0 else first
        end = stack[i + 1][0] if i + 1 < len(stack) else len(P)
        blocks.append((start, end, p, w))
    per_bin = []
    for start, end, p, w in blocks:
        per_bin += [(p, w)] * (end - start)
    return per_bin, blocks


def head_rows(state, h):
    """(P [K+1][1024], n [K+1][1024]) int64 of head h, row K the pool."""
    if h < 2:
        P, n = state["hist"][h][:, 1], state["hist"][h][:, 0] + state["hist"][h][:, 1]
    else:
        P, n = state["oks_st"], state["oks_hist"]
    return np.concatenate([P, P.sum(0, keepdims=True)]), np.concatenate([n, n.sum(0, keepdims=True)])


def table_value(h, P, N) -> np.float32:
    if N == 0:
        return np.float32(0)
    q = float(P) / float(N)                     # two exact-or-rounded conversions, one float64 division
    return np.float32(q if h < 2 else q * 2.0 ** -30)


def fit(state, K, J, min_count, mul=exact_mul):
    """blocks [3][K+1][1024][2] int64, table [3][K+1][1024] float32, row_of [3][K] int32.  J only fixes the layout."""
    assert state["hist"].shape == (2, K, 2, BINS) and state["above"].shape[-1] == J
    blocks = np.zeros((3, K + 1, BINS, 2), dtype=np.int64)
    table = np.zeros((3, K + 1, BINS), dtype=np.float32)
    row_of = np.zeros((3, K), dtype=np.int32)
    for h in range(3):
        P, n = head_rows(state, h)
        for r in range(K + 1):
            per_bin, _ = isotonic_blocks(P[r], n[r], mul)
            blocks[h, r] = np.array(per_bin, dtype=np.int64)
            seen = {}
            for b, (p, w) in enumerate(per_bin):
                if (p, w) not in seen:
                    seen[(p, w)] = table_value(h, p, w)
                table[h, r, b] = seen[(p, w)]
        counts = [int(v) for v in n.sum(1)]
        for k in range(K):
            row_of[h, k] = k if counts[k] >= min_count else (K if counts[K] >= 1 else -1)
    return blocks, table, row_of


def apply(aux, table, row_of):
    """aux [3][B][K] float32 -> the calibrated copy; what is not in [0, 1] or has no row passes bit for bit."""
    aux = np.asarray(aux, dtype=np.float32)
    out = aux.copy()
    _, B, K = aux.shape
    for h in range(3):
        for k in range(K):
            r = int(row_of[h, k])
            if r < 0:
                continue
            p = aux[h, :, k]
            ok = vr.unit_ok(p)
            out[h, ok, k] = table[h, r][vr.fine_bin(p[ok])]
    return out


def ece_bin(y: np.float32, E: int) -> int:
    return min(E - 1, int(np.float32(y) * np.float32(E)))


def _score_row(h, cells, E) -> dict:
    """cells: (n_b, P_b, y_b) of every fine bin of every keypoint of the row that has a table; exact rationals."""
    n = sum(c[0] for c in cells)
    cnt, num, conf = [0] * E, [0] * E, [Fraction(0)] * E
    brier = Fraction(0)
    for w, p, y in cells:
        if w == 0:
            continue
        yf = Fraction(float(y))
        e = ece_bin(y, E)
        cnt[e] += w
        num[e] += p
        conf[e] += w * yf
        if h < 2:
            brier += p * (1 - yf) ** 2 + (w - p) * yf ** 2
    scale = 1 if h < 2 else Q30
    rel = np.full((E, 3), NAN)
    gaps = []
    for e in range(E):
        rel[e, 0] = cnt[e]
        if cnt[e]:
            rel[e, 1], rel[e, 2] = float(conf[e] / cnt[e]), float(Fraction(num[e], cnt[e] * scale))
            gaps.append((abs(conf[e] - Fraction(num[e], scale)), cnt[e]))
    out = dict(n=float(n), reliability=rel)
    out["ece"] = float(sum(g for g, _ in gaps) / n) if n else NAN
    if h < 2:
        out["brier"] = float(brier / n) if n else NAN
        out["mean_conf"] = float(sum(conf) / n) if n else NAN
        out["mce"] = float(max(g / c for g, c in gaps)) if n else NAN
    return out


def score(state, K, J, table, row_of, ece_bins: int = 16) -> dict:
    """The report in the layout of ``probpose_pytorch_amd.calibration.parse_score``: per head a dict of arrays of K+1
    (the last entry pools the keypoints, each through its own table)."""
    assert state["above"].shape[-1] == J
    out = {}
    for h, head in enumerate(HEADS):
        P, n = head_rows(state, h)
        rows = []
        for r in range(K + 1):
            cells, skipped = [], 0
            for k in (range(K) if r == K else (r,)):
                t = int(row_of[h, k])
                if t < 0:
                    skipped += int(n[k].sum())
                    continue
                cells += [(int(n[k, b]), int(P[k, b]), table[h, t, b]) for b in range(BINS)]
            row = _score_row(h, cells, ece_bins)
            row["skipped"] = float(skipped)
            rows.append(row)
        out[head] = {key: np.array([row[key] for row in rows]) for key in rows[0]}
    return out
