"""The gauge of ValidationMeter: its semantics restated with numpy for the integer state and Python integers /
``fractions.Fraction`` for the report (include/probpose_hip.h, "ValidationMeter").

``update`` adds one batch to a state of int64 arrays by the names of the header's sections; ``report`` forms every field
as an exact rational of the integer state and rounds it once (``float(Fraction)`` is correctly rounded), apart from the
square roots, which take the correctly rounded radicand.  The whole-set fields of ``scalars`` are float64 sums in update
order, as on the device.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

BINS = 1024
Q30, Q20 = 2 ** 30, 2 ** 20
FLAG_TARGET_RANGE, FLAG_NONFINITE = 256, 512
BINARY = ("n_pos", "n_neg", "best_bal_acc", "best_thr", "auroc", "brier", "ece", "mce", "mean_conf", "base_rate")
REJECTED = ("mask", "probability", "visibility", "oks", "error")
NAN = float("nan")


def q_fixed(z, scale) -> np.ndarray:
    """rint(z * scale) in float64, ties to even."""
    return np.rint(np.asarray(z, dtype=np.float64) * float(scale)).astype(np.int64)


def fine_bin(p) -> np.ndarray:
    p = np.asarray(p, dtype=np.float32)
    return np.minimum(BINS - 1, np.floor(p * np.float32(1024))).astype(np.int64)


def unit_ok(p) -> np.ndarray:
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (p >= 0) & (p <= 1)


def err_ok(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= np.float32(2 ** 20))


def empty_state(K: int, J: int) -> dict:
    z = lambda *s: np.zeros(s, dtype=np.int64)       # noqa: E731
    return dict(hist=z(2, K, 2, BINS), conf=z(2, K, BINS), above=z(2, K, 2, J), sum_p=z(2, K, 2), sum_p2=z(2, K, 2),
                oks_hist=z(K, BINS), oks_sx=z(K, BINS), oks_st=z(K, BINS), oks_sums=z(K, 5), err=z(K, 4), pck=z(2, K),
                all=z(3), rejected=z(5), scalars=z(15))


def state_words(K: int, J: int) -> int:
    return sum(v.size for v in empty_state(K, J).values())


def _batch_pck_average(counts) -> float:
    s, cnt = 0.0, 0
    for h, v in zip(counts[0], counts[1]):
        if v > 0:
            s += float(h) / float(v)
            cnt += 1
    return s / cnt if cnt else 0.0


def update(state, thresholds, prob, vis, oks, err, in_image, annotated, visibility, gt_oks, gt_err, pck_counts=None,
           map_max=None, res=None) -> None:
    """One batch of [B,K] arrays into ``state``."""
    thr = np.asarray(thresholds, dtype=np.float64)
    f = [np.asarray(a, dtype=np.float32) for a in (prob, vis, oks, err, gt_oks, gt_err)]
    prob, vis, oks, err, gt_oks, gt_err = f
    B, K = prob.shape
    im, an, vz = (np.asarray(a).astype(np.int64).reshape(B, K) for a in (in_image, annotated, visibility))
    kk = np.broadcast_to(np.arange(K), (B, K))

    state["all"][0] += B * K
    ok = unit_ok(prob)
    state["all"][1] += int(ok.sum())
    state["all"][2] += int(q_fixed(prob[ok], Q30).sum())
    bad_mask = ~np.isin(im, (0, 1)) | ~np.isin(an, (0, 1))
    state["rejected"][0] += int(bad_mask.sum())
    pop_prob = ~bad_mask & (an == 1)
    pop_in = pop_prob & (im == 1)

    for h, (p, pop, label) in enumerate(((prob, pop_prob, im), (vis, pop_in, (vz != 0).astype(np.int64)))):
        good = pop & unit_ok(p)
        state["rejected"][1 + h] += int((pop & ~good).sum())
        pv, kv, lv = p[good], kk[good], label[good]
        pd = pv.astype(np.float64)
        np.add.at(state["hist"][h], (kv, lv, fine_bin(pv)), 1)
        np.add.at(state["conf"][h], (kv, fine_bin(pv)), q_fixed(pd, Q30))
        np.add.at(state["sum_p"][h], (kv, lv), q_fixed(pd, Q30))
        np.add.at(state["sum_p2"][h], (kv, lv), q_fixed(pd * pd, Q30))
        over = pd[:, None] > thr[None, :]                # strict, in float64 (loss.py:686)
        for j in range(len(thr)):
            np.add.at(state["above"][h][:, :, j], (kv[over[:, j]], lv[over[:, j]]), 1)

    good = pop_in & unit_ok(oks) & unit_ok(gt_oks)
    state["rejected"][3] += int((pop_in & ~good).sum())
    x, t, kv = oks[good].astype(np.float64), gt_oks[good].astype(np.float64), kk[good]
    b = fine_bin(oks[good])
    np.add.at(state["oks_hist"], (kv, b), 1)
    np.add.at(state["oks_sx"], (kv, b), q_fixed(x, Q30))
    np.add.at(state["oks_st"], (kv, b), q_fixed(t, Q30))
    d = x - t
    for i, z in enumerate((np.abs(d), d * d, x * x, t * t, x * t)):
        np.add.at(state["oks_sums"][:, i], kv, q_fixed(z, Q30))

    good = pop_in & err_ok(err) & err_ok(gt_err)
    state["rejected"][4] += int((pop_in & ~good).sum())
    x, t, kv = err[good].astype(np.float64), gt_err[good].astype(np.float64), kk[good]
    for i, z in enumerate((np.ones_like(x) / Q20, x, t, np.abs(x - t))):
        np.add.at(state["err"][:, i], kv, q_fixed(z, Q20))

    if pck_counts is not None:
        state["pck"] += np.asarray(pck_counts, dtype=np.int64)

    S = state["scalars"]
    D = S[6:].view(np.float64)
    S[0] += 1
    flagged = False
    if res is not None:
        r = np.asarray(res, dtype=np.float32)
        word = int(r[9]) if np.isfinite(r[9]) and abs(float(r[9])) < 2 ** 31 else FLAG_NONFINITE
        if r[2] != 0:
            word |= FLAG_TARGET_RANGE
        finite = bool(np.isfinite(r[[1, 3, 4, 5, 6, 7, 8]]).all())
        if not finite:
            word |= FLAG_NONFINITE
        flagged = bool(r[9] != 0 or r[2] != 0 or not finite)
        S[2] |= word
        if flagged:
            S[1] += 1
        else:
            S[3] += 1
            D[0] += float(r[1])
            for i in range(3, 9):
                D[i - 2] += float(r[i])
    if pck_counts is not None and not flagged:
        S[4] += 1
        D[7] += _batch_pck_average(np.asarray(pck_counts))
    if map_max is not None:
        m = np.asarray(map_max, dtype=np.float32)
        bm = float("nan") if np.isnan(m).any() else float(m.max())
        cur = float(D[8])
        if S[5] == 0 or bm != bm or (cur == cur and bm > cur):
            D[8] = bm
        S[5] += 1


def _f(num, den) -> float:
    return float(Fraction(int(num), int(den)))


def _binary_row(neg, pos, conf, above, sum_p, sum_p2, thr, E) -> dict:
    """neg / pos / conf [1024], above [2][J], sum_p / sum_p2 [2]: Python-int arithmetic."""
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    n, J, width = n_pos + n_neg, len(thr), BINS // E
    out = dict(n_pos=float(n_pos), n_neg=float(n_neg))
    both = n_pos > 0 and n_neg > 0
    vals = [int(above[1][j]) * n_neg + (n_neg - int(above[0][j])) * n_pos for j in range(J)]
    out["bal_acc"] = np.array([_f(v, 2 * n_pos * n_neg) if both else NAN for v in vals])
    if both:
        best = max(range(J), key=lambda j: (vals[j], -j))
        out["best_bal_acc"], out["best_thr"] = _f(vals[best], 2 * n_pos * n_neg), float(thr[best])
        pos_above = np.concatenate([np.cumsum(pos[::-1])[::-1][1:], [0]])
        num = sum(int(a) * (2 * int(u) + int(p)) for a, u, p in zip(neg, pos_above, pos))
        out["auroc"] = _f(num, 2 * n_pos * n_neg)
    else:
        out["best_bal_acc"] = out["best_thr"] = 0.0
        out["auroc"] = NAN
    rel = np.full((E, 3), NAN)
    ece, mce = 0, Fraction(-1)
    for c in range(E):
        s = slice(c * width, (c + 1) * width)
        nc, pc, cc = int(pos[s].sum() + neg[s].sum()), int(pos[s].sum()), int(conf[s].sum())
        rel[c, 0] = nc
        d = abs(cc - pc * Q30)
        ece += d
        if nc:
            mce = max(mce, Fraction(d, nc * Q30))
            rel[c, 1], rel[c, 2] = _f(cc, nc * Q30), _f(pc, nc)
    out["reliability"] = rel
    if n:
        out["brier"] = _f(int(sum_p2[0]) + int(sum_p2[1]) - 2 * int(sum_p[1]) + n_pos * Q30, n * Q30)
        out["ece"], out["mce"] = _f(ece, n * Q30), float(mce)
        out["mean_conf"], out["base_rate"] = _f(int(sum_p[0]) + int(sum_p[1]), n * Q30), _f(n_pos, n)
    else:
        out["brier"] = out["ece"] = out["mce"] = out["mean_conf"] = out["base_rate"] = NAN
    return out


def oks_moments(n, sx, st, sums):
    """(vx, vt, cov) of the OKS head as exact rationals of the state's sums."""
    den = n * Q30
    mx, mt = Fraction(sx, den), Fraction(st, den)
    return (Fraction(int(sums[2]), den) - mx * mx, Fraction(int(sums[3]), den) - mt * mt,
            Fraction(int(sums[4]), den) - mx * mt)


def _oks_row(hist, sx, st, sums, E) -> dict:
    n, width = int(hist.sum()), BINS // E
    rel = np.full((E, 3), NAN)
    for c in range(E):
        s = slice(c * width, (c + 1) * width)
        nc = int(hist[s].sum())
        rel[c, 0] = nc
        if nc:
            rel[c, 1], rel[c, 2] = _f(sx[s].sum(), nc * Q30), _f(st[s].sum(), nc * Q30)
    out = dict(n=float(n), reliability=rel, mae=NAN, rmse=NAN, bias=NAN, pearson=NAN)
    if n:
        tx, tt = int(sx.sum()), int(st.sum())
        out["mae"] = _f(sums[0], n * Q30)
        out["rmse"] = math.sqrt(_f(sums[1], n * Q30))
        out["bias"] = _f(tx - tt, n * Q30)
        vx, vt, cov = oks_moments(n, tx, tt, sums)
        if vx > 0 and vt > 0:
            out["pearson"] = float(cov) / math.sqrt(float(vx * vt))
    return out


def _stack(rows) -> dict:
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def report(state, thresholds, ece_bins: int = 16) -> dict:
    """The report in the layout of ``probpose_pytorch_amd.valmeter.parse_report``: per-row fields are arrays of K+1,
    the last entry the pool over the keypoints."""
    thr = np.asarray(thresholds, dtype=np.float64)
    K = state["oks_hist"].shape[0]
    E = ece_bins
    rows = [slice(k, k + 1) for k in range(K)] + [slice(0, K)]
    out = {"thresholds": thr.copy()}
    for h, head in enumerate(("probability", "visibility")):
        out[head] = _stack([_binary_row(state["hist"][h][r, 0].sum(0), state["hist"][h][r, 1].sum(0),
                                        state["conf"][h][r].sum(0), state["above"][h][r].sum(0),
                                        state["sum_p"][h][r].sum(0), state["sum_p2"][h][r].sum(0), thr, E)
                            for r in rows])
    out["oks"] = _stack([_oks_row(state["oks_hist"][r].sum(0), state["oks_sx"][r].sum(0), state["oks_st"][r].sum(0),
                                  state["oks_sums"][r].sum(0), E) for r in rows])
    err = []
    for r in rows:
        s = [int(v) for v in state["err"][r].sum(0)]
        err.append(dict(n=float(s[0]), mae=_f(s[3], s[0] * Q20) if s[0] else NAN,
                        bias=_f(s[1] - s[2], s[0] * Q20) if s[0] else NAN))
    out["error"] = _stack(err)
    hits, valid = state["pck"]
    pck = [float(h) / float(v) if v > 0 else -1.0 for h, v in zip(hits, valid)]
    seen = [p for p, v in zip(pck, valid) if v > 0]
    s = 0.0
    for p in seen:
        s += p
    out["pck"] = np.array(pck + [s / len(seen) if seen else NAN])
    S = state["scalars"]
    D = S[6:].view(np.float64)
    mean = lambda v, n: float(v) / float(n) if n > 0 else NAN      # noqa: E731
    out["reference"] = dict(loss_kpt=mean(D[0], S[3]), loss_probability=mean(D[1], S[3]),
                            loss_visibility=mean(D[2], S[3]), loss_oks=mean(D[3], S[3]), loss_error=mean(D[4], S[3]),
                            acc_kpt=mean(D[7], S[4]), acc_oks=mean(D[5], S[3]), acc_error=mean(D[6], S[3]))
    out["max_heatmap"] = float(D[8]) if S[5] > 0 else NAN
    A = state["all"]
    out["mean_prob"] = _f(A[2], int(A[1]) * Q30) if A[1] > 0 else NAN
    out["batches"], out["flagged_batches"], out["flags"] = int(S[0]), int(S[1]), int(S[2])
    out["rejected"] = {name: int(state["rejected"][i]) for i, name in enumerate(REJECTED)}
    return out


# ----------------------------------------------------------------------------------------------- test data
def edge_values():
    """0, 1, some k/1024 with both float32 neighbours, float32(0.15), 0.25 and 0.5 (thresholds of some tests)."""
    v = [0.0, 1.0, np.float32(0.15), np.float32(0.25), np.float32(0.5)]
    for k in (1, 511, 512, 1023):
        x = np.float32(k / 1024)
        v += [x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(1))]
    return np.array(v, dtype=np.float32)


def random_batch(rng, B, K, ties=True):
    """[prob, vis, oks, err, in_image, annotated, visibility, gt_oks, gt_err] as [B,K] arrays, in ``update``'s order."""
    n = B * K
    draw = lambda: rng.random(n, dtype=np.float32)          # noqa: E731
    prob, vis, oks, gt_oks = draw(), draw(), draw(), draw()
    if ties:        # repeated values and bin edges
        e = edge_values()
        for a in (prob, vis, oks, gt_oks):
            idx = rng.integers(0, n, size=n // 2)
            a[idx] = e[rng.integers(0, len(e), size=len(idx))]
    err = (rng.random(n, dtype=np.float32) * 30).astype(np.float32)
    gt_err = (rng.random(n, dtype=np.float32) * 30).astype(np.float32)
    in_image = (rng.random(n) < 0.7).astype(np.int64)
    annotated = (rng.random(n) < 0.8).astype(np.int64)
    visibility = (rng.random(n) < 0.5).astype(np.int64) * rng.integers(1, 3, size=n)
    return [a.reshape(B, K) for a in (prob, vis, oks, err, in_image, annotated, visibility, gt_oks, gt_err)]
