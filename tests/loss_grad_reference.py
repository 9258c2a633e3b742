"""Float64 restatement of the gradients of the reference's losses (probpose/loss.py:55-143, :232-339, :419-464) and of
ProbPoseLoss as train.py weights it.  Built on tests/loss_reference.py, which it leaves as it is.

Every function returns (value, magnitude, c) triples: ``value`` the gradient in float64, ``magnitude`` the sum of the
absolute values of the terms it is built from (each term's own inputs -- a Sobel response, log(1 + x) -- counted by
the magnitudes of their terms), and ``c`` from the kernels' order of evaluation (csrc/pp_loss.hip), for the comparator
``|got - value| <= c * 2^-23 * magnitude`` of ``loss_reference.ratio``:

* C_GRAD_HM = 32, a heatmap gradient.  Per pixel: gx, gy are sums of 6 terms in 3 levels (3 roundings), G lw m gx
  adds 3 more (4 when G is the pixel mean's u / N), the 18 neighbour terms are added in sequence (18), the scaling by
  2 sw and the local term's 7 roundings meet in one more add: 3 + 4 + 18 + 2 + 1 = 28 <= 32.  The per-keypoint and
  mean reductions round fewer times (one Sobel response, no neighbour sum).
* C_GRAD_HEAD = 8, a head gradient: u / N, the difference, the product, (1 - x) x and the quotient (BCE, 5); the
  weighted difference, 2, u / N and the products (MSE, 5); u / N, two logs of about one ulp each, the difference, the
  clamp, two products and the quotient (L1Log, 7).

The arg-max pixel of the per-keypoint and mean reductions is chosen on the float32 energies evaluated exactly as the
kernels evaluate them (``energy_f32``; numpy float32 ops round as the kernels' -ffp-contract=off arithmetic does), so
the restatement puts the max-gradient subgradient at the pixel the kernel finds: the first maximum in row-major order,
a NaN counting as the maximum (torch's CPU max(dim) rule).

``fault`` plants the kernel faults the comparator must reject: 'unflipped' (the Sobel kernels not flipped in the
backward), 'border' (energies of out-of-map neighbours contribute at the border), ('seam', rows) (the halo row above
each tile of ``rows`` rows lost), 'last_max' (the subgradient at the last maximal pixel), 'bce_noclamp' (no 1e-12
clamp), 'l1log_nodiv' (no 1 / (1 + x) factor), 'vis_weighted' (the visibility BCE weighted by the visibility weights
before their normalisation).
"""
from __future__ import annotations

import numpy as np

try:
    from tests import loss_reference as LR
except ImportError:     # loaded by path (tests/golden/make_goldens_loss_grad.py)
    import loss_reference as LR

C_GRAD_HM = 32
C_GRAD_HEAD = 8
LOSS_WEIGHTS = {"kpt": 1.0, "probability": 1.0, "visibility": 0.0, "oks": 1.0, "error": 1.0}     # train.py:26-32
LOSS_KEYS = ("kpt", "probability", "visibility", "oks", "error")
PRED_KEYS = ("heatmaps", "probs", "vis", "oks", "errs")

SOBEL_X = np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=np.float64)
SOBEL_Y = np.array([[1, 2, 1], [0, 0, 0], [-1, -2, -1]], dtype=np.float64)


def _mask(B, K, H, W, target, target_weights, mask, skip_empty, dtype):
    """The forward's mask (spatial mask * weight * non-empty channel) as (B,K,H,W), multiplied in the kernel's order."""
    m = np.ones((B, K, H, W), dtype=dtype)
    if mask is not None:
        m = m * np.broadcast_to(np.asarray(mask, dtype=dtype), (B, K, H, W))
    if target_weights is not None:
        w = np.asarray(target_weights, dtype=dtype)
        m = m * np.broadcast_to(w.reshape(w.shape + (1,) * (4 - w.ndim)), (B, K, H, W))
    if skip_empty:
        ne = (np.asarray(target) != 0).reshape(B, K, -1).any(axis=2).astype(dtype)
        m = m * ne[..., None, None]
    return m


def energy_f32(output, m32):
    """The masked Sobel energy (gx^2 + gy^2) * m in float32, operation by operation as the kernels compute it."""
    o = np.asarray(output, dtype=np.float32)
    H, W = o.shape[-2:]
    p = np.pad(o, [(0, 0)] * (o.ndim - 2) + [(1, 1), (1, 1)])
    a = lambda dr, dc: p[..., dr:dr + H, dc:dc + W]   # noqa: E731
    two = np.float32(2)
    gx = (a(0, 0) - a(0, 2)) + two * (a(1, 0) - a(1, 2)) + (a(2, 0) - a(2, 2))
    gy = (a(0, 0) + two * a(0, 1) + a(0, 2)) - (a(2, 0) + two * a(2, 1) + a(2, 2))
    return (gx * gx + gy * gy) * np.asarray(m32, dtype=np.float32)


def first_max(e, last=False):
    """Row-major index of the first (``last``: the last) maximum of each map of e (B,K,H,W); a NaN is the maximum."""
    B, K = e.shape[:2]
    f = e.reshape(B, K, -1)
    if not last:
        return np.argmax(f, axis=2)       # numpy: the first NaN, else the first maximum
    r = f[..., ::-1]
    return f.shape[2] - 1 - np.argmax(r, axis=2)


def _correlate_back(ex, ey, fault=None):
    """sum over the 3x3 neighbours p = q - d of Sx[d] ex[p] + Sy[d] ey[p] (ex, ey zero outside the map), and the same
    with |Sx|, |Sy| on magnitudes when given pairs."""
    H, W = ex.shape[-2:]
    sx, sy = (SOBEL_X[::-1, ::-1], SOBEL_Y[::-1, ::-1]) if fault == "unflipped" else (SOBEL_X, SOBEL_Y)
    px = np.pad(ex, [(0, 0)] * (ex.ndim - 2) + [(1, 1), (1, 1)])
    py = np.pad(ey, [(0, 0)] * (ey.ndim - 2) + [(1, 1), (1, 1)])
    out = np.zeros_like(ex)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            # p = q - d: padded index (r + 1 - dr, c + 1 - dc)
            cx, cy = sx[dr + 1, dc + 1], sy[dr + 1, dc + 1]
            out = out + cx * px[..., 1 - dr:1 - dr + H, 1 - dc:1 - dc + W] + cy * py[..., 1 - dr:1 - dr + H,
                                                                                     1 - dc:1 - dc + W]
    return out


def oks_heatmap_loss_grad(output, target, target_weights=None, mask=None, skip_empty=False, oks_type="minus",
                          sw=0.2, gw=0.0, lw=1.0, reduction="mean", upstream=1.0, *, fault=None):
    """d/d output of OKSHeatmapLoss (loss.py:55-191) for ``reduction`` in 'pixel', 'keypoint', 'mean' and
    'pixel_mean' (the mean of the per-pixel loss, ProbPoseLoss's kpt term), with the upstream gradient ``upstream``
    ((B,K,H,W), (B,K) or a scalar).  Returns (value, magnitude, C_GRAD_HM), each (B,K,H,W)."""
    o = np.asarray(output, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    B, K, H, W = o.shape
    m = _mask(B, K, H, W, target, target_weights, mask, skip_empty, np.float64)
    am = np.abs(m)
    if oks_type == "minus":
        dok, a_dok = 1 - t, 1 + np.abs(t)
    elif oks_type == "plus":
        dok, a_dok = -t, np.abs(t)
    else:
        dok, a_dok = ((1 - t) - t) / 2, (1 + 2 * np.abs(t)) / 2
    ow = 1 - sw - gw
    gx, gy, ax, ay = LR._sobel(o)
    u = np.asarray(upstream, dtype=np.float64)
    if reduction in ("pixel", "pixel_mean"):
        G = np.broadcast_to(u / (B * K * H * W) if reduction == "pixel_mean" else u, (B, K, H, W))
        s, a_s = G * lw * m, np.abs(G * lw) * am
        ex, ey = s * gx, s * gy
        a_ex, a_ey = a_s * ax, a_s * ay
        if fault == "border":       # the zero-padded ring's energies enter too, with the edge pixel's G and m
            pad = lambda z, mode: np.pad(z, [(0, 0), (0, 0), (1, 1), (1, 1)], mode=mode)   # noqa: E731
            op = pad(o, "constant")
            gxp, gyp, _, _ = LR._sobel(op)
            sp = pad(s, "edge")
            exp, eyp = sp * gxp, sp * gyp
            ring = np.ones((H + 2, W + 2), bool)
            ring[1:-1, 1:-1] = False
            full_x = _correlate_back(np.where(ring, exp, np.pad(ex, [(0, 0), (0, 0), (1, 1), (1, 1)])),
                                     np.where(ring, eyp, np.pad(ey, [(0, 0), (0, 0), (1, 1), (1, 1)])))
            sob = full_x[..., 1:-1, 1:-1]
        elif isinstance(fault, tuple) and fault[0] == "seam":
            rows = fault[1]
            sob = _correlate_back(ex, ey)
            for r in range(rows, H, rows):  # the halo row r - 1 above the tile starting at row r is lost
                lost_x, lost_y = np.zeros_like(ex), np.zeros_like(ey)
                lost_x[..., r - 1, :], lost_y[..., r - 1, :] = ex[..., r - 1, :], ey[..., r - 1, :]
                sob[..., r, :] -= _correlate_back(lost_x, lost_y)[..., r, :]
        else:
            sob = _correlate_back(ex, ey, fault)
        a_sob = _abs_correlate(a_ex, a_ey)
        val = 2 * sw * sob + s * (ow * dok + gw * 2 * (o - t))
        mag = 2 * abs(sw) * a_sob + a_s * (abs(ow) * a_dok + abs(gw) * 2 * (np.abs(o) + np.abs(t)))
        return val, mag, C_GRAD_HM
    # per keypoint / mean: a = d loss / d (per-keypoint loss without lw) * lw
    if reduction == "keypoint":
        a = np.broadcast_to(u, (B, K)) * lw
    elif reduction == "mean":
        a = np.full((B, K), float(u) * lw / (B * K))
    else:
        raise ValueError(reduction)
    a4 = a[..., None, None]
    val = a4 * m * (ow * dok + gw * 2 * (o - t) / (H * W))
    mag = np.abs(a4) * am * (abs(ow) * a_dok + abs(gw) * 2 * (np.abs(o) + np.abs(t)) / (H * W))
    m32 = _mask(B, K, H, W, target, target_weights, mask, skip_empty, np.float32)
    star = first_max(energy_f32(output, m32), last=fault == "last_max")
    sx, sy = (SOBEL_X[::-1, ::-1], SOBEL_Y[::-1, ::-1]) if fault == "unflipped" else (SOBEL_X, SOBEL_Y)
    for b in range(B):
        for k in range(K):
            pr, pc = divmod(int(star[b, k]), W)
            s = a[b, k] * m[b, k, pr, pc] * 2 * sw
            as_ = abs(s)
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    r, c = pr + dr, pc + dc
                    if 0 <= r < H and 0 <= c < W:
                        val[b, k, r, c] += s * (gx[b, k, pr, pc] * sx[dr + 1, dc + 1] + gy[b, k, pr, pc] *
                                                sy[dr + 1, dc + 1])
                        mag[b, k, r, c] += as_ * (ax[b, k, pr, pc] * abs(SOBEL_X[dr + 1, dc + 1]) +
                                                  ay[b, k, pr, pc] * abs(SOBEL_Y[dr + 1, dc + 1]))
    return val, mag, C_GRAD_HM


def _abs_correlate(a_ex, a_ey):
    H, W = a_ex.shape[-2:]
    px = np.pad(a_ex, [(0, 0)] * (a_ex.ndim - 2) + [(1, 1), (1, 1)])
    py = np.pad(a_ey, [(0, 0)] * (a_ey.ndim - 2) + [(1, 1), (1, 1)])
    out = np.zeros_like(a_ex)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            out = out + (abs(SOBEL_X[dr + 1, dc + 1]) * px[..., 1 - dr:1 - dr + H, 1 - dc:1 - dc + W]
                         + abs(SOBEL_Y[dr + 1, dc + 1]) * py[..., 1 - dr:1 - dr + H, 1 - dc:1 - dc + W])
    return out


# ----------------------------------------------------------------------------------------------- the four heads
def visibility_weights(annotated, in_image, vis, normalise=True):
    """loss.py:436-450 (float32 counts as torch forms them); ``normalise=False`` stops before the division."""
    annotated_in = annotated & (in_image > 0.5)
    invisible_in = (vis == 0) & (annotated > 0.5)
    visible_in = (vis > 0) & (annotated > 0.5)
    wv = annotated_in.astype(np.float64)
    wv[invisible_in] = np.float64(np.float32(1) / (np.float32(invisible_in.sum()) + np.float32(1e-10)))
    wv[visible_in] = np.float64(np.float32(1) / (np.float32(visible_in.sum()) + np.float32(1e-10)))
    return wv / wv[wv > 0].min() if normalise else wv


def head_grads(dt_probs, dt_vis, dt_oks, dt_errs, gt_oks, gt_err, in_image, annotated, visibility, upstream,
               *, fault=None) -> dict:
    """d/d head of the four small losses of ProbPoseLoss.forward (loss.py:432-464), each a mean over N = B*K, with
    the float32 targets gt_oks / gt_err the loss was given.  ``upstream``: {probability, visibility, oks, error} ->
    float.  Returns {'probs', 'vis', 'oks', 'errs'}: (value, magnitude, C_GRAD_HEAD), each (B,K)."""
    probs = np.asarray(in_image).astype(np.int64)
    ann = np.asarray(annotated).astype(np.int64)
    vis = np.asarray(visibility).astype(np.int64)
    B, K = probs.shape
    N = B * K
    w = (ann & (probs > 0)).astype(np.float64)
    out = {}
    for key, x, y, name in (("probs", dt_probs, probs, "probability"), ("vis", dt_vis, vis, "visibility")):
        x = np.asarray(x, dtype=np.float64).reshape(B, K)
        y = y.astype(np.float64)
        g = upstream[name] / N
        den = (1 - x) * x if fault == "bce_noclamp" else np.maximum((1 - x) * x, 1e-12)
        with np.errstate(divide="ignore", invalid="ignore"):
            v, a = g * (x - y) / den, abs(g) * (np.abs(x) + np.abs(y)) / np.abs(den)
        if key == "vis" and fault == "vis_weighted":
            v = v * visibility_weights(ann, probs, vis, normalise=False)
        out[key] = (v, a, C_GRAD_HEAD)
    g = upstream["oks"] / N
    x = np.asarray(dt_oks, dtype=np.float64).reshape(B, K)
    y = np.asarray(gt_oks, dtype=np.float64).reshape(B, K)
    out["oks"] = (2 * w * (x * w - y * w) * g, 2 * np.abs(w) * (np.abs(x * w) + np.abs(y * w)) * abs(g), C_GRAD_HEAD)
    g = upstream["error"] / N
    x = np.asarray(dt_errs, dtype=np.float32).reshape(B, K)
    x1 = (np.float32(1) + x).astype(np.float64)              # torch.log(1 + x): 1 + x rounded to float32
    la, lb = LR.log1x(x) * w, LR.log1x(np.asarray(gt_err, dtype=np.float32).reshape(B, K)) * w
    z = la - lb
    s = np.clip(z, -1, 1)
    div = 1.0 if fault == "l1log_nodiv" else x1
    mag = np.where(np.abs(z) < 1, np.abs(z) + np.abs(la) + np.abs(lb), 1.0) * abs(g) * np.abs(w) / np.abs(x1)
    out["errs"] = (s * g * w / div, mag, C_GRAD_HEAD)
    return out


def probpose_loss_grads(gt, pred, gt_oks, gt_err, keypoint_weights=None, learn_heatmaps_from_zeros=False,
                        upstream=None, *, fault=None) -> dict:
    """d/d prediction of sum_k upstream[k] * losses[k] for ProbPoseLoss.forward (loss.py:360-464), given the float32
    targets gt_oks / gt_err (B,K) the forward computed (from detached decodes).  ``upstream`` defaults to train.py's
    LOSS_WEIGHTS.  Returns {'heatmaps', 'probs', 'vis', 'oks', 'errs'}: (value, magnitude, c) in the shapes (B,K,H,W)
    and (B,K)."""
    upstream = LOSS_WEIGHTS if upstream is None else upstream
    dt_hm = np.asarray(pred[0], dtype=np.float32)
    B, K, H, W = dt_hm.shape
    as_int = lambda x: np.asarray(x).astype(np.int64).reshape(B, K)   # noqa: E731
    probs, ann, vis = as_int(gt["in_image"]), as_int(gt["keypoints_visible"]), as_int(gt["keypoints_visibility"])
    kw = np.ones((B, K), np.float32) if keypoint_weights is None else np.asarray(keypoint_weights).reshape(B, K)
    hw = ann.astype(np.float32) if learn_heatmaps_from_zeros else kw
    hm_fault = fault if fault in ("unflipped", "border", "last_max") or isinstance(fault, tuple) else None
    out = {"heatmaps": oks_heatmap_loss_grad(dt_hm, np.asarray(gt["heatmaps"], np.float32).reshape(B, K, H, W), hw,
                                             sw=0.05, reduction="pixel_mean", upstream=upstream["kpt"],
                                             fault=hm_fault)}
    out.update(head_grads(*(np.asarray(p, np.float32).reshape(B, K) for p in pred[1:]), gt_oks, gt_err, probs, ann,
                          vis, upstream, fault=fault))
    return out


def one_hot(key) -> dict:
    return {k: float(k == key) for k in LOSS_KEYS}


def targets_f32(gt, pred, gt_kpts, dt_kpts, sigmas, freeze_error=True):
    """The float32 OKS and error targets the forward hands the losses (loss.py:512-640), from decoded coordinates."""
    R = LR.probpose_loss(gt, pred, gt_kpts, dt_kpts, sigmas, freeze_error=freeze_error)
    return R["gt_oks"][0].astype(np.float32), R["gt_err"][0].astype(np.float32)
