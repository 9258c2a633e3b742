"""Float64 restatement of the reference's losses (probpose/loss.py:18-712) and the comparator the loss tests use.

Every function returns (value, scale) pairs: ``value`` in float64, ``scale`` = the sum of the magnitudes of the terms
the value is built from.  A float32 evaluation of the same formula -- the reference's torch ops or the HIP kernels of
csrc/pp_loss.hip -- may differ from ``value`` by a few float32 roundings of those terms, so the comparator accepts
``|got - value| <= c * 2^-23 * scale`` with ``c`` pinned per quantity from the kernel's order of evaluation:

* C_PIX = 8: one per-pixel value (Sobel sums of 5 terms, a square, the mask products, the weighted sum);
* c_sum(n) = 16 + ceil(n / 256): a per-map sum of n pixel values -- each of the 256 lanes adds ceil(n / 256) values in
  sequence, then an 8-level tree (torch's cascade sums stay well inside this);
* C_MEAN = 16: a mean over the B*K keypoints (the kernel sums in float64; torch's float32 mean over a few thousand
  values is a 12-level tree at worst);
* C_TARGET = 2: a float64 quantity rounded once to float32 (OKS and error targets, visibility weights).

The quirks that make the reference's float32 evaluation differ from exact arithmetic by more than rounding are stated
explicitly: ``log(1 + x)`` rounds ``1 + x`` to float32 before the log (loss.py:325-326).

The inputs of the golden cases (tests/golden/loss.npz) are regenerated here from seeds; ``encode_probmaps`` restates
the reference's ProbMap.encode (codec.py:11-70, :176-182) and the fixture's sha256 pins that the maps are the ones
the reference produced.
"""
from __future__ import annotations

import hashlib
import math

import numpy as np

EPS32 = 2.0 ** -23
TINY32 = 2.0 ** -126        # a float32 result is never closer than this to a value below the normal range (flushed)
C_PIX = 8
C_MEAN = 16
C_TARGET = 2

COCO17_SIGMAS = np.array([.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087,
                          .089, .089])


def c_sum(n: int) -> int:
    return 16 + math.ceil(n / 256)


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ----------------------------------------------------------------------------------------------- comparator
def ratio(got, ref, scale, c) -> float:
    """Worst |got - ref| / (c * 2^-23 * scale + 2^-126) over the elements (NaN matches NaN only; inf matches itself)."""
    g = np.asarray(got, dtype=np.float64)
    r = np.broadcast_to(np.asarray(ref, dtype=np.float64), g.shape)
    s = np.broadcast_to(np.asarray(scale, dtype=np.float64), g.shape)
    gn, rn = np.isnan(g), np.isnan(r)
    if (gn != rn).any():
        return math.inf
    same = gn | (g == r)
    d = np.where(same, 0.0, np.abs(g - r))
    bound = c * EPS32 * s + TINY32
    return float((d / bound).max(initial=0.0))


def assert_within(got, ref, scale, c, what=""):
    q = ratio(got, ref, scale, c)
    assert q <= 1.0, f"{what}: d/bound = {q:.3g}"
    return q


# ----------------------------------------------------------------------------------------------- inputs
def encode_probmaps(keypoints, visible, input_size, heatmap_size, sigma=2.0):
    """ProbMap.encode of each crop (reference codec.py:176-182 -> generate_probmaps :11-70, sigma > 0): keypoints
    (B,K,2) f32 input-image pixels, visible (B,K) -> heatmaps (B,K,H,W) f32, in_image (B,K) bool."""
    kp = np.asarray(keypoints, dtype=np.float32)
    B, K = kp.shape[:2]
    W, H = heatmap_size
    scale = ((np.array(input_size) - 1) / (np.array(heatmap_size) - 1)).astype(np.float32)
    hk = kp / scale
    y_idx, x_idx = np.indices((H, W))
    out = np.zeros((B, K, H, W), dtype=np.float32)
    for b in range(B):
        for k in range(K):
            if visible[b, k] < 0.5:
                continue
            dx = x_idx - hk[b, k, 0]
            dy = y_idx - hk[b, k, 1]
            dist = np.sqrt(dx ** 2 + dy ** 2)
            out[b, k] = np.exp(-(dist ** 2 / (2 * sigma)))
    in_image = ((kp[..., 0] >= 0) & (kp[..., 0] < input_size[0]) & (kp[..., 1] >= 0) & (kp[..., 1] < input_size[1]))
    return out, in_image


CASES = {
    # name: (B, K, H, W, input_size, sigmas, seed)
    "G1": (8, 17, 64, 48, (192, 256), COCO17_SIGMAS, 11),
    "G3": (4, 20, 96, 96, (384, 384), np.array([0.05] * 20), 33),
}


def case_inputs(name: str) -> dict:
    """Seeded inputs of a ProbPoseLoss golden case: the reference's collated ground truth and the five heads."""
    B, K, H, W, input_size, sigmas, seed = CASES[name]
    rng = np.random.default_rng(seed)
    lo, hi = -0.1 * np.array(input_size), 1.1 * np.array(input_size)
    kps = rng.uniform(lo, hi, (B, K, 2)).astype(np.float32)          # some keypoints lie outside the image
    annotated = rng.random((B, K)) > 0.25
    visibility = (rng.random((B, K)) > 0.4).astype(np.float32)
    if name == "G3":
        annotated[2] = False                                          # a crop with no annotated keypoint
        annotated[1, 3] = True
        kps[1, 3] = (100.0, 120.0)                                    # annotated, in the image ...
    gt_hm, in_image = encode_probmaps(kps, annotated.astype(np.float32), input_size, (W, H))
    if name == "G3":
        gt_hm[1, 3] = 0.0                                             # ... with an all-zero gt map: NaN coordinates
    # peaked noise: a blob near the gt location of every keypoint, clamped to [0, 1]
    scale = ((np.array(input_size) - 1) / (np.array((W, H)) - 1)).astype(np.float32)
    centre = kps / scale + rng.normal(0, 2.0, (B, K, 2)).astype(np.float32)
    y, x = np.indices((H, W)).astype(np.float32)
    blob = np.exp(-((x - centre[..., 0, None, None]) ** 2 + (y - centre[..., 1, None, None]) ** 2) / 8.0)
    dt_hm = np.clip(blob * 0.9 + rng.random((B, K, H, W), dtype=np.float32) * 0.15, 0, 1).astype(np.float32)
    head = lambda a: a.astype(np.float32).reshape(B, K, 1, 1)   # noqa: E731
    probs = head(rng.uniform(0.01, 0.99, (B, K)))
    vis = head(rng.uniform(0.01, 0.99, (B, K)))
    oks = head(rng.uniform(0.0, 1.0, (B, K)))
    small = rng.random((B, K)) < 0.5
    errs = head(np.where(small, rng.uniform(0, 0.01, (B, K)), rng.uniform(0, 40.0, (B, K))))
    kw = np.where(rng.random((B, K)) < 0.2, 0.0, np.where(rng.random((B, K)) < 0.5, 0.3, 1.0)).astype(np.float32)
    gt = dict(heatmaps=gt_hm, in_image=in_image[:, None, :], keypoints_visible=annotated[:, None, :],
              keypoints_visibility=visibility[:, None, :])
    return dict(gt=gt, pred=(dt_hm, probs, vis, oks, errs), keypoint_weights=kw, sigmas=sigmas, B=B, K=K, H=H, W=W,
                input_size=input_size)


def heatmap_case_inputs(seed: int = 5, B: int = 2, K: int = 3, H: int = 10, W: int = 7) -> dict:
    """Inputs of the OKSHeatmapLoss golden cases: output in [-0.2, 1.2), target in [0, 1] with one all-zero channel."""
    rng = np.random.default_rng(seed)
    out = rng.uniform(-0.2, 1.2, (B, K, H, W)).astype(np.float32)
    tgt = rng.random((B, K, H, W), dtype=np.float32)
    tgt[1, 2] = 0.0
    w2 = np.where(rng.random((B, K)) < 0.3, 0.0, rng.random((B, K))).astype(np.float32)
    w4 = np.where(rng.random((B, K, H, W)) < 0.3, 0.0, rng.random((B, K, H, W))).astype(np.float32)
    mask = (rng.random((B, 1, H, W)) > 0.3).astype(np.float32)
    return dict(output=out, target=tgt, w2=w2, w4=w4, mask=mask)


def heatmap_options():
    """Every option combination of the OKSHeatmapLoss goldens: (oks_type, skip_empty, weights, mask, sw, gw, lw)."""
    out = []
    for i, (ot, skip, wk, mk) in enumerate((ot, skip, wk, mk) for ot in ("minus", "plus", "both")
                                           for skip in (False, True) for wk in (None, "w2", "w4")
                                           for mk in (None, "mask")):
        sw, gw, lw = (0.2, 0.0, 1.0) if i % 2 == 0 else (0.05, 0.3, 2.5)
        out.append((ot, skip, wk, mk, sw, gw, lw))
    return out


def small_inputs(seed: int = 77) -> dict:
    """Inputs of the BCELoss / MSELoss / L1LogLoss goldens.  The L1Log operands are mostly below 0.01, where
    rounding 1 + x to float32 is visible against the loss (log(1 + x), not log1p)."""
    rng = np.random.default_rng(seed)
    s = dict(x=rng.uniform(0.01, 0.99, (6, 5)).astype(np.float32), logits=rng.normal(0, 3, (6, 5)).astype(np.float32),
             y=(rng.random((6, 5)) > 0.5).astype(np.float32), w1=rng.random(6).astype(np.float32),
             w2=rng.random((6, 5)).astype(np.float32), a=rng.normal(0, 1, (4, 5, 2)).astype(np.float32),
             b=rng.normal(0, 1, (4, 5, 2)).astype(np.float32), wm=(rng.random((4, 5, 2)) > 0.3).astype(np.float32))
    for D in (1, 2):
        eo = rng.uniform(0, 1e-3, (4, 3, D)).astype(np.float32)
        et = (eo * rng.uniform(0.5, 1.5, (4, 3, D))).astype(np.float32)
        eo[0, 0], et[0, 0] = 3.0, 0.1                                   # one element in the linear branch ...
        wl = (rng.random((4, 3)) > 0.2).astype(np.float32)
        wl[0, 0] = 0.0                                                  # ... masked out where weights are used
        s[f"eo{D}"], s[f"et{D}"], s[f"wl{D}"] = eo, et, wl
    return s


# ----------------------------------------------------------------------------------------------- OKSHeatmapLoss
def _sobel(o, pad="zero"):
    """gx, gy of F.conv2d(o, sobel, padding='same') (cross-correlation) and the magnitudes of their terms."""
    mode = "constant" if pad == "zero" else "reflect"
    p = np.pad(o, [(0, 0)] * (o.ndim - 2) + [(1, 1), (1, 1)], mode=mode)
    H, W = o.shape[-2:]
    a = lambda dr, dc: p[..., dr:dr + H, dc:dc + W]   # noqa: E731
    sx = [(0, 0, 1), (0, 2, -1), (1, 0, 2), (1, 2, -2), (2, 0, 1), (2, 2, -1)]
    sy = [(0, 0, 1), (0, 1, 2), (0, 2, 1), (2, 0, -1), (2, 1, -2), (2, 2, -1)]
    gx = sum(c * a(r, q) for r, q, c in sx)
    gy = sum(c * a(r, q) for r, q, c in sy)
    ax = sum(abs(c) * np.abs(a(r, q)) for r, q, c in sx)
    ay = sum(abs(c) * np.abs(a(r, q)) for r, q, c in sy)
    return gx, gy, ax, ay


def oks_heatmap_loss(output, target, target_weights=None, mask=None, skip_empty=False, oks_type="minus",
                     sw=0.2, gw=0.0, lw=1.0, *, fault=None) -> dict:
    """loss.py:55-191 in float64.  Returns {'pixel', 'keypoint', 'mean', 'pixel_mean'}: (value, scale, c) each.
    ``fault``: 'reflect' (Sobel with reflect padding), 'drop_weights' (the keypoint mask ignored)."""
    o = np.asarray(output, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    B, K, H, W = o.shape
    om, op = o * (1 - t), (1 - o) * t
    if oks_type == "minus":
        oks, a_oks = om, np.abs(om)
    elif oks_type == "plus":
        oks, a_oks = op, np.abs(op)
    else:
        oks, a_oks = (om + op) / 2, (np.abs(om) + np.abs(op)) / 2
    mse, a_mse = (o - t) ** 2, (np.abs(o) + np.abs(t)) ** 2
    gx, gy, ax, ay = _sobel(o, "reflect" if fault == "reflect" else "zero")
    g, a_g = gx ** 2 + gy ** 2, ax ** 2 + ay ** 2
    m = np.ones((B, K, 1, 1))
    if mask is not None:
        m = m * np.asarray(mask, dtype=np.float64)
    if target_weights is not None and fault != "drop_weights":
        w = np.asarray(target_weights, dtype=np.float64)
        m = m * w.reshape(w.shape + (1,) * (4 - w.ndim))
    if skip_empty:
        m = m * (t != 0).reshape(B, K, -1).any(axis=2)[..., None, None]
    am = np.abs(m)
    oks, mse, g = oks * m, mse * m, g * m
    a_oks, a_mse, a_g = a_oks * am, a_mse * am, a_g * am
    ow = 1 - sw - gw
    pix = (sw * g + ow * oks + gw * mse) * lw
    a_pix = (abs(sw) * a_g + abs(ow) * a_oks + abs(gw) * a_mse) * abs(lw)
    gm = g.reshape(B, K, -1)
    gmax = np.where(np.isnan(gm).any(axis=2), np.nan, gm.max(axis=2))
    a_gmax = a_g.reshape(B, K, -1).max(axis=2)
    kp = (ow * oks.sum(axis=(2, 3)) + sw * gmax + gw * mse.mean(axis=(2, 3))) * lw
    a_kp = (abs(ow) * a_oks.sum(axis=(2, 3)) + abs(sw) * a_gmax + abs(gw) * a_mse.mean(axis=(2, 3))) * abs(lw)
    cs = c_sum(H * W)
    return dict(pixel=(pix, a_pix, C_PIX), keypoint=(kp, a_kp, C_PIX + cs), mean=(kp.mean(), a_kp.mean(), C_PIX + cs + 2),
                pixel_mean=(pix.mean(), a_pix.mean(), C_PIX + cs + 2))


# ----------------------------------------------------------------------------------------------- small losses
def _bce_terms(x, y, use_sigmoid):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if use_sigmoid:         # F.binary_cross_entropy: logs clamped at -100
        with np.errstate(divide="ignore"):
            l0, l1 = np.maximum(np.log(x), -100.0), np.maximum(np.log(1 - x), -100.0)
        return (y - 1) * l1 - y * l0, np.abs((y - 1) * l1) + np.abs(y * l0)
    sp = np.log1p(np.exp(-np.abs(x)))     # F.binary_cross_entropy_with_logits
    return np.maximum(x, 0) - x * y + sp, np.abs(x) + np.abs(x * y) + sp


def bce_loss(output, target, target_weight=None, use_sigmoid=False, use_target_weight=False, reduction="mean",
             loss_weight=1.0):
    """loss.py:194-260."""
    v, a = _bce_terms(output, target, use_sigmoid)
    if use_target_weight:
        w = np.asarray(target_weight, dtype=np.float64)
        if w.ndim == 1:
            w = w[:, None]
        v, a = v * w, a * np.abs(w)
    if reduction == "sum":
        v, a = v.sum(), a.sum()
    elif reduction == "mean":
        v, a = v.mean(), a.mean()
    return v * loss_weight, a * abs(loss_weight), C_MEAN


def mse_loss(output, target, target_weight=None, use_target_weight=False, loss_weight=1.0):
    """loss.py:263-292: the mean over every entry, masked zeros included."""
    a = np.asarray(output, dtype=np.float64)
    b = np.asarray(target, dtype=np.float64)
    if use_target_weight:
        w = np.asarray(target_weight, dtype=np.float64)
        a, b = a * w, b * w
    return ((a - b) ** 2).mean() * loss_weight, ((np.abs(a) + np.abs(b)) ** 2).mean() * abs(loss_weight), C_MEAN


def log1x(x, *, fault=None):
    """torch.log(1 + x) on float32 x: 1 + x is rounded to float32 first.  fault='log1p' drops that rounding."""
    x32 = np.asarray(x, dtype=np.float32)
    if fault == "log1p":
        return np.log1p(x32.astype(np.float64))
    return np.log((np.float32(1) + x32).astype(np.float64))


def l1log_loss(output, target, target_weight=None, use_target_weight=False, loss_weight=1.0, *, fault=None):
    """loss.py:295-339: smooth-L1 (beta 1) of log(1 + x), weights unsqueezed to the operand's rank."""
    a, b = log1x(output, fault=fault), log1x(target, fault=fault)
    if use_target_weight:
        w = np.asarray(target_weight, dtype=np.float64)
        w = w.reshape(w.shape + (1,) * (a.ndim - w.ndim))
        a, b = a * w, b * w
    z = np.abs(a - b)
    v = np.where(z < 1, 0.5 * z * z, z - 0.5)
    s = np.abs(a) + np.abs(b) + z
    a_v = np.where(z < 1, z * s, s)
    return v.mean() * loss_weight, a_v.mean() * abs(loss_weight), C_MEAN


# ----------------------------------------------------------------------------------------------- ProbPoseLoss
def probpose_loss(gt, pred, gt_kpts, dt_kpts, sigmas, freeze_error=True, keypoint_weights=None,
                  learn_heatmaps_from_zeros=False, *, fault=None) -> dict:
    """loss.py:360-640 in float64, fed the decoded gt / dt coordinates (B,K,2) in input-image pixels.

    Returns (value, scale, c) for the five losses and for the B*K intermediates (gt_oks, gt_err, vis_weight), the
    per-crop oks_weight and the two MAE accuracies.  ``fault``: 'reflect', 'drop_weights' (heatmap loss),
    'unnormalised_vis' (visibility weights not divided by their minimum), 'log1p', 'nan_gt' (gt NaN not zeroed)."""
    dt_hm = np.asarray(pred[0], dtype=np.float32)
    B, K, H, W = dt_hm.shape
    as_int = lambda x: np.asarray(x).astype(np.int64).reshape(B, K)   # noqa: E731
    probs, annotated, vis = as_int(gt["in_image"]), as_int(gt["keypoints_visible"]), as_int(gt["keypoints_visibility"])
    dt_probs, dt_vis, dt_oks, dt_errs = (np.asarray(p, dtype=np.float32).reshape(B, K) for p in pred[1:])
    kw = np.ones((B, K), np.float32) if keypoint_weights is None else np.asarray(keypoint_weights).reshape(B, K)
    out = {}
    # --- targets (loss.py:512-640)
    w = (probs & annotated).astype(np.float64)
    g = np.array(gt_kpts, dtype=np.float64)
    if fault != "nan_gt":
        g[np.isnan(g)] = 0
    g, d = g * w[..., None], np.asarray(dt_kpts, dtype=np.float64) * w[..., None]
    var = (np.asarray(sigmas) * 2) ** 2
    e = ((d - g) ** 2).sum(axis=2) / var / ((W * H) * 0.53 + np.spacing(1)) / 2
    valid = w > 0
    crop = valid.any(axis=1)
    with np.errstate(invalid="ignore"):
        oks = np.where(crop[:, None] & valid, np.exp(-e), 0.0)
    gt_oks = oks.astype(np.float32)
    out["gt_oks"] = (oks, np.abs(oks), C_TARGET)
    out["oks_weight"] = (crop.astype(np.float64), 0.0, C_TARGET)
    if freeze_error:
        err = np.zeros((B, K))
    else:
        ge = np.array(gt_kpts, dtype=np.float64)
        ge[np.isnan(ge)] = -1
        err = np.linalg.norm(ge - np.asarray(dt_kpts, dtype=np.float64), axis=2)
        assert (err >= 0).all(), "Euclidean distance cannot be negative"
    gt_err = err.astype(np.float32)
    out["gt_err"] = (err, np.abs(err), C_TARGET)
    # --- heatmap loss (loss.py:423-431)
    hw = annotated if learn_heatmaps_from_zeros else kw
    hl = oks_heatmap_loss(dt_hm, np.asarray(gt["heatmaps"], np.float32).reshape(B, K, H, W), hw, sw=0.05,
                          fault=fault if fault in ("reflect", "drop_weights") else None)
    out["kpt"] = hl["pixel_mean"]
    out["probability"] = bce_loss(dt_probs, probs, use_sigmoid=True)
    # --- visibility weights (loss.py:436-450)
    annotated_in = annotated & (probs > 0.5)
    invisible_in = (vis == 0) & (annotated > 0.5)
    visible_in = (vis > 0) & (annotated > 0.5)
    wv = annotated_in.astype(np.float64)
    wv[invisible_in] = np.float64(np.float32(1) / (np.float32(invisible_in.sum()) + np.float32(1e-10)))
    wv[visible_in] = np.float64(np.float32(1) / (np.float32(visible_in.sum()) + np.float32(1e-10)))
    if not (wv > 0).any():
        raise RuntimeError("min() of an empty tensor (loss.py:448)")
    if fault != "unnormalised_vis":
        wv = wv / wv[wv > 0].min()
    out["vis_weight"] = (wv, np.abs(wv), C_TARGET)
    out["visibility"] = bce_loss(dt_vis, vis, use_sigmoid=True)    # BCELoss(use_target_weight=False): weights unused
    out["oks"] = mse_loss(dt_oks, gt_oks, annotated_in, use_target_weight=True)
    out["error"] = l1log_loss(dt_errs, gt_err, annotated_in, use_target_weight=True,
                              fault="log1p" if fault == "log1p" else None)
    sel = annotated_in > 0.5
    for key, dt_, gt_ in (("mae_oks", dt_oks, gt_oks), ("mae_err", dt_errs, gt_err)):
        a, b = dt_[sel].astype(np.float64), gt_[sel].astype(np.float64)
        with np.errstate(invalid="ignore"):
            out[key] = (np.abs(a - b).mean() if a.size else np.nan,
                        (np.abs(a) + np.abs(b)).mean() if a.size else 0.0, C_MEAN)
    return out
