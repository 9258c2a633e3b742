"""The rules of probpose_pytorch_amd/viz.py restated in numpy: float32 and float64 exactly where the rules say so,
integers for the drawing.  Written from the rules, not from the kernels (probpose_pytorch_amd/csrc/pp_viz.hip); pinned
on the reference's overlay_heatmap_on_image, on matplotlib and on PIL by tests/test_viz_reference.py, and the gauge of
tests/test_viz_gpu.py.  ``fault=`` plants one deliberate error, for the tests that show the checks can see it."""
import json
import os

import numpy as np

THRESHOLD = np.float32(0.01)
TABLE_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "probpose_pytorch_amd", "data",
                          "colormaps.json")


def table(name):
    with open(TABLE_FILE) as f:
        return np.asarray(json.load(f)[name], dtype=np.float64)


# ---- colour ----------------------------------------------------------------------------------------------------------
def lut_rows(v):
    """float32 array -> the row of the [256, 3] table, -1 for NaN (matplotlib's Colormap.__call__)."""
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        xa = v * np.float32(256.0)
        rows = np.where(xa < 0, 0, np.where(xa >= 256, 255, np.trunc(np.where(np.isfinite(xa), xa, 0)))).astype(np.int64)
    return np.where(np.isnan(xa), -1, rows)


def colours(v, lut):
    """float32 [...] -> float64 [..., 3]; NaN gives (0, 0, 0)."""
    rows = lut_rows(v)
    return np.where((rows < 0)[..., None], 0.0, lut[np.maximum(rows, 0)])


def upsample(hm, H, W):
    """float32 [K, h, w] -> float32 [K, H, W]: the maps themselves at their own size, else bilinear in float64."""
    K, h, w = hm.shape
    if (h, w) == (H, W):
        return hm

    def axis(n_out, n_in):
        u = np.arange(n_out, dtype=np.float64) * (n_in - 1) / (n_out - 1) if n_out > 1 else np.zeros(1)
        i0 = np.minimum(np.floor(u).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), u - i0

    y0, y1, fy = axis(H, h)
    x0, x1, fx = axis(W, w)
    a = hm.astype(np.float64)
    fy, fx = fy[None, :, None], fx[None, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        top = a[:, y0][:, :, x0] * (1.0 - fx) + a[:, y0][:, :, x1] * fx
        bot = a[:, y1][:, :, x0] * (1.0 - fx) + a[:, y1][:, :, x1] * fx
        return (top * (1.0 - fy) + bot * fy).astype(np.float32)


def image_bytes(x):
    """float32 [3, H, W] in [0, 1] -> uint8 [H, W, 3]: trunc(min(max(v * 255 + 0.5, 0), 255)) in float32, NaN -> 0."""
    assert x.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * np.float32(255.0) + np.float32(0.5)
        t = np.where(t > 0, t, np.float32(0.0))
        t = np.where(t < 255, t, np.float32(255.0))
    return np.ascontiguousarray(t.astype(np.uint8).transpose(1, 2, 0))


def overlay(image, heat, lut, fault=None):
    """uint8 [H, W, 3] (or float32 [3, H, W]) with float32 [K, h, w] -> uint8 [H, W, 3]."""
    if image.dtype == np.float32:
        image = image_bytes(image)
    H, W = image.shape[:2]
    v = upsample(heat, H, W)
    acc = np.zeros((H, W, 3), dtype=np.float64)
    ks = range(v.shape[0])
    for k in (reversed(ks) if fault == "descending_k" else ks):
        c = colours(v[k], lut)
        with np.errstate(invalid="ignore"):
            zero = v[k] <= THRESHOLD if fault == "le_threshold" else v[k] < THRESHOLD
        c[zero] = 0.0
        acc = acc + c
    s = acc * 255.0
    if fault == "wrap":
        return ((image.astype(np.int64) + s.astype(np.int64) % 256) % 256).astype(np.uint8)
    add = np.where(s < 255.0, s, 255.0).astype(np.int64)
    return np.minimum(255, image.astype(np.int64) + add).astype(np.uint8)


def colorize(maps, lut, normalize=False):
    """float32 [..., h, w] -> uint8 [..., h, w, 4]."""
    maps = np.asarray(maps, dtype=np.float32)
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            maps = (maps / maps.max(axis=(-2, -1), keepdims=True)).astype(np.float32)
    rows = lut_rows(maps)
    out = np.empty(maps.shape + (4,), dtype=np.uint8)
    out[..., :3] = (lut[np.maximum(rows, 0)] * 255.0).astype(np.uint8)
    out[..., 3] = 255
    out[rows < 0] = 0
    return out


# ---- drawing ---------------------------------------------------------------------------------------------------------
def centre(kp, prob, threshold, H, W):
    """(x, y) of a drawn keypoint or None: the reference's loop, inference.py:115-125."""
    if prob < threshold:
        return None
    if not (abs(kp[0]) < 2.0 ** 31 and abs(kp[1]) < 2.0 ** 31):          # NaN, inf, too large
        return None
    x, y = int(kp[0]), int(kp[1])
    return (x, y) if 0 <= x < W and 0 <= y < H else None


def disc_mask(H, W, x, y, r, fault=None):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    return (xx - x) ** 2 + (yy - y) ** 2 <= (r * r if fault == "r2" else r * r + r)


def limb_mask(H, W, a, b, line_width):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    dx, dy = b[0] - a[0], b[1] - a[1]
    L2 = dx * dx + dy * dy
    ex, ey = xx - a[0], yy - a[1]
    t = ex * dx + ey * dy
    cross = ex * dy - ey * dx
    lw2 = line_width * line_width
    return np.where(t <= 0, 4 * (ex * ex + ey * ey) <= lw2,
                    np.where(t >= L2, 4 * ((xx - b[0]) ** 2 + (yy - b[1]) ** 2) <= lw2, 4 * cross * cross <= lw2 * L2))


def _window(mask_fn, H, W, x0, x1, y0, y1, *args):
    """``mask_fn`` evaluated on the window [y0, y1] x [x0, x1] of the image only (the primitives are small)."""
    x0, x1, y0, y1 = max(x0, 0), min(x1, W - 1), max(y0, 0), min(y1, H - 1)
    full = np.zeros((H, W), dtype=bool)
    if x0 <= x1 and y0 <= y1:
        shifted = [(p[0] - x0, p[1] - y0) if isinstance(p, tuple) else p for p in args]
        full[y0:y1 + 1, x0:x1 + 1] = mask_fn(y1 - y0 + 1, x1 - x0 + 1, *shifted)
    return full


def draw(images, keypoints, probabilities, *, threshold=0.9, radius=5, colors=(255, 0, 0), skeleton=None,
         limb_colors=None, line_width=2, image_index=None, fault=None):
    """uint8 [B, H, W, 3] -> a drawn copy.  Painter's order: all limbs (instance, then skeleton order), then all
    discs (instance, then keypoint): what is painted later covers what was painted earlier."""
    out = np.array(images, dtype=np.uint8, copy=True)
    B, H, W = out.shape[:3]
    kp, pr = np.asarray(keypoints, dtype=np.float64), np.asarray(probabilities, dtype=np.float64)
    N, K = pr.shape
    index = np.arange(B) if image_index is None else np.asarray(image_index)
    colors = np.broadcast_to(np.asarray(colors, dtype=np.uint8), (K, 3))
    skeleton = [] if skeleton is None else [tuple(int(v) for v in s) for s in skeleton]
    if limb_colors is not None:
        limb_colors = np.broadcast_to(np.asarray(limb_colors, dtype=np.uint8), (len(skeleton), 3))
    pad = (line_width + 1) // 2

    def limbs():
        for n in range(N):
            c = [centre(kp[n, k], pr[n, k], threshold, H, W) for k in range(K)]
            for l, (i, j) in enumerate(skeleton):
                if c[i] is None or c[j] is None or c[i] == c[j]:
                    continue
                a, b = c[i], c[j]
                mask = _window(limb_mask, H, W, min(a[0], b[0]) - pad, max(a[0], b[0]) + pad, min(a[1], b[1]) - pad,
                               max(a[1], b[1]) + pad, a, b, line_width)
                out[index[n]][mask] = colors[i] if limb_colors is None else limb_colors[l]

    def discs():
        for n in range(N):
            for k in range(K):
                c = centre(kp[n, k], pr[n, k], threshold, H, W)
                if c is not None:
                    mask = _window(lambda h, w, p, r: disc_mask(h, w, p[0], p[1], r, fault), H, W, c[0] - radius,
                                   c[0] + radius, c[1] - radius, c[1] + radius, c, radius)
                    out[index[n]][mask] = colors[k]

    for step in ((discs, limbs) if fault == "discs_under_limbs" else (limbs, discs)):
        step()
    return out


def render(images, heat, lut, keypoints, probabilities, **kw):
    """Overlay, then draw: uint8 [B, H, W, 3] with float32 [B, K, h, w]."""
    return draw(np.stack([overlay(im, hm, lut) for im, hm in zip(images, heat)]), keypoints, probabilities, **kw)


# ---- inputs shared by the golden file's script and the tests ---------------------------------------------------------
GOLDEN_SEED, GOLDEN_SHAPE = 2026, (3, 5, 24, 20)


def golden_inputs(colormap, seed=GOLDEN_SEED):
    """(images uint8 [3, 24, 20, 3] below 128, maps float32 [3, 5, 24, 20]) on which the reference's overlay cannot
    wrap (called with an int64 image): image 0 and 1 have disjoint supports above the threshold (image 0 with the
    special values), image 2 has overlapping maps whose per-channel colour sums stay below 1 for ``colormap``."""
    B, K, h, w = GOLDEN_SHAPE
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 128, (B, h, w, 3), dtype=np.uint8)
    owner = rng.integers(0, K, (B, h, w))
    maps = np.zeros(GOLDEN_SHAPE, dtype=np.float32)
    for b in range(2):
        full = rng.random((K, h, w), dtype=np.float32)
        below = (rng.random((K, h, w), dtype=np.float32) * np.float32(0.0099)).astype(np.float32)
        maps[b] = np.where(owner[b][None] == np.arange(K)[:, None, None], full, below)
    lo = np.nextafter(THRESHOLD, np.float32(0))
    special = [1.0, np.nan, -0.5, 1.5, THRESHOLD, lo, np.nextafter(THRESHOLD, np.float32(1)), 0.0, -0.0, 0.5,
               np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(1), np.float32(0))]
    for i, v in enumerate(special):              # one special value a pixel, in the map that owns the pixel
        maps[0, owner[0, 0, i], 0, i] = v
        maps[0, owner[0, 1, i], 1, i] = v
        maps[0, (owner[0, 1, i] + 1) % K, 1, i] = lo
    if colormap == "jet":                        # blue only (0.02 - 0.10) over red only (0.92 - 1): sums below 1
        maps[2, 0] = np.float32(0.02) + rng.random((h, w), dtype=np.float32) * np.float32(0.08)
        maps[2, 3] = np.float32(0.92) + rng.random((h, w), dtype=np.float32) * np.float32(0.08)
    else:                                        # inferno is dark below 0.15: three maps sum below 1
        for k in (0, 2, 4):
            maps[2, k] = np.float32(0.01) + rng.random((h, w), dtype=np.float32) * np.float32(0.14)
    return images, maps
