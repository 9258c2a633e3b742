"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of the augmentation of ``YOLOPoseDataset(augment=Augment(...))``,
written from its specification, not from the kernels or from ``dataset.augment_matrices``.

Geometry, for output pixel (u, v) of an in_w x in_h crop, parameters [flip, s, theta, tx, ty, c, b], box [x, y, bw, bh]:
  1. n = ((u + 0.5) / in_w - 0.5, (v + 0.5) / in_h - 0.5)
  2. with flip, n.x = -n.x
  3. p = (n.x * bw * s, n.y * bh * s)
  4. source = centre + (tx * bw, ty * bh) + R(theta) p, image pixels with pixel centres at half-integers
The pixel matrix is read off ``source_point`` at three output pixels (the map is affine); the keypoint matrix is the
chain of the inverse steps.  Neither is a closed form shared with the product.

``fault`` plants a mistake, for the tests that must reject one:
  "theta_sign"      the keypoint matrix rotates the wrong way
  "swap_no_mirror"  a flipped sample swaps its keypoint slots but does not mirror their coordinates
  "mirror_no_swap"  a flipped sample mirrors the coordinates but leaves the slots alone
"""
from __future__ import annotations

import numpy as np


def rotation(theta):
    return np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])


def source_point(u, v, bbox, params, in_size):
    """Steps 1-4: the image-pixel point (continuous; pixel i covers [i, i + 1)) that output pixel (u, v) shows."""
    x, y, bw, bh = (float(t) for t in bbox)
    flip, s, theta, tx, ty = (float(t) for t in params[:5])
    n = np.array([(u + 0.5) / in_size[0] - 0.5, (v + 0.5) / in_size[1] - 0.5])
    if flip:
        n[0] = -n[0]
    p = np.array([n[0] * bw * s, n[1] * bh * s])
    return np.array([x + bw / 2, y + bh / 2]) + np.array([tx * bw, ty * bh]) + rotation(theta) @ p


def pixel_matrix(bbox, origin, params, in_size):
    """2x3: output pixel index (u, v, 1) -> pixel-index coordinates in the region whose corner pixel is ``origin``
    (pixel (i, j) of the region centred at (i, j): the source point minus the origin minus 0.5)."""
    o = source_point(0, 0, bbox, params, in_size)
    du = source_point(1, 0, bbox, params, in_size) - o
    dv = source_point(0, 1, bbox, params, in_size) - o
    return np.stack([du, dv, o - np.asarray(origin, dtype=np.float64) - 0.5], axis=1)


def keypoint_matrix(bbox, params, in_size, fault=None):
    """2x3: image-pixel keypoint (kx, ky, 1) -> crop coordinates (left edge 0, right edge in_w), by undoing steps 4
    to 1 one after the other as 3x3 matrices."""
    x, y, bw, bh = (float(t) for t in bbox)
    flip, s, theta, tx, ty = (float(t) for t in params[:5])
    if fault == "theta_sign":
        theta = -theta
    if fault == "swap_no_mirror":
        flip = 0.0

    def mat(a, t):
        m = np.eye(3)
        m[:2, :2], m[:2, 2] = a, t
        return m

    centre = np.array([x + bw / 2 + tx * bw, y + bh / 2 + ty * bh])
    undo4 = mat(rotation(-theta), [0, 0]) @ mat(np.eye(2), -centre)
    undo3 = mat(np.diag([1 / (bw * s), 1 / (bh * s)]), [0, 0])
    undo2 = mat(np.diag([-1.0 if flip else 1.0, 1.0]), [0, 0])
    undo1 = mat(np.diag([float(in_size[0]), float(in_size[1])]), [in_size[0] / 2, in_size[1] / 2])
    return (undo1 @ undo2 @ undo3 @ undo4)[:2]


def as3(m):
    return np.vstack([m, [0.0, 0.0, 1.0]])


def matrix_product(bbox, origin, params, in_size):
    """keypoint matrix x (region index -> image point) x pixel matrix x (crop coordinate -> output index): the
    identity when the two matrices are inverse to each other."""
    to_image = np.array([[1, 0, origin[0] + 0.5], [0, 1, origin[1] + 0.5], [0, 0, 1.0]])
    to_index = np.array([[1, 0, -0.5], [0, 1, -0.5], [0, 0, 1.0]])
    return as3(keypoint_matrix(bbox, params, in_size)) @ to_image @ as3(pixel_matrix(bbox, origin, params, in_size)) @ to_index


def permutation(flip_pairs, K):
    perm = np.arange(K)
    used = []
    for i, j in flip_pairs:
        if i == j or i in used or j in used or not (0 <= i < K and 0 <= j < K):
            raise ValueError(f"flip pair ({i}, {j})")
        used += [i, j]
        perm[i], perm[j] = j, i
    return perm


def warp(src, m, c, b, in_size, tap_offset=(0, 0)):
    """Bilinear sampling + colour step in float64.  src uint8 (h, w, 3); m 2x3 as ``pixel_matrix``; the taps of output
    pixel (u, v) are the pixels floor(x) + tap_offset[0], + 1 (and y) of ``src``, zero outside it.  Returns
    (3, in_h, in_w) float64 = clamp(c * value / 255 + b, 0, 1)."""
    in_w, in_h = in_size
    h, w = src.shape[:2]
    vv, uu = np.mgrid[0:in_h, 0:in_w].astype(np.float64)
    x = (m[0, 0] * uu + m[0, 1] * vv) + m[0, 2]
    y = (m[1, 0] * uu + m[1, 1] * vv) + m[1, 2]
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    ix, iy = x0.astype(np.int64) + int(tap_offset[0]), y0.astype(np.int64) + int(tap_offset[1])

    def tap(jx, jy):
        inside = (jx >= 0) & (jx < w) & (jy >= 0) & (jy < h)
        px = src[np.clip(jy, 0, h - 1), np.clip(jx, 0, w - 1)].astype(np.float64)
        return np.where(inside[..., None], px, 0.0)

    top = tap(ix, iy) * (1 - fx)[..., None] + tap(ix + 1, iy) * fx[..., None]
    bot = tap(ix, iy + 1) * (1 - fx)[..., None] + tap(ix + 1, iy + 1) * fx[..., None]
    val = (top * (1 - fy)[..., None] + bot * fy[..., None]) / 255.0
    return np.clip(c * val + b, 0.0, 1.0).transpose(2, 0, 1)


def warp_bound(c, b):
    """Counted first-order bound on |kernel - warp| in units of u = 2^-24, values in [0, 1].  In units of the 0..255
    tap scale: each float32 weight is off by at most 2 u (fx rounded, then 1 - fx rounded); a horizontal blend
    p0 * w0 + p1 * w1 then carries 4 u from its weights, 1 u from its two products (w0 + w1 = 1) and 1 u from its sum
    = 6 u; the vertical blend adds the same again on top of what it carries over = 12 u; the division by 255 adds
    1 u = 13 u of a value in [0, 1].  c * x + b with c and b rounded to float32: 13 |c| carried, |c| from rounding c,
    |c| from the product, |b| from rounding b, |c| + |b| from the sum = 16 |c| + 2 |b|.  One more u covers the
    second-order terms and a last-bit difference between two float64 matrices of the same geometry (1e-12 pixel
    against a slope of at most |c| per pixel).  The clamp is exact and does not increase a difference."""
    return (16.0 * abs(c) + 2.0 * abs(b) + 1.0) * 2.0 ** -24


def keypoints(kps_raw, bbox, params, perm, in_size, scale_factor, fault=None):
    """The keypoint path in float64.  kps_raw (K, 3) in image pixels -> dict of crop (K, 2), hm (K, 2), in_image,
    visible (K,) bool, visibility (K,) and ``bound`` (K, 2): the counted float32 bound on the crop coordinates."""
    kps_raw = np.asarray(kps_raw, dtype=np.float64)
    a = keypoint_matrix(bbox, params, in_size, fault)
    swap = bool(params[0]) and fault != "mirror_no_swap"
    src = kps_raw[np.asarray(perm)] if swap else kps_raw
    kx, ky, v = src[:, 0], src[:, 1], src[:, 2]
    crop = np.stack([(a[0, 0] * kx + a[0, 1] * ky) + a[0, 2], (a[1, 0] * kx + a[1, 1] * ky) + a[1, 2]], -1)
    # float32 evaluation of (a0 * kx + a1 * ky) + a2 with the matrix rounded to float32: a0 and a1 rounded (1 u of
    # each product), the two products (1 u each), their sum (1 u), a2 rounded (1 u), the final sum (1 u); 1e-9 pixel
    # for a last-bit difference between two float64 matrices of the same geometry
    u = 2.0 ** -24
    bound = np.stack([u * (2 * abs(a[r, 0] * kx) + 2 * abs(a[r, 1] * ky) + abs(a[r, 0] * kx + a[r, 1] * ky)
                           + abs(a[r, 2]) + abs(crop[:, r])) * (1 + 2.0 ** -10) + 1e-9 for r in (0, 1)], -1)
    scale = np.asarray(scale_factor, dtype=np.float32).astype(np.float64)
    in_image = (crop[:, 0] >= 0) & (crop[:, 0] < in_size[0]) & (crop[:, 1] >= 0) & (crop[:, 1] < in_size[1])
    return dict(crop=crop, hm=crop / scale, in_image=in_image, visible=v == 2, visibility=np.minimum(v, 1.0),
                bound=bound, hm_bound=bound / scale + u * np.abs(crop / scale) * (1 + 2.0 ** -10))


def border_margin(crop, in_size):
    """Distance of every crop coordinate from the nearest border value (0 or the size) of its axis."""
    size = np.asarray(in_size, dtype=np.float64)
    return np.minimum(np.abs(crop), np.abs(crop - size))


def region_rect(bbox, params):
    """(x0, y0, x1, y1): the bounding rectangle of the transformed box's corners, rounded outward, plus the one pixel a
    bilinear tap next to the edge reaches."""
    x, y, bw, bh = (float(t) for t in bbox)
    _, s, theta, tx, ty = (float(t) for t in params[:5])
    centre = np.array([x + bw / 2 + tx * bw, y + bh / 2 + ty * bh])
    corners = np.array([centre + rotation(theta) @ np.array([sx * bw * s / 2, sy * bh * s / 2])
                        for sx in (-1, 1) for sy in (-1, 1)])
    lo, hi = np.floor(corners.min(0)).astype(int) - 1, np.ceil(corners.max(0)).astype(int) + 1
    return int(lo[0]), int(lo[1]), int(hi[0]), int(hi[1])


def sample(frame, ann_bbox, kps_raw, params, perm, in_size, scale_factor):
    """The restated augmented sample from the whole frame (zero outside it): (img (3, h, w) f64, keypoints dict)."""
    x0, y0, _, _ = region_rect(ann_bbox, params)
    m = pixel_matrix(ann_bbox, (x0, y0), params, in_size)
    img = warp(frame, m, params[5], params[6], in_size, tap_offset=(x0, y0))
    return img, keypoints(kps_raw, ann_bbox, params, perm, in_size, scale_factor)


# ---- what tests/test_augment.py and tests/test_augment_gpu.py share ------------------------------------------------------
# K = 20 of tests/dataset_reference.py: eight left / right pairs, keypoints 0, 17, 18 and 19 on the axis
FLIP_PAIRS = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]
# [flip, s, theta, tx, ty, c, b]; no entry is the identity, so that the tree's keypoints "exactly on 0 and on in_w" are
# moved off the crop's border (the flags are compared exactly: see border_margin)
PARAM_GRID = np.array([
    [0, 0.80, 0.0, 0.0, 0.0, 1.0, 0.0],
    [1, 1.23, 0.0, 0.0, 0.0, 1.0, 0.0],
    [0, 1.00, 0.5, 0.0, 0.0, 1.1, -0.1],
    [1, 1.00, -0.5, 0.0, 0.0, 0.9, 0.1],
    [0, 0.77, 0.69, 0.05, -0.07, 1.2, 0.2],
    [1, 1.25, -0.69, -0.1, 0.1, 0.8, -0.2],
    [1, 0.90, 0.31, 0.03, 0.02, 1.0, 0.0],
    [0, 1.10, -0.2, 0.0, 0.1, 1.15, 0.05],
], dtype=np.float64)
MARGIN = 1e-3        # every restated crop coordinate stays this far from 0 and from the size, or the inputs are unfit
