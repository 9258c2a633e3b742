"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of the steps of ``Augment`` that DESIGN §4.4d specifies: the
box / median blur and the holes of ``pp_augment_post``, the half-body rule and the arithmetic of ``draw_post``.  Written
from the specification, not from the kernel or from ``dataset.py``; the uniforms are an argument, so the rules are
restated without a generator.

``fault`` plants a mistake in ``half_body``, for the tests that must reject one:
  "unlabelled"     the chosen half takes its keypoints whether they are labelled or not
  "pad_centre"     the padding factor is applied to the centre as well as to the extents
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
WORDS = 24
BOX_SIZES, MEDIAN_SIZES = (3, 5, 7), (3, 5)


def reflect101(i, n):
    """Index -i reads i, index n - 1 + i reads n - 1 - i (one reflection: |offset| <= n - 1)."""
    i = np.abs(np.asarray(i))
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def windows(plane, k):
    """(h, w, k * k): the k x k window of every pixel of a 2-D plane under reflect-101 borders."""
    h, w = plane.shape
    assert k % 2 == 1 and k <= min(h, w)
    r = k // 2
    ys = reflect101(np.arange(-r, h + r), h)
    xs = reflect101(np.arange(-r, w + r), w)
    ext = plane[np.ix_(ys, xs)]
    return np.stack([ext[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)], -1)


def box_mean(img, k):
    """float64 mean of the k x k window, img (..., h, w)."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape[-2:]
    assert k % 2 == 1 and k <= min(h, w)
    r = k // 2
    ext = img[..., reflect101(np.arange(-r, h + r), h), :][..., reflect101(np.arange(-r, w + r), w)]
    total = np.zeros_like(img)
    for dy in range(k):
        for dx in range(k):
            total += ext[..., dy:dy + h, dx:dx + w]
    return total / (k * k)


def median(img, k):
    """np.median of the k x k window (odd count: an element of it), in the dtype of img."""
    img = np.asarray(img)
    flat = img.reshape(-1, *img.shape[-2:])
    return np.stack([np.median(windows(p, k), axis=-1) for p in flat]).reshape(img.shape).astype(img.dtype)


def box_bound(k):
    """|float32 mean - float64 mean| on inputs in [0, 1]: at most k^2 - 1 additions, each rounding a partial sum of at
    most k^2 (error <= k^2 u each, (k^2 - 1) u after the division by k^2), then the division's own rounding of a value
    of at most 1 (u): k^2 u in any summation order."""
    return k * k * U


def fill_of(record):
    return np.asarray(record[3:4], dtype=np.int32).view(np.float32)[0]


def apply(img, record, filters):
    """One sample (3, h, w) through §4.4d's two steps.  Returns (result, is_box): the result in float64 where a box
    mean was taken (compare within ``box_bound``), else in the dtype of img (compare bit for bit)."""
    kind, k, n_holes = (int(v) for v in record[:3])
    out, is_box = np.array(img), False
    if filters and kind == 1:
        out, is_box = box_mean(img, k), True
    elif filters and kind == 2:
        out = median(img, k)
    for j in range(n_holes):
        x0, y0, x1, y1 = (int(v) for v in record[4 + 4 * j:8 + 4 * j])
        out[:, y0:y1, x0:x1] = fill_of(record)
    return out, is_box


def record(kind=0, k=0, holes=(), fill=0.0):
    rec = np.zeros(WORDS, dtype=np.int32)
    rec[0], rec[1], rec[2] = kind, k, len(holes)
    rec[3] = np.float32(fill).view(np.int32)
    for j, h in enumerate(holes):
        rec[4 + 4 * j:8 + 4 * j] = h
    return rec


# ---- draw_post's arithmetic from its 20 uniforms ---------------------------------------------------------------------------
def post_record(r, input_size, blur_prob=0.0, blur_kernel=(3, 7), median_prob=0.0, median_kernel=(3, 5),
                erase_prob=0.0, erase_holes=(1, 1), erase_size=(0.2, 0.4), erase_fill=0.0):
    in_w, in_h = input_size
    kind = 1 if r[0] < blur_prob else 2 if r[0] < blur_prob + median_prob else 0
    k = 0
    if kind:
        lo, hi = blur_kernel if kind == 1 else median_kernel
        sizes = [s for s in range(lo, hi + 1) if s % 2 == 1]
        k = sizes[min(int(r[1] * len(sizes)), len(sizes) - 1)]
    lo, hi = erase_holes
    n = lo + min(int(r[3] * (hi - lo + 1)), hi - lo) if r[2] < erase_prob else 0
    holes = []
    for j in range(n):
        q = r[4 + 4 * j:8 + 4 * j]
        w = int(np.clip(np.rint((erase_size[0] + q[0] * (erase_size[1] - erase_size[0])) * in_w), 1, in_w))
        h = int(np.clip(np.rint((erase_size[0] + q[1] * (erase_size[1] - erase_size[0])) * in_h), 1, in_h))
        x0, y0 = min(int(q[2] * (in_w - w + 1)), in_w - w), min(int(q[3] * (in_h - h + 1)), in_h - h)
        holes.append((x0, y0, x0 + w, y0 + h))
    return record(kind, k, holes, erase_fill)


# ---- the half-body rule from its 2 uniforms --------------------------------------------------------------------------------
def half_body(r, keypoints, bbox, upper_body, prob, min_keypoints=9, padding=1.5, fault=None):
    """Returns (box float64 [x, y, w, h], chosen): ``chosen`` the indices of the labelled keypoints the box was built
    from, or None where the original box is returned."""
    kps = np.asarray(keypoints, dtype=np.float64)
    bbox = np.asarray(bbox, dtype=np.float64)
    K = len(kps)
    labelled = [i for i in range(K) if kps[i, 2] > 0]
    if not (r[0] < prob and len(labelled) >= min_keypoints):
        return bbox, None
    upper = [i for i in labelled if i in upper_body]
    lower = [i for i in labelled if i not in upper_body]
    if len(upper) >= 2 and len(lower) >= 3:
        take_upper = r[1] < 0.7
    elif len(upper) >= 2:
        take_upper = True
    elif len(lower) >= 3:
        take_upper = False
    else:
        return bbox, None
    chosen = upper if take_upper else lower
    pts = chosen
    if fault == "unlabelled":
        pts = [i for i in range(K) if (i in upper_body) == take_upper]
    xs, ys = kps[pts, 0], kps[pts, 1]
    cx, cy = (xs.min() + xs.max()) / 2, (ys.min() + ys.max()) / 2
    if fault == "pad_centre":
        cx, cy = cx * padding, cy * padding
    w = max((xs.max() - xs.min()) * padding, 0.25 * bbox[2])
    h = max((ys.max() - ys.min()) * padding, 0.25 * bbox[3])
    return np.array([cx - w / 2, cy - h / 2, w, h]), chosen


def box_contains(box, points):
    x, y, w, h = box
    p = np.asarray(points, dtype=np.float64)
    return bool(((p[:, 0] >= x) & (p[:, 0] <= x + w) & (p[:, 1] >= y) & (p[:, 1] <= y + h)).all())
