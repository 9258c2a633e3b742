"""The gauge of CocoKeypointEval: COCO keypoint evaluation restated in plain loops over numpy float64.

Written from the rules, not from the kernels (probpose_pytorch_amd/csrc/pp_cocoeval.hip) and not from any evaluation
package.  Four steps:

  compute_oks(dt_kpts, gt_kpts, gt_bbox, gt_area, sigmas)            -> [D, G] similarities
  evaluate_image(image, sigmas, area_range, thresholds, max_dets)    -> the matching of one image in one area range
  accumulate(results, recall_thresholds)                             -> precision [T, R], recall [T] of one area range
  summarize(precision [T, R, A], recall [T, A], thresholds)          -> the ten stats

An ``image`` is a dict of arrays: gt_kpts [G, K, 3], gt_bbox [G, 4], gt_area [G], gt_crowd [G], dt_kpts [D, K, 2|3],
dt_score [D], dt_area [D].  ``evaluate`` chains the four steps over a list of images (their order is the insertion
order that breaks ties between equal scores of different images).

The three switches (``tie_first``, ``early_stop``, ``envelope``) exist so that tests/test_cocoeval_reference.py can
show that the gauge tells the rule from its mutation; their defaults are the rules.
"""
import numpy as np

EPS = float(np.spacing(1.0))
OKS_THRESHOLDS = np.linspace(0.5, 0.95, 10)
RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101)
AREA_RANGES = ((0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, medium, large
MAX_DETS = 20
COCO17_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
STATS = ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl")


def compute_oks(dt_kpts, gt_kpts, gt_bbox, gt_area, sigmas):
    """[D, G] float64.  Over the keypoints with v > 0 of a ground truth: e = (dx^2 + dy^2) / (2 sigma)^2 / (area + eps)
    / 2 and OKS = mean(exp(-e)); a ground truth with no such keypoint is scored over all K keypoints by the distance to
    its box grown by its own size on every side."""
    dt_kpts = np.asarray(dt_kpts, dtype=np.float64)
    gt_kpts = np.asarray(gt_kpts, dtype=np.float64)
    gt_bbox = np.asarray(gt_bbox, dtype=np.float64).reshape(-1, 4)
    gt_area = np.asarray(gt_area, dtype=np.float64).reshape(-1)
    variances = (np.asarray(sigmas, dtype=np.float64) * 2) ** 2
    D, G, K = dt_kpts.shape[0], gt_kpts.shape[0], len(variances)
    out = np.zeros((D, G), dtype=np.float64)
    for g in range(G):
        k1 = 0
        for k in range(K):
            if gt_kpts[g, k, 2] > 0:
                k1 += 1
        size = gt_area[g] + EPS
        bx, by, bw, bh = gt_bbox[g]
        x0, x1 = bx - bw, bx + bw * 2
        y0, y1 = by - bh, by + bh * 2
        for d in range(D):
            total, count = np.float64(0.0), 0
            for k in range(K):
                xd, yd = dt_kpts[d, k, 0], dt_kpts[d, k, 1]
                if k1 > 0:
                    if not gt_kpts[g, k, 2] > 0:
                        continue
                    dx = xd - gt_kpts[g, k, 0]
                    dy = yd - gt_kpts[g, k, 1]
                else:
                    dx = max(np.float64(0.0), x0 - xd) + max(np.float64(0.0), xd - x1)
                    dy = max(np.float64(0.0), y0 - yd) + max(np.float64(0.0), yd - y1)
                e = (dx * dx + dy * dy) / variances[k] / size / 2
                total = total + np.exp(-e)
                count += 1
            out[d, g] = total / count
    return out


def stable_descending(scores):
    """Indices that sort ``scores`` from high to low; equal scores keep their input order."""
    return sorted(range(len(scores)), key=lambda i: -float(scores[i]))       # Python's sort is stable


def evaluate_image(image, sigmas, area_range, thresholds=OKS_THRESHOLDS, max_dets=MAX_DETS, tie_first=False,
                   early_stop=True):
    """The greedy matching of one image in one area range, for every threshold.

    Returns dict(dt_index [D'] (input positions of the kept detections, by descending score), dt_score [D'],
    dt_matched [T, D'], dt_ignore [T, D'], gt_ignore [G] (input order), gt_matched [T, G] (input order), npig,
    oks [D', G] (input order of the ground truths))."""
    lo, hi = area_range
    gt_kpts = np.asarray(image["gt_kpts"], dtype=np.float64)
    G = gt_kpts.shape[0]
    gt_area = np.asarray(image["gt_area"], dtype=np.float64).reshape(-1)
    crowd = np.asarray(image["gt_crowd"]).reshape(-1).astype(bool) if G else np.zeros(0, dtype=bool)
    gt_ignore = np.zeros(G, dtype=bool)
    for g in range(G):
        visible = any(gt_kpts[g, k, 2] > 0 for k in range(gt_kpts.shape[1]))
        gt_ignore[g] = bool(crowd[g]) or not visible or gt_area[g] < lo or gt_area[g] > hi
    gt_order = sorted(range(G), key=lambda g: int(gt_ignore[g]))               # non-ignored first, stable
    dt_score = np.asarray(image["dt_score"], dtype=np.float64).reshape(-1)
    dt_index = stable_descending(dt_score)[:max_dets]
    dt_kpts = np.asarray(image["dt_kpts"], dtype=np.float64)
    dt_area = np.asarray(image["dt_area"], dtype=np.float64).reshape(-1)
    D, T = len(dt_index), len(thresholds)
    kept = dt_kpts[dt_index] if D else np.zeros((0,) + gt_kpts.shape[1:])
    oks = compute_oks(kept, gt_kpts, image["gt_bbox"], gt_area, sigmas) if D and G else np.zeros((D, G))
    dt_matched = np.zeros((T, D), dtype=bool)
    dt_ignore = np.zeros((T, D), dtype=bool)
    gt_matched = np.zeros((T, G), dtype=bool)
    for ti, t in enumerate(thresholds):
        for di in range(D):
            best = min(float(t), 1 - 1e-10)
            m = -1
            for g in gt_order:
                if gt_matched[ti, g] and not crowd[g]:
                    continue
                if early_stop and m > -1 and not gt_ignore[m] and gt_ignore[g]:
                    break
                if oks[di, g] < best or (tie_first and m > -1 and oks[di, g] == best):
                    continue
                best = oks[di, g]
                m = g
            if m > -1:
                gt_matched[ti, m] = True
                dt_matched[ti, di] = True
                dt_ignore[ti, di] = gt_ignore[m]
            else:
                a = dt_area[dt_index[di]]
                dt_ignore[ti, di] = a < lo or a > hi
    return dict(dt_index=np.asarray(dt_index, dtype=np.int64), dt_score=dt_score[dt_index] if D else np.zeros(0),
                dt_matched=dt_matched, dt_ignore=dt_ignore, gt_ignore=gt_ignore, gt_matched=gt_matched,
                npig=int((~gt_ignore).sum()), oks=oks)


def accumulate(results, recall_thresholds=RECALL_THRESHOLDS, envelope=True):
    """precision [T, R] and recall [T] of one area range from the per-image results, in image insertion order."""
    R = len(recall_thresholds)
    T = results[0]["dt_matched"].shape[0] if results else 0
    npig = sum(r["npig"] for r in results)
    if npig == 0:
        return np.full((T, R), -1.0), np.full(T, -1.0)
    scores = [s for r in results for s in r["dt_score"]]
    order = stable_descending(scores)
    precision = np.zeros((T, R), dtype=np.float64)
    recall = np.zeros(T, dtype=np.float64)
    for ti in range(T):
        matched = [m for r in results for m in r["dt_matched"][ti]]
        ignored = [i for r in results for i in r["dt_ignore"][ti]]
        rc, pr = [], []
        tp = fp = 0
        for i in order:
            if ignored[i]:
                continue
            if matched[i]:
                tp += 1
            else:
                fp += 1
            rc.append(np.float64(tp) / np.float64(npig))
            pr.append(np.float64(tp) / (np.float64(tp + fp) + EPS))
        recall[ti] = rc[-1] if rc else 0.0
        if envelope:
            for i in range(len(pr) - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
        for ri, r in enumerate(recall_thresholds):
            value = 0.0
            for i in range(len(rc)):
                if rc[i] >= r:
                    value = pr[i]
                    break
            precision[ti, ri] = value
    return precision, recall


def _mean_present(values):
    total, count = 0.0, 0
    for v in np.asarray(values, dtype=np.float64).reshape(-1):
        if v > -1:
            total += float(v)
            count += 1
    return total / count if count else -1.0


def _at(thresholds, value):
    hits = [i for i, t in enumerate(thresholds) if abs(float(t) - value) < 1e-9]
    return hits[0] if hits else None


def summarize(precision, recall, thresholds=OKS_THRESHOLDS):
    """The ten stats from precision [T, R, A] and recall [T, A]; areas are (all, medium, large)."""
    i50, i75 = _at(thresholds, 0.5), _at(thresholds, 0.75)
    A = precision.shape[2]
    return {
        "AP": _mean_present(precision[:, :, 0]),
        "AP50": _mean_present(precision[i50, :, 0]) if i50 is not None else -1.0,
        "AP75": _mean_present(precision[i75, :, 0]) if i75 is not None else -1.0,
        "APm": _mean_present(precision[:, :, 1]) if A > 1 else -1.0,
        "APl": _mean_present(precision[:, :, 2]) if A > 2 else -1.0,
        "AR": _mean_present(recall[:, 0]),
        "AR50": _mean_present(recall[i50, 0]) if i50 is not None else -1.0,
        "AR75": _mean_present(recall[i75, 0]) if i75 is not None else -1.0,
        "ARm": _mean_present(recall[:, 1]) if A > 1 else -1.0,
        "ARl": _mean_present(recall[:, 2]) if A > 2 else -1.0,
    }


def evaluate(images, sigmas, thresholds=OKS_THRESHOLDS, recall_thresholds=RECALL_THRESHOLDS, area_ranges=AREA_RANGES,
             max_dets=MAX_DETS, tie_first=False, early_stop=True, envelope=True):
    """The four steps over a list of images: the ten stats plus "precision" [T, R, A], "recall" [T, A] and
    "per_image" [A][image] (the evaluate_image results)."""
    T, R, A = len(thresholds), len(recall_thresholds), len(area_ranges)
    precision = np.zeros((T, R, A))
    recall = np.zeros((T, A))
    per_image = []
    for a, rng in enumerate(area_ranges):
        results = [evaluate_image(im, sigmas, rng, thresholds, max_dets, tie_first=tie_first, early_stop=early_stop)
                   for im in images]
        per_image.append(results)
        if results:
            precision[:, :, a], recall[:, a] = accumulate(results, recall_thresholds, envelope=envelope)
        else:
            precision[:, :, a], recall[:, a] = -1.0, -1.0
    out = summarize(precision, recall, thresholds)
    out.update(precision=precision, recall=recall, per_image=per_image)
    return out


# ------------------------------------------------------------------------------------------------ fixtures
def shift_for_oks(oks, sigma, area):
    """The shift d of every keypoint (along x) that gives this OKS when all sigmas are equal:
    d^2 = -ln(OKS) * 2 (2 sigma)^2 area."""
    return float(np.sqrt(-np.log(oks) * 2 * (2 * sigma) ** 2 * area))


def make_image(gt_kpts=None, gt_bbox=None, gt_area=None, gt_crowd=None, dt_kpts=None, dt_score=None, dt_area=None,
               K=17):
    """An image dict with empty arrays for whatever is not given."""
    gt_kpts = np.zeros((0, K, 3)) if gt_kpts is None else np.asarray(gt_kpts, dtype=np.float64)
    G = gt_kpts.shape[0]
    dt_kpts = np.zeros((0, K, 2)) if dt_kpts is None else np.asarray(dt_kpts, dtype=np.float64)
    D = dt_kpts.shape[0]
    return dict(gt_kpts=gt_kpts,
                gt_bbox=np.zeros((G, 4)) if gt_bbox is None else np.asarray(gt_bbox, dtype=np.float64).reshape(G, 4),
                gt_area=np.zeros(G) if gt_area is None else np.asarray(gt_area, dtype=np.float64).reshape(G),
                gt_crowd=np.zeros(G, dtype=bool) if gt_crowd is None else np.asarray(gt_crowd).astype(bool).reshape(G),
                dt_kpts=dt_kpts,
                dt_score=np.zeros(D) if dt_score is None else np.asarray(dt_score, dtype=np.float64).reshape(D),
                dt_area=np.zeros(D) if dt_area is None else np.asarray(dt_area, dtype=np.float64).reshape(D))


def default_sigmas(K):
    return COCO17_SIGMAS.copy() if K == 17 else np.full(K, 0.05)


def random_image(rng, K, G, D, crowd_p=0.1, zero_visible=False, duplicate_gt=False, equal_scores=False,
                 compact=False):
    """A seeded image: people of varied size (small, medium and large areas), detections that are jittered copies of
    ground truths (jitter relative to the person's size, so the OKS values spread over (0, 1)) or strays.

    ``compact`` puts every keypoint of the image, ground truth or detection, into one square of side 0.208 s (s = the
    smallest person's side): with area = 0.6 s^2 and sigma >= 0.025, e = d^2 / (2 sigma)^2 / area / 2 <=
    2 * 0.208^2 / (0.0025 * 0.6 * 2) < 29 for EVERY (detection, ground truth) pair, which is what the OKS bound of
    tests/test_cocoeval_gpu.py asks of its fixture.  ``duplicate_gt`` makes ground truth 1 a bit-identical copy of
    ground truth 0; ``zero_visible`` clears every visibility of the last ground truth."""
    sig = default_sigmas(K)
    sides = rng.choice([40.0, 60.0, 150.0], max(G, 1)) * rng.uniform(0.8, 1.25, max(G, 1))
    if not compact:
        sides = sides * np.where(sides < 55, 0.5, 1.0)
    reach = 0.2 * float(sides.min())
    base = rng.uniform(50, 300, 2)
    gt_kpts = np.zeros((G, K, 3))
    gt_bbox = np.zeros((G, 4))
    gt_area = np.zeros(G)
    for g in range(G):
        side = float(sides[g])
        gt_area[g] = side * side * 0.6
        if compact:
            gt_bbox[g] = (base[0], base[1], 0.1 * reach, 0.1 * reach)
            gt_kpts[g, :, :2] = base + rng.uniform(0, reach, (K, 2))
        else:
            x, y = rng.uniform(0, 400, 2)
            gt_bbox[g] = (x, y, side, side)
            gt_kpts[g, :, :2] = (x, y) + rng.uniform(0, side, (K, 2))
        gt_kpts[g, :, 2] = rng.integers(0, 3, K)
        if not (gt_kpts[g, :, 2] > 0).any():
            gt_kpts[g, 0, 2] = 2
    gt_crowd = rng.random(G) < crowd_p
    if zero_visible and G:
        gt_kpts[G - 1, :, 2] = 0
    if duplicate_gt and G > 1:
        gt_kpts[1], gt_bbox[1], gt_area[1], gt_crowd[1] = gt_kpts[0], gt_bbox[0], gt_area[0], gt_crowd[0]
    dt_kpts = np.zeros((D, K, 2))
    dt_area = np.zeros(D)
    for d in range(D):
        if G and rng.random() < 0.8:
            g = int(rng.integers(0, G))
            jitter = rng.choice([0.01, 0.03, 0.06, 0.12]) * float(sides[g])
            dt_kpts[d] = gt_kpts[g, :, :2] + rng.normal(0, 1, (K, 2)).clip(-2, 2) * jitter * sig[:, None] * 10
            dt_area[d] = gt_area[g] * rng.uniform(0.7, 1.4)
        else:
            side = float(rng.choice([20.0, 60.0, 150.0]))
            dt_kpts[d] = (base if compact else rng.uniform(0, 400, 2)) + rng.uniform(0, reach if compact else side,
                                                                                     (K, 2))
            dt_area[d] = side * side * 0.6
        if compact:
            dt_kpts[d] = np.clip(dt_kpts[d], base - 0.02 * reach, base + 1.02 * reach)
    dt_score = rng.uniform(0.05, 1.0, D)
    if equal_scores and D > 2:
        dt_score[D // 2:] = dt_score[D // 2]
    return make_image(gt_kpts, gt_bbox, gt_area, gt_crowd, dt_kpts, dt_score, dt_area, K=K)
