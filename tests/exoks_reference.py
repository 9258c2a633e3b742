"""The gauge of CocoKeypointEval(ex_oks=True): Ex-OKS, the presence-aware OKS of ProbPose, in plain loops over numpy
float64, written from the definition and not from the kernel (probpose_pytorch_amd/csrc/pp_cocoeval.hip).

A detection d has keypoints (xd, yd) and presence probabilities p[d, k] in [0, 1]; a ground truth g has keypoints
(xg, yg, v), an area and an activation window (x0, y0, x1, y1), the region the model saw; tau is the presence threshold.
For every keypoint with v > 0:

  gin = x0 <= xg < x1 and y0 <= yg < y1        (half open, as in_image of codec.py)
  pin = p[d, k] >= tau                         (equal counts as present)
  gin and pin          exp(-e), e = (dx^2 + dy^2) / (2 sigma)^2 / (area + eps) / 2: the plain OKS term
  gin and not pin      0: missed
  not gin and not pin  1: correctly reported absent
  not gin and pin      exp(-e), e = b^2 / (2 sigma)^2 / (area + eps) / 2 with
                       b = max(0, min(xd - x0, x1 - xd, yd - y0, y1 - yd)): a false positive, charged by how far inside
                       the window it was placed; on or outside the border it costs nothing

  ExOKS = (sum of the terms, in keypoint order) / (number of keypoints with v > 0)

A ground truth without any v > 0 keeps the grown-box score of tests/cocoeval_reference.compute_oks (it is ignored in
matching anyway).

An ``image`` is cocoeval_reference's dict plus gt_window [G, 4] and dt_presence [D, K].  ``accumulate``, ``summarize``
and ``stable_descending`` are cocoeval_reference's.  Its ``evaluate_image`` calls ``compute_oks`` itself and cannot be
given another similarity, so the matching walk is restated here with the similarity as an argument;
tests/test_exoks_reference.py holds the restatement to the original by running both on the plain OKS.
"""
import numpy as np

from tests import cocoeval_reference as CR

TAU = 0.5
CASES = ("both", "missed", "absent", "false_positive")


def compute_exoks(dt_kpts, dt_presence, gt_kpts, gt_bbox, gt_area, gt_window, sigmas, tau=TAU, info=None):
    """[D, G] float64.  ``info``, a dict, collects how often each of CASES occurred and the largest exponent e."""
    dt_kpts = np.asarray(dt_kpts, dtype=np.float64)
    dt_presence = np.asarray(dt_presence, dtype=np.float64)
    gt_kpts = np.asarray(gt_kpts, dtype=np.float64)
    gt_area = np.asarray(gt_area, dtype=np.float64).reshape(-1)
    gt_window = np.asarray(gt_window, dtype=np.float64).reshape(-1, 4)
    variances = (np.asarray(sigmas, dtype=np.float64) * 2) ** 2
    D, G, K = dt_kpts.shape[0], gt_kpts.shape[0], len(variances)
    if info is not None:
        for name in CASES:
            info.setdefault(name, 0)
        info.setdefault("e_max", 0.0)
    out = np.zeros((D, G), dtype=np.float64)
    for g in range(G):
        annotated = [k for k in range(K) if gt_kpts[g, k, 2] > 0]
        if not annotated:
            out[:, g] = CR.compute_oks(dt_kpts, gt_kpts[g:g + 1], np.asarray(gt_bbox).reshape(-1, 4)[g:g + 1],
                                       gt_area[g:g + 1], sigmas)[:, 0]
            continue
        size = gt_area[g] + CR.EPS
        x0, y0, x1, y1 = gt_window[g]
        for d in range(D):
            total = np.float64(0.0)
            for k in annotated:
                xg, yg = gt_kpts[g, k, 0], gt_kpts[g, k, 1]
                xd, yd = dt_kpts[d, k, 0], dt_kpts[d, k, 1]
                gin = bool(x0 <= xg < x1 and y0 <= yg < y1)
                pin = bool(dt_presence[d, k] >= tau)
                if gin and pin:
                    case = "both"
                    dx, dy = xd - xg, yd - yg
                    e = (dx * dx + dy * dy) / variances[k] / size / 2
                    term = np.exp(-e)
                elif gin:
                    case, e, term = "missed", 0.0, np.float64(0.0)
                elif not pin:
                    case, e, term = "absent", 0.0, np.float64(1.0)
                else:
                    case = "false_positive"
                    b = max(np.float64(0.0), min(xd - x0, x1 - xd, yd - y0, y1 - yd))
                    e = b * b / variances[k] / size / 2
                    term = np.exp(-e)
                total = total + term
                if info is not None:
                    info[case] += 1
                    info["e_max"] = max(info["e_max"], float(e))
            out[d, g] = total / len(annotated)
    return out


def plain_similarity(image, kept, sigmas, tau=TAU, info=None):
    return CR.compute_oks(image["dt_kpts"][kept], image["gt_kpts"], image["gt_bbox"], image["gt_area"], sigmas)


def ex_similarity(image, kept, sigmas, tau=TAU, info=None):
    return compute_exoks(image["dt_kpts"][kept], image["dt_presence"][kept], image["gt_kpts"], image["gt_bbox"],
                         image["gt_area"], image["gt_window"], sigmas, tau, info)


def evaluate_image(image, sigmas, area_range, thresholds=CR.OKS_THRESHOLDS, max_dets=CR.MAX_DETS, tau=TAU,
                   similarity=ex_similarity, info=None):
    """cocoeval_reference.evaluate_image (its rules, none of its mutation switches) on ``similarity``; the same
    result dict, "oks" being the similarity matrix [D', G]."""
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
    dt_index = CR.stable_descending(dt_score)[:max_dets]
    dt_area = np.asarray(image["dt_area"], dtype=np.float64).reshape(-1)
    D, T = len(dt_index), len(thresholds)
    oks = similarity(image, dt_index, sigmas, tau, info) if D and G else np.zeros((D, G))
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
                if m > -1 and not gt_ignore[m] and gt_ignore[g]:
                    break
                if oks[di, g] < best:
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


def evaluate(images, sigmas, tau=TAU, thresholds=CR.OKS_THRESHOLDS, recall_thresholds=CR.RECALL_THRESHOLDS,
             area_ranges=CR.AREA_RANGES, max_dets=CR.MAX_DETS, similarity=ex_similarity):
    """cocoeval_reference.evaluate on Ex-OKS: the ten stats, "precision" [T, R, A], "recall" [T, A], "per_image"
    [A][image], and "info" (case counts and the largest exponent, of the first area range's pass)."""
    T, R, A = len(thresholds), len(recall_thresholds), len(area_ranges)
    precision = np.zeros((T, R, A))
    recall = np.zeros((T, A))
    per_image, info = [], {}
    for a, rng in enumerate(area_ranges):
        results = [evaluate_image(im, sigmas, rng, thresholds, max_dets, tau, similarity, info if a == 0 else None)
                   for im in images]
        per_image.append(results)
        if results:
            precision[:, :, a], recall[:, a] = CR.accumulate(results, recall_thresholds)
        else:
            precision[:, :, a], recall[:, a] = -1.0, -1.0
    out = CR.summarize(precision, recall, thresholds)
    out.update(precision=precision, recall=recall, per_image=per_image, info=info)
    return out


# ------------------------------------------------------------------------------------------------ fixtures
def add_presence_fields(rng, image, tau=TAU, all_inside=False):
    """gt_window and dt_presence for an image of cocoeval_reference.random_image(..., compact=True).

    The compact square is recovered from the boxes (every box is (base, 0.1 reach, 0.1 reach)).  A window spans
    [0 .. 0.15, 0.85 .. 1] of the square on each axis, so about a quarter of the annotated keypoints fall outside it
    and the depth b of a false positive is at most half a window, 0.5 reach = 0.1 s (s = the smallest person's side):
    e = b^2 / (2 sigma)^2 / area / 2 <= 0.1^2 / (0.0025 * 0.6 * 2) = 3.3, well inside the fixture's e < 29.
    Bit-identical ground truths get the same window, so they stay twins.  Presence is drawn per (detection, keypoint)
    from {0, just below tau, exactly tau, 1, uniform} with weights (0.1, 0.1, 0.25, 0.3, 0.25), all float32 values, so
    a float32 tensor holds them exactly.  Window and weights lean towards "inside" and "present" because the other
    three cases mostly give terms of exactly 0 or 1 (a false positive outside the window costs nothing), and an
    Ex-OKS made of such terms alone is a fraction m / n that can sit exactly on a threshold, which the flag
    comparison's fixture condition forbids.
    ``all_inside``: the window holds the whole image's keypoints and every presence is 1 (Ex-OKS = OKS)."""
    gt_kpts, gt_bbox, dt_kpts = image["gt_kpts"], image["gt_bbox"], image["dt_kpts"]
    G, (D, K) = gt_kpts.shape[0], dt_kpts.shape[:2]
    window = np.zeros((G, 4))
    for g in range(G):
        base, reach = gt_bbox[g, :2], gt_bbox[g, 2] * 10.0
        lo, hi = rng.uniform(0.0, 0.15, 2), rng.uniform(0.85, 1.0, 2)
        window[g] = (base[0] + lo[0] * reach, base[1] + lo[1] * reach, base[0] + hi[0] * reach,
                     base[1] + hi[1] * reach)
        if all_inside:
            window[g] = (base[0] - reach, base[1] - reach, base[0] + 2 * reach, base[1] + 2 * reach)
        for h in range(g):
            if (gt_kpts[h].tobytes() == gt_kpts[g].tobytes() and gt_bbox[h].tobytes() == gt_bbox[g].tobytes()
                    and image["gt_area"][h] == image["gt_area"][g]):
                window[g] = window[h]
    below = np.nextafter(np.float32(tau), np.float32(0.0))
    kind = rng.choice(5, (D, K), p=(0.1, 0.1, 0.25, 0.3, 0.25))
    uniform = rng.random((D, K)).astype(np.float32)
    presence = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                         [np.float32(0.0), below, np.float32(tau), np.float32(1.0)], uniform).astype(np.float32)
    if all_inside:
        presence[:] = 1.0
    return dict(image, gt_window=window, dt_presence=presence.astype(np.float64))


def random_image(rng, K, G, D, tau=TAU, all_inside=False, **kw):
    """cocoeval_reference.random_image(compact=True) with windows and presence."""
    return add_presence_fields(rng, CR.random_image(rng, K, G, D, compact=True, **kw), tau, all_inside)


RAGGED = ((0, 3), (3, 0), (1, 1), (20, 7), (33, 2), (5, 70))          # (D, G) per image, as tests/test_cocoeval_gpu.py
RAGGED_SEED = {1: 101, 17: 117, 133: 233}                              # chosen in tests/test_exoks_reference.py
BATCH64_SEED = 2024


def ragged_images(K, all_inside=False):
    """The ragged batch of tests/test_cocoeval_gpu.py (same switches per image) with windows and presence."""
    rng = np.random.default_rng(RAGGED_SEED[K])
    images = []
    for i, (D, G) in enumerate(RAGGED):
        im = random_image(rng, K, G, D, all_inside=all_inside, crowd_p=0.1, zero_visible=(i == 3),
                          duplicate_gt=(i == 4), equal_scores=(i == 5))
        if i == 3:
            im["gt_crowd"][:] = False
            im["gt_crowd"][2] = True
        images.append(im)
    return _frozen(images)


def batch64():
    """64 seeded images, K = 17: 0 - 5 ground truths, 0 - 25 detections (more than max_dets = 20 in some); every eighth
    image has a bit-identical pair of ground truths, every eighth equal scores, every sixteenth a ground truth without
    visible keypoints."""
    rng = np.random.default_rng(BATCH64_SEED)
    images = []
    for i in range(64):
        G, D = int(rng.integers(0, 6)), int(rng.integers(0, 26))
        if i % 8 == 3:
            G = max(G, 2)
        images.append(random_image(rng, 17, G, D, crowd_p=0.15, zero_visible=(i % 16 == 5),
                                   duplicate_gt=(i % 8 == 3), equal_scores=(i % 8 == 6)))
    return _frozen(images)


def _frozen(images):
    for im in images:
        for a in im.values():
            a.setflags(write=False)
    return tuple(images)


def image_sizes(images):
    """A (width, height) per image that cuts through its compact square at 0.9 of its side, so that the window
    (0, 0, width, height) a COCO file implies leaves some annotated keypoints outside (and few enough for the reason
    add_presence_fields gives)."""
    sizes = []
    for im in images:
        if im["gt_bbox"].shape[0]:
            base, reach = im["gt_bbox"][0, :2], im["gt_bbox"][0, 2] * 10.0
            sizes.append((float(base[0] + 0.9 * reach), float(base[1] + 0.9 * reach)))
        else:
            sizes.append((640.0, 480.0))
    return sizes


def with_image_windows(images, sizes):
    """The images with every window replaced by (0, 0, width, height)."""
    return tuple(dict(im, gt_window=np.tile([0.0, 0.0, w, h], (im["gt_kpts"].shape[0], 1)))
                 for im, (w, h) in zip(images, sizes))


def coco_files(folder, images, sizes=None, presence_key=True, first_id=10):
    """A COCO annotation file and a result file of the images, as (dict, list, path, path).  A window cannot be
    stored: it is (0, 0, width, height) of ``sizes`` (None: the images carry neither key).  Presence goes under
    "presence", or into the third number of each keypoint triple."""
    import json
    k = images[0]["gt_kpts"].shape[1]
    gt = dict(images=[dict(id=first_id + i) for i in range(len(images))], annotations=[],
              categories=[dict(id=1, name="person")])
    if sizes is not None:
        for entry, (w, h) in zip(gt["images"], sizes):
            entry.update(width=w, height=h)
    res = []
    for i, im in enumerate(images):
        for g in range(im["gt_kpts"].shape[0]):
            gt["annotations"].append(dict(id=len(gt["annotations"]), image_id=first_id + i, category_id=1,
                                          keypoints=im["gt_kpts"][g].reshape(-1).tolist(),
                                          bbox=im["gt_bbox"][g].tolist(), area=float(im["gt_area"][g]),
                                          iscrowd=int(im["gt_crowd"][g])))
        for d in range(im["dt_kpts"].shape[0]):
            third = np.ones((k, 1)) if presence_key else im["dt_presence"][d][:, None]
            r = dict(image_id=first_id + i, category_id=1,
                     keypoints=np.concatenate([im["dt_kpts"][d], third], axis=1).reshape(-1).tolist(),
                     score=float(im["dt_score"][d]), area=float(im["dt_area"][d]))
            if presence_key:
                r["presence"] = im["dt_presence"][d].tolist()
            res.append(r)
    gpath, rpath = folder / "gt.json", folder / "res.json"
    gpath.write_text(json.dumps(gt))
    rpath.write_text(json.dumps(res))
    return gt, res, str(gpath), str(rpath)
