"""COCO keypoint AP / AR computed on the GPU (the other half of metrics.py: only the result arrays leave the device).

``CocoKeypointEval`` collects ground truths (host arrays: they come from an annotation file) and detections (numpy
arrays or device tensors: what ``Codec.decode`` leaves on the device after rescaling to image coordinates is never
copied to the host) and evaluates them with three HIP launches of csrc/pp_cocoeval.hip:

  pp_cocoeval_oks         the float64 OKS matrices of all images, packed D_i x G_i per image
  pp_cocoeval_match       the greedy matching of every (image, area range, OKS threshold) triple
  pp_cocoeval_accumulate  per (area range, threshold): tp / fp over the globally score-sorted detections, the
                          right-to-left precision envelope and the samples at the recall thresholds

Between them run two kinds of torch device ops, none of which synchronises: stable sorts (per image by score to cut
to ``max_dets``, and once over all kept detections) and gathers.  ``evaluate()`` synchronises exactly once, when it
reads precision [T, R, A] and recall [T, A] back; the ten stats are means over those arrays.

Rules (restated in tests/cocoeval_reference.py, the gauge this module is tested against):
* detections of an image are taken by descending score, equal scores in the order they were added, the first
  ``max_dets`` kept; across images equal scores keep image order: the order of ``add_ground_truth`` calls, then image
  ids first seen in ``add_detections``;
* a ground truth is ignored in an area range when it is crowd, has no keypoint with v > 0, or its area is outside;
* a detection takes the free ground truth with the largest OKS >= min(t, 1 - 1e-10), non-ignored ones first, the
  later one on equal OKS; crowd ground truths stay free; an unmatched detection with its area outside is ignored.

There is no CPU fallback: without a GPU ``evaluate()`` raises ``_lib.HipExtensionError``.
"""
from __future__ import annotations

import json
from functools import partial

import numpy as np
import torch

from . import _lib
from ._buffers import host_array as _host, room, upload

STATS = ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl")
_AREA_RANGES = ((0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))


def _mean_present(a: np.ndarray) -> float:
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    a = a[a > -1]
    return float(a.mean()) if a.size else -1.0


class CocoKeypointEval:
    """COCO keypoint evaluation of one category.

    ``sigmas`` [K] are the per-keypoint constants; ``oks_thresholds`` defaults to linspace(0.5, 0.95, 10),
    ``recall_thresholds`` to linspace(0, 1, 101), ``area_ranges`` to all / medium / large.  The ten stats read the area
    ranges by position (0 = all, 1 = medium, 2 = large) and the thresholds 0.5 and 0.75 by value; a stat whose range
    or threshold is not configured is -1."""

    def __init__(self, sigmas, *, oks_thresholds=None, recall_thresholds=None, area_ranges=None, max_dets: int = 20):
        self.sigmas = _host(sigmas, "sigmas", np.float64).reshape(-1)
        if self.sigmas.size == 0 or not np.all(np.isfinite(self.sigmas)) or np.any(self.sigmas <= 0):
            raise ValueError("sigmas: need K > 0 finite positive values")
        self.K = int(self.sigmas.size)
        self.oks_thresholds = (np.linspace(0.5, 0.95, 10) if oks_thresholds is None
                               else _host(oks_thresholds, "oks_thresholds", np.float64).reshape(-1))
        self.recall_thresholds = (np.linspace(0.0, 1.0, 101) if recall_thresholds is None
                                  else _host(recall_thresholds, "recall_thresholds", np.float64).reshape(-1))
        self.area_ranges = _host(_AREA_RANGES if area_ranges is None else area_ranges, "area_ranges", np.float64)
        if self.oks_thresholds.size == 0 or self.recall_thresholds.size == 0:
            raise ValueError("oks_thresholds / recall_thresholds: need at least one value")
        if self.area_ranges.ndim != 2 or self.area_ranges.shape[1] != 2 or self.area_ranges.shape[0] == 0:
            raise ValueError(f"area_ranges: expected [A, 2] (lo, hi), got {self.area_ranges.shape}")
        if int(max_dets) <= 0:
            raise ValueError(f"max_dets: {max_dets} is not positive")
        self.max_dets = int(max_dets)
        self.reset()

    # ------------------------------------------------------------------------------------------- collecting
    def reset(self) -> None:
        """Forget every ground truth and detection."""
        self._index = {}            # image id -> position (insertion order)
        self._gts = {}              # position -> list of (keypoints, bboxes, areas, iscrowd)
        self._dets = []             # (image positions [M] int64 host, keypoints, scores, areas): numpy or device
        self._gt_cache = None       # the concatenated ground truth, until an image or an instance is added

    def _position(self, image_id) -> int:
        key = image_id.item() if isinstance(image_id, np.generic) else image_id
        if key not in self._index:
            self._index[key] = len(self._index)
        return self._index[key]

    def add_ground_truth(self, image_id, keypoints, bboxes, areas, iscrowd=None) -> None:
        """The G annotated instances of one image (host arrays): keypoints [G, K, 3] (x, y, v), bboxes [G, 4] xywh,
        areas [G], iscrowd [G].  May be called again for the same image: the instances add up.  G = 0 registers the
        image."""
        kp = _host(keypoints, "keypoints", np.float64)
        if kp.ndim != 3 or kp.shape[1:] != (self.K, 3):
            raise ValueError(f"keypoints: expected [G, {self.K}, 3] (K = len(sigmas)), got {kp.shape}")
        G = kp.shape[0]
        bb = _host(bboxes, "bboxes", np.float64)
        if bb.shape != (G, 4):
            raise ValueError(f"bboxes: expected [{G}, 4], got {bb.shape}")
        ar = _host(areas, "areas", np.float64)
        if ar.shape != (G,):
            raise ValueError(f"areas: expected [{G}], got {ar.shape}")
        cr = np.zeros(G, dtype=bool) if iscrowd is None else _host(iscrowd, "iscrowd", np.int64).astype(bool)
        if cr.shape != (G,):
            raise ValueError(f"iscrowd: expected [{G}], got {cr.shape}")
        for name, a in (("keypoints", kp), ("bboxes", bb), ("areas", ar)):
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{name}: non-finite values")
        self._gts.setdefault(self._position(image_id), []).append((kp.copy(), bb.copy(), ar.copy(), cr.copy()))
        self._gt_cache = None

    def add_detections(self, image_ids, keypoints, scores, areas) -> None:
        """M detections: image_ids [M], keypoints [M, K, 2|3] (a third column is not used), scores [M], areas [M].
        keypoints / scores / areas given as device tensors stay on the device.  The image ids are bookkeeping of the
        host (they decide the ragged layout), so a tensor of ids is read here, once.  An image id without ground truth
        is evaluated against zero ground truths."""
        ids = image_ids.detach().cpu().numpy() if isinstance(image_ids, torch.Tensor) else np.asarray(image_ids)
        if ids.ndim != 1:
            raise ValueError(f"image_ids: expected [M], got {ids.shape}")
        M = int(ids.shape[0])
        keypoints, scores, areas = (a if isinstance(a, torch.Tensor) else np.asarray(a)
                                    for a in (keypoints, scores, areas))
        shape = tuple(keypoints.shape)
        if len(shape) != 3 or shape[0] != M or shape[1] != self.K or shape[2] not in (2, 3):
            raise ValueError(f"keypoints: expected [{M}, {self.K}, 2|3] (K = len(sigmas)), got {shape}")
        for name, a in (("scores", scores), ("areas", areas)):
            if tuple(a.shape) != (M,):
                raise ValueError(f"{name}: expected [{M}], got {tuple(a.shape)}")
        dev = [isinstance(a, torch.Tensor) and a.is_cuda for a in (keypoints, scores, areas)]
        if any(dev) and not all(dev):
            raise ValueError("keypoints / scores / areas: either all device tensors or all host arrays")
        if all(dev):
            kp = keypoints.detach()[..., :2].to(torch.float64).contiguous()
            sc, ar = scores.detach().to(torch.float64).contiguous(), areas.detach().to(torch.float64).contiguous()
            finite = torch.stack([torch.isfinite(sc).all(), torch.isfinite(ar).all(), torch.isfinite(kp).all()])
            finite = finite.cpu().numpy()       # three booleans; the detections themselves stay where they are
        else:
            kp = _host(keypoints, "keypoints", np.float64)[..., :2].copy()
            sc, ar = _host(scores, "scores", np.float64).copy(), _host(areas, "areas", np.float64).copy()
            finite = [np.all(np.isfinite(sc)), np.all(np.isfinite(ar)), np.all(np.isfinite(kp))]
        for name, ok in zip(("scores", "areas", "keypoints"), finite):
            if not bool(ok):
                raise ValueError(f"{name}: non-finite values")
        known = len(self._index)
        pos = np.fromiter((self._position(i) for i in ids), dtype=np.int64, count=M)
        if len(self._index) != known:
            self._gt_cache = None
        self._dets.append((pos, kp, sc, ar))

    # ------------------------------------------------------------------------------------------- JSON helpers
    @classmethod
    def from_coco_json(cls, path_or_dict, sigmas, category_id: int = 1, **kwargs) -> "CocoKeypointEval":
        """An evaluator holding the ground truth of a COCO annotation file (or its parsed dict): every image of
        "images" is registered, in file order; annotations of ``category_id`` with a "keypoints" list are added."""
        data = path_or_dict
        if not isinstance(data, dict):
            with open(path_or_dict) as f:
                data = json.load(f)
        ev = cls(sigmas, **kwargs)
        per_image = {}
        for im in data.get("images", []):
            per_image[im["id"]] = []
        for ann in data.get("annotations", []):
            if ann.get("category_id", category_id) != category_id or "keypoints" not in ann:
                continue
            per_image.setdefault(ann["image_id"], []).append(ann)
        for image_id, anns in per_image.items():
            kp = np.asarray([a["keypoints"] for a in anns], dtype=np.float64).reshape(len(anns), ev.K, 3)
            bb = np.asarray([a["bbox"] for a in anns], dtype=np.float64).reshape(len(anns), 4)
            ar = np.asarray([a.get("area", a["bbox"][2] * a["bbox"][3]) for a in anns], dtype=np.float64)
            cr = np.asarray([a.get("iscrowd", 0) for a in anns], dtype=np.int64)
            ev.add_ground_truth(image_id, kp, bb, ar.reshape(len(anns)), cr.reshape(len(anns)))
        ev.category_id = category_id
        return ev

    def add_results_json(self, path_or_list) -> None:
        """Detections in COCO's result format: a list of {"image_id", "category_id", "keypoints": 3 K numbers,
        "score"[, "area"]}.  Without "area" the area of the keypoints' bounding extent is used.  Entries of another
        category than the evaluator's (from_coco_json) are left out."""
        res = path_or_list
        if not isinstance(res, (list, tuple)):
            with open(path_or_list) as f:
                res = json.load(f)
        want = getattr(self, "category_id", None)
        res = [r for r in res if want is None or r.get("category_id", want) == want]
        if not res:
            return
        for r in res:
            if len(r["keypoints"]) != 3 * self.K:
                raise ValueError(f"keypoints: a result of image {r['image_id']} has {len(r['keypoints'])} numbers, "
                                 f"expected {3 * self.K}")
        kp = np.asarray([r["keypoints"] for r in res], dtype=np.float64).reshape(len(res), self.K, 3)
        extent = kp[..., :2].max(axis=1) - kp[..., :2].min(axis=1)
        areas = np.asarray([r["area"] if "area" in r else extent[i, 0] * extent[i, 1] for i, r in enumerate(res)],
                           dtype=np.float64)
        self.add_detections([r["image_id"] for r in res], kp, np.asarray([r["score"] for r in res], dtype=np.float64),
                            areas)

    # ------------------------------------------------------------------------------------------- evaluation
    def _ground_truth_arrays(self, n_img: int):
        if self._gt_cache is not None:
            return self._gt_cache
        K = self.K
        kps, bbs, ars, crs, counts = [], [], [], [], np.zeros(n_img, dtype=np.int64)
        for i in range(n_img):
            for kp, bb, ar, cr in self._gts.get(i, ()):
                kps.append(kp), bbs.append(bb), ars.append(ar), crs.append(cr)
                counts[i] += kp.shape[0]
        kp = np.concatenate(kps) if kps else np.zeros((0, K, 3))
        bb = np.concatenate(bbs) if bbs else np.zeros((0, 4))
        ar = np.concatenate(ars) if ars else np.zeros(0)
        cr = np.concatenate(crs) if crs else np.zeros(0, dtype=bool)
        flags = (cr.astype(np.uint8) * _lib.PP_COCO_GT_CROWD
                 + (~(kp[..., 2] > 0).any(axis=1)).astype(np.uint8) * _lib.PP_COCO_GT_NO_VISIBLE).astype(np.uint8)
        self._gt_cache = (kp, bb, ar, flags, counts)
        return self._gt_cache

    def _device_batch(self):
        """Everything of the ragged batch on the device: offsets, ground truth, the kept detections in per-image
        descending score order.  The layout (counts, offsets) is host arithmetic on the image ids; scores are only
        ever compared on the device."""
        dev = torch.device("cuda")
        n_img = len(self._index)
        gt_kp, gt_bb, gt_ar, gt_flags, g_cnt = self._ground_truth_arrays(n_img)
        pos = np.concatenate([d[0] for d in self._dets]) if self._dets else np.zeros(0, dtype=np.int64)
        d_all = np.bincount(pos, minlength=n_img).astype(np.int64) if n_img else np.zeros(0, dtype=np.int64)
        d_cnt = np.minimum(d_all, self.max_dets)
        offs = np.zeros((3, n_img + 1), dtype=np.int64)
        offs[0, 1:], offs[1, 1:], offs[2, 1:] = np.cumsum(d_cnt), np.cumsum(g_cnt), np.cumsum(d_cnt * g_cnt)
        Dtot = int(offs[0, -1])

        staged = []                 # pinned host copies, alive until the results are back
        up = partial(upload, device=dev, keep=staged)
        if pos.size:
            kp = torch.cat([up(d[1], dtype=torch.float64) for d in self._dets])
            sc = torch.cat([up(d[2], dtype=torch.float64) for d in self._dets])
            ar = torch.cat([up(d[3], dtype=torch.float64) for d in self._dets])
            # descending score, then image: two stable sorts leave every image's detections in score order, equal
            # scores in the order they were added
            by_score = torch.sort(sc, descending=True, stable=True).indices
            by_image = torch.sort(up(pos)[by_score], stable=True).indices
            perm = by_score[by_image]
            # positions of the sorted list whose rank within their image is below max_dets
            rank = np.arange(pos.size, dtype=np.int64) - np.repeat(np.cumsum(d_all) - d_all, d_all)
            sel = perm[up(np.nonzero(rank < self.max_dets)[0].astype(np.int64))]
            kp, sc, ar = kp[sel].contiguous(), sc[sel].contiguous(), ar[sel].contiguous()
        else:
            kp = torch.zeros((0, self.K, 2), dtype=torch.float64, device=dev)
            sc = torch.zeros(0, dtype=torch.float64, device=dev)
            ar = torch.zeros(0, dtype=torch.float64, device=dev)
        return dict(n_img=n_img, offs_host=offs, offs=up(offs), staged=staged, Dtot=Dtot, Gtot=int(offs[1, -1]),
                    oks_total=int(offs[2, -1]), dt_kpts=kp, dt_score=sc, dt_area=ar, gt_kpts=up(gt_kp),
                    gt_bbox=up(gt_bb), gt_area=up(gt_ar), gt_flags=up(gt_flags))

    def _oks(self, b) -> torch.Tensor:
        oks = torch.empty(max(b["oks_total"], 1), dtype=torch.float64, device="cuda")
        variances = upload((self.sigmas * 2) ** 2, "cuda", b["staged"], torch.float64)
        keep = [room(b[k]) for k in ("dt_kpts", "gt_kpts", "gt_bbox", "gt_area", "gt_flags")]
        _lib.launch("pp_cocoeval_oks", b["n_img"], self.K, b["Dtot"], b["Gtot"], b["oks_total"], b["offs_host"],
                    b["offs"], *keep, variances, oks)
        b["_keep_oks"] = (keep, variances)      # referenced until the results are back
        return oks

    def _match(self, b, oks):
        A, T = self.area_ranges.shape[0], self.oks_thresholds.size
        ranges = upload(self.area_ranges, "cuda", b["staged"], torch.float64)
        thr = upload(self.oks_thresholds, "cuda", b["staged"], torch.float64)
        gt_matched = torch.empty(max(A * T * b["Gtot"], 1), dtype=torch.uint8, device="cuda")
        dt_matched = torch.empty(max(A * T * b["Dtot"], 1), dtype=torch.uint8, device="cuda")
        dt_ignore = torch.empty(max(A * T * b["Dtot"], 1), dtype=torch.uint8, device="cuda")
        npig = torch.empty(A, dtype=torch.int32, device="cuda")
        keep = [room(b[k]) for k in ("gt_flags", "gt_area", "dt_area")]
        _lib.launch("pp_cocoeval_match", b["n_img"], A, T, b["Dtot"], b["Gtot"], b["oks_total"], b["offs_host"],
                    b["offs"], oks, *keep, ranges, thr, gt_matched, dt_matched, dt_ignore, npig)
        b["_keep_match"] = (keep, ranges, thr)
        return gt_matched, dt_matched, dt_ignore, npig

    def _accumulate(self, b, dt_matched, dt_ignore, npig) -> torch.Tensor:
        A, T, R = self.area_ranges.shape[0], self.oks_thresholds.size, self.recall_thresholds.size
        order = room(torch.sort(b["dt_score"], descending=True, stable=True).indices)
        rec = upload(self.recall_thresholds, "cuda", b["staged"], torch.float64)
        ws_env = torch.empty(max(A * T * b["Dtot"], 1), dtype=torch.float64, device="cuda")
        ws_tp = torch.empty(max(A * T * b["Dtot"], 1), dtype=torch.int32, device="cuda")
        out = torch.empty(T * R * A + T * A, dtype=torch.float64, device="cuda")
        precision, recall = out[:T * R * A], out[T * R * A:]
        _lib.launch("pp_cocoeval_accumulate", b["Dtot"], A, T, R, order, dt_matched, dt_ignore, npig, rec, ws_env,
                    ws_tp, precision, recall)
        b["_keep_acc"] = (order, rec, ws_env, ws_tp)
        return out

    def evaluate(self) -> dict:
        """The ten stats as floats plus "precision" [T, R, A] and "recall" [T, A] (numpy float64; -1 = no ground truth
        in that area range)."""
        _lib.require_device()
        b = self._device_batch()
        oks = self._oks(b)
        _, dt_matched, dt_ignore, npig = self._match(b, oks)
        out = self._accumulate(b, dt_matched, dt_ignore, npig)
        A, T, R = self.area_ranges.shape[0], self.oks_thresholds.size, self.recall_thresholds.size
        host = out.cpu().numpy()            # the one synchronisation
        del b, oks
        precision = host[:T * R * A].reshape(T, R, A).copy()
        recall = host[T * R * A:].reshape(T, A).copy()
        res = self.summarize(precision, recall)
        res.update(precision=precision, recall=recall)
        return res

    def summarize(self, precision: np.ndarray, recall: np.ndarray) -> dict:
        """The ten stats of precision [T, R, A] and recall [T, A]: means over the entries greater than -1."""
        A = precision.shape[2]

        def at(value):
            hit = np.nonzero(np.abs(self.oks_thresholds - value) < 1e-9)[0]
            return int(hit[0]) if hit.size else None

        def stat(arr, t=None, a=0):
            if a >= A or (t is not None and at(t) is None):
                return -1.0
            sel = arr[:, ..., a] if t is None else arr[at(t), ..., a]
            return _mean_present(sel)

        return {"AP": stat(precision), "AP50": stat(precision, 0.5), "AP75": stat(precision, 0.75),
                "APm": stat(precision, a=1), "APl": stat(precision, a=2),
                "AR": stat(recall), "AR50": stat(recall, 0.5), "AR75": stat(recall, 0.75),
                "ARm": stat(recall, a=1), "ARl": stat(recall, a=2)}
