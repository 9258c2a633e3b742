"""COCO keypoint AP / AR computed on the GPU (the other half of metrics.py: only the result arrays leave the device).

``CocoKeypointEval`` collects ground truths (host arrays: they come from an annotation file) and detections (numpy
arrays or device tensors: what ``Codec.decode`` leaves on the device after rescaling to image coordinates is never
copied to the host) and evaluates them with three HIP launches of csrc/pp_cocoeval.hip:

  pp_cocoeval_oks         the float64 OKS matrices of all images, packed D_i x G_i per image
                          (pp_cocoeval_exoks with ``ex_oks=True``: the presence-aware Ex-OKS, below)
  pp_cocoeval_match       the greedy matching of every (image, area range, OKS threshold) triple
  pp_cocoeval_accumulate  per (area range, threshold): tp / fp over the globally score-sorted detections, the
                          right-to-left precision envelope and the samples at the recall thresholds

Between them run two kinds of torch device ops, none of which synchronises: stable sorts (per image by score to cut
to ``max_dets``: _ragged.visiting_order, the order PoseNMS and PoseTracker visit by; and once over all kept
detections) and gathers.  The shape and placement checks of ``add_detections`` and its read-back are _ragged.py's
too.  ``evaluate()`` synchronises exactly once, when it reads precision [T, R, A] and recall [T, A] back; the ten
stats are means over those arrays.

Rules (restated in tests/cocoeval_reference.py, the gauge this module is tested against):
* detections of an image are taken by descending score, equal scores in the order they were added, the first
  ``max_dets`` kept; across images equal scores keep image order: the order of ``add_ground_truth`` calls, then image
  ids first seen in ``add_detections``;
* a ground truth is ignored in an area range when it is crowd, has no keypoint with v > 0, or its area is outside;
* a detection takes the free ground truth with the largest OKS >= min(t, 1 - 1e-10), non-ignored ones first, the
  later one on equal OKS; crowd ground truths stay free; an unmatched detection with its area outside is ignored.

Ex-OKS (``ex_oks=True``; DESIGN 4.7b, include/probpose_hip.h) scores what ProbPose adds: a ground truth carries the
activation window (x0, y0, x1, y1) the model saw, a detection a presence probability per keypoint.  Per keypoint with
v > 0, with gin = the ground truth lies in the window (half open, as ``in_image`` of codec.py) and pin = presence >=
``presence_threshold``: both, the plain OKS term; gin only, 0 (missed); neither, 1 (correctly reported absent); pin
only, exp(-e) of the depth b = max(0, min(xd - x0, x1 - xd, yd - y0, y1 - yd)) of the prediction inside the window.
Ex-OKS is the mean of the terms; matching and accumulation run on it unchanged.

There is no CPU fallback: without a GPU ``evaluate()`` raises ``_lib.HipExtensionError``.

``python -m probpose_pytorch_amd.cocoeval GT.json RESULTS.json [--sigmas coco17|FLOAT] [--category-id N] [--max-dets N]
[--ex-oks] [--presence-thr P]`` prints the ten stats as one JSON object.
"""
from __future__ import annotations

import argparse
import json
import sys
from functools import partial

import numpy as np
import torch

from . import _lib
from ._buffers import host_array as _host, room, upload
from ._ragged import FINITE, check_pose_batch, checked_f64, group_layout, host_ids, on_device, visiting_order

STATS = ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl")
_AREA_RANGES = ((0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
# the 17 COCO person keypoint constants, in the form they are published (tenths, divided by 10)
COCO17_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
# what add_detections asks of a device tensor of presence probabilities (false for a NaN as well) and says if not
_IN_UNIT = (lambda p: ((p >= 0) & (p <= 1)).all(), "non-finite values or values outside [0, 1]")


def _mean_present(a: np.ndarray) -> float:
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    a = a[a > -1]
    return float(a.mean()) if a.size else -1.0


class CocoKeypointEval:
    """COCO keypoint evaluation of one category.

    ``sigmas`` [K] are the per-keypoint constants; ``oks_thresholds`` defaults to linspace(0.5, 0.95, 10),
    ``recall_thresholds`` to linspace(0, 1, 101), ``area_ranges`` to all / medium / large.  The ten stats read the area
    ranges by position (0 = all, 1 = medium, 2 = large) and the thresholds 0.5 and 0.75 by value; a stat whose range
    or threshold is not configured is -1.

    ``ex_oks=True`` scores Ex-OKS (module docstring) in place of OKS: every ground truth then needs its activation
    window and every detection its presence probabilities, read against ``presence_threshold`` (in [0, 1]; equal
    counts as present)."""

    def __init__(self, sigmas, *, oks_thresholds=None, recall_thresholds=None, area_ranges=None, max_dets: int = 20,
                 ex_oks: bool = False, presence_threshold: float = 0.5):
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
        self.ex_oks = bool(ex_oks)
        self.presence_threshold = float(presence_threshold)
        if not 0.0 <= self.presence_threshold <= 1.0:          # a NaN fails it too
            raise ValueError(f"presence_threshold: {presence_threshold} is not in [0, 1]")
        self.reset()

    # ------------------------------------------------------------------------------------------- collecting
    def reset(self) -> None:
        """Forget every ground truth and detection."""
        self._index = {}            # image id -> position (insertion order)
        self._gts = {}              # position -> list of (keypoints, bboxes, areas, iscrowd)
        self._windows = {}          # position -> list of windows [G, 4] xyxy (or None), one per entry of _gts
        self._dets = []             # (image positions [M] int64 host, keypoints, scores, areas): numpy or device
        self._presence = []         # per entry of _dets: presence [M, K] float64 on the same side, or None
        self._gt_cache = None       # the concatenated ground truth, until an image or an instance is added

    def _position(self, image_id) -> int:
        key = image_id.item() if isinstance(image_id, np.generic) else image_id
        if key not in self._index:
            self._index[key] = len(self._index)
        return self._index[key]

    def add_ground_truth(self, image_id, keypoints, bboxes, areas, iscrowd=None, windows=None) -> None:
        """The G annotated instances of one image (host arrays): keypoints [G, K, 3] (x, y, v), bboxes [G, 4] xywh,
        areas [G], iscrowd [G].  May be called again for the same image: the instances add up.  G = 0 registers the
        image.  ``windows`` [G, 4] (or [4] for all instances) are the activation windows (x0, y0, x1, y1) of Ex-OKS:
        required with ``ex_oks=True``, checked and not used without."""
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
        win = None
        if windows is not None:
            win = _host(windows, "windows", np.float64)
            if win.shape == (4,):
                win = np.broadcast_to(win, (G, 4))
            if win.shape != (G, 4):
                raise ValueError(f"windows: expected [{G}, 4] or [4] (x0, y0, x1, y1), got {win.shape}")
            if not np.all(np.isfinite(win)):
                raise ValueError("windows: non-finite values")
            if not (np.all(win[:, 2] > win[:, 0]) and np.all(win[:, 3] > win[:, 1])):
                raise ValueError("windows: need x1 > x0 and y1 > y0")
            win = win.copy()
        elif self.ex_oks and G > 0:
            raise ValueError("windows: Ex-OKS needs the activation window of every ground truth")
        pos = self._position(image_id)
        self._gts.setdefault(pos, []).append((kp.copy(), bb.copy(), ar.copy(), cr.copy()))
        self._windows.setdefault(pos, []).append(win)
        self._gt_cache = None

    def add_detections(self, image_ids, keypoints, scores, areas, presence=None) -> None:
        """M detections: image_ids [M], keypoints [M, K, 2|3] (a third column is not used), scores [M], areas [M].
        keypoints / scores / areas given as device tensors stay on the device.  The image ids are bookkeeping of the
        host (they decide the ragged layout), so a tensor of ids is read here, once.  An image id without ground truth
        is evaluated against zero ground truths.  ``presence`` [M, K] in [0, 1] are the presence probabilities of
        Ex-OKS (``Codec.decode_device``'s ``aux[0]``), on the same side as the rest; a device tensor of any float type
        is widened to float64 there.  Required with ``ex_oks=True``, checked and not used without."""
        ids = host_ids(image_ids)
        if ids.ndim != 1:
            raise ValueError(f"image_ids: expected [M], got {ids.shape}")
        named = [("keypoints", keypoints), ("scores", scores), ("areas", areas)]
        if presence is not None:
            named.append(("presence", presence))
        named, M = check_pose_batch(named, self.K, int(ids.shape[0]))
        device = on_device(named[:3])
        if presence is not None:
            if (isinstance(named[3][1], torch.Tensor) and named[3][1].is_cuda) != device:
                raise ValueError("presence: must be on the same side (device or host) as keypoints / scores / areas")
        elif self.ex_oks:
            raise ValueError("presence: Ex-OKS needs the presence probabilities of every detection")
        # a refusal names scores, areas, keypoints and presence in this order; a third keypoint column is not looked at
        named = [named[1], named[2], ("keypoints", named[0][1][..., :2])] + named[3:]
        if device:      # three or four booleans in one readback; the detections themselves stay where they are
            sc, ar, kp, *pr = checked_f64(named, {"presence": _IN_UNIT})
        else:
            sc, ar, kp, *pr = (_host(a, n, np.float64).copy() for n, a in named)
            for (n, _), a in zip(named, (sc, ar, kp)):
                if not np.all(np.isfinite(a)):
                    raise ValueError(f"{n}: {FINITE[1]}")
            if pr and not np.all((pr[0] >= 0) & (pr[0] <= 1)):
                raise ValueError(f"presence: {_IN_UNIT[1]}")
        known = len(self._index)
        pos = np.fromiter((self._position(i) for i in ids), dtype=np.int64, count=M)
        if len(self._index) != known:
            self._gt_cache = None
        self._dets.append((pos, kp, sc, ar))
        self._presence.append(pr[0] if pr else None)

    # ------------------------------------------------------------------------------------------- JSON helpers
    @classmethod
    def from_coco_json(cls, path_or_dict, sigmas, category_id: int = 1, **kwargs) -> "CocoKeypointEval":
        """An evaluator holding the ground truth of a COCO annotation file (or its parsed dict): every image of
        "images" is registered, in file order; annotations of ``category_id`` with a "keypoints" list are added.
        With ``ex_oks=True`` the activation window of an image's ground truths is the whole image,
        (0, 0, "width", "height") of its "images" entry."""
        data = path_or_dict
        if not isinstance(data, dict):
            with open(path_or_dict) as f:
                data = json.load(f)
        ev = cls(sigmas, **kwargs)
        per_image, window = {}, {}
        for im in data.get("images", []):
            per_image[im["id"]] = []
            if ev.ex_oks:
                if "width" not in im or "height" not in im:
                    raise ValueError(f"images: image {im['id']} has no \"width\" / \"height\" to take its Ex-OKS "
                                     "window from")
                window[im["id"]] = (0.0, 0.0, float(im["width"]), float(im["height"]))
        for ann in data.get("annotations", []):
            if ann.get("category_id", category_id) != category_id or "keypoints" not in ann:
                continue
            per_image.setdefault(ann["image_id"], []).append(ann)
        for image_id, anns in per_image.items():
            kp = np.asarray([a["keypoints"] for a in anns], dtype=np.float64).reshape(len(anns), ev.K, 3)
            bb = np.asarray([a["bbox"] for a in anns], dtype=np.float64).reshape(len(anns), 4)
            ar = np.asarray([a.get("area", a["bbox"][2] * a["bbox"][3]) for a in anns], dtype=np.float64)
            cr = np.asarray([a.get("iscrowd", 0) for a in anns], dtype=np.int64)
            if ev.ex_oks and image_id not in window:
                raise ValueError(f"images: annotations name image {image_id}, which has no entry to take its Ex-OKS "
                                 "window from")
            ev.add_ground_truth(image_id, kp, bb, ar.reshape(len(anns)), cr.reshape(len(anns)),
                                windows=window.get(image_id))
        ev.category_id = category_id
        return ev

    def add_results_json(self, path_or_list) -> None:
        """Detections in COCO's result format: a list of {"image_id", "category_id", "keypoints": 3 K numbers,
        "score"[, "area"]}.  Without "area" the area of the keypoints' bounding extent is used.  Entries of another
        category than the evaluator's (from_coco_json) are left out.  In Ex-OKS mode a result's presence probabilities
        are its "presence" (K numbers) when it has that key, else the third number of each keypoint triple."""
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
        presence = None
        if self.ex_oks:
            for r in res:
                if "presence" in r and len(r["presence"]) != self.K:
                    raise ValueError(f"presence: a result of image {r['image_id']} has {len(r['presence'])} numbers, "
                                     f"expected {self.K}")
            presence = np.asarray([r["presence"] if "presence" in r else kp[i, :, 2] for i, r in enumerate(res)],
                                  dtype=np.float64).reshape(len(res), self.K)
        self.add_detections([r["image_id"] for r in res], kp, np.asarray([r["score"] for r in res], dtype=np.float64),
                            areas, presence=presence)

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

    def _window_array(self, n_img: int) -> np.ndarray:
        """[Gtot, 4] windows in the order of _ground_truth_arrays (Ex-OKS: every entry with instances has them)."""
        wins = [w for i in range(n_img) for w in self._windows.get(i, ()) if w is not None]
        return np.concatenate(wins) if wins else np.zeros((0, 4))

    def _device_batch(self):
        """Everything of the ragged batch on the device: offsets, ground truth, the kept detections in per-image
        descending score order (in Ex-OKS mode their presence rows with them, and the ground truths' windows).  The
        layout (counts, offsets) is host arithmetic on the image ids; scores are only ever compared on the device."""
        dev = torch.device("cuda")
        n_img = len(self._index)
        gt_kp, gt_bb, gt_ar, gt_flags, g_cnt = self._ground_truth_arrays(n_img)
        pos = np.concatenate([d[0] for d in self._dets]) if self._dets else np.zeros(0, dtype=np.int64)
        d_all = group_layout(pos, n_img)[0]
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
            perm, _ = visiting_order(sc, pos, up)
            # positions of the sorted list whose rank within their image is below max_dets
            rank = np.arange(pos.size, dtype=np.int64) - np.repeat(np.cumsum(d_all) - d_all, d_all)
            sel = perm[up(np.nonzero(rank < self.max_dets)[0].astype(np.int64))]
            kp, sc, ar = kp[sel].contiguous(), sc[sel].contiguous(), ar[sel].contiguous()
            if self.ex_oks:         # the same gather: the cut and the score order apply to the presence rows alike
                pr = torch.cat([up(p, dtype=torch.float64) for p in self._presence])[sel].contiguous()
        else:
            kp = torch.zeros((0, self.K, 2), dtype=torch.float64, device=dev)
            sc = torch.zeros(0, dtype=torch.float64, device=dev)
            ar = torch.zeros(0, dtype=torch.float64, device=dev)
            pr = torch.zeros((0, self.K), dtype=torch.float64, device=dev)
        b = dict(n_img=n_img, offs_host=offs, offs=up(offs), staged=staged, Dtot=Dtot, Gtot=int(offs[1, -1]),
                 oks_total=int(offs[2, -1]), dt_kpts=kp, dt_score=sc, dt_area=ar, gt_kpts=up(gt_kp),
                 gt_bbox=up(gt_bb), gt_area=up(gt_ar), gt_flags=up(gt_flags))
        if self.ex_oks:
            gt_win = self._window_array(n_img)
            assert gt_win.shape[0] == b["Gtot"] and pr.shape[0] == Dtot
            b.update(dt_presence=pr, gt_window=up(gt_win))
        return b

    def _oks(self, b) -> torch.Tensor:
        oks = torch.empty(max(b["oks_total"], 1), dtype=torch.float64, device="cuda")
        variances = upload((self.sigmas * 2) ** 2, "cuda", b["staged"], torch.float64)
        keep = [room(b[k]) for k in ("dt_kpts", "gt_kpts", "gt_bbox", "gt_area", "gt_flags")]
        if self.ex_oks:
            keep += [variances, room(b["dt_presence"]), room(b["gt_window"])]
            _lib.launch("pp_cocoeval_exoks", b["n_img"], self.K, b["Dtot"], b["Gtot"], b["oks_total"], b["offs_host"],
                        b["offs"], *keep, self.presence_threshold, oks)
        else:
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


# ------------------------------------------------------------------------------------------------ command line
def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m probpose_pytorch_amd.cocoeval",
                                 description="COCO keypoint AP / AR of a result file, computed on the GPU; prints the "
                                             "ten stats as one JSON object.")
    ap.add_argument("ground_truth", metavar="GT.json", help="COCO annotation file")
    ap.add_argument("results", metavar="RESULTS.json", help="COCO keypoint result file")
    ap.add_argument("--sigmas", default="coco17", help="'coco17', or one positive number used for every keypoint")
    ap.add_argument("--category-id", type=int, default=1)
    ap.add_argument("--max-dets", type=int, default=20)
    ap.add_argument("--ex-oks", action="store_true",
                    help="score Ex-OKS: windows from the images' width / height, presence from the results' "
                         "\"presence\" or the third number of each keypoint triple")
    ap.add_argument("--presence-thr", type=float, default=0.5)
    return ap


def _cli_sigmas(spec: str, data: dict, category_id: int) -> np.ndarray:
    if spec == "coco17":
        return COCO17_SIGMAS.copy()
    try:
        value = float(spec)
    except ValueError:
        raise ValueError(f"--sigmas: expected 'coco17' or a number, got {spec!r}") from None
    # one constant for all keypoints: their number is the category's, else that of its first annotation
    for cat in data.get("categories", []):
        if cat.get("id") == category_id and "keypoints" in cat:
            return np.full(len(cat["keypoints"]), value)
    for ann in data.get("annotations", []):
        if ann.get("category_id", category_id) == category_id and "keypoints" in ann:
            return np.full(len(ann["keypoints"]) // 3, value)
    raise ValueError(f"--sigmas {spec}: the annotation file does not say how many keypoints category {category_id} has")


def main(argv=None) -> int:
    args = _parser().parse_args(argv)
    with open(args.ground_truth) as f:
        data = json.load(f)
    ev = CocoKeypointEval.from_coco_json(data, _cli_sigmas(args.sigmas, data, args.category_id),
                                         category_id=args.category_id, max_dets=args.max_dets, ex_oks=args.ex_oks,
                                         presence_threshold=args.presence_thr)
    ev.add_results_json(args.results)
    res = ev.evaluate()
    print(json.dumps({k: res[k] for k in STATS}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
