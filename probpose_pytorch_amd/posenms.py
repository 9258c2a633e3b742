"""Instance rescoring and OKS-NMS of decoded poses on the GPU: the stage between ``Codec.decode`` and
``CocoKeypointEval.add_detections`` of every top-down evaluation protocol.

A person detector emits several overlapping boxes per person; the duplicate poses would count as false positives.
``rescore_instances`` makes an instance's score its box score times the mean of its confident keypoint scores;
``PoseNMS`` suppresses the duplicates per image, by hard OKS-NMS or by soft OKS-NMS, with the two launches of
csrc/pp_posenms.hip:

  pp_posenms_rescore   one lane per detection
  pp_posenms           one wave per image; lane j % 64 owns detection j's live flag and current score

Between them run torch device ops that do not synchronise: casts to float64, two stable sorts (descending score, then
image: every image's detections end up in score order, equal scores in the order they were given) and gathers.  That
front end (the layout from the image ids, the shape, placement and finiteness checks, the visiting order and the way
back) is _ragged.py's, which PoseTracker and CocoKeypointEval use too.

Rules (restated in tests/posenms_reference.py, the gauge this module is tested against), float64 throughout:
* rescoring: n = the keypoints with score > kpt_thr, score = box_score * (their sum in ascending k / n), 0 with n = 0;
* OKS of detections a, b of one image: the mean over the keypoints that count of exp(-e_k), e_k = (dx^2 + dy^2) /
  (2 sigma_k)^2 / ((area_a + area_b) / 2 + eps) / 2; with ``vis_thr`` None every keypoint counts, otherwise those whose
  visibility is above it in both; none counting gives 0;
* detections of an image are visited by descending score, equal scores in the order they were given;
* hard: a detection not yet suppressed is kept and suppresses every later live one whose OKS with it is > oks_thr;
  scores are unchanged;
* soft_gaussian / soft_linear: until nothing is live or ``max_dets`` are kept, the live detection with the largest
  current score (the earliest on equal scores) is kept with that score and every other live detection's score is
  multiplied by exp(-OKS^2 / oks_thr), or by (1 - OKS) where OKS >= oks_thr; detections never picked are not kept and
  return their current score.

There is no CPU fallback: without a GPU the calls raise ``_lib.HipExtensionError``.
"""
from __future__ import annotations

from functools import partial

import numpy as np
import torch

from . import _lib
from ._buffers import host_array as _host, room as _room, upload
from ._ragged import (check_pose_batch, device_f64, first_seen, group_layout, host_ids, unsorted, visibilities,
                      visiting_order)

MODES = {"hard": _lib.PP_POSENMS_HARD, "soft_gaussian": _lib.PP_POSENMS_SOFT_GAUSSIAN,
         "soft_linear": _lib.PP_POSENMS_SOFT_LINEAR}
MAX_DETS_PER_IMAGE = _lib.PP_POSENMS_MAX_DETS


def _rescore(ks: torch.Tensor, bs: torch.Tensor, kpt_thr: float) -> torch.Tensor:
    M, K = ks.shape
    out = torch.empty(M, dtype=torch.float64, device=ks.device)
    _lib.launch("pp_posenms_rescore", M, K, _room(ks), _room(bs), float(kpt_thr), _room(out))
    return out


def rescore_instances(kpt_scores, box_scores, kpt_thr: float = 0.2) -> torch.Tensor:
    """box_scores [M] times the mean of the kpt_scores [M, K] above ``kpt_thr``: a device float64 tensor [M].  An
    instance with no keypoint above the threshold scores 0.  The inputs are device tensors of any float dtype."""
    shape, bshape = tuple(kpt_scores.shape), tuple(box_scores.shape)
    if len(shape) != 2 or shape[1] == 0:
        raise ValueError(f"kpt_scores: expected [M, K] with K > 0, got {shape}")
    if bshape != (shape[0],):
        raise ValueError(f"box_scores: expected [{shape[0]}], got {bshape}")
    if not np.isfinite(kpt_thr):
        raise ValueError(f"kpt_thr: {kpt_thr} is not finite")
    ks, bs = device_f64((("kpt_scores", kpt_scores), ("box_scores", box_scores)))
    return _rescore(ks, bs, kpt_thr)


class PoseNMSResult:
    """What ``PoseNMS.__call__`` returns, in the order the detections were given: ``keep`` [M] bool and ``scores``
    [M] float64 on the device, ``counts`` [n_img] int32 on the device (kept per image) and ``image_ids`` (host list),
    both in first-seen image order."""
    __slots__ = ("keep", "scores", "counts", "image_ids", "_staged")

    def __init__(self, keep, scores, counts, image_ids, staged):
        self.keep, self.scores, self.counts, self.image_ids, self._staged = keep, scores, counts, image_ids, staged

    def __repr__(self):
        return f"PoseNMSResult({self.keep.shape[0]} detections of {len(self.image_ids)} images)"


class PoseNMS:
    """OKS-NMS of the decoded poses of a batch, per image.

    ``sigmas`` [K] are the per-keypoint constants; ``mode`` is "hard", "soft_gaussian" or "soft_linear";
    ``oks_thr`` in (0, 1]; ``vis_thr`` None lets every keypoint count in the OKS; ``kpt_thr`` is the rescoring
    threshold; ``max_dets`` bounds what the soft modes keep per image (hard mode does not use it)."""

    def __init__(self, sigmas, *, mode: str = "hard", oks_thr: float = 0.9, vis_thr=None, kpt_thr: float = 0.2,
                 max_dets: int = 20):
        self.sigmas = _host(sigmas, "sigmas", np.float64).reshape(-1)
        if self.sigmas.size == 0 or not np.all(np.isfinite(self.sigmas)) or np.any(self.sigmas <= 0):
            raise ValueError("sigmas: need K > 0 finite positive values")
        self.K = int(self.sigmas.size)
        if mode not in MODES:
            raise ValueError(f"mode: {mode!r} is not one of {tuple(MODES)}")
        if not 0.0 < float(oks_thr) <= 1.0:
            raise ValueError(f"oks_thr: {oks_thr} is outside (0, 1]")
        if vis_thr is not None and not np.isfinite(vis_thr):
            raise ValueError(f"vis_thr: {vis_thr} is not finite")
        if not np.isfinite(kpt_thr):
            raise ValueError(f"kpt_thr: {kpt_thr} is not finite")
        if int(max_dets) <= 0:
            raise ValueError(f"max_dets: {max_dets} is not positive")
        self.mode, self.oks_thr, self.kpt_thr = mode, float(oks_thr), float(kpt_thr)
        self.vis_thr = None if vis_thr is None else float(vis_thr)
        self.max_dets = int(max_dets)

    def _launch(self, n_img, off, off_dev, kp_s, vis_s, ar_s, sc_s, variances):
        """pp_posenms on a batch in visiting order: (scores [M] float64, keep [M] uint8, counts [n_img] int32)."""
        M, dev = int(off[-1]), kp_s.device
        out_s = torch.empty(M, dtype=torch.float64, device=dev)
        keep_s = torch.empty(M, dtype=torch.uint8, device=dev)
        counts = torch.zeros(n_img, dtype=torch.int32, device=dev)
        hold = [_room(t) for t in (kp_s, ar_s, sc_s, out_s, keep_s, counts)]
        vis_hold = None if vis_s is None else _room(vis_s)
        _lib.launch("pp_posenms", n_img, self.K, M, off, off_dev, hold[0], vis_hold, hold[1], hold[2], variances,
                    MODES[self.mode], self.oks_thr, 0.0 if self.vis_thr is None else self.vis_thr, self.max_dets,
                    *hold[3:])
        return out_s, keep_s, counts

    def __call__(self, image_ids, keypoints, box_scores, areas, kpt_scores=None) -> PoseNMSResult:
        """M detections: image_ids [M], keypoints [M, K, 2|3], box_scores [M], areas [M], kpt_scores [M, K] or None.

        The image ids are bookkeeping of the host (they decide the ragged layout), so a tensor of ids is read here,
        once; the other inputs are device tensors of any float dtype and stay on the device.  With ``kpt_scores`` the
        instances are rescored first (``rescore_instances``) and ``kpt_scores`` is the per-keypoint visibility that
        ``vis_thr`` reads; without it ``box_scores`` are the scores and a third keypoint column, if there is one, is
        the visibility.

        Apart from the finiteness booleans of the inputs nothing is read back and nothing waits for the device: the
        result's tensors are still being computed when this returns.  Boolean indexing by ``keep``
        (``keypoints[res.keep]``) is the caller's one readback, since the number of survivors decides a shape."""
        ids = host_ids(image_ids)
        if ids.ndim != 1:
            raise ValueError(f"image_ids: expected [M], got {ids.shape}")
        named = [("keypoints", keypoints), ("box_scores", box_scores), ("areas", areas)]
        if kpt_scores is not None:
            named.append(("kpt_scores", kpt_scores))
        named, _ = check_pose_batch(named, self.K, int(ids.shape[0]), self.vis_thr)
        image_list, pos = first_seen(ids)
        _, off = group_layout(pos, image_list, "image_ids: image",
                              [(MAX_DETS_PER_IMAGE, "that PoseNMS handles per image")])

        tensors = device_f64(named)
        kp3, bs, ar = tensors[:3]
        dev = kp3.device
        sc = bs if kpt_scores is None else _rescore(tensors[3], bs, self.kpt_thr)
        vis = visibilities(tensors, self.vis_thr)
        staged = []
        up = partial(upload, device=dev, keep=staged)
        perm, _ = visiting_order(sc, pos, up)
        kp_s = kp3[..., :2][perm].contiguous()
        vis_s = None if vis is None else vis[perm].contiguous()
        ar_s, sc_s = ar[perm].contiguous(), sc[perm].contiguous()
        variances, off_dev = up((self.sigmas * 2) ** 2), up(off)
        out_s, keep_s, counts = self._launch(len(image_list), off, off_dev, kp_s, vis_s, ar_s, sc_s, variances)
        keep, scores = unsorted(perm, keep_s.to(torch.bool)), unsorted(perm, out_s)
        return PoseNMSResult(keep, scores, counts, image_list, staged)
