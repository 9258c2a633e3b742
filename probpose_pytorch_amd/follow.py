"""Following people through a video without a person box for every frame: boxes on a key frame start the tracks, and
from then on each track's own last pose says where its person is cropped next (``PoseTracker.propose_boxes``, one HIP
launch).  ``PoseFollower`` is the loop around it: propose, crop and estimate, drop what lost its person,
optional ``PoseNMS``, ``PoseTracker.update``.

The proposed boxes cross to the host once per frame (``BoxProposals.compact``): the crops are planned on the host from
integer-rounded boxes (``frontend.FrontendPlan``).  One more boolean per pose crosses for the drop rule, besides what
``PoseNMS`` and ``PoseTracker.update`` read themselves.

The defaults (``pad`` 1.25, ``iou_thr`` 0.3, and the 0.3 a caller usually gives the tracker as ``vis_thr``) are common
top-down practice; they are not tuned on data.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._buffers import host_array as _host

SOURCE_GIVEN, SOURCE_TRACK = 0, 1

FollowStep = namedtuple("FollowStep", "boxes source tracks kpt_scores")
FollowStep.__doc__ = """What ``PoseFollower.step`` returns, over the poses it kept: ``boxes`` [m, 4] float64 xywh (host),
``source`` [m] int64 (0 = a given box, 1 = a track's proposal; host), ``tracks`` (the ``TrackResult`` of the update) and
``kpt_scores`` [m, K] (device)."""


class PoseFollower:
    """``tracker``: a ``PoseTracker`` with ``vis_thr`` set (a track has to be able to lose keypoints, or a lost person
    is followed for ever).  ``estimate(frame, boxes_xywh ndarray [n, 4]) -> (keypoints [n, K, 2], kpt_scores [n, K])``,
    device tensors in frame pixels, is the top-down estimator.  ``nms``: an optional ``PoseNMS`` applied to the frame's
    poses.  The other options are those of ``PoseTracker.propose_boxes``."""

    def __init__(self, tracker, estimate, *, nms=None, pad: float = 1.25, aspect=None, min_side: float = 2.0,
                 min_keypoints: int = 3, max_age: int = 0, extrapolate: bool = True, max_dt=None,
                 iou_thr: float = 0.3):
        if tracker.vis_thr is None:
            raise ValueError("tracker: vis_thr is None; a followed track has to be able to lose keypoints")
        if not callable(estimate):
            raise ValueError("estimate: expected a callable (frame, boxes) -> (keypoints, kpt_scores)")
        if int(min_keypoints) < 1:
            raise ValueError(f"min_keypoints: {min_keypoints} is below 1")
        self.tracker, self.estimate, self.nms = tracker, estimate, nms
        self.options = dict(pad=pad, aspect=aspect, min_side=min_side, min_keypoints=int(min_keypoints),
                            max_age=max_age, extrapolate=extrapolate, max_dt=max_dt, iou_thr=iou_thr)

    def step(self, frame, boxes=None, box_scores=None, *, frame_size=None, t=None, stream=0) -> FollowStep:
        """One frame of ``stream``: ``boxes`` [n, 4] xywh with ``box_scores`` [n] (default: ones) are the person boxes
        somebody else found on this frame, if any; the tracks' proposals that do not duplicate them (IoU <=
        ``iou_thr``) follow them in the crop list.  ``frame`` goes to ``estimate`` as it is; ``frame_size`` (w, h)
        clamps the proposals.  A pose with fewer than ``min_keypoints`` keypoints above the tracker's ``vis_thr`` is
        dropped, so that a track whose person left does not give birth to a new one; with no pose left the tracker is
        still updated, so its tracks age."""
        tr = self.tracker
        K = tr.K
        given = np.zeros((0, 4)) if boxes is None else _host(boxes, "boxes", np.float64).reshape(-1, 4)
        n_given = given.shape[0]
        g_scores = np.ones(n_given) if box_scores is None else _host(box_scores, "box_scores", np.float64).reshape(-1)
        if g_scores.shape != (n_given,):
            raise ValueError(f"box_scores: expected [{n_given}], got {g_scores.shape}")
        if stream in tr._index:
            proposals = tr.propose_boxes(t, streams=[stream], frame_size=frame_size,
                                         suppress=(given, None) if n_given else None, **self.options)
            p_boxes, _, p_scores, _ = proposals.compact()
        else:                                               # nothing to follow yet
            _lib.require_device()
            p_boxes, p_scores = np.zeros((0, 4)), np.zeros(0)
        crops = np.concatenate([given, p_boxes])
        source = np.concatenate([np.full(n_given, SOURCE_GIVEN, dtype=np.int64),
                                 np.full(p_boxes.shape[0], SOURCE_TRACK, dtype=np.int64)])
        scores = np.concatenate([g_scores, p_scores])
        n = crops.shape[0]
        dev = tr._device if tr._device is not None else torch.device("cuda")
        if n:
            kp, vis = self.estimate(frame, crops)
            if tuple(kp.shape) != (n, K, 2) or tuple(vis.shape) != (n, K):
                raise ValueError(f"estimate: expected keypoints [{n}, {K}, 2] and kpt_scores [{n}, {K}], got "
                                 f"{tuple(kp.shape)} and {tuple(vis.shape)}")
            _lib.require_device(kp)
            dev = kp.device
            keep = ((vis > tr.vis_thr).sum(dim=1) >= self.options["min_keypoints"]).cpu().numpy()
        else:
            kp = torch.zeros((0, K, 2), dtype=torch.float64, device=dev)
            vis = torch.zeros((0, K), dtype=torch.float64, device=dev)
            keep = np.zeros(0, dtype=bool)
        if not keep.all():
            on = torch.from_numpy(np.flatnonzero(keep)).to(dev)
            kp, vis, crops, source, scores = kp[on], vis[on], crops[keep], source[keep], scores[keep]
        areas = torch.from_numpy(crops[:, 2] * crops[:, 3]).to(dev)
        scores_dev = torch.from_numpy(scores).to(dev)
        if self.nms is not None and crops.shape[0]:
            res = self.nms(np.zeros(crops.shape[0], dtype=np.int64), kp, scores_dev, areas, kpt_scores=vis)
            kept = res.keep.cpu().numpy()
            on = torch.from_numpy(np.flatnonzero(kept)).to(dev)
            kp, vis, areas, scores_dev = kp[on], vis[on], areas[on], res.scores[on]
            crops, source = crops[kept], source[kept]
        tracks = tr.update(kp, areas, scores_dev, kpt_scores=vis, stream_ids=[stream] * crops.shape[0],
                           streams=[stream], t=t)
        return FollowStep(crops, source, tracks, vis)
