"""Identity and temporal smoothing for poses on video: greedy OKS association of a frame's poses with the tracks of
its stream, and a One-Euro filter per keypoint coordinate, on the GPU.  It reads what ``Codec.decode`` and ``PoseNMS``
leave on the device and keeps its state there, with the three launches of csrc/pp_track.hip per ``update``:

  pp_track_oks      one lane per (detection, slot): every pair OKS of the call
  pp_track_assign   one wave per stream; lane j % 64 owns slot j: association, ageing, births, ids
  pp_track_filter   one lane per (detection, keypoint): the One-Euro step, the output and the slot's new state

Between them run torch device ops that do not synchronise: casts to float64, two stable sorts (descending score, then
stream) and gathers.  The layout from the stream ids, the input checks with their one read-back, that visiting order
and the way back are _ragged.py's, shared with PoseNMS and CocoKeypointEval.

Rules (restated in tests/track_reference.py, the gauge this module is tested against), float64 throughout.  State per
stream: ``max_tracks`` slots (id, age, t_last, area, raw keypoints and visibilities, filter state xhat, dxhat, init) and
the counters next_id and overflow.  For every stream a call names:
* detections are visited by descending score, equal scores in the order they were given;
* the OKS of a detection and a live slot (id >= 0 when the call begins) is PoseNMS's pair OKS with the slot's stored raw
  keypoints, area and visibilities as the second detection;
* each detection, in visiting order, takes the live slot not yet taken in this call with the largest OKS (the lowest
  slot on equal OKS) if that OKS is > ``match_thr``;
* then every live slot not taken ages by one and is freed when its age exceeds ``max_age``;
* a matched detection gets the slot's id and its keypoints go through the One-Euro step with te = t - t_last; a keypoint
  that does not count in this frame (visibility <= ``vis_thr``) is passed through raw and its filter is re-initialised
  when it counts again;
* then each unmatched detection, in visiting order, takes the lowest free slot (those just freed included) with a new
  id from the stream's counter; with no slot free it gets id -1 and counts in ``overflow``.

``PoseTracker(assign="optimal")`` replaces the third rule (restated in tests/trackopt_reference.py): the
detections of a stream take the live slots by the matching of largest total weight, where a pair with OKS >
``match_thr`` weighs 1 + floor(min(OKS - match_thr, 1) * 2^40) and every other pair nothing (Hungarian assignment by
shortest augmenting paths in int64, pp_track_assign_optimal in place of pp_track_assign: still three launches).  Two
people close together then keep their ids where the greedy walk gives the first detection the other's track.  The mode
takes at most ``OPT_MAX`` = 256 slots and 256 detections per stream and call; every other rule is unchanged.

Two options, both off by default, each swapping one of the three launches (restated in
tests/trackstage_reference.py).  ``predict=True`` (pp_track_oks_predicted for pp_track_oks) replaces the slot's stored
raw keypoints in the second rule by where the track expects them: xhat + dxhat * min(t - t_last, predict_max_dt) for
a keypoint whose filter is initialised, the raw keypoint otherwise, which is the pose ``propose_boxes`` moves the
track's box by.  ``high_thr`` / ``birth_thr`` (pp_track_assign_staged for either assign launch) run the third rule in
two stages: first the detections with score >= ``high_thr`` on the live slots at ``match_thr``, then the others on
the live slots still untaken whose age at entry is <= ``low_max_age``, at ``low_match_thr``; a stage is the greedy
walk or the optimal matching, by ``assign``.  An unmatched detection is born only with score >= ``birth_thr``; the
others are dropped (id -1, ``TrackResult.dropped``) and do not count in ``overflow``.

``propose_boxes`` reads the state back out as the person box every track expects its person in next (one more launch,
pp_track_boxes; restated in tests/trackbox_reference.py); follow.py builds the frame loop on it.

There is no CPU fallback: without a GPU ``update`` and ``propose_boxes`` raise ``_lib.HipExtensionError``.
"""
from __future__ import annotations

from functools import partial

import numpy as np
import torch

from . import _lib
from ._buffers import host_array as _host, room as _room, upload
from ._ragged import (check_pose_batch, device_f64, first_seen, group_layout, host_ids, unsorted, visibilities,
                      visiting_order)

MAX_TRACKS = _lib.PP_TRACK_MAX_TRACKS
MAX_DETS_PER_STREAM = _lib.PP_TRACK_MAX_DETS
OPT_MAX = _lib.PP_TRACK_OPT_MAX         # slots, and detections per stream and call, of assign="optimal"
STREAMS_PER_CHUNK = 16


class OneEuro:
    """The constants of the One-Euro filter (Casiez et al. 2012): the cutoff at rest, its growth with speed, and the
    cutoff of the speed estimate, in Hz, 1 / (unit / second) and Hz."""
    __slots__ = ("min_cutoff", "beta", "d_cutoff")

    def __init__(self, min_cutoff: float = 1.0, beta: float = 0.05, d_cutoff: float = 1.0):
        for name, v in (("min_cutoff", min_cutoff), ("beta", beta), ("d_cutoff", d_cutoff)):
            if not np.isfinite(v):
                raise ValueError(f"{name}: {v} is not finite")
        if not min_cutoff > 0:
            raise ValueError(f"min_cutoff: {min_cutoff} is not positive")
        if not d_cutoff > 0:
            raise ValueError(f"d_cutoff: {d_cutoff} is not positive")
        if beta < 0:
            raise ValueError(f"beta: {beta} is negative")
        self.min_cutoff, self.beta, self.d_cutoff = float(min_cutoff), float(beta), float(d_cutoff)

    def __repr__(self):
        return f"OneEuro(min_cutoff={self.min_cutoff}, beta={self.beta}, d_cutoff={self.d_cutoff})"


def state_layout(max_tracks: int, K: int) -> dict:
    """name -> (byte offset, numpy dtype, shape) of a stream's state block (include/probpose_hip.h), and "bytes"."""
    T, pad8 = int(max_tracks), lambda n: (n + 7) & ~7
    parts = (("id", np.int64, (T,)), ("t_last", np.float64, (T,)), ("area", np.float64, (T,)),
             ("keypoints", np.float64, (T, K, 2)), ("vis", np.float64, (T, K)), ("xhat", np.float64, (T, K, 2)),
             ("dxhat", np.float64, (T, K, 2)), ("next_id", np.int64, (1,)), ("overflow", np.int64, (1,)),
             ("age", np.int32, (T,)), ("init", np.uint8, (T, K)))
    layout, at = {}, 0
    for name, dtype, shape in parts:
        layout[name] = (at, np.dtype(dtype), shape)
        at += pad8(int(np.prod(shape)) * np.dtype(dtype).itemsize)
    layout["bytes"] = at
    return layout


class TrackResult:
    """What ``PoseTracker.update`` returns, in the order the detections were given, on the device: ``ids`` [M] int64
    (-1 = not tracked), ``keypoints`` [M, K, 2] float64 (smoothed; raw where not smoothed), ``oks`` [M] float64 (with the
    matched track, 0 otherwise), ``born`` [M] bool, ``dropped`` [M] bool (unmatched and below ``birth_thr``: neither
    tracked nor counted in ``overflow``; all False without ``high_thr`` / ``birth_thr``); ``stream_ids``: host list in
    first-seen order."""
    __slots__ = ("ids", "keypoints", "oks", "born", "dropped", "stream_ids", "_staged")

    def __init__(self, ids, keypoints, oks, born, stream_ids, staged, dropped):
        self.ids, self.keypoints, self.oks, self.born, self.dropped = ids, keypoints, oks, born, dropped
        self.stream_ids, self._staged = stream_ids, staged

    def __repr__(self):
        return f"TrackResult({self.ids.shape[0]} detections of {len(self.stream_ids)} streams)"


class BoxProposals:
    """What ``PoseTracker.propose_boxes`` returns, on the device, over the S named streams and their T = ``max_tracks``
    slots: ``boxes`` [S, T, 4] float64 xywh, ``ids`` [S, T] int64 (-1 = free slot), ``scores`` [S, T] float64 (the mean
    visibility of the counted keypoints), ``status`` [S, T] uint8 (``_lib.PP_TRACK_BOX_*``); ``stream_ids``: host list.
    Rows that are neither PROPOSED nor SUPPRESSED hold zeros."""
    __slots__ = ("boxes", "ids", "scores", "status", "stream_ids", "_staged")

    def __init__(self, boxes, ids, scores, status, stream_ids, staged):
        self.boxes, self.ids, self.scores, self.status = boxes, ids, scores, status
        self.stream_ids, self._staged = stream_ids, staged

    def __repr__(self):
        return f"BoxProposals({self.status.shape[1]} slots of {len(self.stream_ids)} streams)"

    def compact(self):
        """The PROPOSED rows as host arrays, streams in order and slots ascending: (boxes [P, 4] float64, ids [P]
        int64, scores [P] float64, stream_index [P] int64 into ``stream_ids``).  The one call that waits for the device:
        the four tensors cross in one copy."""
        S, T = self.status.shape
        n = S * T
        if n == 0:
            return np.zeros((0, 4)), np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0, dtype=np.int64)
        raw = torch.cat([x.reshape(-1).view(torch.uint8) for x in (self.boxes, self.ids, self.scores, self.status)])
        raw = raw.cpu().numpy()
        boxes = raw[:32 * n].view(np.float64).reshape(n, 4)
        ids, scores = raw[32 * n:40 * n].view(np.int64), raw[40 * n:48 * n].view(np.float64)
        rows = np.flatnonzero(raw[48 * n:] == _lib.PP_TRACK_BOX_PROPOSED)
        return boxes[rows].copy(), ids[rows].copy(), scores[rows].copy(), (rows // T).astype(np.int64)


class PoseTracker:
    """Tracks of the poses of independent streams (cameras, videos), one frame of each named stream per ``update``.

    ``sigmas`` [K] are the per-keypoint OKS constants; ``match_thr`` in [0, 1) is the OKS a detection needs to continue
    a track; a track unseen for more than ``max_age`` frames of its stream is dropped; ``max_tracks`` slots per stream;
    ``vis_thr`` None lets every keypoint count; ``smooth`` is a ``OneEuro`` or None (raw keypoints out); ``fps`` gives
    the default time stamps; ``assign`` is "greedy" (each detection in turn takes its best free track) or "optimal"
    (the matching of largest total weight; at most ``OPT_MAX`` slots and detections per stream and call).

    Off by default (the module docstring has the rules): ``predict`` compares a detection with where the track's
    One-Euro speed expects its pose at the frame's time, ``predict_max_dt`` (None: no limit) bounding the time it
    extrapolates over; ``high_thr`` associates the detections scoring at least that much first and lets the others
    only continue tracks unseen for at most ``low_max_age`` frames, at ``low_match_thr`` (default ``match_thr``);
    ``birth_thr`` (default ``high_thr``) is the score an unmatched detection needs to start a track, the others are
    dropped.  ``birth_thr`` alone gives one stage with gated births."""

    def __init__(self, sigmas, *, match_thr: float = 0.3, max_age: int = 30, max_tracks: int = 64, vis_thr=None,
                 smooth: OneEuro | None = None, fps: float = 30.0, assign: str = "greedy", predict: bool = False,
                 predict_max_dt=None, high_thr=None, low_match_thr=None, low_max_age: int = 0, birth_thr=None):
        if predict and smooth is None:
            raise ValueError("predict: needs smooth (the speed it moves a track by is the One-Euro filter's)")
        if predict_max_dt is not None and not predict:
            raise ValueError("predict_max_dt: given without predict")
        max_dt = np.inf if predict_max_dt is None else float(predict_max_dt)
        if predict_max_dt is not None and not (np.isfinite(max_dt) and max_dt >= 0):
            raise ValueError(f"predict_max_dt: {predict_max_dt} is not None or a finite value >= 0")
        for name, v in (("high_thr", high_thr), ("birth_thr", birth_thr), ("low_match_thr", low_match_thr)):
            if v is not None and not np.isfinite(v):
                raise ValueError(f"{name}: {v} is not finite")
        if high_thr is None and low_match_thr is not None:
            raise ValueError("low_match_thr: given without high_thr, there is no second stage")
        if high_thr is None and int(low_max_age) != 0:
            raise ValueError("low_max_age: given without high_thr, there is no second stage")
        if low_match_thr is not None and not 0.0 <= float(low_match_thr) < 1.0:
            raise ValueError(f"low_match_thr: {low_match_thr} is outside [0, 1)")
        if int(low_max_age) < 0:
            raise ValueError(f"low_max_age: {low_max_age} is negative")
        self.predict, self.predict_max_dt = bool(predict), max_dt
        self.high_thr = None if high_thr is None else float(high_thr)
        self.birth_thr = self.high_thr if birth_thr is None else float(birth_thr)
        self.low_match_thr = None if low_match_thr is None else float(low_match_thr)
        self.low_max_age = int(low_max_age)
        if assign not in ("greedy", "optimal"):
            raise ValueError(f'assign: expected "greedy" or "optimal", got {assign!r}')
        self.assign = assign
        self.sigmas = _host(sigmas, "sigmas", np.float64).reshape(-1)
        if self.sigmas.size == 0 or not np.all(np.isfinite(self.sigmas)) or np.any(self.sigmas <= 0):
            raise ValueError("sigmas: need K > 0 finite positive values")
        self.K = int(self.sigmas.size)
        if not 0.0 <= float(match_thr) < 1.0:
            raise ValueError(f"match_thr: {match_thr} is outside [0, 1)")
        if int(max_age) < 0:
            raise ValueError(f"max_age: {max_age} is negative")
        if not 1 <= int(max_tracks) <= MAX_TRACKS:
            raise ValueError(f"max_tracks: {max_tracks} is outside 1..{MAX_TRACKS}")
        if assign == "optimal" and int(max_tracks) > OPT_MAX:
            raise ValueError(f'max_tracks: {max_tracks} is above the {OPT_MAX} that assign="optimal" takes')
        if vis_thr is not None and not np.isfinite(vis_thr):
            raise ValueError(f"vis_thr: {vis_thr} is not finite")
        if smooth is not None and not isinstance(smooth, OneEuro):
            raise ValueError(f"smooth: expected a OneEuro or None, got {type(smooth).__name__}")
        if not (np.isfinite(fps) and fps > 0):
            raise ValueError(f"fps: {fps} is not a positive number")
        self.match_thr, self.max_age, self.max_tracks = float(match_thr), int(max_age), int(max_tracks)
        if self.low_match_thr is None:
            self.low_match_thr = self.match_thr
        self.vis_thr = None if vis_thr is None else float(vis_thr)
        self.smooth, self.fps = smooth, float(fps)
        self.layout = state_layout(self.max_tracks, self.K)
        self._index = {}            # stream id -> its number, in first-seen order
        self._chunks = []           # uint8 [STREAMS_PER_CHUNK, bytes]: state is never reallocated, only added to
        self._device = None
        self._calls = 0
        self._t_prev = -np.inf

    # ------------------------------------------------------------------------------------------- state
    def _block(self, n: int) -> torch.Tensor:
        return self._chunks[n // STREAMS_PER_CHUNK][n % STREAMS_PER_CHUNK]

    def _field(self, block: torch.Tensor, name: str) -> torch.Tensor:
        at, dtype, shape = self.layout[name]
        nbytes = int(np.prod(shape)) * dtype.itemsize
        return block[..., at:at + nbytes].view(getattr(torch, dtype.name))

    def _clear(self, block: torch.Tensor) -> None:
        block.zero_()
        self._field(block, "id").fill_(-1)

    def _number(self, stream, device) -> int:
        n = self._index.get(stream)
        if n is None:
            n = self._index[stream] = len(self._index)
            if n // STREAMS_PER_CHUNK == len(self._chunks):
                assert _lib.call("pp_track_state_bytes", self.max_tracks, self.K) == self.layout["bytes"]
                chunk = torch.empty((STREAMS_PER_CHUNK, self.layout["bytes"]), dtype=torch.uint8, device=device)
                self._clear(chunk)
                self._chunks.append(chunk)
        return n

    def reset(self, stream=None) -> None:
        """Forget one stream's tracks, or every stream's: its slots are free and its ids restart at 0."""
        if stream is None:
            for chunk in self._chunks:
                self._clear(chunk)
        elif stream in self._index:
            self._clear(self._block(self._index[stream]))

    def tracks(self, stream) -> dict:
        """Debugging read-back (synchronises): host arrays over the stream's ``max_tracks`` slots: id (-1 = free), age,
        t_last, area, keypoints (raw), and the filter state xhat, dxhat, init."""
        if stream not in self._index:
            raise KeyError(f"stream: {stream!r} has not been seen")
        raw = self._block(self._index[stream]).cpu().numpy()
        out = {}
        for name in ("id", "age", "t_last", "area", "keypoints", "xhat", "dxhat", "init"):
            at, dtype, shape = self.layout[name]
            out[name] = raw[at:at + int(np.prod(shape)) * dtype.itemsize].view(dtype).reshape(shape).copy()
        return out

    @property
    def overflow(self) -> torch.Tensor:
        """Device int64 [number of streams seen so far]: the detections that found no free slot, per stream in
        first-seen order."""
        n = len(self._index)
        if not n:
            return torch.zeros(0, dtype=torch.int64, device=self._device or "cpu")
        return torch.cat([self._field(c, "overflow").reshape(-1) for c in self._chunks])[:n]

    def _time(self, t, previous: str) -> float:
        """The time of an ``update`` or ``propose_boxes`` call: ``t`` or the next default, past the last update's."""
        t_now = (self._calls + 1) / self.fps if t is None else float(t)
        if not (np.isfinite(t_now) and t_now > self._t_prev):
            raise ValueError(f"t: {t_now} is not greater than the previous {previous} {self._t_prev}")
        return t_now

    @staticmethod
    def _named(streams):
        """(the streams a call names as a list, stream -> its place in that list); a stream named twice raises."""
        stream_list = list(streams)
        where = {s: i for i, s in enumerate(stream_list)}
        if len(where) != len(stream_list):
            raise ValueError("streams: a stream is named twice")
        return stream_list, where

    @staticmethod
    def _places(where: dict, names: list, who: str) -> np.ndarray:
        """[len(names)] int64: every name's place in the call's streams; one the call does not name raises."""
        missing = [s for s in names if s not in where]
        if missing:
            raise ValueError(f"{who}: stream {missing[0]!r} is not in streams")
        return np.fromiter((where[s] for s in names), dtype=np.int64, count=len(names))

    # ------------------------------------------------------------------------------------------- boxes
    def _launch_boxes(self, n_str, blocks, t, frame_wh, sup_off, sup_off_dev, sup_boxes, opts, device):
        """The one launch of ``propose_boxes``: (boxes [S, T, 4], ids, scores, status) on ``device``."""
        K, T = self.K, self.max_tracks
        new = partial(torch.empty, device=device)
        boxes, ids = new((n_str, T, 4), dtype=torch.float64), new((n_str, T), dtype=torch.int64)
        scores, status = new((n_str, T), dtype=torch.float64), new((n_str, T), dtype=torch.uint8)
        pad, aspect, min_side, min_keypoints, max_age, extrapolate, max_dt, iou_thr = opts
        _lib.launch("pp_track_boxes", n_str, K, T, blocks, t, int(self.vis_thr is not None),
                    0.0 if self.vis_thr is None else self.vis_thr, int(self.smooth is not None), int(extrapolate),
                    max_dt, max_age, min_keypoints, pad, min_side, aspect, frame_wh, sup_off, sup_off_dev,
                    None if sup_boxes is None else _room(sup_boxes), iou_thr, boxes, ids, scores, status)
        return boxes, ids, scores, status

    def propose_boxes(self, t=None, *, streams=None, frame_size=None, pad: float = 1.25, aspect=None,
                      min_side: float = 2.0, min_keypoints: int = 3, max_age: int = 0, extrapolate: bool = True,
                      max_dt=None, suppress=None, iou_thr: float = 0.3) -> BoxProposals:
        """The person box every track is expected in at time ``t``, from the tracks' own last poses: what a top-down
        estimator crops next when no detector runs on the frame.  One launch (pp_track_boxes, whose rule
        include/probpose_hip.h states); it is no update: neither the state nor the call count nor the time change, and
        nothing is read back (``BoxProposals.compact`` does that).

        ``t`` defaults to the time the next default ``update`` would use and must be greater than the previous
        update's.  ``streams`` defaults to every stream seen so far, in first-seen order; an unseen one raises
        ``KeyError``.  A box is the extent of the track's counted keypoints (visibility > ``vis_thr``), taken from the
        One-Euro position, moved by the One-Euro speed times ``min(t - t_last, max_dt)`` with ``extrapolate``, or from
        the raw keypoints where no filter runs; grown by ``pad`` about its centre, at least ``min_side`` wide and high,
        widened or heightened to ``aspect`` (w / h, None: as it is) and clamped to ``frame_size``: (w, h), or
        {stream: (w, h)}, a stream it does not name is not clamped.  Tracks unseen for more than ``max_age`` of their
        stream's frames or with fewer than ``min_keypoints`` counted keypoints propose nothing.  ``suppress`` = (boxes
        [n, 4] xywh, stream_ids [n] or None for the only stream): a proposal whose IoU with one of its stream's boxes
        exceeds ``iou_thr`` is marked SUPPRESSED.  The defaults are common top-down practice, not tuned on data."""
        t_now = self._time(t, "update's")
        for name, v in (("pad", pad), ("min_side", min_side)):
            if not (np.isfinite(v) and v > 0):
                raise ValueError(f"{name}: {v} is not a positive number")
        if aspect is not None and not (np.isfinite(aspect) and aspect > 0):
            raise ValueError(f"aspect: {aspect} is not a positive number (None: none)")
        aspect = 0.0 if aspect is None else float(aspect)
        if int(min_keypoints) < 1:
            raise ValueError(f"min_keypoints: {min_keypoints} is below 1")
        if int(max_age) < 0:
            raise ValueError(f"max_age: {max_age} is negative")
        max_dt = np.inf if max_dt is None else float(max_dt)
        if not max_dt >= 0:
            raise ValueError(f"max_dt: {max_dt} is negative or not a number")
        if not 0.0 <= float(iou_thr) <= 1.0:
            raise ValueError(f"iou_thr: {iou_thr} is outside [0, 1]")
        stream_list, where = self._named(self._index if streams is None else streams)
        for s in stream_list:
            if s not in self._index:
                raise KeyError(f"stream: {s!r} has not been seen")
        n_str = len(stream_list)

        frame_wh = None
        if frame_size is not None:
            sizes = frame_size if isinstance(frame_size, dict) else dict.fromkeys(stream_list or [None], frame_size)
            frame_wh = np.zeros((n_str, 2), dtype=np.float64)
            for s, wh in sizes.items():
                wh = np.asarray(wh, dtype=np.float64).reshape(-1)
                if wh.shape != (2,) or not np.all(np.isfinite(wh)) or not np.all(wh > 0):
                    raise ValueError(f"frame_size: expected positive (w, h), got {wh.tolist()} for stream {s!r}")
                if s in where:
                    frame_wh[where[s]] = wh

        sup_off = sup_boxes = sup_perm = None
        if suppress is not None:
            sup_boxes, sup_streams = suppress
            if not isinstance(sup_boxes, torch.Tensor):
                sup_boxes = _host(sup_boxes, "suppress", np.float64)
            if sup_boxes.ndim != 2 or sup_boxes.shape[1] != 4:
                raise ValueError(f"suppress: expected boxes [n, 4], got {tuple(sup_boxes.shape)}")
            n_sup = int(sup_boxes.shape[0])
            if sup_streams is None:
                if n_sup and n_str != 1:
                    raise ValueError(f"suppress: stream_ids are needed with {n_str} streams")
                pos = np.zeros(n_sup, dtype=np.int64)
            else:
                names = host_ids(sup_streams).tolist()
                if len(names) != n_sup:
                    raise ValueError(f"suppress: expected stream_ids [{n_sup}], got {len(names)}")
                pos = self._places(where, names, "suppress")
            sup_perm = np.argsort(pos, kind="stable")                   # by stream, the given order within it
            sup_off = group_layout(pos, n_str)[1]

        _lib.require_device()
        dev = self._device if self._device is not None else torch.device("cuda")
        opts = (float(pad), aspect, float(min_side), int(min_keypoints), int(max_age), bool(extrapolate), max_dt,
                float(iou_thr))
        if n_str == 0:
            empty = partial(torch.zeros, device=dev)
            return BoxProposals(empty((0, self.max_tracks, 4), dtype=torch.float64),
                                empty((0, self.max_tracks), dtype=torch.int64),
                                empty((0, self.max_tracks), dtype=torch.float64),
                                empty((0, self.max_tracks), dtype=torch.uint8), stream_list, [])
        staged = []
        up = partial(upload, device=dev, keep=staged)
        blocks = up(np.array([self._block(self._index[s]).data_ptr() for s in stream_list], dtype=np.int64))
        frame_dev = None if frame_wh is None else up(frame_wh)
        sup_off_dev = sup_dev = None
        if sup_off is not None:
            sup_off_dev = up(sup_off)
            if isinstance(sup_boxes, torch.Tensor) and sup_boxes.is_cuda:
                sup_dev = sup_boxes.detach().to(torch.float64)[up(sup_perm)].contiguous()
            else:
                sup_dev = up(np.ascontiguousarray(np.asarray(sup_boxes, dtype=np.float64)[sup_perm]))
        out = self._launch_boxes(n_str, blocks, t_now, frame_dev, sup_off, sup_off_dev, sup_dev, opts, dev)
        return BoxProposals(*out, stream_list, staged)

    # ------------------------------------------------------------------------------------------- update
    def _launch(self, n_str, off, off_dev, det_stream, blocks, kp_s, vis_s, ar_s, sc_s, variances, t_now, t_prev):
        """The three launches on a batch in visiting order: (ids [M] int64, oks [M] float64, born [M] uint8, keypoints
        [M, K, 2] float64, dropped [M] uint8 or None), still in that order.  ``sc_s`` is read by the staged launch
        alone."""
        K, T, M, dev = self.K, self.max_tracks, int(off[-1]), kp_s.device
        new = partial(torch.empty, device=dev)
        oks_ws = new(M * T, dtype=torch.float64)
        ids_s, oks_s = new(M, dtype=torch.int64), new(M, dtype=torch.float64)
        born_s, slot_s, te_s = new(M, dtype=torch.uint8), new(M, dtype=torch.int32), new(M, dtype=torch.float64)
        out_s = new((M, K, 2), dtype=torch.float64)
        vis_thr = 0.0 if self.vis_thr is None else self.vis_thr
        vis_hold = None if vis_s is None else _room(vis_s)
        hold = [_room(x) for x in (det_stream, blocks, kp_s, ar_s, oks_ws, ids_s, oks_s, born_s, slot_s, te_s, out_s)]
        det_stream_h, blocks_h, kp_h, ar_h, ws_h, ids_h, oks_h, born_h, slot_h, te_h, out_h = hold
        oks_args = (n_str, K, T, M, off, det_stream_h, blocks_h, kp_h, vis_hold, ar_h, variances, vis_thr)
        if self.predict:
            _lib.launch("pp_track_oks_predicted", *oks_args, t_now, self.predict_max_dt, ws_h)
        else:
            _lib.launch("pp_track_oks", *oks_args, ws_h)
        # the assign entries: batch, [scores,] match_thr, [stage options,] clock and outputs, [dropped / total]
        batch = (n_str, K, T, M, off, off_dev, blocks_h, ws_h, ar_h)
        clock_and_outputs = (self.max_age, t_now, t_prev, ids_h, oks_h, born_h, slot_h, te_h)
        optimal = self.assign == "optimal"
        dropped_s = None
        if sc_s is not None:                                # update decides, once: it sorts the scores for this entry
            dropped_s = new(M, dtype=torch.uint8)
            high = -np.inf if self.high_thr is None else self.high_thr      # birth_thr alone: everything is stage 1
            _lib.launch("pp_track_assign_staged", *batch, _room(sc_s), self.match_thr, high, self.low_match_thr,
                        self.low_max_age, self.birth_thr, int(optimal), *clock_and_outputs, _room(dropped_s))
        elif optimal:
            _lib.launch("pp_track_assign_optimal", *batch, self.match_thr, *clock_and_outputs, None)
        else:
            _lib.launch("pp_track_assign", *batch, self.match_thr, *clock_and_outputs)
        sm = self.smooth
        _lib.launch("pp_track_filter", K, T, M, det_stream_h, blocks_h, kp_h, vis_hold, vis_thr, slot_h, born_h,
                    te_h, int(sm is not None), *((sm.min_cutoff, sm.beta, sm.d_cutoff) if sm else (1.0, 0.0, 1.0)),
                    out_h)
        return ids_s, oks_s, born_s, out_s, dropped_s

    def update(self, keypoints, areas, scores, kpt_scores=None, *, stream_ids=None, t=None, streams=None):
        """One frame of every named stream: keypoints [M, K, 2|3], areas [M], scores [M], kpt_scores [M, K] or None:
        device tensors of any float dtype.  ``stream_ids`` [M] says which stream a detection belongs to (host
        bookkeeping, like PoseNMS's image ids; None: one stream, id 0).  ``streams`` lists the streams this call names
        when some of them may have no detection (they still age); by default those are the streams of ``stream_ids`` in
        first-seen order.  A stream the call does not name is untouched.  ``t`` is the frame time in seconds (default:
        (number of update calls so far + 1) / fps) and must increase strictly from call to call.

        With ``kpt_scores`` they are the visibilities ``vis_thr`` reads, otherwise a third keypoint column is.  Apart
        from one finiteness boolean per input nothing is read back and nothing waits for the device."""
        named = [("keypoints", keypoints), ("areas", areas), ("scores", scores)]
        if kpt_scores is not None:
            named.append(("kpt_scores", kpt_scores))
        named, M = check_pose_batch(named, self.K, None, self.vis_thr)
        ids = np.zeros(M, dtype=np.int64) if stream_ids is None else host_ids(stream_ids)
        if ids.shape != (M,):
            raise ValueError(f"stream_ids: expected [{M}], got {ids.shape}")
        if streams is not None:
            stream_list, where = self._named(streams)
            pos = self._places(where, ids.tolist(), "stream_ids")
        else:
            stream_list, pos = first_seen(ids) if (M or stream_ids is not None) else ([0], np.zeros(0, np.int64))
        n_str = len(stream_list)
        limits = [(MAX_DETS_PER_STREAM, "that PoseTracker takes per stream and call")]
        if self.assign == "optimal":
            limits.append((OPT_MAX, 'that assign="optimal" takes per stream and call'))
        _, off = group_layout(pos, stream_list, "stream_ids: stream", limits)
        t_now = self._time(t, "call's")
        tensors = device_f64(named, "keypoints / areas / scores")      # the one read-back
        kp3, ar, sc = tensors[:3]
        dev = kp3.device
        if self._device is None:
            self._device = dev
        elif dev != self._device:
            raise ValueError(f"keypoints: on {dev}, the tracker's state is on {self._device}")
        vis = visibilities(tensors, self.vis_thr)
        addresses = np.array([self._block(self._number(s, dev)).data_ptr() for s in stream_list], dtype=np.int64)

        staged = []
        up = partial(upload, device=dev, keep=staged)
        perm, pos_dev = visiting_order(sc, pos, up)
        kp_s = kp3[..., :2][perm].contiguous()
        vis_s = None if vis is None else vis[perm].contiguous()
        ar_s, det_stream = ar[perm].contiguous(), pos_dev[perm].contiguous()
        variances, off_dev, blocks = up((self.sigmas * 2) ** 2), up(off), up(addresses)
        sc_s = sc[perm].contiguous() if self.high_thr is not None or self.birth_thr is not None else None

        ids_s, oks_s, born_s, out_s, dropped_s = self._launch(n_str, off, off_dev, det_stream, blocks, kp_s, vis_s,
                                                              ar_s, sc_s, variances, t_now, self._t_prev)
        self._calls += 1
        self._t_prev = t_now

        ids_out, oks_out, kp_out, born_out = (unsorted(perm, x) for x in (ids_s, oks_s, out_s, born_s.to(torch.bool)))
        dropped_out = (torch.zeros(M, dtype=torch.bool, device=dev) if dropped_s is None
                       else unsorted(perm, dropped_s.to(torch.bool)))
        return TrackResult(ids_out, kp_out, oks_out, born_out, stream_list, staged, dropped_out)
