"""CLEAR-MOT and identity (IDF1) metrics of tracked poses, computed on the GPU (the rule:
include/probpose_hip.h, restated in tests/trackeval_reference.py, the gauge this module is tested against).

``PoseTrackEval`` collects, frame by frame, the annotated people of a sequence (ids, keypoints, boxes, areas: host
arrays) and what a tracker said (ids and keypoints: numpy arrays or device tensors, which stay on the device) and
scores them with four HIP launches and one synchronisation, whatever the number of sequences and frames:

  pp_cocoeval_oks        the OKS matrices of all frames of all sequences: CocoKeypointEval's kernel, unchanged
  pp_trackeval_clear     per (sequence, threshold) the frames in order: the matching of largest total weight in which
                         a pair that was matched in the frame before outweighs any set of new pairs; TP FN FP IDSW, the
                         OKS sum, and per ground-truth identity the frames it was matched in and its runs
  pp_trackeval_overlap   per (sequence, threshold) c[a][b]: the frames in which identities a and b meet with OKS >= thr
  pp_trackeval_identity  per (sequence, threshold) IDTP: the largest total of c over one-to-one assignments

Ids are arbitrary non-negative int64; they become dense indices per sequence in order of first appearance, here on the
host, as cocoeval.py turns image ids into positions.  MT / PT / ML / Frag and the ratios are finished on the host from
the integers that come back.  No parity with any evaluation package is claimed.

``PoseTrackEval(..., hota=True)`` adds HOTA (Luiten et al., IJCV 2021; DESIGN 4.7h, the gauge: tests/
hota_reference.py) with OKS as the similarity: four more launches on the same stream, the same one synchronisation:

  pp_trackeval_hota_align    per frame the soft-Jaccard potential matches, added into the sequence's int64 pmc[a][b]
  pp_trackeval_hota_weights  per OKS entry the integer weight 1 + floor(A s 2^32), A the alignment of the two identities
  pp_trackeval_hota_match    per frame ONE matching of largest total weight for all alphas; per alpha the counted pairs:
                             the frame's TP and OKS sum, and mc[a][b] += 1
  pp_trackeval_hota_assoc    per (sequence, alpha) the frames added up and the association sums over mc

There is no CPU fallback: without a GPU ``evaluate()`` raises ``_lib.HipExtensionError``.

``python -m probpose_pytorch_amd.trackeval GT.json TRACKS.json [--thr 0.5[,0.75..]] [--sigmas coco17|v,v,..]
[--seq NAME] [--hota]`` scores the ``tracks.json`` of ``inference.py --track`` against ``[{frame, persons: [{id,
keypoints [K][3], bbox [4], area}]}]`` and prints one JSON line per threshold; with ``--hota`` one more line with the
eight HOTA means and the HOTA curve.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from functools import partial

import numpy as np
import torch

from . import _lib
from ._buffers import host_array as _host, room, upload
from .cocoeval import COCO17_SIGMAS

INT_KEYS = ("TP", "FN", "FP", "IDSW", "MT", "PT", "ML", "Frag", "IDTP", "IDFN", "IDFP")
RATIO_KEYS = ("MOTA", "MOTP", "IDF1", "IDP", "IDR")
MAX_FRAME, MAX_IDS = _lib.PP_TRACKEVAL_MAX_FRAME, _lib.PP_TRACKEVAL_MAX_IDS
HOTA_KEYS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")
HOTA_SUM_KEYS = ("loc_sum", "assa_sum", "assre_sum", "asspr_sum")
HOTA_MAX_ALPHAS, HOTA_MAX_FRAMES = _lib.PP_TRACKEVAL_HOTA_MAX_ALPHAS, _lib.PP_TRACKEVAL_HOTA_MAX_FRAMES


def _ratio(num, den) -> float:
    return float(np.float64(num) / np.float64(den)) if den else float("nan")


def ratios(r: dict) -> dict:
    """MOTA MOTP IDF1 IDP IDR of a record of integers and its ``oks_sum``; a ratio whose denominator is 0 is NaN."""
    return dict(MOTA=1.0 - _ratio(r["FN"] + r["FP"] + r["IDSW"], r["TP"] + r["FN"]) if r["TP"] + r["FN"] else
                float("nan"),
                MOTP=_ratio(r["oks_sum"], r["TP"]),
                IDF1=_ratio(2 * r["IDTP"], 2 * r["IDTP"] + r["IDFP"] + r["IDFN"]),
                IDP=_ratio(r["IDTP"], r["IDTP"] + r["IDFP"]),
                IDR=_ratio(r["IDTP"], r["IDTP"] + r["IDFN"]))


def _ids(x, name: str, n_max: int) -> np.ndarray:
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.ndim != 1:
        raise ValueError(f"{name}: expected [N], got {a.shape}")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: expected integers, got {a.dtype}")
    a = a.astype(np.int64)
    if a.size > n_max:
        raise ValueError(f"{name}: a frame holds {a.size}, more than PP_TRACKEVAL_MAX_FRAME = {n_max}")
    if a.size and a.min() < 0:
        raise ValueError(f"{name}: id {int(a.min())} is negative")
    if np.unique(a).size != a.size:
        vals, cnt = np.unique(a, return_counts=True)
        raise ValueError(f"{name}: id {int(vals[cnt > 1][0])} occurs twice in one frame")
    return a


def _float_dtype(a, name: str) -> None:
    ok = a.dtype.is_floating_point if isinstance(a, torch.Tensor) else np.issubdtype(a.dtype, np.floating)
    if not ok:
        raise ValueError(f"{name}: expected a float dtype for coordinates, got {a.dtype}")


def _hota_ratio(num, den, empty=0.0) -> float:
    return float(np.float64(num) / np.float64(den)) if den else empty


def hota_curves(tot: dict, alphas) -> dict:
    """``res["hota"]`` from TP FN FP (ints) and loc_sum assa_sum assre_sum asspr_sum (floats), each a list per alpha.  A
    ratio whose denominator is 0 is 0 and LocA is then 1, as HOTA's reference practice has it."""
    curves = {k: [] for k in HOTA_KEYS}
    for i in range(len(alphas)):
        tp, fn, fp = tot["TP"][i], tot["FN"][i], tot["FP"][i]
        det_a, ass_a = _hota_ratio(tp, tp + fn + fp), _hota_ratio(tot["assa_sum"][i], tp)
        for k, v in (("HOTA", math.sqrt(det_a * ass_a)), ("DetA", det_a), ("AssA", ass_a),
                     ("DetRe", _hota_ratio(tp, tp + fn)), ("DetPr", _hota_ratio(tp, tp + fp)),
                     ("AssRe", _hota_ratio(tot["assre_sum"][i], tp)), ("AssPr", _hota_ratio(tot["asspr_sum"][i], tp)),
                     ("LocA", _hota_ratio(tot["loc_sum"][i], tp, empty=1.0))):
            curves[k].append(v)
    out = dict(alphas=[float(a) for a in alphas], TP=list(tot["TP"]), FN=list(tot["FN"]), FP=list(tot["FP"]),
               curves=curves)
    out.update({k: float(np.mean(np.asarray(curves[k], dtype=np.float64))) for k in HOTA_KEYS})
    return out


class _Sequence:
    def __init__(self):
        self.gt_index, self.pred_index = {}, {}     # id -> dense index, in order of first appearance
        self.frames = []                            # (gt dense [G], kp, bb, ar, pred dense [D], pred kp)


class PoseTrackEval:
    """CLEAR-MOT and identity metrics over any number of sequences.

    ``sigmas`` [K] are the per-keypoint OKS constants; ``thresholds`` the OKS thresholds a pair needs to count, each in
    (0, 1].  ``evaluate()`` returns ``{"thresholds": [...], "metrics": [one dict per threshold], "per_sequence": {name:
    [one dict per threshold]}}``: a metrics dict holds TP FN FP IDSW MT PT ML Frag IDTP IDFN IDFP (Python ints, summed
    over the sequences) and MOTA MOTP IDF1 IDP IDR (floats; NaN where the denominator is 0); a per-sequence dict the
    integers and ``oks_sum``.

    ``hota=True`` adds ``"hota"``: ``{"alphas", "TP" / "FN" / "FP": ints per alpha, "curves": {HOTA DetA AssA DetRe
    DetPr AssRe AssPr LocA: floats per alpha}, and under the same eight names the means over the alphas}``, and
    ``"per_sequence_hota"``: ``{name: {TP FN FP loc_sum assa_sum assre_sum asspr_sum: lists per alpha}}``.
    ``hota_alphas`` (default 0.05, 0.10 .. 0.95) are the localisation thresholds, each in (0, 1], 32 at the most.
    Unlike the CLEAR keys, a HOTA ratio whose denominator is 0 is 0, and LocA is then 1: HOTA's reference practice.  A
    sequence may then have at most 2^20 frames."""

    def __init__(self, sigmas, thresholds=(0.5,), *, hota=False, hota_alphas=None):
        self.sigmas = _host(sigmas, "sigmas", np.float64).reshape(-1)
        if self.sigmas.size == 0 or not np.all(np.isfinite(self.sigmas)) or np.any(self.sigmas <= 0):
            raise ValueError("sigmas: need K > 0 finite positive values")
        self.K = int(self.sigmas.size)
        self.thresholds = _host(thresholds, "thresholds", np.float64).reshape(-1)
        if self.thresholds.size == 0:
            raise ValueError("thresholds: need at least one value")
        if not np.all((self.thresholds > 0) & (self.thresholds <= 1)):        # false for a NaN as well
            raise ValueError(f"thresholds: {self.thresholds.tolist()} are not all in (0, 1]")
        self.hota = bool(hota)
        self.hota_alphas = _host([i / 20.0 for i in range(1, 20)] if hota_alphas is None else hota_alphas,
                                 "hota_alphas", np.float64).reshape(-1)
        if self.hota_alphas.size == 0 or self.hota_alphas.size > HOTA_MAX_ALPHAS:
            raise ValueError(f"hota_alphas: need between 1 and {HOTA_MAX_ALPHAS} values, got {self.hota_alphas.size}")
        if not np.all((self.hota_alphas > 0) & (self.hota_alphas <= 1)):
            raise ValueError(f"hota_alphas: {self.hota_alphas.tolist()} are not all in (0, 1]")
        self.reset()

    def reset(self) -> None:
        """Forget every frame of every sequence."""
        self._seqs = {}

    # ------------------------------------------------------------------------------------------- collecting
    def add_frame(self, seq, gt_ids, gt_keypoints, gt_bboxes, gt_areas, pred_ids, pred_keypoints) -> None:
        """The next frame of sequence ``seq`` (any hashable): gt_ids [G] int, gt_keypoints [G, K, 3] (x, y, v),
        gt_bboxes [G, 4] xywh, gt_areas [G]; pred_ids [D] int, pred_keypoints [D, K, 2|3] (a third column is not
        used; a device tensor stays on the device).  G and D may be 0.  Nothing is kept when it raises."""
        gid = _ids(gt_ids, "gt_ids", MAX_FRAME)
        pid = _ids(pred_ids, "pred_ids", MAX_FRAME)
        G, D = gid.size, pid.size
        gt_keypoints, gt_bboxes, gt_areas = (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
                                             for a in (gt_keypoints, gt_bboxes, gt_areas))
        if gt_keypoints.ndim != 3 or gt_keypoints.shape != (G, self.K, 3):
            raise ValueError(f"gt_keypoints: expected [{G}, {self.K}, 3] (G = len(gt_ids), K = len(sigmas)), got "
                             f"{gt_keypoints.shape}")
        if gt_bboxes.shape != (G, 4):
            raise ValueError(f"gt_bboxes: expected [{G}, 4], got {gt_bboxes.shape}")
        if gt_areas.shape != (G,):
            raise ValueError(f"gt_areas: expected [{G}], got {gt_areas.shape}")
        if not isinstance(pred_keypoints, torch.Tensor):
            pred_keypoints = np.asarray(pred_keypoints)
        shape = tuple(pred_keypoints.shape)
        if len(shape) != 3 or shape[0] != D or shape[1] != self.K or shape[2] not in (2, 3):
            raise ValueError(f"pred_keypoints: expected [{D}, {self.K}, 2|3] (D = len(pred_ids), K = len(sigmas)), got "
                             f"{shape}")
        for name, a in (("gt_keypoints", gt_keypoints), ("gt_bboxes", gt_bboxes), ("gt_areas", gt_areas),
                        ("pred_keypoints", pred_keypoints)):
            if a.shape[0]:
                _float_dtype(a, name)
        kp, bb, ar = (np.ascontiguousarray(a, dtype=np.float64) for a in (gt_keypoints, gt_bboxes, gt_areas))
        for name, a in (("gt_keypoints", kp), ("gt_bboxes", bb), ("gt_areas", ar)):
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{name}: non-finite values")
        if isinstance(pred_keypoints, torch.Tensor) and pred_keypoints.is_cuda:
            pk = pred_keypoints.detach()[..., :2].to(torch.float64).contiguous()
        else:
            pk = np.ascontiguousarray(_host(pred_keypoints, "pred_keypoints", np.float64)[..., :2])
            if not np.all(np.isfinite(pk)):
                raise ValueError("pred_keypoints: non-finite values")
        key = seq.item() if isinstance(seq, np.generic) else seq
        sq = self._seqs.setdefault(key, _Sequence())
        gdense = np.fromiter((sq.gt_index.setdefault(int(i), len(sq.gt_index)) for i in gid), np.int32, count=G)
        pdense = np.fromiter((sq.pred_index.setdefault(int(i), len(sq.pred_index)) for i in pid), np.int32, count=D)
        sq.frames.append((gdense, kp.copy(), bb.copy(), ar.copy(), pdense, pk))

    # ------------------------------------------------------------------------------------------- evaluation
    def _tables(self):
        """The host arithmetic of a batch: both offset tables, the dense identity indices, the ground truth."""
        K, seqs = self.K, list(self._seqs.items())
        for name, sq in seqs:
            for what, n in (("ground-truth", len(sq.gt_index)), ("predicted", len(sq.pred_index))):
                if n > MAX_IDS:
                    raise ValueError(f"sequence {name!r} has {n} {what} identities, more than PP_TRACKEVAL_MAX_IDS = "
                                     f"{MAX_IDS}")
            if self.hota and len(sq.frames) > HOTA_MAX_FRAMES:
                raise ValueError(f"sequence {name!r} has {len(sq.frames)} frames, more than "
                                 f"PP_TRACKEVAL_HOTA_MAX_FRAMES = {HOTA_MAX_FRAMES}")
        frames = [f for _, sq in seqs for f in sq.frames]
        S, F = len(seqs), len(frames)
        g_cnt = np.array([f[0].size for f in frames], dtype=np.int64)
        d_cnt = np.array([f[4].size for f in frames], dtype=np.int64)
        offs = np.zeros((3, F + 1), dtype=np.int64)
        offs[0, 1:], offs[1, 1:], offs[2, 1:] = np.cumsum(d_cnt), np.cumsum(g_cnt), np.cumsum(d_cnt * g_cnt)
        n_f = np.array([len(sq.frames) for _, sq in seqs], dtype=np.int64)
        ng = np.array([len(sq.gt_index) for _, sq in seqs], dtype=np.int64)
        npr = np.array([len(sq.pred_index) for _, sq in seqs], dtype=np.int64)
        table = np.zeros((4, S + 1), dtype=np.int64)
        table[0, 1:], table[1, 1:], table[2, 1:], table[3, 1:] = (np.cumsum(n_f), np.cumsum(ng), np.cumsum(npr),
                                                                 np.cumsum(ng * npr))

        def cat(i, empty, dtype):
            parts = [f[i] for f in frames if f[i].shape[0]]
            return np.concatenate(parts).astype(dtype, copy=False) if parts else np.zeros(empty, dtype=dtype)

        gt_kp, gt_bb, gt_ar = cat(1, (0, K, 3), np.float64), cat(2, (0, 4), np.float64), cat(3, (0,), np.float64)
        flags = ((~(gt_kp[..., 2] > 0).any(axis=1)).astype(np.uint8) * _lib.PP_COCO_GT_NO_VISIBLE).astype(np.uint8)
        # per sequence: instances of either side, and the frames every ground-truth identity appears in
        seq_of_frame = np.repeat(np.arange(S), n_f)
        present = np.bincount(np.repeat(table[1, seq_of_frame], g_cnt) + cat(0, (0,), np.int64),
                              minlength=int(table[1, -1])).astype(np.int64)
        pred_present = np.bincount(np.repeat(table[2, seq_of_frame], d_cnt) + cat(4, (0,), np.int64),
                                   minlength=int(table[2, -1])).astype(np.int64)
        return dict(names=[n for n, _ in seqs], S=S, F=F, offs=offs, table=table, frames=frames, gt_kp=gt_kp,
                    gt_bb=gt_bb, gt_ar=gt_ar, flags=flags, gt_idx=cat(0, (0,), np.int32),
                    pred_idx=cat(4, (0,), np.int32), present=present, pred_present=pred_present,
                    n_gt=np.bincount(seq_of_frame, weights=g_cnt, minlength=S).astype(np.int64),
                    n_pred=np.bincount(seq_of_frame, weights=d_cnt, minlength=S).astype(np.int64))

    def evaluate(self) -> dict:
        """Score everything added so far (module docstring): four launches, with ``hota=True`` eight, and one
        synchronisation."""
        b = self._tables()
        _lib.require_device()
        out, sizes, keep = self._enqueue(b)
        host = out.cpu().numpy()            # the one synchronisation
        del keep
        return self._finish(b, host, *sizes)

    def _enqueue(self, b):
        """The uploads and the four launches of a batch; nothing here waits for the device.  Returns the buffer that
        comes back, the sizes of its parts, and what has to stay alive until it is back."""
        dev = torch.device("cuda")
        S, F, T, K = b["S"], b["F"], int(self.thresholds.size), self.K
        offs, table = b["offs"], b["table"]
        Dtot, Gtot, oks_total = int(offs[0, -1]), int(offs[1, -1]), int(offs[2, -1])
        n_gid, c_total = int(table[1, -1]), int(table[3, -1])
        staged = []                 # pinned host copies, alive until the results are back
        up = partial(upload, device=dev, keep=staged)
        pk = [f[5] for f in b["frames"] if f[5].shape[0]]
        if pk and not any(isinstance(p, torch.Tensor) for p in pk):         # all on the host: one upload
            pred_kp = up(np.concatenate(pk))
        elif pk:
            pred_kp = torch.cat([up(p, dtype=torch.float64) for p in pk])
        else:
            pred_kp = torch.zeros((0, K, 2), dtype=torch.float64, device=dev)
        d_offs, d_table, d_thr = up(offs), up(table), up(self.thresholds)
        args = [room(up(b[k])) for k in ("gt_kp", "gt_bb", "gt_ar", "flags")]
        variances = up((self.sigmas * 2) ** 2)
        gt_idx, pred_idx = room(up(b["gt_idx"])), room(up(b["pred_idx"]))
        oks = torch.empty(max(oks_total, 1), dtype=torch.float64, device=dev)
        _lib.launch("pp_cocoeval_oks", F, K, Dtot, Gtot, oks_total, offs, d_offs, room(pred_kp), *args, variances, oks)

        # everything that comes back, in one buffer of 8-byte words: rec [S, T, 4] | idtp [S, T] | oks_sum [S, T] f64 |
        # matched, runs [T, n_gid] int32 (two to a word)
        n_rec, n_st, n_id = 4 * S * T, S * T, (T * n_gid + 1) // 2
        # with hota, after those: tp [S, A] | sums [S, A, 4] f64 = loc, assA, assRe, assPr
        A = int(self.hota_alphas.size) if self.hota else 0
        n_base = n_rec + 2 * n_st + 2 * n_id
        out = torch.empty(max(n_base + 5 * S * A, 1), dtype=torch.int64, device=dev)
        rec, idtp = out[:n_rec], out[n_rec:n_rec + n_st]
        oks_sum = out[n_rec + n_st:n_rec + 2 * n_st].view(torch.float64)
        matched = out[n_rec + 2 * n_st:n_rec + 2 * n_st + n_id].view(torch.int32)
        runs = out[n_rec + 2 * n_st + n_id:n_rec + 2 * n_st + 2 * n_id].view(torch.int32)
        last = torch.empty(max(T * n_gid, 1), dtype=torch.int32, device=dev)
        prev = torch.empty(max(T * n_gid, 1), dtype=torch.int64, device=dev)
        c = torch.zeros(max(T * c_total, 1), dtype=torch.int32, device=dev)
        if S:
            _lib.launch("pp_trackeval_clear", S, T, F, Dtot, Gtot, oks_total, n_gid, offs, table, self.thresholds,
                        d_offs, d_table, d_thr, oks, gt_idx, pred_idx, last, prev, room(matched), room(runs), rec,
                        room(oks_sum))
            _lib.launch("pp_trackeval_overlap", S, T, F, Dtot, Gtot, oks_total, c_total, offs, table, self.thresholds,
                        d_offs, d_table, d_thr, oks, gt_idx, pred_idx, c)
            _lib.launch("pp_trackeval_identity", S, T, c_total, table, d_table, c, idtp)
        keep = [staged, pred_kp, d_offs, d_table, d_thr, args, variances, gt_idx, pred_idx, oks, last, prev, c]
        if self.hota and S:
            n_pid = int(table[2, -1])
            d_alpha = up(self.hota_alphas)
            gt_present, pred_present = room(up(b["present"])), room(up(b["pred_present"]))
            pmc = torch.zeros(max(c_total, 1), dtype=torch.int64, device=dev)
            mc = torch.zeros(max(A * c_total, 1), dtype=torch.int32, device=dev)
            q = torch.empty(max(oks_total, 1), dtype=torch.int64, device=dev)
            held_row = torch.empty(max(Dtot, 1), dtype=torch.int32, device=dev)
            frame_tp = torch.empty(max(F * A, 1), dtype=torch.int64, device=dev)
            frame_loc = torch.empty(max(F * A, 1), dtype=torch.float64, device=dev)
            h_tp = out[n_base:n_base + S * A]
            h_sums = out[n_base + S * A:n_base + 5 * S * A].view(torch.float64)
            _lib.launch("pp_trackeval_hota_align", S, F, Dtot, Gtot, oks_total, c_total, offs, table, d_offs, d_table,
                        oks, gt_idx, pred_idx, pmc)
            _lib.launch("pp_trackeval_hota_weights", S, F, Dtot, Gtot, oks_total, c_total, n_gid, n_pid, offs, table,
                        d_offs, d_table, oks, gt_idx, pred_idx, pmc, gt_present, pred_present, q)
            _lib.launch("pp_trackeval_hota_match", S, A, F, Dtot, Gtot, oks_total, c_total, offs, table,
                        self.hota_alphas, d_offs, d_table, d_alpha, oks, q, gt_idx, pred_idx, mc, held_row, frame_tp,
                        frame_loc)
            _lib.launch("pp_trackeval_hota_assoc", S, A, F, c_total, n_gid, n_pid, table, d_table, mc, gt_present,
                        pred_present, frame_tp, frame_loc, h_tp, h_sums)
            keep += [d_alpha, gt_present, pred_present, pmc, mc, q, held_row, frame_tp, frame_loc]
        return out, (n_rec, n_st, n_id), keep

    def _finish(self, b, host, n_rec, n_st, n_id) -> dict:
        S, T, table = b["S"], int(self.thresholds.size), b["table"]
        n_gid = int(table[1, -1])
        rec = host[:n_rec].reshape(S, T, 4)
        idtp = host[n_rec:n_rec + n_st].reshape(S, T)
        oks_sum = host[n_rec + n_st:n_rec + 2 * n_st].view(np.float64).reshape(S, T)
        matched = host[n_rec + 2 * n_st:n_rec + 2 * n_st + n_id].view(np.int32)[:T * n_gid].reshape(T, n_gid)
        runs = host[n_rec + 2 * n_st + n_id:n_rec + 2 * n_st + 2 * n_id].view(np.int32)[:T * n_gid].reshape(T, n_gid)
        per_sequence = {}
        for s, name in enumerate(b["names"]):
            a0, a1 = int(table[1, s]), int(table[1, s + 1])
            present = b["present"][a0:a1]
            per_sequence[name] = []
            for t in range(T):
                m, r = matched[t, a0:a1].astype(np.int64), runs[t, a0:a1].astype(np.int64)
                mt, ml = 5 * m > 4 * present, 5 * m < present
                r_ = dict(TP=int(rec[s, t, 0]), FN=int(rec[s, t, 1]), FP=int(rec[s, t, 2]), IDSW=int(rec[s, t, 3]),
                          MT=int(mt.sum()), PT=int((~mt & ~ml).sum()), ML=int(ml.sum()),
                          Frag=int(np.maximum(r - 1, 0).sum()), IDTP=int(idtp[s, t]),
                          IDFN=int(b["n_gt"][s] - idtp[s, t]), IDFP=int(b["n_pred"][s] - idtp[s, t]),
                          oks_sum=float(oks_sum[s, t]))
                per_sequence[name].append(r_)
        metrics = []
        for t in range(T):
            tot = {k: sum(per_sequence[n][t][k] for n in per_sequence) for k in INT_KEYS}
            tot["oks_sum"] = float(sum(np.float64(per_sequence[n][t]["oks_sum"]) for n in per_sequence))
            tot.update(ratios(tot))
            metrics.append(tot)
        res = dict(thresholds=[float(t) for t in self.thresholds], metrics=metrics, per_sequence=per_sequence)
        if self.hota:
            A, n_base = int(self.hota_alphas.size), n_rec + 2 * n_st + 2 * n_id
            h_tp = host[n_base:n_base + S * A].reshape(S, A)
            h_sums = host[n_base + S * A:n_base + 5 * S * A].view(np.float64).reshape(S, A, 4)
            per_seq = {}
            for s, name in enumerate(b["names"]):
                tp = [int(v) for v in h_tp[s]]
                per_seq[name] = dict(TP=tp, FN=[int(b["n_gt"][s]) - v for v in tp],
                                     FP=[int(b["n_pred"][s]) - v for v in tp],
                                     **{k: [float(v) for v in h_sums[s, :, j]] for j, k in enumerate(HOTA_SUM_KEYS)})
            tot = {k: [sum(r[k][i] for r in per_seq.values()) for i in range(A)] for k in ("TP", "FN", "FP")}
            for k in HOTA_SUM_KEYS:
                tot[k] = [float(sum(np.float64(r[k][i]) for r in per_seq.values())) for i in range(A)]
            res["hota"] = hota_curves(tot, self.hota_alphas)
            res["per_sequence_hota"] = per_seq
        return res


# ------------------------------------------------------------------------------------------------ command line
def load_json_frames(gt, tracks, K=None):
    """The frames of GT.json (a path or the parsed list) with the detections of TRACKS.json matched by frame name, in
    GT.json's order -> (list of add_frame argument tuples without ``seq``, K, the number of detections without a slot).
    A frame absent from TRACKS.json has no predictions.  A detection whose id is negative had no slot in the tracker:
    it gets a fresh id of its own, above every id of the file, and so scores as a one-frame track."""
    def read(x):
        if isinstance(x, (list, tuple)):
            return x
        with open(x) as f:
            return json.load(f)

    gt, tracks = read(gt), read(tracks)
    by_name = {}
    for fr in tracks:
        if fr["frame"] in by_name:
            raise ValueError(f"TRACKS: frame {fr['frame']!r} occurs twice")
        by_name[fr["frame"]] = fr.get("detections", [])
    if K is None:
        for fr in gt:
            for p in fr.get("persons", []):
                K = len(p["keypoints"])
                break
            if K is not None:
                break
    if K is None:
        for dets in by_name.values():
            for d in dets:
                K = len(d["keypoints"])
                break
            if K is not None:
                break
    if K is None:
        raise ValueError("neither file holds a person: the number of keypoints is unknown")
    fresh = 1 + max([int(d["id"]) for dets in by_name.values() for d in dets] + [-1])
    out, slotless = [], 0
    for fr in gt:
        persons, dets = fr.get("persons", []), by_name.get(fr["frame"], [])
        G, D = len(persons), len(dets)
        gid = np.asarray([p["id"] for p in persons], dtype=np.int64).reshape(G)
        kp = np.asarray([p["keypoints"] for p in persons], dtype=np.float64).reshape(G, K, 3)
        bb = np.asarray([p["bbox"] for p in persons], dtype=np.float64).reshape(G, 4)
        ar = np.asarray([p.get("area", p["bbox"][2] * p["bbox"][3]) for p in persons], dtype=np.float64).reshape(G)
        pid = np.zeros(D, dtype=np.int64)
        for i, d in enumerate(dets):
            pid[i] = int(d["id"])
            if pid[i] < 0:
                pid[i], fresh, slotless = fresh, fresh + 1, slotless + 1
        pk = np.asarray([d["keypoints"] for d in dets], dtype=np.float64)
        pk = pk.reshape(D, K, -1) if D else np.zeros((0, K, 2))
        out.append((gid, kp, bb, ar, pid, pk))
    return out, K, slotless


def _cli_sigmas(spec: str, K: int) -> np.ndarray:
    if spec == "coco17":
        sig = COCO17_SIGMAS.copy()
    else:
        try:
            sig = np.asarray([float(v) for v in spec.split(",")], dtype=np.float64)
        except ValueError:
            raise ValueError(f"--sigmas: expected 'coco17' or numbers separated by commas, got {spec!r}") from None
        if sig.size == 1:
            sig = np.full(K, sig[0])
    if sig.size != K:
        raise ValueError(f"--sigmas {spec}: {sig.size} values for {K} keypoints")
    return sig


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m probpose_pytorch_amd.trackeval",
                                 description="CLEAR-MOT and IDF1 (with --hota also HOTA) of a tracks.json against "
                                             "annotated tracks, computed on the GPU; prints one JSON line per OKS "
                                             "threshold.")
    ap.add_argument("ground_truth", metavar="GT.json",
                    help="[{frame, persons: [{id, keypoints [K][3], bbox [4], area}]}]")
    ap.add_argument("tracks", metavar="TRACKS.json", help="what inference.py --track writes")
    ap.add_argument("--thr", default="0.5", help="OKS thresholds in (0, 1], separated by commas")
    ap.add_argument("--sigmas", default="coco17", help="'coco17', one number for every keypoint, or K numbers")
    ap.add_argument("--seq", default="sequence", help="the name the sequence is reported under")
    ap.add_argument("--hota", action="store_true",
                    help="one more JSON line: HOTA DetA AssA DetRe DetPr AssRe AssPr LocA (means over the alphas "
                         "0.05 .. 0.95), the alphas and the HOTA curve")
    return ap


def main(argv=None) -> int:
    args = _parser().parse_args(argv)
    try:
        thr = [float(v) for v in args.thr.split(",")]
    except ValueError:
        raise ValueError(f"--thr: expected numbers separated by commas, got {args.thr!r}") from None
    frames, K, slotless = load_json_frames(args.ground_truth, args.tracks)
    ev = PoseTrackEval(_cli_sigmas(args.sigmas, K), thresholds=thr, hota=args.hota)
    for fr in frames:
        ev.add_frame(args.seq, *fr)
    res = ev.evaluate()
    print(f"{args.seq}: {len(frames)} frames; {slotless} detections without a slot scored as one-frame tracks")
    for t, m in zip(res["thresholds"], res["metrics"]):
        print(json.dumps(dict(thr=t, **{k: m[k] for k in INT_KEYS + RATIO_KEYS})))
    if args.hota:
        h = res["hota"]
        print(json.dumps(dict(**{k: h[k] for k in HOTA_KEYS}, alphas=h["alphas"], curve=h["curves"]["HOTA"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
