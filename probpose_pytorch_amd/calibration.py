"""``HeadCalibration``: isotonic recalibration of the probability, visibility and OKS heads, fitted on the device from
a ``ValidationMeter``.

``ValidationMeter.compute()`` says how far a predicted 0.8 is from 0.8 (reliability tables, ECE, Brier); this corrects
the number.  Every consumer of the decoded heads compares them with a fixed threshold or multiplies them into a score
(``PoseNMS`` / ``rescore_instances``, ``PoseTracker(high_thr, birth_thr)``, ``CocoKeypointEval(ex_oks=True)``,
``viz.render(threshold=...)``); a calibrated probability is what makes a fixed 0.5 mean the same from one checkpoint to
the next.

The fit is the weighted isotonic (non-decreasing) least-squares regression of the observed frequency (for the OKS head:
of the achieved OKS) on the meter's 1024 fine bins, per head and per keypoint, and once more for the keypoints pooled.
The meter's state holds all it needs as integers, so the fit is exact (``pp_calib_fit``, csrc/pp_calib.hip:
pool-adjacent-violators on integer blocks, compared with 128-bit products) and no pass over the data is repeated.
``apply`` is a table lookup by the meter's fine bin (``pp_calib_apply``), one launch that allocates nothing and so can
be captured in a graph; ``Codec(probmap, calibration=cal)`` runs it inside ``decode_device``.  ``score`` says what the
calibration makes of the samples of any meter with the same keypoints, typically a held-out one (``pp_calib_score``).

There is no CPU fallback: without a GPU the calibration raises ``HipExtensionError``.  Definitions:
include/probpose_hip.h; tests/calibration_reference.py restates them; DESIGN §4.5j.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .valmeter import BINS, check_ece_bins, head_fields

__all__ = ["HeadCalibration", "score_fields", "parse_score"]

HEADS = ("probability", "visibility", "oks")
_BINARY = ("n", "skipped", "brier", "mean_conf", "ece", "mce")
_OKS = ("n", "skipped", "ece")


def score_fields(E: int) -> int:
    return 2 * (len(_BINARY) + 3 * E) + len(_OKS) + 3 * E


def parse_score(rep: np.ndarray, ece_bins: int) -> dict:
    """The [K+1][F] float64 report of ``pp_calib_score`` as a dict per head; every field is an array of K+1 (the last
    entry pools the keypoints), ``reliability`` [K+1][E][3]."""
    out, o = {}, 0
    for head in HEADS:
        out[head], o = head_fields(rep, o, _OKS if head == "oks" else _BINARY, ece_bins)
    return out


class HeadCalibration:
    """Isotonic tables for the three decoded heads: ``cal = HeadCalibration.fit(meter)``, then ``cal(aux)`` on the
    ``[3,B,K]`` float32 ``aux`` of ``Codec.decode_device``, or ``Codec(probmap, calibration=cal)``.

    ``table`` [3][K+1][1024] float32, ``blocks`` [3][K+1][1024][2] int64 (the (P, N) behind every table entry) and
    ``row_of`` [3][K] int32 are device tensors; row K of a head is the table of the keypoints pooled."""

    def __init__(self, table: Tensor, blocks: Tensor, row_of: Tensor, min_count: int):
        K = int(row_of.shape[1])
        if tuple(table.shape) != (3, K + 1, BINS) or tuple(blocks.shape) != (3, K + 1, BINS, 2) or \
                tuple(row_of.shape) != (3, K):
            raise ValueError(f"table {tuple(table.shape)}, blocks {tuple(blocks.shape)}, row_of {tuple(row_of.shape)}: "
                             f"expected (3, K+1, {BINS}), (3, K+1, {BINS}, 2), (3, K)")
        if table.dtype != torch.float32 or blocks.dtype != torch.int64 or row_of.dtype != torch.int32:
            raise TypeError("table is float32, blocks int64, row_of int32")
        self.table, self.blocks, self.row_of = table.contiguous(), blocks.contiguous(), row_of.contiguous()
        self.K, self.min_count = K, int(min_count)

    # ------------------------------------------------------------------------------------------- fit
    @classmethod
    def fit(cls, meter, min_count: int = 1000) -> "HeadCalibration":
        """Fit on everything ``meter`` has seen; nothing comes to the host.  A keypoint with fewer than ``min_count``
        samples of a head uses the table of the keypoints pooled instead of an overfit one of its own, and passes
        through when the pool is empty too.  1000 is a convention (about one sample per fine bin), not tuned on data.
        Precondition: fewer than 2^31 samples per head, the keypoints together."""
        _lib.require_device()
        if min_count < 1:
            raise ValueError(f"min_count is at least 1, got {min_count}")
        state, K, J = meter.device_state()
        dev = state.device
        blocks = torch.empty((3, K + 1, BINS, 2), dtype=torch.int64, device=dev)
        table = torch.empty((3, K + 1, BINS), dtype=torch.float32, device=dev)
        row_of = torch.empty((3, K), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.launch("pp_calib_fit", state, K, J, int(min_count), blocks, table, row_of)
        return cls(table, blocks, row_of, min_count)

    # ------------------------------------------------------------------------------------------- apply
    def apply(self, aux: Tensor, out: Tensor | None = None) -> Tensor:
        """``aux`` [3,B,K] float32 on the device -> the calibrated values, in ``out`` (``out=aux`` works in place) or in
        a new tensor.  NaN, values outside [0, 1] and keypoints without a table pass bit for bit.  One launch."""
        _lib.require_device(aux)
        if aux.ndim != 3 or aux.shape[0] != 3 or aux.dtype != torch.float32 or not aux.is_contiguous():
            raise ValueError(f"apply takes a contiguous [3,B,K] float32 tensor, got {tuple(aux.shape)} {aux.dtype}")
        B, K = int(aux.shape[1]), int(aux.shape[2])
        if K != self.K:
            raise ValueError(f"the calibration holds {self.K} keypoints; the prediction has {K}")
        if aux.device != self.table.device:
            raise ValueError(f"the calibration is on {self.table.device}; the prediction on {aux.device}")
        if out is None:
            out = torch.empty_like(aux)
        elif out.shape != aux.shape or out.dtype != aux.dtype or out.device != aux.device or not out.is_contiguous():
            raise ValueError("out must match aux in shape, dtype, device and be contiguous")
        if B * K == 0:
            return out
        with torch.cuda.device(aux.device):
            _lib.launch("pp_calib_apply", aux, out, B, K, self.table, self.row_of)
        return out

    __call__ = apply

    # ------------------------------------------------------------------------------------------- score
    def score(self, meter, ece_bins: int = 16) -> dict:
        """What the calibration makes of the samples ``meter`` has seen (typically a held-out meter): per head and per
        keypoint (last entry: the keypoints pooled) n, skipped, ece and the reliability table of the calibrated values,
        for the two binary heads also brier, mean_conf and mce.  The numbers before calibration are
        ``meter.compute()``'s.  This is the one synchronisation."""
        _lib.require_device()
        check_ece_bins(ece_bins)
        state, K, J = meter.device_state()
        if K != self.K:
            raise ValueError(f"the calibration holds {self.K} keypoints; the meter {K}")
        if state.device != self.table.device:
            raise ValueError(f"the calibration is on {self.table.device}; the meter on {state.device}")
        rep = torch.empty((self.K + 1, score_fields(ece_bins)), dtype=torch.float64, device=state.device)
        with torch.cuda.device(state.device):
            _lib.launch("pp_calib_score", state, K, J, self.table, self.row_of, int(ece_bins), rep)
        return parse_score(rep.cpu().numpy(), ece_bins)

    # ------------------------------------------------------------------------------------------- persistence
    def state_dict(self) -> dict:
        return dict(table=self.table, blocks=self.blocks, row_of=self.row_of, K=self.K, min_count=self.min_count)

    @classmethod
    def from_state_dict(cls, sd: dict, device=None) -> "HeadCalibration":
        t = [sd[name] if device is None else sd[name].to(device) for name in ("table", "blocks", "row_of")]
        cal = cls(*t, int(sd["min_count"]))
        if cal.K != int(sd["K"]):
            raise ValueError(f"the state says K={sd['K']}; its tensors hold {cal.K} keypoints")
        return cal

    def load_state_dict(self, sd: dict) -> None:
        other = self.from_state_dict(sd, self.table.device)
        self.table, self.blocks, self.row_of = other.table, other.blocks, other.row_of
        self.K, self.min_count = other.K, other.min_count

    def save(self, path) -> None:
        sd = self.state_dict()
        torch.save({k: v.cpu() if isinstance(v, Tensor) else v for k, v in sd.items()}, path)

    @classmethod
    def load(cls, path, device="cuda") -> "HeadCalibration":
        return cls.from_state_dict(torch.load(path, map_location="cpu", weights_only=True), device)
