"""ModelEma: an exponential moving average of a model's weights (timm's ``ModelEmaV2``, Ultralytics' ``ModelEMA``),
updated by ONE HIP launch whatever the number of state tensors.

``ema_update_(dsts, srcs, weight)`` is the multi-tensor primitive: ``dst += weight (src - dst)`` for float32 tensors
(evaluated in float64, rounded once at the store) and ``dst = src`` for everything else (BatchNorm's int64
``num_batches_tracked``), over all tensors at once (csrc/pp_ema.hip).  The device table that describes the tensors
depends on their addresses and sizes only, so it is built and uploaded once and reused until one of them changes.
No host synchronisation; afterwards the autograd version counter of every written tensor is bumped, as for any
in-place change: ``engine.plan_for`` keys its packed weights on it, so an averaged module never serves a stale plan.

There is no CPU fallback, and nothing outside contiguous tensors on one GPU is emulated: it raises.
"""
from __future__ import annotations

import ctypes as C
import math
from copy import deepcopy
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._buffers import CaptureCache

_plans = CaptureCache(16)       # key -> _Plan: the device table and its pinned host copy live and die together


class _Plan:
    """The uploaded table of one list of (src, dst) pairs."""

    def __init__(self, device, table, host, n_chunks):
        self.device = device
        self.table = table              # uint8 on the device
        self.host = host                # the pinned buffer the asynchronous upload reads; never rewritten
        self.n_chunks = n_chunks
        self.stream = torch.cuda.current_stream(device)
        self.uploaded = torch.cuda.Event()
        self.uploaded.record(self.stream)

    def launch(self, weight: float) -> None:
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream()
            if stream != self.stream:   # the upload was queued on another stream: wait for it on the device
                stream.wait_event(self.uploaded)
            _lib.launch("pp_ema_update", self.table, self.n_chunks, float(weight))


def _kind_of(t: torch.Tensor, what: str) -> int:
    if t.dtype == torch.float32:
        return _lib.PP_EMA_LERP_F32
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise NotImplementedError(f"ema_update_: {what} has dtype {t.dtype} (float32 is averaged, non-float state is "
                                  "copied; other floating types are not implemented)")
    if t.element_size() % 4 != 0:
        raise NotImplementedError(f"ema_update_: {what} has dtype {t.dtype}, whose size is not a multiple of 4 bytes")
    return _lib.PP_EMA_COPY_WORDS


def _check_disjoint(rows) -> None:
    """rows: (src address, dst address, bytes, index).  Every dst range must be disjoint from every src range and
    from every other dst range."""
    spans = []
    for s, d, nbytes, i in rows:
        spans.append((s, s + nbytes, False, i))
        spans.append((d, d + nbytes, True, i))
    spans.sort()
    end_any, end_dst, who_any, who_dst = 0, 0, -1, -1
    for lo, hi, is_dst, i in spans:
        if lo < end_dst:
            raise ValueError(f"ema_update_: tensor {i} overlaps the destination {who_dst}")
        if is_dst and lo < end_any:
            raise ValueError(f"ema_update_: destination {i} overlaps tensor {who_any}")
        if hi > end_any:
            end_any, who_any = hi, i
        if is_dst and hi > end_dst:
            end_dst, who_dst = hi, i


def _plan_for(dsts: Sequence[torch.Tensor], srcs: Sequence[torch.Tensor]) -> Tuple[Optional[_Plan], list]:
    """The cached plan of these pairs and the indices (into the lists) of the tensors the kernel writes."""
    if len(dsts) != len(srcs):
        raise ValueError(f"ema_update_: {len(dsts)} destinations, {len(srcs)} sources")
    rows, seen, device = [], set(), None
    for i, (d, s) in enumerate(zip(dsts, srcs)):
        if not (isinstance(d, torch.Tensor) and isinstance(s, torch.Tensor)):
            raise TypeError(f"ema_update_: pair {i} is ({type(d).__name__}, {type(s).__name__}), not tensors")
        if d.dtype != s.dtype:
            raise ValueError(f"ema_update_: pair {i} has dtypes {d.dtype} and {s.dtype}")
        if tuple(d.shape) != tuple(s.shape):
            raise ValueError(f"ema_update_: pair {i} has shapes {tuple(d.shape)} and {tuple(s.shape)}")
        kind = _kind_of(d, f"pair {i}")
        if d.is_sparse or s.is_sparse or not (d.is_contiguous() and s.is_contiguous()):
            raise NotImplementedError(f"ema_update_: pair {i} is not contiguous and dense")
        if d.device != s.device or (device is not None and d.device != device):
            raise NotImplementedError(f"ema_update_: pair {i} is on {d.device} / {s.device}, the others on "
                                      f"{device or d.device} (one device per update)")
        device = d.device
        if d.numel() == 0:
            continue
        row = (s.data_ptr(), d.data_ptr(), d.numel() * d.element_size(), kind)
        if row in seen:                 # the same pair twice (tied weights): once is enough
            continue
        seen.add(row)
        rows.append((*row, i))
    written = [r[4] for r in rows]

    def build():
        _check_disjoint([(s, d, nbytes, i) for s, d, nbytes, _, i in rows])
        for d in dsts:
            _lib.require_device(d)
        n = len(rows)
        src = np.fromiter((r[0] for r in rows), dtype=np.uint64, count=n)
        dst = np.fromiter((r[1] for r in rows), dtype=np.uint64, count=n)
        counts = np.fromiter((r[2] // 4 for r in rows), dtype=np.int64, count=n)
        kinds = np.fromiter((r[3] for r in rows), dtype=np.int32, count=n)
        nbytes = int(_lib.call("pp_ema_table_bytes", n, counts))
        with torch.cuda.device(device):
            host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            n_chunks = C.c_int(0)
            _lib.call("pp_ema_table_build", n, src, dst, counts, kinds, host, C.byref(n_chunks))
            table = torch.empty(nbytes, dtype=torch.uint8, device=device)
            table.copy_(host, non_blocking=True)
            return _Plan(device, table, host, int(n_chunks.value))

    if not rows:                        # nothing but zero-element tensors
        for d in dsts:
            _lib.require_device(d)
        return None, written
    return _plans.get((str(device), tuple(r[:4] for r in rows)), build), written


def _run(plan: Optional[_Plan], written, dsts: Sequence[torch.Tensor], weight: float) -> None:
    if not 0.0 <= weight <= 1.0:
        raise ValueError(f"ema_update_: weight={weight} is not in [0, 1]")
    if plan is None:
        return
    plan.launch(weight)
    torch.autograd.graph.increment_version([dsts[i] for i in written])


@torch.no_grad()
def ema_update_(dsts: Sequence[torch.Tensor], srcs: Sequence[torch.Tensor], weight: float) -> None:
    """``dsts[i] += weight (srcs[i] - dsts[i])`` for float32 pairs (float64 arithmetic, one rounding), ``dsts[i] =
    srcs[i]`` for pairs of any non-float dtype whose element size is a multiple of 4 bytes; all pairs in one launch on
    the current stream, no host synchronisation.  The pairs are equally shaped contiguous tensors on one GPU; no
    destination may overlap a source or another destination.  Zero-element pairs are skipped.

    Raises NotImplementedError for a floating dtype other than float32, a non-contiguous tensor or a second device;
    ValueError for shape or dtype mismatches and overlapping tensors; there is no CPU fallback."""
    dsts, srcs = list(dsts), list(srcs)
    _run(*_plan_for(dsts, srcs), dsts, float(weight))


class ModelEma:
    """An averaged copy of ``model``: ``.module = deepcopy(model).eval()`` with ``requires_grad_(False)``.

    ``update(model)`` moves every float32 entry of ``module.state_dict()`` (parameters AND buffers, so the BatchNorm
    running statistics too, as in timm) towards the entry of the same name in ``model.state_dict()``:
    ``ema = decay_t ema + (1 - decay_t) model``; every other entry (``num_batches_tracked``) is copied.  One launch
    (``ema_update_``), no host synchronisation.

    ``decay_at(t)``: ``decay`` when ``tau`` is None (timm), else ``decay (1 - exp(-t / tau))`` (Ultralytics' warm-up:
    early updates follow the model closely); ``t`` is the number of the update, from 1.

    ``state_dict()`` is ``{"module": module.state_dict(), "updates", "decay", "tau"}``; ``load_state_dict`` restores
    it and a resumed run continues the same decay sequence.  ``module.state_dict()`` alone is an ordinary model
    checkpoint.  ``.module`` is a plain module: eval, flip test, decode and sharding take it unchanged.
    """

    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, tau: Optional[float] = None):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"ModelEma: decay={decay} is not in [0, 1]")
        if tau is not None and not float(tau) > 0.0:
            raise ValueError(f"ModelEma: tau={tau} must be positive (or None)")
        self.module = deepcopy(model).eval()
        self.module.requires_grad_(False)
        for p in self.module.parameters():
            p.grad = None
        self.decay = float(decay)
        self.tau = None if tau is None else float(tau)
        self.updates = 0
        self._keys = list(self.module.state_dict(keep_vars=True))
        self._plan = None
        self._sig = None

    def decay_at(self, t: int) -> float:
        if self.tau is None:
            return self.decay
        return self.decay * (1.0 - math.exp(-t / self.tau))

    def _pairs(self, model: torch.nn.Module):
        src = model.state_dict(keep_vars=True)
        dst = self.module.state_dict(keep_vars=True)
        if list(src) != self._keys or list(dst) != self._keys:
            missing = sorted(set(self._keys) - set(src))
            extra = sorted(set(src) - set(self._keys))
            raise ValueError(f"ModelEma: the model's state no longer matches the average: missing {missing[:5]}, "
                             f"unexpected {extra[:5]}" if missing or extra else
                             "ModelEma: the order of the model's state entries changed")
        dsts, srcs = list(dst.values()), list(src.values())
        for k, d, s in zip(self._keys, dsts, srcs):
            if d.shape != s.shape:
                raise ValueError(f"ModelEma: {k} has shape {tuple(s.shape)} in the model, {tuple(d.shape)} in the "
                                 "average")
        return dsts, srcs

    @torch.no_grad()
    def update(self, model: torch.nn.Module) -> None:
        dsts, srcs = self._pairs(model)
        _lib.require_device(next((t for t in srcs + dsts if not t.is_cuda), None))
        sig = tuple((d.data_ptr(), s.data_ptr()) for d, s in zip(dsts, srcs))
        if sig != self._sig:            # first update, or a tensor moved (.to(), a reassigned parameter)
            self._plan = _plan_for(dsts, srcs)
            self._sig = sig
        self.updates += 1
        _run(*self._plan, dsts, 1.0 - self.decay_at(self.updates))

    def state_dict(self) -> Dict[str, Any]:
        return {"module": self.module.state_dict(), "updates": self.updates, "decay": self.decay, "tau": self.tau}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        missing = [k for k in ("module", "updates", "decay", "tau") if k not in state]
        if missing:
            raise ValueError(f"ModelEma: the state_dict lacks {missing}")
        self.module.load_state_dict(state["module"])
        self.updates = int(state["updates"])
        self.decay = float(state["decay"])
        self.tau = None if state["tau"] is None else float(state["tau"])
