"""FusedAdamW: ``clip_grad_norm_`` + ``torch.optim.AdamW.step()`` of the reference's training loop
(train.py:113-115) in at most three HIP launches, whatever the number of parameter tensors.

Per step the host packs one table (pointers to p, grad, exp_avg, exp_avg_sq and the step count of every parameter
that has a gradient, its element count and group; lr, betas, eps, weight_decay per group as the scheduler left them;
a chunk -> (tensor, offset) map) with ``pp_optim_table_build``, copies it to the device asynchronously and launches
``pp_grad_sqnorm_partials``, ``pp_grad_norm_finish`` and ``pp_adamw_step`` (csrc/pp_optim.hip).  No host
synchronisation: the norm, the clip coefficient, the finite flag and every parameter's step count ``t`` stay on the
device, and the bias corrections are formed in the kernel from that ``t``.

The gradients are NOT rewritten by the clip: the coefficient is applied inside the update, so after ``step()``
``p.grad`` still holds the unclipped gradient (``clip_grad_norm_`` scales it in place; that second write of every
gradient buys nothing here).  The norm is ``optimizer.grad_norm``.

There is no CPU fallback, and nothing outside contiguous float32 parameters on one GPU is emulated: it raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List

import numpy as np
import torch

from . import _lib
from ._buffers import PinnedStaging

_STATE_KEYS = ("step", "exp_avg", "exp_avg_sq")
_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay")


def validate_state_dict(state_dict: Dict[str, Any], param_groups: List[Dict[str, Any]]) -> None:
    """Check that ``state_dict`` (torch's AdamW layout: ``state[i] = {"step", "exp_avg", "exp_avg_sq"}``, one saved
    group per group) fits the parameters of ``param_groups``.  Pure Python on shapes and keys: no device needed."""
    saved = state_dict.get("param_groups")
    state = state_dict.get("state")
    if saved is None or state is None:
        raise ValueError("FusedAdamW: a state_dict needs 'state' and 'param_groups'")
    if len(saved) != len(param_groups):
        raise ValueError(f"FusedAdamW: the state_dict has {len(saved)} parameter groups, the optimizer "
                         f"{len(param_groups)}")
    for gi, (sg, g) in enumerate(zip(saved, param_groups)):
        missing = [k for k in _GROUP_KEYS if k not in sg]
        if missing:
            raise ValueError(f"FusedAdamW: saved group {gi} lacks {missing}")
        if sg.get("amsgrad") or sg.get("maximize"):
            raise NotImplementedError(f"FusedAdamW: saved group {gi} has amsgrad / maximize set")
        if sg.get("decoupled_weight_decay") is False:
            raise NotImplementedError(f"FusedAdamW: saved group {gi} is Adam with L2 decay, not AdamW")
        if len(sg["params"]) != len(g["params"]):
            raise ValueError(f"FusedAdamW: saved group {gi} has {len(sg['params'])} parameters, the optimizer's "
                             f"{len(g['params'])}")
        for idx, p in zip(sg["params"], g["params"]):
            st = state.get(idx)
            if st is None:
                continue                                # a parameter that never had a gradient
            if set(st) != set(_STATE_KEYS):
                raise ValueError(f"FusedAdamW: state[{idx}] has keys {sorted(st)}, expected {sorted(_STATE_KEYS)}")
            for k in ("exp_avg", "exp_avg_sq"):
                if tuple(st[k].shape) != tuple(p.shape):
                    raise ValueError(f"FusedAdamW: state[{idx}][{k!r}] has shape {tuple(st[k].shape)}, the parameter "
                                     f"{tuple(p.shape)}")
            if torch.is_tensor(st["step"]) and st["step"].numel() != 1:
                raise ValueError(f"FusedAdamW: state[{idx}]['step'] has {st['step'].numel()} elements")


def _ptr_array(ts) -> np.ndarray:
    return np.fromiter((t.data_ptr() for t in ts), dtype=np.uint64, count=len(ts))


class FusedAdamW(torch.optim.Optimizer):
    """AdamW with decoupled weight decay, optional global gradient-norm clipping and an optional skip of non-finite
    steps, as HIP kernels over all parameters at once.

    The update is torch's (``p *= 1 - lr wd``; ``m``, ``v`` moving averages of the clipped gradient
    ``g min(1, max_grad_norm / (norm + 1e-6))``; ``p -= lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)``),
    and ``state_dict()`` has ``torch.optim.AdamW``'s layout, so state moves between the two.  Any
    ``torch.optim.lr_scheduler`` works: ``param_groups[i]["lr"]`` and ``["betas"]`` are read every step.

    ``max_grad_norm``: clip by the global 2-norm over every parameter that has a gradient.  The gradients themselves
    are NOT rewritten (``clip_grad_norm_`` rewrites them).  ``grad_norm``: the last step's norm, a 0-d float32 device
    tensor (None while no step has taken a norm); reading it as a number is the caller's sync, ``step()`` has none.
    ``skip_nonfinite``: a step whose gradient norm is inf or NaN leaves parameters, moments and step counts untouched
    and adds one to ``skipped_steps`` (0-d int32 device tensor).  Off by default: then it propagates, as in torch.
    Both are optimizer-wide: every group carries the same value.  ``grad_norm`` and ``skipped_steps`` are not part of
    ``state_dict()`` (torch's AdamW layout has no place for them): the counter starts at zero after a resume.

    ``step()`` runs on the current stream like any torch op.  A step issued on another stream than the one before
    first waits (on the device, not the host) for that earlier step, whose kernels read the table this one rewrites.

    Parameters whose ``.grad`` is None are left out of a step entirely (no state, no decay, not in the norm).  After
    the update each stepped parameter's autograd version counter is bumped, as for any in-place change.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_grad_norm=None,
                 skip_nonfinite=False, amsgrad=False, maximize=False):
        if amsgrad:
            raise NotImplementedError("FusedAdamW: amsgrad is not implemented")
        if maximize:
            raise NotImplementedError("FusedAdamW: maximize is not implemented")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"FusedAdamW: max_grad_norm={max_grad_norm} must be positive (or None)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=True, max_grad_norm=max_grad_norm,
                        skip_nonfinite=bool(skip_nonfinite))
        self._device = None
        self._layout = None          # element counts of the tensors whose chunk map is on the device
        self._table = None           # the device table, uint8
        self._table_bytes = 0
        self._last_step = None       # event behind the last step's kernels: they read the table the next step rewrites
        self._staging = PinnedStaging()
        self._partials = None
        self._arrive = None
        self._record = None
        self._norm_taken = False
        super().__init__(params, defaults)

    # ---- construction ------------------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        for k in ("amsgrad", "maximize"):
            if param_group.get(k):
                raise NotImplementedError(f"FusedAdamW: {k} is not implemented")
        ps = param_group["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        param_group["params"] = ps
        for p in ps:
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"FusedAdamW: cannot optimize a {type(p).__name__}")
            if p.dtype != torch.float32 or p.is_sparse or not p.is_contiguous():
                raise NotImplementedError(f"FusedAdamW: a parameter of dtype {p.dtype}, shape {tuple(p.shape)}, "
                                          f"contiguous={p.is_contiguous()} (contiguous dense float32 only)")
            _lib.require_device(p)
            if self._device is None:
                self._device = p.device
            elif p.device != self._device:
                raise NotImplementedError(f"FusedAdamW: parameters on {self._device} and {p.device} (one device "
                                          "per optimizer)")
        super().add_param_group(param_group)
        for k, v in (("lr", 0.0), ("eps", 0.0), ("weight_decay", 0.0)):
            if not float(self.param_groups[-1][k]) >= v:
                raise ValueError(f"FusedAdamW: {k}={self.param_groups[-1][k]}")
        self._layout = None

    @property
    def grad_norm(self):
        return None if self._record is None or not self._norm_taken else self._record[0:1].view(torch.float32)[0]

    @property
    def skipped_steps(self):
        self._ensure_record()
        return self._record[3]

    def _ensure_record(self):
        if self._record is None:
            self._record = torch.zeros(4, dtype=torch.int32, device=self._device)

    # ---- state -------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        validate_state_dict(state_dict, self.param_groups)
        super().load_state_dict(state_dict)
        for g in self.param_groups:       # a dict saved by torch.optim.AdamW lacks the two keys that are ours
            g.setdefault("max_grad_norm", self.defaults["max_grad_norm"])
            g.setdefault("skip_nonfinite", self.defaults["skip_nonfinite"])
            for k in ("amsgrad", "maximize"):
                g[k] = False
        for p, st in self.state.items():  # torch keeps `step` where it was saved (the CPU, for its default path)
            st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).reshape(()).to(p.device)
            for k in ("exp_avg", "exp_avg_sq"):
                st[k] = st[k].contiguous()
        self._layout = None

    # ---- the step ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        clips = {g["max_grad_norm"] for g in groups}
        skips = {bool(g["skip_nonfinite"]) for g in groups}
        if len(clips) != 1 or len(skips) != 1:
            raise ValueError("FusedAdamW: max_grad_norm and skip_nonfinite are optimizer-wide; the groups disagree: "
                             f"{sorted(map(str, clips))}, {sorted(skips)}")
        max_norm, skip = clips.pop(), skips.pop()
        if max_norm is not None and not max_norm > 0:
            raise ValueError(f"FusedAdamW: max_grad_norm={max_norm} must be positive (or None)")
        ps, gs, ms, vs, ts, gidx = [], [], [], [], [], []
        hyper = np.empty((len(groups), 5), dtype=np.float64)
        for gi, group in enumerate(groups):
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("FusedAdamW: amsgrad / maximize are not implemented")
            b1, b2 = group["betas"]
            hyper[gi] = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise NotImplementedError("FusedAdamW: sparse gradients are not implemented")
                if g.dtype != torch.float32 or p.dtype != torch.float32:
                    raise NotImplementedError(f"FusedAdamW: parameter / gradient of dtype {p.dtype} / {g.dtype} "
                                              "(float32 only)")
                if not (g.is_contiguous() and p.is_contiguous()):
                    raise NotImplementedError("FusedAdamW: a non-contiguous parameter or gradient")
                if p.device != self._device or g.device != self._device:
                    raise NotImplementedError(f"FusedAdamW: a parameter or gradient on {p.device} / {g.device}, the "
                                              f"optimizer on {self._device}")
                st = self.state[p]
                if not st:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if p.numel() == 0:
                    continue
                ps.append(p)
                gs.append(g)
                ms.append(st["exp_avg"])
                vs.append(st["exp_avg_sq"])
                ts.append(st["step"])
                gidx.append(gi)
        if not ps:
            return loss
        n = len(ps)
        with torch.cuda.device(self._device):
            counts = np.fromiter((p.numel() for p in ps), dtype=np.int64, count=n)
            layout = counts.tobytes()
            fresh = layout != self._layout
            if fresh:
                nbytes = int(_lib.call("pp_optim_table_bytes", n, counts, len(groups)))
                self._table_bytes = nbytes
                if self._table is None or self._table.numel() < nbytes:
                    self._table = torch.empty(nbytes, dtype=torch.uint8, device=self._device)
                if self._arrive is None or self._arrive.numel() < n:
                    self._arrive = torch.zeros(n, dtype=torch.int32, device=self._device)
            self._ensure_record()
            if self._last_step is not None:     # a step issued on another stream may still be reading the table
                torch.cuda.current_stream().wait_event(self._last_step)
            slot = self._staging.take(self._table_bytes)
            host = slot[0]
            arrs = [_ptr_array(x) for x in (ps, gs, ms, vs, ts)]
            group_ix = np.asarray(gidx, dtype=np.int32)
            n_chunks, prefix = C.c_int(0), C.c_longlong(0)
            _lib.call("pp_optim_table_build", n, *arrs, counts, group_ix, len(groups), hyper, self._arrive, host,
                      int(fresh), C.byref(n_chunks), C.byref(prefix))
            nb = self._table_bytes if fresh else int(prefix.value)
            self._table[:nb].copy_(host[:nb], non_blocking=True)
            slot[1].record()
            self._layout = layout
            nc = int(n_chunks.value)
            record = None
            if max_norm is not None or skip:
                if self._partials is None or self._partials.numel() < nc:
                    self._partials = torch.empty(nc, dtype=torch.float64, device=self._device)
                _lib.launch("pp_grad_sqnorm_partials", self._table, nc, self._partials)
                _lib.launch("pp_grad_norm_finish", self._partials, nc, int(max_norm is not None),
                            float(max_norm or 0.0), int(skip), self._record)
                record = self._record
                self._norm_taken = True
            _lib.launch("pp_adamw_step", self._table, nc, record, int(skip))
            if self._last_step is None:
                self._last_step = torch.cuda.Event()
            self._last_step.record()
        torch.autograd.graph.increment_version(ps)
        return loss
