"""The reference's ``probpose/loss.py`` (loss.py:18-712) for device tensors, with HIP backward kernels.

* ``OKSHeatmapLoss`` runs ``pp_oks_heatmap_loss`` (csrc/pp_loss.hip): oks term, MSE term and Sobel gradient energy of
  every pixel, their masks and the three reductions in one pass over the heatmaps (two launches).
* ``BCELoss`` / ``MSELoss`` / ``L1LogLoss`` on their own are the reference's few torch ops on the device.
* ``ProbPoseLoss`` decodes the gt and dt heatmap batches with ``codec.probmap.decode_device`` (one launch each, where
  the reference copies both stacks to the host and decodes them crop by crop), runs the heatmap loss on them and gets
  every B*K term -- the per-keypoint OKS and error targets, the visibility weights, the four small losses and the MAE
  accuracies -- from one ``pp_probpose_loss_terms`` launch.  One small D2H brings back the scalars and the flags the
  reference would raise on.  ``compute_acc`` adds the arg-max PCK of ``metrics.pose_pck_accuracy`` and the balanced
  binary accuracies, which draw from numpy's global RNG exactly as the reference does (only B*K values leave the
  device for them).

By default the losses are forward only: a ``pred`` tensor that requires grad while grad mode is on is refused.  With
``differentiable=True`` they carry a gradient to the predictions (a torch model trained on ROCm, as in the reference's
train.py): ``OKSHeatmapLoss`` and ``ProbPoseLoss`` are ``torch.autograd.Function``s whose backward runs
``pp_oks_heatmap_loss_backward`` and ``pp_probpose_loss_grads`` without a host sync; ``BCELoss`` / ``MSELoss`` /
``L1LogLoss`` are torch ops and simply stop refusing.  The targets, weights and masks are constants, as in the reference
(its targets come from detached decodes): one that requires grad is refused.  Without grad, ``differentiable=True`` runs
exactly the forward-only path.  The evaluation metrics the reference keeps in the same file (loss.py:715-866) are
re-exported from ``metrics`` as the same objects.
"""
from __future__ import annotations

from functools import partial
from typing import Sequence

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _buffers, _lib
from .metrics import (compute_oks, get_heatmap_expected_value, get_heatmap_maximum,  # noqa: F401
                      keypoint_pck_accuracy, oks_batch, pck_counts, pose_pck_accuracy, pose_pck_accuracy_expected)
from .util import to_numpy

__all__ = ["OKSHeatmapLoss", "BCELoss", "MSELoss", "L1LogLoss", "ProbPoseLoss", "compute_oks", "oks_batch",
           "pck_counts", "keypoint_pck_accuracy", "pose_pck_accuracy", "pose_pck_accuracy_expected",
           "get_heatmap_maximum", "get_heatmap_expected_value"]

_OKS_TYPES = {"minus": 0, "plus": 1, "both": 2}
# flags of pp_probpose_loss_terms (include/probpose_hip.h)
_FLAG_NO_ANNOTATED, _FLAG_NAN_ERROR, _FLAG_BCE_RANGE = 1, 2, 4


# reductions of pp_oks_heatmap_loss_backward (include/probpose_hip.h)
_RED_PIXEL, _RED_KEYPOINT, _RED_MEAN, _RED_PIXEL_MEAN = 0, 1, 2, 3


def _refuse_grad(*tensors) -> None:
    if _wants_grad(*tensors):
        raise RuntimeError("the ProbPose losses run forward only (HIP kernels, no backward): an input requires grad; "
                           "call them under torch.no_grad() or pass detached tensors (or differentiable=True)")


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, Tensor) and t.requires_grad for t in tensors)


def _refuse_target_grad(**tensors) -> None:
    """No gradient is provided for targets, weights or masks: refuse rather than return none."""
    names = [k for k, t in tensors.items() if isinstance(t, Tensor) and t.requires_grad]
    if names and torch.is_grad_enabled():
        raise RuntimeError(f"the ProbPose losses differentiate the predictions only; {', '.join(names)} requires "
                           "grad: detach it")


def _grad_as(g: Tensor, like) -> Tensor:
    """A float32 gradient in the (shape, dtype) of the prediction it belongs to."""
    shape, dtype = like
    g = g.view(shape)
    return g if g.dtype == dtype else g.to(dtype)


def _f32(t: Tensor, device) -> Tensor:
    t = torch.as_tensor(t)
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _oks_heatmap_loss(output, target, weights, mask, skip_empty, oks_type, sw, gw, lw, per_pixel_out,
                      per_keypoint_out, scalars):
    """Launch pp_oks_heatmap_loss; the caller checks scalars[2] (target elements outside [0, 1])."""
    B, K, H, W = output.shape
    dev = output.device
    per_pixel_weights = 0
    if weights is not None:
        per_pixel_weights = int(weights.ndim == 4)
    mask_sb = mask_sk = 0
    if mask is not None:
        mb, mk = mask.shape[0], mask.shape[1]
        mask_sb = 0 if mb == 1 else mk * H * W
        mask_sk = 0 if mk == 1 else H * W
    parts = torch.empty((B * K * 5,), dtype=torch.float32, device=dev)
    ow = 1.0 - sw - gw
    with torch.cuda.device(dev):
        _lib.launch("pp_oks_heatmap_loss", output, target, weights, per_pixel_weights, mask, mask_sb, mask_sk,
                    int(bool(skip_empty)), _OKS_TYPES[oks_type], float(sw), float(ow), float(gw), float(lw),
                    B, K, H, W, per_pixel_out, per_keypoint_out, parts, scalars)
    return parts


def _mask_strides(mask, K, H, W):
    if mask is None:
        return 0, 0
    mb, mk = mask.shape[0], mask.shape[1]
    return (0 if mb == 1 else mk * H * W), (0 if mk == 1 else H * W)


def _oks_heatmap_loss_backward(output, target, weights, mask, skip_empty, oks_type, sw, gw, lw, reduction, grad):
    """Launch pp_oks_heatmap_loss_backward: d loss / d output [B,K,H,W] f32 for the upstream gradient ``grad`` (a
    float32 device tensor, read through its strides: [B,K,H,W] per pixel, [B,K] per keypoint, 0-d for the means)."""
    B, K, H, W = output.shape
    dev = output.device
    mask_sb, mask_sk = _mask_strides(mask, K, H, W)
    strides = [0, 0, 0, 0]
    if reduction in (_RED_PIXEL, _RED_KEYPOINT):
        strides[:grad.ndim] = grad.stride()
    grad_output = torch.empty((B, K, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.launch("pp_oks_heatmap_loss_backward", output, target, weights,
                    int(weights is not None and weights.ndim == 4), mask, mask_sb, mask_sk, int(bool(skip_empty)),
                    _OKS_TYPES[oks_type], float(sw), float(1.0 - sw - gw), float(gw), float(lw), reduction, grad,
                    *strides, B, K, H, W, grad_output)
    return grad_output


def _upstream(g: Tensor, shape) -> Tensor:
    """An upstream gradient as float32 with the output's shape, strides kept (an expanded one broadcasts)."""
    g = g if g.dtype == torch.float32 else g.float()
    return g if tuple(g.shape) == tuple(shape) else g.expand(shape)


class _OKSHeatmapLossFn(torch.autograd.Function):
    """OKSHeatmapLoss with a backward: inputs (module, reduction, output, f32 operands), output the loss."""

    @staticmethod
    def forward(ctx, module, reduction, output, out, tgt, wts, msk):
        ctx.module, ctx.reduction, ctx.like = module, reduction, (output.shape, output.dtype)
        ctx.save_for_backward(out, tgt, wts, msk)
        return module._forward(out, tgt, wts, msk, reduction)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        out, tgt, wts, msk = ctx.saved_tensors
        m, red = ctx.module, ctx.reduction
        shape = {_RED_PIXEL: out.shape, _RED_KEYPOINT: out.shape[:2], _RED_MEAN: ()}[red]
        dh = _oks_heatmap_loss_backward(out, tgt, wts, msk, m.skip_empty_channel, m.oks_type, m.smoothing_weight,
                                        m.gaussian_weight, m.loss_weight, red, _upstream(g, shape))
        return None, None, _grad_as(dh, ctx.like), None, None, None, None


class OKSHeatmapLoss(nn.Module):
    """Reference loss.py:18-191: expected-OKS heatmap loss plus Sobel smoothness and MSE terms, on the GPU.

    ``differentiable=True``: with grad mode on and ``output`` requiring grad, the loss carries a gradient to
    ``output`` (all three reductions, any upstream gradient; ``pp_oks_heatmap_loss_backward``).  The default stays
    forward only; a later release may flip it."""

    def __init__(self, use_target_weight: bool = False, skip_empty_channel: bool = False,
                 smoothing_weight: float = 0.2, gaussian_weight: float = 0.0, loss_weight: float = 1.,
                 oks_type: str = "minus", differentiable: bool = False):
        super().__init__()
        self.differentiable = differentiable
        self.use_target_weight = use_target_weight
        self.skip_empty_channel = skip_empty_channel
        self.loss_weight = loss_weight
        self.smoothing_weight = smoothing_weight
        self.gaussian_weight = gaussian_weight
        self.oks_type = oks_type.lower()
        assert self.oks_type in ["minus", "plus", "both"]

    def _operands(self, output, target, target_weights, mask):
        _lib.require_device(output)
        assert output.ndim == 4 and target.shape == output.shape, \
            f"output and target shapes differ: {tuple(output.shape)} v.s. {tuple(target.shape)}"
        dev = output.device
        out, tgt = _f32(output, dev), _f32(target, dev)
        B, K, H, W = out.shape
        if mask is not None:     # loss.py:155-161
            mask = torch.as_tensor(mask)
            assert (mask.ndim == tgt.ndim and all(d_m == d_t or d_m == 1 for d_m, d_t in zip(mask.shape, tgt.shape))), (
                f'mask and target have mismatched shapes {mask.shape} v.s.{tgt.shape}')
            mask = _f32(mask, dev)
            if tuple(mask.shape[2:]) != (H, W):
                mask = mask.expand(mask.shape[0], mask.shape[1], H, W).contiguous()
        if target_weights is not None:     # loss.py:164-169
            target_weights = torch.as_tensor(target_weights)
            assert (target_weights.ndim in (2, 4) and target_weights.shape == tgt.shape[:target_weights.ndim]), (
                'target_weights and target have mismatched shapes '
                f'{target_weights.shape} v.s. {tgt.shape}')
            target_weights = _f32(target_weights, dev)
        return out, tgt, target_weights, mask

    def forward(self, output: Tensor, target: Tensor, target_weights: Tensor | None = None,
                mask: Tensor | None = None, per_pixel: bool = False, per_keypoint: bool = False) -> Tensor:
        """loss.py:55-143.  Per-pixel map [B,K,H,W], per-keypoint loss [B,K] or the scalar mean (0-d)."""
        red = _RED_PIXEL if per_pixel else (_RED_KEYPOINT if per_keypoint else _RED_MEAN)
        if not (self.differentiable and _wants_grad(output)):
            _refuse_grad(output, target, target_weights, mask)
            return self._forward(*self._operands(output, target, target_weights, mask), red)
        _refuse_target_grad(target=target, target_weights=target_weights, mask=mask)
        out, tgt, wts, msk = self._operands(output, target, target_weights, mask)
        return _OKSHeatmapLossFn.apply(self, red, output, out, tgt, wts, msk)

    def _forward(self, out, tgt, wts, msk, red):
        B, K, H, W = out.shape
        scalars = torch.empty((3,), dtype=torch.float32, device=out.device)
        pix = torch.empty_like(out) if red == _RED_PIXEL else None
        kp = torch.empty((B, K), dtype=torch.float32, device=out.device) if red == _RED_KEYPOINT else None
        _oks_heatmap_loss(out, tgt, wts, msk, self.skip_empty_channel, self.oks_type, self.smoothing_weight,
                          self.gaussian_weight, self.loss_weight, pix, kp, scalars)
        assert float(scalars[2]) == 0, 'target should be normalized'
        if red == _RED_PIXEL:
            return pix
        if red == _RED_KEYPOINT:
            return kp
        return scalars[0]


def _check_grad(module, output, target, target_weight) -> None:
    """The small losses are torch ops: differentiable ones let autograd through for ``output`` only."""
    if module.differentiable:
        _refuse_target_grad(target=target, target_weight=target_weight)
    else:
        _refuse_grad(output, target, target_weight)


class BCELoss(nn.Module):
    """Reference loss.py:194-260.  ``use_sigmoid=True`` means the inputs are probabilities (F.binary_cross_entropy),
    otherwise logits (F.binary_cross_entropy_with_logits).  ``differentiable=True``: torch's autograd differentiates
    ``output`` (the default stays forward only; a later release may flip it)."""

    def __init__(self, use_target_weight=False, loss_weight=1.0, reduction="mean", use_sigmoid=False,
                 differentiable: bool = False):
        super().__init__()
        self.differentiable = differentiable
        assert reduction in ("mean", "sum", "none"), (
            f"the argument `reduction` should be either 'mean', 'sum' or 'none', but got {reduction}")
        self.reduction = reduction
        self.use_sigmoid = use_sigmoid
        criterion = F.binary_cross_entropy if use_sigmoid else F.binary_cross_entropy_with_logits
        self.criterion = partial(criterion, reduction="none")
        self.use_target_weight = use_target_weight
        self.loss_weight = loss_weight

    def forward(self, output, target, target_weight=None):
        _check_grad(self, output, target, target_weight)
        _lib.require_device(output)
        loss = self.criterion(output, target)
        if self.use_target_weight:
            assert target_weight is not None
            if target_weight.dim() == 1:
                target_weight = target_weight[:, None]
            loss = loss * target_weight
        if self.reduction == "sum":
            loss = loss.sum()
        elif self.reduction == "mean":
            loss = loss.mean()
        return loss * self.loss_weight


class MSELoss(nn.Module):
    """Reference loss.py:263-292.  With weights both operands are multiplied by them and the mean runs over every
    entry, masked zeros included.  ``differentiable`` as in ``BCELoss``."""

    def __init__(self, use_target_weight=False, loss_weight=1.0, differentiable: bool = False):
        super().__init__()
        self.differentiable = differentiable
        self.criterion = F.mse_loss
        self.use_target_weight = use_target_weight
        self.loss_weight = loss_weight

    def forward(self, output, target, target_weight=None):
        _check_grad(self, output, target, target_weight)
        _lib.require_device(output)
        if self.use_target_weight:
            assert target_weight is not None
            loss = self.criterion(output * target_weight, target * target_weight)
        else:
            loss = self.criterion(output, target)
        return loss * self.loss_weight


class L1LogLoss(nn.Module):
    """Reference loss.py:295-339: smooth-L1 (beta 1) between log(1 + x) of both operands -- ``log(1 + x)`` as
    written, not ``log1p``.  ``differentiable`` as in ``BCELoss``."""

    def __init__(self, use_target_weight=False, loss_weight=1.0, differentiable: bool = False):
        super().__init__()
        self.differentiable = differentiable
        self.criterion = F.smooth_l1_loss
        self.use_target_weight = use_target_weight
        self.loss_weight = loss_weight

    def forward(self, output, target, target_weight=None):
        _check_grad(self, output, target, target_weight)
        _lib.require_device(output)
        output = torch.log(1 + output)
        target = torch.log(1 + target)
        if self.use_target_weight:
            assert target_weight is not None
            assert output.ndim >= target_weight.ndim
            for _ in range(output.ndim - target_weight.ndim):
                target_weight = target_weight.unsqueeze(-1)
            loss = self.criterion(output * target_weight, target * target_weight)
        else:
            loss = self.criterion(output, target)
        return loss * self.loss_weight


def _host_int(x, B: int, C: int) -> np.ndarray:
    """A (B,1,C) / (B,C) mask (numpy, host or device tensor) -> int64 (B,C) like the reference's ``.to(int)``."""
    t = x.detach().cpu() if isinstance(x, Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(torch.int64).reshape(B, C).numpy()


def _binary_accuracy(dt: np.ndarray, gt: np.ndarray, mask: np.ndarray, device, force_balanced=False):
    """loss.py:653-697 on host copies of B*K values: the same numpy calls in the same order, so the same draws
    from numpy's global RNG."""
    assert dt.shape == gt.shape
    dt = dt[mask]
    gt = gt[mask]
    gt = gt.astype(bool)
    if force_balanced:
        pos_num = np.sum(gt)
        neg_num = len(gt) - pos_num
        num = min(pos_num, neg_num)
        if num == 0:
            return torch.tensor([0.0], device=device), torch.tensor([0.0], device=device)
        pos_idx = np.where(gt)[0]
        neg_idx = np.where(~gt)[0]
        np.random.shuffle(pos_idx)
        np.random.shuffle(neg_idx)
        idx = np.concatenate([pos_idx[:num], neg_idx[:num]])
        dt = dt[idx]
        gt = gt[idx]
    n_samples = len(gt)
    thresholds = np.arange(0.1, 1.0, 0.05)
    preds = dt[:, None] > thresholds
    correct = preds == gt[:, None]
    counts = correct.sum(axis=0)
    best_idx = np.argmax(counts)
    best_threshold = thresholds[best_idx]
    best_acc = counts[best_idx] / n_samples
    return (torch.tensor(best_acc, device=device).float(), torch.tensor(best_threshold, device=device).float())


_LOSS_KEYS = ("kpt", "probability", "visibility", "oks", "error")


class _ProbPoseLossFn(torch.autograd.Function):
    """ProbPoseLoss.forward as one autograd node: inputs (module, gt, keypoint_weights, learn_heatmaps_from_zeros, box,
    the five predictions), outputs the five losses.  ``box`` receives the forward's terms for ``compute_acc``."""

    @staticmethod
    def forward(ctx, module, gt, keypoint_weights, from_zeros, box, *pred):
        T = module.terms(gt, pred, keypoint_weights, from_zeros)
        losses = module._losses(T)
        box["T"] = T
        ctx.module = module
        ctx.like = [(p.shape, p.dtype) for p in pred]
        ctx.save_for_backward(T["hm"], T["gt_hm"], T["heat_w"], *T["heads"], T["gt_oks"], T["gt_err"], T["masks"])
        return tuple(losses[k] for k in _LOSS_KEYS)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_kpt, g_prob, g_vis, g_oks, g_err):
        hm, gt_hm, heat_w, dt_prob, dt_vis, dt_oks, dt_err, gt_oks, gt_err, masks = ctx.saved_tensors
        need = ctx.needs_input_grad[5:]
        grads = [None] * 5
        km = ctx.module.keypoint_loss_module
        if need[0]:         # loss.py:427-431: heatmap_loss_pxl.mean()
            dh = _oks_heatmap_loss_backward(hm, gt_hm, heat_w, None, km.skip_empty_channel, km.oks_type,
                                            km.smoothing_weight, km.gaussian_weight, km.loss_weight, _RED_PIXEL_MEAN,
                                            _upstream(g_kpt, ()))
            grads[0] = _grad_as(dh, ctx.like[0])
        if any(need[1:]):   # loss.py:432-464, one launch for the four heads
            B, K = hm.shape[:2]
            d = torch.empty((4, B * K), dtype=torch.float32, device=hm.device)
            u = [_upstream(g, ()).contiguous() for g in (g_prob, g_vis, g_oks, g_err)]
            with torch.cuda.device(hm.device):
                _lib.launch("pp_probpose_loss_grads", dt_prob, dt_vis, dt_oks, dt_err, gt_oks, gt_err, *masks[:3], *u,
                            B, K, *d)
            for i in range(4):
                if need[1 + i]:
                    grads[1 + i] = _grad_as(d[i], ctx.like[1 + i])
        return (None, None, None, None, None, *grads)


class ProbPoseLoss(nn.Module):
    """Reference loss.py:342-712: the five per-head losses of the training and validation loops and, with
    ``compute_acc``, the five accuracies.

    ``differentiable=True``: with grad mode on and a prediction requiring grad, the five losses come from one autograd
    node whose backward computes the heatmap gradient (``pp_oks_heatmap_loss_backward``, skipped when the heatmaps need
    none) and the four head gradients (``pp_probpose_loss_grads``) on the device, reading the upstream gradients there:
    no host sync.  The OKS and error targets are constants, as in the reference (detached decodes); the accuracies
    carry no gradient; double backward is an error.  The default stays forward only; a later release may flip it."""

    def __init__(self, codec, freeze_error: bool = True, differentiable: bool = False):
        super().__init__()
        self.differentiable = differentiable
        self.codec = codec
        self.keypoint_loss_module = OKSHeatmapLoss(use_target_weight=True, smoothing_weight=0.05, oks_type="minus")
        self.probability_loss_module = BCELoss(use_target_weight=False, use_sigmoid=True)
        self.visibility_loss_module = BCELoss(use_target_weight=False, use_sigmoid=True)
        self.oks_loss_module = MSELoss(use_target_weight=True)
        self.error_loss_module = L1LogLoss(use_target_weight=True)
        self.freeze_error = freeze_error
        self.freeze_oks = False
        self._variance = {}

    def _device_variance(self, K, dev):
        sig = np.asarray(self.codec.probmap.sigmas)
        key = (str(dev), sig.dtype.str, sig.tobytes())
        v = self._variance.get(key)
        if v is None:
            keep = []       # the pinned source of the asynchronous upload lives as long as the cached copy
            v = _buffers.upload(np.ascontiguousarray((sig * 2) ** 2, dtype=np.float64), dev, keep)   # compute_oks :716
            self._variance, self._variance_host = {key: v}, keep
        if v.numel() != K:
            raise ValueError(f"{K} keypoints but {v.numel()} sigmas")
        return v

    def terms(self, gt, pred, keypoint_weights=None, learn_heatmaps_from_zeros: bool = False) -> dict:
        """Every device-side quantity of one forward: the decodes (gt_kpts, dt_kpts), the B*K targets (gt_oks,
        gt_err, vis_weight, oks_weight), ``res`` = the 11 scalars of both kernels, the int masks on the device
        (``masks``: in_image, annotated, visibility) and on the host, and the heatmap weights (``heat_w``)."""
        dev, (B, C, _, _) = self._check_pred(pred)
        probs = _host_int(gt["in_image"], B, C)
        annotated = _host_int(gt["keypoints_visible"], B, C)
        vis = _host_int(gt["keypoints_visibility"], B, C)
        masks = torch.from_numpy(np.stack([probs, annotated, vis]).astype(np.int32)).to(dev)
        T = self._device_terms(gt, pred, masks, keypoint_weights, learn_heatmaps_from_zeros)
        T.update(probs=probs, annotated=annotated, vis=vis)
        return T

    def _check_pred(self, pred):
        if self.freeze_oks:
            raise NotImplementedError("freeze_oks is not supported (the reference never sets it)")
        _refuse_grad(*pred)
        _lib.require_device(pred[0])
        return pred[0].device, pred[0].shape

    def _device_terms(self, gt, pred, masks, keypoint_weights=None, learn_heatmaps_from_zeros: bool = False) -> dict:
        """The launch sequence of ``terms`` for masks that are on the device already (``masks`` [3,B,K] int32:
        in_image, annotated, visibility): nothing here reads a device value on the host."""
        dev, (B, C, H, W) = self._check_pred(pred)
        dt_heatmaps, dt_probs, dt_vis, dt_oks, dt_errs = pred
        hm = _f32(dt_heatmaps, dev)
        gt_hm = _f32(gt["heatmaps"], dev).view(B, C, H, W)
        if keypoint_weights is None:
            kw = torch.ones((B, C), device=dev, dtype=torch.float32)
        else:
            kw = _f32(keypoint_weights, dev).view(B, C)
        heads = []
        for t in (dt_probs, dt_vis, dt_oks, dt_errs):
            t = _f32(t, dev).view(-1)
            if t.numel() != B * C:
                raise ValueError(f"scalar heads must hold B*K = {B * C} values, got {t.numel()}")
            heads.append(t)
        # both decodes on the whole batch, no heatmap leaves the device (loss.py:574-585 decodes crop by crop)
        gt_kpts = self.codec.probmap.decode_device(gt_hm)["kpts"]
        dt_kpts = self.codec.probmap.decode_device(hm)["kpts"]
        res = torch.empty((11,), dtype=torch.float32, device=dev)
        heat_weights = masks[1].float() if learn_heatmaps_from_zeros else kw     # loss.py:423-426
        km = self.keypoint_loss_module
        _oks_heatmap_loss(hm, gt_hm, heat_weights, None, km.skip_empty_channel, km.oks_type, km.smoothing_weight,
                          km.gaussian_weight, km.loss_weight, None, None, res[0:3])
        gt_oks = torch.empty((B, C), dtype=torch.float32, device=dev)
        gt_err = torch.empty((B, C), dtype=torch.float32, device=dev)
        vis_weight = torch.empty((B, C), dtype=torch.float32, device=dev)
        oks_weight = torch.empty((B,), dtype=torch.float32, device=dev)
        oks_area = (W * H) * 0.53 + np.spacing(1)    # bbox [0, 0, H, W] from heatmap_size=(W, H) (loss.py:395, :609-620)
        var = self._device_variance(C, dev)
        with torch.cuda.device(dev):
            _lib.launch("pp_probpose_loss_terms", gt_kpts, dt_kpts, *masks[:3], *heads, var, float(oks_area), B, C,
                        int(bool(self.freeze_error)), gt_oks, gt_err, vis_weight, oks_weight, res[3:])
        return dict(hm=hm, gt_hm=gt_hm, kw=kw, heads=heads, gt_kpts=gt_kpts, dt_kpts=dt_kpts, gt_oks=gt_oks,
                    gt_err=gt_err, vis_weight=vis_weight, oks_weight=oks_weight, res=res, masks=masks,
                    heat_w=heat_weights)

    def forward(self, gt, pred: Sequence[Tensor], keypoint_weights: Tensor | None = None,
                learn_heatmaps_from_zeros: bool = False, compute_acc: bool = False):
        """loss.py:360-510: ``losses`` (kpt, probability, visibility, oks, error), and ``(losses, accs)`` with
        ``compute_acc``; 0-d device tensors."""
        if self.differentiable and _wants_grad(*pred):
            gh = gt["heatmaps"] if isinstance(gt, dict) else None
            _refuse_target_grad(gt_heatmaps=gh, keypoint_weights=keypoint_weights)
            box = {}
            out = _ProbPoseLossFn.apply(self, gt, keypoint_weights, learn_heatmaps_from_zeros, box, *pred)
            T, losses = box["T"], dict(zip(_LOSS_KEYS, out))
        else:
            T = self.terms(gt, pred, keypoint_weights, learn_heatmaps_from_zeros)
            losses = self._losses(T)
        if not compute_acc:
            return losses
        return losses, self._accuracies(T)

    def _losses(self, T) -> dict:
        """The reference's raises from one small D2H, then the five losses (views of the kernels' results)."""
        res = T["res"]
        host = res.cpu().numpy()          # the one sync: the scalars the reference would raise on
        flags = int(host[9])
        if flags & _FLAG_NAN_ERROR:
            raise AssertionError("Euclidean distance cannot be negative")
        if host[2] != 0:
            raise AssertionError('target should be normalized')
        if flags & _FLAG_BCE_RANGE:
            raise RuntimeError("all elements of input should be between 0 and 1")
        if flags & _FLAG_NO_ANNOTATED:
            raise RuntimeError("min(): Expected reduction dim to be specified for input.numel() == 0 "
                               "(loss.py:448: the batch has no annotated keypoint)")
        return dict(kpt=res[1], probability=res[3], visibility=res[4], oks=res[5], error=res[6])

    def _accuracies(self, T) -> dict:
        res = T["res"]
        dev = res.device
        _, avg_acc, _ = pose_pck_accuracy(T["hm"], T["gt_hm"], T["kw"] > 0.5, method="argmax")    # loss.py:642-651
        acc_pose = torch.tensor(avg_acc, device=dev)
        small = torch.stack([T["heads"][0], T["heads"][1]]).cpu().numpy()
        B, C = T["probs"].shape
        dt_probs, dt_vis = small[0].reshape(B, C), small[1].reshape(B, C)
        annotated_in = T["annotated"] & (T["probs"] > 0.5)
        acc_prob, _ = _binary_accuracy(dt_probs, T["probs"], T["annotated"] > 0.5, dev, force_balanced=True)
        acc_vis, _ = _binary_accuracy(dt_vis, T["vis"], annotated_in > 0.5, dev, force_balanced=True)
        return {"kpt": acc_pose, "probability": acc_prob, "visibility": acc_vis, "oks": res[7], "error": res[8]}

    def get_binary_accuracy(self, dt, gt, mask, force_balanced=False):
        """loss.py:653-697."""
        device = gt.device if isinstance(gt, Tensor) else None
        return _binary_accuracy(to_numpy(dt), to_numpy(gt), to_numpy(mask), device, force_balanced)
