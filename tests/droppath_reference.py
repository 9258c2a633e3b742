"""Float64 gauge of the ViT backbone's train-mode step with stochastic depth (timm's DropPath, scale_by_keep):
tests/vit_grad_reference.vit_forward with every residual update written as

    t = t + keep[i, j, :, None, None] / (1 - p_i) * branch(t)        (j = 0 attention, j = 1 MLP)

through an explicit autograd function, so that the scale of the backward is stated and not inherited.  ``keep`` is the
bool [depth, 2, B] mask of vit_train.draw_keep, ``rates`` the per-block p_i.

``fault`` plants what the comparators must reject: 'no_scale_backward' (forward scaled, gradient of the branch not),
'branches_swapped' (the attention mask applied to the MLP branch and the reverse), 'scale_by_rate' (1 / p in place of
1 / (1 - p)); tests/vit_grad_reference's faults pass through.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import vit_grad_reference as VR
from tests.vit_grad_reference import U_BF16, U_F32, _AddPos, _Gelu, _leaves, _Softmax, depth_of, ratio  # noqa: F401

FAULTS = ("no_scale_backward", "branches_swapped", "scale_by_rate")


class _DropPath(torch.autograd.Function):
    """t + w * branch, w [B, 1, 1] = keep / (1 - p); gradient of the branch: w * g (fault: keep * g)."""

    @staticmethod
    def forward(ctx, t, branch, w, w_back):
        ctx.save_for_backward(w_back)
        return t + w * branch

    @staticmethod
    def backward(ctx, g):
        (w_back,) = ctx.saved_tensors
        return g, w_back * g, None, None


def _weights(keep, rates, i, j, fault):
    if fault == "branches_swapped":
        j = 1 - j
    k = keep[i, j].double()[:, None, None]
    p = float(rates[i])
    if p == 0:
        return k, k
    s = 1.0 / p if fault == "scale_by_rate" else 1.0 / (1.0 - p)
    return k * s, (k if fault == "no_scale_backward" else k * s)


def vit_forward_droppath(sd, x, keep, rates, patch: int, heads: int, fault=None):
    """VisionTransformer.forward_features (B, N, C) in train mode under the keep mask."""
    g = sd.__getitem__
    t = F.conv2d(x, g("patch_embed.proj.weight"), g("patch_embed.proj.bias"), stride=patch).flatten(2).transpose(1, 2)
    t = _AddPos.apply(t, g("pos_embed"), fault == "pos_transposed")
    B, N, C = t.shape
    hd = C // heads
    for i in range(depth_of(sd)):
        p = f"blocks.{i}."
        h = F.layer_norm(t, (C,), g(p + "norm1.weight"), g(p + "norm1.bias"), 1e-6)
        qkv = F.linear(h, g(p + "attn.qkv.weight"), g(p + "attn.qkv.bias"))
        q, k, v = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
        a = _Softmax.apply((q * hd ** -0.5) @ k.transpose(-2, -1), fault == "softmax_nojac")
        o = (a @ v).transpose(1, 2).reshape(B, N, C)
        t = _DropPath.apply(t, F.linear(o, g(p + "attn.proj.weight"), g(p + "attn.proj.bias")),
                            *_weights(keep, rates, i, 0, fault))
        h = F.layer_norm(t, (C,), g(p + "norm2.weight"), g(p + "norm2.bias"), 1e-6)
        h = _Gelu.apply(F.linear(h, g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias")), fault == "gelu_grad")
        t = _DropPath.apply(t, F.linear(h, g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias")),
                            *_weights(keep, rates, i, 1, fault))
    return F.layer_norm(t, (C,), g("norm.weight"), g("norm.bias"), 1e-6)


def vit_step_droppath(state, x, upstream, keep, rates, *, patch: int, heads: int, trainable=None, fault=None):
    """One train-mode forward + backward in float64 under the keep mask, as vit_grad_reference.vit_step.  Returns
    dict(features, grads {name: tensor}); a parameter the mask cuts off has a zero gradient."""
    sd = _leaves(state, trainable)
    f = vit_forward_droppath(sd, x.detach().double(), keep, rates, patch, heads, fault=fault)
    names = [k for k, v in sd.items() if v.requires_grad]
    gr = torch.autograd.grad(f, [sd[k] for k in names], upstream.double().reshape(f.shape), allow_unused=True)
    return dict(features=f.detach(), grads={k: (g if g is not None else torch.zeros_like(sd[k]))
                                            for k, g in zip(names, gr)})


def n_stages(depth: int, droppable: int) -> int:
    """Kernel stages on the longest backward chain that round: vit_grad_reference.n_stages(depth) plus, for each of
    the ``droppable`` blocks (rate > 0) and each of its two branches, pp_droppath_add (forward: the residual stream
    every later stage reads), the scaled pp_crop_rows_gather (the branch's output gradient) and
    pp_crop_rows_scatter_add (the add into dR): 8 depth + 2 + 6 droppable."""
    return VR.n_stages(depth) + 6 * droppable
