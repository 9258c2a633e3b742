"""Float64 gauge of the ViT backbone's train-mode step: ``oracle.probpose_oracle.vit_forward_features`` restated with
the three pieces whose backward convention matters written out as explicit autograd functions -- the exact-erf GELU
(d/dx = Phi(x) + x phi(x)), the softmax (Jacobian p (g - sum(g p))) and the pos_embed add (its gradient a sum over
crops) -- and differentiated by torch's float64 autograd.  ``model_step`` composes it with
tests/head_grad_reference.head_forward for ProbPoseModel steps.

``fault`` plants what the comparators must reject: 'gelu_grad' (GELU derivative without the x phi(x) term),
'softmax_nojac' (the softmax backward without its -p sum(g p) term), 'pos_transposed' (the pos_embed gradient summed
over the rows as if they were token-major, [N, B] instead of [B, N]).

Bounds: |got - want| <= c u max|want| per tensor (head_grad_reference.ratio), c derived in the GPU tests.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests.head_grad_reference import U_BF16, U_F32, head_forward, ratio  # noqa: F401

FAULTS = ("gelu_grad", "softmax_nojac", "pos_transposed")


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fault):
        ctx.save_for_backward(x)
        ctx.fault = fault
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
        pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        return g * (cdf if ctx.fault else cdf + x * pdf), None


class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, fault):
        p = a.softmax(-1)
        ctx.save_for_backward(p)
        ctx.fault = fault
        return p

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        if ctx.fault:
            return g * p, None
        return p * (g - (g * p).sum(-1, keepdim=True)), None


class _AddPos(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, pos, fault):
        ctx.fault = fault
        return t + pos

    @staticmethod
    def backward(ctx, g):
        B, N, C = g.shape
        gp = g.reshape(N, B, C).sum(1) if ctx.fault else g.sum(0)
        return g, gp.reshape(1, N, C), None


def depth_of(sd) -> int:
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))


def vit_forward(sd, x, *, patch: int, heads: int, fault=None):
    """VisionTransformer.forward_features (B, N, C), as the oracle's vit_forward_features."""
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
        t = t + F.linear(o, g(p + "attn.proj.weight"), g(p + "attn.proj.bias"))
        h = F.layer_norm(t, (C,), g(p + "norm2.weight"), g(p + "norm2.bias"), 1e-6)
        h = _Gelu.apply(F.linear(h, g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias")), fault == "gelu_grad")
        t = t + F.linear(h, g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias"))
    return F.layer_norm(t, (C,), g("norm.weight"), g("norm.bias"), 1e-6)


def _leaves(state, trainable):
    sd = {}
    for k, v in state.items():
        v = v.detach().clone()
        if v.is_floating_point():
            v = v.double()
            if not any(k.endswith(s) for s in ("running_mean", "running_var")) and (trainable is None or trainable(k)):
                v.requires_grad_(True)
        sd[k] = v
    return sd


def vit_step(state, x, upstream, *, patch: int, heads: int, trainable=None, fault=None):
    """One train-mode forward + backward of the backbone in float64.  state: a VisionTransformer state_dict; upstream:
    the gradient of the (B, N, C) features.  Returns dict(features, grads {name: tensor})."""
    sd = _leaves(state, trainable)
    f = vit_forward(sd, x.detach().double(), patch=patch, heads=heads, fault=fault)
    names = [k for k, v in sd.items() if v.requires_grad]
    gr = torch.autograd.grad(f, [sd[k] for k in names], upstream.double().reshape(f.shape), allow_unused=True)
    return dict(features=f.detach(), grads={k: (g if g is not None else torch.zeros_like(sd[k]))
                                            for k, g in zip(names, gr)})


def model_step(vit_state, head_state, cfg, x, upstream, *, patch: int, heads: int, vit_trainable=None,
               head_trainable=None):
    """ProbPoseModel's train-mode step in float64: the backbone above, its (B, N, C) features as the (B, C, gh, gw) map,
    then head_grad_reference.head_forward.  upstream: the five outputs' gradients.  Returns dict(outputs, vit_grads,
    head_grads, dy_mag) (dy_mag as head_grad_reference.head_step: the row sums of |dY| of the conv biases ahead of a
    train-mode BN)."""
    vsd = _leaves(vit_state, vit_trainable)
    hsd = _leaves(head_state, head_trainable)
    B, _, H, W = x.shape
    f = vit_forward(vsd, x.detach().double(), patch=patch, heads=heads)
    feats = f.reshape(B, H // patch, W // patch, -1).permute(0, 3, 1, 2)
    inter = {}
    outs, _ = head_forward(hsd, cfg, feats, None, inter)
    inter = {k: v for k, v in inter.items() if v.requires_grad}
    pairs = [(o, g.double()) for o, g in zip(outs, upstream) if g is not None and o.requires_grad]
    vn = [k for k, v in vsd.items() if v.requires_grad]
    hn = [k for k, v in hsd.items() if v.requires_grad]
    leaves = [vsd[k] for k in vn] + [hsd[k] for k in hn] + list(inter.values())
    gr = torch.autograd.grad([o for o, _ in pairs], leaves, [g for _, g in pairs], allow_unused=True)
    z = lambda g, t: g if g is not None else torch.zeros_like(t)  # noqa: E731
    vg = {k: z(g, vsd[k]) for k, g in zip(vn, gr[:len(vn)])}
    hg = {k: z(g, hsd[k]) for k, g in zip(hn, gr[len(vn):len(vn) + len(hn)])}
    gi = gr[len(vn) + len(hn):]
    dy_mag = {k: (g.abs().sum((0, 2, 3)) if g is not None else torch.zeros(v.shape[1], dtype=torch.float64))
              for (k, v), g in zip(inter.items(), gi)}
    return dict(outputs=[o.detach() for o in outs], vit_grads=vg, head_grads=hg, dy_mag=dy_mag)


def grad_class(name: str) -> str:
    """The comparison class of a backbone parameter's gradient."""
    if name == "pos_embed":
        return "pos_embed"
    if name.startswith("patch_embed"):
        return "patch_embed"
    if "norm" in name:
        return "layernorm"
    if ".attn.qkv." in name:
        return "qkv"
    return "linear"


def n_stages(depth: int) -> int:
    """Kernel stages on the longest backward chain (final LN; per block fc2 dgrad, GELU, fc1 dgrad, LN2, proj dgrad,
    attention, qkv dgrad, LN1; the patch-embed weight gradient)."""
    return 8 * depth + 2
