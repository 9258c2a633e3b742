"""Training the ViT backbone on the HIP path (``ScratchViTBackbone(differentiable=True)`` in ``.train()`` mode).

The forward runs the kernels of ``VitPlan._run_chain`` (pp_patchify, pp_gemm, pp_layernorm, pp_attention on the
row-layout qkv) with three changes that the backward needs: every residual write goes to a new f32 buffer (the
residual input stays intact), fc1 stores its f32 pre-activation and GELU runs as its own exact-erf kernel, and every
activation the backward reads is kept in a per-call allocation (never in the plan's workspace, so two forwards
before two backwards give correct gradients).  One once-differentiable ``torch.autograd.Function`` per call; its
backward launches, block by block in reverse, only what the trainable parameters need and does no host sync.  The
weights (and their transposed copies for the data gradients) are packed from the parameters on the device at every
call: no host copy, no ``VitPlan`` rebuild.  The backward packs the transposed weights from the parameters as they
are then; the parameters are saved with ``save_for_backward``, so an in-place update between the forward and the
backward (an optimizer step before a delayed backward) raises instead of mixing weights.  The saved activations are
released as soon as the backward has run.
"""
from __future__ import annotations

from typing import List

import torch
from torch import nn

from . import _lib, engine, ops
from .head_train import _wgrad
from .ops import EPI_OUT_F32

PER_BLOCK = 12      # parameters per block in vit_parameters' order


def vit_parameters(vit) -> List[nn.Parameter]:
    """The backbone's parameters in the order the autograd node takes them."""
    pe = vit.patch_embed.proj
    ps = [pe.weight, pe.bias, vit.pos_embed]
    for b in vit.blocks:
        ps += [b.norm1.weight, b.norm1.bias, b.attn.qkv.weight, b.attn.qkv.bias, b.attn.proj.weight,
               b.attn.proj.bias, b.norm2.weight, b.norm2.bias, b.mlp.fc1.weight, b.mlp.fc1.bias, b.mlp.fc2.weight,
               b.mlp.fc2.bias]
    return ps + [vit.norm.weight, vit.norm.bias]


def check_trainable(vit, x) -> None:
    """Raise NotImplementedError naming the piece the training path does not cover."""
    if vit.compute_dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"ScratchViTBackbone training: compute dtype {vit.compute_dtype} (float32 and "
                                  "bfloat16 are supported)")
    hd = vit.embed_dim // vit.num_heads
    if hd not in (32, 64):
        raise NotImplementedError(f"ScratchViTBackbone training: head_dim {hd} (32 and 64 are supported)")
    if x.requires_grad:
        raise NotImplementedError("ScratchViTBackbone training: an input image that requires grad (there is no "
                                  "patchify backward)")
    if engine.DUAL_CHAIN:
        raise NotImplementedError("ScratchViTBackbone training: engine.DUAL_CHAIN (two half-batch kernel chains)")


def _w(p, dt):
    return p.detach().to(dt).contiguous()


def _wt(p, dt):
    """W^T [in, out]: the pp_gemm weight of the data gradient dX = dY W."""
    return p.detach().t().to(dt).contiguous()


def _f(p):
    return p.detach().float().contiguous()


class _VitTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vit, x, nchw, *params):
        dt = vit.compute_dtype
        dev = x.device
        B, _, H, W = x.shape
        pe = vit.patch_embed
        if (H, W) != tuple(pe.img_size):
            raise AssertionError(f"Input size ({H}, {W}) doesn't match model {tuple(pe.img_size)}")
        p, C, N, heads = int(pe.patch_size[0]), vit.embed_dim, pe.num_patches, vit.num_heads
        hd, M, K0 = C // heads, B * N, 3 * p * p
        f32 = torch.float32
        x = x.detach().contiguous().float()
        a0 = torch.empty((M, K0), dtype=dt, device=dev)
        ops.patchify(x, a0, p)
        r = torch.empty((M, C), dtype=f32, device=dev)
        ops.gemm(a0, _w(pe.proj.weight.reshape(C, K0), dt), r, M=M, N=C, Kd=K0, lda=K0, ldw=K0, ldc=C,
                 bias=_f(pe.proj.bias), rowbias=_f(vit.pos_embed.reshape(N, C)), rowbias_period=N,
                 epilogue=EPI_OUT_F32)
        res, blocks = [r], []
        for blk in vit.blocks:
            hidden = blk.mlp.fc1.out_features
            ln1 = torch.empty((M, C), dtype=dt, device=dev)
            ops.layernorm(r, _f(blk.norm1.weight), _f(blk.norm1.bias), blk.norm1.eps, ln1)
            qkv = torch.empty((M, 3 * C), dtype=dt, device=dev)
            ops.linear(ln1, _w(blk.attn.qkv.weight, dt), _f(blk.attn.qkv.bias), out=qkv)
            ao = torch.empty((M, C), dtype=dt, device=dev)
            ops.attention(qkv, ao, B, N, heads, hd)
            r1 = torch.empty((M, C), dtype=f32, device=dev)
            ops.linear(ao, _w(blk.attn.proj.weight, dt), _f(blk.attn.proj.bias), out=r1, residual=r)
            ln2 = torch.empty((M, C), dtype=dt, device=dev)
            ops.layernorm(r1, _f(blk.norm2.weight), _f(blk.norm2.bias), blk.norm2.eps, ln2)
            pre = torch.empty((M, hidden), dtype=f32, device=dev)
            ops.linear(ln2, _w(blk.mlp.fc1.weight, dt), _f(blk.mlp.fc1.bias), out=pre, out_dtype=f32)
            hid = torch.empty((M, hidden), dtype=dt, device=dev)
            ops.gelu_forward(pre, hid)
            r2 = torch.empty((M, C), dtype=f32, device=dev)
            ops.linear(hid, _w(blk.mlp.fc2.weight, dt), _f(blk.mlp.fc2.bias), out=r2, residual=r1)
            blocks.append(dict(ln1=ln1, qkv=qkv, ao=ao, ln2=ln2, pre=pre, hid=hid))
            res += [r1, r2]
            r = r2
        feats = torch.empty((M, C), dtype=dt, device=dev)
        ops.layernorm(r, _f(vit.norm.weight), _f(vit.norm.bias), vit.norm.eps, feats)
        ctx.vit = vit
        ctx.save_for_backward(*params)
        ctx.saved = dict(B=B, N=N, a0=a0, res=res, blocks=blocks, nchw=nchw)
        if nchw:
            gh, gw = pe.dynamic_feat_size((H, W))
            out = torch.empty((B, C, gh, gw), dtype=f32, device=dev)
            ops.tokens_to_nchw(feats, out, B, N, C)
            return out
        return feats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        vit, S = ctx.vit, ctx.saved
        if S is None:
            raise RuntimeError("ScratchViTBackbone training: backward through the same forward twice (its saved "
                               "activations are released after the first backward)")
        ctx.saved = None         # once differentiable: the activations go with this call
        need = ctx.needs_input_grad[3:]
        params = list(ctx.saved_tensors)     # raises if a parameter was modified in place since the forward
        grads = [None] * len(params)
        if g is None or not any(need):
            return (None, None, None, *grads)
        dt = vit.compute_dtype
        dev = g.device
        B, N, C, heads = S["B"], S["N"], vit.embed_dim, vit.num_heads
        hd, M = C // heads, B * N
        f32 = torch.float32
        res = S["res"]
        D = len(vit.blocks)

        def wants(i):
            return need[i]

        def below(i):        # some parameter with index < i needs its gradient
            return any(need[:i])

        def put(i, t):
            if wants(i):
                grads[i] = t.reshape(params[i].shape).to(params[i].dtype)

        def linear_wgrad(i, dY, A, n_out, k_in):
            if wants(i) or wants(i + 1):
                dW = torch.empty((n_out, k_in), dtype=f32, device=dev)
                dB = torch.empty((n_out,), dtype=f32, device=dev)
                _wgrad(dY, A, dW, M=M, N=n_out, Kd=k_in, ldd=n_out, lda=k_in, dB=dB)
                put(i, dW)
                put(i + 1, dB)

        def ln_backward(i, ln, x, dy, accumulate):
            dgb = torch.empty((2, C), dtype=f32, device=dev) if (wants(i) or wants(i + 1)) else None
            ops.layernorm_backward(x, _f(ln.weight), ln.eps, dy, dR, dRc, accumulate,
                                   dgamma=None if dgb is None else dgb[0], dbeta=None if dgb is None else dgb[1])
            if dgb is not None:
                put(i, dgb[0])
                put(i + 1, dgb[1])

        # ---- final LayerNorm: dR (f32) and dR_c (compute dtype) = the residual stream's gradient
        if S["nchw"]:
            gy = torch.empty((M, C), dtype=f32, device=dev)
            ops.nchw_to_tokens(g.contiguous().float(), gy, B, C, N)
        else:
            gy = g.contiguous().float()
        dR = torch.empty((M, C), dtype=f32, device=dev)
        dRc = torch.empty((M, C), dtype=dt, device=dev)
        ln_backward(3 + PER_BLOCK * D, vit.norm, res[-1], gy, False)
        reached_embed = True
        for bi in range(D - 1, -1, -1):
            base = 3 + PER_BLOCK * bi
            blk, s = vit.blocks[bi], S["blocks"][bi]
            hidden = blk.mlp.fc1.out_features
            if not below(base + PER_BLOCK):
                reached_embed = False
                break
            # fc2 (+ residual): its output gradient is dR
            linear_wgrad(base + 10, dRc, s["hid"], C, hidden)
            if not below(base + 10):
                reached_embed = False
                break
            dH = torch.empty((M, hidden), dtype=f32, device=dev)
            ops.gemm(dRc, _wt(blk.mlp.fc2.weight, dt), dH, M=M, N=hidden, Kd=C, lda=C, ldw=C, ldc=hidden,
                     epilogue=EPI_OUT_F32)
            dPre = torch.empty((M, hidden), dtype=dt, device=dev)
            ops.gelu_backward(s["pre"], dH, dPre)
            del dH
            # fc1
            linear_wgrad(base + 8, dPre, s["ln2"], hidden, C)
            if not below(base + 8):
                reached_embed = False
                break
            dL = torch.empty((M, C), dtype=f32, device=dev)
            ops.gemm(dPre, _wt(blk.mlp.fc1.weight, dt), dL, M=M, N=C, Kd=hidden, lda=hidden, ldw=hidden, ldc=C,
                     epilogue=EPI_OUT_F32)
            del dPre
            ln_backward(base + 6, blk.norm2, res[2 * bi + 1], dL, True)
            if not below(base + 6):
                reached_embed = False
                break
            # proj (+ residual)
            linear_wgrad(base + 4, dRc, s["ao"], C, C)
            if not below(base + 4):
                reached_embed = False
                break
            dO = torch.empty((M, C), dtype=dt, device=dev)
            ops.gemm(dRc, _wt(blk.attn.proj.weight, dt), dO, M=M, N=C, Kd=C, lda=C, ldw=C, ldc=C)
            dqkv = torch.empty((M, 3 * C), dtype=dt, device=dev)
            ops.attention_backward(s["qkv"], s["ao"], dO, dqkv, B, N, heads, hd)
            del dO
            # qkv
            linear_wgrad(base + 2, dqkv, s["ln1"], 3 * C, C)
            if not below(base + 2):
                reached_embed = False
                break
            ops.gemm(dqkv, _wt(blk.attn.qkv.weight, dt), dL, M=M, N=C, Kd=3 * C, lda=3 * C, ldw=3 * C, ldc=C,
                     epilogue=EPI_OUT_F32)
            del dqkv
            ln_backward(base, blk.norm1, res[2 * bi], dL, True)
        if reached_embed:
            K0 = S["a0"].shape[1]
            if wants(0) or wants(1):
                dW = torch.empty((C, K0), dtype=f32, device=dev)
                dB = torch.empty((C,), dtype=f32, device=dev)
                _wgrad(dRc, S["a0"], dW, M=M, N=C, Kd=K0, ldd=C, lda=K0, dB=dB)
                put(0, dW)          # k = c p^2 + py p + px, as pp_patchify packs it: Conv2d's [C, 3, p, p]
                put(1, dB)
            if wants(2):
                pos = torch.empty((N, C), dtype=f32, device=dev)
                ops.rows_period_sum(dR, B, N, C, pos)
                put(2, pos)
        return (None, None, None, *grads)


def train_forward(vit, x: torch.Tensor, nchw: bool = False) -> torch.Tensor:
    """The training forward of ``vit`` (backbone.VisionTransformer) on crops x (B, 3, H, W): tokens [B*N, C] in the
    compute dtype, or (nchw=True) the (B, C, gh, gw) f32 map of ScratchViTBackbone.forward; both carry the gradient."""
    _lib.require_device(x)
    check_trainable(vit, x)
    params = vit_parameters(vit)
    for p in params:
        if p.device != x.device:
            raise ValueError(f"ScratchViTBackbone parameters are on {p.device}, the input on {x.device}: move the "
                             "backbone first")
    with torch.cuda.device(x.device):
        return _VitTrainFn.apply(vit, x, nchw, *params)
