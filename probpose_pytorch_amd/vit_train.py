"""Training the ViT backbone on the HIP path (``ScratchViTBackbone(differentiable=True)`` in ``.train()`` mode).

The forward runs the kernels of ``VitPlan._run_blocks`` (pp_patchify, pp_gemm, pp_layernorm, pp_attention on the
row-layout qkv; the patch-embed step and the weight packing are engine.py's own) with three changes that the backward needs: every residual write goes to a new f32 buffer (the
residual input stays intact), fc1 stores its f32 pre-activation and GELU runs as its own exact-erf kernel, and every
activation the backward reads is kept in a per-call allocation (never in the plan's workspace, so two forwards
before two backwards give correct gradients).  One once-differentiable ``torch.autograd.Function`` per call; its
backward launches, block by block in reverse, only what the trainable parameters need and does no host sync.  The
weights (and their transposed copies for the data gradients) are packed from the parameters on the device at every
call: no host copy, no ``VitPlan`` rebuild.  The backward packs the transposed weights from the parameters as they
are then; the parameters are saved with ``save_for_backward``, so an in-place update between the forward and the
backward (an optimizer step before a delayed backward) raises instead of mixing weights.  The saved activations are
released as soon as the backward has run.

Stochastic depth (``drop_path_rate > 0``, timm's DropPath with scale_by_keep): block i drops each crop's attention
branch and MLP branch independently with probability ``drop_path_rates[i]``; r_out[b] = r_in[b] + keep[b] / (1 - p_i)
branch(r_in)[b].  The keep mask is drawn on the host (``draw_keep``), so the host knows every branch's kept count and
nothing is read back.  A branch with p_i > 0 gathers the kept crops' residual rows into a compact buffer, runs the
same kernels on it at batch B' and ends in pp_droppath_add; its backward gathers the scaled output gradient, runs on
the compact rows and ends in pp_crop_rows_scatter_add (csrc/pp_droppath.hip).  A branch with nothing kept launches
nothing; a branch with p_i == 0 runs exactly the path above.
"""
from __future__ import annotations

from functools import partial
from typing import List, Optional

import numpy as np
import torch
from torch import nn

from . import _lib, engine, ops
from .engine import _dev
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


def draw_keep(rates, B: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The keep mask of one training forward: bool [depth, 2, B] on the CPU, [:, 0] the attention branches, [:, 1] the
    MLP branches, True with probability 1 - rates[i].  Drawn from torch's default CPU generator (``torch.manual_seed``
    makes a run reproducible) or from ``generator``; a block at rate 0 is all True and draws nothing."""
    keep = torch.ones((len(rates), 2, B), dtype=torch.bool)
    for i, p in enumerate(rates):
        if p > 0:
            keep[i] = torch.rand((2, B), generator=generator) >= p
    return keep


def _check_keep(vit, keep, B):
    rates = vit.drop_path_rates
    if not (isinstance(keep, torch.Tensor) and keep.dtype == torch.bool and keep.device.type == "cpu"
            and tuple(keep.shape) == (len(rates), 2, B)):
        raise ValueError(f"keep must be a bool CPU tensor of shape ({len(rates)}, 2, {B})")
    for i, p in enumerate(rates):
        if p == 0 and not bool(keep[i].all()):
            raise ValueError(f"keep drops a crop in block {i}, whose drop-path rate is 0")


def _drop_plan(vit, keep, B, device):
    """Per block (attention, MLP): None for a branch at rate 0, else dict(k = kept crops, scale = 1 / (1 - p), idx
    [k] / slot [B] int32 on the device).  Every table goes up in one asynchronous copy from one pinned buffer."""
    k_np = keep.numpy()
    slots = np.where(k_np, np.cumsum(k_np, axis=-1, dtype=np.int32) - 1, -1).astype(np.int32)
    plan, parts, off = [], [], 0
    for i, p in enumerate(vit.drop_path_rates):
        if p == 0:
            plan.append((None, None))
            continue
        pair = []
        for j in range(2):
            idx = np.flatnonzero(k_np[i, j]).astype(np.int32)
            pair.append(dict(k=int(idx.size), scale=1.0 / (1.0 - p), off=off))
            if idx.size:
                parts += [idx, slots[i, j]]
                off += idx.size + B
        plan.append(tuple(pair))
    if parts:
        host = torch.empty(off, dtype=torch.int32, pin_memory=True)
        host.numpy()[:] = np.concatenate(parts)
        table = host.to(device, non_blocking=True)
        for pair in plan:
            for d in pair:
                if d is not None and d["k"]:
                    d["idx"] = table[d["off"]:d["off"] + d["k"]]
                    d["slot"] = table[d["off"] + d["k"]:d["off"] + d["k"] + B]
    return plan


def _wt(p, dt):
    """W^T [in, out]: the pp_gemm weight of the data gradient dX = dY W."""
    return p.detach().t().to(dt).contiguous()


def _branch(r, dp, B, N, dt, norm, body, last):
    """One residual branch of a block, r [B*N, C] f32 -> (r + branch(r) in a new buffer, the activations its backward
    reads): on all rows (dp None: rate 0), on the kept crops' rows, or (nothing kept) not at all.  norm = (gamma, beta,
    eps); body(LN output, crops) -> (the last linear's input, activations to save); last = (weight, bias)."""
    if dp is not None and not dp["k"]:
        return r, {}
    M, C = r.shape
    dev, f32 = r.device, torch.float32
    Bb = B if dp is None else dp["k"]
    Mb = Bb * N
    xin = r
    if dp is not None:
        xin = dp["x"] = torch.empty((Mb, C), dtype=f32, device=dev)
        ops.crop_rows_gather(r, dp["idx"], B, N, C, xin)
    ln = torch.empty((Mb, C), dtype=dt, device=dev)
    ops.layernorm(xin, *norm, ln)
    y, saved = body(ln, Bb)
    out = torch.empty((M, C), dtype=f32, device=dev)
    if dp is None:
        ops.linear(y, *last, out=out, residual=r)
    else:
        br = torch.empty((Mb, C), dtype=f32, device=dev)
        ops.linear(y, *last, out=br, out_dtype=f32)
        ops.droppath_add(r, br, dp["slot"], B, Bb, N, C, dp["scale"], out)
    return out, saved


class _VitTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vit, x, nchw, keep, *params):
        dt = vit.compute_dtype
        dev = x.device
        B, _, H, W = x.shape
        pe = vit.patch_embed
        if (H, W) != tuple(pe.img_size):
            raise AssertionError(f"Input size ({H}, {W}) doesn't match model {tuple(pe.img_size)}")
        p, C, N, heads = int(pe.patch_size[0]), vit.embed_dim, pe.num_patches, vit.num_heads
        hd, M = C // heads, B * N
        f32 = torch.float32
        x = x.detach().contiguous().float()
        a0 = torch.empty((M, 3 * p * p), dtype=dt, device=dev)
        r = torch.empty((M, C), dtype=f32, device=dev)
        engine.patch_embed(x, a0, r, p, *engine.pack_embed(vit, dt))

        def attention(w, ln1, Bb):         # w: the block's packed weights
            qkv = torch.empty((Bb * N, 3 * C), dtype=dt, device=dev)
            ops.linear(ln1, w["qkv_w"], w["qkv_b"], out=qkv)
            ao = torch.empty((Bb * N, C), dtype=dt, device=dev)
            ops.attention(qkv, ao, Bb, N, heads, hd)
            return ao, dict(ln1=ln1, qkv=qkv, ao=ao)

        def mlp(w, ln2, Bb):
            hidden = w["fc1_w"].shape[0]
            pre = torch.empty((Bb * N, hidden), dtype=f32, device=dev)
            ops.linear(ln2, w["fc1_w"], w["fc1_b"], out=pre, out_dtype=f32)
            hid = torch.empty((Bb * N, hidden), dtype=dt, device=dev)
            ops.gelu_forward(pre, hid)
            return hid, dict(ln2=ln2, pre=pre, hid=hid)

        drop = [(None, None)] * len(vit.blocks) if keep is None else _drop_plan(vit, keep, B, dev)
        res, blocks = [r], []
        for blk, (dpa, dpm) in zip(vit.blocks, drop):
            w = engine.pack_block(blk, dt)
            r1, sa = _branch(r, dpa, B, N, dt, (w["n1w"], w["n1b"], w["eps1"]), partial(attention, w),
                             (w["proj_w"], w["proj_b"]))
            r2, sm = _branch(r1, dpm, B, N, dt, (w["n2w"], w["n2b"], w["eps2"]), partial(mlp, w),
                             (w["fc2_w"], w["fc2_b"]))
            blocks.append(dict(sa, **sm, dpa=dpa, dpm=dpm))
            res += [r1, r2]
            r = r2
        feats = torch.empty((M, C), dtype=dt, device=dev)
        ops.layernorm(r, _dev(vit.norm.weight, None, f32), _dev(vit.norm.bias, None, f32), vit.norm.eps, feats)
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
        need = ctx.needs_input_grad[4:]
        params = list(ctx.saved_tensors)     # raises if a parameter was modified in place since the forward
        grads = [None] * len(params)
        if g is None or not any(need):
            return (None, None, None, None, *grads)
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

        def put_zeros(lo, hi):          # a branch that kept no crop: its parameters' gradients are zero
            for i in range(lo, hi):
                if wants(i):
                    grads[i] = torch.zeros_like(params[i])

        def linear_wgrad(i, dY, A, n_out, k_in, rows):
            if wants(i) or wants(i + 1):
                dW = torch.empty((n_out, k_in), dtype=f32, device=dev)
                dB = torch.empty((n_out,), dtype=f32, device=dev)
                _wgrad(dY, A, dW, M=rows, N=n_out, Kd=k_in, ldd=n_out, lda=k_in, dB=dB)
                put(i, dW)
                put(i + 1, dB)

        def ln_backward(i, ln, x, dy, accumulate, dp=None):
            """The LayerNorm's input gradient into dR / dRc: added in place, or (a branch on compact rows, dp) written
            to compact scratch and added to its crops' rows by pp_crop_rows_scatter_add."""
            dgb = torch.empty((2, C), dtype=f32, device=dev) if (wants(i) or wants(i + 1)) else None
            if dp is None:
                out, out_c = dR, dRc
            else:
                out, out_c, accumulate = torch.empty_like(x), torch.empty(x.shape, dtype=dt, device=dev), False
            ops.layernorm_backward(x, _dev(ln.weight, None, f32), ln.eps, dy, out, out_c, accumulate,
                                   dgamma=None if dgb is None else dgb[0], dbeta=None if dgb is None else dgb[1])
            if dp is not None:
                ops.crop_rows_scatter_add(out, dp["idx"], B, N, C, dR, dRc)
            if dgb is not None:
                put(i, dgb[0])
                put(i + 1, dgb[1])

        def branch_backward(lo, blk, s, dp, ln, x, a_last, body):
            """The backward of one residual branch whose six parameters start at index lo (LayerNorm, first linear at
            lo + 2, last linear at lo + 4): x is the branch's input residual, a_last the last linear's input;
            body(lo, blk, s, dY, rows, crops) takes the branch's output gradient to the LayerNorm's output gradient, or
            returns None when nothing below the first linear needs one.  False: nothing below the branch needs a
            gradient."""
            if dp is not None and not dp["k"]:
                put_zeros(lo, lo + 6)
                return below(lo)
            if dp is None:          # the residual gradient itself, or the kept crops' rows of it times 1 / (1 - p)
                Mb, Bb, dY = M, B, dRc
            else:
                Mb, Bb = dp["k"] * N, dp["k"]
                dY = torch.empty((Mb, C), dtype=dt, device=dev)
                ops.crop_rows_gather(dR, dp["idx"], B, N, C, dY, dp["scale"])
            linear_wgrad(lo + 4, dY, a_last, C, a_last.shape[1], Mb)
            if not below(lo + 4):
                return False
            dL = body(lo, blk, s, dY, Mb, Bb)
            if dL is None:
                return False
            ln_backward(lo, ln, x if dp is None else dp["x"], dL, True, dp)
            return below(lo)

        def mlp_backward(lo, blk, s, dY, Mb, Bb):
            hidden = blk.mlp.fc1.out_features
            dH = torch.empty((Mb, hidden), dtype=f32, device=dev)
            ops.gemm(dY, _wt(blk.mlp.fc2.weight, dt), dH, M=Mb, N=hidden, Kd=C, lda=C, ldw=C, ldc=hidden,
                     epilogue=EPI_OUT_F32)
            dPre = torch.empty((Mb, hidden), dtype=dt, device=dev)
            ops.gelu_backward(s["pre"], dH, dPre)
            del dH
            linear_wgrad(lo + 2, dPre, s["ln2"], hidden, C, Mb)
            if not below(lo + 2):
                return None
            dL = torch.empty((Mb, C), dtype=f32, device=dev)
            ops.gemm(dPre, _wt(blk.mlp.fc1.weight, dt), dL, M=Mb, N=C, Kd=hidden, lda=hidden, ldw=hidden, ldc=C,
                     epilogue=EPI_OUT_F32)
            return dL

        def attn_backward(lo, blk, s, dY, Mb, Bb):
            dO = torch.empty((Mb, C), dtype=dt, device=dev)
            ops.gemm(dY, _wt(blk.attn.proj.weight, dt), dO, M=Mb, N=C, Kd=C, lda=C, ldw=C, ldc=C)
            dqkv = torch.empty((Mb, 3 * C), dtype=dt, device=dev)
            ops.attention_backward(s["qkv"], s["ao"], dO, dqkv, Bb, N, heads, hd)
            del dO
            linear_wgrad(lo + 2, dqkv, s["ln1"], 3 * C, C, Mb)
            if not below(lo + 2):
                return None
            dL = torch.empty((Mb, C), dtype=f32, device=dev)
            ops.gemm(dqkv, _wt(blk.attn.qkv.weight, dt), dL, M=Mb, N=C, Kd=3 * C, lda=3 * C, ldw=3 * C, ldc=C,
                     epilogue=EPI_OUT_F32)
            return dL

        # ---- final LayerNorm: dR (f32) and dR_c (compute dtype) = the residual stream's gradient
        if S["nchw"]:
            gy = torch.empty((M, C), dtype=f32, device=dev)
            ops.nchw_to_tokens(g.contiguous().float(), gy, B, C, N)
        else:
            gy = g.contiguous().float()
        dR = torch.empty((M, C), dtype=f32, device=dev)
        dRc = torch.empty((M, C), dtype=dt, device=dev)
        ln_backward(3 + PER_BLOCK * D, vit.norm, res[-1], gy, False)
        reached_embed = below(3 + PER_BLOCK * D)
        for bi in range(D - 1, -1, -1):
            if not reached_embed:
                break
            base = 3 + PER_BLOCK * bi
            blk, s = vit.blocks[bi], S["blocks"][bi]
            reached_embed = (
                branch_backward(base + 6, blk, s, s["dpm"], blk.norm2, res[2 * bi + 1], s.get("hid"), mlp_backward)
                and branch_backward(base, blk, s, s["dpa"], blk.norm1, res[2 * bi], s.get("ao"), attn_backward))
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
        return (None, None, None, None, *grads)


def train_forward(vit, x: torch.Tensor, nchw: bool = False, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The training forward of ``vit`` (backbone.VisionTransformer) on crops x (B, 3, H, W): tokens [B*N, C] in the
    compute dtype, or (nchw=True) the (B, C, gh, gw) f32 map of ScratchViTBackbone.forward; both carry the gradient.
    ``keep``: an explicit drop-path mask (bool [depth, 2, B] on the CPU, as ``draw_keep`` returns) in place of a draw;
    the mask that was used is left in ``vit.last_drop_path_keep`` (None when every rate is 0)."""
    _lib.require_device(x)
    check_trainable(vit, x)
    params = vit_parameters(vit)
    for p in params:
        if p.device != x.device:
            raise ValueError(f"ScratchViTBackbone parameters are on {p.device}, the input on {x.device}: move the "
                             "backbone first")
    if keep is not None:
        _check_keep(vit, keep, x.shape[0])
    if not any(vit.drop_path_rates):
        keep = None
    elif keep is None:
        keep = draw_keep(vit.drop_path_rates, x.shape[0])
    vit.last_drop_path_keep = keep
    with torch.cuda.device(x.device):
        return _VitTrainFn.apply(vit, x, nchw, keep, *params)
