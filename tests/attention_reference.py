"""Float64 restatements of pp_attention (row-major and head-major qkv) and pp_layernorm, and a per-element comparator
that follows the kernels' precision model.

Attention is timm's softmax(q k^T * hd^-0.5) v per (crop, head), read from the layouts of include/probpose_hip.h:
row-major qkv [B*N][3][heads][hd] or head-major qkv [3][heads][B*N][hd]; the output is [B*N][heads*hd].  The
restatement runs in float64 on qkv's device, a chunk of (crop, head) problems at a time, and also returns
ref_abs = softmax(S) @ |V|, the scale of the second product.

Precision model of the kernels (pp_attention.hip, attention_valu_kernel in pp_ops.hip): Q and K are read exactly,
S is accumulated in f32, P is rounded to bf16 before the second product (its f32 value goes into the row sum), O is
accumulated in f32, and the output is rounded once.  Rounding P costs at most 2^-9 ref_abs and rounding a bf16 output
2^-9 |ref|; the bf16 bound is twice their sum.  The exact-fp32 VALU kernel keeps P in f32 and is held to the same form
with 1e-5.  An e4m3 output (out_scale, stored value = o / out_scale) is held to the bf16 term in the stored domain
(`band`) plus one e4m3 half-step at that magnitude (2^-10 in the subnormal range).  Beyond that bound, an e4m3 output
must equal the rounded float64 result wherever the whole band [y - band, y + band] rounds to one e4m3 value: it may
differ only where the float64 value lies within `band` of a rounding midpoint.  (This replaces the 2 % rule of
gemm_reference.compare for these kernels: rounding P to bf16 moves an output by up to 2^-9 ref_abs, about 2^-6 of an
e4m3 step, and flips about 5 % of unit-normal outputs in an emulation of the kernel; the band rule admits exactly the
flips that error can cause and nothing else.)

Every element of the output region is written by a call; every element outside it (guards) must stay bit-identical,
and an unwritten element (NaN from gemm_reference.nan_like_bits) never passes."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from tests import gemm_reference as gr

FP8 = gr.FP8
FP8_MAX = gr.FP8_MAX
CHUNK_ELEMS = 1 << 25          # float64 score elements per chunk of (crop, head) problems

ATT_BF16 = 2.0 ** -8           # bf16 (and e4m3) outputs: |d| <= ATT_BF16 * (|ref| + ref_abs)
ATT_F32 = 1e-5                 # attention_valu_kernel<float>: the constant of test_ops_gpu.py::test_attention
LN_F32 = 1e-5                  # layernorm, f32 output: |d| <= 1e-5 + 1e-5 |ref| (test_ops_gpu.py::test_layernorm)
LN_TERM = 1e-5                 # layernorm, f32 arithmetic: 1e-5 (|gamma| (|x| + |mean|) rstd + |beta|)


def problems(qkv: torch.Tensor, B: int, N: int, heads: int, hd: int, headmajor: bool = False):
    """q, k, v of every (crop, head) problem as (B * heads, N, hd) tensors in qkv's dtype (problem b * heads + h)."""
    if headmajor:
        t = qkv.reshape(3, heads, B, N, hd).transpose(1, 2)
    else:
        t = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    t = t.reshape(3, B * heads, N, hd)
    return t[0], t[1], t[2]


def expected_attention(qkv: torch.Tensor, B: int, N: int, heads: int, hd: int, headmajor: bool = False):
    """(ref, ref_abs): float64 [B*N, heads*hd] in the output layout; ref_abs = softmax(S) @ |V|."""
    q, k, v = problems(qkv, B, N, heads, hd, headmajor)
    P = B * heads
    ref = torch.empty((P, N, hd), dtype=torch.float64, device=qkv.device)
    ref_abs = torch.empty_like(ref)
    scale = hd ** -0.5
    chunk = max(1, CHUNK_ELEMS // (N * max(N, hd)))
    for p0 in range(0, P, chunk):
        p1 = min(P, p0 + chunk)
        qq, kk, vv = q[p0:p1].double(), k[p0:p1].double(), v[p0:p1].double()
        p = torch.softmax((qq @ kk.transpose(1, 2)) * scale, dim=-1)
        del qq, kk
        ref[p0:p1] = p @ vv
        ref_abs[p0:p1] = p @ vv.abs()
        del p, vv

    def out_layout(t):
        return t.reshape(B, heads, N, hd).transpose(1, 2).reshape(B * N, heads * hd)
    return out_layout(ref), out_layout(ref_abs)


def expected_layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """(ref, term): float64 LayerNorm of the rows of x, and the scale of its f32 arithmetic,
    |gamma| (|x| + |mean|) rstd + |beta|.  The f32 difference x - mean is off by up to an ulp of |x| or |mean|, not of
    |x - mean|: where the row's mean is large against its spread and gamma * xhat cancels beta, |gamma * xhat| + |beta|
    alone is too small a scale (found on rows of mean ~4 std, outputs ~1e-5, with a 0.014 scale)."""
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    var = (xd - mean).square().mean(dim=1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    g = gamma.double()
    ref = (xd - mean) * rstd * g + beta.double()
    term = (xd.abs() + mean.abs()) * rstd * g.abs() + beta.double().abs()
    del xd
    return ref, term


# ---------------------------------------------------------------------------------------------------------------
# per-element bounds, in the stored domain (an e4m3 output stores value / out_scale)
# ---------------------------------------------------------------------------------------------------------------
def _e4m3_target(ref, err, inv_scale: float):
    """(stored-domain reference, bound, band): `err` bounds the error of the f32 value before the e4m3 rounding (value
    domain); band is that bound in the stored domain, and the rounding adds one half-step at the magnitude the
    kernel's value can reach (2^-10 below 2^-6)."""
    y = (ref * inv_scale).clamp(-FP8_MAX, FP8_MAX)
    band = err * inv_scale
    top = (y.abs() + band).clamp(min=2.0 ** -6)
    half_step = torch.exp2(torch.floor(torch.log2(top)) - 4)
    return y, band + half_step, band


def attention_target(ref, ref_abs, out_dtype, inv_scale: float | None = None):
    """(stored-domain reference, per-element bound, e4m3 band or None) of an attention output in out_dtype."""
    if out_dtype == torch.float32:
        return ref, ATT_F32 * (ref.abs() + ref_abs), None
    err = ATT_BF16 * (ref.abs() + ref_abs)
    if out_dtype == FP8:
        return _e4m3_target(ref, err, inv_scale)
    return ref, err, None


def layernorm_target(ref, term, out_dtype, inv_scale: float | None = None):
    """(stored-domain reference, per-element bound, e4m3 band or None) of a LayerNorm output in out_dtype."""
    if out_dtype == torch.float32:
        return ref, LN_F32 + LN_F32 * ref.abs(), None
    if out_dtype == FP8:
        return _e4m3_target(ref, LN_TERM * term, inv_scale)
    return ref, 2.0 ** -8 * ref.abs() + LN_TERM * term, None


@dataclass
class Verdict(gr.Verdict):
    worst: float = 0.0    # max |d| / bound over the written elements (inf: a NaN, or a miss where the bound is 0)

    def __str__(self):
        return f"max d/bound {self.worst:.3f}  " + super().__str__()


def _to_e4m3(t):
    return t.clamp(-FP8_MAX, FP8_MAX).float().to(FP8).double()


def compare(got: torch.Tensor, before: torch.Tensor, lo: int, y: torch.Tensor, bound: torch.Tensor,
            band: torch.Tensor | None = None) -> Verdict:
    """got / before: 1-D buffers (same dtype) after / before the call; the call writes got[lo : lo + y.numel()],
    whose stored-domain reference, bound and e4m3 band come from attention_target / layernorm_target.  Everything
    else must be bit-identical."""
    n = y.numel()
    bits = gr._BITS[got.dtype]
    gb, bb = got.view(bits), before.view(bits)
    changed = int((gb[:lo] != bb[:lo]).sum()) + int((gb[lo + n:] != bb[lo + n:]).sum())
    o = got[lo:lo + n].double()
    y, bound = y.reshape(-1), bound.reshape(-1)
    d = (o - y).abs()
    ok = d <= bound                                   # a NaN never passes
    bad = int((~ok).sum())
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max()) if n else 0.0
    note = ""
    if got.dtype == FP8 and n:
        band = band.reshape(-1)
        off = o != _to_e4m3(y)
        firm = _to_e4m3(y - band) == _to_e4m3(y + band)     # the whole band rounds to one e4m3 value
        flips = int((off & firm).sum())
        bad += flips
        note = f"({float(off.double().mean()):.2%} of the e4m3 outputs differ from the rounded float64 result"
        note += f", {flips} where the band does not allow it)" if flips else ", all inside the band)"
    rms = float(y.square().mean().sqrt()) if n else 0.0
    dm = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    dmax = float(dm.max()) if n else 0.0
    rel = dmax / rms if rms > 0 else dmax
    return Verdict(ok=bad == 0 and changed == 0, rel=rel, rms=rms, bad=bad, changed=changed, note=note, worst=worst)
