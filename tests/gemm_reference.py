"""Float64 restatement of pp_gemm and a comparator for what a launch left in its output buffer.

The restatement is written from the contract in include/probpose_hip.h (the epilogue flags, the gather
A(m, k) = Abase[rowoff[(k / seg_len) * M + m] + k % seg_len] with rowoff < 0 reading as 0, batch and split-K
strides, the head-major and NCHW heatmap layouts), not from the kernels.  A call is described by the keyword
arguments of ``ops.gemm`` (A, W, out and the named fields); the flags ``ops.gemm`` derives from them (a bias
tensor sets PP_EPI_BIAS, ...) are derived here the same way.  Operands are read exactly as the kernel reads them
(bf16 / e4m3 / f32 storage converted to float64) and the contraction runs on the operands' device in float64,
a chunk of rows at a time, so that a gathered K = 9 C operand is never materialised whole.

``expected_output`` returns the whole expected buffer from C onwards: written elements hold the float64 result in
the storage domain (before rounding to the output dtype; e4m3 outputs already multiplied by out_scale and
saturated at +-448), every other element keeps its value from before the call.  ``compare`` bounds the error of
the written elements by the call's own scale and requires every other element to be bit-identical."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

# include/probpose_hip.h, epilogue flags of pp_gemm
EPI_BIAS, EPI_GELU, EPI_RELU, EPI_RESIDUAL, EPI_OUT_F32, EPI_ROWBIAS = 1, 2, 4, 8, 16, 32
EPI_HEATMAP, EPI_OUT_FP8, EPI_NOCLAMP, EPI_FUSE_FINAL, EPI_HEADMAJOR = 64, 512, 1024, 2048, 4096

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
CHUNK_ELEMS = 1 << 25          # float64 elements per row chunk of the gathered operand / the output


def flags(kw) -> int:
    """The epilogue bits a call of ops.gemm with these keyword arguments launches with."""
    epi = kw.get("epilogue", 0)
    if kw.get("bias") is not None:
        epi |= EPI_BIAS
    if kw.get("residual") is not None:
        epi |= EPI_RESIDUAL
    if kw.get("rowbias") is not None:
        epi |= EPI_ROWBIAS
    if kw.get("heatmap") is not None:
        epi |= EPI_HEATMAP
        if len(kw["heatmap"]) > 3 and not kw["heatmap"][3]:
            epi |= EPI_NOCLAMP
    if kw.get("headmajor") is not None:
        epi |= EPI_HEADMAJOR
    if kw.get("fuse_final") is not None:
        epi |= EPI_FUSE_FINAL
    if kw["W"].dtype == FP8:
        if kw["out"].dtype == FP8:
            epi |= EPI_OUT_FP8
        elif kw["out"].dtype == torch.float32:
            epi |= EPI_OUT_F32
    return epi


def flat(t: torch.Tensor) -> torch.Tensor:
    """1-D view of t's storage from t's first element to the end of the allocation (what a pointer reaches)."""
    n = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
    return torch.as_strided(t, (n,), (1,), t.storage_offset())


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * (0.5 ** 0.5)))


def expected_output(kw, before: torch.Tensor):
    """kw: ops.gemm keyword arguments (A, W, out, M, N, Kd, ...) with the tensors as the call saw them (a residual
    tensor holds its values from before the call).  before: 1-D, the output buffer from C onwards as it was before
    the call (guard elements after it included).  Returns (ref float64, written bool), both shaped like before."""
    epi = flags(kw)
    if epi & EPI_FUSE_FINAL:
        raise NotImplementedError("PP_EPI_FUSE_FINAL launches are not restated (fixed tile, never tuned)")
    dev = before.device
    M, N, Kd, lda, ldw, ldc = (kw[k] for k in ("M", "N", "Kd", "lda", "ldw", "ldc"))
    batch = max(1, kw.get("batch", 1))
    S = max(1, kw.get("splitk", 1))
    g = lambda k: kw.get(k, 0)  # noqa: E731
    seg = g("seg_len") or Kd
    fp8 = kw["W"].dtype == FP8
    Af, Wf = flat(kw["A"]), flat(kw["W"])
    ro_f = flat(kw["rowoff"]) if kw.get("rowoff") is not None else None
    rm_f = flat(kw["out_rowmap"]) if kw.get("out_rowmap") is not None else None
    bias_f = flat(kw["bias"]).double() if epi & EPI_BIAS else None
    cs_f = flat(kw["colscale"]).double() if fp8 else None
    rb_f = flat(kw["rowbias"]).double() if epi & EPI_ROWBIAS else None
    res_f = flat(kw["residual"]) if epi & EPI_RESIDUAL else None
    P = kw.get("rowbias_period", 0) or 1
    hm = kw.get("heatmap") or (None, None)
    hm_K, hm_HW = (kw["headmajor"] if epi & EPI_HEADMAJOR else hm[:2])
    T = kw["heatmap"][2] if epi & EPI_HEATMAP else None
    q = 1.0 / float(kw["out_scale"]) if epi & EPI_OUT_FP8 else None

    ref = before.double()
    written = torch.zeros(before.shape, dtype=torch.bool, device=dev)
    n = torch.arange(N, device=dev)
    chunk = max(16, CHUNK_ELEMS // max(Kd, N))
    for z in range(batch):
        for zs in range(S):
            abase = z * g("strideA") + zs * g("strideA_k")
            wz = torch.as_strided(Wf, (N, Kd), (ldw, 1), z * g("strideW") + zs * g("strideW_k")).double()
            for r0 in range(0, M, chunk):
                r1 = min(M, r0 + chunk)
                rows = torch.arange(r0, r1, device=dev)
                if ro_f is None:
                    a = torch.as_strided(Af, (r1 - r0, Kd), (lda, 1), abase + r0 * lda).double()
                else:
                    ro = torch.as_strided(ro_f, (Kd // seg, r1 - r0), (M, 1),
                                          z * g("strideRowoff") + zs * g("strideRowoff_k") + r0).long()
                    ok = (ro >= 0)[:, :, None]
                    idx = torch.where(ok, abase + ro[:, :, None] + torch.arange(seg, device=dev), 0)
                    a = torch.where(ok, Af[idx].double(), 0.0).permute(1, 0, 2).reshape(r1 - r0, Kd)
                    del idx
                v = a @ wz.t()
                del a
                if fp8:
                    v *= cs_f[z * g("strideBias") + n]
                if bias_f is not None:
                    v += bias_f[z * g("strideBias") + n]
                if rb_f is not None:
                    v += rb_f[((rows % P) * ldc)[:, None] + n]
                out_row = rows if rm_f is None else rm_f[z * g("strideRowmap") + rows].long()
                if epi & EPI_GELU:
                    v = _gelu(v)
                if epi & EPI_RELU:
                    v = v.clamp_min(0.0)
                if res_f is not None:
                    v += res_f[z * g("strideC") + (out_row * ldc)[:, None] + n].double()
                if epi & EPI_HEATMAP:
                    v = v / T
                    if not epi & EPI_NOCLAMP:
                        v = v.clamp(0.0, 1.0)
                    b, hw = out_row // hm_HW, out_row % hm_HW
                    dest = z * g("strideC") + ((b * hm_K)[:, None] + n) * hm_HW + hw[:, None]
                elif epi & EPI_HEADMAJOR:
                    Cc = hm_K * hm_HW
                    which, rem = n // Cc, n % Cc
                    dest = ((which * hm_K + rem // hm_HW) * M)[None, :] * hm_HW + (rows * hm_HW)[:, None] + (rem % hm_HW)
                else:
                    dest = z * g("strideC") + zs * g("strideC_k") + (out_row * ldc)[:, None] + n
                if q is not None:
                    v = (v * q).clamp(-FP8_MAX, FP8_MAX)
                dest = dest.reshape(-1)
                assert int(dest.min()) >= 0 and int(dest.max()) < before.numel(), "call writes outside the buffer"
                ref[dest] = v.reshape(-1)
                written[dest] = True
    return ref, written


# ---------------------------------------------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------------------------------------------
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, FP8: torch.uint8, torch.float64: torch.int64}


def nan_like_bits(n: int, dtype, device) -> torch.Tensor:
    """n elements of `dtype`, every one a quiet NaN (an element nobody wrote)."""
    pat = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0, FP8: 0x7F}[dtype]
    return torch.full((n,), pat, dtype=_BITS[dtype], device=device).view(dtype)


def tolerance(compute_dtype, out_dtype, rms: float):
    """(rtol, atol) for |out - ref| <= rtol |ref| + atol: the bound of tests/test_ops_gpu.py::_tol, with the absolute
    part scaled down to the call's own rms where that is smaller (never looser than _tol)."""
    if compute_dtype == torch.float32:
        return 2e-5, 2e-5 * min(1.0, rms)
    if out_dtype == torch.float32:
        return 1e-4, min(1e-3, 1e-4 * rms)
    if out_dtype == FP8:
        # stored domain (value * out_scale): the f32 accumulation error of an f32 output (1e-4 rms; near zero it is
        # larger than the e4m3 subnormal step 2^-9 once out_scale is ~80), then one e4m3 step
        return 2.0 ** -3 + 1e-4, 2.0 ** -9 + 1e-4 * rms
    return 2.0 ** -7, min(2e-2, 2.0 ** -7 * rms)


@dataclass
class Verdict:
    ok: bool
    rel: float            # max |out - ref| / rms(ref) over the written elements
    rms: float
    bad: int              # written elements outside the bound
    changed: int          # elements outside what the call writes that are not bit-identical to before
    note: str = ""

    def __str__(self):
        s = f"max|d|/rms {self.rel:.3e} (rms {self.rms:.3g})"
        if not self.ok:
            s += f"  FAIL: {self.bad} outside the bound, {self.changed} unwritten elements changed {self.note}"
        return s


def compare(got: torch.Tensor, before: torch.Tensor, ref: torch.Tensor, written: torch.Tensor, compute_dtype) -> Verdict:
    """got / before: 1-D output buffers (same dtype) after / before the call; ref, written from expected_output."""
    bits = _BITS[got.dtype]
    same = got.view(bits) == before.view(bits)
    changed = int((~same & ~written).sum())
    r = ref[written]
    o = got[written].double()
    rms = float(r.square().mean().sqrt()) if r.numel() else 0.0
    rtol, atol = tolerance(compute_dtype, got.dtype, rms)
    d = (o - r).abs()
    bad_mask = ~(d <= rtol * r.abs() + atol)          # a NaN never passes
    bad = int(bad_mask.sum())
    note = ""
    if got.dtype == FP8 and r.numel():
        # e4m3 outputs: beyond the one-step bound, few values may round differently from the float64 result
        off = float((o != r.float().to(FP8).double()).double().mean())
        if off > 0.02:
            bad = max(bad, 1)
            note = f"({off:.1%} of the e4m3 outputs differ from the rounded float64 result)"
    dmax = float(torch.where(torch.isnan(d), torch.full_like(d, math.inf), d).max()) if d.numel() else 0.0
    rel = dmax / rms if rms > 0 else dmax
    return Verdict(ok=bad == 0 and changed == 0, rel=rel, rms=rms, bad=bad, changed=changed, note=note)
