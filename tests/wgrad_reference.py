"""Float64 restatement of pp_wgrad_gemm and a comparator for what a launch left in dW, dB and around them.

Written from the addressing formula in include/probpose_hip.h, not from the kernel: per batch entry b
    dY(m, n) = dY[b strideDY + (dy_rowmap ? dy_rowmap[b strideRowmap + m] : m) ldd + n]
    A(m, k)  = A[b strideA + rowoff[b strideRowoff + (k / seg_len) M + m] + k % seg_len]   (rowoff < 0 reads as 0), or
               A[b strideA + m lda + k] when rowoff is absent
    dW[b strideDW + n lddw + k] = sum_m dY(m, n) A(m, k),    dB[b strideDB + n] = sum_m dY(m, n)   (optional)
A call is described by the keyword arguments of ``ops.wgrad`` plus dY, A (and dW / dB where a caller wants them);
every tensor stands for its pointer: element 0 is what the kernel's pointer addresses and the storage behind it is
what the pointer can reach (``gemm_reference.flat``).  The stored inputs convert to float64 exactly (bf16 and f32
alike); the contraction runs in float64 on the device the caller names, a chunk of rows at a time, so that a gathered
K = 9 C operand is never materialised whole.

``expected`` returns, for the dW buffer from the dW pointer onwards (guard elements behind it included) and likewise
for dB: the float64 result where the call writes and the value from before the call elsewhere, the mask of written
elements, and the magnitude sums S[n, k] = sum_m |dY(m, n) A(m, k)|, Sb[n] = sum_m |dY(m, n)| that scale the
element-wise rounding bound.  ``compare`` holds every written element to |got - want| <= n u S (or to equality, for
inputs whose sums are exact in f32) and every other element to bit-identity with before.

``fault`` names a wrong variant of the addressing (FAULTS); tests/test_wgrad_reference.py asserts that ``compare``
rejects each."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from tests.gemm_reference import _BITS, flat, nan_like_bits  # noqa: F401  (re-exported for the GPU tests)

U_F32 = 2.0 ** -24
SLAB = 32                      # rows the kernel stages per step; a split's row count is a whole number of slabs
CHUNK_ELEMS = 1 << 23          # elements of the widest gathered operand per row chunk

FAULTS = ("drop_last_row", "pad_reads_offset_zero", "segment_off_by_one", "rowmap_ignored", "bias_over_slab",
          "neighbour_rowoff")


def split_of(workspace_floats: int, N: int, Kd: int, batch: int) -> int:
    """The split a shape takes, from pp_wgrad_workspace_floats(M, N, Kd, batch) (0 = no split)."""
    per = batch * (N * Kd + N)
    assert workspace_floats % per == 0
    return max(1, workspace_floats // per)


def roundings(M: int, split: int, dtype) -> int:
    """f32 roundings on the path of one dW (or dB) element, counted from the kernel: one per accumulated row of a
    split (ceil(M / split) rounded up to a slab, at most M), the split - 1 additions of the reduction, and for f32
    operands the rounding of the product itself (a bf16 x bf16 product is exact in f32)."""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    rows = min(M, cdiv(cdiv(M, split), SLAB) * SLAB)
    return rows + (split - 1) + (1 if dtype == torch.float32 else 0)


@dataclass
class Expected:
    dW: torch.Tensor                    # float64, shaped like the dW buffer handed in
    dW_written: torch.Tensor            # bool
    S: torch.Tensor                     # float64, 0 outside the written elements
    dB: Optional[torch.Tensor] = None
    dB_written: Optional[torch.Tensor] = None
    Sb: Optional[torch.Tensor] = None


def operands(kw, b: int, r0: int, r1: int, device, fault: Optional[str] = None):
    """(dY(m, :) [r1 - r0, N], A(m, :) [r1 - r0, Kd]) of batch entry b for rows r0 <= m < r1, float64 on device."""
    dev = torch.device(device)
    M, N, Kd = kw["M"], kw["N"], kw["Kd"]
    g = lambda k: kw.get(k, 0) or 0  # noqa: E731
    batch = max(1, g("batch") or 1)
    Yf, Af = flat(kw["dY"]).to(dev), flat(kw["A"]).to(dev)
    m = torch.arange(r0, r1, device=dev)
    ym = m
    if kw.get("dy_rowmap") is not None and fault != "rowmap_ignored":
        ym = flat(kw["dy_rowmap"]).to(dev)[b * g("strideRowmap") + m].long()
    yidx = b * g("strideDY") + (ym * kw["ldd"])[:, None] + torch.arange(N, device=dev)
    Y = Yf[yidx].double()
    k = torch.arange(Kd, device=dev)
    if kw.get("rowoff") is None:
        A = Af[b * g("strideA") + (m * kw["lda"])[:, None] + k].double()
    else:
        seg_len = kw["seg_len"]
        seg, within = k // seg_len, k % seg_len
        if fault == "segment_off_by_one":           # the first column of a segment still reads the previous one
            seg = torch.where((within == 0) & (k > 0), seg - 1, seg)
        bb = (b + 1) % batch if fault == "neighbour_rowoff" else b
        ro = flat(kw["rowoff"]).to(dev)[bb * g("strideRowoff") + (seg * M)[None, :] + m[:, None]].long()
        ok = ro >= 0
        if fault == "pad_reads_offset_zero":
            A = Af[b * g("strideA") + torch.where(ok, ro, 0) + within].double()
        else:
            A = torch.where(ok, Af[torch.where(ok, b * g("strideA") + ro + within, 0)].double(), 0.0)
    return Y, A


def expected(kw, dW_before: torch.Tensor, dB_before: Optional[torch.Tensor] = None, device=None,
             fault: Optional[str] = None) -> Expected:
    """kw: the call (see the module docstring).  dW_before / dB_before: 1-D, the dW / dB buffers from the pointers
    onwards as they were before the call; dB_before None = the call passes no dB."""
    dev = torch.device(device) if device is not None else dW_before.device
    M, N, Kd = kw["M"], kw["N"], kw["Kd"]
    g = lambda k: kw.get(k, 0) or 0  # noqa: E731
    batch = max(1, g("batch") or 1)
    lddw = kw.get("lddw") or Kd
    e = Expected(dW=dW_before.double().to(dev), dW_written=torch.zeros(dW_before.shape, dtype=torch.bool, device=dev),
                 S=torch.zeros(dW_before.shape, dtype=torch.float64, device=dev))
    if dB_before is not None:
        e.dB = dB_before.double().to(dev)
        e.dB_written = torch.zeros(dB_before.shape, dtype=torch.bool, device=dev)
        e.Sb = torch.zeros(dB_before.shape, dtype=torch.float64, device=dev)
    n = torch.arange(N, device=dev)
    kk = torch.arange(Kd, device=dev)
    chunk = max(SLAB, CHUNK_ELEMS // max(N, Kd))
    rows = M - 1 if fault == "drop_last_row" else M
    for b in range(batch):
        dW = torch.zeros((N, Kd), dtype=torch.float64, device=dev)
        S = torch.zeros((N, Kd), dtype=torch.float64, device=dev)
        dB = torch.zeros((N,), dtype=torch.float64, device=dev)
        Sb = torch.zeros((N,), dtype=torch.float64, device=dev)
        for r0 in range(0, rows, chunk):
            Y, A = operands(kw, b, r0, min(rows, r0 + chunk), dev, fault)
            dW += Y.t() @ A
            S += Y.abs().t() @ A.abs()
            dB += Y.sum(0)
            Sb += Y.abs().sum(0)
            del Y, A
        if fault == "bias_over_slab" and M % SLAB:    # the rows that pad M to a whole slab, read where they would lie
            Yf = flat(kw["dY"]).to(dev)
            mm = torch.arange(M, -(-M // SLAB) * SLAB, device=dev)
            idx = b * g("strideDY") + (mm * kw["ldd"])[:, None] + n
            assert int(idx.max()) < Yf.numel(), "bias_over_slab needs the rows behind M inside the dY buffer"
            dB += Yf[idx].double().sum(0)
        dest = (b * g("strideDW") + (n * lddw)[:, None] + kk).reshape(-1)
        assert int(dest.max()) < e.dW.numel(), "call writes outside the dW buffer"
        e.dW[dest] = dW.reshape(-1)
        e.S[dest] = S.reshape(-1)
        e.dW_written[dest] = True
        if e.dB is not None:
            dest = b * g("strideDB") + n
            assert int(dest.max()) < e.dB.numel(), "call writes outside the dB buffer"
            e.dB[dest] = dB
            e.Sb[dest] = Sb
            e.dB_written[dest] = True
    return e


@dataclass
class Verdict:
    ok: bool
    ratio: float          # worst |got - want| / (n u S) over the written elements (inf: an error where S = 0, or NaN)
    bad: int              # written elements outside the bound (exact: not equal to the float64 result)
    changed: int          # elements outside what the call writes that are not bit-identical to before

    def __str__(self):
        s = f"d/bound {self.ratio:.3g}"
        if not self.ok:
            s += f"  FAIL: {self.bad} outside the bound, {self.changed} unwritten elements changed"
        return s


def compare(got: torch.Tensor, before: torch.Tensor, ref: torch.Tensor, written: torch.Tensor, S: torch.Tensor,
            n: int, exact: bool = False) -> Verdict:
    """got / before: 1-D f32 buffers after / before the call; ref, written, S from ``expected`` (same shape).
    exact: every sum is exact in f32 in any order, so got must equal ref; otherwise |got - ref| <= n u S."""
    dev = ref.device
    got, before = got.to(dev), before.to(dev)
    bits = _BITS[got.dtype]
    changed = int(((got.view(bits) != before.view(bits)) & ~written).sum())
    o, r, s = got[written].double(), ref[written], S[written]
    d = (o - r).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    bound = torch.zeros_like(s) if exact else n * U_F32 * s
    bad = int((~(d <= bound)).sum())
    q = torch.where(d == 0, torch.zeros_like(d), d / (n * U_F32 * s))       # d > 0 over S = 0 gives inf
    ratio = float(q.max()) if q.numel() else 0.0
    return Verdict(ok=bad == 0 and changed == 0, ratio=ratio, bad=bad, changed=changed)
