"""CPU tests of the float64 attention restatement (tests/attention_reference.py) and of its comparator.

(1) The restatement equals F.scaled_dot_product_attention in float64, and its head-major read equals the row-major
read of the permuted buffer.
(2) The comparator accepts an emulation of the kernels' algorithm (f32 scores, online softmax over key blocks with the
running-max rescale, P rounded to bf16 for the second product, f32 accumulation, one rounding of the output), and
rejects what a subtly broken kernel would leave behind: a dropped key (first and tail key block), a missing rescale, a
softmax scale 1 % off, two 16-row query groups swapped, a 16-dim output tile taken from the neighbouring head, a row
never written, a guard element written."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attention_reference as ar
from tests import gemm_reference as gr

BF16, F32, FP8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
LEAD, TRAIL = 8, 24


def _qkv(B, N, heads, hd, qscale, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn((B * N, 3, heads * hd), generator=g)
    t[:, 0] *= qscale
    return t.reshape(B * N, 3 * heads * hd).to(BF16)


def emulate(qkv, B, N, heads, hd, out_dtype=BF16, inv_scale=None, kb=64, drop=None, rescale=True, scale_mult=1.0):
    """The kernels' algorithm in f32: key blocks of kb, running max of the scaled scores, P rounded to bf16 for P V
    (f32 P in the row sum), output rounded once.  drop: a key index every query ignores."""
    q, k, v = (t.float() for t in ar.problems(qkv, B, N, heads, hd))
    c = torch.tensor(math.log2(math.e) / math.sqrt(hd) * scale_mult, dtype=F32)
    P = B * heads
    m = torch.full((P, N, 1), -math.inf)
    l = torch.zeros((P, N, 1))
    o = torch.zeros((P, N, hd))
    for k0 in range(0, N, kb):
        s = (q @ k[:, k0:k0 + kb].transpose(1, 2)) * c
        if drop is not None and k0 <= drop < k0 + kb:
            s[:, :, drop - k0] = -math.inf
        m_new = torch.maximum(m, s.amax(dim=-1, keepdim=True))
        alpha = torch.exp2(m - m_new) if rescale else torch.ones_like(m)
        p = torch.exp2(s - m_new)
        l = l * alpha + p.sum(dim=-1, keepdim=True)
        pv = p if out_dtype == F32 else p.to(BF16).float()
        o = o * alpha + pv @ v[:, k0:k0 + kb]
        m = m_new
    o = o / l
    o = o.reshape(B, heads, N, hd).transpose(1, 2).reshape(B * N, heads * hd)
    if out_dtype == FP8:
        return (o * torch.tensor(inv_scale, dtype=F32)).clamp(-448.0, 448.0).to(FP8)
    return o.to(out_dtype)


def _buffers(out):
    before = gr.nan_like_bits(LEAD + out.numel() + TRAIL, out.dtype, "cpu")
    got = before.clone()
    got[LEAD:LEAD + out.numel()] = out.reshape(-1)
    return got, before


def _verdict(got, before, qkv, B, N, heads, hd, out_dtype=BF16, inv_scale=None):
    ref, ref_abs = ar.expected_attention(qkv, B, N, heads, hd)
    return ar.compare(got, before, LEAD, *ar.attention_target(ref, ref_abs, out_dtype, inv_scale))


@pytest.mark.parametrize("hd", [32, 64, 80])
@pytest.mark.parametrize("headmajor", [False, True])
def test_restatement_equals_sdpa_and_headmajor_read(hd, headmajor):
    B, N, heads = 2, 37, 3
    qkv = _qkv(B, N, heads, hd, 1.0, 1)
    q, k, v = qkv.double().reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * N, heads * hd)
    ref, ref_abs = ar.expected_attention(qkv, B, N, heads, hd)
    torch.testing.assert_close(ref, want, rtol=1e-12, atol=1e-12)
    want_abs = F.scaled_dot_product_attention(q, k, v.abs()).transpose(1, 2).reshape(B * N, heads * hd)
    torch.testing.assert_close(ref_abs, want_abs, rtol=1e-12, atol=1e-12)
    if headmajor:
        hm = qkv.reshape(B * N, 3, heads, hd).permute(1, 2, 0, 3).contiguous().reshape(B * N, 3 * heads * hd)
        r2, a2 = ar.expected_attention(hm, B, N, heads, hd, headmajor=True)
        assert torch.equal(r2, ref) and torch.equal(a2, ref_abs)


@pytest.mark.parametrize("qscale", [0.1, 1.0, 3.0])
@pytest.mark.parametrize("N", [192, 432, 1000])
@pytest.mark.parametrize("hd", [32, 64, 80])
def test_comparator_accepts_the_emulated_kernel(hd, N, qscale):
    B, heads = 1, 2
    qkv = _qkv(B, N, heads, hd, qscale, 2)
    for kb in (32, 96):
        out = emulate(qkv, B, N, heads, hd, kb=kb)
        v = _verdict(*_buffers(out), qkv, B, N, heads, hd)
        assert v.ok and v.worst < 1.0, f"kb {kb}: {v}"


@pytest.mark.parametrize("out_dtype", [F32, FP8])
@pytest.mark.parametrize("hd", [32, 80])
def test_comparator_accepts_the_emulated_f32_and_e4m3_outputs(hd, out_dtype):
    B, N, heads = 1, 433, 2
    qkv = _qkv(B, N, heads, hd, 3.0, 3)
    if out_dtype == F32:       # the VALU kernel reads bf16 or f32 qkv, keeps P in f32
        qkv = qkv.float()
    inv = None
    if out_dtype == FP8:
        ref, _ = ar.expected_attention(qkv, B, N, heads, hd)
        inv = 448.0 / (1.25 * float(ref.abs().max()))
    out = emulate(qkv, B, N, heads, hd, out_dtype=out_dtype, inv_scale=inv)
    v = _verdict(*_buffers(out), qkv, B, N, heads, hd, out_dtype, inv)
    assert v.ok and v.worst < 1.0, str(v)


FAULTS = ["drop_first_block", "drop_tail_block", "no_rescale", "scale_1.01", "swap_query_groups", "neighbour_head_tile",
          "unwritten_row", "guard_written"]


# a 1 % scale error on the nearly flat softmax of q scale 0.1 moves outputs less than rounding P does: not a fault
# any per-element bound can see, so it is planted at q scales 1 and 3 only
CASES = [(f, s) for f in FAULTS for s in (0.1, 1.0, 3.0) if not (f == "scale_1.01" and s < 1)]


@pytest.mark.parametrize("fault,qscale", CASES)
def test_comparator_rejects_planted_faults(fault, qscale):
    B, N, heads, hd = 2, 433, 3, 64
    qkv = _qkv(B, N, heads, hd, qscale, 4)
    C = heads * hd
    kw = {"drop_first_block": dict(drop=5), "drop_tail_block": dict(drop=N - 3), "no_rescale": dict(rescale=False),
          "scale_1.01": dict(scale_mult=1.01)}.get(fault, {})
    out = emulate(qkv, B, N, heads, hd, **kw)
    if fault == "swap_query_groups":
        out = out.clone()
        out[N + 32:N + 48], out[N + 48:N + 64] = out[N + 48:N + 64].clone(), out[N + 32:N + 48].clone()
    if fault == "neighbour_head_tile":
        out = out.clone()
        out[:N, 16:32] = out[:N, hd + 16:hd + 32]
    got, before = _buffers(out)
    if fault == "unwritten_row":
        got[LEAD + 7 * C:LEAD + 8 * C] = before[LEAD + 7 * C:LEAD + 8 * C]
    if fault == "guard_written":
        got[LEAD + B * N * C + 5] = 0.0
    v = _verdict(got, before, qkv, B, N, heads, hd)
    assert not v.ok, f"{fault} passed: {v}"
    print(f"{fault} qscale {qscale}: {v}")
