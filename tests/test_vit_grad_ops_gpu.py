"""GPU tests of the backbone's backward kernels (csrc/pp_vit_grad.hip) against float64 torch.

Bounds, |got - want| <= c u max|want| per tensor (head_grad_reference.ratio), u = 2^-24 (f32) or 2^-8 (bf16 storage):
* attention backward, f32 (VALU): each output element is a sum over N keys (or queries) of products whose factors
  carry the rounding of a dot product of length hd and of one exp: c = 4 (sqrt(N) + sqrt(hd)) + 16.  bf16 (MFMA): the
  inputs are the bf16 values the reference also takes and the accumulation is f32, but the second products take P
  and dS rounded to bf16 (u relative per term of a length-N sum of terms with varying signs: about sqrt(N) u against
  the result), O is the forward's bf16 output (one rounding inside D = rowsum(dO o O)) and the result is rounded once
  to bf16: c = 2 sqrt(N) + 4.
* LayerNorm backward: row sums of length C in f32 (mean, variance, two projections): c = 4 sqrt(C) + 16 for dx;
  the column sums run in float64 over f32 products: c = 16 for dgamma / dbeta.  bf16 dres_c: one more rounding, c = 1
  against the f32 result.
* GELU forward / backward: erff / expf to a few ulps, c = 16; bf16 output: c = 1 (one rounding).
* pos_embed sum: B f32 additions, c = B.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.head_grad_reference import U_BF16, U_F32, ratio

pytestmark = pytest.mark.gpu

U = {torch.float32: U_F32, torch.bfloat16: U_BF16}


@pytest.fixture
def ops(built_lib):
    from probpose_pytorch_amd import ops
    return ops


def _attn_ref(qkv, dO, B, N, heads, hd):
    qkv = qkv.double().cpu().requires_grad_(True)
    q, k, v = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * N, heads * hd)
    (g,) = torch.autograd.grad(o, qkv, dO.double().cpu())
    return g


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [35, 48, 192, 576])
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_backward_matches_sdpa_autograd(ops, hd, N, dt):
    B, heads = 2, 2
    C = heads * hd
    gen = torch.Generator().manual_seed(hd * 1000 + N)
    qkv = torch.randn((B * N, 3 * C), generator=gen).to(dt).cuda()
    dO = torch.randn((B * N, C), generator=gen).to(dt).cuda()
    out = torch.empty((B * N, C), dtype=dt, device="cuda")
    ops.attention(qkv, out, B, N, heads, hd)
    dqkv = torch.empty((B * N, 3 * C), dtype=dt, device="cuda")
    ops.attention_backward(qkv, out, dO, dqkv, B, N, heads, hd)
    want = _attn_ref(qkv, dO, B, N, heads, hd)
    c = 4 * (math.sqrt(N) + math.sqrt(hd)) + 16 if dt == torch.float32 else 2 * math.sqrt(N) + 4
    for part, name in enumerate("qkv"):
        sl = slice(part * C, (part + 1) * C)
        r = ratio(dqkv[:, sl], want[:, sl], U[dt], c)
        print(f"d/bound attention backward hd {hd} N {N} {dt} d{name}: {r:.3g}")
        assert r <= 1.0, (name, r)
    again = torch.empty_like(dqkv)
    ops.attention_backward(qkv, out, dO, again, B, N, heads, hd)
    assert torch.equal(dqkv, again)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,C", [(300, 64), (1152, 384), (2500, 768)])
def test_layernorm_backward_matches_float64(ops, rows, C, dt):
    gen = torch.Generator().manual_seed(rows + C)
    x = (torch.randn((rows, C), generator=gen) * 2 + 0.5).cuda()
    gamma = (0.8 + 0.4 * torch.rand(C, generator=gen)).cuda()
    dy = torch.randn((rows, C), generator=gen).cuda()
    dres0 = torch.randn((rows, C), generator=gen).cuda()
    dres = dres0.clone()
    dres_c = torch.empty((rows, C), dtype=dt, device="cuda")
    dgb = torch.empty((2, C), device="cuda")
    ops.layernorm_backward(x, gamma, 1e-6, dy, dres, dres_c, True, dgamma=dgb[0], dbeta=dgb[1])
    xd = x.double().cpu().requires_grad_(True)
    gd = gamma.double().cpu().requires_grad_(True)
    bd = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    y = F.layer_norm(xd, (C,), gd, bd, 1e-6)
    dx, dg, db = torch.autograd.grad(y, (xd, gd, bd), dy.double().cpu())
    assert ratio(dres - dres0, dx, U_F32, 4 * math.sqrt(C) + 16 + 4) <= 1.0
    assert ratio(dgb[0], dg, U_F32, 16) <= 1.0 and ratio(dgb[1], db, U_F32, 16) <= 1.0
    assert ratio(dres_c, dres, U[dt], 1) <= 1.0
    # overwrite form, and repeated calls give the same bits
    d2 = torch.empty_like(dres)
    c2 = torch.empty_like(dres_c)
    dgb2 = torch.empty_like(dgb)
    ops.layernorm_backward(x, gamma, 1e-6, dy, d2, c2, False, dgamma=dgb2[0], dbeta=dgb2[1])
    assert ratio(d2, dx, U_F32, 4 * math.sqrt(C) + 16) <= 1.0
    d3 = torch.empty_like(dres)
    c3 = torch.empty_like(dres_c)
    dgb3 = torch.empty_like(dgb)
    ops.layernorm_backward(x, gamma, 1e-6, dy, d3, c3, False, dgamma=dgb3[0], dbeta=dgb3[1])
    assert torch.equal(d2, d3) and torch.equal(c2, c3) and torch.equal(dgb2, dgb3)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_gelu_forward_backward_match_float64(ops, dt):
    n = 4099
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(n, generator=gen) * 16 - 8).cuda()
    g = torch.randn(n, generator=gen).cuda()
    y = torch.empty(n, dtype=dt, device="cuda")
    dx = torch.empty(n, dtype=dt, device="cuda")
    ops.gelu_forward(x, y)
    ops.gelu_backward(x, g, dx)
    xd = x.double().cpu().requires_grad_(True)
    yd = F.gelu(xd)
    (gd,) = torch.autograd.grad(yd, xd, g.double().cpu())
    c = 16 if dt == torch.float32 else 1 + 16 * U_F32 / U_BF16
    assert ratio(y, yd.detach(), U[dt], c) <= 1.0
    assert ratio(dx, gd, U[dt], c) <= 1.0


def test_rows_period_sum_is_the_pos_embed_gradient(ops):
    B, N, C = 5, 35, 64
    x = torch.randn((B * N, C), generator=torch.Generator().manual_seed(9)).cuda()
    out = torch.empty((N, C), device="cuda")
    ops.rows_period_sum(x, B, N, C, out)
    want = x.double().cpu().reshape(B, N, C).sum(0)
    assert ratio(out, want, U_F32, B) <= 1.0
    out2 = torch.empty_like(out)
    ops.rows_period_sum(x, B, N, C, out2)
    assert torch.equal(out, out2)


def test_argument_validation(ops):
    from probpose_pytorch_amd import _lib
    qkv = torch.zeros((2 * 16, 3 * 160), device="cuda")
    with pytest.raises(_lib.HipExtensionError, match="head_dim 80"):
        ops.attention_backward(qkv, qkv[:, :160], qkv[:, :160], qkv, 2, 16, 2, 80)
