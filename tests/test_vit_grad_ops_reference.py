"""CPU checks of tests/vit_grad_ops_reference.py: the explicit float64 backward is the SDPA autograd's, the bf16 rounding
model lies inside the float64 bound the GPU test has always used, and every planted fault falls outside the
element-wise bounds at every shape tests/test_vit_grad_ops_gpu.py runs.

Two planted faults compute the fault-free function at one shape each, so no bound can reject them there; the tests
assert that identity instead of a rejection:
* 'dropped_last_key' at N = 1: dS = P (dO . v - dO . O) and O = v, so dQ is 0 with or without its only key.
* 'unmasked_key' in the peaked case: the zero key's score 0 lies about 50 below the row maxima, its share of every
  P is exp(-lse): the exact results differ by less than 10^-3 of the f32 bound, and the model's do not differ.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import vit_grad_ops_reference as R

SHAPES = [(hd, B, heads, N, False) for hd in R.ATTN_HD for B, heads in R.ATTN_BH for N in R.ATTN_N]
SHAPES += [(hd, 1, 1, R.PEAKED_N, True) for hd in R.ATTN_HD]


@functools.lru_cache(maxsize=2)
def _case(hd, B, heads, N, peaked):
    """Inputs, the float64 forward, its bf16 rounding (what the bf16 forward kernel hands the backward), the exact
    backward with companions and the fault-free model."""
    qkv, dO = R.attention_inputs(B, N, heads, hd, seed=hd * 1000 + N, peaked=peaked)
    O64 = R.attention_forward(qkv, B, N, heads, hd)
    O16 = R.rn_bf16(O64)
    want, comp = R.attention_backward(qkv, O64, dO, B, N, heads, hd)
    x, E = R.attention_backward_bf16_model(qkv, O16, dO, B, N, heads, hd)
    return qkv, dO, O64, O16, want, comp, x, E


def test_rn_bf16_is_torch_rounding():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * torch.logspace(-30, 30, 4096)
    x = torch.cat([x, torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0, 2.0 ** -130])])   # ties, 0, subnormal
    assert torch.equal(R.rn_bf16(x.double()), x.bfloat16().double())
    # one rounding: a float64 just above a bf16 tie that f32 would first round onto the tie
    y = torch.tensor([1.00390625 + 2.0 ** -40], dtype=torch.float64)
    assert float(R.rn_bf16(y)) == 1.0078125 and float(y.float().bfloat16()) == 1.0


@pytest.mark.parametrize("hd,B,heads,N", [(32, 2, 2, 35), (64, 2, 3, 17), (32, 1, 1, 1), (64, 1, 2, 129)])
def test_explicit_backward_is_sdpa_autograd(hd, B, heads, N):
    qkv, dO = R.attention_inputs(B, N, heads, hd, seed=N)
    leaf = qkv.double().requires_grad_(True)
    q, k, v = leaf.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * N, heads * hd)
    (g,) = torch.autograd.grad(o, leaf, dO.double())
    O = R.attention_forward(qkv, B, N, heads, hd)
    assert float((O - o.detach()).abs().max()) <= 1e-12 * float(o.detach().abs().max())
    got, comp = R.attention_backward(qkv, O, dO, B, N, heads, hd)
    assert float((got - g).abs().max()) <= 1e-12 * float(g.abs().max())
    assert bool((got.abs() <= comp * (1 + 1e-12)).all())          # a companion dominates its value


@pytest.mark.parametrize("hd,B,heads,N,peaked", SHAPES)
def test_bf16_model_lies_inside_the_float64_bound(hd, B, heads, N, peaked):
    _, _, _, _, want, _, x, _ = _case(hd, B, heads, N, peaked)
    C = heads * hd
    for part in range(3):
        sl = slice(part * C, (part + 1) * C)
        r = R.ratio_per_tensor(R.rn_bf16(x[:, sl]), want[:, sl], R.U_BF16, R.c_attention_f64_vs_bf16(N))
        assert r <= 1.0, ("qkv"[part], r)


@pytest.mark.parametrize("hd,B,heads,N,peaked,fault", [s + (f,) for s in SHAPES for f in R.ATTENTION_FAULTS])
def test_planted_attention_faults_exceed_both_bounds(hd, B, heads, N, peaked, fault):
    qkv, dO, O64, O16, want, comp, x, E = _case(hd, B, heads, N, peaked)
    xf, _ = R.attention_backward_bf16_model(qkv, O16, dO, B, N, heads, hd, fault=fault)
    wf, _ = R.attention_backward(qkv, O64, dO, B, N, heads, hd, fault=fault)
    f32_bound = R.c_attention_f32(N, hd) * R.U_F32 * comp
    if fault == "dropped_last_key" and N == 1:
        assert torch.equal(xf, x) and torch.equal(wf, want)
        return
    if fault == "unmasked_key" and peaked:
        assert R.within(wf, want, 1e-3 * f32_bound)[0] and torch.equal(R.rn_bf16(xf), R.rn_bf16(x))
        return
    ok16, r16 = R.inside_model(R.rn_bf16(xf), x, E)
    ok32, r32 = R.within(wf, want, f32_bound)
    assert not ok16 and r16 > 1.0, r16
    assert not ok32 and r32 > 1.0, r32


def test_model_inside_its_own_bound():
    _, _, _, _, _, _, x, E = _case(32, 2, 3, 33, False)
    assert R.inside_model(R.rn_bf16(x), x, E) == (True, 0.0)
    assert bool((E > 0).all())


@pytest.mark.parametrize("fault", R.LN_FAULTS)
@pytest.mark.parametrize("rows,C,large_mean", [s + (False,) for s in R.LN_SHAPES] + [R.LN_LARGE_MEAN_SHAPE + (True,)])
def test_planted_layernorm_faults_exceed_the_bounds(rows, C, large_mean, fault):
    x, gamma, dy, _ = R.ln_inputs(rows, C, rows + C, *((50.0, 1.0) if large_mean else (0.5, 2.0)))
    ref = R.layernorm_backward(x, gamma, dy, 1e-6)
    bad = R.layernorm_backward(x, gamma, dy, 1e-6, fault=fault)
    bdx, bdg, bdb = R.ln_bounds(ref, C)
    if fault == "last_column_skipped":
        assert not R.within(bad["dx"], ref["dx"], bdx)[0]
    else:
        assert not R.within(bad["dgamma"], ref["dgamma"], bdg)[0]
        assert not R.within(bad["dbeta"], ref["dbeta"], bdb)[0]


@pytest.mark.parametrize("rows,C", [(5, 65), (1025, 36)])
def test_layernorm_reference_is_torch_autograd(rows, C):
    x, gamma, dy, _ = R.ln_inputs(rows, C, 1)
    xd, gd = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    bd = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    want = torch.autograd.grad(F.layer_norm(xd, (C,), gd, bd, 1e-6), (xd, gd, bd), dy.double())
    ref = R.layernorm_backward(x, gamma, dy, 1e-6)
    for name, w in zip(("dx", "dgamma", "dbeta"), want):
        assert float((ref[name] - w).abs().max()) <= 1e-12 * float(w.abs().max()), name
        assert bool((ref[name].abs() <= ref["comp_" + name] * (1 + 1e-12)).all()), name
    assert 1.0 <= float(ref["kappa"].min()) and float(ref["kappa"].max()) < 2.0


def test_gelu_reference_and_its_fault():
    x, g = R.gelu_inputs(4099, 5)
    xd = x.double().requires_grad_(True)
    y = F.gelu(xd)
    (gd,) = torch.autograd.grad(y, xd, g.double())
    want_y, by = R.gelu(x)
    want_g, bg = R.gelu(x, g)
    assert float((want_y - y.detach()).abs().max()) <= 1e-15 * 8 and float((want_g - gd).abs().max()) <= 1e-14
    # the negative tail keeps its digits where 0.5 (1 + erf) has none left
    assert float(R.gelu(torch.tensor([-40.0]))[0]) == 0.0 and float(R.gelu(torch.tensor([-8.0]))[0]) < 0
    # the derivative without its x phi(x) term (vit_grad_reference's 'gelu_grad') is outside the bound
    cdf = 0.5 * torch.special.erfc(-x.double() / math.sqrt(2.0))
    assert not R.within(g.double() * cdf, want_g, bg)[0]
    assert float(by[0]) == 0.0 and float(by[1]) == 0.0          # +-0: the output is exactly 0
