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

The tests of the second half are element-wise, |got - want| <= bound per element, at the shapes that reach every tile
edge; tests/vit_grad_ops_reference.py derives each bound and its CPU tests show that every planted fault exceeds it.
Worst d/bound measured on an MI355X (printed under -s):
* attention backward f32 (VALU) against float64, c = 4 (sqrt(N) + sqrt(hd)) + 16 per element: dq 0.041, dk 0.037,
  dv 0.095 over hd {32, 64} x (B, heads) {(1, 1), (2, 3)} x 15 N.  Peaked case (|s| about 50): hd 32 dq 0.17, dk 0.26,
  dv 0.72; hd 64 dq 0.15, dk 0.13, dv 0.65 -- see test_attention_backward_elementwise_peaked.
* attention backward bf16 (MFMA) against the rounding model: every element inside [rn(x - E), rn(x + E)]; the share of
  E needed reaches 0.996 (a term whose bf16 rounding flipped uses the whole ulp it is allowed, so shares near 1 are
  flips, not a thin constant); peaked 0.010.  About 0.1 % of the elements differ from the model's own bits.  Measured
  once with c_model scaled down: all 3.0 M elements of these shapes stay inside at c_model / 16, 3 fall outside at
  c_model / 32.
* LayerNorm backward: dx 0.26 (large mean 0.0037), dgamma 0.11 (0.073), dbeta 0.99 (0.92: one rounding, c = 1).
* GELU: forward 0.25, backward 0.37 (f32); 0.996 with a bf16 output (one rounding, c = 1).  rows_period_sum 0.5.
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


# ===============================================================================================================
# Element by element, at the tile edges (tests/vit_grad_ops_reference.py states and derives every bound).  Every
# output and workspace lies inside a larger allocation filled with a sentinel bit pattern: the guard zones keep their
# bits, and no sentinel is left where the kernel has to write.
# ===============================================================================================================
import functools  # noqa: E402

from tests import vit_grad_ops_reference as R  # noqa: E402
from tests.gemm_reference import nan_like_bits  # noqa: E402
from tests.test_droppath_ops_gpu import _bits, _buf  # noqa: E402

GUARD = 64                      # elements on either side of an output (a multiple of 16 bytes in both dtypes)
WS_GUARD = 256                  # bytes on either side of a workspace
DTYPES = [torch.float32, torch.bfloat16]
_WORST: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k in sorted(_WORST):
        print(f"worst d/bound {k}: {_WORST[k]:.3g}")


def _note(cls, r):
    _WORST[cls] = max(_WORST.get(cls, 0.0), float(r))
    return r


def _tag(dt):
    return str(dt).replace("torch.", "")


class Guarded:
    """A contiguous tensor of ``shape`` inside a sentinel-filled allocation (a quiet NaN in every element) with GUARD
    elements on either side."""

    def __init__(self, shape, dtype):
        n = math.prod(shape)
        self.n = n
        self.buf = nan_like_bits(n + 2 * GUARD, dtype, "cuda")
        self.before = _bits(self.buf).clone()
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def guards_intact(self):
        now = _bits(self.buf)
        return (torch.equal(now[:GUARD], self.before[:GUARD])
                and torch.equal(now[GUARD + self.n:], self.before[GUARD + self.n:]))

    def sentinels(self, t=None):
        """How many elements of t (default: the whole tensor) still hold the sentinel."""
        t = self.t if t is None else t
        return int((_bits(t) == self.before[0]).sum())


class GuardedBytes:
    """A workspace of ``nbytes`` whose guard zone starts right at nbytes (and one ahead of it)."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t = self.buf[WS_GUARD:WS_GUARD + self.n]

    def guards_intact(self):
        return bool((self.buf[:WS_GUARD] == 0xA5).all()) and bool((self.buf[WS_GUARD + self.n:] == 0xA5).all())


def _attn_ws_bytes(built_lib, B, N, heads):
    return int(built_lib.pp_attention_backward_workspace_bytes(B, N, heads))


def _attention_call(ops, built_lib, qkv, dO, B, N, heads, hd, dt):
    """Forward by ops.attention, backward into guarded buffers: (out, dqkv), both on the device."""
    C = heads * hd
    qkv_d, dO_d = qkv.to(dt).cuda(), dO.to(dt).cuda()
    out = torch.empty((B * N, C), dtype=dt, device="cuda")
    ops.attention(qkv_d, out, B, N, heads, hd)
    dqkv = Guarded((B * N, 3 * C), dt)
    ws = GuardedBytes(_attn_ws_bytes(built_lib, B, N, heads))
    assert ws.n == 2 * B * heads * N * 4
    ops.attention_backward(qkv_d, out, dO_d, dqkv.t, B, N, heads, hd, ws=ws.t)
    torch.cuda.synchronize()
    assert dqkv.guards_intact(), "dqkv guard zone written"
    assert ws.guards_intact(), "workspace guard zone written"
    assert dqkv.sentinels() == 0, "dqkv element not written"
    return out, dqkv.t


def _attention_check(ops, built_lib, B, N, heads, hd, dt, peaked):
    C = heads * hd
    qkv, dO = R.attention_inputs(B, N, heads, hd, seed=hd * 1000 + N, peaked=peaked, dtype=dt)
    out, dqkv = _attention_call(ops, built_lib, qkv, dO, B, N, heads, hd, dt)
    kind = "peaked" if peaked else "randn"
    fails = []
    if dt == torch.float32:
        want, comp = R.attention_backward(qkv, out, dO, B, N, heads, hd)
        bound = R.c_attention_f32(N, hd) * R.U_F32 * comp
    else:
        x, E = R.attention_backward_bf16_model(qkv, out, dO, B, N, heads, hd)
    for part, name in enumerate("qkv"):
        sl = slice(part * C, (part + 1) * C)
        if dt == torch.float32:
            ok, r = R.within(dqkv[:, sl], want[:, sl], bound[:, sl])
            cls = f"attention_backward float32 d{name} {kind} [c u companion, against float64]"
        else:
            ok, r = R.inside_model(dqkv[:, sl], x[:, sl], E[:, sl])
            cls = f"attention_backward bfloat16 d{name} {kind} [share of E, against the bf16 model]"
        _note(cls, r)
        print(f"d/bound attention backward hd {hd} B {B} heads {heads} N {N} {_tag(dt)} {kind} d{name}: {r:.3g}")
        if not ok:
            fails.append((name, r))
    assert not fails, fails


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", R.ATTN_N)
@pytest.mark.parametrize("B,heads", R.ATTN_BH)
@pytest.mark.parametrize("hd", R.ATTN_HD)
def test_attention_backward_elementwise_at_tile_edges(ops, built_lib, hd, B, heads, N, dt):
    _attention_check(ops, built_lib, B, N, heads, hd, dt, False)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hd", R.ATTN_HD)
def test_attention_backward_elementwise_peaked(ops, built_lib, hd, dt):
    """q and k times 4: |s| about 50, rows of P nearly one-hot.

    P = expf(s - lse) turns an absolute error of the score into a relative error of P, and the companion
    sum_i P_ij |dO_i| carries no |s| factor: this case holds the f32 kernels to a score that is right to one rounding
    of its own size.  With the score summed as a plain f32 fma chain they missed the bound (measured d/bound: hd 32
    dq 1.09, dk 1.17, dv 3.15; hd 64 dq 0.46, dk 0.47, dv 1.84; numpy float32 on the CPU: dv 2.3 and 4.4); with the
    compensated score of csrc/pp_vit_grad.hip they need hd 32 dq 0.17, dk 0.26, dv 0.72 and hd 64 dq 0.15, dk 0.13,
    dv 0.65, which is what float64 arithmetic on a score rounded once to f32 gives on the CPU (0.71 and 0.67: the
    half ulp of a score of 50 and of its lse, 32 u each, is the floor of the format).  The bf16 kernels stay inside
    the model's allowance (worst share 0.010)."""
    _attention_check(ops, built_lib, 1, R.PEAKED_N, 1, hd, dt, True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hd", R.ATTN_HD)
def test_attention_backward_isolates_crops_and_heads(ops, built_lib, hd, dt):
    """Changing the inputs of one (crop, head) leaves every other (crop, head) slice of dqkv bit-identical, and each
    crop alone at B = 1 gives the bits it gives inside the batch."""
    B, heads, N = 3, 3, 33
    C = heads * hd
    qkv, dO = R.attention_inputs(B, N, heads, hd, seed=7 + hd, dtype=dt)
    _, base = _attention_call(ops, built_lib, qkv, dO, B, N, heads, hd, dt)
    noise_q, noise_g = R.attention_inputs(B, N, heads, hd, seed=8 + hd, dtype=dt)

    def cols(h, width):          # the columns of head h in a row of `width` / C parts
        return [p * C + h * hd + d for p in range(width) for d in range(hd)]

    for b, h in ((0, 0), (1, 2), (2, 1)):
        q2, g2 = qkv.clone(), dO.clone()
        rows = slice(b * N, (b + 1) * N)
        q2[rows, cols(h, 3)] = noise_q[rows, cols(h, 3)]
        g2[rows, cols(h, 1)] = noise_g[rows, cols(h, 1)]
        _, got = _attention_call(ops, built_lib, q2, g2, B, N, heads, hd, dt)
        same = torch.ones((B * N, 3 * C), dtype=torch.bool, device="cuda")
        same[rows, cols(h, 3)] = False
        assert torch.equal(_bits(got)[same], _bits(base)[same]), (b, h)
        assert not torch.equal(_bits(got)[~same], _bits(base)[~same]), (b, h)
    for b in range(B):
        rows = slice(b * N, (b + 1) * N)
        _, alone = _attention_call(ops, built_lib, qkv[rows].clone(), dO[rows].clone(), 1, N, heads, hd, dt)
        assert torch.equal(_bits(alone), _bits(base[rows])), b


@pytest.mark.parametrize("hd", R.ATTN_HD)
def test_attention_backward_f32_from_unaligned_buffers(ops, built_lib, hd):
    """The VALU kernels load and store scalars: buffers (the workspace too) that start 4 bytes past an aligned address
    give the bits that aligned buffers give."""
    B, heads, N = 2, 3, 65
    C = heads * hd
    qkv, dO = R.attention_inputs(B, N, heads, hd, seed=11 + hd, dtype=torch.float32)
    out, base = _attention_call(ops, built_lib, qkv, dO, B, N, heads, hd, torch.float32)
    f32 = torch.float32
    q1, o1, g1 = _buf(qkv.shape, f32, 1, fill=qkv), _buf(out.shape, f32, 1, fill=out), _buf(dO.shape, f32, 1, fill=dO)
    d1 = _buf((B * N, 3 * C), f32, 1, fill=torch.full((B * N, 3 * C), math.nan))
    ws = torch.empty(_attn_ws_bytes(built_lib, B, N, heads) + 4, dtype=torch.uint8, device="cuda")[4:]
    assert all(t.data_ptr() % 16 == 4 for t in (q1, o1, g1, d1, ws))
    ops.attention_backward(q1, o1, g1, d1, B, N, heads, hd, ws=ws)
    assert torch.equal(_bits(d1), _bits(base))


# ---- LayerNorm backward -----------------------------------------------------------------------------------------
LN_CASES = [s + (False,) for s in R.LN_SHAPES] + [R.LN_LARGE_MEAN_SHAPE + (True,)]
LN_PAD, LN_LEAD = 12, 5         # dy as columns [5, 5 + C) of a [rows, C + 12] tensor whose other columns are NaN


@functools.lru_cache(maxsize=2)
def _ln_case(rows, C, large):
    x, gamma, dy, dres0 = R.ln_inputs(rows, C, rows + C, *((50.0, 1.0) if large else (0.5, 2.0)))
    ref = R.layernorm_backward(x, gamma, dy, 1e-6)
    return x, gamma, dy, dres0, ref, R.ln_bounds(ref, C)


@pytest.mark.parametrize("rows,C,large,dt", [c + (dt,) for c in LN_CASES for dt in DTYPES])
def test_layernorm_backward_elementwise_at_the_tails(ops, built_lib, rows, C, large, dt):
    """Row tail (rows % 4), lane and column tails (C % 64), one chunk / two chunks / the 256-chunk clamp, ldy = C and
    ldy = C + 12, accumulate on and off, dgamma / dbeta both, either, neither.  The large-mean case (x = 50 + randn,
    kappa = 51) runs under the same bounds: they carry kappa = (|mean| + sigma) / sigma per row."""
    x, gamma, dy, dres0, ref, (bdx, bdg, bdb) = _ln_case(rows, C, large)
    x_d, gamma_d, dres0_d = x.cuda(), gamma.cuda(), dres0.cuda()
    wide = torch.full((rows, C + LN_PAD), math.nan, device="cuda")
    wide[:, LN_LEAD:LN_LEAD + C] = dy.cuda()
    dys = {C: dy.cuda(), C + LN_PAD: wide[:, LN_LEAD:LN_LEAD + C]}
    ws_bytes = int(built_lib.pp_layernorm_backward_workspace_bytes(rows, C))
    chunks = min(max((rows + 1023) // 1024, 1), 256)
    assert ws_bytes == 8 * rows + 16 * chunks * C
    kind = "large mean" if large else "randn"
    first = {}
    for ldy, dy_d in dys.items():
        assert dy_d.stride(0) == ldy
        for accumulate in (False, True):
            for which in ("both", "dgamma", "dbeta", "neither"):
                dres, dres_c = Guarded((rows, C), torch.float32), Guarded((rows, C), dt)
                dgb, ws = Guarded((2, C), torch.float32), GuardedBytes(ws_bytes)
                if accumulate:
                    dres.t.copy_(dres0_d)
                ops.layernorm_backward(x_d, gamma_d, 1e-6, dy_d, dres.t, dres_c.t, accumulate,
                                       dgamma=dgb.t[0] if which in ("both", "dgamma") else None,
                                       dbeta=dgb.t[1] if which in ("both", "dbeta") else None, ws=ws.t)
                torch.cuda.synchronize()
                where = (ldy, accumulate, which)
                assert dres.guards_intact() and dres_c.guards_intact() and dgb.guards_intact(), where
                assert ws.guards_intact(), where
                assert dres.sentinels() == 0 and dres_c.sentinels() == 0, where
                got = dres.t.double().cpu()
                bound = bdx
                if accumulate:          # one more f32 addition
                    bound = bdx + R.U_F32 * got.abs()
                    got = got - dres0.double()
                ok, r = R.within(got, ref["dx"], bound)
                _note(f"layernorm_backward dx {kind} [c kappa u companion]", r)
                assert ok, (where, r)
                assert torch.equal(_bits(dres_c.t), _bits(dres.t.to(dt))), where
                for row, name, b in ((0, "dgamma", bdg), (1, "dbeta", bdb)):
                    if which in ("both", name):
                        assert dgb.sentinels(dgb.t[row]) == 0, (where, name)
                        ok, r = R.within(dgb.t[row], ref[name], b)
                        _note(f"layernorm_backward {name} {kind}", r)
                        assert ok, (where, name, r)
                    else:
                        assert dgb.sentinels(dgb.t[row]) == C, (where, name)
                # the same bits whatever the pitch of dy and whichever column sums are asked for
                for key, t in (("dres", dres.t), ("dgamma", dgb.t[0]), ("dbeta", dgb.t[1])):
                    if key != "dres" and which not in ("both", key):
                        continue
                    keep = first.setdefault((key, accumulate), _bits(t).clone())
                    assert torch.equal(_bits(t), keep), (where, key)
    print(f"d/bound layernorm backward {(rows, C)} {kind} {_tag(dt)}: "
          + ", ".join(f"{k.split()[1]} {v:.3g}" for k, v in sorted(_WORST.items()) if k.startswith("layernorm")))


# ---- GELU ---------------------------------------------------------------------------------------------------------
GELU_WRAP = 4 * 256 * 8192 + 4 * 256 + 3       # the second sweep of the grid-stride loop, and a scalar tail


@functools.lru_cache(maxsize=1)
def _gelu_case(n):
    x, g = R.gelu_inputs(n, 5 + n)
    return x, g, R.gelu(x), R.gelu(x, g)


@pytest.mark.parametrize("n,dt", [(n, dt) for n in (0, 1, 3, 4, 5, 4099, GELU_WRAP) for dt in DTYPES])
def test_gelu_elementwise(ops, n, dt):
    x, g, (want_y, by), (want_g, bg) = _gelu_case(n)
    x_d, g_d = x.cuda(), g.cuda()
    y, dx = Guarded((n,), dt), Guarded((n,), dt)
    ops.gelu_forward(x_d, y.t)
    ops.gelu_backward(x_d, g_d, dx.t)
    torch.cuda.synchronize()
    assert y.guards_intact() and dx.guards_intact()
    assert y.sentinels() == 0 and dx.sentinels() == 0
    if dt == torch.bfloat16:      # the f32 value inside its bound, rounded once
        by = by * (1 + R.U_BF16) + R.U_BF16 * want_y.abs()
        bg = bg * (1 + R.U_BF16) + R.U_BF16 * want_g.abs()
    ok_y, r_y = R.within(y.t, want_y, by)
    ok_g, r_g = R.within(dx.t, want_g, bg)
    _note(f"gelu_forward {_tag(dt)}", r_y)
    _note(f"gelu_backward {_tag(dt)}", r_g)
    print(f"d/bound gelu n {n} {_tag(dt)}: forward {r_y:.3g}, backward {r_g:.3g}")
    assert ok_y and ok_g, (r_y, r_g)


# ---- rows_period_sum ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C", [(1, 1, 1), (7, 35, 36), (2, 8192 * 4 + 1, 64)])
def test_rows_period_sum_elementwise(ops, B, N, C):
    """The last shape has N C > 8192 * 256 elements: the grid-stride loop wraps."""
    x = torch.randn((B * N, C), generator=torch.Generator().manual_seed(B + N))
    out = Guarded((N, C), torch.float32)
    ops.rows_period_sum(x.cuda(), B, N, C, out.t)
    torch.cuda.synchronize()
    assert out.guards_intact() and out.sentinels() == 0
    want, bound = R.rows_period_sum(x, B, N, C)
    ok, r = R.within(out.t, want, bound)
    _note("rows_period_sum", r)
    print(f"d/bound rows_period_sum {(B, N, C)}: {r:.3g}")
    assert ok, r


# ---- argument checks: refused on the host before any launch, so the pointers are never dereferenced --------------
def test_argument_checks_refuse_before_any_launch(built_lib):
    from probpose_pytorch_amd import _lib
    L = built_lib
    a = [0x10000 * (i + 1) for i in range(6)]        # 16-byte aligned, never dereferenced
    F32, BF16, FP8 = _lib.PP_F32, _lib.PP_BF16, _lib.PP_FP8

    def attn(qkv=a[0], out=a[1], dout=a[2], dqkv=a[3], N=16, hd=32, dtype=BF16):
        return L.pp_attention_backward(qkv, out, dout, dqkv, 2, N, 2, hd, dtype, a[4], None)

    def ln(ldy=64, dtype=F32):
        return L.pp_layernorm_backward(a[0], a[1], 1e-6, 8, 64, a[2], ldy, a[3], 0, a[4], dtype, None, None, a[5], None)

    def refused(rc, name, match):
        with pytest.raises(_lib.HipExtensionError, match=match):
            _lib.check(rc, name)

    for arg in ("qkv", "out", "dout", "dqkv"):
        refused(attn(**{arg: a[0] + 0x100000 + 2}), "pp_attention_backward", "bf16 buffers must be 16-byte aligned")
    refused(attn(dtype=FP8), "pp_attention_backward", "bad dtype 2")
    refused(attn(N=0), "pp_attention_backward", "bad shape B=2 N=0 heads=2")
    refused(attn(hd=48), "pp_attention_backward", r"head_dim 48 not supported \(32, 64\)")
    refused(ln(ldy=63), "pp_layernorm_backward", "bad shape rows=8 C=64 ldy=63")
    refused(ln(dtype=FP8), "pp_layernorm_backward", "bad dtype 2")
    for x, g, out in ((a[0] + 4, a[1], a[2]), (a[0], a[1] + 4, a[2]), (a[0], a[1], a[2] + 4)):
        refused(L.pp_gelu_backward(x, g, 8, out, F32, None), "pp_gelu_backward", "buffers must be 16-byte aligned")
    refused(L.pp_gelu_forward(a[0] + 4, 8, a[1], BF16, None), "pp_gelu_forward", "buffers must be 16-byte aligned")
    refused(L.pp_gelu_forward(a[0], 8, a[1] + 4, BF16, None), "pp_gelu_forward", "buffers must be 16-byte aligned")
    refused(L.pp_gelu_forward(a[0], 8, a[1], FP8, None), "pp_gelu_forward", "bad dtype 2")
    refused(L.pp_gelu_forward(a[0], -1, a[1], F32, None), "pp_gelu_forward", "bad length -1")
    for args in ((0, 16, 2), (2, 0, 2), (2, 16, 0), (-1, 16, 2)):
        assert L.pp_attention_backward_workspace_bytes(*args) == 0
    for args in ((0, 64), (8, 0), (-3, 64)):
        assert L.pp_layernorm_backward_workspace_bytes(*args) == 0
    assert L.pp_attention_backward_workspace_bytes(2, 16, 2) == 2 * 2 * 2 * 16 * 4
