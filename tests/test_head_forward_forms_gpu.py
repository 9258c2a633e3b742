"""The forward head kernels form by form: pp_final_heatmap / pp_final_logits (both kernels, every instantiation), patchify,
the two poolings, the aux tail, the layout transposes (csrc/pp_ops.hip) and the DARK decoder (csrc/pp_dark.hip), each
against the restatements of tests/head_forward_reference.py (pinned on the CPU by tests/test_head_forward_reference.py).

Every launch writes into a NaN-bit buffer with a guard on either side; the guards must keep their bits.

a. Final layer, exact.  Coded operands (head_forward_reference.coded_operands): the result is the same float32 in any
   summation order and names its output element, so pp_final_logits must give it bit for bit in both kernels and both
   dtypes, and pp_final_heatmap its clamp, with both clamp bounds binding.
b. Final layer, rounding.  x ~ N(0, 1), w ~ N(0, 1 / Cin), bias ~ 0.1 N, T = 0.5 against float64 within
   gemm_reference.tolerance(compute dtype, float32, rms of the unclamped float64 logits).
c. Non-finite activations, refusals; the other ops exactly (selections and copies) or within the bounds of
   tests/test_ops_gpu.py; DARK within head_forward_reference.dark_tolerance of the oracle, locations and scores equal.
"""
import numpy as np
import pytest
import torch

from oracle import probpose_oracle as orc
from tests import gemm_reference as gr
from tests import head_forward_reference as hr

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF16]
GUARD_BYTES = 256
_WORST: dict = {}
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ops(built_lib):
    assert torch.cuda.is_available()
    from probpose_pytorch_amd import ops as o
    return o


def _tag(dt):
    return str(dt).replace("torch.", "")


def _note(family, ratio):
    _WORST[family] = max(_WORST.get(family, 0.0), ratio)
    print(f"[{family}] error / bound {ratio:.3g} (worst so far {_WORST[family]:.3g})")


class Guarded:
    """numel elements of dtype inside a NaN-bit buffer, starting off_bytes past a 16-byte boundary."""

    def __init__(self, numel, dtype, off_bytes=0):
        es = torch.empty((), dtype=dtype).element_size()
        assert off_bytes % es == 0 and off_bytes < 16
        self.lead, self.numel = (GUARD_BYTES + off_bytes) // es, numel
        self.buf = gr.nan_like_bits(self.lead + numel + GUARD_BYTES // es, dtype, "cuda")
        self.fresh = self.buf.clone()
        self.out = self.buf[self.lead:self.lead + numel]
        assert self.out.data_ptr() % 16 == off_bytes

    def _bits(self, t):
        return t.view(gr._BITS[t.dtype])

    def guards_intact(self):
        torch.cuda.synchronize()
        a, b, e = self._bits(self.buf), self._bits(self.fresh), self.lead + self.numel
        return torch.equal(a[:self.lead], b[:self.lead]) and torch.equal(a[e:], b[e:])

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self._bits(self.buf), self._bits(self.fresh))


# ---------------------------------------------------------------------------------------------------------------
# final heatmap / logits
# ---------------------------------------------------------------------------------------------------------------
def _fh_launch(ops, x, w, bias, c, T, clamp):
    B, HW, Cin, K = (c[k] for k in ("B", "HW", "Cin", "K"))
    assert x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    g = Guarded(B * K * HW, F32, c["out_off"])
    ops.final_heatmap(x, w, bias, g.out, B, HW, Cin, K, T, clamp=clamp)
    assert g.guards_intact(), "the launch wrote outside its output"
    return g.out.view(B, K, HW)


FH_PARAMS = [pytest.param(c, id=hr.fh_case_id(c)) for c in hr.FH_CASES]


@pytest.mark.parametrize("c", FH_PARAMS)
def test_final_layer_coded_operands_exact(ops, c):
    B, HW, Cin, K, dt = (c[k] for k in ("B", "HW", "Cin", "K", "dtype"))
    for clamp in (False, True):
        form = hr.fh_case_form(c, clamp)
        print(f"{hr.fh_case_id(c)} clamp={clamp}: {form.name}, {form.lds} B LDS"
              + (f", {form.tiles} tiles on {form.nwaves} waves, at most {form.max_tiles} per wave" if form.mfma else ""))
        for which in ("m", "k"):
            cd = hr.coded_operands(B, HW, Cin, K, which, clamp)
            x, w, bias = cd.x.to(dt).cuda(), cd.w.to(dt).cuda(), cd.bias.cuda()
            want = hr.final_heatmap_f64(x, w, bias, B, HW, K, cd.T, clamp)
            got = _fh_launch(ops, x, w, bias, c, cd.T, clamp)
            bad = hr.bits_differ(got, want)
            assert bad == 0, f"{form.name} coding {which}: {bad} of {want.numel()} elements differ"
            if clamp and B * HW * K > 2:
                assert bool((got == 0).any()) and bool((got == 1).any()) and bool(((got > 0) & (got < 1)).any())


def _random_operands(c, seed=0):
    B, HW, Cin, K, dt = (c[k] for k in ("B", "HW", "Cin", "K", "dtype"))
    g = torch.Generator().manual_seed(1000 * seed + Cin + K)
    x = torch.randn((B * HW, Cin), generator=g).to(dt)
    w = (torch.randn((K, Cin), generator=g) * Cin ** -0.5).to(dt)
    bias = torch.randn((K,), generator=g) * 0.1
    return x, w, bias


@pytest.mark.parametrize("c", FH_PARAMS)
def test_final_layer_random_operands_against_float64(ops, c):
    B, HW, K, dt = (c[k] for k in ("B", "HW", "K", "dtype"))
    x, w, bias = (t.cuda() for t in _random_operands(c))
    logits = hr.final_heatmap_f64(x, w, bias, B, HW, K, 0.5, False)
    rms = float(logits.square().mean().sqrt())
    rtol, atol = gr.tolerance(dt, F32, rms)
    for clamp in (False, True):
        got = _fh_launch(ops, x, w, bias, c, 0.5, clamp)
        ref = torch.clamp(logits, 0.0, 1.0) if clamp else logits
        bad, ratio = hr.out_of_bound(got, ref, rtol, atol)
        form = hr.fh_case_form(c, clamp).name
        _note("final " + form.split("<")[0] + " " + _tag(dt), ratio)
        assert bad == 0, f"{form}: {bad} elements outside rtol {rtol} atol {atol:.3g} (worst ratio {ratio:.3g})"


@pytest.mark.parametrize("dt,B,HW,Cin,K,T", hr.FH_REFUSALS,
                         ids=[f"{_tag(r[0])}-B{r[1]}-HW{r[2]}-C{r[3]}-K{r[4]}-T{r[5]}" for r in hr.FH_REFUSALS])
def test_final_layer_refusals_write_nothing(ops, dt, B, HW, Cin, K, T):
    from probpose_pytorch_amd import _lib
    assert hr.final_heatmap_form(dt, B, HW, Cin, K, temperature=T) is None
    x = torch.ones((B * HW, Cin), dtype=dt, device="cuda")
    w = torch.ones((K, Cin), dtype=dt, device="cuda")
    bias = torch.ones((K,), device="cuda")
    for clamp in (True, False):
        g = Guarded(B * K * HW, F32)
        with pytest.raises(_lib.HipExtensionError):
            ops.final_heatmap(x, w, bias, g.out, B, HW, Cin, K, T, clamp=clamp)
        assert g.untouched()


@pytest.mark.parametrize("c", [pytest.param(hr._fh(BF16, 3, 48, 256, 17), id="mfma"),
                               pytest.param(hr._fh(F32, 3, 50, 36, 21), id="valu-f32"),
                               pytest.param(hr._fh(BF16, 3, 50, 40, 21), id="valu-bf16")])
def test_final_layer_non_finite_activations(ops, c):
    """One NaN and one +Inf activation: pp_final_logits gives NaN on exactly the K outputs of the NaN pixel and what
    float64 gives (+-Inf by the weight's sign) on the Inf pixel; pp_final_heatmap gives 0 for the NaN pixel
    (fminf(fmaxf(NaN, 0), 1), include/probpose_hip.h) and 1 / 0 for +-Inf.  Every other element is unaffected."""
    B, HW, Cin, K, dt = (c[k] for k in ("B", "HW", "Cin", "K", "dtype"))
    assert hr.fh_case_form(c).mfma == (dt == BF16 and HW % 16 == 0)
    x, w, bias = _random_operands(c, seed=1)
    assert bool((w != 0).all())
    m_nan, m_inf = HW + 7, 2 * HW + 21                    # crop 1 pixel 7, crop 2 pixel 21
    clean = hr.final_heatmap_f64(x, w, bias, B, HW, K, 0.5, False)
    x[m_nan, Cin // 2 + 1] = NAN
    x[m_inf, Cin - 3] = INF
    logits = hr.final_heatmap_f64(x, w, bias, B, HW, K, 0.5, False)             # CPU float64
    special = torch.zeros((B, K, HW), dtype=torch.bool)
    special[1, :, 7] = special[2, :, 21] = True
    assert bool(torch.isnan(logits[1, :, 7]).all()) and bool(torch.isinf(logits[2, :, 21]).all())
    assert torch.equal(logits[~special], clean[~special])
    rms = float(clean.square().mean().sqrt())
    rtol, atol = gr.tolerance(dt, F32, rms)
    xg, wg, bg = x.cuda(), w.cuda(), bias.cuda()
    got = _fh_launch(ops, xg, wg, bg, c, 0.5, False).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(logits))
    assert torch.equal(got[2, :, 21].double(), logits[2, :, 21])
    assert hr.out_of_bound(got[~special], logits[~special], rtol, atol)[0] == 0
    heat = _fh_launch(ops, xg, wg, bg, c, 0.5, True).cpu()
    want = hr.product_clamp(logits)
    assert not bool(torch.isnan(heat).any())
    assert torch.equal(heat[special].double(), want[special]) and bool((want[1, :, 7] == 0).all())
    assert set(want[2, :, 21].tolist()) == {0.0, 1.0}
    assert hr.out_of_bound(heat[~special], want[~special], rtol, atol)[0] == 0


# ---------------------------------------------------------------------------------------------------------------
# patchify
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("B,H,W,p", [(2, 64, 48, 16), (1, 37, 44, 8), (3, 20, 12, 4), (1, 16, 16, 16), (2, 33, 52, 16),
                                     (57, 256, 192, 16)])
def test_patchify_ragged_and_grid_stride(ops, dtype, B, H, W, p):
    if B == 57:
        assert B * 3 * H * (W // 4) > 8192 * 256                    # more items than one pass of the largest grid
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(H + W)).cuda()
    rows = B * (H // p) * (W // p)
    g = Guarded(rows * 3 * p * p, dtype)
    ops.patchify(x, g.out.view(rows, 3 * p * p), p)
    assert g.guards_intact()
    assert torch.equal(g.out.view(rows, 3 * p * p), hr.patchify_ref(x, p, dtype))


def test_patchify_refusals(ops):
    from probpose_pytorch_amd import _lib
    for W, p in ((46, 4), (48, 6)):
        x = torch.rand((1, 3, 16, W), device="cuda")
        g = Guarded(3 * 16 * W, F32)
        with pytest.raises(_lib.HipExtensionError, match="multiples of 4"):
            ops.patchify(x, g.out, p)
        assert g.untouched()


# ---------------------------------------------------------------------------------------------------------------
# max-pool + ReLU
# ---------------------------------------------------------------------------------------------------------------
def _same_with_nan(got, want):
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got.float()),
                                                                            torch.nan_to_num(want.float()))


@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("h,w,kh,kw", [(16, 12, 4, 3), (5, 5, 2, 2), (2, 2, 2, 2), (6, 6, 3, 3)])
@pytest.mark.parametrize("wide", [False, True], ids=["C=vec", "C=64"])
def test_maxpool_relu_edges(ops, dtype, h, w, kh, kw, wide):
    B = 2
    vec = 4 if dtype == F32 else 8
    C = 64 if wide else vec
    oh, ow = h // kh, w // kw
    x = torch.randn((B, h, w, C), generator=torch.Generator().manual_seed(h * w + C))
    x[0, :kh, :kw, 0] = -x[0, :kh, :kw, 0].abs() - 0.1            # an all-negative window: 0
    x[0, :kh, :kw, 1] = -INF                                       # a window of -Inf: 0
    x[0, :kh, :kw, 2] = -0.0                                       # a window of -0.0: 0
    x[1, 0, 0, 3] = -INF                                           # -Inf beside finite values: ignored
    x[1, (oh - 1) * kh + kh - 1, (ow - 1) * kw + kw - 1, C - 1] = NAN   # the last element of the last window: NaN there only
    x[1, 0, kw - 1, 0] = NAN                                       # a NaN followed by larger finite values stays
    x = x.to(dtype).reshape(B * h * w, C)
    want = hr.maxpool_relu_ref(x, B, h, w, C, kh, kw)
    assert int(torch.isnan(want).sum()) == 2 and bool((want[0, :3] == 0).all())
    g = Guarded(B * oh * ow * C, dtype)
    ops.maxpool_relu(x.cuda(), g.out, B, h, w, C, kh, kw)
    assert g.guards_intact()
    assert _same_with_nan(g.out.view(-1, C).cpu(), want)


def test_maxpool_relu_refusals(ops):
    from probpose_pytorch_amd import _lib
    for dtype, C, h, kh, pat in ((F32, 8, 2, 3, "larger than input"), (BF16, 8, 2, 3, "larger than input"),
                                 (F32, 6, 4, 2, "multiple of 4"), (BF16, 12, 4, 2, "multiple of 8")):
        x = torch.zeros((1 * h * 4, C), dtype=dtype, device="cuda")
        g = Guarded(h * 4 * C, dtype)
        with pytest.raises(_lib.HipExtensionError, match=pat):
            ops.maxpool_relu(x, g.out, 1, h, 4, C, kh, 2)
        assert g.untouched()


# ---------------------------------------------------------------------------------------------------------------
# split-K consumer
# ---------------------------------------------------------------------------------------------------------------
def _split_parts(S, n, pad, seed):
    """[S, n + pad] f32 whose padding holds NaN (shape[1] = n + pad is the split stride)."""
    big = torch.full((S, n + pad), NAN)
    big[:, :n] = torch.randn((S, n), generator=torch.Generator().manual_seed(seed))
    return big


@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("nsplit", [1, 2, 9])
@pytest.mark.parametrize("h,w,kh,kw", [(4, 4, 2, 2), (5, 7, 2, 3), (2, 2, 2, 2)])
@pytest.mark.parametrize("C,pad", [(4, 12), (4, 0), (64, 1024)])
def test_maxpool_relu_sum_is_the_sequential_sum(ops, dtype, nsplit, h, w, kh, kw, C, pad):
    """f32 additions in split order, then the bias, then the pooling (the build never contracts a * b + c): the f32
    output equals the restatement bit for bit, the bf16 output its round-to-nearest-even cast.  A padded split stride:
    the NaN padding is never read."""
    B = 3
    n = B * h * w * C
    parts = _split_parts(nsplit, n, pad, seed=nsplit * 100 + h * w + C)
    bias = torch.randn((C,), generator=torch.Generator().manual_seed(C)) - nsplit ** 0.5    # the ReLU binds on about half
    want = hr.maxpool_relu_sum_ref(parts, bias, B, h, w, C, kh, kw, dtype)
    assert not bool(torch.isnan(want).any()) and bool((want == 0).any()) and bool((want > 0).any())
    g = Guarded(want.numel(), dtype)
    pg = parts.cuda()
    assert pg.stride(0) == n + pad and pg.shape[0] == nsplit
    ops.maxpool_relu_sum(pg, bias.cuda(), g.out, B, h, w, C, kh, kw)
    assert g.guards_intact()
    assert torch.equal(g.out.view(-1, C).cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
def test_maxpool_relu_sum_nan_partial(ops, dtype):
    B, h, w, C, kh, kw, S = 2, 4, 4, 8, 2, 2, 3
    n = B * h * w * C
    parts = _split_parts(S, n, 8, seed=5)
    parts[1, ((1 * h + 3) * w + 2) * C + 5] = NAN                   # crop 1, pixel (3, 2), channel 5 -> window (1, 1)
    bias = torch.zeros((C,))
    want = hr.maxpool_relu_sum_ref(parts, bias, B, h, w, C, kh, kw, dtype)
    nan_at = torch.zeros((B, 2, 2, C), dtype=torch.bool)
    nan_at[1, 1, 1, 5] = True
    assert torch.equal(torch.isnan(want).reshape(B, 2, 2, C), nan_at)
    g = Guarded(want.numel(), dtype)
    ops.maxpool_relu_sum(parts.cuda(), bias.cuda(), g.out, B, h, w, C, kh, kw)
    assert g.guards_intact() and _same_with_nan(g.out.view(-1, C).cpu(), want)


# ---------------------------------------------------------------------------------------------------------------
# aux tail
# ---------------------------------------------------------------------------------------------------------------
AUX_SHAPES = [(1, 8, 1), (5, 64, 17), (3, 100, 133), (2, 1280, 17)]


def _aux_launch(ops, x, w, bias, B, C, K, dtype):
    g = Guarded(4 * B * K, F32)
    ops.aux_tail(x.to(dtype).cuda(), w.to(dtype).cuda(), bias.cuda(), g.out, B, C, K)
    assert g.guards_intact()
    return g.out.view(4, B, K).cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("B,C,K", AUX_SHAPES)
def test_aux_tail_coded_placement(ops, dtype, B, C, K):
    """Pre-activations exact in float32 that name (branch, crop, map): the ReLU branch is exact, a sigmoid branch lies
    within 1e-5 of float64 while neighbouring codes are more than 1e-4 apart."""
    x, w, bias = hr.aux_coded(B, C, K)
    want = hr.aux_tail_ref(x.to(dtype), w.to(dtype), bias)
    got = _aux_launch(ops, x, w, bias, B, C, K, dtype)
    assert torch.equal(got[3].double(), want[3])
    bad, ratio = hr.out_of_bound(got[:3], want[:3], 1e-5, 1e-5)
    _note("aux_tail", ratio)
    assert bad == 0
    assert bool((got[:3] > 0).all()) and bool((got[:3] < 1).all())                  # branch 3 is the only ReLU
    if B * K > 2:
        assert bool((got[3] == 0).any()) and bool((got[3] >= 1).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("B,C,K", AUX_SHAPES)
def test_aux_tail_random(ops, dtype, B, C, K):
    g = torch.Generator().manual_seed(B * C + K)
    x = torch.randn((B, 4 * C), generator=g).to(dtype)
    w = (torch.randn((4, K, C), generator=g) * C ** -0.5).to(dtype)
    bias = torch.randn((4, K), generator=g)
    got = _aux_launch(ops, x, w, bias, B, C, K, dtype)
    bad, ratio = hr.out_of_bound(got, hr.aux_tail_ref(x, w, bias), 1e-5, 1e-5)
    _note("aux_tail", ratio)
    assert bad == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
def test_aux_tail_saturation_and_nan(ops, dtype):
    B, C, K = 2, 8, 3
    x = torch.full((B, 4 * C), 0.5)
    w = torch.zeros((4, K, C))
    bias = torch.tensor([[100.0, -100.0, 0.0]] * 4)
    got = _aux_launch(ops, x, w, bias, B, C, K, dtype)
    for br in range(3):                                   # +-100 saturate the sigmoid to exactly 1 / 0, no NaN
        assert got[br].tolist() == [[1.0, 0.0, 0.5]] * B
    assert got[3].tolist() == [[100.0, 0.0, 0.0]] * B
    # a NaN feature: the sigmoid branches keep it, the ReLU branch gives 0 (fmaxf; include/probpose_hip.h)
    w[:] = 1.0
    x[0, 1 * C + 2] = NAN
    x[1, 3 * C + 5] = NAN
    got = _aux_launch(ops, x, w, torch.zeros((4, K)), B, C, K, dtype)
    want = hr.aux_tail_ref(x, w, torch.zeros((4, K)))
    assert bool(torch.isnan(got[1, 0]).all()) and bool((got[3, 1] == 0).all())
    want[3, 1] = 0.0
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert hr.out_of_bound(got[ok], want[ok], 1e-5, 1e-5)[0] == 0


# ---------------------------------------------------------------------------------------------------------------
# layout transposes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("B,R,S", [(1, 1, 1), (3, 31, 33), (2, 32, 32), (2, 65, 100), (1, 192, 7)])
def test_layout_transposes_exact(ops, dtype, B, R, S):
    t = torch.randn((B * R, S), generator=torch.Generator().manual_seed(R * S)).to(dtype).cuda()
    g = Guarded(B * S * R, F32)
    ops.tokens_to_nchw(t, g.out, B, R, S)                                  # [B, R, S] dtype -> [B, S, R] f32
    assert g.guards_intact()
    assert torch.equal(g.out.view(B, S, R), hr.tokens_to_nchw_ref(t, B, R, S))
    src = torch.randn((B, R, S), generator=torch.Generator().manual_seed(R + S)).cuda()
    g2 = Guarded(B * S * R, dtype)
    ops.nchw_to_tokens(src, g2.out, B, R, S)                               # [B, R, S] f32 -> [B, S, R] dtype
    assert g2.guards_intact()
    assert torch.equal(g2.out.view(B, S, R), hr.nchw_to_tokens_ref(src, B, R, S, dtype))


# ---------------------------------------------------------------------------------------------------------------
# DARK
# ---------------------------------------------------------------------------------------------------------------
def _dark_check(hm, ks, exact=()):
    """hm [B, K, H, W] f32 through ArgMaxProbMap.decode_device against the oracle, crop by crop.  Returns the worst
    error / tolerance over the live keypoints."""
    from probpose_pytorch_amd import ArgMaxProbMap
    B, K, H, W = hm.shape
    in_size = (4 * W, 4 * H)
    codec = ArgMaxProbMap(in_size, (W, H), blur_kernel_size=ks)
    out = codec.decode_device(torch.from_numpy(hm).cuda())
    kp, sc, locs = (out[k].cpu().numpy() for k in ("kpts", "scores", "locs"))
    kp2, sc2 = codec.decode(hm)
    np.testing.assert_array_equal(kp2, kp)
    np.testing.assert_array_equal(sc2, sc)
    worst = 0.0
    for b in range(B):
        want_kp, want_sc = orc.dark_udp_decode(hm[b], ks, in_size, (W, H))
        want_locs, _ = orc.get_heatmap_maximum(hm[b])
        np.testing.assert_array_equal(locs[b], want_locs)
        np.testing.assert_array_equal(sc[b], want_sc[0])
        tol = hr.dark_tolerance(hm[b], ks, in_size)
        d = np.abs(kp[b] - want_kp[0])
        assert np.isfinite(kp[b]).all()
        assert (d <= tol).all(), (b, d.max(), (d / np.maximum(tol, 1e-300)).max())
        live = tol > 0
        if live.any():
            worst = max(worst, float((d[live] / tol[live]).max()))
        for k in exact:
            np.testing.assert_array_equal(kp[b, k], want_kp[0, k])
    return worst


@pytest.mark.parametrize("H,W,ks", hr.DARK_CASES)
def test_dark_edges_corners_and_kernel_sizes(built_lib, H, W, ks):
    worst = _dark_check(hr.dark_blobs(H, W), ks)
    _note("dark", worst)


def test_dark_ties_negative_maps_clip_and_dead_map(built_lib):
    H, W, ks = 64, 48, 11
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    blob = lambda cx, cy, sg, a: (a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sg * sg))).astype(np.float32)  # noqa: E731
    hm = np.zeros((1, 5, H, W), np.float32)
    i = 1000
    for k, step in ((0, 256), (1, 64 + 1)):          # two equal maxima: the same thread's next pixel, another wave
        hm[0, k] = blob(24.0, 30.0, 4.0, 0.3)
        hm[0, k].reshape(-1)[[i, i + step]] = 0.9
    hm[0, 2] = -0.5                                   # a positive maximum on a negative map
    hm[0, 2, 10, 20] = 0.7
    hm[0, 3] = blob(20.3, 30.6, 3.0, 80.0)            # above 50: the upper clip binds on all seven stencil points,
    #                                                   every difference is 0 and the keypoint is the arg-max exactly
    L3 = orc.gaussian_blur_zero_padded(hm[0, 3], ks)
    y3, x3 = np.unravel_index(np.argmax(hm[0, 3]), (H, W))
    assert (L3[y3 - 1:y3 + 2, x3 - 1:x3 + 2] > 50).all()
    _note("dark", _dark_check(hm, ks, exact=(3, 4)))
    from probpose_pytorch_amd import ArgMaxProbMap
    out = ArgMaxProbMap((4 * W, 4 * H), (W, H), blur_kernel_size=ks).decode_device(torch.from_numpy(hm).cuda())
    locs = out["locs"].cpu().numpy()[0]
    assert locs[0].tolist() == [i % W, i // W] and locs[1].tolist() == [i % W, i // W]      # the first index wins
    assert locs[2].tolist() == [20, 10] and locs[4].tolist() == [-1, -1]
    assert out["kpts"].cpu().numpy()[0, 3].tolist() == [float(locs[3, 0]) / (W - 1) * (4 * W),
                                                      float(locs[3, 1]) / (H - 1) * (4 * H)]


def test_zz_report_worst_ratios():
    """Prints the worst error / bound per kernel family seen by this module's tests (run with -s or -rP)."""
    for fam in sorted(_WORST):
        print(f"worst error / bound, {fam}: {_WORST[fam]:.3g}")
    assert all(v <= 1.0 for v in _WORST.values())
