"""CPU checks of tests/head_forward_reference.py: the final-heatmap case list reaches every kernel form, the coded
operands are exact and identify their output element, the comparator rejects planted kernel faults on them, the DARK
bound stays below a quarter of an input pixel on its case list, and the Sparsemax restatement gives NaN rows."""
import numpy as np
import pytest
import torch

from oracle import probpose_oracle as orc
from tests import head_forward_reference as hr

BF16, F32 = hr.BF16, hr.F32


# ---------------------------------------------------------------------------------------------------------------
# case coverage
# ---------------------------------------------------------------------------------------------------------------
def test_final_heatmap_cases_reach_every_form():
    forms = {clamp: [hr.fh_case_form(c, clamp) for c in hr.FH_CASES] for clamp in (True, False)}
    assert all(f is not None for fs in forms.values() for f in fs)               # no case is a refusal
    assert {f.name for fs in forms.values() for f in fs} == set(hr.FH_FORMS)     # all 10 instantiations
    fs = forms[True]
    mf = [(c, f) for c, f in zip(hr.FH_CASES, fs) if f.mfma]
    for NT, lo, hi in ((2, 1, 32), (4, 33, 64), (9, 65, 144)):                   # every NT at both ends of its K range
        ks = {c["K"] for c, f in mf if f.name.startswith(f"final_heatmap_mfma_kernel<{NT},")}
        assert lo in ks and hi in ks, (NT, sorted(ks))
    counts = set().union(*[f.tiles_per_wave() for _, f in mf])
    assert {0, 1, 2, 3} <= counts                                                # idle waves and 1, 2, 3 tiles
    assert {1, 2} <= hr.fh_case_form(hr._fh(BF16, 11, 3072, 256, 17)).tiles_per_wave()
    assert {2, 3} == hr.fh_case_form(hr._fh(BF16, 1367, 48, 32, 17)).tiles_per_wave()
    assert {c["Cin"] // 32 for c, _ in mf} >= {1, 16}                            # ks = 1 and ks = FHM_MAXKS
    assert any(f.lds > 64 * 1024 for _, f in mf)                                 # both opt-ins to more than 64 KB
    assert any(f.lds > 64 * 1024 for c, f in zip(hr.FH_CASES, fs) if not f.mfma and c["dtype"] == F32)
    assert any(f.lds > 64 * 1024 for c, f in zip(hr.FH_CASES, fs) if not f.mfma and c["dtype"] == BF16)
    assert hr.final_heatmap_form(BF16, 2, 48, 512, 144).lds == 149760
    assert hr.final_heatmap_form(F32, 2, 50, 256, 60).lds == 128000
    # the VALU form: one and two k passes, every row tail, one chunk per row, HW = 1
    valu = [c for c, f in zip(hr.FH_CASES, fs) if not f.mfma]
    for dt in (F32, BF16):
        assert {20, 21, 24, 41} <= {c["K"] for c in valu if c["dtype"] == dt}
        assert {1, 63, 64, 65, 129} <= {c["B"] * c["HW"] for c in valu if c["dtype"] == dt}
        assert any(c["HW"] == 1 and c["B"] > 64 for c in valu if c["dtype"] == dt)
        assert any(c["Cin"] == 16 // (2 if dt == BF16 else 4) for c in valu if c["dtype"] == dt)
    # each fall-back from the matrix-core form is a bf16 case that misses exactly one of its conditions
    fb = [c for c in valu if c["note"].startswith("fall-back")]
    why = [(c["K"] > 144, c["Cin"] > 512, c["HW"] % 16 != 0, c["Cin"] % 32 != 0, c["out_off"] % 16 != 0) for c in fb]
    assert all(c["dtype"] == BF16 for c in fb) and all(sum(w) == 1 for w in why)
    assert [any(w[i] for w in why) for i in range(5)] == [True] * 5
    # both alignment fall-backs of the dispatch (x / w are never moved on the GPU: the VALU form loads 16 B from them)
    al = hr._fh(BF16, 3, 48, 256, 17)
    assert hr.fh_case_form(al).mfma and not hr.fh_case_form(dict(al, out_off=4)).mfma
    assert not hr.final_heatmap_form(BF16, 3, 48, 256, 17, x_mod16=8).mfma
    assert not hr.final_heatmap_form(BF16, 3, 48, 256, 17, w_mod16=8).mfma


def test_final_heatmap_refusals_are_refusals():
    for dt, B, HW, Cin, K, T in hr.FH_REFUSALS:
        assert hr.final_heatmap_form(dt, B, HW, Cin, K, temperature=T) is None
    assert hr.final_heatmap_form(F32, 1, 64, 256, 133) is None and hr.final_heatmap_form(BF16, 1, 64, 256, 133)


# ---------------------------------------------------------------------------------------------------------------
# coded operands
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hr.FH_CASES, ids=hr.fh_case_id)
def test_coded_operands_are_exact_and_identify_the_element(case):
    B, HW, Cin, K = (case[k] for k in ("B", "HW", "Cin", "K"))
    for which in ("m", "k"):
        for clamp in (False, True):
            cd = hr.coded_operands(B, HW, Cin, K, which, clamp)
            for t in (cd.x, cd.w):
                assert torch.equal(t.to(BF16).float(), t)                           # exact in bf16
            assert cd.abs_sum < 2 ** 24 and np.log2(cd.T) == int(np.log2(cd.T))
            assert len(set(cd.bias.tolist())) == K                                  # distinct per k (f32 by dtype)
            v = hr.final_heatmap_f64(cd.x, cd.w, cd.bias, B, HW, K, cd.T, False)
            assert torch.equal(v.float().double(), v)                               # exact in f32
            if not clamp:
                u = v.reshape(-1)
                if which == "m":
                    assert u.unique().numel() == u.numel()                          # names (m, k)
                else:                                                               # names (k, m mod 256)
                    assert u.unique().numel() == K * min(B * HW, 256)
                    assert v[:, :, :].permute(1, 0, 2).reshape(K, -1).unique(dim=0).shape[0] == K
            elif B * HW * K > 2:
                assert float(v.min()) >= -0.5 and float(v.max()) <= 2.5
                assert bool((v < 0).any()) and bool((v > 1).any()) and bool(((v > 0) & (v < 1)).any())


# ---------------------------------------------------------------------------------------------------------------
# planted faults: each is what a wrong kernel would leave in the output buffer, and the comparator must see it
# ---------------------------------------------------------------------------------------------------------------
def _expected(case, which, clamp=False):
    B, HW, Cin, K = (case[k] for k in ("B", "HW", "Cin", "K"))
    cd = hr.coded_operands(B, HW, Cin, K, which, clamp)
    return cd, hr.final_heatmap_f64(cd.x, cd.w, cd.bias, B, HW, K, cd.T, clamp)


def _rows(v):            # [B, K, HW] -> [M, K]
    B, K, HW = v.shape
    return v.permute(0, 2, 1).reshape(B * HW, K)


def _maps(r, B, HW):     # [M, K] -> [B, K, HW]
    return r.reshape(B, HW, -1).permute(0, 2, 1).contiguous()


def test_planted_faults_are_rejected():
    nan = float("nan")
    big = hr._fh(BF16, 1367, 48, 32, 17)
    form = hr.fh_case_form(big)
    cd, want = _expected(big, "m")
    assert hr.bits_differ(want.float(), want) == 0
    # the second tile of a wave computed from the first tile's rows (cur = nxt lost)
    r = _rows(want).clone()
    n = form.nwaves * 16
    r[n:2 * n] = r[:n]
    assert hr.bits_differ(_maps(r, 1367, 48).float(), want) == n * 17
    # the crop index taken from the wrong tile: the last tile of every crop lands in the next crop
    bad = want.clone()
    bad[1:, :, 32:] = want[:-1, :, 32:]
    bad[0, :, 32:] = nan
    assert hr.bits_differ(bad.float(), want) == 1367 * 17 * 16
    # the four pixels of a float4 store rotated
    bad = want.reshape(1367, 17, 12, 4).roll(1, dims=-1).reshape(want.shape)
    assert hr.bits_differ(bad.float(), want) == want.numel()
    # the bias of map k + 1 added: seen by both codings
    for which in ("m", "k"):
        for clamp in (False, True):
            cd, w2 = _expected(hr._fh(BF16, 3, 48, 256, 17), which, clamp)
            shifted = hr.final_heatmap_f64(cd.x, cd.w, torch.roll(cd.bias, -1), 3, 48, 17, cd.T, clamp)
            assert hr.bits_differ(shifted.float(), w2) > 0
    # the weights of map k + 1 used: only the "k" coding carries k in the weights
    cd, w2 = _expected(hr._fh(BF16, 3, 48, 256, 17), "k")
    assert hr.bits_differ(hr.final_heatmap_f64(cd.x, torch.roll(cd.w, -1, 0), cd.bias, 3, 48, 17, cd.T, False).float(), w2) > 0
    # maps n >= 32 dropped (NT too small): those elements keep the buffer's NaN
    c4 = hr._fh(BF16, 3, 48, 64, 48)
    _, w4 = _expected(c4, "m")
    bad = w4.clone()
    bad[:, 32:] = nan
    assert hr.bits_differ(bad.float(), w4) == 3 * 16 * 48
    # the second k pass of the VALU form dropped
    for dt, Cin in ((F32, 36), (BF16, 40)):
        _, wv = _expected(hr._fh(dt, 3, 50, Cin, 21), "k")
        bad = wv.clone()
        bad[:, 20:] = nan
        assert hr.bits_differ(bad.float(), wv) == 3 * 50
    # a dropped 8-column chunk of the contraction changes every value
    cd, w2 = _expected(hr._fh(BF16, 3, 48, 256, 17), "m")
    x2 = cd.x.clone()
    x2[:, 8:16] = 0
    assert hr.bits_differ(hr.final_heatmap_f64(x2, cd.w, cd.bias, 3, 48, 17, cd.T, False).float(), w2) == w2.numel()
    # the toleranced comparator counts a NaN and an error just above the bound
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    assert hr.out_of_bound(ref.float(), ref, 1e-4, 1e-6)[0] == 0
    assert hr.out_of_bound(torch.tensor([1.0, nan, 0.0]), ref, 1e-4, 1e-6)[0] == 1
    assert hr.out_of_bound(torch.tensor([1.0, -2.0, 2e-6]), ref, 1e-4, 1e-6) == (1, pytest.approx(2.0, rel=1e-3))


def test_product_clamp_rule():
    v = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.25, 3.0, -1.0], dtype=torch.float64)
    assert hr.product_clamp(v).tolist() == [0.0, 1.0, 0.0, 0.25, 1.0, 0.0]
    assert torch.isnan(torch.clamp(v, 0, 1)[0])                                    # torch keeps it: the open item


# ---------------------------------------------------------------------------------------------------------------
# the other restatements
# ---------------------------------------------------------------------------------------------------------------
def test_patchify_ref_drops_partial_patches():
    x = torch.arange(1 * 3 * 9 * 12, dtype=torch.float32).reshape(1, 3, 9, 12)
    r = hr.patchify_ref(x, 4, F32)
    assert r.shape == (2 * 3, 48)
    assert r[4, 16 * 2 + 4 * 1 + 3] == x[0, 2, 4 + 1, 4 + 3]                      # patch (1, 1), c 2, py 1, px 3
    assert not bool((r == x[0, 0, 8, 0]).any())                                    # row 8 is past the last whole patch


def test_pool_refs_follow_torch():
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)
    B, h, w, C = 2, 5, 7, 4
    x = torch.randn((B * h * w, C), generator=g)
    x[3, 1] = float("nan")
    x[20, 2] = -float("inf")
    got = hr.maxpool_relu_ref(x, B, h, w, C, 2, 3)
    want = F.relu(F.max_pool2d(x.reshape(B, h, w, C).permute(0, 3, 1, 2), (2, 3))).permute(0, 2, 3, 1).reshape(-1, C)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 1
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    parts = torch.randn((3, B * h * w * C + 8), generator=g)
    parts[:, B * h * w * C:] = float("nan")                                        # padding: never read
    bias = torch.randn((C,), generator=g)
    s = hr.maxpool_relu_sum_ref(parts, bias, B, h, w, C, 2, 3, F32)
    seq = ((parts[0, :-8] + parts[1, :-8]) + parts[2, :-8]).reshape(-1, C) + bias
    assert torch.equal(s, hr.maxpool_relu_ref(seq, B, h, w, C, 2, 3)) and not torch.isnan(s).any()


@pytest.mark.parametrize("B,C,K", [(1, 8, 1), (5, 64, 17), (3, 100, 133), (2, 1280, 17)])
def test_aux_coded_names_branch_crop_and_map(B, C, K):
    x, w, bias = hr.aux_coded(B, C, K)
    assert torch.equal(x.to(BF16).float(), x) and torch.equal(w.to(BF16).float(), w)
    ref = hr.aux_tail_ref(x, w, bias)
    n = torch.arange(B * K, dtype=torch.float64).reshape(B, K) - (B * K) // 2
    for br, step in enumerate(hr.AUX_STEPS):
        pre = n * step
        assert torch.equal(ref[br], torch.relu(pre) if br == 3 else torch.sigmoid(pre))
        if br < 3 and B * K > 1:          # neighbours in a sigmoid branch are further apart than twice the 1e-5 + 1e-5 bound
            assert float(ref[br].reshape(-1).sort().values.diff().min()) > 1e-4
    # each branch reads only its own columns and weights
    for br in range(4):
        other = (br + 1) % 4
        assert not torch.equal(x[:, br * C:(br + 1) * C] @ w[other].t(), x[:, br * C:(br + 1) * C] @ w[br].t()) or B * K == 1
    if B * K > 1:
        assert len({tuple(ref[br].reshape(-1).tolist()) for br in range(4)}) == 4


# ---------------------------------------------------------------------------------------------------------------
# DARK
# ---------------------------------------------------------------------------------------------------------------
def test_dark_case_list_is_the_literal_grid():
    assert hr.DARK_CASES == [(H, W, ks) for H, W in ((2, 2), (3, 5), (8, 6), (33, 27), (64, 48)) for ks in (1, 3, 11, 31)]


@pytest.mark.parametrize("H,W,ks", hr.DARK_CASES)
def test_dark_tolerance_is_below_a_quarter_pixel(H, W, ks):
    hm = hr.dark_blobs(H, W)
    assert hm.shape == (3, 9, H, W) and hm.dtype == np.float32
    worst = 0.0
    for b in range(3):
        assert (hm[b].reshape(9, -1).max(1) > 0).all()                               # no dead keypoint
        tol = hr.dark_tolerance(hm[b], ks, (4 * W, 4 * H))
        assert tol.shape == (9, 2) and (tol > 0).all()
        worst = max(worst, float(tol.max()))
    assert worst <= 0.25, worst
    # every border of the edge clamp is met: peaks on the four corners and the four edges
    locs, _ = orc.get_heatmap_maximum(hm[0])
    assert {(int(x), int(y)) for x, y in locs[:4]} == {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}
    assert locs[4, 1] == 0 and locs[5, 1] == H - 1 and locs[6, 0] == 0 and locs[7, 0] == W - 1


def test_dark_tolerance_of_a_dead_map_is_zero():
    hm = np.zeros((2, 8, 6), np.float32)
    hm[1, 3, 3] = 0.5
    tol = hr.dark_tolerance(hm, 3, (24, 32))
    assert (tol[0] == 0).all() and (tol[1] > 0).all()


# ---------------------------------------------------------------------------------------------------------------
# Sparsemax
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3072, 1001, 7])
def test_sparsemax_restatement_gives_nan_rows(n):
    z = torch.randn((5, n), generator=torch.Generator().manual_seed(n))
    z[1, n // 3] = float("nan")
    z[2] = float("nan")
    z[3, n - 2] = float("inf")
    p = hr.sparsemax_ref(z)
    assert bool(torch.isnan(p[1:4]).all()) and not bool(torch.isnan(p[[0, 4]]).any())
    clean = orc.sparsemax_lastdim(z[[0, 4]])
    assert torch.equal(p[[0, 4]], clean)                                             # finite rows are unaffected
    # a row holding -Inf: the restatement gives NaN (0 * -Inf in the support sum), not the projection of the rest, so
    # the GPU tests feed no -Inf row
    z2 = z[[0]].clone()
    z2[0, 1] = -float("inf")
    assert bool(torch.isnan(orc.sparsemax_lastdim(z2)).any())
