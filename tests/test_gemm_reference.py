"""CPU tests of the float64 pp_gemm restatement (tests/gemm_reference.py) and of its comparator.

(1) The restatement, driven with the tables pack.py builds and the head layers' own calls (head_calls), equals torch's own
operators (F.linear, F.conv2d with its zero padding, F.conv_transpose2d, the head-major permute, the NCHW heatmap
store).  Operands are small integers, so every product and sum is exact and equality is exact.
(2) The comparator rejects what a broken tile would leave behind: a K-tile missing from one 16x16 block, two
16-row groups swapped, a bias added twice in one column tile, a tile never written, a guard element written."""
import pytest
import torch
import torch.nn.functional as F

from probpose_pytorch_amd import head_calls, pack
from tests import gemm_reference as gr

BF16, F32 = torch.bfloat16, torch.float32


def _int(shape, seed, lo=-3, hi=4, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).to(dtype)


def _run(kw, extra=0):
    """The expected buffer of a call whose output starts NaN (extra = guard elements after it)."""
    out = kw["out"]
    before = torch.cat([gr.nan_like_bits(out.numel(), out.dtype, "cpu"), gr.nan_like_bits(extra, out.dtype, "cpu")])
    ref, written = gr.expected_output(kw, before)
    return ref, written


@pytest.mark.parametrize("epi", ["none", "gelu", "relu"])
def test_plain_linear_with_bias_equals_f_linear(epi):
    M, N, K = 37, 24, 128
    A, W = _int((M, K), 1), _int((N, K), 2)
    b = _int((N,), 3, dtype=F32)
    flag = {"none": 0, "gelu": gr.EPI_GELU, "relu": gr.EPI_RELU}[epi]
    out = torch.empty((M, N), dtype=BF16)
    ref, written = _run(dict(A=A, W=W, out=out, M=M, N=N, Kd=K, lda=K, ldw=K, ldc=N, bias=b, epilogue=flag), extra=40)
    want = F.linear(A.double(), W.double(), b.double())
    want = {"none": want, "gelu": F.gelu(want), "relu": F.relu(want)}[epi]
    torch.testing.assert_close(ref[:M * N].reshape(M, N), want, rtol=1e-15, atol=1e-12)
    assert written[:M * N].all() and not written[M * N:].any() and torch.isnan(ref[M * N:]).all()


def test_strided_output_rowbias_and_residual():
    """ldc > N: the columns beyond N keep their values; pos-embed row bias with a period; the f32 residual in place."""
    M, N, K, ldc, P = 12, 8, 64, 11, 5
    A, W = _int((M, K), 1), _int((N, K), 2)
    b, rb = _int((N,), 3, dtype=F32), _int((P, ldc), 4, dtype=F32)
    out = _int((M, ldc), 5, dtype=F32)
    ref, written = gr.expected_output(dict(A=A, W=W, out=out, M=M, N=N, Kd=K, lda=K, ldw=K, ldc=ldc, bias=b,
                                           rowbias=rb, rowbias_period=P, epilogue=gr.EPI_OUT_F32), out.reshape(-1))
    pre = A.double() @ W.double().t() + b.double()
    want = out.double().clone()
    want[:, :N] = pre + rb.double()[torch.arange(M) % P, :N]
    assert torch.equal(ref.reshape(M, ldc), want)
    assert written.reshape(M, ldc)[:, :N].all() and not written.reshape(M, ldc)[:, N:].any()
    ref, _ = gr.expected_output(dict(A=A, W=W, out=out, M=M, N=N, Kd=K, lda=K, ldw=K, ldc=ldc, bias=b, residual=out,
                                     epilogue=gr.EPI_OUT_F32), out.reshape(-1))
    want = out.double().clone()
    want[:, :N] += pre
    assert torch.equal(ref.reshape(M, ldc), want)


def test_conv3x3_gather_stage0_and_batched_branches_equal_conv2d():
    """The aux convolutions as the engine launches them: stage 0 (N = 4C, one gather over C-wide rows) and a later
    stage (4 branches as batch entries, each on its C-wide slice of 4C-wide rows), zero padding through rowoff = -1."""
    B, h, w, C = 2, 5, 4, 64
    M = B * h * w
    # stage 0
    x0 = _int((M, C), 1)
    wt0 = _int((4 * C, C, 3, 3), 2, -1, 2, F32)
    b0 = _int((4 * C,), 3, dtype=F32)
    Wp0 = pack.conv_taps_major(wt0).to(BF16)
    ro0 = pack.conv_gather_table(B, h, w, 3, 3, 1, 1, C)
    out = torch.empty((M, 4 * C), dtype=BF16)
    ref, written = _run(dict(head_calls.aux_stage0(M, C), A=x0, W=Wp0, out=out, bias=b0, rowoff=ro0))
    want = F.conv2d(x0.double().reshape(B, h, w, C).permute(0, 3, 1, 2), wt0.double(), b0.double(), padding=1)
    assert torch.equal(ref.reshape(M, 4 * C), want.permute(0, 2, 3, 1).reshape(M, 4 * C)) and written.all()
    # stage >= 1: batch = 4 branches
    x = _int((M, 4 * C), 4)
    wt = _int((4, C, C, 3, 3), 5, -1, 2, F32)
    bias = _int((4, C), 6, dtype=F32)
    Wp = torch.stack([pack.conv_taps_major(wt[i]) for i in range(4)]).to(BF16)
    ro = pack.conv_gather_table(B, h, w, 3, 3, 1, 1, 4 * C)
    ref, written = _run(dict(head_calls.aux_stage(M, C), A=x, W=Wp, out=out, bias=bias, rowoff=ro))
    ref = ref.reshape(M, 4 * C)
    for i in range(4):
        xi = x[:, i * C:(i + 1) * C].double().reshape(B, h, w, C).permute(0, 3, 1, 2)
        want = F.conv2d(xi, wt[i].double(), bias[i].double(), padding=1).permute(0, 2, 3, 1).reshape(M, C)
        assert torch.equal(ref[:, i * C:(i + 1) * C], want)
    assert written.all()
    # the padding rows really are zeros: a corner pixel sees 4 of its 9 taps
    assert int((ro[:, 0] < 0).sum()) == 5


@pytest.mark.parametrize("split", [3, 9])
def test_splitk_partials_sum_to_the_convolution(split):
    B, h, w, C = 2, 4, 3, 64
    M = B * h * w
    x = _int((M, 4 * C), 1)
    wt = _int((4, C, C, 3, 3), 2, -1, 2, F32)
    Wp = torch.stack([pack.conv_taps_major(wt[i]) for i in range(4)]).to(BF16)
    ro = pack.conv_gather_table(B, h, w, 3, 3, 1, 1, 4 * C)
    taps = 9 // split
    parts = torch.empty((split, M, 4 * C), dtype=F32)
    ref, written = _run(dict(head_calls.aux_stage(M, C, split=split), A=x, W=Wp, out=parts, rowoff=ro,
                             epilogue=gr.EPI_OUT_F32))
    assert written.all()
    ref = ref.reshape(split, M, 4 * C)
    total = ref.sum(0)
    for i in range(4):
        xi = x[:, i * C:(i + 1) * C].double().reshape(B, h, w, C).permute(0, 3, 1, 2)
        want = F.conv2d(xi, wt[i].double(), padding=1).permute(0, 2, 3, 1).reshape(M, C)
        assert torch.equal(total[:, i * C:(i + 1) * C], want)
        # partial s is the convolution restricted to taps [s * taps, (s + 1) * taps)
        for s in range(split):
            mask = torch.zeros(9)
            mask[s * taps:(s + 1) * taps] = 1
            ws = wt[i].double() * mask.double().reshape(1, 1, 3, 3)
            part = F.conv2d(xi, ws, padding=1).permute(0, 2, 3, 1).reshape(M, C)
            assert torch.equal(ref[s, :, i * C:(i + 1) * C], part)


@pytest.mark.parametrize("k", [4, 3, 2])
def test_deconv_parities_with_row_scatter_equal_conv_transpose2d(k):
    B, h, w, Cin, Cout = 2, 3, 4, 64, 16
    M = B * h * w
    x = _int((M, Cin), 1)
    wt = _int((Cin, Cout, k, k), 2, -1, 2, F32)
    bias = _int((Cout,), 3, dtype=F32)
    Wp = pack.pack_deconv_parities(wt, k).to(BF16)
    ro, rm = pack.deconv_tables(B, h, w, k, Cin)
    out = torch.empty((4 * M, Cout), dtype=BF16)
    ref, written = _run(dict(head_calls.deconv(M, Cin, Cout), A=x, W=Wp, out=out, bias=bias, rowoff=ro, out_rowmap=rm,
                             epilogue=gr.EPI_RELU))
    pad, op = pack.deconv_geometry(k)
    want = F.relu(F.conv_transpose2d(x.double().reshape(B, h, w, Cin).permute(0, 3, 1, 2), wt.double(), bias.double(),
                                     stride=2, padding=pad, output_padding=op))
    assert torch.equal(ref.reshape(4 * M, Cout), want.permute(0, 2, 3, 1).reshape(4 * M, Cout)) and written.all()


@pytest.mark.parametrize("fn,key,wrong,test,arg", [
    ("deconv", "strideRowoff", lambda v: v // 2, "test_deconv_parities_with_row_scatter_equal_conv_transpose2d", 4),
    ("aux_stage0", "Kd", lambda v: v - v // 9, "test_conv3x3_gather_stage0_and_batched_branches_equal_conv2d", None),
    ("aux_stage", "strideC", lambda v: v // 2, "test_conv3x3_gather_stage0_and_batched_branches_equal_conv2d", None),
    ("aux_stage", "strideRowoff_k", lambda v: 0, "test_splitk_partials_sum_to_the_convolution", 3),
    ("conv", "Kd", lambda v: v // 2, "test_heatmap_epilogue_is_the_nchw_store_over_temperature", True),
], ids=lambda v: v if isinstance(v, str) and not v.startswith("test_") else None)
def test_a_wrong_head_descriptor_fails_its_comparison(monkeypatch, fn, key, wrong, test, arg):
    """The cases above hold head_calls' own descriptors, so they must notice a wrong one (they are not circular)."""
    run = globals()[test]
    args = () if arg is None else (arg,)
    run(*args)
    real = getattr(head_calls, fn)

    def faulty(*a, **k):
        kw = real(*a, **k)
        return dict(kw, **{key: wrong(kw[key])}) if key in kw else kw

    monkeypatch.setattr(head_calls, fn, faulty)
    with pytest.raises(AssertionError):
        run(*args)


def test_headmajor_layout_is_the_permuted_projection():
    M, heads, hd = 20, 3, 16
    C = heads * hd
    x, W = _int((M, C), 1), _int((3 * C, C), 2)
    b = _int((3 * C,), 3, dtype=F32)
    out = torch.empty((M, 3 * C), dtype=BF16)
    kw = dict(A=x, W=W, out=out, M=M, N=3 * C, Kd=C, lda=C, ldw=C, ldc=3 * C, bias=b)
    rowmajor, _ = _run(kw)
    hmaj, written = _run(dict(kw, headmajor=(heads, hd)))
    want = rowmajor.reshape(M, 3, heads, hd).permute(1, 2, 0, 3).reshape(-1)      # [3][heads][M][hd]
    assert torch.equal(hmaj, want) and written.all()


@pytest.mark.parametrize("clamp", [True, False])
def test_heatmap_epilogue_is_the_nchw_store_over_temperature(clamp):
    B, HW, Cin, K, T = 2, 30, 64, 5, 0.5
    x, W = _int((B * HW, Cin), 1), _int((K, Cin), 2)
    b = _int((K,), 3, dtype=F32)
    out = torch.empty((B, K, HW), dtype=F32)
    ref, written = _run(dict(head_calls.conv(B * HW, Cin, K, 1), A=x, W=W, out=out, bias=b, heatmap=(K, HW, T, clamp)))
    want = ((x.double() @ W.double().t() + b.double()) / T).reshape(B, HW, K).permute(0, 2, 1)
    if clamp:
        want = want.clamp(0, 1)
    assert torch.equal(ref.reshape(B, K, HW), want) and written.all()


def test_fp8_column_scales_and_e4m3_output_scale():
    M, N, K = 16, 32, 128
    a8 = (torch.randn((M, K), generator=torch.Generator().manual_seed(1)) * 40).to(gr.FP8)
    w8 = (torch.randn((N, K), generator=torch.Generator().manual_seed(2)) * 40).to(gr.FP8)
    cs = torch.rand((N,), generator=torch.Generator().manual_seed(3)) * 1e-3
    b = torch.randn((N,), generator=torch.Generator().manual_seed(4))
    pre = (a8.double() @ w8.double().t()) * cs.double() + b.double()
    out = torch.empty((M, N), dtype=BF16)
    ref, _ = _run(dict(A=a8, W=w8, out=out, M=M, N=N, Kd=K, lda=K, ldw=K, ldc=N, bias=b, colscale=cs))
    torch.testing.assert_close(ref.reshape(M, N), pre, rtol=1e-14, atol=1e-14)
    out8 = torch.empty((M, N), dtype=gr.FP8)
    so = float(F.gelu(pre).abs().max()) / 600.0            # some values saturate
    ref, _ = _run(dict(A=a8, W=w8, out=out8, M=M, N=N, Kd=K, lda=K, ldw=K, ldc=N, bias=b, colscale=cs, out_scale=so,
                       epilogue=gr.EPI_GELU))
    want = (F.gelu(pre) / so).clamp(-448, 448)
    torch.testing.assert_close(ref.reshape(M, N), want, rtol=1e-14, atol=1e-14)
    assert float(ref.abs().max()) == 448.0


# ---------------------------------------------------------------------------------------------------------------
# the comparator rejects planted faults
# ---------------------------------------------------------------------------------------------------------------
def _faulty_case(compute, out_dtype):
    """A 128x192 output at K = 4096 with a column bias, computed exactly, then stored the way a correct kernel would."""
    M, N, K = 128, 192, 4096
    g = torch.Generator().manual_seed(7)
    A = torch.randn((M, K), generator=g).to(compute)
    W = (torch.randn((N, K), generator=g) * K ** -0.5).to(compute)
    b = torch.randn((N,), generator=g)
    out = torch.empty((M, N), dtype=out_dtype)
    epi = gr.EPI_OUT_F32 if (out_dtype == F32 and compute != F32) else 0
    kw = dict(A=A, W=W, out=out, M=M, N=N, Kd=K, lda=K, ldw=K, ldc=N, bias=b, epilogue=epi)
    guard = 4 * N
    before = torch.cat([gr.nan_like_bits(M * N, out_dtype, "cpu"), gr.nan_like_bits(guard, out_dtype, "cpu")])
    ref, written = gr.expected_output(kw, before)
    return A, W, b, before, ref, written, (M, N)


@pytest.mark.parametrize("compute,out_dtype", [(BF16, BF16), (BF16, F32), (F32, F32)])
def test_comparator_rejects_planted_faults(compute, out_dtype):
    A, W, b, before, ref, written, (M, N) = _faulty_case(compute, out_dtype)
    good = before.clone()
    good[written] = ref[written].to(out_dtype)
    v = gr.compare(good, before, ref, written, compute)
    assert v.ok, v

    def store(mat):
        t = good.clone()
        t[:M * N] = mat.reshape(-1).to(out_dtype)
        return t

    full = ref[:M * N].reshape(M, N).clone()
    faults = {}
    # one 32-deep K-tile missing from one 16x16 block
    r0, c0, k0 = 48, 96, 2048
    f = full.clone()
    f[r0:r0 + 16, c0:c0 + 16] -= A[r0:r0 + 16, k0:k0 + 32].double() @ W[c0:c0 + 16, k0:k0 + 32].double().t()
    faults["missing K-tile"] = store(f)
    # two 16-row groups swapped inside a tile
    f = full.clone()
    f[[*range(16, 32), *range(32, 48)]] = f[[*range(32, 48), *range(16, 32)]]
    faults["swapped row groups"] = store(f)
    # the bias added twice in one 96-wide column tile
    f = full.clone()
    f[:, 96:192] += b[96:192].double()
    faults["bias twice"] = store(f)
    # one 32x32 tile never written
    t = good.clone()
    t.view(-1)[:M * N].view(M, N)[64:96, 32:64] = before[:M * N].view(M, N)[64:96, 32:64]
    faults["tile unwritten"] = t
    # one guard element written
    t = good.clone()
    t[M * N + 3] = 0.0
    faults["guard written"] = t
    for name, t in faults.items():
        v = gr.compare(t, before, ref, written, compute)
        assert not v.ok, f"{name} slipped through: {v}"
    assert gr.compare(faults["guard written"], before, ref, written, compute).changed == 1
