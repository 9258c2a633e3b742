"""The pp_wgrad_gemm restatement (tests/wgrad_reference.py) pinned on the CPU: fed the tables of pack.py the way
head_train.py and vit_train.py feed the kernel, it equals torch's float64 autograd weight and bias gradients of
Conv2d 3x3, ConvTranspose2d 4x4 stride 2, nn.Linear and the four batched aux convolutions; and its comparison, the one
tests/test_wgrad_gpu.py holds the kernel to, rejects each planted addressing fault."""
import pytest
import torch
import torch.nn.functional as F

from probpose_pytorch_amd import head_calls, pack
from tests import wgrad_reference as WR

F64_TOL = 1e-12        # relative to the largest gradient element: float64 sums of at most a few thousand terms


def _rows(t):
    """(B, C, h, w) -> channels-last rows [B*h*w, C]."""
    B, C, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * h * w, C).contiguous()


def _close(got, want):
    return float((got - want).abs().max()) <= F64_TOL * max(1.0, float(want.abs().max()))


def _run(kw, dW_shape, dB_shape=None, **extra):
    dW0 = torch.full((int(torch.tensor(dW_shape).prod()),), float("nan"), dtype=torch.float64)
    dB0 = None if dB_shape is None else torch.full((int(torch.tensor(dB_shape).prod()),), float("nan"),
                                                   dtype=torch.float64)
    e = WR.expected(kw, dW0, dB0, **extra)
    assert bool(e.dW_written.all()) and (dB0 is None or bool(e.dB_written.all()))
    return e.dW.view(dW_shape), (None if dB0 is None else e.dB.view(dB_shape))


def test_conv3x3_weight_and_bias_gradient():
    B, C, Co, h, w = 2, 5, 7, 6, 4
    gen = torch.Generator().manual_seed(1)
    x = torch.randn((B, C, h, w), generator=gen, dtype=torch.float64)
    wt = torch.randn((Co, C, 3, 3), generator=gen, dtype=torch.float64, requires_grad=True)
    bs = torch.randn((Co,), generator=gen, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((B, Co, h, w), generator=gen, dtype=torch.float64)
    gw, gb = torch.autograd.grad(F.conv2d(x, wt, bs, padding=1), (wt, bs), dy)
    ro = pack.conv_gather_table(B, h, w, 3, 3, 1, 1, C)
    assert int((ro < 0).sum()) > 0
    kw = dict(head_calls.wgrad_of(head_calls.conv(B * h * w, C, Co, 3)), dY=_rows(dy), A=_rows(x), rowoff=ro)
    dW, dB = _run(kw, (Co, 9 * C), (Co,))
    assert _close(dW.view(Co, 3, 3, C).permute(0, 3, 1, 2), gw) and _close(dB, gb)
    # the gathered operand is pack.gather_rows' (the forward GEMM's A)
    _, A = WR.operands(kw, 0, 0, B * h * w, "cpu")
    assert torch.equal(A, pack.gather_rows(_rows(x), ro, C))


def test_deconv4x4_weight_gradient_through_the_parity_scatter():
    B, ci, co, h, w = 2, 3, 5, 4, 3
    gen = torch.Generator().manual_seed(2)
    x = torch.randn((B, ci, h, w), generator=gen, dtype=torch.float64)
    wt = torch.randn((ci, co, 4, 4), generator=gen, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((B, co, 2 * h, 2 * w), generator=gen, dtype=torch.float64)
    (gw,) = torch.autograd.grad(F.conv_transpose2d(x, wt, stride=2, padding=1), (wt,), dy)
    M = B * h * w
    ro, rm = pack.deconv_tables(B, h, w, 4, ci)
    kw = dict(head_calls.wgrad_of(head_calls.deconv(M, ci, co)), dY=_rows(dy), A=_rows(x), rowoff=ro, dy_rowmap=rm)
    dwp, _ = _run(kw, (4, co, 4 * ci))
    assert _close(pack.unpack_deconv_parities(dwp), gw)                  # head_train.py's scatter


def test_linear_plain_form():
    M, n_in, n_out = 37, 11, 6
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((M, n_in), generator=gen, dtype=torch.float64)
    wt = torch.randn((n_out, n_in), generator=gen, dtype=torch.float64, requires_grad=True)
    bs = torch.randn((n_out,), generator=gen, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((M, n_out), generator=gen, dtype=torch.float64)
    gw, gb = torch.autograd.grad(F.linear(x, wt, bs), (wt, bs), dy)
    dW, dB = _run(dict(dY=dy, A=x, M=M, N=n_out, Kd=n_in, ldd=n_out, lda=n_in), (n_out, n_in), (n_out,))
    assert _close(dW, gw) and _close(dB, gb)
    # pitches: ldd, lda and lddw wider than the rows
    dyp = torch.full((M, n_out + 3), 7.0, dtype=torch.float64)
    dyp[:, :n_out] = dy
    xp = torch.full((M, n_in + 5), -3.0, dtype=torch.float64)
    xp[:, :n_in] = x
    kw = dict(dY=dyp, A=xp, M=M, N=n_out, Kd=n_in, ldd=n_out + 3, lda=n_in + 5, lddw=n_in + 2)
    e = WR.expected(kw, torch.full((n_out * (n_in + 2),), float("nan"), dtype=torch.float64))
    got = e.dW.view(n_out, n_in + 2)
    assert _close(got[:, :n_in], gw) and bool(got[:, n_in:].isnan().all())
    assert torch.equal(e.dW_written.view(n_out, n_in + 2)[:, n_in:], torch.zeros((n_out, 2), dtype=torch.bool))


def test_batched_aux_form_equals_four_convolutions():
    """head_train.py's later aux stages: dY and A are column blocks of [M, 4C] rows (strideDY = strideA = C), one
    gather table for all four, dW [4, C, 9C]."""
    B, C, h, w = 2, 4, 3, 5
    M = B * h * w
    gen = torch.Generator().manual_seed(4)
    x = torch.randn((B, 4 * C, h, w), generator=gen, dtype=torch.float64)
    dy = torch.randn((B, 4 * C, h, w), generator=gen, dtype=torch.float64)
    ro = pack.conv_gather_table(B, h, w, 3, 3, 1, 1, 4 * C)
    for b0, b1 in ((0, 4), (1, 3)):
        kw = dict(head_calls.wgrad_of(head_calls.aux_stage(M, C, b1 - b0)), dY=_rows(dy)[:, b0 * C:],
                  A=_rows(x)[:, b0 * C:], rowoff=ro)
        dW, dB = _run(kw, (b1 - b0, C, 9 * C), (b1 - b0, C))
        for br in range(b0, b1):
            wt = torch.zeros((C, C, 3, 3), dtype=torch.float64, requires_grad=True)
            bs = torch.zeros((C,), dtype=torch.float64, requires_grad=True)
            sl = slice(br * C, (br + 1) * C)
            gw, gb = torch.autograd.grad(F.conv2d(x[:, sl], wt, bs, padding=1), (wt, bs), dy[:, sl])
            assert _close(dW[br - b0].view(C, 3, 3, C).permute(0, 3, 1, 2), gw) and _close(dB[br - b0], gb)


def _fault_case(ints):
    """A batched, gathered, row-mapped call with a bias whose every addressing field matters."""
    M, N, seg, segs, batch, R, RY = 45, 9, 6, 5, 2, 30, 96
    gen = torch.Generator().manual_seed(11)
    draw = (lambda s: torch.randint(-4, 5, s, generator=gen).double()) if ints else \
        (lambda s: torch.randn(s, generator=gen, dtype=torch.float64).float().double())
    rs = seg + 2
    A = draw((batch * R * rs + 8,))
    dY = draw((batch * RY * (N + 1),))
    ro = torch.randint(0, R, (batch, segs, M), generator=gen) * rs + torch.randint(0, 3, (batch, segs, M), generator=gen)
    ro = torch.where(torch.rand((batch, segs, M), generator=gen) < 0.2, torch.full_like(ro, -1), ro).to(torch.int32)
    rm = torch.stack([torch.randperm(RY, generator=gen)[:M] for _ in range(batch)]).to(torch.int32)
    return dict(dY=dY, A=A, M=M, N=N, Kd=seg * segs, ldd=N + 1, rowoff=ro, seg_len=seg, dy_rowmap=rm, batch=batch,
                strideDY=RY * (N + 1), strideA=R * rs, strideRowoff=segs * M, strideRowmap=M, strideDW=N * seg * segs + 5,
                strideDB=N + 2, lddw=seg * segs)


@pytest.mark.parametrize("ints", [True, False], ids=["exact", "rounding"])
def test_comparison_rejects_planted_faults(ints):
    kw = _fault_case(ints)
    nW = kw["strideDW"] * kw["batch"] + 16
    nB = kw["strideDB"] * kw["batch"] + 16
    dW0, dB0 = WR.nan_like_bits(nW, torch.float32, "cpu"), WR.nan_like_bits(nB, torch.float32, "cpu")
    right = WR.expected(kw, dW0, dB0)
    n = WR.roundings(kw["M"], 1, torch.float32)

    def verdicts(e):
        # what a kernel computing e would leave: its float64 result rounded once to f32, the rest untouched
        gW = torch.where(e.dW_written, e.dW.float(), dW0)
        gB = torch.where(e.dB_written, e.dB.float(), dB0)
        return (WR.compare(gW, dW0, right.dW, right.dW_written, right.S, n, exact=ints),
                WR.compare(gB, dB0, right.dB, right.dB_written, right.Sb, n, exact=ints))

    vW, vB = verdicts(right)
    assert vW.ok and vB.ok, (str(vW), str(vB))
    assert vW.ratio <= 1.0 / n + 1e-9 and vB.ratio <= 1.0 / n + 1e-9        # one rounding: u |sum| <= u S
    for fault in WR.FAULTS:
        vW, vB = verdicts(WR.expected(kw, dW0, dB0, fault=fault))
        print(f"{fault}: dW {vW}; dB {vB}")
        if fault == "bias_over_slab":
            assert vW.ok and not vB.ok, fault
        elif fault in ("drop_last_row", "rowmap_ignored"):
            assert not vW.ok and not vB.ok, fault
        else:
            assert not vW.ok and vB.ok, fault
    # a write outside the call's elements is a failure of its own
    gW = torch.where(right.dW_written, right.dW.float(), dW0)
    hole = int((~right.dW_written).nonzero()[0])
    gW[hole] = 0.0
    assert not WR.compare(gW, dW0, right.dW, right.dW_written, right.S, n).ok


def test_split_and_rounding_count():
    assert WR.split_of(0, 64, 64, 1) == 1 and WR.split_of(3 * 2 * (64 * 64 + 64), 64, 64, 2) == 3
    assert WR.roundings(1, 1, torch.bfloat16) == 1 and WR.roundings(1, 1, torch.float32) == 2
    assert WR.roundings(40000, 64, torch.bfloat16) == 640 + 63
    assert WR.roundings(1025, 3, torch.float32) == 352 + 2 + 1
