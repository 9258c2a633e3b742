"""GPU tests of the kernels of csrc/pp_head_grad.hip other than the weight-gradient GEMM (tests/test_wgrad_gpu.py),
each called through ops and compared with float64 torch.  Every output lies in a NaN-bit-filled buffer with guard
elements on both sides (pitch padding included): what the call does not write keeps its bits, and a second run gives
the same bits.

Bounds are element-wise and counted from the kernels' f32 steps, u = 2^-24 (the float64 accumulations contribute
2^-50 of the magnitude sum, written out below where it matters):
* pp_bn_train_stats.  mean: the float64 mean rounded once, u |mean|.  rstd = 1 / sqrtf((float)var + eps): the
  radicand carries two roundings (halved by the square root), the root and the division one each: 3 u.  scale = gamma
  rstd: 4 u.  shift = beta - mean scale: 6 u |mean scale| + u |shift|.  Running statistics (1 - m) r + m s: 1 - m,
  both products, the rounded statistic and the sum: 4 u (|(1 - m) r| + |m s|).
* pp_bn_apply_relu, pp_bn_pool_relu: inputs for which y scale + shift is exact in f32 and in bf16: outputs and arg-max
  indices bit for bit.
* pp_bn_train_backward.  xhat = (y - mean) rstd from the f32 mean and rstd handed in: E_x = u (|mean| rstd + 3 |xhat|).
  dbeta: the float64 sum rounded once.  dgamma: sum |g| E_x + u |dgamma|.  dx = gamma rstd (g - c0 - xhat c1) with
  c0, c1 the rounded means: gamma rstd (u |c0| + u |g - c0| + E_p + u |g - c0 - xhat c1|) + 3 u |dx|,
  E_p = |c1| E_x + |xhat| E_c1 + u |xhat c1|, E_c1 = mean(|g| E_x) + u |c1|.  bf16 dx: one more rounding of the f32 dx.
* pp_aux_tail_backward.  dl = g o (1 - o) from the saved f32 output o: E_dl = u |g| (o |1 - 2 o| + 3 o (1 - o)); the
  ReLU branch's dl is exact.  A length-L f32 dot product of dl with x (or w): sum E_dl |x| + (L + 1) u sum |dl x|.
* pp_heat_clamp: one exact-in-float64 product rounded once: bit for bit.  pp_heat_tail_backward: the masks are taken
  on values where f32 and float64 agree (scale a power of two); gz = (g scale - mean) / T with the float64 mean
  rounded once: u |mean| / T + 2 u |gz| (no Sparsemax: u |gz|).  bf16 dz: one more rounding.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import head_grad_reference as HR
from tests.gemm_reference import nan_like_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
U_BF16 = 2.0 ** -8
TINY = 2.0 ** -50
GUARD = 64
DTYPES = [torch.float32, torch.bfloat16]
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32}
_WORST: dict = {}


@pytest.fixture
def ops(built_lib):
    assert torch.cuda.is_available()
    from probpose_pytorch_amd import ops as o
    return o


def _tag(dt):
    return str(dt).replace("torch.", "")


def _note(cls, r):
    _WORST[cls] = max(_WORST.get(cls, 0.0), float(r))


class Out:
    """A [rows, cols] output of row pitch `pitch` inside a NaN-bit-filled buffer with guards."""

    def __init__(self, rows, cols, dtype=torch.float32, pitch=None):
        pitch = pitch or cols
        fdt = torch.float32 if dtype == torch.int32 else dtype
        self.buf = nan_like_bits(2 * GUARD + rows * pitch, fdt, "cuda").view(dtype)
        self.before = self.buf.clone()
        self.t = self.buf[GUARD:GUARD + rows * pitch].view(rows, pitch)[:, :cols]
        self.written = torch.zeros(self.buf.shape, dtype=torch.bool, device="cuda")
        self.written[GUARD:GUARD + rows * pitch].view(rows, pitch)[:, :cols] = True

    def untouched(self):
        b = _BITS[self.buf.dtype]
        return bool(((self.buf.view(b) == self.before.view(b)) | self.written).all())

    def bits(self):
        return self.buf.view(_BITS[self.buf.dtype]).clone()


def _vec(n, dtype=torch.float32):
    return Out(1, n, dtype)


def _within(got, want, bound, cls):
    """Element-wise |got - want| <= bound; a NaN never passes.  Records the worst ratio."""
    d = (got.double().cpu() - want.double().cpu()).abs()
    bound = bound.double().cpu()
    ok = d <= bound
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    _note(cls, r.max())
    return bool(ok.all()), float(r.max())


def _same_bits(got, want):
    b = _BITS[got.dtype]
    return torch.equal(got.contiguous().view(b).cpu(), want.to(got.dtype).contiguous().view(b).cpu())


# ---------------------------------------------------------------------------------------------------------------
# pp_bn_train_stats
# ---------------------------------------------------------------------------------------------------------------
STATS = [(2, 1, 0), (2, 3072, 0), (2047, 63, 0), (2048, 64, 0), (2049, 65, 0), (2049, 3072, 0), (2049, 65, 3),
         (600000, 1, 0), (600000, 65, 0), (600000, 64, 8)]


def _stats_run(ops, y, M, Cc, gamma, beta, eps, mom, rm, rv):
    st = [_vec(Cc) for _ in range(4)]
    ws = torch.empty(ops.bn_workspace_bytes(M, Cc), dtype=torch.uint8, device="cuda")
    ops.bn_train_stats(y, M, Cc, gamma, beta, eps, mom, rm, rv, *[s.t[0] for s in st], ws)
    torch.cuda.synchronize()
    return st


def _stats_check(ops, y, M, Cc, affine, track, mom, cls):
    gen = torch.Generator().manual_seed(M + Cc)
    eps = 1e-5
    gamma = (0.5 + torch.rand(Cc, generator=gen)).cuda() if affine else None
    beta = torch.randn(Cc, generator=gen).cuda() if affine else None
    rm0 = torch.randn(Cc, generator=gen).cuda() if track else None
    rv0 = (0.5 + torch.rand(Cc, generator=gen)).cuda() if track else None
    rm, rv = (Out(1, Cc), Out(1, Cc)) if track else (None, None)
    if track:
        rm.t[0] = rm0
        rv.t[0] = rv0
        rm.before, rv.before = rm.buf.clone(), rv.buf.clone()
    st = _stats_run(ops, y, M, Cc, gamma, beta, eps, mom, rm.t[0] if track else None, rv.t[0] if track else None)
    yd = y.double()
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    e32 = float(torch.tensor(eps, dtype=torch.float32))
    m32 = float(torch.tensor(mom, dtype=torch.float32))
    rstd = 1.0 / torch.sqrt(var + e32)
    g = gamma.double() if affine else torch.ones_like(mean)
    b = beta.double() if affine else torch.zeros_like(mean)
    scale, shift = g * rstd, b - mean * g * rstd
    fails = []
    for name, out, want, bound in (("mean", st[0], mean, U * mean.abs() + TINY * yd.abs().mean(0)),
                                   ("rstd", st[1], rstd, 3 * U * rstd),
                                   ("scale", st[2], scale, 4 * U * scale.abs()),
                                   ("shift", st[3], shift, 6 * U * (mean * scale).abs() + U * shift.abs())):
        ok, r = _within(out.t[0], want, bound * (1 + 2.0 ** -10), f"bn_train_stats {name}")
        if not (ok and out.untouched()):
            fails.append((cls, name, r, out.untouched()))
    if track:
        # torch's own running update in float64, momentum as the f32 value the kernel receives
        trm, trv = rm0.double().cpu(), rv0.double().cpu()
        F.batch_norm(yd.cpu()[:, :, None], trm, trv, None, None, True, m32, e32)
        varu = var * M / (M - 1)
        for name, out, want, r0, s in (("running_mean", rm, trm, rm0.double(), mean),
                                       ("running_var", rv, trv, rv0.double(), varu)):
            bound = 4 * U * (((1 - m32) * r0).abs() + (m32 * s).abs())
            ok, r = _within(out.t[0], want, bound * (1 + 2.0 ** -10), f"bn_train_stats {name}")
            if mom == 0.0:
                ok = ok and torch.equal(out.t[0], r0.float())
            if not (ok and out.untouched()):
                fails.append((cls, name, r, out.untouched()))
    again = _stats_run(ops, y, M, Cc, gamma, beta, eps, mom, None, None)
    for a, b2 in zip(st, again):
        if not torch.equal(a.bits(), b2.bits()):
            fails.append((cls, "second run differs"))
    return fails


@pytest.mark.parametrize("M,Cc,pad", STATS)
def test_bn_train_stats(ops, M, Cc, pad):
    gen = torch.Generator().manual_seed(7 * M + Cc)
    buf = (torch.randn((M, Cc + pad), generator=gen) * 1.5 + 0.3).cuda()
    y = buf[:, :Cc]
    fails = _stats_check(ops, y, M, Cc, True, True, 0.1, "plain")
    assert not fails, fails


def test_bn_train_stats_large_mean_absent_arguments_and_zero_momentum(ops):
    M, Cc = 5000, 65
    gen = torch.Generator().manual_seed(3)
    y = (torch.randn((M, Cc), generator=gen) + 1e4).cuda()
    fails = _stats_check(ops, y, M, Cc, True, True, 0.1, "mean 1e4")
    var = y.double().var(0, unbiased=False)
    assert float(var.min()) > 0.8 and float(var.max()) < 1.25          # the case is what it claims to be
    y2 = (torch.randn((M, Cc), generator=gen) * 2 - 1).cuda()
    fails += _stats_check(ops, y2, M, Cc, False, True, 0.1, "no gamma / beta")
    fails += _stats_check(ops, y2, M, Cc, True, False, 0.1, "no running statistics")
    fails += _stats_check(ops, y2, M, Cc, True, True, 0.0, "momentum 0")
    fails += _stats_check(ops, y2, M, Cc, True, True, 1.0, "momentum 1")
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------
# pp_bn_apply_relu, pp_bn_pool_relu: exact inputs
# ---------------------------------------------------------------------------------------------------------------
def _exact_inputs(rows, Cc, gen):
    """y multiples of 1/2 up to 3, scale in +-{1/2, 1, 2}, shift multiples of 1/2 up to 2: y scale + shift is a multiple
    of 1/4 below 8, exact in f32 and in bf16 with or without fusion, and never -0 (shift is +0 where it is 0)."""
    y = torch.randint(-6, 7, (rows, Cc), generator=gen).float() / 2
    scale = 2.0 ** torch.randint(-1, 2, (Cc,), generator=gen).float() * (1 - 2 * (torch.rand(Cc, generator=gen) < 0.25).float())
    shift = torch.randint(-4, 5, (Cc,), generator=gen).float() / 2
    return y, scale, shift


@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("M,Cc,ldy,ldo", [(1, 1, 1, 1), (37, 65, 65, 65), (300, 63, 70, 67), (1031, 256, 256, 264)])
def test_bn_apply_relu_exact(ops, M, Cc, ldy, ldo, dt):
    gen = torch.Generator().manual_seed(M + Cc)
    y0, scale, shift = _exact_inputs(M, Cc, gen)
    if M > 2:
        y0[1, 0] = float("nan")
    ybuf = torch.full((M, ldy), 99.0)
    ybuf[:, :Cc] = y0
    y = ybuf.cuda()[:, :Cc]
    z = y0.double() * scale.double() + shift.double()
    for relu in (True, False):
        out = Out(M, Cc, dt, ldo)
        ops.bn_apply_relu(y, M, Cc, scale.cuda(), shift.cuda(), out.t, relu=relu)
        torch.cuda.synchronize()
        want = torch.relu(z) if relu else z
        assert _same_bits(out.t[~want.isnan().cuda()], want[~want.isnan()].float()), (relu,)
        assert bool(out.t.isnan().cpu().eq(want.isnan()).all()) and out.untouched()
        again = Out(M, Cc, dt, ldo)
        ops.bn_apply_relu(y, M, Cc, scale.cuda(), shift.cuda(), again.t, relu=relu)
        assert torch.equal(out.bits(), again.bits())


POOLS = [(2, 8, 6, 5, 4, 3), (2, 9, 7, 64, 4, 3), (1, 7, 5, 65, 2, 2), (3, 5, 9, 3, 1, 4), (2, 6, 7, 130, 3, 2),
         (2, 4, 4, 7, 4, 4)]


def _pool_reference(z, B, h, w, Cc, kh, kw):
    """z [B*h*w, C] float64 on the CPU -> (ReLU(MaxPool(z)) [B*oh*ow, C], argmax int64 element index or -1): torch's
    CPU max_pool2d (the first maximum in scan order, a NaN winning), then the ReLU's gradient mask."""
    zn = z.view(B, h, w, Cc).permute(0, 3, 1, 2).contiguous()
    best, idx = F.max_pool2d(zn, (kh, kw), return_indices=True)
    bb = torch.arange(B).view(B, 1, 1, 1)
    cc = torch.arange(Cc).view(1, Cc, 1, 1)
    elem = (bb * h * w + idx) * Cc + cc
    passes = ~(best <= 0)
    out = torch.where(passes, best, torch.zeros_like(best))
    arg = torch.where(passes, elem, torch.full_like(elem, -1))
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Cc)  # noqa: E731
    return rows(out), rows(arg)


def _planted_pool_input(B, h, w, Cc, kh, kw, gen):
    y, scale, shift = _exact_inputs(B * h * w, Cc, gen)
    oh, ow = h // kh, w // kw
    y4 = y.view(B, h, w, Cc)
    scale[0], shift[0] = 1.0, 0.5                 # channel 0: ties planted at every window position
    for j in range(kh * kw):
        wy, wx = (j // ow) % oh, j % ow           # window j (wrapping when there are fewer windows than positions)
        blk = y4[0, wy * kh:(wy + 1) * kh, wx * kw:(wx + 1) * kw, 0]
        flat = torch.full((kh * kw,), -1.0)
        flat[j:] = 2.0                            # positions j .. end tie for the maximum: j wins
        blk.copy_(flat.view(kh, kw))
    if Cc > 1:                                    # channel 1: nothing positive anywhere -> 0 and arg-max -1
        scale[1], shift[1] = 2.0, -0.5
        y4[..., 1] = -y4[..., 1].abs()
    if Cc > 2:                                    # channel 2: a NaN in a window (then a larger value), and two NaNs
        y4[0, 0, 0, 2] = float("nan")
        y4[B - 1, kh - 1, kw - 1, 2] = float("nan")
        y4[B - 1, 0, 0, 2] = float("nan")
    return y, scale, shift


@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("B,h,w,Cc,kh,kw", POOLS)
def test_bn_pool_relu_exact(ops, B, h, w, Cc, kh, kw, dt):
    gen = torch.Generator().manual_seed(h * 100 + w * 10 + Cc)
    y, scale, shift = _planted_pool_input(B, h, w, Cc, kh, kw, gen)
    z = y.double() * scale.double() + shift.double()
    want, warg = _pool_reference(z, B, h, w, Cc, kh, kw)
    if kh * kw > 1:
        assert int((warg[:, 0] % (w * Cc) // Cc % kw + (warg[:, 0] // (w * Cc)) % h % kh * kw).max()) > 0
    if Cc > 1:
        assert bool((warg[:, 1] == -1).all())
    n = B * (h // kh) * (w // kw)
    runs = []
    for _ in range(2):
        out, arg = Out(n, Cc, dt), Out(n, Cc, torch.int32)
        ops.bn_pool_relu(y.cuda(), B, h, w, Cc, kh, kw, scale.cuda(), shift.cuda(), out.t, arg.t)
        torch.cuda.synchronize()
        runs.append((out, arg))
    out, arg = runs[0]
    assert torch.equal(arg.t.cpu().long(), warg), "arg-max indices"
    fin = ~want.isnan()
    assert bool(out.t.isnan().cpu().eq(want.isnan()).all())
    if Cc > 2:
        assert bool(want.isnan().any())
    assert _same_bits(out.t.cpu()[fin], want[fin].float())
    assert out.untouched() and arg.untouched()
    assert torch.equal(out.bits(), runs[1][0].bits()) and torch.equal(arg.bits(), runs[1][1].bits())


# ---------------------------------------------------------------------------------------------------------------
# pp_bn_train_backward
# ---------------------------------------------------------------------------------------------------------------
def _bn_backward_case(ops, mode, dt, B, h, w, Cc, kh, kw, pads, with_dgb, seed):
    M = B * h * w
    ldg_pad, ldy_pad, ldx_pad = pads
    gen = torch.Generator().manual_seed(seed)
    y0 = torch.randint(-6, 7, (M, Cc), generator=gen).float() / 2
    y0[0] += 0.25                                       # the batch mean stays off the grid of the values
    gamma = ((0.5 + torch.rand(Cc, generator=gen)) * (1 - 2 * (torch.rand(Cc, generator=gen) < 0.25).float()))
    beta = torch.randn(Cc, generator=gen) * 0.3
    eps = 1e-5
    yd = y0.double()
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    e32 = float(torch.tensor(eps, dtype=torch.float32))
    rstd = 1.0 / torch.sqrt(var + e32)
    for _ in range(32):                                 # keep every z = gamma xhat + beta clear of the ReLU's edge
        near = ((yd - mean) * rstd * gamma.double() + beta.double()).abs().min(0).values < 1e-3
        if not bool(near.any()):
            break
        beta[near] += 0.0137
    mean32, rstd32 = mean.float(), rstd.float()
    scale32 = gamma * rstd32
    shift32 = beta - mean32 * scale32
    ybuf = torch.full((M, Cc + ldy_pad), 55.0)
    ybuf[:, :Cc] = y0
    y = ybuf.cuda()[:, :Cc]
    # float64 autograd of batch_norm(training=True) [+ ReLU | + MaxPool + ReLU]
    yl = yd.clone().requires_grad_(True)
    gl, bl = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.batch_norm(yl, None, None, gl, bl, True, 0.0, e32)
    argmax = None
    if mode == 0:
        tail, grows = z, M
    elif mode == 1:
        assert float(z.detach().abs().min()) > 1e-4, "a pre-activation too close to 0 for a mask test"
        tail, grows = torch.relu(z), M
    else:
        assert float(z.detach().abs().min()) > 1e-4
        oh, ow = h // kh, w // kw
        zn = z.view(B, h, w, Cc).permute(0, 3, 1, 2)
        tail = torch.relu(F.max_pool2d(zn, (kh, kw))).permute(0, 2, 3, 1).reshape(B * oh * ow, Cc)
        grows = B * oh * ow
        _, warg = _pool_reference(z.detach(), B, h, w, Cc, kh, kw)
        pooled, arg = Out(grows, Cc, dt), Out(grows, Cc, torch.int32)
        ops.bn_pool_relu(y.contiguous(), B, h, w, Cc, kh, kw, scale32.cuda(), shift32.cuda(), pooled.t, arg.t)
        assert torch.equal(arg.t.cpu().long(), warg), "the forward's arg-max differs from torch's"
        argmax = arg.t.contiguous()
    gbuf = torch.full((grows, Cc + ldg_pad), 77.0)
    g0 = torch.randn((grows, Cc), generator=gen)
    gbuf[:, :Cc] = g0
    g = gbuf.cuda()[:, :Cc]
    dxw, dgw, dbw = torch.autograd.grad(tail, (yl, gl, bl), g0.double())
    # the gradient reaching z, for the bound's terms
    zl = z.detach().clone().requires_grad_(True)
    if mode == 0:
        t2 = zl
    elif mode == 1:
        t2 = torch.relu(zl)
    else:
        t2 = torch.relu(F.max_pool2d(zl.view(B, h, w, Cc).permute(0, 3, 1, 2), (kh, kw))).permute(0, 2, 3, 1).reshape(grows, Cc)
    (gz,) = torch.autograd.grad(t2, zl, g0.double())
    xhat = (yd - mean) * rstd
    Ex = U * (mean.abs() * rstd + 3 * xhat.abs())
    c0, c1 = gz.mean(0), (gz * xhat).mean(0)
    Ec1 = (gz.abs() * Ex).mean(0) + U * c1.abs()
    Ep = c1.abs() * Ex + xhat.abs() * Ec1 + U * (xhat * c1).abs()
    inner = gz - c0 - xhat * c1
    coef = (gamma.double() * rstd).abs()
    bdx = coef * (U * c0.abs() + U * (gz - c0).abs() + Ep + U * inner.abs()) + 3 * U * dxw.abs()
    bdg = (gz.abs() * Ex).sum(0) + U * dgw.abs() + TINY * (gz * xhat).abs().sum(0)
    bdb = U * dbw.abs() + TINY * gz.abs().sum(0)
    fails = []
    ws = torch.empty(ops.bn_workspace_bytes(M, Cc), dtype=torch.uint8, device="cuda")
    kwargs = dict(mode=mode, scale=scale32.cuda(), shift=shift32.cuda(), argmax=argmax, pool=(B, h, w, kh, kw))
    if mode == 0:
        kwargs.update(scale=None, shift=None)

    def run(dtype, dgb):
        dx = Out(M, Cc, dtype, Cc + ldx_pad)
        dg, db = (_vec(Cc), _vec(Cc)) if dgb else (None, None)
        ops.bn_train_backward(g, y, M, Cc, mean32.cuda(), rstd32.cuda(), gamma.cuda(), dx.t, ws,
                              dgamma=dg.t[0] if dgb else None, dbeta=db.t[0] if dgb else None, **kwargs)
        torch.cuda.synchronize()
        return dx, dg, db

    dx32, dg, db = run(torch.float32, True)
    cls = f"bn_train_backward mode {mode}"
    for name, out, want, bound in (("dx", dx32, dxw, bdx), ("dgamma", dg, dgw, bdg), ("dbeta", db, dbw, bdb)):
        got = out.t if name == "dx" else out.t[0]
        ok, r = _within(got, want, bound * (1 + 2.0 ** -10), f"{cls} {name}")
        if not (ok and out.untouched()):
            fails.append((name, r, out.untouched()))
    if mode == 2:       # the floor-mode remainder: no window covers these rows / columns, their upstream gradient is 0
        rem = torch.zeros((B, h, w), dtype=torch.bool)
        rem[:, (h // kh) * kh:, :] = True
        rem[:, :, (w // kw) * kw:] = True
        assert bool((gz.view(B, h, w, Cc)[rem] == 0).all())
    if dt == torch.bfloat16:
        dx16, _, _ = run(torch.bfloat16, True)
        ok, r = _within(dx16.t, dx32.t, U_BF16 * dx32.t.abs(), f"{cls} dx bf16 vs f32")
        if not (ok and dx16.untouched()):
            fails.append(("dx bf16", r, dx16.untouched()))
    again, dg2, db2 = run(torch.float32, True)
    if not (torch.equal(again.bits(), dx32.bits()) and torch.equal(dg2.bits(), dg.bits())
            and torch.equal(db2.bits(), db.bits())):
        fails.append("second run differs")
    if not with_dgb:
        alone, _, _ = run(torch.float32, False)
        if not torch.equal(alone.bits(), dx32.bits()):
            fails.append("dx differs without dgamma / dbeta")
    return fails


BWD = [(2, 8, 6, 5, 4, 3, (0, 0, 0)), (2, 9, 7, 64, 4, 3, (5, 0, 3)), (1, 7, 5, 65, 2, 2, (0, 0, 1)),
       (3, 5, 9, 3, 1, 4, (2, 0, 0)), (5, 21, 20, 130, 3, 2, (0, 0, 0))]


@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,h,w,Cc,kh,kw,pads", BWD)
def test_bn_train_backward(ops, B, h, w, Cc, kh, kw, pads, mode, dt):
    if mode != 2:
        pads = (pads[0], 4, pads[2])            # modes 0 and 1 take a pitched y as well
    fails = _bn_backward_case(ops, mode, dt, B, h, w, Cc, kh, kw, pads, with_dgb=(Cc % 2 == 0),
                              seed=Cc + 10 * mode)
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------
# pp_aux_tail_backward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("B,Cc,K", [(2, 64, 5), (7, 65, 17), (33, 384, 20), (3, 1, 133)])
def test_aux_tail_backward(ops, B, Cc, K, dt):
    gen = torch.Generator().manual_seed(B * 1000 + Cc + K)
    x = torch.randn((B, 4 * Cc), generator=gen).to(dt)
    w = (torch.randn((4, K, Cc), generator=gen) / Cc ** 0.5).to(dt)
    bias = torch.randn((4, K), generator=gen) * 0.3
    x[0, 3 * Cc:] = 0                                    # ReLU branch, crop 0: the pre-activation is the bias
    bias[3, 0] = 0.0                                     # ... exactly 0
    bias[3, 1] = -0.25                                   # ... negative: the output is exactly 0
    gout = torch.randn((4, B, K), generator=gen)
    xl = x.double().requires_grad_(True)
    wl, bl = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    pre = torch.stack([xl[:, br * Cc:(br + 1) * Cc] @ wl[br].t() + bl[br] for br in range(4)])
    o64 = torch.cat([torch.sigmoid(pre[:3]), torch.relu(pre[3:])])
    assert float(o64[3, 0, 0]) == 0.0 and float(o64[3, 0, 1]) == 0.0
    dxw, dWw, dBw = torch.autograd.grad(o64, (xl, wl, bl), gout.double())
    out32 = o64.detach().float()
    o, gd = out32.double(), gout.double()
    dl = torch.cat([gd[:3] * o[:3] * (1 - o[:3]), torch.where(o[3:] > 0, gd[3:], torch.zeros_like(gd[3:]))])
    Edl = U * gd.abs() * (o * (1 - 2 * o).abs() + 3 * o * (1 - o))
    Edl[3] = 0
    xb = x.double().view(B, 4, Cc).permute(1, 0, 2)                           # [4, B, C]
    wd = w.double()
    bW = torch.einsum("rbk,rbc->rkc", Edl, xb.abs()) + (B + 1) * U * torch.einsum("rbk,rbc->rkc", dl.abs(), xb.abs())
    bB = Edl.sum(1) + B * U * dl.abs().sum(1)
    bX = (torch.einsum("rbk,rkc->brc", Edl, wd.abs()) + (K + 1) * U * torch.einsum("rbk,rkc->brc", dl.abs(), wd.abs()))
    bX = bX.reshape(B, 4 * Cc)
    xc, wc, oc, gc = x.cuda(), w.cuda(), out32.cuda(), gout.cuda()

    def run(which):
        dW = Out(4 * K, Cc) if "W" in which else None
        dB = Out(4, K) if "B" in which else None
        dx = Out(B, 4 * Cc) if "x" in which else None
        ops.aux_tail_backward(xc, wc, oc, gc, B, Cc, K, dW.t if dW else None, dB.t if dB else None,
                              dx.t if dx else None)
        torch.cuda.synchronize()
        return dict(W=dW, B=dB, x=dx)

    full = run("WBx")
    for name, want, bound in (("W", dWw.reshape(4 * K, Cc), bW.reshape(4 * K, Cc)), ("B", dBw, bB), ("x", dxw, bX)):
        ok, r = _within(full[name].t, want, bound * (1 + 2.0 ** -10), f"aux_tail_backward d{name} {_tag(dt)}")
        assert ok and full[name].untouched(), (name, r)
    for which in ("Bx", "Wx", "WB", "WBx"):
        part = run(which)
        for name in which:
            assert torch.equal(part[name].bits(), full[name].bits()), (which, name)


# ---------------------------------------------------------------------------------------------------------------
# pp_heat_clamp, pp_heat_tail_backward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.5, 3.0])
def test_heat_clamp_bit_for_bit(ops, scale):
    gen = torch.Generator().manual_seed(1)
    p = torch.randn(70001, generator=gen) * 1.5
    p[:6] = torch.tensor([0.0, 1.0 / scale, -0.0, float("nan"), 2.0 / scale, -1.0])
    out = _vec(p.numel())
    ops.heat_clamp(p.cuda(), out.t[0], scale)
    torch.cuda.synchronize()
    want = (p.double() * scale).float().clamp(0, 1)
    assert bool(out.t[0].isnan().cpu().eq(want.isnan()).all()) and int(want.isnan().sum()) == 1
    fin = ~want.isnan()
    assert torch.equal(out.t[0].cpu()[fin], want[fin]) and out.untouched()
    again = _vec(p.numel())
    ops.heat_clamp(p.cuda(), again.t[0], scale)
    assert torch.equal(out.bits(), again.bits())


HEAT = [(hw, 17, 0) for hw in (1, 255, 256, 257, 3072)] + [(257, 20, 0), (257, 133, 0), (255, 17, 64), (3072, 20, 64),
                                                          (256, 133, 192)]


@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("HW,K,ldz", HEAT)
def test_heat_tail_backward(ops, HW, K, ldz, sparse, dt):
    B, T = 2, 1.5
    ldz = ldz or K
    scale = 1.0 if sparse else 0.5
    gen = torch.Generator().manual_seed(HW + K + sparse)
    logits = torch.randn((B * K, HW), generator=gen, dtype=torch.float64) * (4.0 if sparse else 1.5)
    if sparse:
        logits[0] = -3.0
        logits[0, HW // 2] = 9.0               # a map whose support is a single pixel: p = 1 there, at the upper bound
    vl = (logits / T).requires_grad_(True)
    if sparse:
        p64 = HR._Sparsemax.apply(vl, False)
        assert float(p64[0, HW // 2]) == 1.0 and int((p64[0] > 0).sum()) == 1
    else:
        with torch.no_grad():                  # both clamp bounds hit exactly (p scale = 0 and 1), and a NaN
            vl[1, 0], vl[1, HW - 1] = 0.0, 1.0 / scale
            if HW > 2:
                vl[1, 1] = float("nan")
        p64 = vl * 1.0
    heat = HR._Clamp01.apply(p64 * scale, False)
    g0 = torch.randn((B * K, HW), generator=gen)
    (gv,) = torch.autograd.grad(heat, vl, g0.double())
    want = gv / T                               # the gradient of the final layer's output, logits = v T
    p32 = p64.detach().float()
    if not sparse:
        assert float(want[1, 0]) == float(g0[1, 0]) * scale / T and float(want[1, HW - 1]) == float(g0[1, HW - 1]) * scale / T
        if HW > 2:
            assert float(want[1, 1]) == 0.0
    s = (p32 > 0).double()
    inside = ((p32.double() * scale >= 0) & (p32.double() * scale <= 1)).double()
    gp = g0.double() * scale * inside
    mean = (gp * s).sum(1, keepdim=True) / s.sum(1, keepdim=True).clamp_min(1)
    bound = (U * mean.abs() / T * s + 2 * U * want.abs()) if sparse else U * want.abs()
    rows = lambda t: t.view(B, K, HW).permute(0, 2, 1).reshape(B * HW, K)  # noqa: E731
    runs = []
    for _ in range(2):
        dz = Out(B * HW, ldz, dt)
        ops.heat_tail_backward(p32.cuda(), g0.cuda(), B, K, HW, scale, sparse, T, dz.t)
        torch.cuda.synchronize()
        runs.append(dz)
    dz = runs[0]
    b = rows(bound) * (1 + 2.0 ** -10)
    if dt == torch.bfloat16:
        b = b + U_BF16 * (rows(want).abs() + b)
    ok, r = _within(dz.t[:, :K], rows(want), b, f"heat_tail_backward sparse {sparse} {_tag(dt)}")
    assert ok, r
    assert bool((dz.t[:, K:].view(_BITS[dt]) == 0).all()), "columns K .. ldz - 1 must be +0"
    assert dz.untouched() and torch.equal(dz.bits(), runs[1].bits())


def test_report_worst_ratios():
    """Prints the worst d/bound per class of the tests above (run with -s)."""
    for k, v in sorted(_WORST.items()):
        print(f"worst d/bound {k}: {v:.3g}")
