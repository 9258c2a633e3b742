"""FusedAdamW on the GPU against the float64 gauge of tests/optim_reference.py.

The bound (derived in tests/optim_reference.py, u = 2^-24): after T steps
    |p - gauge| <= T (2 u max|p| + c_upd(T) u lr_max R),   c_upd(T) = 12 + inherit (T - 1),   R = max |m_hat / denom|
    |m - gauge| <= c_m T u G,   |v - gauge| <= c_v T u G^2,   G = max |g'|
    |grad_norm - gauge| <= 2 u norm
with max|p|, R, G and the norm taken from the gauge.  The 12 are the kernel's own roundings of the update term.
FusedAdamW is held to the constants counted from its kernel (OR.KERNEL: inherit 3.5, c_m 2, c_v 3: m and v are
rounded once per step); torch's float32 AdamW, and a state that torch's steps have been through, to those of a plain
float32 moving average (OR.FLOAT32: inherit 6, c_m 4, c_v 6).
"""
import copy

import numpy as np
import pytest
import torch

from tests import optim_reference as OR

pytestmark = pytest.mark.gpu

# 1 .. 4097 around the 128-bit and workgroup boundaries, 8191 .. 16385 around the chunk (8192), and train.py's own
SHAPES = [(1,), (3,), (4,), (63,), (64,), (65,), (4095,), (4096,), (4097,), (8191,), (8192,), (8193,), (16385,),
          (384, 1536), (1152, 384), (384,), (1536,), (20, 256, 1, 1)]
GROUP_OF = [1 if len(s) == 1 and s[0] in (384, 1536) else 0 for s in SHAPES]
NONE_EVERY = {2: 3, 8: 4, 13: 5}          # these tensors' gradients are None on every 3rd / 4th / 5th step


def _params(arrays, misalign=()):
    """Fresh device parameters; `misalign`: indices placed one element into a larger buffer (4-byte aligned only)."""
    ps = []
    for i, a in enumerate(arrays):
        t = torch.from_numpy(a).cuda()
        if i in misalign:
            buf = torch.zeros(t.numel() + 1, device="cuda")
            buf[1:].copy_(t.flatten())
            t = buf[1:].view(t.shape)
            assert t.data_ptr() % 16 != 0 and t.is_contiguous()
        ps.append(torch.nn.Parameter(t))
    return ps


def _groups(ps, group_of):
    return [dict(params=[p for p, k in zip(ps, group_of) if k == 0], weight_decay=0.1),
            dict(params=[p for p, k in zip(ps, group_of) if k == 1], weight_decay=0.0)]


def _set_grads(ps, row):
    for p, g in zip(ps, row):
        p.grad = None if g is None else torch.from_numpy(g).cuda()      # a fresh tensor: a new address every step


def _state(opt, ps):
    ms = [opt.state[p]["exp_avg"].cpu().numpy() if p in opt.state and opt.state[p] else None for p in ps]
    vs = [opt.state[p]["exp_avg_sq"].cpu().numpy() if p in opt.state and opt.state[p] else None for p in ps]
    return [p.detach().cpu().numpy() for p in ps], ms, vs


def _check(gauge, opt, ps, what, T=None, worst=None, c=OR.KERNEL):
    got = _state(opt, ps)
    r = OR.ratios(gauge, *got, T=T, c=c)
    if worst is not None:
        for k in r:
            worst[k] = max(worst.get(k, 0.0), r[k])
    assert r["p"] <= 1.0 and r["m"] <= 1.0 and r["v"] <= 1.0, (what, r)
    return r


def _fused(ps, group_of=None, **kw):
    from probpose_pytorch_amd import FusedAdamW
    return FusedAdamW(_groups(ps, group_of) if group_of else ps, lr=1e-3, **kw)


def _one_cycle(opt, T):
    return torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-4, total_steps=T, pct_start=0.1, anneal_strategy="cos")


def test_update_against_the_gauge():
    """Twenty steps under OneCycleLR (lr and beta1 change every step), max_grad_norm = 1, two groups, fresh gradient
    tensors every step, some gradients None on some steps, one parameter on a 4-byte-aligned address: p, exp_avg,
    exp_avg_sq and grad_norm after EVERY step within the bound of the module docstring."""
    T = 20
    params, grads = OR.synthetic_case(SHAPES, T, seed=21, none_every=NONE_EVERY)
    ps = _params(params, misalign=(8, 12))
    opt = _fused(ps, GROUP_OF, max_grad_norm=1.0)
    sched = _one_cycle(opt, T)
    gauge = OR.Gauge(params, GROUP_OF)
    worst, coefs, lrs = {}, set(), set()
    assert opt.grad_norm is None
    for t, row in enumerate(grads):
        _set_grads(ps, row)
        h = OR.hyper_of(opt)
        lrs.add((h[0][0], h[0][1]))
        kept = [None if p.grad is None else p.grad.clone() for p in ps]
        assert opt.step() is None
        sched.step()
        norm = gauge.step(row, h, max_norm=1.0)
        coefs.add(gauge.coef == 1.0)
        _check(gauge, opt, ps, f"step {t}", worst=worst)
        rn = abs(float(opt.grad_norm) - norm) / gauge.bound_norm()
        worst["norm"] = max(worst.get("norm", 0.0), rn)
        assert rn <= 1.0, (t, float(opt.grad_norm), norm)
        for p, k, g in zip(ps, kept, row):                     # left out entirely / gradient not rewritten by the clip
            assert (p.grad is None) == (g is None)
            if k is not None:
                assert torch.equal(p.grad, k)
    assert coefs == {True, False} and len(lrs) == T
    for i, p in enumerate(ps):
        assert int(opt.state[p]["step"]) == gauge.t[i]
    assert gauge.t[2] < gauge.t[0] == T
    assert int(opt.skipped_steps) == 0
    print("worst d / bound per class over 20 steps:", {k: round(v, 4) for k, v in worst.items()})


def test_agreement_with_torch_on_the_device():
    T = 20
    params, grads = OR.synthetic_case(SHAPES, T, seed=22, none_every=NONE_EVERY)
    ps_f, ps_t = _params(params), _params(params)
    opt_f = _fused(ps_f, GROUP_OF, max_grad_norm=1.0)
    opt_t = torch.optim.AdamW(_groups(ps_t, GROUP_OF), lr=1e-3, foreach=False)
    sch_f, sch_t = _one_cycle(opt_f, T), _one_cycle(opt_t, T)
    gauge = OR.Gauge(params, GROUP_OF)
    for row in grads:
        _set_grads(ps_f, row)
        _set_grads(ps_t, row)
        h = OR.hyper_of(opt_f)
        assert h == OR.hyper_of(opt_t)
        opt_f.step()
        torch.nn.utils.clip_grad_norm_(ps_t, max_norm=1.0)
        opt_t.step()
        sch_f.step()
        sch_t.step()
        gauge.step(row, h, max_norm=1.0)
    rf = _check(gauge, opt_f, ps_f, "FusedAdamW")
    rt = _check(gauge, opt_t, ps_t, "torch.optim.AdamW", c=OR.FLOAT32)
    bound = gauge.bound_p(c=OR.FLOAT32)
    for a, b in zip(ps_f, ps_t):
        assert float((a.detach().double() - b.detach().double()).abs().max()) <= 2 * bound
    print("d / bound after 20 steps: FusedAdamW", rf, "torch", rt)


def test_determinism():
    params, grads = OR.synthetic_case(SHAPES, 5, seed=23, none_every=NONE_EVERY)
    runs = []
    for _ in range(2):
        ps = _params(params, misalign=(8,))
        opt = _fused(ps, GROUP_OF, max_grad_norm=1.0)
        sched = _one_cycle(opt, 5)
        norms = []
        for row in grads:
            _set_grads(ps, row)
            opt.step()
            sched.step()
            norms.append(opt.grad_norm.clone())
        runs.append((_state(opt, ps), torch.stack(norms).cpu().numpy()))
    (a, na), (b, nb) = runs
    assert na.tobytes() == nb.tobytes()
    for xs, ys in zip(a, b):
        for x, y in zip(xs, ys):
            assert (x is None) == (y is None)
            if x is not None:
                assert x.tobytes() == y.tobytes()


def test_clip_branches_and_no_clipping():
    shapes = SHAPES[:14]
    group_of = GROUP_OF[:14]
    params, _ = OR.synthetic_case(shapes, 0, seed=24)
    rng = np.random.default_rng(25)
    small = [(rng.standard_normal(s) * 1e-5).astype(np.float32) for s in shapes]        # norm << 1
    big = [(rng.standard_normal(s) * 1e-1).astype(np.float32) for s in shapes]          # norm >> 1
    # below max_norm: the coefficient is exactly 1, so the bits are those of a run without clipping
    a, b = _params(params), _params(params)
    oa, ob = _fused(a, group_of, max_grad_norm=1.0), _fused(b, group_of)
    _set_grads(a, small)
    _set_grads(b, small)
    oa.step()
    ob.step()
    assert float(oa.grad_norm) < 1.0 and ob.grad_norm is None
    for xs, ys in zip(_state(oa, a), _state(ob, b)):
        for x, y in zip(xs, ys):
            assert x.tobytes() == y.tobytes()
    # above: max_norm / (norm + 1e-6), for two values of max_norm; None: the gauge without clipping
    for max_norm in (1.0, 0.25, None):
        ps = _params(params)
        opt = _fused(ps, group_of, max_grad_norm=max_norm)
        gauge = OR.Gauge(params, group_of)
        for row in (big, small, big):
            _set_grads(ps, row)
            norm = gauge.step(row, OR.hyper_of(opt), max_norm=max_norm)
            opt.step()
            _check(gauge, opt, ps, f"max_grad_norm={max_norm}")
            if max_norm is None:
                assert opt.grad_norm is None and gauge.coef == 1.0
            else:
                assert abs(float(opt.grad_norm) - norm) <= gauge.bound_norm()
        if max_norm is not None:
            assert gauge.coef == max_norm / (gauge.norm + 1e-6) < 1.0


def test_nonfinite_gradients():
    shapes = SHAPES[:14]
    group_of = GROUP_OF[:14]
    params, grads = OR.synthetic_case(shapes, 3, seed=26)
    bad = [g.copy() for g in grads[1]]
    bad[13][5, 7] = np.inf
    ps = _params(params)
    opt = _fused(ps, group_of, max_grad_norm=1.0, skip_nonfinite=True)
    gauge = OR.Gauge(params, group_of)
    _set_grads(ps, grads[0])
    gauge.step(grads[0], OR.hyper_of(opt), max_norm=1.0, skip_nonfinite=True)
    opt.step()
    before = _state(opt, ps)
    _set_grads(ps, bad)
    gauge.step(bad, OR.hyper_of(opt), max_norm=1.0, skip_nonfinite=True)
    opt.step()
    assert int(opt.skipped_steps) == 1 == gauge.skipped and not np.isfinite(float(opt.grad_norm))
    for xs, ys in zip(before, _state(opt, ps)):
        for x, y in zip(xs, ys):
            assert x.tobytes() == y.tobytes()
    assert all(int(opt.state[p]["step"]) == 1 for p in ps)
    _set_grads(ps, grads[2])
    gauge.step(grads[2], OR.hyper_of(opt), max_norm=1.0, skip_nonfinite=True)
    opt.step()
    assert all(int(opt.state[p]["step"]) == 2 for p in ps) and int(opt.skipped_steps) == 1
    _check(gauge, opt, ps, "the step after a skipped one")
    # the default: the non-finite values propagate exactly where they do under torch (inf: norm inf, coefficient 0,
    # inf * 0 = NaN in that element; NaN: the coefficient is NaN and so is everything)
    for poison in (np.inf, np.nan):
        bad[13][5, 7] = poison
        pf, pt = _params(params), _params(params)
        of = _fused(pf, group_of, max_grad_norm=1.0)
        ot = torch.optim.AdamW(_groups(pt, group_of), lr=1e-3, foreach=False)
        _set_grads(pf, bad)
        _set_grads(pt, bad)
        of.step()
        torch.nn.utils.clip_grad_norm_(pt, max_norm=1.0)
        ot.step()
        assert int(of.skipped_steps) == 0
        n_bad = 0
        for a, b in zip(pf, pt):
            assert torch.equal(torch.isfinite(a), torch.isfinite(b))
            n_bad += int((~torch.isfinite(a)).sum())
        assert n_bad >= 1


def _tiny_backbone():
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_vit_state
    size = (64, 48)
    bb = ScratchViTBackbone(size, 16, embed_dim=128, depth=1, num_heads=2, differentiable=True)
    bb.model.load_state_dict(synthetic_vit_state(size, 16, 128, 1, seed=31))
    return bb.cuda().train(), synthetic_crops(2, *size, seed=32).cuda()


@pytest.mark.parametrize("which", ["torch", "fused"])
def test_version_counter_guards_a_delayed_backward(which):
    """An optimizer step between a forward and its delayed backward raises instead of mixing weights: the kernels
    write through raw pointers, so FusedAdamW bumps the version counters itself."""
    bb, x = _tiny_backbone()
    params = [p for p in bb.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-3) if which == "torch" else _fused(params, max_grad_norm=1.0)
    bb(x).square().sum().backward()                 # gradients from an earlier backward
    versions = [p._version for p in params]
    pending = bb(x).square().sum()
    opt.step()
    assert all(p._version > v for p, v in zip(params, versions) if p.grad is not None)
    with pytest.raises(RuntimeError):
        pending.backward()


def _manual_lr(opt, t):
    for g in opt.param_groups:
        g["lr"] = 5e-4 * (0.5 + 0.05 * t)
        g["betas"] = (0.95 - 0.01 * t, 0.999)


@pytest.mark.parametrize("first", ["torch", "fused"])
def test_state_interchange(first):
    """Five steps under one optimizer, its state_dict() into the other, five more: ten gauge steps, bound (1)."""
    T = 10
    params, grads = OR.synthetic_case(SHAPES, T, seed=27, none_every=NONE_EVERY)
    ps = _params(params)
    gauge = OR.Gauge(params, GROUP_OF)

    def make(kind):
        if kind == "torch":
            return torch.optim.AdamW(_groups(ps, GROUP_OF), lr=1e-3, foreach=False)
        return _fused(ps, GROUP_OF, max_grad_norm=1.0)

    def run(opt, kind, lo, hi):
        for t in range(lo, hi):
            _set_grads(ps, grads[t])
            _manual_lr(opt, t)
            gauge.step(grads[t], OR.hyper_of(opt), max_norm=1.0)
            if kind == "torch":
                torch.nn.utils.clip_grad_norm_(ps, max_norm=1.0)
            opt.step()

    second = "fused" if first == "torch" else "torch"
    a = make(first)
    run(a, first, 0, 5)
    sd = copy.deepcopy(a.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    b = make(second)
    b.load_state_dict(sd)
    if second == "torch":
        for g in b.param_groups:          # the loaded groups carry foreach=None: keep the single-tensor path
            g["foreach"] = False
    if second == "fused":
        assert all(g["max_grad_norm"] == 1.0 and g["skip_nonfinite"] is False for g in b.param_groups)
    run(b, second, 5, T)
    _check(gauge, b, ps, f"{first} -> {second}", c=OR.FLOAT32)       # five of the ten steps are torch's
    for i, p in enumerate(ps):
        assert int(b.state[p]["step"]) == gauge.t[i]


def test_training_loop():
    """The setup of tests/test_model_train_gpu.py with FusedAdamW(weight_decay=0.1, max_grad_norm=1.0) + OneCycleLR in
    place of the torch pair: after each of the six steps the parameters match the gauge fed with that step's actual
    gradients; frozen head parameters keep grad None and their bits; the eval path reproduces the oracle forward from
    the trained state_dict."""
    from oracle import probpose_oracle as orc
    from probpose_pytorch_amd import FusedAdamW
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.loss import ProbPoseLoss
    from probpose_pytorch_amd.model import ProbPoseModel
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_head_state, synthetic_vit_state
    from tests import loss_grad_reference as LG
    from tests import loss_reference as LR
    B, K, C, heads, depth, size = 2, 20, 384, 12, 2, (384, 384)
    H = W = 96
    pools = [(4, 4), (2, 2), (2, 2)]
    rng = np.random.default_rng(11)
    kps = rng.uniform(20, 364, (B, K, 2)).astype(np.float32)
    annotated = rng.random((B, K)) > 0.2
    vis = (rng.random((B, K)) > 0.3).astype(np.float32)
    gt_hm, in_image = LR.encode_probmaps(kps, annotated.astype(np.float32), size, (W, H))
    gt_np = dict(heatmaps=gt_hm, in_image=in_image[:, None, :], keypoints_visible=annotated[:, None, :],
                 keypoints_visibility=vis[:, None, :])
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in gt_np.items()}
    loss_fn = ProbPoseLoss(Codec(ArgMaxProbMap(size, (W, H), np.full(K, 0.05))), freeze_error=True,
                           differentiable=True)
    backbone = ScratchViTBackbone(size, 16, embed_dim=C, depth=depth, num_heads=heads, differentiable=True)
    backbone.model.load_state_dict(synthetic_vit_state(size, 16, C, depth, seed=12))
    head = ProbMapHead(C, K, pools, (256, 256), (4, 4), final_layer_kernel_size=1, freeze_error=True,
                       normalize=1.0, differentiable=True)
    head.load_state_dict(synthetic_head_state(C, K, n_pools=3, deconv_out=(256, 256), seed=13), strict=False)
    model = ProbPoseModel(backbone, head).cuda().train()
    x = synthetic_crops(B, *size, seed=14)
    xc = x.cuda()
    ps = list(model.parameters())
    start = [p.detach().cpu().numpy().copy() for p in ps]
    frozen = [i for i, p in enumerate(ps) if not p.requires_grad]
    assert frozen and len(frozen) < len(ps)
    opt = FusedAdamW(model.parameters(), weight_decay=0.1, max_grad_norm=1.0)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-4, total_steps=6, pct_start=0.1)
    gauge = OR.Gauge(start, [0] * len(ps))
    worst = {}
    for step in range(6):
        opt.zero_grad()
        pred = model(xc)
        losses = loss_fn(gt, pred)
        loss = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
        loss.backward()
        row = [None if p.grad is None else p.grad.detach().cpu().numpy() for p in ps]
        for i in frozen:
            assert row[i] is None
        assert all(row[i] is not None for i in range(len(ps)) if i not in frozen)
        h = OR.hyper_of(opt)
        opt.step()
        sched.step()
        norm = gauge.step(row, h, max_norm=1.0)
        _check(gauge, opt, ps, f"training step {step}", worst=worst)
        worst["norm"] = max(worst.get("norm", 0.0), abs(float(opt.grad_norm) - norm) / gauge.bound_norm())
        assert worst["norm"] <= 1.0, (step, float(opt.grad_norm), norm)
    for i in frozen:
        assert ps[i].detach().cpu().numpy().tobytes() == start[i].tobytes() and ps[i] not in opt.state
    print("training loop, worst d / bound per class:", {k: round(v, 4) for k, v in worst.items()})
    # the eval path (cached plans) picks up the trained parameters
    model.eval()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        got = model(xc)
        want = orc.model_forward(sd, x, patch=16, heads=heads, pools=pools, normalize=1.0)
        f_got = model.backbone(xc)
        f_want = orc.backbone_forward(sd, x, patch=16, heads=heads, prefix="backbone.model.")
    assert float((f_got.cpu() - f_want).abs().max()) <= 1e-4
    for g, w in zip(got, want):
        assert float((g.cpu() - w).abs().max()) <= 1e-4
