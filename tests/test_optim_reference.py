"""The FusedAdamW gauge (tests/optim_reference.py) pinned on the CPU: equal to torch.optim.AdamW + clip_grad_norm_ +
OneCycleLR in float64, and sharp enough that a wrong optimizer misses the float32 bound by a wide factor."""
import numpy as np
import pytest
import torch

from tests import optim_reference as OR

TRAIN_SHAPES = [(384, 1536), (1152, 384), (384,), (1536,), (20, 256, 1, 1)]
GROUP_OF = [0, 0, 1, 1, 0]


def _torch_run(params, grads, dtype, group_of, total_steps):
    ps = [torch.nn.Parameter(torch.from_numpy(p).to(dtype, copy=True)) for p in params]
    opt = torch.optim.AdamW([dict(params=[p for p, k in zip(ps, group_of) if k == 0], weight_decay=0.1),
                             dict(params=[p for p, k in zip(ps, group_of) if k == 1], weight_decay=0.0)], lr=1e-3)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-4, total_steps=total_steps, pct_start=0.1,
                                                anneal_strategy="cos")
    hypers, betas1 = [], set()
    for row in grads:
        for p, g in zip(ps, row):
            # a copy: clip_grad_norm_ rewrites the gradient in place
            p.grad = None if g is None else torch.from_numpy(g).to(dtype, copy=True)
        torch.nn.utils.clip_grad_norm_(ps, max_norm=1.0)
        hypers.append(OR.hyper_of(opt))
        betas1.add(hypers[-1][0][1])
        opt.step()
        sched.step()
    assert len(betas1) > 1, "OneCycleLR cycles beta1 on AdamW: the gauge must be fed per-step betas"
    return [p.detach().numpy() for p in ps], opt, hypers


def test_gauge_equals_torch_float64():
    shapes = [(7, 5), (33,), (4, 3, 2), (1,)]
    group_of = [0, 1, 0, 1]
    params, grads = OR.synthetic_case(shapes, 12, seed=3, none_every={1: 4}, g_std=0.5)
    got, opt, hypers = _torch_run(params, grads, torch.float64, group_of, 12)
    gauge = OR.Gauge(params, group_of)
    coefs = set()
    for row, h in zip(grads, hypers):
        gauge.step(row, h, max_norm=1.0)
        coefs.add(gauge.coef == 1.0)
    assert coefs == {True, False}, "both clip branches must be taken"
    ulp = 2.0 ** -52
    for a, w in zip(got, gauge.p):
        assert float(np.abs(a - w).max()) <= 8 * ulp * gauge.max_p
    # the state torch keeps is the gauge's too
    order = [i for k in (0, 1) for i, gk in enumerate(group_of) if gk == k]
    for p_t, i in zip([p for g in opt.param_groups for p in g["params"]], order):
        st = opt.state[p_t]
        assert int(st["step"]) == gauge.t[i]
        assert float(np.abs(st["exp_avg"].numpy() - gauge.m[i]).max()) <= 8 * ulp * max(gauge.G, 1e-300)
        assert float(np.abs(st["exp_avg_sq"].numpy() - gauge.v[i]).max()) <= 8 * ulp * max(gauge.G ** 2, 1e-300)


def test_gauge_has_teeth():
    """Twenty steps on five tensors shaped like train.py's: torch's float32 CPU arithmetic stays inside the float32
    bound of the gauge, each wrong variant misses it by more than two orders of magnitude."""
    T = 20
    params, grads = OR.synthetic_case(TRAIN_SHAPES, T, seed=5)
    got32, _, hypers = _torch_run(params, grads, torch.float32, GROUP_OF, T)
    gauge = OR.Gauge(params, GROUP_OF)
    wrong = {k: OR.Gauge(params, GROUP_OF, variant=k) for k in ("l2", "nobias", "pertensor")}
    coefs = set()
    for row, h in zip(grads, hypers):
        gauge.step(row, h, max_norm=1.0)
        coefs.add(gauge.coef == 1.0)
        for w in wrong.values():
            w.step(row, h, max_norm=1.0)
    assert coefs == {True, False}
    r32 = OR.ratios(gauge, got32, [None] * 5, [None] * 5, c=OR.FLOAT32)["p"]
    print(f"torch float32 on the CPU: d / bound = {r32:.4f} "
          f"({r32 * gauge.bound_p(c=OR.FLOAT32) / (OR.U * gauge.max_p):.2f} u max|p|)")
    assert r32 <= 1.0
    for k, w in wrong.items():
        r = OR.ratios(gauge, w.p, [None] * 5, [None] * 5, c=OR.FLOAT32)["p"]    # the wider of the two bounds
        print(f"wrong variant {k}: d / bound = {r:.3g}")
        assert r >= 100.0, (k, r)
