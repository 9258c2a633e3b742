"""The ModelEma gauge (tests/ema_reference.py) pinned on the CPU: equal to timm's formula in float64, sharp enough that
each planted fault misses the float32 bound by a wide factor; ModelEma's own schedule, key matching and state_dict on
a CPU model (the update itself has no CPU path and raises)."""
import copy
import math

import numpy as np
import pytest
import torch

from tests import ema_reference as ER

TRAIN_SHAPES = [(384, 1536), (1152, 384), (384,), (1536,), (20, 256, 1, 1), (256,)]


def test_gauge_equals_timm_formula_in_float64():
    """timm: ema = d ema + (1 - d) model.  The gauge's s + w (p - s) is the same number up to float64 roundings."""
    start, rows = ER.synthetic_states([(7, 5), (33,), (4, 3, 2), (1,)], 12, seed=3, drift=0.5)
    for decay, tau in ((0.9999, None), (0.99, 3.0), (0.5, None)):
        gauge = ER.Gauge(start, decay, tau)
        timm = [a.astype(np.float64) if ER.is_averaged(a) else a.copy() for a in start]
        for t, row in enumerate(rows, 1):
            w = gauge.step(row)
            d = ER.decay_at(decay, tau, t)
            assert w == 1.0 - d
            timm = [d * s + (1.0 - d) * p.astype(np.float64) if ER.is_averaged(p) else p.copy()
                    for s, p in zip(timm, row)]
        for i, (a, b) in enumerate(zip(timm, gauge.s)):
            if gauge.averaged[i]:
                assert float(np.abs(a - b).max()) <= 8 * 12 * 2.0 ** -53 * gauge.M[i]
            else:
                assert a.dtype == np.int64 and int(a) == int(b) == 12


def test_one_update_is_the_chained_gauge_first_step():
    start, rows = ER.synthetic_states([(9,), (2, 3)], 1, seed=4, drift=0.5)
    gauge = ER.Gauge(start, 0.9)
    gauge.step(rows[0])
    one = ER.update(start, rows[0], 1.0 - 0.9)
    for a, b in zip(one, gauge.s):
        assert a.tobytes() == b.tobytes()
    f32 = [a.astype(np.float32) if a.dtype == np.float64 else a for a in one]
    for g, w, s, p in zip(f32[:2], one[:2], start[:2], rows[0][:2]):
        assert np.all(np.abs(g.astype(np.float64) - w) <= ER.bound_one(w, s, p))


def test_gauge_has_teeth():
    """Six updates with decay 0.99, tau 3 on tensors shaped like train.py's and a step counter: a float32 evaluation
    (subtract, multiply, add, each rounded) stays inside 3 T u M, the float64 evaluation rounded once per update
    inside T u M, and each planted fault misses T u M by more than two orders of magnitude."""
    T, decay, tau = 6, 0.99, 3.0
    start, rows = ER.synthetic_states(TRAIN_SHAPES, T, seed=5)
    gauge = ER.Gauge(start, decay, tau)
    wrong = {k: ER.Gauge(start, decay, tau, variant=k) for k in ER.VARIANTS if k}
    f32 = [a.copy() for a in start]
    once = [a.copy() for a in start]
    for row in rows:
        w = gauge.step(row)
        for g in wrong.values():
            g.step(row)
        w32 = np.float32(w)
        f32 = [s + w32 * (p - s) if ER.is_averaged(s) else p.copy() for s, p in zip(f32, row)]
        once = [a.astype(np.float32) if ER.is_averaged(s) else a for a, s in zip(ER.update(once, row, w), once)]
    assert all(a.dtype == s.dtype for a, s in zip(f32, start))
    r32, r1 = gauge.ratio(f32, c=3.0), gauge.ratio(once)
    print(f"float32 lerp: d / (3 T u M) = {r32:.4f}; float64 rounded once per update: d / (T u M) = {r1:.4f}")
    assert r32 <= 1.0 and r1 <= 1.0
    for k, g in wrong.items():
        r = gauge.ratio(g.s)
        print(f"planted fault {k}: d / bound = {r:.3g}")
        assert r >= 100.0, (k, r)


def test_decay_schedule_closed_forms():
    from probpose_pytorch_amd.ema import ModelEma
    model = torch.nn.Linear(3, 2)
    flat = ModelEma(model, decay=0.9999)
    assert all(flat.decay_at(t) == 0.9999 for t in (1, 2, 1000))
    warm = ModelEma(model, decay=0.9999, tau=2000)
    for t in (1, 2, 10, 2000, 20000, 10 ** 6):
        assert warm.decay_at(t) == 0.9999 * (1.0 - math.exp(-t / 2000)) == ER.decay_at(0.9999, 2000, t)
    assert warm.decay_at(1) < 1e-3 and abs(warm.decay_at(2000) - 0.9999 * (1 - 1 / math.e)) < 1e-15
    assert warm.decay_at(10 ** 6) == 0.9999
    assert ModelEma(model).decay == 0.9999 and ModelEma(model).tau is None
    for bad in (dict(decay=1.5), dict(decay=-0.1), dict(tau=0.0), dict(tau=-1.0)):
        with pytest.raises(ValueError):
            ModelEma(model, **bad)


def _cpu_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                               torch.nn.Linear(4, 2))


def test_model_ema_construction_and_state_dict_on_cpu():
    from probpose_pytorch_amd import ModelEma, _lib
    model = _cpu_model().train()
    model[0].weight.grad = torch.ones_like(model[0].weight)
    ema = ModelEma(model, decay=0.99, tau=3)
    assert ema.module is not model and not ema.module.training and model.training
    assert all(not p.requires_grad and p.grad is None for p in ema.module.parameters())
    assert all(p.requires_grad for p in model.parameters())
    sd, md = ema.module.state_dict(), model.state_dict()
    assert list(sd) == list(md) and "1.num_batches_tracked" in sd and "1.running_var" in sd
    for k in sd:
        assert sd[k].data_ptr() != md[k].data_ptr() and torch.equal(sd[k], md[k])
    state = ema.state_dict()
    assert set(state) == {"module", "updates", "decay", "tau"}
    assert state["updates"] == 0 and state["decay"] == 0.99 and state["tau"] == 3.0
    # a checkpoint of the average is an ordinary model checkpoint
    _cpu_model().load_state_dict(state["module"])
    # the round trip, with a resumed update count
    saved = copy.deepcopy(state)
    saved["updates"] = 41
    with torch.no_grad():
        saved["module"]["3.bias"].fill_(0.25)
        saved["module"]["1.num_batches_tracked"].fill_(7)
    other = ModelEma(_cpu_model(), decay=0.5)
    other.load_state_dict(saved)
    assert other.updates == 41 and other.decay == 0.99 and other.tau == 3.0
    assert other.decay_at(other.updates + 1) == ER.decay_at(0.99, 3.0, 42)
    assert torch.equal(other.module[3].bias, torch.full((2,), 0.25))
    assert int(other.module[1].num_batches_tracked) == 7
    assert all(not p.requires_grad for p in other.module.parameters())
    with pytest.raises(ValueError, match="lacks"):
        other.load_state_dict({"module": saved["module"]})
    # the update has no CPU path
    with pytest.raises(_lib.HipExtensionError):
        ema.update(model)
    assert ema.updates == 0


def test_model_ema_refuses_a_model_that_no_longer_matches():
    from probpose_pytorch_amd import ModelEma
    model = _cpu_model()
    ema = ModelEma(model)
    grown = _cpu_model()
    grown.add_module("4", torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="unexpected"):
        ema.update(grown)
    with pytest.raises(ValueError, match="missing"):
        ema.update(torch.nn.Sequential(*list(_cpu_model())[:3]))
    reshaped = _cpu_model()
    reshaped[3] = torch.nn.Linear(4, 5)
    with pytest.raises(ValueError, match="shape"):
        ema.update(reshaped)
    assert ema.updates == 0


def test_ema_update_refusals():
    from probpose_pytorch_amd import _lib, ema_update_
    f = torch.zeros(8)
    with pytest.raises(NotImplementedError):
        ema_update_([torch.zeros(8, dtype=torch.float64)], [torch.zeros(8, dtype=torch.float64)], 0.1)
    with pytest.raises(NotImplementedError):
        ema_update_([torch.zeros(8, dtype=torch.bfloat16)], [torch.zeros(8, dtype=torch.bfloat16)], 0.1)
    with pytest.raises(NotImplementedError):
        ema_update_([torch.zeros(8, dtype=torch.int8)], [torch.zeros(8, dtype=torch.int8)], 0.1)
    with pytest.raises(NotImplementedError):
        ema_update_([torch.zeros(4, 3).t()], [torch.zeros(3, 4)], 0.1)
    with pytest.raises(NotImplementedError):
        ema_update_([torch.zeros(3, 4)], [torch.zeros(4, 3).t()], 0.1)
    with pytest.raises(NotImplementedError):                 # a second device
        ema_update_([f, torch.zeros(8, device="meta")], [torch.ones(8), torch.zeros(8, device="meta")], 0.1)
    with pytest.raises(ValueError, match="shapes"):
        ema_update_([torch.zeros(8)], [torch.zeros(2, 4)], 0.1)
    with pytest.raises(ValueError, match="dtypes"):
        ema_update_([torch.zeros(8)], [torch.zeros(8, dtype=torch.int32)], 0.1)
    with pytest.raises(ValueError, match="sources"):
        ema_update_([f], [], 0.1)
    buf = torch.zeros(32)
    for dsts, srcs in (([f], [f]),                                        # dst is src
                       ([buf[:16]], [buf[8:24]]),                         # dst overlaps its src
                       ([buf[:8], buf[16:24]], [buf[24:], buf[4:12]]),    # dst 0 overlaps the src of pair 1
                       ([buf[:8], buf[4:12]], [torch.ones(8), torch.ones(8)])):   # two dsts overlap
        with pytest.raises(ValueError, match="overlaps"):
            ema_update_(dsts, srcs, 0.1)
    if not f.is_cuda:
        with pytest.raises(_lib.HipExtensionError):          # the hot path has no CPU fallback
            ema_update_([torch.zeros(8)], [torch.ones(8)], 0.1)
