"""CPU tests of tests/head_grad_reference.py: the float64 restatement of the train-mode ProbMapHead reproduces the
reference's own train-mode step (tests/golden/head_grad.npz, minted from the unmodified reference head) and rejects
planted faults."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_grad_reference as HR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_grad.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLD)


def _worst(golden, name, fault=None):
    head, feats, ups, cfg, xg = HR.case(name)
    r = HR.head_step(head.state_dict(), cfg, feats, ups, HR.trainable_of(head), xg, fault)
    worst = 0.0
    for i, o in enumerate(r["outputs"]):
        worst = max(worst, HR.golden_ratio(golden, f"{name}/out{i}", o))
    for k, p in head.named_parameters():
        if f"{name}/nograd/{k}" in golden:
            assert k not in r["grads"], k
            continue
        if k in r["dy_mag"]:    # a conv bias ahead of a train-mode BN: zero up to rounding, bounded in absolute terms
            worst = max(worst, HR.golden_abs_ratio(golden, f"{name}/grad/{k}", r["grads"][k], r["dy_mag"][k]))
        else:
            worst = max(worst, HR.golden_ratio(golden, f"{name}/grad/{k}", r["grads"][k], tol=1e-7))
    if xg:
        worst = max(worst, HR.golden_ratio(golden, f"{name}/xgrad", r["x_grad"], tol=1e-7))
    for k, v in r["running"].items():
        worst = max(worst, HR.golden_ratio(golden, f"{name}/run/{k}", v))
    return worst


@pytest.mark.parametrize("name", sorted(HR.CASES))
def test_restatement_matches_reference_goldens(golden, name):
    assert _worst(golden, name) <= 1.0


@pytest.mark.parametrize("fault", ["unbiased_norm", "biased_running"])
def test_bn_faults_rejected_on_goldens(golden, fault):
    assert _worst(golden, "T1", fault) > 1.0


def test_missing_probability_detach_rejected_on_goldens(golden):
    assert _worst(golden, "T4", "no_prob_detach") > 1.0


def test_pooling_ties_follow_torch_first_maximum():
    x = torch.tensor([[[[1.0, 3.0, 3.0], [3.0, 0.5, 3.0]]]], dtype=torch.float64, requires_grad=True)
    g = torch.tensor([[[[2.0]]]], dtype=torch.float64)
    (want,) = torch.autograd.grad(F.max_pool2d(x, (2, 3), (2, 3)), x, g)
    (got,) = torch.autograd.grad(HR.maxpool(x, 2, 3), x, g)
    assert torch.equal(got, want)
    (bad,) = torch.autograd.grad(HR.maxpool(x, 2, 3, fault="last_max"), x, g)
    assert not torch.equal(bad, want)


def test_clamp_mask_is_inclusive_as_torch():
    v = torch.tensor([-0.5, 0.0, 0.25, 1.0, 1.5], dtype=torch.float64, requires_grad=True)
    g = torch.arange(1.0, 6.0, dtype=torch.float64)
    (want,) = torch.autograd.grad(torch.clamp(v, 0, 1), v, g)
    (got,) = torch.autograd.grad(HR._Clamp01.apply(v, False), v, g)
    (bad,) = torch.autograd.grad(HR._Clamp01.apply(v, True), v, g)
    assert torch.equal(got, want) and not torch.equal(bad, want)


def test_sparsemax_backward_by_finite_differences():
    torch.manual_seed(0)
    z = (torch.randn(3, 40, dtype=torch.float64) * 2).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: HR._Sparsemax.apply(t, False), (z,))
    assert not torch.autograd.gradcheck(lambda t: HR._Sparsemax.apply(t, True), (z,), raise_exception=False)


def test_sparsemax_forward_matches_sort_definition():
    torch.manual_seed(1)
    z = torch.randn(4, 50, dtype=torch.float64)
    p = HR._Sparsemax.apply(z, False)
    assert torch.allclose(p.sum(-1), torch.ones(4, dtype=torch.float64))
    assert torch.allclose(p, HR._sparsemax_sort(z))
