"""CPU tests of tests/vit_grad_reference.py (the float64 gauge of the backbone's training step) and of the CPU-side
surface of ``ScratchViTBackbone(differentiable=True)``."""
import pytest
import torch

from oracle import probpose_oracle as orc
from tests import vit_grad_reference as VR


def _tiny(img=(32, 48), C=16, depth=1, seed=0):
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_vit_state
    sd = synthetic_vit_state(img, 16, C, depth, seed=seed)
    x = synthetic_crops(2, *img, seed=seed + 1)
    N = (img[0] // 16) * (img[1] // 16)
    ups = torch.randn((2, N, C), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64)
    return sd, x, ups


def test_gauge_forward_is_the_oracle():
    sd, x, _ = _tiny(depth=2)
    sdd = {k: v.double() for k, v in sd.items()}
    want = orc.vit_forward_features(sdd, x.double(), patch=16, heads=2)
    got = VR.vit_forward(sdd, x.double(), patch=16, heads=2)
    assert float((got - want).abs().max()) <= 1e-12


def test_gauge_agrees_with_gradcheck():
    sd, x, _ = _tiny(img=(32, 32), C=8)
    names = list(sd)
    xd = x.double()

    def f(*ps):
        return VR.vit_forward(dict(zip(names, ps)), xd, patch=16, heads=2)

    ps = tuple(v.double().requires_grad_(True) for v in sd.values())
    assert torch.autograd.gradcheck(f, ps, eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("fault", VR.FAULTS)
def test_gauge_rejects_planted_faults(fault):
    sd, x, ups = _tiny()
    want = VR.vit_step(sd, x, ups, patch=16, heads=2)
    got = VR.vit_step(sd, x, ups, patch=16, heads=2, fault=fault)
    assert torch.equal(got["features"], want["features"])
    worst = max(VR.ratio(got["grads"][k], want["grads"][k], VR.U_F32, 4096) for k in want["grads"])
    assert worst > 1.0, fault


def test_differentiable_backbone_refuses_cpu_tensors():
    from probpose_pytorch_amd._lib import HipExtensionError
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    bb = ScratchViTBackbone((32, 48), 16, embed_dim=16, depth=1, num_heads=2, differentiable=True).train()
    assert bb.differentiable and bb.model.differentiable
    x = torch.rand(2, 3, 32, 48)
    with pytest.raises(HipExtensionError):
        bb(x)
    with pytest.raises(HipExtensionError):
        bb.model.forward_tokens(x)


def test_flag_changes_no_state_dict_key():
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.synthetic import synthetic_vit_state
    a = ScratchViTBackbone((64, 48), 16, embed_dim=32, depth=2, num_heads=2, differentiable=True)
    b = ScratchViTBackbone((64, 48), 16, embed_dim=32, depth=2, num_heads=2)
    assert list(a.state_dict()) == list(b.state_dict())
    assert sorted(a.state_dict()) == sorted("model." + k for k in synthetic_vit_state((64, 48), 16, 32, 2))
    a.load_state_dict(b.state_dict())
