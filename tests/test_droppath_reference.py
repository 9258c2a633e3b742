"""CPU tests of tests/droppath_reference.py (the float64 gauge of the backbone's training step with stochastic depth),
of vit_train.draw_keep and of the CPU-side surface of ``ScratchViTBackbone(drop_path_rate=...)``."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import droppath_reference as DR
from tests import vit_grad_reference as VR

IMG, C, HEADS, DEPTH, B = (32, 48), 32, 2, 3, 4
RATES = [float(v) for v in torch.linspace(0, 0.4, DEPTH)]
# every crop kept in block 0 (rate 0); the two branches of blocks 1 and 2 differ
KEEP = torch.tensor([[[1, 1, 1, 1], [1, 1, 1, 1]],
                     [[1, 0, 1, 1], [0, 1, 1, 0]],
                     [[0, 1, 0, 1], [1, 1, 0, 1]]], dtype=torch.bool)


def _case(seed=0):
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_vit_state
    sd = synthetic_vit_state(IMG, 16, C, DEPTH, seed=seed)
    x = synthetic_crops(B, *IMG, seed=seed + 1)
    N = (IMG[0] // 16) * (IMG[1] // 16)
    ups = torch.randn((B, N, C), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64)
    return sd, x, ups, N


def test_gauge_without_drops_is_the_plain_gauge():
    sd, x, ups, _ = _case()
    want = VR.vit_step(sd, x, ups, patch=16, heads=HEADS)
    got = DR.vit_step_droppath(sd, x, ups, torch.ones((DEPTH, 2, B), dtype=torch.bool), [0.0] * DEPTH, patch=16,
                               heads=HEADS)
    assert torch.equal(got["features"], want["features"])
    for k, g in want["grads"].items():
        assert torch.equal(got["grads"][k], g), k


def _restated(sd, x, keep, rates):
    """The same step from plain torch ops and torch.where on whole crops, differentiated by plain autograd."""
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=16).flatten(2).transpose(1, 2)
    t = t + sd["pos_embed"]
    Bn, N, Cc = t.shape
    hd = Cc // HEADS
    for i, p in enumerate(rates):
        b = f"blocks.{i}."
        h = F.layer_norm(t, (Cc,), sd[b + "norm1.weight"], sd[b + "norm1.bias"], 1e-6)
        q, k, v = F.linear(h, sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]).reshape(Bn, N, 3, HEADS, hd) \
            .permute(2, 0, 3, 1, 4).unbind(0)
        o = (((q @ k.transpose(-2, -1)) / math.sqrt(hd)).softmax(-1) @ v).transpose(1, 2).reshape(Bn, N, Cc)
        o = F.linear(o, sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"])
        t = torch.where(keep[i, 0][:, None, None], t + o / (1.0 - p), t)
        h = F.layer_norm(t, (Cc,), sd[b + "norm2.weight"], sd[b + "norm2.bias"], 1e-6)
        h = F.gelu(F.linear(h, sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"]))
        h = F.linear(h, sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"])
        t = torch.where(keep[i, 1][:, None, None], t + h / (1.0 - p), t)
    return F.layer_norm(t, (Cc,), sd["norm.weight"], sd["norm.bias"], 1e-6)


def test_gauge_agrees_with_autograd_of_a_restatement():
    sd, x, ups, _ = _case()
    got = DR.vit_step_droppath(sd, x, ups, KEEP, RATES, patch=16, heads=HEADS)
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    f = _restated(leaves, x.double(), KEEP, RATES)
    names = list(leaves)
    gr = torch.autograd.grad(f, [leaves[k] for k in names], ups, allow_unused=True)
    assert float((got["features"] - f.detach()).abs().max()) <= 1e-12 * float(f.detach().abs().max())
    for k, g in zip(names, gr):
        assert g is not None, k
        mag = max(float(g.abs().max()), 1e-300)
        assert float((got["grads"][k] - g).abs().max()) <= 1e-11 * mag, k


@pytest.mark.parametrize("fault", DR.FAULTS)
def test_gauge_rejects_planted_faults(fault):
    """Each fault misses the GPU test's fp32 bound (tests/test_droppath_gpu.py: c = 2 S' sqrt(K))."""
    sd, x, ups, N = _case()
    c = 2 * DR.n_stages(DEPTH, sum(p > 0 for p in RATES)) * math.sqrt(max(4 * C, B * N))
    want = DR.vit_step_droppath(sd, x, ups, KEEP, RATES, patch=16, heads=HEADS)
    got = DR.vit_step_droppath(sd, x, ups, KEEP, RATES, patch=16, heads=HEADS, fault=fault)
    worst = max(VR.ratio(got["grads"][k], want["grads"][k], VR.U_F32, c) for k in want["grads"])
    print(f"fault {fault}: worst gradient d/bound {worst:.3g}")
    assert worst > 1.0, fault


def test_draw_keep_shape_rate_zero_and_seed():
    from probpose_pytorch_amd.vit_train import draw_keep
    torch.manual_seed(3)
    a = draw_keep(RATES, 16)
    assert a.shape == (DEPTH, 2, 16) and a.dtype == torch.bool and a.device.type == "cpu"
    assert bool(a[0].all())
    torch.manual_seed(3)
    assert torch.equal(draw_keep(RATES, 16), a)
    torch.manual_seed(4)
    assert not torch.equal(draw_keep(RATES, 16), a)
    g = torch.Generator().manual_seed(3)
    assert torch.equal(draw_keep(RATES, 16, generator=g), a)
    # a block at rate 0 draws nothing: the stream of the blocks above it does not move
    torch.manual_seed(3)
    assert torch.equal(draw_keep([0.0] + RATES, 16)[1:], a)
    assert bool(draw_keep([0.0] * 4, 8).all())


def test_draw_keep_frequency():
    from probpose_pytorch_amd.vit_train import draw_keep
    rates = [float(v) for v in torch.linspace(0, 0.55, 6)]
    n = 4096
    keep = draw_keep(rates, n // 2, generator=torch.Generator().manual_seed(11))
    for i, p in enumerate(rates):
        freq = float(keep[i].double().mean())
        assert abs(freq - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), (i, p, freq)


def test_constructor_surface():
    from probpose_pytorch_amd.backbone import ScratchViTBackbone, VisionTransformer
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError):
            ScratchViTBackbone((64, 48), 16, embed_dim=32, depth=2, num_heads=2, drop_path_rate=bad)
        with pytest.raises(ValueError):
            VisionTransformer(img_size=(64, 48), embed_dim=32, depth=2, num_heads=2, drop_path_rate=bad)
    a = ScratchViTBackbone((64, 48), 16, embed_dim=32, depth=4, num_heads=2, drop_path_rate=0.3, differentiable=True)
    assert torch.equal(torch.tensor(a.drop_path_rates), torch.linspace(0, 0.3, 4))
    assert torch.equal(torch.tensor(a.model.drop_path_rates), torch.linspace(0, 0.3, 4))
    assert a.last_drop_path_keep is None
    one = ScratchViTBackbone((64, 48), 16, embed_dim=32, depth=1, num_heads=2, drop_path_rate=0.3)
    assert one.drop_path_rates == [0.0]
    b = ScratchViTBackbone((64, 48), 16, embed_dim=32, depth=4, num_heads=2)
    assert b.drop_path_rates == [0.0] * 4
    assert list(a.state_dict()) == list(b.state_dict())
    assert not list(a.buffers())
    a.load_state_dict(b.state_dict())


def test_explicit_keep_is_checked():
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.vit_train import _check_keep
    vit = ScratchViTBackbone((64, 48), 16, embed_dim=32, depth=3, num_heads=2, drop_path_rate=0.4).model
    _check_keep(vit, KEEP, 4)
    with pytest.raises(ValueError):
        _check_keep(vit, KEEP[:, :, :3], 4)
    with pytest.raises(ValueError):
        _check_keep(vit, KEEP.to(torch.int32), 4)
    bad = KEEP.clone()
    bad[0, 1, 2] = False
    with pytest.raises(ValueError, match="rate is 0"):
        _check_keep(vit, bad, 4)
