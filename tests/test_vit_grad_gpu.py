"""GPU tests of the training ScratchViTBackbone (``ScratchViTBackbone(differentiable=True)`` in ``.train()`` mode,
vit_train.py and csrc/pp_vit_grad.hip) against the float64 gauge tests/vit_grad_reference.py.

Bounds, |got - want| <= c u max|want| per tensor (head_grad_reference.ratio):
* fp32 (exact-fp32 MFMA, u = 2^-24).  A value is the end of a chain of S kernel stages (vit_grad_reference.n_stages:
  S = 8 depth + 2 for a gradient, 4 depth + 2 for the features), each a reduction of depth at most K = max(4C, B N)
  (the GEMM depths and the weight gradients' row sums) whose f32 rounding adds about sqrt(K) u relative to the
  magnitude of its terms; the residual stream and the normalisations keep the terms within a small factor of the
  result: c = 2 S sqrt(K).
* bf16 against fp32 mode (u = 2^-8): every stage rounds its operands (activations, weights, the residual gradient's
  copy) to bf16 once, 2 u relative per stage: c = 2 S against the largest element.  Norm-wise, the roundings of the
  S stages are independent, so the Frobenius error grows like sqrt(S): ||got - want|| <= 2 sqrt(S) u ||want||.
Each test prints its worst d/bound per class (run with -s).
"""
import math

import pytest
import torch

from tests import vit_grad_reference as VR

pytestmark = pytest.mark.gpu

MODELS = {
    # name: (img, C, heads, depth, B)
    "tiny": ((128, 96), 64, 2, 2, 2),
    "tiny_hd64": ((128, 96), 128, 2, 2, 2),
    "ragged": ((112, 80), 64, 2, 2, 2),
    "train_py_d2": ((384, 384), 384, 12, 2, 2),
    "vit_b_d1": ((256, 192), 768, 12, 1, 2),
}


def _note(cls, worst, r):
    worst[cls] = max(worst.get(cls, 0.0), r)


def _report(worst):
    for k, v in sorted(worst.items()):
        print(f"worst d/bound {k}: {v:.3g}")


def _fro_ratio(got, want, u, c):
    """||got - want|| / (c u ||want||): <= 1 passes."""
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).norm()) / max(c * u * float(want.norm()), 1e-300)


def _case(name, seed=0, differentiable=True):
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_vit_state
    img, C, heads, depth, B = MODELS[name]
    bb = ScratchViTBackbone(img, 16, embed_dim=C, depth=depth, num_heads=heads, differentiable=differentiable)
    bb.model.load_state_dict(synthetic_vit_state(img, 16, C, depth, seed=seed))
    x = synthetic_crops(B, *img, seed=seed + 1)
    N = (img[0] // 16) * (img[1] // 16)
    ups = torch.randn((B, N, C), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64)
    return bb, x, ups


def _hip_step(bb, x, ups, dtype):
    bb = bb.cuda().set_compute_dtype(dtype).train()
    f = bb.model.forward_features(x.cuda())
    f.backward(ups.float().cuda())
    return f.detach(), {k: p.grad for k, p in bb.model.named_parameters()}


def _bounds(name):
    img, C, heads, depth, B = MODELS[name]
    N = (img[0] // 16) * (img[1] // 16)
    K = max(4 * C, B * N)
    return 2 * VR.n_stages(depth) * math.sqrt(K), 2 * (4 * depth + 2) * math.sqrt(K)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_fp32_step_matches_gauge(name):
    bb, x, ups = _case(name)
    img, C, heads, depth, B = MODELS[name]
    want = VR.vit_step(bb.model.state_dict(), x, ups, patch=16, heads=heads)
    f, grads = _hip_step(bb, x, ups, torch.float32)
    cg, cf = _bounds(name)
    worst = {}
    r = VR.ratio(f, want["features"], VR.U_F32, cf)
    _note("fp32 features", worst, r)
    assert r <= 1.0, ("features", r)
    for k, g in grads.items():
        assert g is not None, k
        r = VR.ratio(g, want["grads"][k], VR.U_F32, cg)
        _note(f"fp32 {VR.grad_class(k)}", worst, r)
        assert r <= 1.0, (name, k, r)
    _report(worst)


def test_fp32_train_forward_matches_eval_forward():
    bb, x, _ = _case("ragged")
    bb = bb.cuda().train()
    xc = x.cuda()
    f = bb.model.forward_features(xc)
    assert f.requires_grad
    with torch.no_grad():
        e = bb.model.forward_features(xc)
    assert float((f.detach() - e).abs().max()) <= 1e-5
    bb.set_compute_dtype(torch.bfloat16)
    fb = bb.model.forward_features(xc).detach()
    with torch.no_grad():
        eb = bb.model.forward_features(xc)
    print(f"bf16 train forward (exact-erf GELU) against the eval path (fitted GELU): max |d| "
          f"{float((fb - eb).abs().max()):.3g}, features max {float(eb.abs().max()):.3g}")


@pytest.mark.parametrize("name", ["tiny", "tiny_hd64", "vit_b_d1"])
def test_bf16_step_within_bound_of_fp32(name):
    bb, x, ups = _case(name)
    _, g32 = _hip_step(bb, x, ups, torch.float32)
    g32 = {k: g.clone() for k, g in g32.items()}
    bb.zero_grad(set_to_none=True)
    _, g16 = _hip_step(bb, x, ups, torch.bfloat16)
    S = VR.n_stages(MODELS[name][3])
    worst = {}
    for k, g in g16.items():
        assert torch.isfinite(g).all(), k
        r = VR.ratio(g, g32[k], VR.U_BF16, 2 * S)
        _note("bf16 vs fp32 max", worst, r)
        assert r <= 1.0, (name, k, r)
        r = _fro_ratio(g, g32[k], VR.U_BF16, 2 * math.sqrt(S))
        _note("bf16 vs fp32 norm-wise", worst, r)
        assert r <= 1.0, (name, k, r)
    _report(worst)


def test_nchw_forward_carries_the_gradient():
    """ScratchViTBackbone.forward's (B, C, gh, gw) map: the same gradients as the token path."""
    bb, x, ups = _case("ragged")
    _, gt = _hip_step(bb, x, ups, torch.float32)
    gt = {k: g.clone() for k, g in gt.items()}
    bb.zero_grad(set_to_none=True)
    out = bb(x.cuda())
    B, C, gh, gw = out.shape
    out.backward(ups.float().cuda().reshape(B, gh, gw, C).permute(0, 3, 1, 2))
    for k, p in bb.model.named_parameters():
        assert torch.equal(p.grad, gt[k]), k


def test_frozen_parameters_get_no_gradient():
    bb, x, ups = _case("tiny")
    bb.model.pos_embed.requires_grad_(False)
    bb.model.patch_embed.requires_grad_(False)
    bb.model.blocks[1].attn.requires_grad_(False)
    _, grads = _hip_step(bb, x, ups, torch.float32)
    for k, p in bb.model.named_parameters():
        assert (p.grad is None) == (not p.requires_grad), k
    # only the last block trainable: nothing below it runs
    bb2, _, _ = _case("tiny")
    bb2.requires_grad_(False)
    bb2.model.blocks[1].mlp.fc2.requires_grad_(True)
    _, grads = _hip_step(bb2, x, ups, torch.float32)
    assert bb2.model.blocks[1].mlp.fc2.weight.grad is not None and bb2.model.blocks[0].norm1.weight.grad is None


def test_gradient_accumulation_over_two_forwards():
    from probpose_pytorch_amd.synthetic import synthetic_crops
    bb, x1, u1 = _case("tiny")
    x2 = synthetic_crops(2, 128, 96, seed=77)
    u2 = torch.randn_like(u1)
    bb = bb.cuda().train()
    singles = []
    for x, u in ((x2, u2), (x1, u1)):
        bb.zero_grad(set_to_none=True)
        bb.model.forward_features(x.cuda()).backward(u.float().cuda())
        singles.append({k: p.grad.clone() for k, p in bb.model.named_parameters()})
    bb.zero_grad(set_to_none=True)
    f1 = bb.model.forward_features(x1.cuda())
    f2 = bb.model.forward_features(x2.cuda())
    f2.backward(u2.float().cuda())
    f1.backward(u1.float().cuda())
    for k, p in bb.model.named_parameters():
        assert torch.equal(p.grad, singles[0][k] + singles[1][k]), k


def test_repeated_steps_are_bit_identical():
    runs = []
    for _ in range(2):
        bb, x, ups = _case("tiny_hd64")
        f, g = _hip_step(bb, x, ups, torch.bfloat16)
        runs.append([f] + [g[k] for k in sorted(g)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_eval_no_grad_and_flag_off_paths_unchanged():
    bb, x, _ = _case("tiny")
    off, _, _ = _case("tiny", differentiable=False)
    bb, off = bb.cuda(), off.cuda()
    xc = x.cuda()
    a = off.train()(xc)
    assert not a.requires_grad
    b = bb.eval()(xc)
    assert not b.requires_grad and torch.equal(a, b)
    with torch.no_grad():
        c = bb.train()(xc)
    assert torch.equal(a, c)


@pytest.mark.parametrize("what", ["fp8", "hd80", "image_grad", "dual_chain"])
def test_unsupported_cases_raise(what, monkeypatch):
    from probpose_pytorch_amd import engine
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    C, heads = (160, 2) if what == "hd80" else (64, 2)
    bb = ScratchViTBackbone((64, 48), 16, embed_dim=C, depth=1, num_heads=heads, differentiable=True).cuda().train()
    x = torch.rand(2, 3, 64, 48, device="cuda")
    match = {"fp8": "float8", "hd80": "head_dim 80", "image_grad": "requires grad", "dual_chain": "DUAL_CHAIN"}[what]
    if what == "fp8":
        bb.set_compute_dtype(torch.float8_e4m3fn)
    if what == "image_grad":
        x.requires_grad_(True)
    if what == "dual_chain":
        monkeypatch.setattr(engine, "DUAL_CHAIN", True)
    with pytest.raises(NotImplementedError, match=match):
        bb(x)


@pytest.mark.parametrize("cfg", [((256, 192), 768, 12, 12, 64), ((384, 384), 384, 12, 12, 32)],
                         ids=["vit_b_bs64", "train_py_bs32"])
def test_full_depth_bf16_step_within_bound_of_fp32(cfg):
    """A full-depth ViT-B bs 64 and train.py's backbone at bs 32: the bf16 step's gradients are finite and agree with
    the fp32 mode's within the bf16 bound."""
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_vit_state
    img, C, heads, depth, B = cfg
    bb = ScratchViTBackbone(img, 16, embed_dim=C, depth=depth, num_heads=heads, differentiable=True)
    bb.model.load_state_dict(synthetic_vit_state(img, 16, C, depth, seed=4))
    bb = bb.cuda()
    x = synthetic_crops(B, *img, seed=5).cuda()
    N = (img[0] // 16) * (img[1] // 16)
    ups = torch.randn((B, N, C), generator=torch.Generator().manual_seed(6)).cuda()
    grads = {}
    for dt in (torch.float32, torch.bfloat16):
        bb.zero_grad(set_to_none=True)
        _, g = _hip_step(bb, x, ups, dt)
        grads[dt] = {k: v.clone() for k, v in g.items()}
    S = VR.n_stages(depth)
    worst = {}
    for k, g in grads[torch.bfloat16].items():
        assert torch.isfinite(g).all(), k
        r = VR.ratio(g, grads[torch.float32][k], VR.U_BF16, 2 * S)
        _note("bf16 vs fp32 full depth max", worst, r)
        assert r <= 1.0, (k, r)
        r = _fro_ratio(g, grads[torch.float32][k], VR.U_BF16, 2 * math.sqrt(S))
        _note("bf16 vs fp32 full depth norm-wise", worst, r)
        assert r <= 1.0, (k, r)
    _report(worst)


def test_inplace_update_before_backward_raises():
    """The backward packs the weights as they are then: an in-place update since the forward must not pass silently."""
    bb, x, ups = _case("tiny")
    bb = bb.cuda().train()
    f = bb.model.forward_features(x.cuda())
    with torch.no_grad():
        bb.model.blocks[0].mlp.fc1.weight.add_(1e-3)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        f.backward(ups.float().cuda())
