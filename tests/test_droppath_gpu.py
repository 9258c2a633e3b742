"""GPU tests of stochastic depth in the training ScratchViTBackbone (``drop_path_rate``; vit_train.py and
csrc/pp_droppath.hip) against the float64 gauge tests/droppath_reference.py, always under the same keep mask.

Models: patch 16, depth 3, rate 0.4, so the blocks' rates are 0, 0.2 and 0.4: a block on today's path next to two
droppable ones.  Masks (bool [depth, 2, B]; block 0 always keeps everything): (a) every crop kept, (b) one crop kept in
every droppable branch, (c) block 1's attention branch and block 2's MLP branch all dropped, (d) mixed, the two
branches of each droppable block differ and a branch keeps B - 1 crops.

Bounds, |got - want| <= c u max|want| per tensor (head_grad_reference.ratio), as tests/test_vit_grad_gpu.py:
* fp32 (u = 2^-24): c = 2 S' sqrt(K), K = max(4C, B N).  S' counts the kernel stages on the longest chain that round
  (droppath_reference.n_stages): vit_grad_reference.n_stages(depth) = 8 depth + 2 = 26, plus per droppable branch
  pp_droppath_add (forward), the scaled pp_crop_rows_gather (the branch's output gradient; the unscaled gather of the
  forward is a copy and rounds nothing) and pp_crop_rows_scatter_add: 3 kernels x 2 branches x 2 droppable blocks = 12.
  S' = 38.  The scale 1 / (1 - p) reaches the kernels rounded to f32 (u relative), inside the stage that applies it.
* bf16 against fp32 mode (u = 2^-8): c = 2 S' against the largest element, and ||got - want|| <= 2 sqrt(S') u ||want||.
A branch that kept no crop gives gradients that are exactly zero.  Each test prints its worst d/bound per class (-s).
"""
import functools
import math

import pytest
import torch

from tests import droppath_reference as DR
from tests import vit_grad_reference as VR

pytestmark = pytest.mark.gpu

RATE, DEPTH = 0.4, 3
MODELS = {
    # name: (img, C, heads, B)
    "tiny": ((128, 96), 64, 2, 4),
    "tiny_hd64": ((128, 96), 128, 2, 4),
    "ragged": ((112, 80), 64, 2, 3),
}
MASKS = "abcd"
S_PRIME = DR.n_stages(DEPTH, 2)


def _mask(kind, B):
    keep = torch.ones((DEPTH, 2, B), dtype=torch.bool)
    if kind == "b":
        keep[1:] = False
        keep[1, 0, 0] = keep[1, 1, B - 1] = keep[2, 0, 1] = keep[2, 1, 0] = True
    elif kind == "c":
        keep[1, 0] = False
        keep[2, 1] = False
    elif kind == "d":
        keep[1, 0] = torch.tensor([1, 0, 1, 1][:B], dtype=torch.bool)
        keep[1, 1] = torch.tensor([0, 1, 1, 0][:B], dtype=torch.bool)
        keep[2, 0] = torch.tensor([0, 1, 0, 1][:B], dtype=torch.bool)
        keep[2, 1] = torch.tensor([1, 1, 0, 1][:B], dtype=torch.bool)
    return keep


def _note(cls, worst, r):
    worst[cls] = max(worst.get(cls, 0.0), r)


def _report(worst):
    for k, v in sorted(worst.items()):
        print(f"worst d/bound {k}: {v:.3g}")


def _fro_ratio(got, want, u, c):
    got, want = got.double().cpu(), want.double().cpu()
    err = float((got - want).norm())
    return err / max(c * u * float(want.norm()), 1e-300)


def _geom(name):
    img, C, heads, B = MODELS[name]
    return img, C, heads, B, (img[0] // 16) * (img[1] // 16)


def _case(name, seed=0, rate=RATE, depth=DEPTH, **kw):
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_vit_state
    img, C, heads, B, N = _geom(name)
    if rate is not None:
        kw["drop_path_rate"] = rate
    bb = ScratchViTBackbone(img, 16, embed_dim=C, depth=depth, num_heads=heads, differentiable=True, **kw)
    bb.model.load_state_dict(synthetic_vit_state(img, 16, C, depth, seed=seed))
    x = synthetic_crops(B, *img, seed=seed + 1)
    ups = torch.randn((B, N, C), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64)
    return bb, x, ups


@functools.lru_cache(maxsize=None)
def _gauge(name, kind, seed=0):
    """The float64 step of model ``name`` under mask ``kind``, computed once and shared (never modified)."""
    bb, x, ups = _case(name, seed)
    return DR.vit_step_droppath(bb.model.state_dict(), x, ups, _mask(kind, x.shape[0]), bb.drop_path_rates, patch=16,
                                heads=MODELS[name][2])


def _hip_step(bb, x, ups, dtype, keep):
    """features (B, N, C) f32 and the parameters' gradients of one training step under the mask ``keep``."""
    from probpose_pytorch_amd import vit_train
    bb = bb.cuda().set_compute_dtype(dtype).train()
    t = vit_train.train_forward(bb.model, x.cuda(), keep=keep)
    t.backward(ups.reshape(t.shape).to(t.dtype).cuda())
    if keep is not None:
        assert torch.equal(bb.last_drop_path_keep, keep)
    return t.detach().float().reshape(ups.shape), {k: p.grad for k, p in bb.model.named_parameters()}


def _cpu_state(bb):
    return {k: v.detach().cpu() for k, v in bb.model.state_dict().items()}


def _c32(name):
    _, C, _, B, N = _geom(name)
    return 2 * S_PRIME * math.sqrt(max(4 * C, B * N))


def _check_fp32(name, f, grads, want, worst, scale=1.0):
    c = _c32(name) * scale
    if f is not None:
        r = VR.ratio(f, want["features"], VR.U_F32, c)
        _note("fp32 features", worst, r)
        assert r <= 1.0, ("features", r)
    for k, w in want["grads"].items():
        assert grads[k] is not None, k
        r = VR.ratio(grads[k], w, VR.U_F32, c)
        _note(f"fp32 {VR.grad_class(k)}", worst, r)
        assert r <= 1.0, (name, k, r)


def _dropped_parameters(kind):
    if kind != "c":
        return []
    return ([f"blocks.1.{p}" for p in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias",
                                       "attn.proj.weight", "attn.proj.bias")]
            + [f"blocks.2.{p}" for p in ("norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                                         "mlp.fc2.weight", "mlp.fc2.bias")])


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_fp32_step_matches_gauge(name, kind):
    bb, x, ups = _case(name)
    f, grads = _hip_step(bb, x, ups, torch.float32, _mask(kind, x.shape[0]))
    worst = {}
    _check_fp32(name, f, grads, _gauge(name, kind), worst)
    for k in _dropped_parameters(kind):
        assert grads[k].shape == dict(bb.model.named_parameters())[k].shape
        assert int(torch.count_nonzero(grads[k])) == 0, k
    _report(worst)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_bf16_step_within_bound_of_fp32(name, kind):
    bb, x, ups = _case(name)
    keep = _mask(kind, x.shape[0])
    _, g32 = _hip_step(bb, x, ups, torch.float32, keep)
    g32 = {k: g.clone() for k, g in g32.items()}
    bb.zero_grad(set_to_none=True)
    _, g16 = _hip_step(bb, x, ups, torch.bfloat16, keep)
    worst = {}
    for k, g in g16.items():
        assert torch.isfinite(g).all(), k
        r = VR.ratio(g, g32[k], VR.U_BF16, 2 * S_PRIME)
        _note("bf16 vs fp32 max", worst, r)
        assert r <= 1.0, (name, k, r)
        r = _fro_ratio(g, g32[k], VR.U_BF16, 2 * math.sqrt(S_PRIME))
        _note("bf16 vs fp32 norm-wise", worst, r)
        assert r <= 1.0, (name, k, r)
    for k in _dropped_parameters(kind):
        assert int(torch.count_nonzero(g16[k])) == 0, k
    _report(worst)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rate_zero_is_the_path_without_the_argument(dtype):
    with_arg, x, ups = _case("tiny", rate=0.0)
    without, _, _ = _case("tiny", rate=None)
    fa, ga = _hip_step(with_arg, x, ups, dtype, None)
    fb, gb = _hip_step(without, x, ups, dtype, None)
    assert with_arg.last_drop_path_keep is None and without.last_drop_path_keep is None
    assert with_arg.drop_path_rates == [0.0] * DEPTH
    assert torch.equal(fa, fb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_public_path_draws_the_mask_from_the_default_generator():
    from probpose_pytorch_amd.vit_train import draw_keep
    name = "tiny"
    bb, x, ups = _case(name)
    _, C, heads, B, N = _geom(name)
    bb = bb.cuda().train()
    torch.manual_seed(7)
    out = bb(x.cuda())
    keep = bb.last_drop_path_keep
    torch.manual_seed(7)
    assert torch.equal(keep, draw_keep(bb.drop_path_rates, B))
    assert not bool(keep.all()), "seed 7 keeps every crop: the test would not see a drop"
    _, _, gh, gw = out.shape
    out.backward(ups.float().cuda().reshape(B, gh, gw, C).permute(0, 3, 1, 2))
    want = DR.vit_step_droppath(_cpu_state(bb), x, ups, keep, bb.drop_path_rates, patch=16, heads=heads)
    f = out.detach().permute(0, 2, 3, 1).reshape(B, N, C)
    worst = {}
    _check_fp32(name, f, {k: p.grad for k, p in bb.model.named_parameters()}, want, worst)
    _report(worst)


def test_eval_and_no_grad_are_untouched():
    bb, x, _ = _case("ragged")
    plain, _, _ = _case("ragged", rate=0.0)
    bb, plain = bb.cuda(), plain.cuda()
    xc = x.cuda()
    a = plain.eval()(xc).clone()
    b = bb.eval()(xc)
    assert not b.requires_grad and torch.equal(a, b)
    with torch.no_grad():
        c = bb.train()(xc)
    assert not c.requires_grad and torch.equal(a, c)
    assert bb.last_drop_path_keep is None


def test_repeated_steps_are_bit_identical():
    runs = []
    for _ in range(2):
        bb, x, ups = _case("tiny_hd64")
        f, g = _hip_step(bb, x, ups, torch.bfloat16, _mask("d", x.shape[0]))
        runs.append([f] + [g[k] for k in sorted(g)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_frozen_lower_layers():
    """Only block 2 and the final norm train, mask (d): nothing below block 2 gets a gradient (or runs)."""
    name = "tiny"
    bb, x, ups = _case(name)
    trainable = lambda k: k.startswith("blocks.2.") or k.startswith("norm.")  # noqa: E731
    for k, p in bb.model.named_parameters():
        p.requires_grad_(trainable(k))
    keep = _mask("d", x.shape[0])
    _, grads = _hip_step(bb, x, ups, torch.float32, keep)
    want = DR.vit_step_droppath(_cpu_state(bb), x, ups, keep, bb.drop_path_rates, patch=16,
                                heads=MODELS[name][2], trainable=trainable)
    assert sorted(want["grads"]) == sorted(k for k in grads if trainable(k))
    for k, g in grads.items():
        assert (g is None) == (not trainable(k)), k
    worst = {}
    _check_fp32(name, None, grads, want, worst)
    _report(worst)


def test_two_forwards_then_two_backwards_with_different_masks():
    from probpose_pytorch_amd import vit_train
    from probpose_pytorch_amd.synthetic import synthetic_crops
    name = "tiny"
    bb, x1, u1 = _case(name)
    img, C, heads, B, N = _geom(name)
    x2 = synthetic_crops(B, *img, seed=77)
    u2 = torch.randn(u1.shape, generator=torch.Generator().manual_seed(78), dtype=torch.float64)
    k1, k2 = _mask("d", B), _mask("b", B)
    sd = bb.model.state_dict()
    w1 = _gauge(name, "d")
    w2 = DR.vit_step_droppath(sd, x2, u2, k2, bb.drop_path_rates, patch=16, heads=heads)
    bb = bb.cuda().train()
    f1 = vit_train.train_forward(bb.model, x1.cuda(), keep=k1)
    f2 = vit_train.train_forward(bb.model, x2.cuda(), keep=k2)
    assert torch.equal(bb.last_drop_path_keep, k2)
    f2.backward(u2.float().reshape(f2.shape).cuda())
    f1.backward(u1.float().reshape(f1.shape).cuda())
    c, worst = _c32(name), 0.0
    for k, p in bb.model.named_parameters():
        a, b = w1["grads"][k], w2["grads"][k]
        bound = c * VR.U_F32 * (float(a.abs().max()) + float(b.abs().max()))      # the two steps' bounds, added
        d = float((p.grad.double().cpu() - (a + b)).abs().max())
        worst = max(worst, d / bound)
        assert d <= bound, (k, d / bound)
    print(f"worst d/bound two forwards, two backwards: {worst:.3g}")
    with pytest.raises(RuntimeError, match="twice"):
        f1.backward(u1.float().reshape(f1.shape).cuda())


def test_inplace_update_before_backward_raises():
    from probpose_pytorch_amd import vit_train
    bb, x, ups = _case("tiny")
    bb = bb.cuda().train()
    f = vit_train.train_forward(bb.model, x.cuda(), keep=_mask("d", x.shape[0]))
    with torch.no_grad():
        bb.model.blocks[2].mlp.fc1.weight.add_(1e-3)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        f.backward(ups.float().reshape(f.shape).cuda())


def test_training_step_does_no_host_sync():
    from probpose_pytorch_amd import vit_train
    bb, x, ups = _case("tiny")
    bb = bb.cuda().set_compute_dtype(torch.bfloat16).train()
    xc = x.cuda()
    keep = _mask("d", x.shape[0])
    up = ups.reshape(-1, ups.shape[-1]).to(torch.bfloat16).cuda()
    vit_train.train_forward(bb.model, xc, keep=keep).backward(up)        # warm-up: code objects, pinned memory
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        vit_train.train_forward(bb.model, xc, keep=keep).backward(up)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in bb.model.parameters())


def test_train_py_loop_with_drop_path():
    """train.py's loop at depth 2 with drop_path_rate 0.1, the differentiable head and loss and FusedAdamW: six steps
    on a fixed batch, finite losses, the last below the first."""
    import numpy as np

    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.loss import ProbPoseLoss
    from probpose_pytorch_amd.model import ProbPoseModel
    from probpose_pytorch_amd.optim import FusedAdamW
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_head_state, synthetic_vit_state
    from tests import loss_grad_reference as LG
    from tests import loss_reference as LR
    B, K, C, heads, depth, size = 4, 20, 384, 12, 2, (384, 384)
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
    backbone = ScratchViTBackbone(size, 16, embed_dim=C, depth=depth, num_heads=heads, drop_path_rate=0.1,
                                  differentiable=True)
    backbone.model.load_state_dict(synthetic_vit_state(size, 16, C, depth, seed=12))
    head = ProbMapHead(C, K, pools, (256, 256), (4, 4), final_layer_kernel_size=1, freeze_error=True,
                       normalize=1.0, differentiable=True)
    head.load_state_dict(synthetic_head_state(C, K, n_pools=3, deconv_out=(256, 256), seed=13), strict=False)
    model = ProbPoseModel(backbone, head).cuda().train()
    xc = synthetic_crops(B, *size, seed=14).cuda()
    opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=3e-4, max_grad_norm=1.0)
    torch.manual_seed(5)
    hist, kept = [], []
    for _ in range(6):
        opt.zero_grad()
        losses = loss_fn(gt, model(xc))
        loss = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
        kept.append(int(backbone.last_drop_path_keep.sum()))
    print("losses", [round(v, 4) for v in hist], "kept branches of", 2 * depth * B, "per step:", kept)
    assert backbone.last_drop_path_keep.shape == (depth, 2, B)
    assert all(math.isfinite(v) for v in hist) and hist[-1] < hist[0], hist
