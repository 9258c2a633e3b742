"""GPU tests of the training ProbMapHead (``ProbMapHead(differentiable=True)`` in ``.train()`` mode, head_train.py and
csrc/pp_head_grad.hip) against the float64 restatement of the reference's train-mode step (tests/head_grad_reference.py,
itself pinned on tests/golden/head_grad.npz minted from the unmodified reference head).

Bounds, |got - want| <= c u max|want| per tensor (head_grad_reference.ratio):
* fp32 (exact-fp32 MFMA), u = 2^-24: c = 64 for the outputs and running statistics, 512 for gradients (chains of up
  to ten reductions of depth <= 9 C, each adding ~sqrt(depth) u of norm-wise error).
* bf16, u = 2^-8: c = 2 L 4^n.  Every GEMM layer on a value's chain rounds both operands to bf16 (2 u relative per
  product, accumulation in f32): 2 L for L layers.  Each train-mode BatchNorm on the chain divides by the batch
  standard deviation and its backward subtracts two batch means, which can amplify a relative error by up to 4: 4^n
  for n BNs.  Longest chains: a gradient (the first deconvolution's weight: deconv0, deconv1, final forward, their
  three backward GEMMs, 2 BNs; the first aux stage's weight likewise) L = 6, n = 2: c = 192.  An output (the heatmap:
  3 layers, 2 BNs): c = 96.  The running statistics (at most 2 rounded layers, 1 BN): c = 16.
* The conv bias ahead of a train-mode BN, and the final layer's bias under Sparsemax (whose backward sums to zero over
  each map): the true gradient is 0; |got| <= c u sum_m |dY(m, n)| with c = 16: each
  dY element carries the BN backward's own roundings (the two mean subtractions, the products: ~6 u relative to its
  terms, which are at most |dY|-sized) and the column sum rounds once per slab and once per split partial.
"""
import copy

import numpy as np
import pytest
import torch

from tests import head_grad_reference as HR

pytestmark = pytest.mark.gpu

GOLD = "tests/golden/head_grad.npz"
C_OUT = {torch.float32: 64, torch.bfloat16: 96}
C_STATS = {torch.float32: 64, torch.bfloat16: 16}
C_GRAD = {torch.float32: 512, torch.bfloat16: 192}
C_BIAS = 16
U = {torch.float32: HR.U_F32, torch.bfloat16: HR.U_BF16}
_WORST: dict = {}


@pytest.fixture(scope="module")
def golden():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return np.load(os.path.join(root, GOLD))


def _hip_step(head, feats, ups, xg, dtype):
    head = head.cuda().set_compute_dtype(dtype).train()
    x = feats.cuda().requires_grad_(xg)
    outs = head(x)
    pairs = [(o, u.cuda()) for o, u in zip(outs, ups) if u is not None]
    torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])
    return head, [o.detach() for o in outs], x


def _note(cls, r):
    _WORST[cls] = max(_WORST.get(cls, 0.0), r)


def _compare(name, golden, dtype, **extra):
    head, feats, ups, cfg, xg = HR.case(name, differentiable=True, **extra)
    state = copy.deepcopy(head.state_dict())
    want = HR.head_step(state, cfg, feats, ups, HR.trainable_of(head), xg)
    head, outs, x = _hip_step(head, feats, ups, xg, dtype)
    u, co, cg = U[dtype], C_OUT[dtype], C_GRAD[dtype]
    tag = "fp32" if dtype == torch.float32 else "bf16"
    for i, (o, w) in enumerate(zip(outs, want["outputs"])):
        r = HR.ratio(o, w, u, co)
        _note(f"{tag} out", r)
        assert r <= 1.0, (name, "output", i, r)
    for k, p in head.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        if k in want["dy_mag"]:
            bound = C_BIAS * u * want["dy_mag"][k]
            r = float((p.grad.double().cpu().abs() / bound.clamp_min(1e-300)).max())
            _note(f"{tag} pre-BN bias", r)
        else:
            r = HR.ratio(p.grad, want["grads"][k], u, cg)
            _note(f"{tag} {HR.grad_class(k)}", r)
        assert r <= 1.0, (name, k, r)
    if xg:
        r = HR.ratio(x.grad, want["x_grad"], u, cg)
        _note(f"{tag} x", r)
        assert r <= 1.0, (name, "x", r)
    bufs = dict(head.named_buffers())
    for k, v in want["running"].items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v), k
            continue
        r = HR.ratio(bufs[k], v, u, C_STATS[dtype])
        _note(f"{tag} stats", r)
        assert r <= 1.0, (name, k, r)
    return head, outs, x


@pytest.mark.parametrize("name", sorted(HR.CASES))
def test_fp32_train_step_matches_restatement(golden, name):
    _compare(name, golden, torch.float32)


@pytest.mark.parametrize("name", ["T1", "T2", "T4"])
def test_bf16_train_step_within_bound(golden, name):
    _compare(name, golden, torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_normalize_sparsemax_train_step(golden, dtype):
    _compare("T4", golden, dtype, normalize=1.0)


def test_frozen_parameters_and_detached_branches(golden):
    head, feats, ups, cfg, _ = HR.case("T3", differentiable=True)
    head, _, _ = _hip_step(head, feats, ups, False, torch.float32)
    for k, p in head.error_layers.named_parameters():
        assert p.grad is None, k
    # the default detaches: gradients of the four aux outputs alone send nothing to x
    head, feats, ups, cfg, _ = HR.case("T1", differentiable=True)
    head, _, x = _hip_step(head, feats, [None] + ups[1:], True, torch.float32)
    assert x.grad is not None and float(x.grad.abs().max()) == 0.0
    assert head.probability_layers[0].weight.grad is not None


def test_repeated_steps_are_bit_identical(golden):
    grads = []
    for _ in range(2):
        head, feats, ups, cfg, _ = HR.case("T2", differentiable=True)
        head, outs, x = _hip_step(head, feats, ups, True, torch.bfloat16)
        grads.append([p.grad.clone() for p in head.parameters()] + outs + [x.grad.clone()]
                     + [b.clone() for b in head.buffers()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_eval_and_flag_off_paths_unchanged(golden):
    head, feats, _, _, _ = HR.case("T1")
    head2 = copy.deepcopy(head)
    head2.differentiable = True
    x = feats.cuda()
    for dt in (torch.float32, torch.bfloat16):
        a = head.cuda().set_compute_dtype(dt).eval()(x)
        b = head2.cuda().set_compute_dtype(dt).eval()(x)
        for u, v in zip(a, b):
            assert torch.equal(u, v) and not v.requires_grad
    with pytest.raises(RuntimeError, match="eval"):
        head.train()(x)


@pytest.mark.parametrize("kw,what", [
    (dict(conv_out_channels=(64,), conv_kernel_sizes=(3,)), "conv_out_channels"),
    (dict(deconv_kernel_sizes=(3, 3)), "deconvolution kernel 3"),
    (dict(deconv_kernel_sizes=(2, 2)), "deconvolution kernel 2"),
    (dict(final_layer_kernel_size=3), "final_layer_kernel_size=3"),
    (dict(final_layer_kernel_size=None, deconv_out_channels=(64, 5)), "final_layer_kernel_size=None"),
])
def test_unsupported_constructions_raise(kw, what):
    from probpose_pytorch_amd.head import ProbMapHead
    args = dict(deconv_out_channels=(64, 64), deconv_kernel_sizes=(4, 4))
    args.update(kw)
    head = ProbMapHead(64, 5, [(4, 3), (2, 2)], differentiable=True, **args).cuda().train()
    with pytest.raises(NotImplementedError, match=what):
        head(torch.randn(2, 64, 8, 6, device="cuda"))


def test_fp8_compute_dtype_raises():
    from probpose_pytorch_amd.head import ProbMapHead
    head = ProbMapHead(64, 5, [(4, 3), (2, 2)], (64, 64), (4, 4), differentiable=True).cuda().train()
    head.set_compute_dtype(torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError, match="float8"):
        head(torch.randn(2, 64, 8, 6, device="cuda"))


def test_trained_head_eval_matches_oracle(golden):
    from oracle import probpose_oracle as orc
    head, feats, ups, cfg, _ = HR.case("T1", differentiable=True)
    head = head.cuda().train()
    opt = torch.optim.SGD(head.parameters(), lr=1e-2)
    x = feats.cuda()
    for _ in range(3):
        opt.zero_grad()
        outs = head(x)
        torch.autograd.backward(list(outs), [u.cuda() for u in ups])
        opt.step()
    assert int(head.deconv_layers[1].num_batches_tracked) == 3
    got = head.eval()(x)
    sd = {k: v.detach().cpu() for k, v in head.state_dict().items()}
    with torch.no_grad():
        want = orc.head_forward(sd, feats, pools=cfg["pools"], n_deconv=2)
    for g, w in zip(got, want):
        assert float((g.cpu() - w).abs().max()) <= 1e-4


def test_model_refuses_unfrozen_hip_backbone():
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.model import ProbPoseModel
    from probpose_pytorch_amd.synthetic import synthetic_model_state
    bb = ScratchViTBackbone((128, 96), 16, embed_dim=64, depth=1, num_heads=2)
    head = ProbMapHead(64, 5, [(4, 3), (2, 2)], (64, 64), (4, 4), differentiable=True)
    model = ProbPoseModel(bb, head).cuda().train()
    x = torch.randn(2, 3, 128, 96, device="cuda")
    with pytest.raises(RuntimeError, match=r"model\.backbone\.requires_grad_\(False\)"):
        model(x)
    model.backbone.requires_grad_(False)
    outs = model(x)
    sum(o.sum() for o in outs).backward()
    assert head.final_layer.weight.grad is not None
    with torch.no_grad():
        model.backbone.requires_grad_(True)
        model(x)                     # no grad: nothing is silently skipped, so it runs


def test_vit_b_bench_head_bf16_step():
    """The ViT-B bench head (C = 768, 16x12 features, K = 17) at batch 64: one bf16 training step runs, its gradients
    are finite and agree with the fp32 mode within the bf16 bound."""
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.synthetic import synthetic_features, synthetic_head_state
    C, K, pools = 768, 17, [(4, 3), (2, 2), (2, 2)]
    grads = {}
    feats = synthetic_features(64, C, 16, 12, seed=5).cuda()
    g = torch.Generator().manual_seed(6)
    ups = None
    for dt in (torch.float32, torch.bfloat16):
        head = ProbMapHead(C, K, pools, (256, 256), (4, 4), differentiable=True)
        head.load_state_dict(synthetic_head_state(C, K, n_pools=3, deconv_out=(256, 256), seed=5), strict=False)
        head = head.cuda().set_compute_dtype(dt).train()
        outs = head(feats)
        if ups is None:
            ups = [torch.randn(o.shape, generator=g).cuda() for o in outs]
        torch.autograd.backward(list(outs), ups)
        grads[dt] = {k: p.grad for k, p in head.named_parameters()}
    for k, gb in grads[torch.bfloat16].items():
        assert torch.isfinite(gb).all(), k
        if k.endswith(".bias") and "_layers." in k and int(k.split(".")[1]) % 4 == 0 and not k.startswith("deconv"):
            idx = int(k.split(".")[1])
            if idx < 4 * len(pools):
                continue            # zero up to rounding: no relative comparison
        r = HR.ratio(gb, grads[torch.float32][k], HR.U_BF16, C_GRAD[torch.bfloat16])
        _note("bf16-vs-fp32 ViT-B", r)
        assert r <= 1.0, (k, r)


def test_train_py_head_loop_loss_falls():
    """train.py's head (train.py:166-180: C = 384, K = 20, pools (4, 4), (2, 2), (2, 2), two k4 deconvolutions,
    freeze_error, normalize = 1.0) on a fixed batch of 24x24 features through ProbPoseLoss(freeze_error=True,
    differentiable=True) with LOSS_WEIGHTS, AdamW and clip_grad_norm_: every step's prediction gradients meet the loss
    restatement's bound, the first step's head gradients meet the head restatement's bound, and the weighted loss
    falls.  (Later steps' head gradients are not held to the norm-wise bound: as the branches fit, the BN backward's
    mean subtractions cancel the first aux convolutions' gradients to a few times below the magnitude of their terms,
    where f32 rounding of the terms exceeds c u max|gradient|.)"""
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.loss import ProbPoseLoss
    from probpose_pytorch_amd.synthetic import synthetic_features, synthetic_head_state
    from tests import loss_grad_reference as LG
    from tests import loss_reference as LR
    B, K, C, H, W, size = 3, 20, 384, 96, 96, (384, 384)
    rng = np.random.default_rng(7)
    kps = rng.uniform(20, 364, (B, K, 2)).astype(np.float32)
    annotated = rng.random((B, K)) > 0.2
    vis = (rng.random((B, K)) > 0.3).astype(np.float32)
    gt_hm, in_image = LR.encode_probmaps(kps, annotated.astype(np.float32), size, (W, H))
    gt_np = dict(heatmaps=gt_hm, in_image=in_image[:, None, :], keypoints_visible=annotated[:, None, :],
                 keypoints_visibility=vis[:, None, :])
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in gt_np.items()}
    sigmas = np.full(K, 0.05)
    loss_fn = ProbPoseLoss(Codec(ArgMaxProbMap(size, (W, H), sigmas)), freeze_error=True, differentiable=True)
    torch.manual_seed(3)
    head = ProbMapHead(C, K, [(4, 4), (2, 2), (2, 2)], (256, 256), (4, 4), final_layer_kernel_size=1,
                       freeze_error=True, normalize=1.0, differentiable=True)
    # seeded weights of unit-scale activations (the reference's N(0, 0.001) start leaves nearly flat maps whose
    # Sparsemax and BN backwards cancel to far below the magnitude of their terms, out of reach of a norm-wise bound)
    head.load_state_dict(synthetic_head_state(C, K, n_pools=3, deconv_out=(256, 256), seed=3), strict=False)
    head = head.cuda().train()
    cfg = dict(pools=[(4, 4), (2, 2), (2, 2)], n_deconv=2, normalize=1.0)
    feats = synthetic_features(B, C, 24, 24, seed=8)
    x = feats.cuda()
    opt = torch.optim.AdamW(head.parameters(), lr=1e-3)
    hist = []
    steps = 20
    for step in range(steps):
        opt.zero_grad()
        state = ({k: v.detach().cpu().clone() for k, v in head.state_dict().items()}
                 if step == 0 else None)
        pred = head(x)
        if state is not None:       # the forward's own pooling picks (near-ties of its float32 values)
            cfg["pool_decide"] = HR.pool_decisions(pred[0].grad_fn.saved, C, cfg["pools"], B, 24, 24)
        for p in pred:
            p.retain_grad()
        losses = loss_fn(gt, pred)
        loss = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
        loss.backward()
        hist.append(float(loss.detach()))
        with torch.no_grad():
            T = loss_fn.terms(gt, pred)
        pn = [p.detach().cpu().numpy() for p in pred]
        R = LG.probpose_loss_grads(gt_np, pn, T["gt_oks"].cpu().numpy(), T["gt_err"].cpu().numpy())
        for key, g in zip(LG.PRED_KEYS, [p.grad for p in pred]):
            assert LR.ratio(g.detach().cpu().numpy().reshape(R[key][0].shape), *R[key]) <= 1.0, (step, key)
        if state is not None:
            ups = [p.grad.detach().cpu() for p in pred]
            want = HR.head_step(state, cfg, feats, ups, HR.trainable_of(head), False)
            for k, p in head.named_parameters():
                if not p.requires_grad:
                    assert p.grad is None, k
                    continue
                if k in want["dy_mag"]:
                    r = float((p.grad.double().cpu().abs() / (C_BIAS * HR.U_F32 * want["dy_mag"][k]).clamp_min(1e-300)).max())
                else:
                    r = HR.ratio(p.grad, want["grads"][k], HR.U_F32, C_GRAD[torch.float32])
                _note("fp32 train.py loop", r)
                assert r <= 1.0, (step, k, r)
        torch.nn.utils.clip_grad_norm_(head.parameters(), 1.0)
        opt.step()
    assert hist[-1] < 0.9 * hist[0], hist


def test_report_worst_ratios():
    """Prints the worst d/bound per gradient class of the tests above (run with -s)."""
    for k, v in sorted(_WORST.items()):
        print(f"worst d/bound {k}: {v:.3g}")
