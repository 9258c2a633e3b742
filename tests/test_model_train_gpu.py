"""train.py's training loop on the GPU with the whole model trainable: ProbPoseModel(ScratchViTBackbone(...,
differentiable=True), ProbMapHead(..., differentiable=True)), ProbPoseLoss(differentiable=True) with LOSS_WEIGHTS,
AdamW and clip_grad_norm_, at reduced depth on a fixed batch.

Bounds: the first step's gradients against the composed float64 gauge (tests/vit_grad_reference.model_step) with the
fp32 constants of tests/test_vit_grad_gpu.py (backbone) and tests/test_head_grad_gpu.py (head: c = 512, and the conv
biases ahead of a train-mode BN at 16 u sum_m |dY|).  The head's bound is the head test's: the float64 head here takes
the float64 backbone's features, which differ from the GPU's by the backbone's own fp32 bound (~1e-5 relative),
far below the head's 512 u (3e-5) after its normalisations.
"""
import math

import numpy as np
import pytest
import torch

from tests import head_grad_reference as HR
from tests import vit_grad_reference as VR

pytestmark = pytest.mark.gpu


def test_train_py_loop_reduced_depth():
    from oracle import probpose_oracle as orc
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
    cfg = dict(pools=pools, n_deconv=2, normalize=1.0)
    x = synthetic_crops(B, *size, seed=14)
    xc = x.cuda()
    opt = torch.optim.AdamW(model.parameters(), lr=3e-4)
    hist = []
    for step in range(6):
        opt.zero_grad()
        state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()} if step == 0 else None
        pred = model(xc)
        for p in pred:
            p.retain_grad()
        losses = loss_fn(gt, pred)
        loss = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
        loss.backward()
        hist.append(float(loss.detach()))
        if state is not None:
            cfg["pool_decide"] = HR.pool_decisions(pred[0].grad_fn.saved, C, pools, B, 24, 24)
            vs = {k[len("backbone.model."):]: v for k, v in state.items() if k.startswith("backbone.model.")}
            hs = {k[len("head."):]: v for k, v in state.items() if k.startswith("head.")}
            ups = [p.grad.detach().cpu() for p in pred]
            want = VR.model_step(vs, hs, cfg, x, ups, patch=16, heads=heads,
                                 head_trainable=HR.trainable_of(head))
            N = (size[0] // 16) * (size[1] // 16)
            cg = 2 * VR.n_stages(depth) * math.sqrt(max(4 * C, B * N))
            for k, p in model.backbone.model.named_parameters():
                assert p.grad is not None, k
                r = VR.ratio(p.grad, want["vit_grads"][k], VR.U_F32, cg)
                assert r <= 1.0, ("backbone", k, r)
            for k, p in head.named_parameters():
                if not p.requires_grad:
                    assert p.grad is None, k
                    continue
                if k in want["dy_mag"]:
                    r = float((p.grad.double().cpu().abs()
                               / (16 * HR.U_F32 * want["dy_mag"][k]).clamp_min(1e-300)).max())
                else:
                    r = HR.ratio(p.grad, want["head_grads"][k], HR.U_F32, 512)
                assert r <= 1.0, ("head", k, r)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
    assert hist[-1] < hist[0], hist
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
