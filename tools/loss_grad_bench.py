#!/usr/bin/env python3
"""Time the loss backward on the device: pp_oks_heatmap_loss_backward (ProbPoseLoss's pixel-mean reduction and the
per-keypoint one) beside the forward pp_oks_heatmap_loss, pp_probpose_loss_grads, forward + backward of
ProbPoseLoss(differentiable=True) with train.py's LOSS_WEIGHTS, and torch autograd through a torch formulation of the
same heatmap loss as a yardstick.  Shapes: B=64, K=17, 64x48 and train.py's B=32, K=20, 96x96.  Prints one JSON line:
us per call and, for the kernels, bytes moved and TB/s against the 8 TB/s HBM roofline.  `--once`: one of each, for
`rocprofv3 --kernel-trace` launch counts."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as g

g.build()
from probpose.codec import ArgMaxProbMap, Codec, ProbMap
from probpose.loss import ProbPoseLoss
from probpose_pytorch_amd import _lib
from probpose_pytorch_amd.loss import _RED_KEYPOINT, _RED_PIXEL_MEAN, _oks_heatmap_loss, _oks_heatmap_loss_backward
from tests import loss_reference as LR

once = "--once" in sys.argv
WEIGHTS = {"kpt": 1.0, "probability": 1.0, "visibility": 0.0, "oks": 1.0, "error": 1.0}     # train.py:26-32


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3      # us


def torch_heatmap_loss(o, t, w, sw=0.05):
    """OKSHeatmapLoss per pixel (oks 'minus', loss.py:92-127) in torch ops, then its mean."""
    B, K, H, W = o.shape
    m = w.view(B, K, 1, 1)
    sx = torch.tensor([[1, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=o.dtype, device=o.device).view(1, 1, 3, 3)
    sy = torch.tensor([[1, 2, 1], [0, 0, 0], [-1, -2, -1]], dtype=o.dtype, device=o.device).view(1, 1, 3, 3)
    x = o.reshape(B * K, 1, H, W)
    gr = (F.conv2d(x, sx, padding="same") ** 2 + F.conv2d(x, sy, padding="same") ** 2).reshape(B, K, H, W)
    return (sw * (gr * m) + (1 - sw) * (o * (1 - t) * m)).mean()


def setup(B, K, H, W, input_size, sigmas, codec_cls, seed=0):
    rng = np.random.default_rng(seed)
    kps = rng.uniform(-10, min(input_size) + 10, (B, K, 2)).astype(np.float32)
    annotated = rng.random((B, K)) > 0.2
    gt_hm, in_image = LR.encode_probmaps(kps, annotated.astype(np.float32), input_size, (W, H))
    dt_hm = np.clip(gt_hm * 0.8 + rng.random((B, K, H, W), dtype=np.float32) * 0.1, 0, 1).astype(np.float32)
    heads = [rng.uniform(0.01, 0.99, (B, K, 1, 1)).astype(np.float32) for _ in range(4)]
    gt = dict(heatmaps=torch.from_numpy(gt_hm).cuda(), in_image=torch.from_numpy(in_image[:, None]).cuda(),
              keypoints_visible=torch.from_numpy(annotated[:, None]).cuda(),
              keypoints_visibility=torch.from_numpy((rng.random((B, 1, K)) > 0.5).astype(np.float32)).cuda())
    pred = [torch.from_numpy(p).cuda() for p in (dt_hm, *heads)]
    loss_fn = ProbPoseLoss(Codec(codec_cls(input_size, (W, H), sigmas)), freeze_error=True, differentiable=True)
    return gt, pred, loss_fn


def bench_shape(tag, B, K, H, W, input_size, sigmas, codec_cls, res):
    gt, pred, loss_fn = setup(B, K, H, W, input_size, sigmas, codec_cls)
    out, tgt = pred[0], gt["heatmaps"]
    kw = torch.ones((B, K), device="cuda")
    sc = torch.empty(3, device="cuda")
    u = torch.ones((), device="cuda")
    ukp = torch.ones((B, K), device="cuda")
    leaves = [p.clone().requires_grad_(True) for p in pred]

    def fwd_kernel():
        _oks_heatmap_loss(out, tgt, kw, None, False, "minus", 0.05, 0.0, 1.0, None, None, sc)

    def bwd_kernel():
        _oks_heatmap_loss_backward(out, tgt, kw, None, False, "minus", 0.05, 0.0, 1.0, _RED_PIXEL_MEAN, u)

    def bwd_kernel_kp():
        _oks_heatmap_loss_backward(out, tgt, kw, None, False, "minus", 0.05, 0.0, 1.0, _RED_KEYPOINT, ukp)

    T = loss_fn.terms(gt, pred)
    N = B * K
    d = torch.empty((4, N), device="cuda")
    ups = [torch.ones((), device="cuda") for _ in range(4)]

    def heads_kernel():
        rc = _lib.lib().pp_probpose_loss_grads(
            *[_lib.ptr(t) for t in (*T["heads"], T["gt_oks"], T["gt_err"], T["masks"][0], T["masks"][1],
                                    T["masks"][2], *ups)], B, K, *[_lib.ptr(d[i]) for i in range(4)],
            _lib.stream_ptr())
        _lib.check(rc, "pp_probpose_loss_grads")

    def fwd_bwd():
        for p in leaves:
            p.grad = None
        losses = loss_fn(gt, leaves)
        torch.sum(torch.stack([losses[k] * WEIGHTS[k] for k in WEIGHTS])).backward()

    o_leaf = out.clone().requires_grad_(True)

    def torch_yardstick():
        o_leaf.grad = None
        torch_heatmap_loss(o_leaf, tgt, kw).backward()

    if once:
        for fn in (fwd_kernel, bwd_kernel, bwd_kernel_kp, heads_kernel, fwd_bwd, torch_yardstick):
            fn()
        torch.cuda.synchronize()
        return
    px = B * K * H * W
    r = {}
    r["fwd_kernel_us"] = timed(fwd_kernel, 200)
    r["fwd_kernel_bytes"] = 8 * px + N * 4 + N * 5 * 4 * 2
    r["bwd_kernel_us"] = timed(bwd_kernel, 200)
    r["bwd_kernel_bytes"] = 12 * px + N * 4           # read h and t, write dh; the keypoint weights
    r["bwd_kernel_kp_us"] = timed(bwd_kernel_kp, 200)
    r["bwd_kernel_kp_bytes"] = 16 * px + 2 * N * 4    # h twice (energy pass, gradient pass), t, dh
    r["heads_kernel_us"] = timed(heads_kernel, 200)
    r["heads_kernel_bytes"] = N * 4 * (6 + 3 + 4) + 16
    for k in ("fwd_kernel", "bwd_kernel", "bwd_kernel_kp", "heads_kernel"):
        r[k + "_TBps"] = r[k + "_bytes"] / r[k + "_us"] / 1e6
        r[k + "_roofline_us"] = r[k + "_bytes"] / 8e6
    r["probpose_fwd_bwd_us"] = timed(fwd_bwd, 30)
    r["torch_autograd_heatmap_fwd_bwd_us"] = timed(torch_yardstick, 50)
    res[tag] = r


res = {}
bench_shape("B64_K17_64x48", 64, 17, 64, 48, (192, 256), LR.COCO17_SIGMAS, ProbMap, res)
bench_shape("B32_K20_96x96", 32, 20, 96, 96, (384, 384), np.array([0.05] * 20), ArgMaxProbMap, res)
if not once:
    print(json.dumps(res))
