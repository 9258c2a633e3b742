#!/usr/bin/env python3
"""Time ProbPoseLoss.forward (B=64, K=17, 64x48, ProbMap codec) and pp_oks_heatmap_loss alone on the device, and the
reference-style host path it replaces (both heatmap stacks copied to the host, decoded crop by crop with scipy:
oracle.codec_decode), in one process.  `--once`: one forward of each, for `rocprofv3 --kernel-trace` launch counts."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import __graft_entry__ as g

g.build()
from oracle import probpose_oracle as orc
from probpose.codec import Codec, ProbMap
from probpose.loss import ProbPoseLoss
from probpose_pytorch_amd.loss import _oks_heatmap_loss
from tests import loss_reference as LR

once = "--once" in sys.argv
B, K, H, W = 64, 17, 64, 48
rng = np.random.default_rng(0)
kps = rng.uniform(-10, 200, (B, K, 2)).astype(np.float32)
annotated = rng.random((B, K)) > 0.2
gt_hm, in_image = LR.encode_probmaps(kps, annotated.astype(np.float32), (192, 256), (W, H))
dt_hm = np.clip(gt_hm * 0.8 + rng.random((B, K, H, W), dtype=np.float32) * 0.1, 0, 1).astype(np.float32)
heads = [rng.uniform(0.01, 0.99, (B, K, 1, 1)).astype(np.float32) for _ in range(4)]
gt = dict(heatmaps=torch.from_numpy(gt_hm).cuda(), in_image=torch.from_numpy(in_image[:, None]).cuda(),
          keypoints_visible=torch.from_numpy(annotated[:, None]).cuda(),
          keypoints_visibility=torch.from_numpy((rng.random((B, 1, K)) > 0.5).astype(np.float32)).cuda())
pred = tuple(torch.from_numpy(p).cuda() for p in (dt_hm, *heads))
loss_fn = ProbPoseLoss(Codec(ProbMap((192, 256), (W, H), LR.COCO17_SIGMAS)))
out, tgt = pred[0], gt["heatmaps"]
kw = torch.ones((B, K), device="cuda")
sc = torch.empty(3, device="cuda")


def heat():
    _oks_heatmap_loss(out, tgt, kw, None, False, "minus", 0.05, 0.0, 1.0, None, None, sc)


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


with torch.no_grad():
    if once:
        torch.cuda.synchronize()
        loss_fn(gt, pred)
        loss_fn(gt, pred, compute_acc=True)
        heat()
        torch.cuda.synchronize()
        sys.exit(0)
    res = {}
    res["heatmap_loss_us"] = timed(heat, 200)
    nbytes = 2 * B * K * H * W * 4 + B * K * 4 + B * K * 5 * 4 * 2
    res["heatmap_loss_bytes"] = nbytes
    res["heatmap_loss_GBps"] = nbytes / res["heatmap_loss_us"] / 1e3
    res["forward_us"] = timed(lambda: loss_fn(gt, pred), 50)
    res["forward_acc_us"] = timed(lambda: loss_fn(gt, pred, compute_acc=True), 20)
    # the reference's host path: both stacks to the host, then one scipy decode per crop and stack
    t0 = time.perf_counter()
    n = 8
    for _ in range(n):
        g_h, d_h = gt["heatmaps"].cpu().numpy(), pred[0].cpu().numpy()
        for b in range(2):
            orc.codec_decode((g_h[b:b + 1], *[h[b:b + 1] for h in heads]), (192, 256), (W, H), LR.COCO17_SIGMAS)
            orc.codec_decode((d_h[b:b + 1], *[h[b:b + 1] for h in heads]), (192, 256), (W, H), LR.COCO17_SIGMAS)
    res["cpu_decode_ms_per_crop_stack"] = (time.perf_counter() - t0) / (n * 4) * 1e3
    res["cpu_decode_ms_batch_est"] = res["cpu_decode_ms_per_crop_stack"] * 2 * B
print(json.dumps(res))
