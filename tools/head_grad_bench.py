"""Time the training ProbMapHead (ProbMapHead(differentiable=True) in .train() mode) on the GPU.

Configurations: the ViT-B bench head (C = 768, 16x12 features, K = 17, batch 64) and train.py's head (C = 384, 24x24
features from 384x384 crops, K = 20, normalize = 1.0, freeze_error, batch 32).  For each, in bf16 and fp32:
  * the train-mode forward and the backward (HIP events, median of --iters),
  * the weight-gradient GEMM alone on the first aux stage's shape (M = B*h*w rows reduced, N = 4C, K = 9C): TFLOP/s
    and its fraction of the bf16 dense MFMA peak (2.5 PFLOP/s),
  * torch autograd of the same modules (eager torch ops, MIOpen convolutions, same GPU), for comparison.
One JSON line per configuration.  Per-kernel times of the backward:
  rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/head_grad_bench.py --only-backward
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16_PEAK = 2.5e15

CONFIGS = {
    "vitb_bench": dict(C=768, K=17, pools=[(4, 3), (2, 2), (2, 2)], hw=(16, 12), B=64, kw={}),
    "train_py": dict(C=384, K=20, pools=[(4, 4), (2, 2), (2, 2)], hw=(24, 24), B=32,
                     kw=dict(freeze_error=True, normalize=1.0)),
}


def _median_ms(fn, iters):
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return sorted(ts)[len(ts) // 2]


def _torch_forward(head, x):
    """The reference forward (head.py:487-594) on the head's own torch modules: eager torch autograd."""
    t = head.final_layer(head.deconv_layers(x))
    B, K, H, W = t.shape
    t = t.reshape(B, K, H * W) / head.temperature
    if head.normalize is not None:
        t = t.softmax(-1) * head.normalize      # stand-in of the absent Sparsemax package: same cost class
    heat = t.clamp(0, 1).reshape(B, K, H, W)
    outs = [heat]
    for name in ("probability", "visibility", "oks", "error"):
        outs.append(getattr(head, name + "_layers")(x.detach()))
    return outs


def run(name, cfg, dtype, iters, only_backward):
    from probpose_pytorch_amd import ops
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.synthetic import synthetic_features, synthetic_head_state
    C, K, B, (h, w) = cfg["C"], cfg["K"], cfg["B"], cfg["hw"]
    head = ProbMapHead(C, K, cfg["pools"], (256, 256), (4, 4), final_layer_kernel_size=1, differentiable=True,
                       **cfg["kw"])
    head.load_state_dict(synthetic_head_state(C, K, n_pools=3, deconv_out=(256, 256), seed=1), strict=False)
    head = head.cuda().set_compute_dtype(dtype).train()
    x = synthetic_features(B, C, h, w, seed=2).cuda()
    outs = head(x)
    ups = [torch.randn_like(o) for o in outs]

    def fwd():
        return head(x)

    def step():
        o = head(x)
        torch.autograd.backward(list(o), ups)

    for _ in range(2):
        step()
    res = dict(config=name, dtype=str(dtype).replace("torch.", ""), batch=B)
    if only_backward:
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        return res
    t_f = _median_ms(fwd, iters)
    t_s = _median_ms(step, iters)
    res.update(forward_ms=round(t_f, 3), backward_ms=round(t_s - t_f, 3), step_ms=round(t_s, 3))
    # the weight-gradient GEMM alone on the first aux stage's shape
    from probpose_pytorch_amd import pack
    M = B * h * w
    dt = dtype
    dY = torch.randn(M, 4 * C, device="cuda").to(dt)
    A = torch.randn(M, C, device="cuda").to(dt)
    ro = pack.conv_gather_table(B, h, w, 3, 3, 1, 1, C).cuda()
    dW = torch.empty(4 * C, 9 * C, device="cuda")
    n = ops.wgrad_workspace_floats(M, 4 * C, 9 * C, 1)
    parts = torch.empty(max(n, 1), device="cuda")
    g = lambda: ops.wgrad(dY, A, dW, M=M, N=4 * C, Kd=9 * C, ldd=4 * C, rowoff=ro, seg_len=C, parts=parts)  # noqa: E731
    g()
    t_g = _median_ms(g, iters)
    flop = 2.0 * M * 4 * C * 9 * C
    res.update(wgrad_aux0_ms=round(t_g, 3), wgrad_aux0_tflops=round(flop / t_g / 1e9, 1),
               wgrad_aux0_frac_bf16_peak=round(flop / t_g * 1e3 / BF16_PEAK, 4))
    # torch autograd of the same modules
    tdt = torch.bfloat16 if dtype == torch.bfloat16 else torch.float32
    th = ProbMapHead(C, K, cfg["pools"], (256, 256), (4, 4), final_layer_kernel_size=1, **cfg["kw"])
    th.load_state_dict(head.state_dict())
    th = th.cuda().to(tdt).train()
    xt = x.to(tdt)
    upt = [u.to(tdt) for u in ups]

    def tstep():
        o = _torch_forward(th, xt)
        pairs = [(a, u) for a, u in zip(o, upt) if a.requires_grad]     # a frozen branch has no graph
        torch.autograd.backward([a for a, _ in pairs], [u for _, u in pairs])

    tstep()
    res.update(torch_step_ms=round(_median_ms(tstep, iters), 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--only-backward", action="store_true", help="just run steps (for a rocprofv3 kernel trace)")
    a = ap.parse_args()
    dts = {"bf16": torch.bfloat16, "fp32": torch.float32}
    for name in a.configs.split(","):
        for d in a.dtypes.split(","):
            print(json.dumps(run(name, CONFIGS[name], dts[d], a.iters, a.only_backward)), flush=True)


if __name__ == "__main__":
    main()
