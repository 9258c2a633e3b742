"""Time the training ScratchViTBackbone (ScratchViTBackbone(differentiable=True) in .train() mode) on the GPU.

Configurations: train.py's backbone (384x384 crops, C 384, 12 heads, depth 12, batch 32) and ViT-B 256x192 (C 768, 12
heads, depth 12, batch 64).  For each, in bf16 and fp32: the training forward, the backward and the whole step (HIP
events, median of --iters), and torch autograd of an equivalent torch ViT (nn.Linear / nn.LayerNorm / nn.GELU,
F.scaled_dot_product_attention; same weights, same GPU) for comparison.  One JSON line per configuration.
Per-kernel times of the step:
  rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/vit_grad_bench.py --only-steps
--drop-path RATE builds the backbone with drop_path_rate=RATE (stochastic depth; the masks are drawn from a fixed
seed, a new one every step as in training) and adds the rate and the share of kept branch-crops to the JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "train_py": dict(img=(384, 384), C=384, heads=12, depth=12, B=32),
    "vit_b": dict(img=(256, 192), C=768, heads=12, depth=12, B=64),
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


def _torch_features(vit, x, heads):
    """The same ViT as eager torch ops (the parameters of ``vit``, cast by the caller)."""
    pe = vit.patch_embed.proj
    t = F.conv2d(x, pe.weight, pe.bias, stride=pe.stride).flatten(2).transpose(1, 2) + vit.pos_embed
    B, N, C = t.shape
    for blk in vit.blocks:
        h = F.layer_norm(t, (C,), blk.norm1.weight, blk.norm1.bias, 1e-6)
        q, k, v = F.linear(h, blk.attn.qkv.weight, blk.attn.qkv.bias).reshape(B, N, 3, heads, C // heads) \
            .permute(2, 0, 3, 1, 4).unbind(0)
        o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, C)
        t = t + F.linear(o, blk.attn.proj.weight, blk.attn.proj.bias)
        h = F.layer_norm(t, (C,), blk.norm2.weight, blk.norm2.bias, 1e-6)
        h = F.gelu(F.linear(h, blk.mlp.fc1.weight, blk.mlp.fc1.bias))
        t = t + F.linear(h, blk.mlp.fc2.weight, blk.mlp.fc2.bias)
    return F.layer_norm(t, (C,), vit.norm.weight, vit.norm.bias, 1e-6)


def run(name, cfg, dtype, iters, only_steps, drop_path=None):
    import copy

    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_vit_state
    img, C, heads, depth, B = cfg["img"], cfg["C"], cfg["heads"], cfg["depth"], cfg["B"]
    kw = {} if drop_path is None else dict(drop_path_rate=drop_path)
    bb = ScratchViTBackbone(img, 16, embed_dim=C, depth=depth, num_heads=heads, differentiable=True, **kw)
    bb.model.load_state_dict(synthetic_vit_state(img, 16, C, depth, seed=1))
    bb = bb.cuda().set_compute_dtype(dtype).train()
    x = synthetic_crops(B, *img, seed=2).cuda()
    f = bb.model.forward_tokens(x)
    up = torch.randn_like(f)
    kept = []
    if drop_path is not None:
        torch.manual_seed(1234)

    def fwd():
        return bb.model.forward_tokens(x)

    def step():
        bb.model.forward_tokens(x).backward(up)
        if bb.last_drop_path_keep is not None:
            kept.append(float(bb.last_drop_path_keep.float().mean()))

    for _ in range(2):
        step()
    res = dict(config=name, dtype=str(dtype).replace("torch.", ""), batch=B, depth=depth)
    if drop_path is not None:
        res.update(drop_path_rate=drop_path)
    if only_steps:
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        return res
    t_f = _median_ms(fwd, iters)
    del kept[:]
    t_s = _median_ms(step, iters)
    res.update(forward_ms=round(t_f, 3), backward_ms=round(t_s - t_f, 3), step_ms=round(t_s, 3))
    if kept:
        res.update(kept_share=round(sum(kept) / len(kept), 4))
    tv = copy.deepcopy(bb.model).to(dtype)
    xt = x.to(dtype)
    upt = up.to(dtype).reshape(B, -1, C)

    def tstep():
        _torch_features(tv, xt, heads).backward(upt)

    tstep()
    res.update(torch_step_ms=round(_median_ms(tstep, iters), 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--only-steps", action="store_true", help="just run bf16 steps (for a rocprofv3 kernel trace)")
    ap.add_argument("--drop-path", type=float, default=None, metavar="RATE",
                    help="drop_path_rate of the backbone (masks drawn from a fixed seed)")
    a = ap.parse_args()
    dts = {"bf16": torch.bfloat16, "fp32": torch.float32}
    for name in a.configs.split(","):
        for d in (["bf16"] if a.only_steps else a.dtypes.split(",")):
            print(json.dumps(run(name, CONFIGS[name], dts[d], a.iters, a.only_steps, a.drop_path)), flush=True)


if __name__ == "__main__":
    main()
