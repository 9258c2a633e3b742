"""Optimizer step on the GPU: clip_grad_norm_ + torch.optim.AdamW against FusedAdamW, on the trainable parameter
shapes of train.py's model and of ViT-B 256x192 K=17, with fixed synthetic gradients.

  (a) clip_grad_norm_ + torch.optim.AdamW as torch selects it by default
  (b) the same with fused=True, where this torch build accepts it
  (c) FusedAdamW(max_grad_norm=1.0)

HIP-event time per step: `--steps` steps per window, `--repeats` windows per variant after `--warmup` steps, the
variants alternating; median, min and max of the windows are reported, with the parameter count, the bytes moved at
32 B / parameter and the GB/s that implies.  One JSON line per model.

  --once VARIANT   two steps of one variant on the first model chosen by `--model` (the first step creates the
                   optimizer state) and nothing else, for
                   `rocprofv3 --kernel-trace --stats -- python tools/optim_bench.py --once c`
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = {
    "train_py": dict(size=(384, 384), C=384, depth=12, heads=12, K=20),
    "vit_b_256x192_k17": dict(size=(256, 192), C=768, depth=12, heads=12, K=17),
}


def trainable_shapes(cfg):
    """Shapes of the parameters that train.py would hand to the optimizer (constructed on the CPU, nothing run)."""
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.model import ProbPoseModel
    bb = ScratchViTBackbone(cfg["size"], 16, embed_dim=cfg["C"], depth=cfg["depth"], num_heads=cfg["heads"])
    head = ProbMapHead(cfg["C"], cfg["K"], [(4, 4), (2, 2), (2, 2)], (256, 256), (4, 4), final_layer_kernel_size=1,
                       freeze_error=True, normalize=1.0)
    model = ProbPoseModel(bb, head)
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


def make(shapes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=g) * 0.02) for s in shapes]
    grads = [torch.randn(s, device="cuda", generator=g) * 0.01 for s in shapes]
    return ps, grads


class Variant:
    def __init__(self, name, shapes):
        from probpose_pytorch_amd import FusedAdamW
        self.name = name
        self.ps, self.grads = make(shapes, 0)
        if name == "a":
            self.opt = torch.optim.AdamW(self.ps, lr=5e-4, weight_decay=0.1)
        elif name == "b":
            self.opt = torch.optim.AdamW(self.ps, lr=5e-4, weight_decay=0.1, fused=True)
        else:
            self.opt = FusedAdamW(self.ps, lr=5e-4, weight_decay=0.1, max_grad_norm=1.0)

    def step(self):
        if self.name != "c":
            # clip_grad_norm_ rewrites the fixed gradients in place: after the first step their norm is max_norm and
            # the coefficient 1, but the norm is still taken and every gradient still multiplied: the same work
            torch.nn.utils.clip_grad_norm_(self.ps, max_norm=1.0)
        self.opt.step()

    def bind(self):
        for p, g in zip(self.ps, self.grads):
            p.grad = g

    def window(self, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            self.step()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--once", choices=["a", "b", "c"])
    ap.add_argument("--model", choices=list(MODELS), action="append", help="default: both")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench needs the GPU: there is nothing to time without it"
    lines = []
    for mname in args.model or list(MODELS):
        cfg = MODELS[mname]
        shapes = trainable_shapes(cfg)
        n_param = sum(int(torch.Size(s).numel()) for s in shapes)
        if args.once:
            v = Variant(args.once, shapes)
            v.bind()
            v.step()
            v.step()
            torch.cuda.synchronize()
            print(json.dumps(dict(model=mname, once=args.once, tensors=len(shapes), parameters=n_param)))
            return
        variants = {}
        for name in ("a", "b", "c"):
            try:
                variants[name] = Variant(name, shapes)
                variants[name].bind()
                for _ in range(args.warmup):
                    variants[name].step()
                torch.cuda.synchronize()
            except (RuntimeError, ValueError, NotImplementedError) as e:
                if name != "b":
                    raise
                variants.pop(name, None)
                print(f"(b) fused=True is not available here: {e}", file=sys.stderr)
        times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, v in variants.items():
                times[k].append(v.window(args.steps))
        res = dict(model=mname, tensors=len(shapes), parameters=n_param, bytes_per_step=32 * n_param,
                   steps=args.steps, repeats=args.repeats, warmup=args.warmup)
        for k, ts in times.items():
            med = statistics.median(ts)
            res[k] = dict(ms_median=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                          gb_per_s=round(32 * n_param / (med * 1e-3) / 1e9, 1))
        if "b" not in variants:
            res["b"] = None
        line = json.dumps(res)
        print(line)
        lines.append(line)
        del variants
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
