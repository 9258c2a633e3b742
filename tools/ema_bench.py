"""EMA update on the GPU: the torch ways of averaging a model's weights against ModelEma, on the full state
(parameters and buffers) of train.py's model and of ViT-B 256x192 K=17.

  (a) timm's ModelEmaV2 loop: per entry ema.copy_(decay * ema + (1 - decay) * model)
  (b) timm's ModelEmaV3 foreach path: torch._foreach_lerp_ over the float entries, copy_ for the rest
  (c) ModelEma.update (one launch, csrc/pp_ema.hip)

All three walk both state_dicts on every update, as the originals do.  HIP-event time per update: `--steps` updates per
window, `--repeats` windows per variant after `--warmup` updates, the variants alternating in one process; median, min
and max of the windows are reported, with the host time spent issuing one update (no device wait inside).  Issued back
to back, an update takes as long as the host needs to issue it whenever that is longer than the kernels run, so a second
set of windows (`device_*`) first queues matrix products that keep the GPU busy for longer than the host needs to issue
the window: the updates then run back to back on the device and the events around them give the device time alone, with
the bytes moved at 12 B / averaged element and the GB/s that implies.  One JSON line per model.

  --once VARIANT   two updates of one variant on the first model chosen by `--model` and nothing else, for
                   `rocprofv3 --kernel-trace --stats -- python tools/ema_bench.py --once c`
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = {
    "train_py": dict(size=(384, 384), C=384, depth=12, heads=12, K=20),
    "vit_b_256x192_k17": dict(size=(256, 192), C=768, depth=12, heads=12, K=17),
}
DECAY = 0.9999


def build_model(cfg):
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.model import ProbPoseModel
    bb = ScratchViTBackbone(cfg["size"], 16, embed_dim=cfg["C"], depth=cfg["depth"], num_heads=cfg["heads"])
    head = ProbMapHead(cfg["C"], cfg["K"], [(4, 4), (2, 2), (2, 2)], (256, 256), (4, 4), final_layer_kernel_size=1,
                       freeze_error=True, normalize=1.0)
    return ProbPoseModel(bb, head).cuda()


class Variant:
    def __init__(self, name, model):
        from probpose_pytorch_amd import ModelEma
        self.name, self.model = name, model
        if name == "c":
            self.ema = ModelEma(model, decay=DECAY)
            self.module = self.ema.module
        else:
            self.module = copy.deepcopy(model).eval().requires_grad_(False)

    @torch.no_grad()
    def step(self):
        if self.name == "a":
            for e, m in zip(self.module.state_dict().values(), self.model.state_dict().values()):
                e.copy_(DECAY * e + (1.0 - DECAY) * m)
        elif self.name == "b":
            ef, mf = [], []
            for e, m in zip(self.module.state_dict().values(), self.model.state_dict().values()):
                if e.is_floating_point():
                    ef.append(e)
                    mf.append(m)
                else:
                    e.copy_(m)
            torch._foreach_lerp_(ef, mf, weight=1.0 - DECAY)
        else:
            self.ema.update(self.model)

    def window(self, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        host = time.perf_counter() - t0
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps, host * 1e3 / steps

    def device_window(self, steps, host_ms, blocker):
        """Device time per update with the host run ahead: `blocker` keeps the GPU busy while the window is issued."""
        blocker(1.5 * host_ms * steps + 2.0)
        return self.window(steps)[0]


class Blocker:
    """Queues bf16 matrix products on the current stream for at least `ms` milliseconds of GPU time."""

    def __init__(self, n=8192):
        self.a = torch.randn(n, n, device="cuda", dtype=torch.bfloat16)
        self.c = torch.empty_like(self.a)
        for _ in range(3):
            torch.mm(self.a, self.a, out=self.c)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            torch.mm(self.a, self.a, out=self.c)
        b.record()
        b.synchronize()
        self.ms_each = a.elapsed_time(b) / 10

    def __call__(self, ms):
        for _ in range(int(ms / self.ms_each) + 1):
            torch.mm(self.a, self.a, out=self.c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--device-steps", type=int, default=20, help="updates per device-only window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--once", choices=["a", "b", "c"])
    ap.add_argument("--model", choices=list(MODELS), action="append", help="default: both")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ema_bench needs the GPU: there is nothing to time without it"
    lines = []
    blocker = None if args.once else Blocker()
    for mname in args.model or list(MODELS):
        torch.manual_seed(0)
        model = build_model(MODELS[mname])
        state = model.state_dict()
        n_avg = sum(v.numel() for v in state.values() if v.dtype == torch.float32)
        n_copy = sum(1 for v in state.values() if v.dtype != torch.float32)
        if args.once:
            v = Variant(args.once, model)
            v.step()
            v.step()
            torch.cuda.synchronize()
            print(json.dumps(dict(model=mname, once=args.once, entries=len(state), averaged_elements=n_avg)))
            return
        variants = {name: Variant(name, model) for name in ("a", "b", "c")}
        for v in variants.values():
            for _ in range(args.warmup):
                v.step()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        hosts = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, v in variants.items():
                dev, host = v.window(args.steps)
                times[k].append(dev)
                hosts[k].append(host)
        dev_times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, v in variants.items():
                dev_times[k].append(v.device_window(args.device_steps, statistics.median(hosts[k]), blocker))
        res = dict(model=mname, entries=len(state), copied_entries=n_copy, averaged_elements=n_avg,
                   bytes_per_update=12 * n_avg, steps=args.steps, device_steps=args.device_steps,
                   repeats=args.repeats, warmup=args.warmup, blocker_mm_ms=round(blocker.ms_each, 4))
        for k, ts in times.items():
            med = statistics.median(ts)
            res[k] = dict(ms_median=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                          host_ms_median=round(statistics.median(hosts[k]), 4))
            dev = statistics.median(dev_times[k])
            res[k].update(device_ms_median=round(dev, 4), device_ms_min=round(min(dev_times[k]), 4),
                          device_ms_max=round(max(dev_times[k]), 4),
                          device_gb_per_s=round(12 * n_avg / (dev * 1e-3) / 1e9, 1))
        line = json.dumps(res)
        print(line)
        lines.append(line)
        del variants, model, state
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
