"""Flip test beside the forward it doubles: ProbPoseModel(flip_pairs=...) at batch B against the plain forward at 2B.

Workload: bench.py's `--config` (default vit_b: 256x192 crops, K = 17, batch 64) in `--dtype` (default bf16), eager
launches on one stream, seeded synthetic weights and crops.

  plain_2B     the plain forward on [x, mirrored x] (built once, outside the window): the yardstick, unchanged code
  flip_B       the flip-test forward on x: pp_hflip_pair, the same forward at 2B, pp_flip_merge
  hflip_pair   the first kernel alone; 12 bytes per input element (one read, two writes)
  flip_merge   the second kernel alone on the plain forward's outputs; 12 bytes per output element

`--repeats` rounds; in each round one window of `--steps` calls of each of the four, one after the other (alternating
windows in one process), HIP-event time per call; median, min and max over the rounds.  The kernels' GB/s are their
algorithmic bytes over the median time, next to the device's measured copy rate.  There is no threshold.
One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE_TB_PER_S = (4.9, 5.0)          # what a device-to-device copy reaches


def stats(ts):
    return dict(ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="vit_b", choices=sorted(bench.CONFIGS))
    ap.add_argument("--batch", type=int, default=0, help="B of the flip-test forward (default: the config's)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "flip_bench needs the GPU: there is nothing to time without it"
    from probpose_pytorch_amd import flip, ops
    from probpose_pytorch_amd.synthetic import synthetic_crops
    cfg = bench.CONFIGS[args.config]
    B, K, (H, W) = args.batch or cfg["batch"], cfg["K"], cfg["img"]
    dtype = dict(bf16=torch.bfloat16, fp32=torch.float32)[args.dtype]
    model, _, _ = bench.build(cfg, dtype, "cuda")
    pairs = [(i, i + 1) for i in range(1, K - 1, 2)]
    x = synthetic_crops(B, H, W, seed=1234).cuda()
    x2 = torch.cat([x, x.flip(-1)])
    buf2 = torch.empty_like(x2)
    with torch.no_grad():
        model.set_flip_test(pairs)
        perm = model._flip_perm
        for _ in range(args.warmup):
            got = model(x)
        model.set_flip_test(None)
        for _ in range(args.warmup):
            out2 = model(x2)
        torch.cuda.synchronize()
        # the timed paths agree, at the timed size: flip test is the merge of the plain outputs, bit for bit
        want = flip.flip_merge(out2, perm)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), "flip-test forward differs from the merged plain forward"
        assert torch.equal(ops.hflip_pair(x, buf2), x2), "hflip_pair differs from cat([x, x.flip(-1)])"

        def plain():
            model(x2)

        def flipped():
            model(x)

        def window(fn):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / args.steps

        t = dict(plain_2B=[], flip_B=[], hflip_pair=[], flip_merge=[])
        for _ in range(args.repeats):
            model.set_flip_test(None)
            t["plain_2B"].append(window(plain))
            model.set_flip_test(pairs)
            t["flip_B"].append(window(flipped))
            t["hflip_pair"].append(window(lambda: ops.hflip_pair(x, buf2)))
            t["flip_merge"].append(window(lambda: flip.flip_merge(out2, perm)))
    pair_bytes = x.numel() * 12
    merge_bytes = (got[0].numel() + 4 * B * K) * 12
    res = dict(config=args.config, dtype=args.dtype, batch=B, input=(H, W), K=K, heatmap=tuple(got[0].shape[2:]),
               steps=args.steps, repeats=args.repeats, warmup=args.warmup,
               plain_forward_2B=stats(t["plain_2B"]), flip_test_forward_B=stats(t["flip_B"]),
               hflip_pair=stats(t["hflip_pair"]), flip_merge=stats(t["flip_merge"]),
               hflip_pair_bytes=pair_bytes, flip_merge_bytes=merge_bytes,
               copy_rate_TB_per_s=COPY_RATE_TB_PER_S)
    res["flip_over_plain"] = round(res["flip_test_forward_B"]["ms_median"] / res["plain_forward_2B"]["ms_median"], 4)
    res["hflip_pair_GB_per_s"] = round(pair_bytes / (res["hflip_pair"]["ms_median"] * 1e-3) / 1e9, 1)
    res["flip_merge_GB_per_s"] = round(merge_bytes / (res["flip_merge"]["ms_median"] * 1e-3) / 1e9, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
