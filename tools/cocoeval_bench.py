"""CocoKeypointEval.evaluate() at COCO-val scale on the GPU; the plain-loop numpy gauge on the same data as context.

Synthetic data: `--images` images (5000), 0 - 4 ground truths (2 on average) and 0 - 20 detections per image, K = 17;
people of small, medium and large area, some crowds, detections that are jittered ground truths or strays.

  device   detections handed over as device tensors (what Codec.decode leaves there): evaluate() only
  host     detections handed over as numpy arrays: evaluate() uploads them first
  gauge    tests/cocoeval_reference.evaluate on the same images (wall clock, `--gauge-repeats` runs)

HIP-event time per evaluate(), its final synchronisation included: `--steps` calls per window, `--repeats` windows per
variant after `--warmup` calls, the variants alternating; median, min and max of the windows.  One JSON line.

  --once   three evaluate() calls of the device variant and nothing else, for
           `rocprofv3 --kernel-trace --stats -- python tools/cocoeval_bench.py --once`
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_images(n, seed):
    from tests import cocoeval_reference as CR
    rng = np.random.default_rng(seed)
    return [CR.random_image(rng, 17, int(rng.integers(0, 5)), int(rng.integers(0, 21)), crowd_p=0.05)
            for _ in range(n)]


def fill(ev, images, device):
    for i, im in enumerate(images):
        ev.add_ground_truth(i, im["gt_kpts"], im["gt_bbox"], im["gt_area"], im["gt_crowd"])
    ids = np.concatenate([np.full(im["dt_kpts"].shape[0], i, dtype=np.int64) for i, im in enumerate(images)])
    kp = np.concatenate([im["dt_kpts"] for im in images])
    sc = np.concatenate([im["dt_score"] for im in images])
    ar = np.concatenate([im["dt_area"] for im in images])
    if device:      # float32, as a decoder leaves them
        ev.add_detections(ids, torch.from_numpy(kp).float().cuda(), torch.from_numpy(sc).float().cuda(),
                          torch.from_numpy(ar).float().cuda())
    else:
        ev.add_detections(ids, kp, sc, ar)
    return ev


def window(ev, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        ev.evaluate()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def spread(ts, digits=3):
    return dict(ms_median=round(statistics.median(ts), digits), ms_min=round(min(ts), digits),
                ms_max=round(max(ts), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--gauge-repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--once", action="store_true", help="three evaluate() calls of the device variant, nothing else")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cocoeval_bench needs the GPU: there is nothing to time without it"
    from probpose_pytorch_amd import CocoKeypointEval
    from tests import cocoeval_reference as CR
    images = make_images(args.images, args.seed)
    if args.once:
        ev = fill(CocoKeypointEval(CR.COCO17_SIGMAS), images, device=True)
        for _ in range(3):
            res = ev.evaluate()
        print(json.dumps(dict(images=args.images, once=True, AP=round(res["AP"], 6))))
        return
    variants = {name: fill(CocoKeypointEval(CR.COCO17_SIGMAS), images, device=(name == "device"))
                for name in ("device", "host")}
    stats = {}
    for name, ev in variants.items():
        for _ in range(args.warmup):
            stats[name] = ev.evaluate()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, ev in variants.items():
            times[k].append(window(ev, args.steps))
    gauge_ms, want = [], None
    for _ in range(args.gauge_repeats):
        t0 = time.perf_counter()
        want = CR.evaluate(images, CR.COCO17_SIGMAS)
        gauge_ms.append((time.perf_counter() - t0) * 1e3)
    res = dict(images=args.images, K=17, ground_truths=int(sum(im["gt_kpts"].shape[0] for im in images)),
               detections=int(sum(im["dt_kpts"].shape[0] for im in images)),
               oks_pairs=int(sum(im["gt_kpts"].shape[0] * im["dt_kpts"].shape[0] for im in images)),
               steps=args.steps, repeats=args.repeats, warmup=args.warmup, gauge_repeats=args.gauge_repeats)
    for k, ts in times.items():
        res[k] = spread(ts)
    res["gauge"] = spread(gauge_ms, 1) if gauge_ms else None
    res["AP"] = round(stats["host"]["AP"], 6)
    if want is not None:
        # float64 detections reproduce the gauge; the float32 ones of `device` are a different input
        res["host_vs_gauge_max_stat_diff"] = float(max(abs(stats["host"][k] - want[k]) for k in CR.STATS))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
