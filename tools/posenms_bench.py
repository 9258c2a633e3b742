"""PoseNMS at COCO-val scale on the GPU, and CocoKeypointEval.evaluate() on what it keeps, in the same run.

Synthetic data, K = 17: `--images` images (5000) of `--dets` detections each (20 and 100); an image holds people of
side 32 - 190 with 2 or 3 detections each, which are copies of the person jittered by a level of 0, 0.1, 0.3, 0.6, 1 or 2
times side * 2 sigma_k (as tests/posenms_reference.random_image, vectorised), so the pair OKS straddles 0.9; the people
are the ground truths of the evaluator.  Detections are float32 device tensors, as a decoder leaves them.

  posenms/<mode>   one PoseNMS call: the layout from the image ids (host), casts, the finiteness readback, two stable
                   sorts, gathers, pp_posenms, scatters
  kernel/<mode>    the pp_posenms launch of that call alone, on its sorted batch (with its three output allocations)
  evaluate         CocoKeypointEval.evaluate() on the detections hard NMS keeps (its final synchronisation included)

HIP-event time per call: every variant is warmed up, a window is `--window-ms` of calls (the number of calls is
calibrated per variant), `--repeats` windows per variant, the variants alternating; median, min and max of the windows.
One JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
LEVELS = np.array([0.0, 0.1, 0.3, 0.6, 1.0, 2.0])
MODES = ("hard", "soft_gaussian", "soft_linear")


def make_batch(n_img, D, seed):
    """dict(ids [M], kpts [M, 17, 2], score [M], area [M], vis [M, 17], people: per image (kpts [P, 17, 3], bbox, area))."""
    rng = np.random.default_rng(seed)
    K, P = 17, max(1, math.ceil(D / 2.5))
    person_of = (np.arange(D) * P) // D
    side = rng.choice([40.0, 60.0, 150.0], (n_img, P)) * rng.uniform(0.8, 1.25, (n_img, P))
    origin = rng.uniform(0, 400, (n_img, P, 1, 2))
    people = origin + rng.uniform(0, 1, (n_img, P, K, 2)) * side[..., None, None]
    level = rng.choice(LEVELS, (n_img, P))
    reach = (level * side)[:, person_of, None, None] * 2 * SIGMAS[None, None, :, None]
    kpts = people[:, person_of] + rng.uniform(-1, 1, (n_img, D, K, 2)) * reach
    area = (side * side * 0.6)[:, person_of] * rng.uniform(0.9, 1.1, (n_img, D))
    order = np.argsort(rng.random((n_img, D)), axis=1)              # shuffled within the image
    take = lambda a: np.take_along_axis(a, order.reshape(order.shape + (1,) * (a.ndim - 2)), axis=1)
    gt = np.concatenate([people, np.full((n_img, P, K, 1), 2.0)], axis=3)
    bbox = np.concatenate([origin[:, :, 0], np.repeat(side[..., None], 2, axis=2)], axis=2)
    return dict(n_img=n_img, D=D, ids=np.repeat(np.arange(n_img, dtype=np.int64), D),
                kpts=take(kpts).reshape(n_img * D, K, 2), area=take(area).reshape(-1),
                score=rng.uniform(0.05, 1.0, n_img * D), vis=rng.uniform(0, 1, (n_img * D, K)),
                gt_kpts=gt, gt_bbox=bbox, gt_area=side * side * 0.6)


def launch_arguments(nms, *inputs):
    """One call of ``nms``: (what it hands to its pp_posenms launch, its result)."""
    launch, seen = nms._launch, []

    def spy(*args):
        seen.append(args)
        return launch(*args)

    nms._launch = spy
    try:
        res = nms(*inputs)
    finally:
        del nms._launch             # the instance attribute: the class's method is back
    return seen[0], res


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def spread(ts, digits=3):
    return dict(ms_median=round(statistics.median(ts), digits), ms_min=round(min(ts), digits),
                ms_max=round(max(ts), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--window-ms", type=float, default=1000.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "posenms_bench needs the GPU: there is nothing to time without it"
    from probpose_pytorch_amd import CocoKeypointEval, PoseNMS

    variants, sizes = {}, {}
    for D in args.dets:
        b = make_batch(args.images, D, args.seed + D)
        kp, sc = torch.from_numpy(b["kpts"]).float().cuda(), torch.from_numpy(b["score"]).float().cuda()
        ar = torch.from_numpy(b["area"]).float().cuda()
        kept = {}
        for mode in MODES:
            nms = PoseNMS(SIGMAS, mode=mode)
            variants[f"{D}/posenms/{mode}"] = (lambda nms=nms, b=b, kp=kp, sc=sc, ar=ar: nms(b["ids"], kp, sc, ar))
            launch_args, res = launch_arguments(nms, b["ids"], kp, sc, ar)
            kept[mode] = int(res.keep.sum())
            variants[f"{D}/kernel/{mode}"] = (lambda nms=nms, a=launch_args: nms._launch(*a))
        res = PoseNMS(SIGMAS, mode="hard")(b["ids"], kp, sc, ar)
        keep = res.keep
        ev = CocoKeypointEval(SIGMAS)
        for i in range(args.images):
            ev.add_ground_truth(i, b["gt_kpts"][i], b["gt_bbox"][i], b["gt_area"][i])
        ev.add_detections(b["ids"][keep.cpu().numpy()], kp[keep], res.scores[keep], ar[keep])
        variants[f"{D}/evaluate"] = ev.evaluate
        sizes[str(D)] = dict(detections=int(b["ids"].size), kept=kept, AP_after_hard_nms=round(ev.evaluate()["AP"], 6))

    steps = {}
    for name, fn in variants.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        steps[name] = max(3, math.ceil(args.window_ms / max(window(fn, 3), 1e-3)))
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            times[name].append(window(fn, steps[name]))
    out = dict(images=args.images, K=17, window_ms=args.window_ms, repeats=args.repeats, warmup=args.warmup,
               sizes=sizes, steps=steps)
    for name, ts in times.items():
        out[name] = spread(ts)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
