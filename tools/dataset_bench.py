"""Batch assembly for train.py's step: YOLOPoseDataset.collate on the GPU against the reference's per-sample CPU path.

Workload: 32 samples, 384x384 input, K = 20, 96x96 maps; the sources are crop regions of 200-600 pixels a side cut
from a seeded 1080p frame (what `__getitem__` hands over), held in memory: no file reading or decoding is timed.

  device   HIP-event time of the three launches (crop/resize, ground truth, maps) on uploaded buffers
  copies   HIP-event time of the two host-to-device copies + the three launches of a whole collate()
  host     wall-clock time of collate() per call, `--steps` calls back to back with no synchronisation inside the
           window (the queue is drained before and after it)
  cpu      the reference's per-sample work for the same 32 samples on one thread: PIL crop + LANCZOS resize, /255,
           float32 keypoint rescale, the K float64 numpy maps (the oracle's restatement of generate_probmaps)

`--repeats` windows of `--steps` calls after `--warmup` calls; median, min and max over the windows.  One JSON line.
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

B, K, INPUT, HEAT = 32, 20, (384, 384), (96, 96)


def make_samples(seed=0):
    rng = np.random.default_rng(seed)
    frame = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    samples, boxes = [], []
    for _ in range(B):
        w, h = float(rng.uniform(200, 450)), float(rng.uniform(300, 600))
        x, y = float(rng.uniform(0, 1920 - w)), float(rng.uniform(0, 1080 - h))
        kps = np.stack([rng.uniform(x, x + w, K), rng.uniform(y, y + h, K), rng.integers(0, 2, K) * 2.0], -1)
        x0, y0, x1, y1 = int(round(x)), int(round(y)), int(round(x + w)), int(round(y + h))
        samples.append((np.ascontiguousarray(frame[y0:y1, x0:x1]), kps.astype(np.float32),
                        np.array([x, y, w, h], dtype=np.float64)))
        boxes.append([x, y, w, h])
    return frame, samples, boxes


def cpu_path(frame, samples, boxes, sigmas):
    """The reference's __getitem__ work for every sample, one thread."""
    import PIL.Image
    from oracle import probpose_oracle as orc
    image = PIL.Image.fromarray(frame, "RGB")
    out = []
    for (_, kps, _), (x, y, w, h) in zip(samples, boxes):
        crop = image.crop((x, y, x + w, y + h)).resize(INPUT, resample=PIL.Image.LANCZOS)
        img = (np.asarray(crop, dtype=np.uint8).astype(np.float32) * np.float32(1.0 / 255.0)).transpose(2, 0, 1).copy()
        k = kps.copy()
        k[:, 0] = (k[:, 0] - x) / w * INPUT[0]
        k[:, 1] = (k[:, 1] - y) / h * INPUT[1]
        enc = orc.probmap_encode(k[None, :, :2], k[None, :, 2] == 2, INPUT, HEAT, sigmas, -1)
        out.append((img, enc["heatmaps"]))
    return out


def stats(ts):
    return dict(ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dataset_bench needs the GPU: there is nothing to time without it"
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    sigmas = np.full(K, 0.05)
    ds = YOLOPoseDataset.__new__(YOLOPoseDataset)              # no tree on disk: the samples are made in memory
    ds.codec, ds.annotations, ds._staging = Codec(ArgMaxProbMap(INPUT, HEAT, sigmas)), [], []
    frame, samples, boxes = make_samples()
    src_bytes = sum(s[0].size for s in samples)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    for _ in range(args.warmup):
        img, gt = ds.collate(samples)
    torch.cuda.synchronize()
    # the collated batch is the CPU path's, bit for bit (checked here at the timed size)
    ref = cpu_path(frame, samples, boxes, sigmas)
    assert all(np.array_equal(img[b].cpu().numpy(), ref[b][0]) for b in range(B)), "crops differ from Pillow"
    assert all(np.array_equal(gt["heatmaps"][b].cpu().numpy(), ref[b][1]) for b in range(B)), "maps differ"
    up = ds._upload(samples)
    packed_bytes, plan_bytes = int(up[0].numel()), int(up[1].numel())       # the two copies of a batch
    device, copies, host = [], [], []
    for _ in range(args.repeats):
        up = ds._upload(samples)
        torch.cuda.synchronize()
        a, b = ev(), ev()
        a.record()
        for _ in range(args.steps):
            ds._launch(*up)
        b.record()
        b.synchronize()
        device.append(a.elapsed_time(b) / args.steps)
        a, b = ev(), ev()
        t0 = time.perf_counter()
        a.record()
        for _ in range(args.steps):
            ds.collate(samples)
        b.record()
        t1 = time.perf_counter()
        b.synchronize()
        host.append((t1 - t0) * 1e3 / args.steps)
        copies.append(a.elapsed_time(b) / args.steps)
    cpu = []
    for _ in range(args.cpu_repeats):
        t0 = time.perf_counter()
        cpu_path(frame, samples, boxes, sigmas)
        cpu.append((time.perf_counter() - t0) * 1e3)
    res = dict(batch=B, input=INPUT, heatmap=HEAT, K=K, steps=args.steps, repeats=args.repeats, warmup=args.warmup,
               source_bytes=src_bytes, copy_pixels_bytes=packed_bytes, copy_plan_bytes=plan_bytes,
               image_bytes=B * 3 * INPUT[0] * INPUT[1] * 4,
               heatmap_bytes=B * K * HEAT[0] * HEAT[1] * 4, staging_buffers=len(ds._staging),
               device_three_launches=stats(device), device_collate_with_copies=stats(copies),
               host_collate_wall=stats(host), cpu_reference_path_one_thread=stats(cpu))
    res["samples_per_s"] = dict(device=round(B / (res["device_three_launches"]["ms_median"] * 1e-3)),
                                host=round(B / (res["host_collate_wall"]["ms_median"] * 1e-3)),
                                cpu_one_thread=round(B / (res["cpu_reference_path_one_thread"]["ms_median"] * 1e-3)))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
