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

`--augment` adds the augmented batch (Augment defaults with shift 0.1 and eight flip pairs; the regions are the bounding
rectangles of the transformed boxes, cut from the same frame) to the same process, its windows alternating with the
un-augmented ones: the three launches together and one by one (warp, keypoints, maps; the LANCZOS launch it replaces
beside the warp), a whole collate() in HIP-event and in host time, and the warp's store bandwidth.  Behind the warp
window of the same run it times the blur / erasing launch (pp_augment_post) on the warp's output in three
variants: erase-only in place (one hole per sample of Augment's default erase_size), a 7x7 box blur of every sample
and a 5x5 median of every sample, both into a second tensor; and a whole collate() of 6-tuples with blur, median blur
and erasing switched on.
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


def make_augmented_samples(frame, samples, augment):
    """What __getitem__ hands over with augment set, for the boxes of make_samples, from the frame in memory."""
    import PIL.Image
    from probpose_pytorch_amd.dataset import augment_region
    image = PIL.Image.fromarray(frame, "RGB")
    out = []
    for idx, (_, kps, bbox) in enumerate(samples):
        params = augment.draw(0, idx)
        x0, y0, x1, y1 = augment_region(bbox, params)
        region = np.ascontiguousarray(np.asarray(image.crop((x0, y0, x1, y1)), dtype=np.uint8))
        out.append((region, kps, bbox, np.array([x0, y0], dtype=np.int64), params))
    return out


def stats(ts):
    return dict(ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--augment", action="store_true", help="also time the augmented batch, alternating windows")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dataset_bench needs the GPU: there is nothing to time without it"
    from probpose_pytorch_amd._buffers import PinnedStaging
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    sigmas = np.full(K, 0.05)
    ds = YOLOPoseDataset.__new__(YOLOPoseDataset)              # no tree on disk: the samples are made in memory
    ds.codec, ds.annotations, ds._staging = Codec(ArgMaxProbMap(INPUT, HEAT, sigmas)), [], PinnedStaging()
    ds.augment, ds.epoch, ds._perm = None, 0, None
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
    aug = None
    if args.augment:
        from probpose_pytorch_amd import _lib, frontend
        from probpose_pytorch_amd.dataset import Augment
        ds.augment = Augment(flip_pairs=[(2 * i + 1, 2 * i + 2) for i in range(8)], shift=0.1)
        aug_samples = make_augmented_samples(frame, samples, ds.augment)
        for _ in range(args.warmup):
            ds.collate(aug_samples)
        torch.cuda.synchronize()
        aug = dict(device=[], copies=[], host=[], warp=[], keypoints=[], maps=[], lanczos=[], erase=[], box7=[],
                   median5=[], post_host=[], post_copies=[])
        eraser = Augment(erase_prob=1.0)
        post_records = dict(
            erase=np.stack([eraser.draw_post(0, i, INPUT) for i in range(B)]),
            box7=np.tile(np.array([1, 7] + [0] * 22, dtype=np.int32), (B, 1)),
            median5=np.tile(np.array([2, 5] + [0] * 22, dtype=np.int32), (B, 1)))
        for name, rec in post_records.items():
            _lib.call("pp_augment_post_check", B, rec, INPUT[0], INPUT[1], 0 if name == "erase" else 1)
        d_records = {name: torch.from_numpy(rec).cuda() for name, rec in post_records.items()}
        post_ds = YOLOPoseDataset.__new__(YOLOPoseDataset)
        post_ds.__dict__.update(ds.__dict__)
        post_ds._staging, post_ds._perm = PinnedStaging(), None
        post_ds.augment = Augment(flip_pairs=ds.augment.flip_pairs, shift=0.1, blur_prob=0.3, median_prob=0.3,
                                  erase_prob=0.5, erase_holes=(1, 4))
        post_samples = [s + (post_ds.augment.draw_post(0, i, INPUT),) for i, s in enumerate(aug_samples)]
        for _ in range(args.warmup):
            post_ds.collate(post_samples)
        torch.cuda.synchronize()
        L, pm = _lib.lib(), ds.codec.probmap
        sx, sy = (float(v) for v in np.asarray(pm.scale_factor, dtype=np.float32))

    def window(fn):
        """HIP-event time per call of `--steps` calls of fn, the queue drained before."""
        torch.cuda.synchronize()
        a, b = ev(), ev()
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    for _ in range(args.repeats):
        if aug is not None:
            up_plain = ds._upload(samples)
            d_src, d_meta, d_perm, _, _ = up_a = ds._upload_augmented(aug_samples)
            meta = d_meta.data_ptr()
            img = torch.empty((B, 3, INPUT[1], INPUT[0]), dtype=torch.float32, device="cuda")
            f32 = torch.empty((6, B, K), dtype=torch.float32, device="cuda")
            flags = torch.empty((2, B, K), dtype=torch.bool, device="cuda")
            kp_hm = f32[2:4].view(B, K, 2)
            aug["device"].append(window(lambda: ds._launch_augmented(*up_a)))
            aug["warp"].append(window(lambda: L.pp_augment_warp(_lib.ptr(d_src), meta, meta + 32 * B, B, INPUT[0],
                                                                INPUT[1], _lib.ptr(img), _lib.stream_ptr())))
            img2 = torch.empty_like(img)
            aug["erase"].append(window(lambda: L.pp_augment_post(_lib.ptr(img), _lib.ptr(d_records["erase"]), B, INPUT[0],
                                                                 INPUT[1], 0, _lib.ptr(img), _lib.stream_ptr())))
            for name in ("box7", "median5"):
                aug[name].append(window(lambda: L.pp_augment_post(_lib.ptr(img), _lib.ptr(d_records[name]), B, INPUT[0],
                                                                  INPUT[1], 1, _lib.ptr(img2), _lib.stream_ptr())))
            aug["lanczos"].append(window(lambda: frontend.crop_resize_multi(up_plain[0], up_plain[1], B, up_plain[4],
                                                                            up_plain[5], INPUT)))
            aug["keypoints"].append(window(lambda: L.pp_dataset_ground_truth_affine(
                meta + 128 * B, meta + 96 * B, _lib.ptr(d_perm), B, K, INPUT[0], INPUT[1], sx, sy, _lib.ptr(f32[0:2]),
                _lib.ptr(kp_hm), _lib.ptr(f32[4]), _lib.ptr(flags[0]), _lib.ptr(flags[1]), _lib.ptr(f32[5]),
                _lib.stream_ptr())))
            aug["maps"].append(window(lambda: pm.encode_device_tensors(kp_hm, f32[4])))
            torch.cuda.synchronize()
            a, b = ev(), ev()
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.steps):
                ds.collate(aug_samples)
            b.record()
            t1 = time.perf_counter()
            b.synchronize()
            aug["host"].append((t1 - t0) * 1e3 / args.steps)
            aug["copies"].append(a.elapsed_time(b) / args.steps)
            aug["bytes"] = (int(d_src.numel()), int(d_meta.numel()))
            torch.cuda.synchronize()
            a, b = ev(), ev()
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.steps):
                post_ds.collate(post_samples)
            b.record()
            t1 = time.perf_counter()
            b.synchronize()
            aug["post_host"].append((t1 - t0) * 1e3 / args.steps)
            aug["post_copies"].append(a.elapsed_time(b) / args.steps)
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
    if aug is not None:
        image_bytes = res["image_bytes"]
        res["augment"] = dict(
            copy_pixels_bytes=aug["bytes"][0], copy_meta_bytes=aug["bytes"][1],
            device_three_launches=stats(aug["device"]), warp=stats(aug["warp"]),
            lanczos_launch_it_replaces=stats(aug["lanczos"]), keypoints=stats(aug["keypoints"]),
            maps=stats(aug["maps"]), device_collate_with_copies=stats(aug["copies"]),
            host_collate_wall=stats(aug["host"]),
            warp_store_TB_per_s=round(image_bytes / (statistics.median(aug["warp"]) * 1e-3) / 1e12, 3))
        warp_ms = statistics.median(aug["warp"])
        res["augment"]["post"] = dict(
            erase_only_in_place=stats(aug["erase"]), box_k7=stats(aug["box7"]), median_k5=stats(aug["median5"]),
            ratio_to_warp={k: round(statistics.median(aug[k]) / warp_ms, 3) for k in ("erase", "box7", "median5")},
            box_k7_read_plus_write_TB_per_s=round(2 * image_bytes / (statistics.median(aug["box7"]) * 1e-3) / 1e12, 3),
            median_k5_read_plus_write_TB_per_s=round(2 * image_bytes / (statistics.median(aug["median5"]) * 1e-3) / 1e12,
                                                     3),
            settings=dict(blur_prob=0.3, median_prob=0.3, erase_prob=0.5, erase_holes=[1, 4]),
            device_collate_with_copies=stats(aug["post_copies"]), host_collate_wall=stats(aug["post_host"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
