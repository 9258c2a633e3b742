"""probpose.viz beside the same pictures made with plain torch device ops.

  overlay    overlay_heatmap_on_image on 64 crops of 256 x 192 with K = 17 maps of 64 x 48 (upsampled in the kernel)
  colorize   colorize of the same maps (and with normalize=True)
  draw       draw_keypoints on one 1920 x 1080 frame with 20 poses of 17 keypoints and the COCO skeleton

The torch baselines do what a user would write without the kernels: bilinear ``interpolate`` (float32), index the
colour table, sum over k, clamp, add; a table gather for colorize; one masked assignment per primitive on its bounding
window for draw.  The draw baseline is integer arithmetic and must give the same bytes (asserted); the overlay baseline
interpolates in float32, so the share of equal bytes is reported instead.

`--repeats` rounds (default 10); in each round one window of `--steps` calls of each path, alternating, HIP-event time
per call; median, min and max over the rounds.  GB/s are the algorithmic bytes (every input and output byte once) over
the median time, next to the 8 TB/s HBM figure of DESIGN §4.  `launch` is the time between two HIP events around the
pp_viz_* launch alone (`ops.set_profile`), over `--steps` launches: the call without its Python and torch side.  There
is no threshold.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TB_PER_S = 8.0


def stats(ts):
    return dict(ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))


def torch_overlay(images, maps, lut):
    B, H, W, _ = images.shape
    v = torch.nn.functional.interpolate(maps, size=(H, W), mode="bilinear", align_corners=True)
    acc = torch.zeros((B, H, W, 3), dtype=torch.float64, device=images.device)
    for k in range(maps.shape[1]):
        vk = v[:, k]
        acc += lut[(vk * 256.0).clamp(0, 255).long()] * (vk >= 0.01).unsqueeze(-1)
    add = (acc * 255.0).clamp(max=255.0).to(torch.int16)
    return (images.to(torch.int16) + add).clamp(max=255).to(torch.uint8)


def torch_colorize(maps, lut_rgba, normalize):
    if normalize:
        maps = maps / maps.amax(dim=(-2, -1), keepdim=True)
    return lut_rgba[(maps * 256.0).clamp(0, 255).long()]


def torch_draw(frame, kpts, probs, threshold, radius, skeleton, line_width):
    """kpts / probs are host arrays here: the baseline places its windows on the host."""
    out = frame.clone()
    H, W, _ = frame.shape
    red = torch.tensor([255, 0, 0], dtype=torch.uint8, device=frame.device)
    centres = [[(int(x), int(y)) if p >= threshold and 0 <= int(x) < W and 0 <= int(y) < H else None
                for (x, y), p in zip(kp, pr)] for kp, pr in zip(kpts, probs)]

    def window(x0, x1, y0, y1):
        x0, x1, y0, y1 = max(x0, 0), min(x1, W - 1), max(y0, 0), min(y1, H - 1)
        yy = torch.arange(y0, y1 + 1, device=frame.device)[:, None]
        xx = torch.arange(x0, x1 + 1, device=frame.device)[None, :]
        return out[y0:y1 + 1, x0:x1 + 1], xx, yy

    pad = (line_width + 1) // 2
    for c in centres:
        for i, j in skeleton:
            if c[i] is None or c[j] is None or c[i] == c[j]:
                continue
            (ax, ay), (bx, by) = c[i], c[j]
            view, xx, yy = window(min(ax, bx) - pad, max(ax, bx) + pad, min(ay, by) - pad, max(ay, by) + pad)
            dx, dy = bx - ax, by - ay
            ex, ey = xx - ax, yy - ay
            t, L2 = ex * dx + ey * dy, dx * dx + dy * dy
            d2 = torch.where(t <= 0, 4 * (ex * ex + ey * ey) * L2,
                             torch.where(t >= L2, 4 * ((xx - bx) ** 2 + (yy - by) ** 2) * L2, 4 * (ex * dy - ey * dx) ** 2))
            view.copy_(torch.where((d2 <= line_width * line_width * L2).unsqueeze(-1), red, view))
    for c in centres:
        for p in c:
            if p is not None:
                view, xx, yy = window(p[0] - radius, p[0] + radius, p[1] - radius, p[1] + radius)
                inside = (xx - p[0]) ** 2 + (yy - p[1]) ** 2 <= radius * radius + radius
                view.copy_(torch.where(inside.unsqueeze(-1), red, view))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "viz_bench needs the GPU: there is nothing to time without it"
    from probpose_pytorch_amd import viz
    rng = np.random.default_rng(0)
    B, K, H, W, h, w = 64, 17, 256, 192, 64, 48
    images = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    maps = torch.from_numpy(rng.random((B, K, h, w), dtype=np.float32) ** 8).cuda()        # peaked, mostly below 0.01
    FH, FW, N = 1080, 1920, 20
    frame = torch.from_numpy(rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8)).cuda()
    kp_host = rng.uniform(0, 1, (N, 17, 2)) * (FW, FH)
    pr_host = rng.uniform(0.85, 1.0, (N, 17))
    kpts, probs = torch.from_numpy(kp_host).cuda(), torch.from_numpy(pr_host).cuda()
    index = torch.zeros(N, dtype=torch.int64, device="cuda")
    lut = torch.from_numpy(viz.colormap_table("jet")).cuda()
    inferno = viz.colormap_table("inferno")
    lut_rgba = torch.from_numpy(np.concatenate([(inferno * 255.0).astype(np.uint8),
                                                np.full((256, 1), 255, np.uint8)], axis=1)).cuda()
    o_img, o_rgba, o_frame = torch.empty_like(images), torch.empty(maps.shape + (4,), dtype=torch.uint8,
                                                                   device="cuda"), torch.empty_like(frame)
    draw_kw = dict(threshold=0.9, radius=5, skeleton=viz.COCO17_SKELETON, line_width=2)
    paths = {
        "overlay": lambda: viz.overlay_heatmap_on_image(images, maps, "jet", out=o_img),
        "overlay_torch": lambda: torch_overlay(images, maps, lut),
        "colorize": lambda: viz.colorize(maps, "inferno", False, out=o_rgba),
        "colorize_torch": lambda: torch_colorize(maps, lut_rgba, False),
        "colorize_normalize": lambda: viz.colorize(maps, "inferno", True, out=o_rgba),
        "colorize_normalize_torch": lambda: torch_colorize(maps, lut_rgba, True),
        "draw": lambda: viz.draw_keypoints(frame, kpts, probs, image_index=index, out=o_frame, **draw_kw),
        "draw_torch": lambda: torch_draw(frame, kp_host, pr_host, 0.9, 5, viz.COCO17_SKELETON, 2),
    }
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    # the timed paths agree, at the timed sizes
    assert torch.equal(paths["draw"](), paths["draw_torch"]()), "draw_keypoints differs from the torch baseline"
    assert torch.equal(paths["colorize"](), paths["colorize_torch"]()), "colorize differs from the torch baseline"
    same = float((paths["overlay"]() == paths["overlay_torch"]()).float().mean())

    def window(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    t = {name: [] for name in paths}
    for _ in range(args.repeats):
        for name, fn in paths.items():
            t[name].append(window(fn))
    # the launches alone: HIP events around each pp_viz_* launch (ops.set_profile), `--steps` launches a path
    from probpose_pytorch_amd import ops
    launch = {}
    for name in ("overlay", "colorize", "colorize_normalize", "draw"):
        sink = []
        ops.set_profile(sink)
        for _ in range(args.steps):
            paths[name]()
        ops.set_profile(None)
        torch.cuda.synchronize()
        launch[name] = stats([rec[2].elapsed_time(rec[3]) for rec in sink])
    nbytes = dict(overlay=2 * images.numel() + 4 * maps.numel(), colorize=8 * maps.numel(),
                  colorize_normalize=8 * maps.numel(), draw=2 * frame.numel())
    res = dict(steps=args.steps, repeats=args.repeats, warmup=args.warmup, crops=(B, H, W), maps=(K, h, w),
               frame=(FH, FW), poses=N, hbm_TB_per_s=HBM_TB_PER_S, overlay_bytes_equal_to_torch=round(same, 6))
    for name in paths:
        res[name] = stats(t[name])
    for name, n in nbytes.items():
        res[name]["bytes"] = n
        res[name]["GB_per_s"] = round(n / (res[name]["ms_median"] * 1e-3) / 1e9, 1)
        res[name]["of_hbm"] = round(res[name]["GB_per_s"] / (HBM_TB_PER_S * 1e3), 4)
        res[name]["launch"] = launch[name]
        res[name]["launch_GB_per_s"] = round(n / (launch[name]["ms_median"] * 1e-3) / 1e9, 1)
        res[name]["speedup_over_torch"] = round(res[name + "_torch"]["ms_median"] / res[name]["ms_median"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
