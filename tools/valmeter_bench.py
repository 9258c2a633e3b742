"""A validation pass on the GPU: the per-batch way against ValidationMeter, 32 batches of B=64, K=17, 64x48 maps, with
the ground truth on the device as ``YOLOPoseDataset.collate`` delivers it.

  (a) ``loss_fn(gt, pred, compute_acc=True)`` per batch, the ten numbers read and averaged on the host as
      train.py:146-167 does
  (b) ``meter.update(gt, pred)`` per batch and one ``meter.compute()``

Wall-clock per pass (host clock around a pass that ends in a device synchronise), the two alternating in one process
after a warm-up pass of each: median, min and max over ``--repeats`` passes.  The host synchronisations of one pass
each way are counted in a separate, untimed pass under ``torch.cuda.set_sync_debug_mode("warn")``.  HIP-event time of
``pp_valmeter_update`` and ``pp_valmeter_report`` alone: launches issued back to back behind queued matrix products that
keep the GPU busy while the host issues them, so the events see device time only; at the pass's shape and at
B*K = 256 x 133.  A table on stdout and in ``--out``, then one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COCO17_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
LOSS_KEYS = ("kpt", "probability", "visibility", "oks", "error")


def make_batches(n, B, K, H, W, input_size, codec, seed=0):
    """Seeded (gt, pred) pairs on the device: encoded targets, peaked noisy predictions, random scalar heads."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=g)      # noqa: E731
    size = torch.tensor(input_size, device="cuda", dtype=torch.float32)
    scale = (size - 1) / torch.tensor([W - 1, H - 1], device="cuda", dtype=torch.float32)
    out = []
    for _ in range(n):
        kps = (rand(B, K, 2) * 1.2 - 0.1) * size
        annotated = rand(B, K) > 0.25
        gt_hm, _ = codec.probmap.encode_device_tensors((kps / scale).contiguous(), annotated.float())
        in_image = ((kps >= 0) & (kps < size)).all(-1)
        gt = dict(heatmaps=gt_hm, in_image=in_image[:, None, :], keypoints_visible=annotated[:, None, :],
                  keypoints_visibility=(rand(B, 1, K) > 0.4).float())
        hm = (gt_hm * 0.9 + rand(B, K, H, W) * 0.15).clamp_(0, 1)
        heads = [rand(B, K, 1, 1) * 0.98 + 0.01 for _ in range(3)] + [rand(B, K, 1, 1) * 40.0]
        out.append((gt, (hm, *heads)))
    return out


def pass_a(loss_fn, batches):
    sums = {f"loss_{k}": 0.0 for k in LOSS_KEYS} | {f"acc_{k}": 0.0 for k in LOSS_KEYS}
    with torch.no_grad():
        for gt, pred in batches:
            losses, accs = loss_fn(gt, pred, compute_acc=True)
            for k in LOSS_KEYS:
                sums[f"loss_{k}"] += losses[k].item()
                sums[f"acc_{k}"] += accs[k].item()
    return {k: v / len(batches) for k, v in sums.items()}


def pass_b(meter, batches):
    meter.reset()
    for gt, pred in batches:
        meter.update(gt, pred)
    return meter.compute()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def count_syncs(fn):
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    return sum("synchroniz" in str(w.message).lower() for w in seen)


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


def kernel_times(B, K, blocker, launches=200, repeats=7):
    """Device us per launch of pp_valmeter_update (all optional inputs given) and pp_valmeter_report."""
    from probpose_pytorch_amd import _lib
    from probpose_pytorch_amd.valmeter import ValidationMeter, report_fields
    meter = ValidationMeter(None)
    g = torch.Generator(device="cuda").manual_seed(1)
    f = [torch.rand(B, K, device="cuda", generator=g) for _ in range(6)]
    m = [(torch.rand(B, K, device="cuda", generator=g) < 0.7).int() for _ in range(3)]
    meter.update_heads(*f[:4], *m, f[4], f[5])
    state, _, J = meter.device_state()
    pck = torch.ones((2, K), dtype=torch.int32, device="cuda")
    res = torch.zeros((11,), dtype=torch.float32, device="cuda")
    rep = torch.empty((K + 1, report_fields(J, meter.ece_bins)), dtype=torch.float64, device="cuda")

    def update():
        _lib.launch("pp_valmeter_update", *f[:4], f[4], f[5], *m, meter._thr, J, pck, f[0], res, B, K, state)

    def report():
        _lib.launch("pp_valmeter_report", state, meter._thr, K, J, meter.ece_bins, rep)

    out = {}
    for name, fn in (("update", update), ("report", report)):
        t0 = time.perf_counter()
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        us = []
        for _ in range(repeats):
            blocker(1.5 * host_ms + 2.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / launches)
        out[name] = dict(us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2))
    out["state_bytes"] = int(state.numel()) * 8
    out["report_bytes"] = int(rep.numel()) * 8
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "valmeter_bench needs the GPU: there is nothing to time without it"
    from probpose_pytorch_amd import Codec, ProbMap, ValidationMeter
    from probpose_pytorch_amd.loss import ProbPoseLoss
    B, K, H, W, input_size = 64, 17, 64, 48, (192, 256)
    codec = Codec(ProbMap(input_size, (W, H), COCO17_SIGMAS))
    loss_fn = ProbPoseLoss(codec)
    batches = make_batches(args.batches, B, K, H, W, input_size, codec)
    meter = ValidationMeter(loss_fn)
    np.random.seed(0)
    ways = {"a": lambda: pass_a(loss_fn, batches), "b": lambda: pass_b(meter, batches)}
    first = {k: fn() for k, fn in ways.items()}          # warm-up, and the two views of the same set
    ms = {k: [] for k in ways}
    for _ in range(args.repeats):
        for k, fn in ways.items():
            ms[k].append(timed(fn))
    syncs = {k: count_syncs(fn) for k, fn in ways.items()}
    blocker = Blocker()
    kern = {f"{b}x{k}": kernel_times(b, k, blocker) for b, k in ((B, K), (256, 133))}
    agree = {k: [first["a"][f"loss_{k}"], first["b"]["reference"][f"loss_{k}"]] for k in LOSS_KEYS}
    res = dict(batches=args.batches, B=B, K=K, H=H, W=W, repeats=args.repeats, syncs_per_pass=syncs, kernels=kern,
               loss_means_a_b=agree)
    rows = [f"validation pass: {args.batches} batches, B={B}, K={K}, {H}x{W} maps, gt on the device; "
            f"{args.repeats} passes each way, alternating", "",
            f"{'way':<44}{'ms median':>10}{'min':>9}{'max':>9}{'host syncs / pass':>19}"]
    for k, label in (("a", "(a) loss_fn(compute_acc=True) + host means"), ("b", "(b) meter.update + one compute()")):
        res[k] = dict(ms_median=round(statistics.median(ms[k]), 3), ms_min=round(min(ms[k]), 3),
                      ms_max=round(max(ms[k]), 3))
        rows.append(f"{label:<44}{res[k]['ms_median']:>10.3f}{res[k]['ms_min']:>9.3f}{res[k]['ms_max']:>9.3f}"
                    f"{syncs[k]:>19d}")
    rows += ["", f"{'kernel alone (HIP events, device busy)':<44}{'us median':>10}{'min':>9}{'max':>9}"]
    for shape, d in kern.items():
        for name in ("update", "report"):
            rows.append(f"{'pp_valmeter_' + name + ' B x K = ' + shape:<44}{d[name]['us_median']:>10.2f}"
                        f"{d[name]['us_min']:>9.2f}{d[name]['us_max']:>9.2f}")
        rows.append(f"  state {d['state_bytes']} B, report {d['report_bytes']} B")
    table = "\n".join(rows)
    print(table)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
