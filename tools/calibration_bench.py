"""HIP-event time of the three HeadCalibration kernels, at K = 17 / B = 64 and K = 133 / B = 256.

The meter is fed 32 batches of matched head arrays whose labels follow the prediction with noise (label ~
Bernoulli(p^1.5), achieved OKS = clamp(x^1.5 + noise)): a reliability curve that rises with local violations, the input
isotonic regression is meant for.  ``pp_calib_fit`` is timed on that state and on one whose labels run against the
prediction (label ~ Bernoulli(1 - p)), where every row pools into a few blocks; ``pp_calib_score`` on the first;
``pp_calib_apply`` in place on a [3,B,K] tensor, next to the torch ops it follows in ``ArgMaxProbMap.decode_device``
(``reshape`` / ``float`` / ``stack`` of the three heads).

Launches are issued back to back behind queued matrix products that keep the GPU busy while the host issues them, so
the events see device time only (the method of tools/valmeter_bench.py).  A table on stdout and in ``--out``, then one
JSON line.  No time here is a pass criterion.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from valmeter_bench import Blocker  # noqa: E402


def device_us(fn, blocker, launches=200, repeats=7):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
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
    return dict(us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2))


def fed_meter(B, K, batches, against, seed):
    from probpose_pytorch_amd import ValidationMeter
    g = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda: torch.rand(B, K, device="cuda", generator=g)       # noqa: E731
    meter = ValidationMeter(None)
    ones = torch.ones((B, K), dtype=torch.int32, device="cuda")
    for _ in range(batches):
        prob, vis, oks = rand(), rand(), rand()
        rate = (lambda p: 1 - p) if against else (lambda p: p ** 1.5)
        in_image = (rand() < rate(prob)).int()
        visibility = (rand() < rate(vis)).int()
        gt_oks = (rate(oks) + (rand() - 0.5) * 0.3).clamp_(0, 1)
        # every sample annotated and in the image for the visibility / OKS populations of this bench
        meter.update_heads(prob, vis, oks, rand() * 30, in_image, ones, visibility, gt_oks, rand() * 30)
        meter.update_heads(prob, vis, oks, rand() * 30, ones, ones, visibility, gt_oks, rand() * 30)
    return meter


def kernel_times(B, K, blocker, batches=32):
    from probpose_pytorch_amd import HeadCalibration, _lib
    from probpose_pytorch_amd.calibration import score_fields
    out = {}
    meters = {"rising": fed_meter(B, K, batches, False, 1), "against": fed_meter(B, K, batches, True, 2)}
    cal = HeadCalibration.fit(meters["rising"])
    for name, meter in meters.items():
        state, _, J = meter.device_state()
        out[f"fit ({name})"] = device_us(
            lambda: _lib.launch("pp_calib_fit", state, K, J, 1000, cal.blocks, cal.table, cal.row_of), blocker)
    cal = HeadCalibration.fit(meters["rising"])
    blocks = cal.blocks.cpu()
    out["blocks_per_row"] = round(float((blocks[:, :, 1:] != blocks[:, :, :-1]).any(-1).sum(-1).float().mean()) + 1, 1)
    rep = torch.empty((K + 1, score_fields(16)), dtype=torch.float64, device="cuda")
    state, _, J = meters["rising"].device_state()
    out["score"] = device_us(
        lambda: _lib.launch("pp_calib_score", state, K, J, cal.table, cal.row_of, 16, rep), blocker)
    g = torch.Generator(device="cuda").manual_seed(3)
    heads = [torch.rand(B, K, 1, 1, device="cuda", generator=g) for _ in range(3)]
    aux = torch.stack([t.reshape(B, K).float() for t in heads])
    out["apply (in place)"] = device_us(lambda: _lib.launch("pp_calib_apply", aux, aux, B, K, cal.table, cal.row_of),
                                        blocker)
    out["torch reshape/float/stack before it"] = device_us(
        lambda: torch.stack([t.reshape(B, K).float() for t in heads]), blocker)
    out["samples_per_head"] = int(meters["rising"].state["hist"][0].sum())
    out["table_bytes"] = int(cal.table.numel()) * 4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "calibration_bench needs the GPU: there is nothing to time without it"
    blocker = Blocker()
    res = {f"{b}x{k}": kernel_times(b, k, blocker) for b, k in ((64, 17), (256, 133))}
    rows = [f"{'kernel alone (HIP events, device busy)':<52}{'us median':>10}{'min':>9}{'max':>9}"]
    for shape, d in res.items():
        for name, v in d.items():
            if isinstance(v, dict):
                label = name if name.startswith("torch") else "pp_calib_" + name
                rows.append(f"{label + '  B x K = ' + shape:<52}{v['us_median']:>10.2f}{v['us_min']:>9.2f}"
                            f"{v['us_max']:>9.2f}")
        rows.append(f"  {d['samples_per_head']} samples in the probability head, {d['blocks_per_row']} blocks per "
                    f"fitted row (rising), table {d['table_bytes']} B")
    table = "\n".join(rows)
    print(table)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
