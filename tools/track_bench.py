"""PoseTracker on the GPU beside the same rules in vectorised numpy on the host.

Synthetic video, K = 17: `--streams` streams (64) of `--people` people each (20 and 100), `--frames` frames (200).  People
have a side of 40, 60 or 150 (x 0.8 .. 1.25), drift by at most 1.5 % of it per frame and axis and jitter by 2 % per
keypoint, as tests/track_reference.make_scene; everybody is in every frame, shuffled.  Detections are float32 device
tensors, as a decoder leaves them.  The frames are walked forwards and backwards, so the motion stays continuous.

  update       one PoseTracker.update (One-Euro on, max_tracks 128): the layout from the stream ids (host), casts, the
               finiteness readback, two stable sorts, gathers, the three launches, scatters
  launches     pp_track_oks, pp_track_assign and pp_track_filter of one such call alone, on its sorted batch (with their
               workspace and output allocations), replayed with advancing time
  propose      one PoseTracker.propose_boxes over the 64 streams of the tracker the update variant drives (pad 1.25,
               extrapolation on, no frame, no suppression): the block addresses through a pinned upload, four output
               allocations, the one launch; nothing is read back
  propose_launch  pp_track_boxes of one such call alone (with its output allocations), replayed
  assign_greedy, assign_optimal, update_optimal   with `--assign optimal`: pp_track_assign and pp_track_assign_optimal
               alone (with their output allocations) on one OKS workspace and one state, those of the second frame of a
               tracker that has seen the first, so every detection has its track; and `update` of a tracker built with
               assign="optimal".  `optimal_over_greedy` holds the ratios of the medians
  update_predict_*, update_cascade_*, update_predict_cascade_*   with `--stage`: `update` of trackers built with
               predict=True, with high_thr 0.5 / birth_thr 0.6, and with both, for assign greedy and optimal (beside
               `update` and `update_optimal`, which `--stage` times too)
  host_numpy   the same rules on the host: the D2H copy of keypoints, areas and scores, then per stream a vectorised
               OKS matrix, the greedy walk over the detections, vectorised ageing, births and One-Euro steps

HIP-event time per call: every variant is warmed up, a window is `--window-ms` of calls (the number of calls is
calibrated per variant), `--repeats` windows per variant, the variants alternating; median, min and max of the windows.
The host variant is bracketed by the same events (its D2H copies wait for the device, so the events see its whole
time).  `ids_agree` says whether the host variant assigned the ids the device did over the first frames.  One JSON line.
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
K, MAX_TRACKS, MATCH_THR, MAX_AGE, FPS = 17, 128, 0.3, 30, 30.0
# --stage: the update with motion prediction, with the two-stage association (ByteTrack's usual thresholds; the scores
# are uniform in (0.05, 0.99), so about half the detections are rows of stage 2), and with both
STAGE_VARIANTS = {"predict": dict(predict=True), "cascade": dict(high_thr=0.5, birth_thr=0.6),
                  "predict_cascade": dict(predict=True, high_thr=0.5, birth_thr=0.6)}
EPS = float(np.spacing(1.0))
TWO_PI = 2.0 * np.pi


def make_video(S, P, F, seed):
    """F frames on the device: list of (stream ids [S * P] (host), kpts [S * P, K, 2] f32, area f32, score f32)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=g, dtype=torch.float64)
    side = (torch.tensor([40.0, 60.0, 150.0], device="cuda", dtype=torch.float64)[
        torch.randint(0, 3, (S, P), device="cuda", generator=g)] * (0.8 + 0.45 * rand(S, P)))
    cols = int(math.ceil(math.sqrt(P)))
    grid = torch.stack([torch.arange(P, device="cuda") % cols, torch.arange(P, device="cuda") // cols], dim=1) * 420.0
    base = (grid[None, :, None, :] + rand(S, P, 1, 2) * 60) + rand(S, P, K, 2) * side[..., None, None]
    drift = (rand(S, P, 1, 2) - 0.5) * 0.03 * side[..., None, None]
    ids = np.repeat(np.arange(S, dtype=np.int64), P)
    frames = []
    for f in range(F):
        kp = base + drift * f + (rand(S, P, K, 2) * 2 - 1) * 0.02 * side[..., None, None]
        area = 0.6 * side * side * (0.95 + 0.1 * rand(S, P))
        score = 0.05 + 0.94 * rand(S, P)
        order = torch.argsort(rand(S, P), dim=1)
        take = lambda a: torch.gather(a, 1, order.reshape(order.shape + (1,) * (a.ndim - 2)).expand_as(a))
        frames.append((ids, take(kp).reshape(S * P, K, 2).float().contiguous(), take(area).reshape(-1).float(),
                       take(score).reshape(-1).float()))
    return frames


class HostTracker:
    """The rules of probpose_pytorch_amd/tracker.py in numpy float64 on the host, vectorised per stream."""

    def __init__(self, S, smooth=(1.0, 0.05, 1.0)):
        T = MAX_TRACKS
        self.id = np.full((S, T), -1, dtype=np.int64)
        self.age = np.zeros((S, T), dtype=np.int32)
        self.t_last, self.area = np.zeros((S, T)), np.zeros((S, T))
        self.kp, self.xhat, self.dxhat = (np.zeros((S, T, K, 2)) for _ in range(3))
        self.next_id = np.zeros(S, dtype=np.int64)
        self.overflow = np.zeros(S, dtype=np.int64)
        self.vars, self.smooth, self.calls = (SIGMAS * 2) ** 2, smooth, 0

    def update(self, ids, kp_dev, area_dev, score_dev):
        kp_all = kp_dev.cpu().numpy().astype(np.float64)        # the D2H copy of the decoded poses it needs
        ar_all, sc_all = area_dev.cpu().numpy().astype(np.float64), score_dev.cpu().numpy().astype(np.float64)
        self.calls += 1
        t = self.calls / FPS
        out_ids, out_kp = np.full(ids.shape[0], -1, dtype=np.int64), kp_all.copy()
        bounds = np.flatnonzero(np.diff(ids, prepend=ids[0] - 1, append=ids[-1] + 1))
        mc, beta, dc = self.smooth
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            s = int(ids[lo])
            kp, ar, sc = kp_all[lo:hi], ar_all[lo:hi], sc_all[lo:hi]
            live = self.id[s] >= 0
            d = kp[:, None] - self.kp[s][None]
            e = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) / self.vars / (
                (ar[:, None] + self.area[s][None]) / 2 + EPS)[..., None] / 2
            oks = np.where(live[None], np.exp(-e).sum(axis=2) / K, -1.0)
            order = np.argsort(-sc, kind="stable")
            slot = np.full(hi - lo, -1, dtype=np.int64)
            free = live.copy()
            for i in order:
                row = np.where(free, oks[i], -1.0)
                j = int(row.argmax())
                if row[j] > MATCH_THR:
                    slot[i], free[j] = j, False
            lost = live & free
            self.age[s][lost] += 1
            self.id[s][lost & (self.age[s] > MAX_AGE)] = -1
            m = np.flatnonzero(slot >= 0)
            j = slot[m]
            out_ids[lo + m] = self.id[s][j]
            te = (t - self.t_last[s][j])[:, None, None]
            a_d = (TWO_PI * dc) * te
            a_d = a_d / (a_d + 1.0)
            dxh = a_d * ((kp[m] - self.xhat[s][j]) / te) + (1.0 - a_d) * self.dxhat[s][j]
            a = (TWO_PI * (mc + beta * np.abs(dxh))) * te
            a = a / (a + 1.0)
            xh = a * kp[m] + (1.0 - a) * self.xhat[s][j]
            self.xhat[s][j], self.dxhat[s][j] = xh, dxh
            out_kp[lo + m] = xh
            self.age[s][j], self.t_last[s][j], self.area[s][j], self.kp[s][j] = 0, t, ar[m], kp[m]
            for i in order[slot[order] < 0]:
                empty = np.flatnonzero(self.id[s] < 0)
                if not empty.size:
                    self.overflow[s] += 1
                    continue
                j = int(empty[0])
                self.id[s, j], self.next_id[s] = self.next_id[s], self.next_id[s] + 1
                self.age[s, j], self.t_last[s, j], self.area[s, j] = 0, t, ar[i]
                self.kp[s, j], self.xhat[s, j], self.dxhat[s, j] = kp[i], kp[i], 0.0
                out_ids[lo + i] = self.id[s, j]
        return out_ids, out_kp


def launch_arguments(tracker, *inputs):
    """One update of ``tracker``: what it hands to its three launches."""
    launch, seen = tracker._launch, []

    def spy(*args):
        seen.append(args)
        return launch(*args)

    tracker._launch = spy
    try:
        tracker.update(*inputs[1:], stream_ids=inputs[0])
    finally:
        del tracker._launch
    return seen[0]


def box_launch_arguments(tracker):
    """One propose_boxes of ``tracker``: what it hands to its launch."""
    launch, seen = tracker._launch_boxes, []

    def spy(*args):
        seen.append(args)
        return launch(*args)

    tracker._launch_boxes = spy
    try:
        tracker.propose_boxes()
    finally:
        del tracker._launch_boxes
    return seen[0]


def assign_launchers(tracker, frame):
    """One update of ``tracker`` on ``frame``; before its launches touch the state, pp_track_oks fills a workspace of
    this call's own.  Returns (greedy, optimal): pp_track_assign and pp_track_assign_optimal alone on that workspace
    and on the tracker's state (with their output allocations).  Everybody is matched, so a replay leaves the state's
    ids, and with them what the next replay does, as they are."""
    from probpose_pytorch_amd import _lib
    launch, made = tracker._launch, {}

    def spy(n_str, off, off_dev, det_stream, blocks, kp_s, vis_s, ar_s, sc_s, variances, t_now, t_prev):
        T, M = tracker.max_tracks, int(off[-1])
        ws = torch.empty(M * T, dtype=torch.float64, device=kp_s.device)
        _lib.launch("pp_track_oks", n_str, K, T, M, off, det_stream, blocks, kp_s, None, ar_s, variances, 0.0, ws)

        def run(entry, *tail):
            new = lambda dtype: torch.empty(M, dtype=dtype, device=ws.device)
            _lib.launch(entry, n_str, K, T, M, off, off_dev, blocks, ws, ar_s, MATCH_THR, MAX_AGE, t_now, t_prev,
                        new(torch.int64), new(torch.float64), new(torch.uint8), new(torch.int32), new(torch.float64),
                        *tail)
        made["greedy"] = lambda: run("pp_track_assign")
        made["optimal"] = lambda: run("pp_track_assign_optimal", None)
        return launch(n_str, off, off_dev, det_stream, blocks, kp_s, vis_s, ar_s, sc_s, variances, t_now, t_prev)

    tracker._launch = spy
    try:
        tracker.update(*frame[1:], stream_ids=frame[0])
    finally:
        del tracker._launch
    return made["greedy"], made["optimal"]


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
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--people", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--window-ms", type=float, default=1000.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--assign", choices=["greedy", "optimal"], default="greedy",
                    help="optimal: also time pp_track_assign_optimal beside pp_track_assign and the update in both modes")
    ap.add_argument("--stage", action="store_true",
                    help="also time the update with predict, with high_thr / birth_thr and with both, greedy and optimal")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "track_bench needs the GPU: there is nothing to time without it"
    from probpose_pytorch_amd import OneEuro, PoseTracker

    def walker(frames):
        """The frames forwards, then backwards, for ever."""
        state = dict(n=0)

        def nxt():
            n, F = state["n"], len(frames)
            state["n"] = n + 1
            n %= 2 * F - 2
            return frames[n if n < F else 2 * F - 2 - n]
        return nxt

    new = lambda assign="greedy", **kw: PoseTracker(SIGMAS, match_thr=MATCH_THR, max_age=MAX_AGE, max_tracks=MAX_TRACKS,
                                                    smooth=OneEuro(), fps=FPS, assign=assign, **kw)
    variants, sizes = {}, {}
    for P in args.people:
        frames = make_video(args.streams, P, args.frames, args.seed + P)
        dev, host = new(), HostTracker(args.streams)
        agree, matched, dev_ids = True, 0, []
        for f in frames[:5]:                            # the host variant against the device, before anything is timed
            res = dev.update(*f[1:], stream_ids=f[0])
            dev_ids.append(res.ids)
            got = host.update(*f)[0]
            agree = agree and bool(np.array_equal(res.ids.cpu().numpy(), got))
            matched = int((~res.born).sum())
        sizes[str(P)] = dict(detections=args.streams * P, ids_agree=agree, matched_in_frame_5=matched,
                             overflow=int(dev.overflow.sum()))
        step_dev, step_host = walker(frames[5:]), walker(frames[5:])
        variants[f"{P}/update"] = lambda dev=dev, nxt=step_dev: (lambda f: dev.update(*f[1:], stream_ids=f[0]))(nxt())
        variants[f"{P}/host_numpy"] = lambda host=host, nxt=step_host: host.update(*nxt())
        alone = new()
        a = list(launch_arguments(alone, *frames[0]))
        clock = dict(t=float(a[-2]))

        def launches(alone=alone, a=a, clock=clock):
            a[-1], a[-2] = clock["t"], clock["t"] + 1.0 / FPS
            clock["t"] = a[-2]
            return alone._launch(*a)
        variants[f"{P}/launches"] = launches
        variants[f"{P}/propose"] = dev.propose_boxes
        box_args = box_launch_arguments(alone)
        variants[f"{P}/propose_launch"] = lambda alone=alone, a=box_args: alone._launch_boxes(*a)
        for mode in ("greedy", "optimal") if args.stage else ():
            for label, kw in STAGE_VARIANTS.items():
                tr = new(mode, **kw)
                for f in frames[:5]:
                    tr.update(*f[1:], stream_ids=f[0])
                step = walker(frames[5:])
                variants[f"{P}/update_{label}_{mode}"] = lambda tr=tr, nxt=step: (
                    lambda f: tr.update(*f[1:], stream_ids=f[0]))(nxt())
        if args.assign == "optimal" or args.stage:
            opt, same = new("optimal"), True
            for f in frames[:5]:
                same = same and bool(torch.equal(opt.update(*f[1:], stream_ids=f[0]).ids,
                                                 dev_ids.pop(0)))
            sizes[str(P)]["optimal_ids_are_greedy_ids"] = same
            step_opt = walker(frames[5:])
            variants[f"{P}/update_optimal"] = lambda opt=opt, nxt=step_opt: (
                lambda f: opt.update(*f[1:], stream_ids=f[0]))(nxt())
        if args.assign == "optimal":
            pair = new()
            pair.update(*frames[0][1:], stream_ids=frames[0][0])
            variants[f"{P}/assign_greedy"], variants[f"{P}/assign_optimal"] = assign_launchers(pair, frames[1])

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
    out = dict(streams=args.streams, K=K, frames=args.frames, max_tracks=MAX_TRACKS, window_ms=args.window_ms,
               repeats=args.repeats, warmup=args.warmup, sizes=sizes, steps=steps)
    for name, ts in times.items():
        out[name] = spread(ts)
    if args.assign == "optimal":                        # optimal / greedy, of the medians
        ratio = lambda a, b: round(out[a]["ms_median"] / max(out[b]["ms_median"], 1e-6), 2)
        out["optimal_over_greedy"] = {str(P): dict(assign=ratio(f"{P}/assign_optimal", f"{P}/assign_greedy"),
                                                   update=ratio(f"{P}/update_optimal", f"{P}/update"))
                                      for P in args.people}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
