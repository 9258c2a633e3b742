"""Captured graphs keep replaying through valid memory whatever the caches go through afterwards, and the pinned
staging pool is reused (_buffers.CaptureCache / PinnedStaging behind heatmap, ema and optim)."""
import gc
import weakref

import numpy as np
import pytest
import torch

from oracle import probpose_oracle as orc
from tests import ema_reference as ER
from tests import optim_reference as OR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp(built_lib):
    import probpose_pytorch_amd as p
    assert torch.cuda.is_available()
    return p


def _nan_scratch(sizes, copies=4):
    """Float32 tensors of these element counts, filled with NaN: whatever was freed at those sizes is handed out again
    and visibly overwritten."""
    return [torch.full((max(int(n), 1),), float("nan"), device="cuda") for n in sizes for _ in range(copies)]


def test_decode_replay_survives_the_churn_of_both_decode_caches(pp):
    """A graph holding one wave-path decode (B = 1, K = 17, 64x48), then decodes on 17 fresh streams (more than the 16
    unmarked hand-over lists the cache keeps), 65 decodes with distinct sigmas (more than its 64 tap tables) and NaN
    fills of everything those sizes would free: the replay still gives the bits of an eager decode, and the hand-over
    list and the tap tables the graph reads are still held."""
    from probpose_pytorch_amd import _lib, heatmap
    hm = torch.from_numpy(orc.synthetic_heatmaps(1, 17, 64, 48, seed=31)).cuda()
    sig = np.linspace(0.025, 0.107, 17)
    tiny = torch.from_numpy(orc.synthetic_heatmaps(1, 1, 8, 8, seed=32)).cuda()
    saved = heatmap.DECODE_FLAGS
    heatmap.DECODE_FLAGS = _lib.DECODE_WAVE
    try:
        want = heatmap.decode_on_device(hm, sig)
        want = {k: want[k].clone() for k in ("locs", "scores")}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            heatmap.decode_on_device(hm, sig)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out_g = heatmap.decode_on_device(hm, sig)
        ws_keys = [k for k in heatmap._DECODE_WS if heatmap._DECODE_WS.marked(k)]
        tap_keys = [k for k in heatmap._TAP_CACHE if heatmap._TAP_CACHE.marked(k)]
        assert len(ws_keys) >= 1 and len(tap_keys) >= 1
        ws_bytes = heatmap._DECODE_WS.peek(ws_keys[0]).numel()
        held = [weakref.ref(heatmap._DECODE_WS.peek(k)) for k in ws_keys]
        held += [weakref.ref(t) for k in tap_keys for t in heatmap._TAP_CACHE.peek(k)]
        # churn
        streams = [torch.cuda.Stream() for _ in range(17)]
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                heatmap.decode_on_device(hm, sig)
            torch.cuda.current_stream().wait_stream(s)
        for i in range(65):
            heatmap.decode_on_device(tiny, np.array([0.02 + 0.001 * i]))
        torch.cuda.synchronize()
        junk = _nan_scratch([ws_bytes // 4, 17 * _lib.PP_MAX_TAPS * 2, 17, _lib.PP_MAX_TAPS * 2, 1])
        torch.cuda.synchronize()
        del junk
        for t in out_g.values():
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g["locs"], want["locs"]) and torch.equal(out_g["scores"], want["scores"])
        gc.collect()
        assert all(r() is not None for r in held)
        assert sum(1 for k in heatmap._DECODE_WS if not heatmap._DECODE_WS.marked(k)) <= 16
        assert sum(1 for k in heatmap._TAP_CACHE if not heatmap._TAP_CACHE.marked(k)) <= 64
    finally:
        heatmap.DECODE_FLAGS = saved


def test_ema_replay_survives_seventeen_other_plans(pp):
    """A captured ema_update_ of one float32 pair (5 elements) and one int64 pair (1 element), then 17 other plans
    (the cache keeps 16 unmarked ones) and NaN fills of the table's size: two replays give the bits of two updates of
    the float64 gauge.  With weight 0.5 and values in [1, 2) every float64 operation of d + w (s - d) is exact, so the
    single rounding to float32 decides the bits and they can be compared exactly."""
    from probpose_pytorch_amd import ema, ema_update_
    rng = np.random.default_rng(41)
    start = [(1.0 + rng.random(5)).astype(np.float32), np.array([3], dtype=np.int64)]
    model = [(1.0 + rng.random(5)).astype(np.float32), np.array([11], dtype=np.int64)]
    dsts = [torch.from_numpy(a.copy()).cuda() for a in start]
    srcs = [torch.from_numpy(a.copy()).cuda() for a in model]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ema_update_(dsts, srcs, 0.5)                           # builds and uploads the plan
        for d, a in zip(dsts, start):
            d.copy_(torch.from_numpy(a.copy()))                # in place: the addresses, and so the plan, stay
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ema_update_(dsts, srcs, 0.5)
    marked = [k for k in ema._plans if ema._plans.marked(k)]
    assert len(marked) >= 1
    table_bytes = ema._plans.peek(marked[0]).table.numel()
    others = []
    for i in range(17):
        d, s = torch.full((i + 2,), 1.0, device="cuda"), torch.full((i + 2,), 2.0, device="cuda")
        ema_update_([d], [s], 0.5)
        others.append((d, s))
    torch.cuda.synchronize()
    assert sum(1 for k in ema._plans if not ema._plans.marked(k)) <= 16
    junk = _nan_scratch([table_bytes // 4], copies=8)
    torch.cuda.synchronize()
    del junk
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    want = start
    for _ in range(2):
        want = [w.astype(a.dtype) for w, a in zip(ER.update(want, model, 0.5), start)]
    for d, w in zip(dsts, want):
        assert d.cpu().numpy().tobytes() == w.tobytes()
    assert all(ema._plans.peek(k) is not None for k in marked)


def test_fused_adamw_reuses_its_staging_buffers(pp):
    """Three steps on two 20-element parameters: within the bound of the float64 gauge (tests/optim_reference.py, the
    kernel's constants), and the pinned pool holds at most two buffers once the device is idle: a step whose
    predecessors have completed takes one of theirs.  The gauge's bound is how the suite states what FusedAdamW
    computes (tests/test_optim_gpu.py); a float32 kernel has no bit-identical float64 counterpart to compare with."""
    params, grads = OR.synthetic_case([(20,), (20,)], 3, seed=51)
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in params]
    opt = pp.FusedAdamW(ps, lr=1e-3, max_grad_norm=1.0)
    gauge = OR.Gauge(params, [0, 0])
    for t, row in enumerate(grads):
        for p, gr in zip(ps, row):
            p.grad = torch.from_numpy(gr).cuda()
        if t == 2:
            torch.cuda.synchronize()                           # the first two steps' copies have completed
        opt.step()
        gauge.step(row, OR.hyper_of(opt), max_norm=1.0)
    torch.cuda.synchronize()
    assert 1 <= len(opt._staging) <= 2
    got = ([p.detach().cpu().numpy() for p in ps], [opt.state[p]["exp_avg"].cpu().numpy() for p in ps],
           [opt.state[p]["exp_avg_sq"].cpu().numpy() for p in ps])
    r = OR.ratios(gauge, *got)
    print("d / bound after 3 steps:", r)
    assert r["p"] <= 1.0 and r["m"] <= 1.0 and r["v"] <= 1.0, r
