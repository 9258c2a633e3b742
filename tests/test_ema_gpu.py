"""ModelEma and ema_update_ on the GPU against the float64 gauge of tests/ema_reference.py.

Bounds (derived there, u = 2^-24, M = max(|s_0|, max |p|) per tensor):
    one update from identical float32 inputs:   |got - gauge| <= u |gauge| + 2^-50 (|s| + |p|)
    T chained updates, never resynchronised:    |got - gauge| <= T u M (1 + 2^-20)
Copied (non-float) entries are equal bit for bit.  torch's float32 _foreach_lerp_ is held to 3 T u M for w < 0.5.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ema_reference as ER

pytestmark = pytest.mark.gpu

CHUNK = 8192
SIZES = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7)
OFFSET_SIZES = (5, CHUNK + 1, 2 * CHUNK + 7)      # also placed 4 bytes off a 16-byte boundary: src, dst, both
T = 20
GUARD = 4                                          # sentinel elements on either side of every destination
SENTINEL = -12345.0


@functools.lru_cache(maxsize=None)
def _case():
    """(specs, start, rows): per entry (dtype, n, src one element off, dst one element off); the float32 / int64 start
    of the average and T model states.  Read-only: shared by the tests."""
    specs = [(np.float32, n, False, False) for n in SIZES]
    for n in OFFSET_SIZES:
        specs += [(np.float32, n, True, False), (np.float32, n, False, True), (np.float32, n, True, True)]
    specs += [(np.float32, 0, False, False), (np.int64, 1, False, False), (np.int64, 3, False, False),
              (np.int64, 3, True, True)]
    rng = np.random.default_rng(41)

    def draw(dtype, n):
        if dtype == np.float32:
            return (rng.standard_normal(n) * 0.05).astype(np.float32)
        return rng.integers(-2 ** 62, 2 ** 62, n, dtype=np.int64)

    start = [draw(d, n) for d, n, _, _ in specs]
    rows = [[draw(d, n) for d, n, _, _ in specs] for _ in range(T)]
    for a in start + [a for row in rows for a in row]:
        a.setflags(write=False)
    return specs, start, rows


def _place(a, off, guard_value):
    """`a` on the device inside a larger buffer: 16-byte aligned, or one ELEMENT past that when `off` (4 bytes for
    float32, 8 for int64: neither is 16-byte aligned).  Returns (view, buffer)."""
    lead = GUARD + (1 if off else 0)
    buf = torch.full((lead + a.size + GUARD,), guard_value, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    view = buf[lead:lead + a.size]
    view.copy_(torch.from_numpy(a.copy()))
    assert buf.data_ptr() % 16 == 0 and view.is_contiguous()
    if a.size:
        assert (view.data_ptr() % 16 != 0) == bool(off)
    return view, buf


def _tensors(specs, start, row):
    dsts, dbufs, srcs = [], [], []
    for (dtype, n, soff, doff), s, p in zip(specs, start, row):
        guard = SENTINEL if dtype == np.float32 else -777
        d, db = _place(s, doff, guard)
        sv, _ = _place(p, soff, guard)
        dsts.append(d)
        dbufs.append(db)
        srcs.append(sv)
    return dsts, dbufs, srcs


def _guards_intact(specs, dbufs):
    for (dtype, n, _, doff), b in zip(specs, dbufs):
        lead = GUARD + (1 if doff else 0)
        guard = SENTINEL if dtype == np.float32 else -777
        assert bool((b[:lead] == guard).all()) and bool((b[lead + n:] == guard).all()), (dtype, n, doff)


def _run_chain(weight, check=True):
    """T chained updates with a new model state before each; returns the final bytes and the worst ratios."""
    from probpose_pytorch_amd import ema_update_
    specs, start, rows = _case()
    dsts, dbufs, srcs = _tensors(specs, start, rows[0])
    gauge = ER.Gauge(start, decay=1.0 - weight)
    worst_one = worst_chain = 0.0
    for t, row in enumerate(rows):
        for sv, p in zip(srcs, row):
            sv.copy_(torch.from_numpy(p.copy()))            # in place: the addresses, and so the table, stay
        before = [d.cpu().numpy() for d in dsts]
        versions = [d._version for d in dsts]
        ema_update_(dsts, srcs, weight)
        got = [d.cpu().numpy() for d in dsts]
        gauge.step(row, weight=weight)
        if not check:
            continue
        one = ER.update(before, row, weight)
        for i, ((dtype, n, _, _), g, s, p) in enumerate(zip(specs, got, before, row)):
            assert (dsts[i]._version > versions[i]) == (n > 0), (i, n)
            assert srcs[i].cpu().numpy().tobytes() == p.tobytes(), ("source changed", i)
            if n == 0:
                continue
            if dtype != np.float32:
                assert g.tobytes() == p.tobytes(), ("copy", i, t)
                continue
            r1 = float((np.abs(g.astype(np.float64) - one[i]) / ER.bound_one(one[i], s, p)).max())
            worst_one = max(worst_one, r1)
            assert r1 <= 1.0, ("one update", i, n, t, r1)
        rc = gauge.ratio(got)
        worst_chain = max(worst_chain, rc)
        assert rc <= 1.0, ("chained", t, rc)
    _guards_intact(specs, dbufs)
    return b"".join(d.cpu().numpy().tobytes() for d in dsts), worst_one, worst_chain


@pytest.mark.parametrize("weight", [1e-4, 0.5, 1.0])
def test_primitive_against_the_gauge(weight):
    """20 chained updates over every size around the 128-bit group and the chunk, three alignments, a zero-element
    tensor and int64 entries: every update within both bounds, copies and sources bit-exact, versions advanced,
    nothing written outside the destinations."""
    _, one, chain = _run_chain(weight)
    print(f"weight {weight}: worst d / bound, one update {one:.4f}, {T} chained {chain:.4f}")
    assert one <= 1.0 and chain <= 1.0


def test_same_bits_on_a_repeated_run():
    a = _run_chain(0.25, check=False)[0]
    b = _run_chain(0.25, check=False)[0]
    assert a == b and len(a) > 4 * sum(SIZES)


@pytest.mark.parametrize("weight", [1e-4, 0.25])
def test_agreement_with_torch_on_the_device(weight):
    """torch's float32 _foreach_lerp_ rounds three times per update (3 T u M for w < 0.5); the kernel is held to its
    own bound, a third of that."""
    from probpose_pytorch_amd import ema_update_
    specs, start, rows = _case()
    fl = [i for i, (d, n, _, _) in enumerate(specs) if d == np.float32 and n > 0]
    ours = [torch.from_numpy(start[i].copy()).cuda() for i in fl]
    theirs = [torch.from_numpy(start[i].copy()).cuda() for i in fl]
    srcs = [torch.empty_like(t) for t in ours]
    gauge = ER.Gauge([start[i] for i in fl], decay=1.0 - weight)
    for row in rows:
        for sv, i in zip(srcs, fl):
            sv.copy_(torch.from_numpy(row[i].copy()))
        ema_update_(ours, srcs, weight)
        torch._foreach_lerp_(theirs, srcs, weight)
        gauge.step([row[i] for i in fl], weight=weight)
    rk = gauge.ratio([t.cpu().numpy() for t in ours])
    rt = gauge.ratio([t.cpu().numpy() for t in theirs], c=3.0)
    print(f"weight {weight}, {T} updates: kernel d / (T u M) = {rk:.4f}, torch _foreach_lerp_ d / (3 T u M) = {rt:.4f}")
    assert rk <= 1.0 and rt <= 1.0


def test_table_without_the_magic_word_is_left_alone():
    """The C ABI directly: the same table once with its first word cleared (every workgroup returns at the entry
    check) and once intact."""
    from probpose_pytorch_amd import _lib
    L = _lib.lib()
    n = CHUNK + 5
    src, dst = torch.ones(n, device="cuda"), torch.zeros(n, device="cuda")
    ptrs = np.array([src.data_ptr(), dst.data_ptr()], dtype=np.uint64)
    counts, kinds = np.array([n], dtype=np.int64), np.array([0], dtype=np.int32)
    nbytes = L.pp_ema_table_bytes(1, counts.ctypes.data)
    host = np.zeros(nbytes // 8, dtype=np.uint64)
    nc = C.c_int(0)
    _lib.check(L.pp_ema_table_build(1, ptrs[0:].ctypes.data, ptrs[1:].ctypes.data, counts.ctypes.data,
                                    kinds.ctypes.data, host.ctypes.data, C.byref(nc)), "pp_ema_table_build")
    assert nc.value == 2
    broken = host.copy()
    broken.view(np.uint32)[0] = 0
    for table_host, want in ((broken, 0.0), (host, 0.5)):
        table = torch.from_numpy(table_host.view(np.uint8).copy()).cuda()
        _lib.check(L.pp_ema_update(_lib.ptr(table), nc.value, 0.5, _lib.stream_ptr()), "pp_ema_update")
        torch.cuda.synchronize()
        assert bool((dst == want).all()) and bool((src == 1.0).all())


def _training_setup():
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.loss import ProbPoseLoss
    from probpose_pytorch_amd.model import ProbPoseModel
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_head_state, synthetic_vit_state
    from tests import loss_reference as LR
    B, K, Cd, heads, depth, size = 2, 20, 384, 12, 2, (384, 384)
    H = W = 96
    pools = [(4, 4), (2, 2), (2, 2)]
    rng = np.random.default_rng(11)
    kps = rng.uniform(20, 364, (B, K, 2)).astype(np.float32)
    annotated = rng.random((B, K)) > 0.2
    vis = (rng.random((B, K)) > 0.3).astype(np.float32)
    gt_hm, in_image = LR.encode_probmaps(kps, annotated.astype(np.float32), size, (W, H))
    gt_np = dict(heatmaps=gt_hm, in_image=in_image[:, None, :], keypoints_visible=annotated[:, None, :],
                 keypoints_visibility=vis[:, None, :])
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in gt_np.items()}
    loss_fn = ProbPoseLoss(Codec(ArgMaxProbMap(size, (W, H), np.full(K, 0.05))), freeze_error=True,
                           differentiable=True)
    backbone = ScratchViTBackbone(size, 16, embed_dim=Cd, depth=depth, num_heads=heads, differentiable=True)
    backbone.model.load_state_dict(synthetic_vit_state(size, 16, Cd, depth, seed=12))
    head = ProbMapHead(Cd, K, pools, (256, 256), (4, 4), final_layer_kernel_size=1, freeze_error=True,
                       normalize=1.0, differentiable=True)
    head.load_state_dict(synthetic_head_state(Cd, K, n_pools=3, deconv_out=(256, 256), seed=13), strict=False)
    model = ProbPoseModel(backbone, head).cuda().train()
    return model, loss_fn, gt, synthetic_crops(B, *size, seed=14).cuda()


def _host_state(module):
    return {k: v.detach().cpu().numpy().copy() for k, v in module.state_dict().items()}


def test_model_ema_in_the_training_loop():
    """The depth-2 model of tests/test_model_train_gpu.py, six steps of FusedAdamW with ModelEma(decay=0.99, tau=3)."""
    from probpose_pytorch_amd import FusedAdamW, ModelEma
    from tests import loss_grad_reference as LG
    model, loss_fn, gt, xc = _training_setup()
    ema = ModelEma(model, decay=0.99, tau=3)
    resumed = ModelEma(model, decay=0.5)              # takes the state saved after step 3
    assert not ema.module.training and model.training
    keys = list(model.state_dict())
    start = _host_state(ema.module)
    kinds = {str(a.dtype) for a in start.values()}
    assert kinds == {"float32", "int64"}, kinds       # BN's num_batches_tracked is among the entries
    gauge = ER.Gauge([start[k] for k in keys], decay=0.99, tau=3)
    opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=3e-4, max_grad_norm=1.0)
    worst, out_before = 0.0, None
    for step in range(6):
        opt.zero_grad()
        losses = loss_fn(gt, model(xc))
        loss = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
        loss.backward()
        opt.step()
        if step == 5:       # the eval plan of the average is built from the state before the last update
            with torch.no_grad():
                out_before = [o.clone() for o in ema.module(xc)]
        fed = _host_state(model)
        versions = [v._version for v in ema.module.state_dict(keep_vars=True).values()]
        if step >= 4:       # warmed up: the table is uploaded, the code object loaded
            torch.cuda.synchronize()
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                ema.update(model)
            finally:
                torch.cuda.set_sync_debug_mode(mode)
        else:
            ema.update(model)
        if step >= 3:
            resumed.update(model)
        assert ema.updates == step + 1
        after = _host_state(model)
        for k in keys:
            assert after[k].tobytes() == fed[k].tobytes(), ("the model changed under update", k)
        w = gauge.step([fed[k] for k in keys])
        assert w == 1.0 - ema.decay_at(step + 1) and 0.0 < w < 1.0
        got = _host_state(ema.module)
        for i, k in enumerate(keys):
            if not gauge.averaged[i]:
                assert got[k].tobytes() == fed[k].tobytes(), ("copied entry", k)
        r = gauge.ratio([got[k] for k in keys])
        worst = max(worst, r)
        assert r <= 1.0, (step, r)
        assert all(v._version > v0 for v, v0 in zip(ema.module.state_dict(keep_vars=True).values(), versions))
        if step == 2:
            saved = copy.deepcopy(ema.state_dict())
            resumed.load_state_dict(saved)
            assert resumed.updates == 3 and resumed.decay == 0.99 and resumed.tau == 3.0
    print(f"model level, 6 updates, {len(keys)} entries: worst d / bound = {worst:.4f}")
    counters = [k for k in keys if k.endswith("num_batches_tracked")]
    assert counters and all(int(got[k]) == int(fed[k]) >= 6 for k in counters)
    # a resumed average continues the same sequence
    for k, v in _host_state(resumed.module).items():
        assert v.tobytes() == got[k].tobytes(), ("resumed", k)
    # the eval path of the average serves the NEW weights: same bits as a fresh copy loaded from its state_dict
    with torch.no_grad():
        out = ema.module(xc)
        fresh = copy.deepcopy(ema.module)
        fresh.load_state_dict(ema.module.state_dict())
        out_fresh = fresh(xc)
    assert len(out) == len(out_fresh) == len(out_before)
    for a, b in zip(out, out_fresh):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(out, out_before))
    assert all(not p.requires_grad for p in ema.module.parameters())
