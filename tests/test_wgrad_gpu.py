"""pp_wgrad_gemm (csrc/pp_head_grad.hip) called through ops.wgrad, against its float64 restatement
(tests/wgrad_reference.py, pinned on the CPU by tests/test_wgrad_reference.py).

Every launch writes dW and dB inside NaN-bit-filled buffers with guard elements on both sides, and ``parts`` is exactly
pp_wgrad_workspace_floats long between guards: every element outside what the call writes must keep its bits.

a. Exact cases.  Integer inputs |dY|, |A| <= 4 are exact in bf16 and every partial sum stays below 2^24 (at most
   40000 rows x 16), so any summation order gives the same f32 value: dW and dB must equal the float64 result.  An
   indexing error of any size fails.
b. Rounding cases.  The same shapes with seeded normal inputs, element-wise: |got - want| <= n u S[n, k], u = 2^-24,
   S[n, k] = sum_m |dY(m, n) A(m, k)| (dB: Sb[n] = sum_m |dY(m, n)|).  n counts the f32 roundings on one element's path
   through the kernel (wgrad_reference.roundings): the MFMA accumulator takes one addition per row of the element's
   split, rows = min(M, ceil(ceil(M / split) / 32) 32); wgrad_reduce_kernel adds the split partials in order, split - 1
   roundings (the first addition, to 0, is exact); an f32 product rounds once more, a bf16 x bf16 product is exact in
   f32.  dB: one addition per row of the slab loop, then the same reduction.
c. Recorded calls.  One training step of train.py's head at batch 32 (bf16), of the ViT-B bench head at batch 64 (bf16
   and fp32) and of two backbones (bf16), with ops.wgrad wrapped: one call per distinct argument set is kept with
   copies of what its pointers reach, and replayed under bound b.  The float64 product of these runs on the device
   (torch float64 matmul over rows gathered by the restatement's index code, independent of the kernel under test);
   one small case asserts that the device path and the CPU restatement agree.
d. Two launches of a split case give equal bits.
e. Refusals return a HipExtensionError and write nothing.
"""
import ctypes as C
import time

import pytest
import torch

from probpose_pytorch_amd import head_calls, pack
from tests import wgrad_reference as WR

pytestmark = pytest.mark.gpu

GUARD = 64                                   # f32 guard elements on either side (256 bytes: alignment unchanged)
DTYPES = [torch.float32, torch.bfloat16]
_WORST: dict = {}


@pytest.fixture
def ops(built_lib):
    assert torch.cuda.is_available()
    from probpose_pytorch_amd import ops as o
    return o


def _tag(dt):
    return str(dt).replace("torch.", "")


def _note(cls, r):
    _WORST[cls] = max(_WORST.get(cls, 0.0), r)


def _place(vals: torch.Tensor, off_bytes: int) -> torch.Tensor:
    """vals on the GPU as a 1-D tensor whose address is off_bytes past a 16-byte boundary."""
    es = vals.element_size()
    assert off_bytes % es == 0 and off_bytes < 16
    lead = off_bytes // es
    buf = torch.zeros(lead + vals.numel() + 16, dtype=vals.dtype, device="cuda")
    buf[lead:lead + vals.numel()] = vals.reshape(-1).cuda()
    t = buf[lead:lead + vals.numel()]
    assert t.data_ptr() % 16 == off_bytes
    return t


def _guarded(span: int, off_bytes: int = 0):
    """(whole buffer, lead): NaN-bit f32 elements, span of them from element lead on, GUARD before and after."""
    assert off_bytes % 4 == 0
    lead = GUARD + off_bytes // 4
    buf = WR.nan_like_bits(lead + span + GUARD, torch.float32, "cuda")
    assert buf[lead:].data_ptr() % 16 == off_bytes
    return buf, lead


# ---------------------------------------------------------------------------------------------------------------
# the case set of sections a and b
# ---------------------------------------------------------------------------------------------------------------
EDGES = (1, 63, 64, 65, 129)
ROWS = (1, 31, 32, 33, 511, 512, 513, 1025)


def _cases():
    cs = {}
    for N in EDGES:
        for Kd in EDGES:
            cs[f"tile N{N} K{Kd}"] = dict(M=33, N=N, Kd=Kd)
    for M in ROWS:
        cs[f"rows M{M} ragged"] = dict(M=M, N=65, Kd=63)
        cs[f"rows M{M} whole"] = dict(M=M, N=64, Kd=128)
    cs["split 64, last split empty"] = dict(M=40000, N=64, Kd=48)
    cs["split 64 ragged tile"] = dict(M=40000, N=5, Kd=63)
    # gathered: 8-column loads that straddle a segment, rowoff off the 8-element grid, -1 over whole and part groups
    cs["gather seg 12"] = dict(M=100, N=40, Kd=60, gather=dict(seg=12, rs=16, cols=1, pad=0.2))
    cs["gather seg 20"] = dict(M=100, N=40, Kd=100, gather=dict(seg=20, rs=24, cols=1, pad=0.2))
    cs["gather seg 12 split"] = dict(M=1030, N=40, Kd=60, gather=dict(seg=12, rs=16, cols=1, pad=0.4))
    cs["gather seg 16 rowoff unaligned"] = dict(M=100, N=17, Kd=64, gather=dict(seg=16, rs=19, cols=4, pad=0.1))
    cs["gather seg 8 whole groups of -1"] = dict(M=100, N=17, Kd=72, gather=dict(seg=8, rs=8, cols=1, pad=0.4))
    cs["gather seg 64 aligned"] = dict(M=600, N=64, Kd=192, gather=dict(seg=64, rs=64, cols=1, pad=0.15))
    cs["gather seg 1"] = dict(M=50, N=9, Kd=11, gather=dict(seg=1, rs=3, cols=3, pad=0.2))
    # bases off 16-byte alignment, pitches off the 8-element grid
    for off in ((4, 4, 4), (8, 8, 8), (0, 8, 4), (8, 0, 0)):
        cs[f"offsets {off}"] = dict(M=70, N=40, Kd=72, ldd=43, lda=77, off=off)
        cs[f"offsets {off} whole pitches"] = dict(M=70, N=40, Kd=72, ldd=48, lda=80, off=off)
    cs["offsets (2, 2, 4)"] = dict(M=70, N=40, Kd=72, ldd=43, lda=77, off=(2, 2, 4), only=torch.bfloat16)
    cs["offsets (2, 0, 0) whole pitches"] = dict(M=70, N=40, Kd=72, ldd=48, lda=80, off=(2, 0, 0), only=torch.bfloat16)
    cs["offsets (4, 8, 8) gathered"] = dict(M=70, N=40, Kd=64, ldd=43, off=(4, 8, 8),
                                            gather=dict(seg=16, rs=16, cols=1, pad=0.2))
    cs["lddw > Kd"] = dict(M=33, N=65, Kd=63, lddw=68)
    cs["lddw > Kd split"] = dict(M=600, N=65, Kd=63, lddw=70)
    for batch in (2, 4):
        g = dict(seg=12, rs=15, cols=4, pad=0.2)
        cs[f"batch {batch} every stride"] = dict(M=40, N=20, Kd=36, batch=batch, gather=g, rowmap="perm", ldd=21,
                                                 lddw=37)
        cs[f"batch {batch} every stride split"] = dict(M=1100, N=20, Kd=36, batch=batch, gather=g, rowmap="perm",
                                                       ldd=21, lddw=37)
    cs["no dB"] = dict(M=33, N=65, Kd=63, dB=False)
    cs["no dB split"] = dict(M=600, N=65, Kd=63, dB=False)
    cs["rowmap permutation"] = dict(M=70, N=33, Kd=40, rowmap="perm")
    cs["rowmap permutation split"] = dict(M=600, N=33, Kd=40, rowmap="perm")
    cs["rowmap repeats"] = dict(M=70, N=33, Kd=40, rowmap="repeat")
    cs["rowmap repeats split"] = dict(M=1100, N=64, Kd=64, rowmap="repeat")
    cs["aux batched"] = dict(aux=(2, 5, 4, 24, 4))
    cs["aux batched split"] = dict(aux=(30, 5, 4, 24, 3))
    return cs


CASES = _cases()
PARAMS = [pytest.param(n, dt, id=f"{n}-{_tag(dt)}") for n, s in CASES.items() for dt in DTYPES
          if s.get("only", dt) == dt]


def _shape(spec):
    if "aux" in spec:
        B, h, w, Cc, batch = spec["aux"]
        return B * h * w, Cc, 9 * Cc, batch
    return spec["M"], spec["N"], spec["Kd"], spec.get("batch", 1)


def _build(spec, dt, ints, seed):
    """The keyword arguments of one ops.wgrad call (dY, A and the tables on the GPU, without dW / dB / parts)."""
    gen = torch.Generator().manual_seed(seed)
    draw = (lambda n: torch.randint(-4, 5, (n,), generator=gen).float().to(dt)) if ints else \
        (lambda n: torch.randn((n,), generator=gen).to(dt))
    M, N, Kd, batch = _shape(spec)
    if "aux" in spec:           # head_train.py's later aux stages: column blocks of [M, 4C] rows, one table for all
        B, h, w, Cc, _ = spec["aux"]
        ro = pack.conv_gather_table(B, h, w, 3, 3, 1, 1, 4 * Cc)
        return dict(head_calls.wgrad_of(head_calls.aux_stage(M, Cc, batch)), dY=_place(draw(M * 4 * Cc), 0),
                    A=_place(draw(M * 4 * Cc), 0), rowoff=ro.reshape(-1).cuda()), True
    off = spec.get("off", (0, 0, 0))
    ldd = spec.get("ldd", N)
    many = batch > 1
    kw = dict(M=M, N=N, Kd=Kd, ldd=ldd, batch=batch)
    rowmap = spec.get("rowmap")
    RY = M if rowmap is None else (M + 7 if rowmap == "perm" else M // 3 + 1)
    if many:
        kw["strideDY"] = RY * ldd + 3
    kw["dY"] = _place(draw((batch - 1) * kw.get("strideDY", 0) + RY * ldd), off[0])
    if rowmap is not None:
        rm = [torch.randperm(RY, generator=gen)[:M] if rowmap == "perm" else torch.randint(0, RY, (M,), generator=gen)
              for _ in range(batch)]
        kw["dy_rowmap"] = torch.stack(rm).to(torch.int32).reshape(-1).cuda()
        if many:
            kw["strideRowmap"] = M
    g = spec.get("gather")
    if g is None:
        lda = spec.get("lda", Kd)
        kw["lda"] = lda
        if many:
            kw["strideA"] = M * lda + 5
        kw["A"] = _place(draw((batch - 1) * kw.get("strideA", 0) + M * lda), off[1])
    else:
        seg, rs, R = g["seg"], g["rs"], 37
        segs = Kd // seg
        assert segs * seg == Kd and rs - seg + 1 >= g["cols"]
        if many:
            kw["strideA"] = R * rs + 1
            kw["strideRowoff"] = segs * M
        kw["A"] = _place(draw((batch - 1) * kw.get("strideA", 0) + R * rs), off[1])
        ro = torch.randint(0, R, (batch, segs, M), generator=gen) * rs
        ro = ro + torch.randint(0, g["cols"], (batch, segs, M), generator=gen)
        ro = torch.where(torch.rand((batch, segs, M), generator=gen) < g["pad"], torch.full_like(ro, -1), ro)
        if M > 8:
            ro[:, :, 5] = -1            # one row of nothing but padding
        kw["rowoff"] = ro.to(torch.int32).reshape(-1).cuda()
        kw["seg_len"] = seg
    if "lddw" in spec:
        kw["lddw"] = spec["lddw"]
    lddw = kw.get("lddw", Kd)
    if many:
        kw["strideDW"] = N * lddw + 6
        kw["strideDB"] = N + 1
    kw["_off_dW"] = off[2]
    return kw, spec.get("dB", True)


def _launch(ops, kw, with_dB, off_dW=0, off_dB=0):
    """Run the call into fresh guarded NaN buffers.  Returns dict(dW=(after, before, lead), dB=..., parts=..., split)."""
    kw = {k: v for k, v in kw.items() if not k.startswith("_")}
    M, N, Kd, batch = kw["M"], kw["N"], kw["Kd"], kw.get("batch", 1)
    lddw = kw.get("lddw") or Kd
    ws = ops.wgrad_workspace_floats(M, N, Kd, batch)
    out = dict(split=WR.split_of(ws, N, Kd, batch), ws=ws)
    bW, lW = _guarded((batch - 1) * kw.get("strideDW", 0) + (N - 1) * lddw + Kd, off_dW)
    out["dW"] = (bW, bW.clone(), lW)
    dB = None
    if with_dB:
        bB, lB = _guarded((batch - 1) * kw.get("strideDB", 0) + N, off_dB)
        out["dB"] = (bB, bB.clone(), lB)
        dB = bB[lB:]
    parts = None
    if ws:
        bP, lP = _guarded(ws)
        out["parts"] = (bP, bP.clone(), lP)
        parts = bP[lP:lP + ws]
        assert parts.numel() == ws
    ops.wgrad(kw["dY"], kw["A"], bW[lW:], dB=dB, parts=parts,
              **{k: v for k, v in kw.items() if k not in ("dY", "A")})
    torch.cuda.synchronize()
    return out


def _guards_intact(out):
    bad = []
    i32 = torch.int32
    for name in ("dW", "dB"):
        if name in out:
            after, before, lead = out[name]
            if not torch.equal(after[:lead].view(i32), before[:lead].view(i32)):
                bad.append(f"{name}: front guard written")
    if "parts" in out:
        after, before, lead = out["parts"]
        ws = out["ws"]
        if not (torch.equal(after[:lead].view(i32), before[:lead].view(i32))
                and torch.equal(after[lead + ws:].view(i32), before[lead + ws:].view(i32))):
            bad.append("parts: guard written")
    return bad


def _check(ops, kw, with_dB, dt, exact, device, off_dW=0, off_dB=0):
    """Launch and compare with the restatement: (failures, split, dW verdict, dB verdict or None)."""
    out = _launch(ops, kw, with_dB, off_dW, off_dB)
    call = {k: v for k, v in kw.items() if not k.startswith("_")}
    aW, bW, lW = out["dW"]
    dB_before = out["dB"][1][out["dB"][2]:] if with_dB else None
    e = WR.expected(call, bW[lW:], dB_before, device=device)
    n = WR.roundings(kw["M"], out["split"], dt)
    fails = _guards_intact(out)
    vW = WR.compare(aW[lW:], bW[lW:], e.dW, e.dW_written, e.S, n, exact=exact)
    if not vW.ok:
        fails.append(f"dW: {vW}")
    vB = None
    if with_dB:
        aB, bB, lB = out["dB"]
        vB = WR.compare(aB[lB:], bB[lB:], e.dB, e.dB_written, e.Sb, n, exact=exact)
        if not vB.ok:
            fails.append(f"dB: {vB}")
    return fails, out["split"], vW, vB


def test_case_set_covers_the_splits(ops):
    splits = {}
    for name, spec in CASES.items():
        M, N, Kd, batch = _shape(spec)
        splits.setdefault(WR.split_of(ops.wgrad_workspace_floats(M, N, Kd, batch), N, Kd, batch), []).append(name)
    print({k: len(v) for k, v in sorted(splits.items())})
    assert {1, 2, 3, 64} <= set(splits), sorted(splits)
    # the shape whose last split is empty: 64 splits of 640 rows, the last one starting past M
    assert WR.split_of(ops.wgrad_workspace_floats(40000, 64, 48, 1), 64, 48, 1) == 64
    assert WR.roundings(40000, 64, torch.bfloat16) - 63 == 640 and 63 * 640 >= 40000 > 62 * 640
    batched = [n for s, ns in splits.items() if s > 1 for n in ns if _shape(CASES[n])[3] > 1]
    assert batched, "no batched case splits"


@pytest.mark.parametrize("name,dt", PARAMS)
def test_exact_integer_inputs(ops, name, dt):
    kw, with_dB = _build(CASES[name], dt, True, seed=len(name))
    fails, split, vW, vB = _check(ops, kw, with_dB, dt, True, "cpu", off_dW=kw.get("_off_dW", 0))
    assert not fails, f"{name} {_tag(dt)} split {split}: " + "; ".join(fails)


@pytest.mark.parametrize("name,dt", PARAMS)
def test_rounding_normal_inputs(ops, name, dt):
    kw, with_dB = _build(CASES[name], dt, False, seed=1000 + len(name))
    fails, split, vW, vB = _check(ops, kw, with_dB, dt, False, "cpu", off_dW=kw.get("_off_dW", 0))
    cls = f"{_tag(dt)} {'split' if split > 1 else 'one pass'}"
    print(f"{name} {_tag(dt)} split {split}: dW {vW}" + (f"; dB {vB}" if vB else ""))
    _note(f"cases dW {cls}", vW.ratio)
    if vB is not None:
        _note(f"cases dB {cls}", vB.ratio)
    assert not fails, f"{name} {_tag(dt)} split {split}: " + "; ".join(fails)


# ---------------------------------------------------------------------------------------------------------------
# c. recorded calls
# ---------------------------------------------------------------------------------------------------------------
_TENSORS = ("dY", "A", "rowoff", "dy_rowmap")


def _describe(v):
    if isinstance(v, torch.Tensor):
        return ("T", tuple(v.shape), tuple(v.stride()), str(v.dtype), v.data_ptr() % 16)
    return v


def _record(ops, monkeypatch, step):
    """Run step() with ops.wgrad wrapped: one record per distinct argument set, each tensor kept as a copy of what its
    pointer reaches (placed at the same address modulo 16 on replay)."""
    real = ops.wgrad
    seen, calls = set(), []

    def wrapper(dY, A, dW, **kw):
        sig = (_describe(dY), _describe(A), _describe(dW),
               tuple(sorted((k, _describe(v)) for k, v in kw.items() if k != "parts")))
        if sig not in seen:
            seen.add(sig)
            rec = {k: v for k, v in kw.items() if k not in ("parts", "dB") and v is not None}
            for k, t in (("dY", dY), ("A", A), ("rowoff", kw.get("rowoff")), ("dy_rowmap", kw.get("dy_rowmap"))):
                if t is not None:
                    rec[k] = (WR.flat(t).clone(), t.data_ptr() % 16)
            rec["_with_dB"] = kw.get("dB") is not None
            rec["_off_dW"] = dW.data_ptr() % 16
            rec["_off_dB"] = kw["dB"].data_ptr() % 16 if kw.get("dB") is not None else 0
            calls.append(rec)
        return real(dY, A, dW, **kw)

    monkeypatch.setattr(ops, "wgrad", wrapper)
    step()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "wgrad", real)
    return calls


def _kind(c):
    s = f"M{c['M']} N{c['N']} K{c['Kd']}"
    if c.get("batch", 1) > 1:
        s += f" b{c['batch']}"
    if c.get("rowoff") is not None:
        s += " gathered"
    if c.get("dy_rowmap") is not None:
        s += " row-mapped"
    if c.get("strideDY", 0) and c.get("strideDY") == c.get("strideA") and c.get("batch", 1) > 1:
        s += " aux"
    return s


def _replay(ops, calls, dt, label):
    fails, kinds = [], []
    for c in calls:
        kw = {k: v for k, v in c.items() if k not in _TENSORS}
        for k in _TENSORS:
            if k in c:
                vals, align = c[k]
                kw[k] = _place(vals, align)
        f, split, vW, vB = _check(ops, kw, c["_with_dB"], dt, False, "cuda", off_dW=c["_off_dW"], off_dB=c["_off_dB"])
        print(f"  [{label}] {_kind(c):48s} split {split:2d}: dW {vW}" + (f"; dB {vB}" if vB else ""))
        _note(f"recorded dW {_tag(dt)}", vW.ratio)
        if vB is not None:
            _note(f"recorded dB {_tag(dt)}", vB.ratio)
        fails += [f"{_kind(c)} split {split}: {x}" for x in f]
        kinds.append((c, split))
        del kw
        torch.cuda.empty_cache()
    return fails, kinds


def _head_step(head, feats, dt, seed):
    head = head.cuda().set_compute_dtype(dt).train()
    outs = head(feats)
    g = torch.Generator().manual_seed(seed)
    torch.autograd.backward(list(outs), [torch.randn(o.shape, generator=g).cuda() for o in outs])


def _train_py_head():
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.synthetic import synthetic_features, synthetic_head_state
    Cc, K = 384, 20
    head = ProbMapHead(Cc, K, [(4, 4), (2, 2), (2, 2)], (256, 256), (4, 4), final_layer_kernel_size=1,
                       freeze_error=True, normalize=1.0, differentiable=True)
    head.load_state_dict(synthetic_head_state(Cc, K, n_pools=3, deconv_out=(256, 256), seed=3), strict=False)
    return head, synthetic_features(32, Cc, 24, 24, seed=8).cuda()


def _vit_b_head():
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.synthetic import synthetic_features, synthetic_head_state
    Cc, K = 768, 17
    head = ProbMapHead(Cc, K, [(4, 3), (2, 2), (2, 2)], (256, 256), (4, 4), differentiable=True)
    head.load_state_dict(synthetic_head_state(Cc, K, n_pools=3, deconv_out=(256, 256), seed=5), strict=False)
    return head, synthetic_features(64, Cc, 16, 12, seed=5).cuda()


HEADS = [("train.py head bs 32", _train_py_head, torch.bfloat16), ("ViT-B bench head bs 64", _vit_b_head, torch.bfloat16),
         ("ViT-B bench head bs 64", _vit_b_head, torch.float32)]


@pytest.mark.parametrize("label,make,dt", HEADS, ids=[f"{h[0]}-{_tag(h[2])}" for h in HEADS])
def test_recorded_head_calls(ops, monkeypatch, label, make, dt):
    t0 = time.time()
    head, feats = make()
    calls = _record(ops, monkeypatch, lambda: _head_step(head, feats, dt, 6))
    del head, feats
    torch.cuda.empty_cache()
    print(f"\n[{label} {_tag(dt)}] {len(calls)} distinct wgrad calls")
    fails, kinds = _replay(ops, calls, dt, f"{label} {_tag(dt)}")
    assert any(c.get("rowoff") is not None for c, _ in kinds), "no gathered call recorded"
    assert any(c.get("dy_rowmap") is not None and c.get("batch", 1) > 1 for c, _ in kinds), \
        "no row-mapped batched call recorded"
    assert any(s > 1 for _, s in kinds), "no recorded call splits"
    assert any(c.get("batch", 1) > 1 and c.get("strideDY", 0) == c["N"] and c.get("strideA", 0) == c["N"]
               and c.get("strideDW", 0) == 9 * c["N"] ** 2 for c, _ in kinds), "no batched aux call recorded"
    print(f"[{label} {_tag(dt)}] {time.time() - t0:.0f} s")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ["train_py_d2", "vit_b_d1"])
def test_recorded_backbone_calls(ops, monkeypatch, name):
    from tests import test_vit_grad_gpu as VG
    t0 = time.time()
    bb, x, ups = VG._case(name)
    calls = _record(ops, monkeypatch, lambda: VG._hip_step(bb, x, ups, torch.bfloat16))
    del bb
    torch.cuda.empty_cache()
    print(f"\n[{name} bf16] {len(calls)} distinct wgrad calls")
    fails, kinds = _replay(ops, calls, torch.bfloat16, f"{name} bf16")
    # fc2, fc1, proj and qkv differ in shape (the patch embedding's call shares proj's argument set where K0 = C)
    assert len(kinds) >= 4, "the linear layers' calls were not recorded"
    print(f"[{name} bf16] {time.time() - t0:.0f} s")
    assert not fails, "\n".join(fails)


def test_device_path_agrees_with_the_cpu_restatement(ops):
    kw, _ = _build(CASES["batch 2 every stride split"], torch.bfloat16, False, seed=77)
    call = {k: v for k, v in kw.items() if not k.startswith("_")}
    nW = call["batch"] * call["strideDW"] + 8
    nB = call["batch"] * call["strideDB"] + 8
    dW0, dB0 = WR.nan_like_bits(nW, torch.float32, "cuda"), WR.nan_like_bits(nB, torch.float32, "cuda")
    a, b = WR.expected(call, dW0, dB0, device="cpu"), WR.expected(call, dW0, dB0, device="cuda")
    for name in ("dW", "S", "dB", "Sb"):
        x, y = getattr(a, name), getattr(b, name).cpu()
        scale = getattr(a, "S" if name in ("dW", "S") else "Sb")
        ok = ((x - y).abs() <= 1e-13 * scale) | (x.isnan() & y.isnan())
        assert bool(ok.all()), name
    assert torch.equal(a.dW_written, b.dW_written.cpu()) and torch.equal(a.dB_written, b.dB_written.cpu())


@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("name", ["batch 4 every stride split", "split 64, last split empty", "aux batched split"])
def test_two_launches_give_equal_bits(ops, name, dt):
    kw, with_dB = _build(CASES[name], dt, False, seed=5)
    a, b = _launch(ops, kw, with_dB), _launch(ops, kw, with_dB)
    assert a["split"] > 1
    for k in ("dW", "dB"):
        assert torch.equal(a[k][0].view(torch.int32), b[k][0].view(torch.int32)), k


def test_refusals_write_nothing(ops):
    from probpose_pytorch_amd import _lib
    lib = _lib.lib()
    M, N, Kd = 600, 8, 8
    assert ops.wgrad_workspace_floats(M, N, Kd, 1) > 0
    dY = torch.ones((M, N), device="cuda")
    A = torch.ones((M, Kd), device="cuda")
    ro = torch.zeros((M,), dtype=torch.int32, device="cuda")
    bW, lW = _guarded(N * Kd)
    bB, lB = _guarded(N)
    bP, lP = _guarded(ops.wgrad_workspace_floats(M, N, Kd, 1))
    before = [t.clone() for t in (bW, bB, bP)]

    def args(**over):
        a = _lib.WgradArgs()
        a.dY, a.ldd, a.A, a.lda = _lib.ptr(dY), N, _lib.ptr(A), Kd
        a.dW, a.lddw, a.dB, a.parts = _lib.ptr(bW[lW:]), Kd, _lib.ptr(bB[lB:]), _lib.ptr(bP[lP:])
        a.M, a.N, a.Kd, a.batch, a.dtype = M, N, Kd, 1, _lib.PP_F32
        for k, v in over.items():
            setattr(a, k, v)
        return a

    refused = [("parts", args(parts=None)), ("ldd", args(ldd=N - 1)), ("lddw", args(lddw=Kd - 1)),
               ("seg_len", args(rowoff=_lib.ptr(ro), seg_len=3)), ("dtype", args(dtype=_lib.PP_FP8)),
               ("dtype", args(dtype=7))]
    for what, a in refused:
        rc = lib.pp_wgrad_gemm(C.byref(a), _lib.stream_ptr())
        assert rc != 0, what
        with pytest.raises(_lib.HipExtensionError, match=what):
            _lib.check(rc, "pp_wgrad_gemm")
    # through ops.wgrad: a dtype the C ABI knows but this kernel does not take
    f8 = torch.zeros((M, N), device="cuda").to(torch.float8_e4m3fn)
    with pytest.raises(_lib.HipExtensionError, match="dtype"):
        ops.wgrad(f8, f8, bW[lW:], M=M, N=N, Kd=Kd, ldd=N, lda=Kd, parts=bP[lP:])
    torch.cuda.synchronize()
    for t, b in zip((bW, bB, bP), before):
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    # the accepted call does write (the refusals above were not vacuous)
    rc = lib.pp_wgrad_gemm(C.byref(args()), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and float(bW[lW]) == M and float(bB[lB]) == M


def test_report_worst_ratios():
    """Prints the worst d/bound per class of the tests above (run with -s)."""
    for k, v in sorted(_WORST.items()):
        print(f"worst d/bound {k}: {v:.3g}")
