"""Every GEMM tile form the autotuner can select, on the real layer calls of each benchmarked configuration, against
the float64 restatement of pp_gemm (tests/gemm_reference.py).

bench.py turns ops.AUTOTUNE on: during the warm-up, every GEMM call with M * N * Kd >= 2^24 times each form of
ops._TUNE_CANDIDATES that pp_gemm accepts and keeps the fastest, on speed alone.  Here one forward of each
configuration (bench.build, bench.CONFIGS batch sizes) is recorded through ops.gemm, one call per distinct argument
set is kept with clones of its inputs, and every candidate form is launched on it into a NaN-filled output with guard
elements on both sides (C's 16-byte alignment unchanged: it decides the LDS epilogue and which forms accept the call).
A refusal means "not applicable"; every other form must match the float64 result within the call's own scale and
leave every element outside what the call writes bit-identical."""
import pytest
import torch

from tests import gemm_reference as gr

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
CONFIGS = [("vit_b", torch.bfloat16), ("vit_b", torch.float32), ("vit_l", torch.bfloat16), ("vit_l", FP8),
           ("vit_h_wholebody", torch.bfloat16)]
_TENSOR_ARGS = ("bias", "residual", "rowbias", "rowoff", "out_rowmap", "colscale")


@pytest.fixture
def ops(built_lib, monkeypatch):
    assert torch.cuda.is_available()
    from probpose_pytorch_amd import ops as o
    monkeypatch.setattr(o, "AUTOTUNE", o.AUTOTUNE)
    monkeypatch.setattr(o, "_TUNE_CACHE", dict(o._TUNE_CACHE))
    return o


def _describe(v):
    if isinstance(v, torch.Tensor):
        return ("T", tuple(v.shape), tuple(v.stride()), str(v.dtype), v.data_ptr() % 16)
    return v


def _record(ops, monkeypatch, model, x):
    """One forward with ops.gemm wrapped: every call the tuner would tune (ops.gemm hands it to ops._tune, replaced
    here by a stub that keeps the tune key and selects nothing), once per distinct argument set, with its inputs."""
    real = ops.gemm
    seen, calls = set(), []
    tuned = {}

    def stub(a, key, out, residual):
        tuned["key"] = key
        return 0

    def wrapper(A, W, out, **kw):
        sig = (_describe(A), _describe(W), _describe(out), kw.get("residual") is out,
               tuple(sorted((k, _describe(v)) for k, v in kw.items())))
        if sig in seen:
            return real(A, W, out, **kw)
        assert A.is_contiguous() and W.is_contiguous() and out.is_contiguous()
        rec = dict(kw, A=A.clone(), W=W.clone())
        for k in _TENSOR_ARGS:
            if kw.get(k) is not None:
                rec[k] = kw[k].clone()
        rec["out_like"] = (tuple(out.shape), out.dtype, out.data_ptr() % 16)
        rec["in_place"] = kw.get("residual") is out
        tuned.clear()
        r = real(A, W, out, **kw)
        seen.add(sig)
        if "key" in tuned:
            rec["key"] = tuned["key"]
            calls.append(rec)
        return r

    monkeypatch.setattr(ops, "AUTOTUNE", True)
    monkeypatch.setattr(ops, "_tune", stub)
    monkeypatch.setattr(ops, "gemm", wrapper)
    with torch.no_grad():
        model(x)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "gemm", real)
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    return calls


def _name(c):
    s = f"M{c['M']}xN{c['N']}xK{c['Kd']}"
    for k, tag in (("batch", "b"), ("splitk", "s")):
        if c.get(k, 1) > 1:
            s += f"x{tag}{c[k]}"
    s += "".join(f" {t}" for k, t in (("rowoff", "gather"), ("out_rowmap", "scatter"), ("residual", "resid"),
                                       ("rowbias", "rowbias"), ("headmajor", "headmajor"), ("heatmap", "heatmap"))
                 if c.get(k) is not None)
    epi = c.get("epilogue", 0)
    s += (" gelu" if epi & gr.EPI_GELU else "") + (" relu" if epi & gr.EPI_RELU else "")
    return s + f" ->{str(c['out_like'][1]).replace('torch.', '')}"


def _launch(ops, c, tile, template):
    """Run call c with tile `tile` on a fresh copy of `template` (lead guard + output + trailing guard); returns the
    buffer after the launch, or None when pp_gemm refuses the form."""
    from probpose_pytorch_amd import _lib
    lead, numel = c["lead"], c["numel"]
    buf = template.clone()
    shape = c["out_like"][0]
    out = buf[lead:lead + numel].view(shape)
    kw = {k: v for k, v in c.items() if k not in ("A", "W", "out_like", "in_place", "key", "lead", "numel")}
    if c["in_place"]:
        kw["residual"] = out
    kw["tile"] = tile
    try:
        ops.gemm(c["A"], c["W"], out, **kw)
    except _lib.HipExtensionError:
        return None
    if buf.is_cuda:
        torch.cuda.synchronize()
    return buf


def _sweep_call(ops, c, forms, device, check=None):
    """Launch every form on call c and compare each result with the float64 restatement: (accepted forms, failures).
    check(tile, verdict, buffer from C on, written): a caller's further conditions; it may clear verdict.ok."""
    shape, odt, align = c["out_like"]
    esz = torch.empty((), dtype=odt).element_size()
    numel = 1
    for s in shape:
        numel *= s
    lead = (64 + align) // esz                      # a front guard, and C at the original address modulo 16
    guard = -(-max(4 * shape[-1] * esz, 64) // 16) * 16 // esz
    c["lead"], c["numel"] = lead, numel
    template = gr.nan_like_bits(lead + numel + guard, odt, device)
    if c["in_place"]:
        template[lead:lead + numel] = c["residual"].reshape(-1)
    kw_ref = {k: v for k, v in c.items() if k not in ("out_like", "in_place", "key", "lead", "numel")}
    kw_ref["out"] = template[lead:lead + numel].view(shape)
    compute = torch.bfloat16 if c["W"].dtype == FP8 else c["W"].dtype   # an fp8 GEMM is held to the bf16 bound
    ref, written = gr.expected_output(kw_ref, template[lead:])
    bits = gr._BITS[odt]
    ok_forms, failures = [], []
    for tile in forms:
        buf = _launch(ops, c, tile, template)
        if buf is None:
            print(f"  {_name(c):64s} form {tile:2d}: refused")
            continue
        ok_forms.append(tile)
        v = gr.compare(buf[lead:], template[lead:], ref, written, compute)
        if not torch.equal(buf[:lead].view(bits), template[:lead].view(bits)):
            v.ok = False
            v.note += " (front guard written)"
        if check is not None:
            check(tile, v, buf[lead:], written)
        print(f"  {_name(c):64s} form {tile:2d}: {v}")
        if not v.ok:
            failures.append(f"{_name(c)} form {tile}: {v}")
    return ok_forms, failures


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=[f"{n}-{str(d).replace('torch.', '')}" for n, d in CONFIGS])
def test_every_tuner_form_on_the_benchmark_calls(ops, monkeypatch, name, dtype):
    import time

    import bench
    t0 = time.time()
    cfg = dict(bench.CONFIGS[name])
    model, _, _ = bench.build(cfg, dtype, torch.device("cuda", 0))
    H, W = cfg["img"]
    from probpose_pytorch_amd.synthetic import synthetic_crops
    x = synthetic_crops(cfg["batch"], H, W, seed=1234).cuda()
    calls = _record(ops, monkeypatch, model, x)
    del model, x
    torch.cuda.empty_cache()
    assert calls, "no GEMM call reached the tuner"
    forms = tuple(ops._TUNE_CANDIDATES)
    failures, accepted = [], []
    print(f"\n[{name} {str(dtype).replace('torch.', '')}] {len(calls)} tuned calls, forms {forms}")
    for c in calls:
        ok_forms, bad = _sweep_call(ops, c, forms, "cuda")
        failures += bad
        accepted.append((c["key"], tuple(ok_forms), _name(c)))
        torch.cuda.empty_cache()
    # the tuner caches one winner per tune key: calls that share a key must accept the same forms
    by_key = {}
    for key, ok_forms, nm in accepted:
        by_key.setdefault(key, []).append((ok_forms, nm))
    for key, group in by_key.items():
        if len({f for f, _ in group}) > 1:
            failures.append(f"tune key {key}: calls accept different forms: {group}")
    print(f"[{name}] {time.time() - t0:.0f} s")
    assert not failures, "\n".join(failures)
