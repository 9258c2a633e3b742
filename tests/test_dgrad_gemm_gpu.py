"""The pp_gemm calls that only a training step makes (the data gradients of head_train.py and vit_train.py and the
train-mode forward's f32 linears), each on every tile form of GEMM_FORMS (1 - 10, 13, 14, 18 - 20: a superset of
ops._TUNE_CANDIDATES, any of which the autotuner may choose on speed alone), against float64.

The calls are built by tests/dgrad_reference.py from the product's own packers and tables (pinned on the CPU by
tests/test_dgrad_reference.py) and launched the way tests/test_gemm_tuner_forms_gpu.py launches its recorded calls: into
a NaN-bit output with a front and a back guard, C at the call's address modulo 16, the in-place residual inside the
buffer itself.

a. Exact.  Integer data in [-3, 3]: every sum is exact in f32 (at most 2304 terms of magnitude <= 9), so every form
   must give torch's float64 autograd result of the layer bit for bit and leave every other element's bits alone.  The
   one bf16 output (the proj data gradient) gets output-gradient rows with 28 non-zeros: |result| <= 252, exact in bf16.
b. Rounding.  randn gradients, randn * Kd^-1/2 weights: gemm_reference.compare's verdict (the project's own tolerance,
   gemm_reference.tolerance) must be ok.
c. Recorded calls.  Every ops.gemm call (tuned or not) of one forward + backward step of the training heads
   head_grad_reference.CASES T2 and T4 (and T2 without a heatmap gradient, which is the one way the aux-0 data gradient
   is written plainly) and of the backbones tiny, ragged and tiny_hd64 of test_vit_grad_gpu.MODELS, without and with a
   stochastic-depth mask that drops a crop; one record per distinct argument set, replayed on every form against the
   restatement.  Each test asserts that the call kinds it is there for were recorded.

A HipExtensionError from a form means "not applicable", but every per-launch form (1 - 7 and 10, plus 8 and 9 for
bf16) must accept every call, a call no form accepted fails, and the whole-tile proj shapes must be admitted by forms
13, 14, 18, 19 (768 x 576 x 576) and 20 (768 x 768 x 512).  f32 launches leave out the bf16-only forms.  One line is
printed per (call, form) (run with -s); test_report_worst_ratios prints the worst max|d| / rms per kind and dtype."""
import time

import pytest
import torch

from tests import dgrad_reference as DR
from tests import gemm_reference as gr
from tests import test_gemm_tuner_forms_gpu as TF

pytestmark = pytest.mark.gpu

GRID = (1, 2, 3, 4, 5, 6, 7, 10)             # per-launch forms built for f32 and bf16
WIDE = (8, 9)                                # per-launch forms built for bf16 only
FORMS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 18, 19, 20)
DTYPES = [torch.bfloat16, torch.float32]
PARAMS = [pytest.param(k, dt, id=f"{k}-{str(dt).replace('torch.', '')}") for k in DR.KINDS for dt in DTYPES]
_WORST: dict = {}


@pytest.fixture
def ops(built_lib):
    assert torch.cuda.is_available()
    from probpose_pytorch_amd import ops as o
    assert set(o._TUNE_CANDIDATES) <= set(FORMS)
    return o


def _tag(dt):
    return str(dt).replace("torch.", "")


def _forms(dt):
    return FORMS if dt == torch.bfloat16 else GRID


def _record_of(call):
    """A dgrad_reference.Call as test_gemm_tuner_forms_gpu._sweep_call takes a recorded call, on the GPU."""
    out = call.kw["out"]
    rec = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in call.kw.items() if k != "out"}
    rec["in_place"] = call.in_place
    if call.in_place:
        rec["residual"] = out.reshape(-1).cuda()
    rec["out_like"] = (tuple(out.shape), out.dtype, 0)
    return rec


def _sweep(ops, rec, label, cls, truth=None):
    """Every form of the operand dtype on one call: (accepted forms, failures).  truth: the result every accepting form
    must give bit for bit."""
    dt = rec["W"].dtype

    def check(tile, v, got, written):
        _WORST[cls] = max(_WORST.get(cls, 0.0), v.rel)
        if truth is not None:
            n = truth.numel()
            if not (bool(written[:n].all()) and torch.equal(got[:n].view(truth.shape).double(), truth)):
                v.ok = False
                v.note += " (differs from the float64 autograd result)"

    ok_forms, fails = TF._sweep_call(ops, rec, _forms(dt), "cuda", check=check)
    refused = [t for t in GRID + (WIDE if dt == torch.bfloat16 else ()) if t not in ok_forms]
    if refused:
        fails.append(f"{label}: per-launch forms {refused} refused the call")
    if not ok_forms:
        fails.append(f"{label}: no form accepted the call")
    return ok_forms, [f"{label}: {f}" for f in fails]


def _run_cases(ops, kind, dt, ints):
    fails, accepted = [], {}
    for i, case in enumerate(DR.CASES[kind]):
        call = DR.make(kind, case, dt, ints, seed=100 * int(not ints) + i)
        label = f"{kind} {_tag(dt)} {case}"
        print(f"\n[{label}] {'integer' if ints else 'normal'} data")
        truth = call.truth.cuda() if ints else None
        ok_forms, bad = _sweep(ops, _record_of(call), label, (("exact" if ints else "rounding"), kind, _tag(dt)), truth)
        accepted[case] = ok_forms
        fails += bad
    if kind == "proj_dgrad" and dt == torch.bfloat16:
        if not {13, 14, 18, 19} <= set(accepted[(768, 576, 576)]):
            fails.append(f"(768, 576, 576): forms 13, 14, 18, 19 must admit it, accepted {accepted[(768, 576, 576)]}")
        if 20 not in accepted[(768, 768, 512)]:
            fails.append(f"(768, 768, 512): form 20 must admit it, accepted {accepted[(768, 768, 512)]}")
    return fails


@pytest.mark.parametrize("kind,dt", PARAMS)
def test_exact_integer_data(ops, kind, dt):
    fails = _run_cases(ops, kind, dt, True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind,dt", PARAMS)
def test_rounding_normal_data(ops, kind, dt):
    fails = _run_cases(ops, kind, dt, False)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------
# c. recorded calls
# ---------------------------------------------------------------------------------------------------------------
def _record(ops, monkeypatch, step):
    """Run step() with ops.gemm wrapped: one record per distinct argument set, every tensor kept as a copy of what its
    pointer reaches (the in-place residual as the output's values from before the call)."""
    real = ops.gemm
    seen, calls = set(), []

    def wrapper(A, W, out, **kw):
        in_place = kw.get("residual") is out
        sig = (TF._describe(A), TF._describe(W), TF._describe(out), in_place,
               tuple(sorted((k, TF._describe(v)) for k, v in kw.items())))
        if sig not in seen:
            seen.add(sig)
            assert out.is_contiguous()
            rec = {k: v for k, v in kw.items() if v is not None}
            rec.update(A=gr.flat(A).clone(), W=gr.flat(W).clone())
            for k in TF._TENSOR_ARGS:
                if kw.get(k) is not None:
                    rec[k] = gr.flat(kw[k]).clone()
            if in_place:
                rec["residual"] = out.reshape(-1).clone()
            rec["in_place"] = in_place
            rec["out_like"] = (tuple(out.shape), out.dtype, out.data_ptr() % 16)
            calls.append(rec)
        return real(A, W, out, **kw)

    monkeypatch.setattr(ops, "gemm", wrapper)
    step()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "gemm", real)
    return calls


def _kind(c, C=None, hidden=None, K=None):
    """The training-only call kind of a recorded call (dgrad_reference.KINDS), or None for any other call."""
    N, Kd = c["N"], c["Kd"]
    odt = c["out_like"][1]
    f32_out = odt == torch.float32 and (c["W"].dtype == torch.float32 or c.get("epilogue", 0) & gr.EPI_OUT_F32)
    bias, resid, batch = c.get("bias") is not None, c.get("residual") is not None, c.get("batch", 1)
    if c.get("rowbias") is not None or c.get("out_rowmap") is not None or c.get("heatmap") is not None:
        return None
    if c.get("rowoff") is not None:
        if bias or not f32_out:
            return None
        if batch == 4 and c.get("strideA") == N == c.get("strideC") and c["lda"] == 4 * N == c["ldc"] and not resid:
            return "aux_stage"
        if batch == 1 and c["lda"] == 4 * N and c["ldc"] == N and Kd % (9 * N) == 0 and c["seg_len"] == N:
            return "aux0_resid" if c["in_place"] else (None if resid else "aux0")
        if batch == 1 and Kd == 16 * c["seg_len"] and c["lda"] == c["seg_len"] and not resid:
            return "deconv"
        return None
    if batch != 1:
        return None
    if K is not None:
        KPAD = -(-K // 64) * 64
        if (not bias and not resid and f32_out and Kd == KPAD == c["lda"] == c["ldw"]
                and not bool(c["W"][:N * Kd].view(N, Kd)[:, K:].any())):
            return "final"
        return None
    if not bias and not resid:
        if f32_out and c.get("epilogue", 0) == gr.EPI_OUT_F32:
            return {(hidden, C): "fc2_dgrad", (C, hidden): "fc1_dgrad", (C, 3 * C): "qkv_dgrad"}.get((N, Kd))
        if c.get("epilogue", 0) == 0 and odt == c["W"].dtype and (N, Kd) == (C, C):
            return "proj_dgrad"
        return None
    if bias and f32_out:
        if resid:
            return "fwd_resid" if not c["in_place"] and N == C and Kd in (C, hidden) else None
        if N == C and Kd in (C, hidden):
            return "fwd_branch"
        if (N, Kd) == (hidden, C):
            return "fwd_fc1"
    return None


def _replay(ops, calls, label, **dims):
    fails, kinds = [], {}
    for c in calls:
        k = _kind(c, **dims)
        kinds.setdefault(k, []).append(c)
        print(f"\n[{label}] {k or 'other'}")
        _, bad = _sweep(ops, c, f"{label} {k or 'other'} {TF._name(c)}", ("recorded", k or "other", _tag(c["W"].dtype)))
        fails += bad
        torch.cuda.empty_cache()
    return fails, kinds


HEAD_STEPS = [("T2", True), ("T4", True), ("T2", False)]


@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("name,heat", HEAD_STEPS, ids=["T2", "T4", "T2-no-heatmap-gradient"])
def test_recorded_head_calls(ops, monkeypatch, name, heat, dt):
    from tests import head_grad_reference as HR
    t0 = time.time()
    head, feats, ups, cfg, xg = HR.case(name, differentiable=True)
    assert xg
    head = head.cuda().set_compute_dtype(dt).train()

    def step():
        x = feats.cuda().requires_grad_(True)
        outs = head(x)
        pairs = [(o, u.float().cuda()) for i, (o, u) in enumerate(zip(outs, ups)) if heat or i > 0]
        torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])

    calls = _record(ops, monkeypatch, step)
    label = f"head {name}{'' if heat else ' no heatmap gradient'} {_tag(dt)}"
    print(f"\n[{label}] {len(calls)} distinct gemm calls")
    fails, kinds = _replay(ops, calls, label, K=head.out_channels)
    if heat:
        assert "final" in kinds, "the final layer's data gradient was not recorded"
        assert len(kinds.get("deconv", ())) == 2, "the two deconvolutions' data gradients were not recorded"
        assert not any(bool((c["rowoff"] >= 0).all()) for c in kinds["deconv"]), "a deconv table without a -1"
    assert "aux_stage" in kinds, "the batch = 4 aux-stage data gradient was not recorded"
    if name == "T2":        # detach_probability False: the probability branch's gradient reaches the tokens
        want = "aux0_resid" if heat else "aux0"
        assert want in kinds and bool((kinds[want][0]["rowoff"] < 0).any()), f"the {want} data gradient was not recorded"
    else:
        assert "aux0" not in kinds and "aux0_resid" not in kinds
    print(f"[{label}] {time.time() - t0:.0f} s")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("drop", [False, True], ids=["all-kept", "crop-dropped"])
@pytest.mark.parametrize("name", ["tiny", "ragged", "tiny_hd64"])
def test_recorded_backbone_calls(ops, monkeypatch, name, drop, dt):
    from probpose_pytorch_amd import vit_train
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_vit_state
    from tests import test_vit_grad_gpu as VG
    t0 = time.time()
    img, C, heads, depth, B = VG.MODELS[name]
    extra = dict(drop_path_rate=0.4) if drop else {}
    bb = ScratchViTBackbone(img, 16, embed_dim=C, depth=depth, num_heads=heads, differentiable=True, **extra)
    bb.model.load_state_dict(synthetic_vit_state(img, 16, C, depth, seed=0))
    bb = bb.cuda().set_compute_dtype(dt).train()
    x = synthetic_crops(B, *img, seed=1).cuda()
    keep = None
    if drop:        # the last block (rate 0.4) drops crop 1 in its attention branch and crop 0 in its MLP branch
        assert bb.drop_path_rates[0] == 0 and bb.drop_path_rates[-1] > 0
        keep = torch.ones((depth, 2, B), dtype=torch.bool)
        keep[-1, 0, 1] = keep[-1, 1, 0] = False

    def step():
        t = vit_train.train_forward(bb.model, x, keep=keep)
        t.backward(torch.randn(t.shape, generator=torch.Generator().manual_seed(2)).to(t.dtype).cuda())

    calls = _record(ops, monkeypatch, step)
    hidden = bb.model.blocks[0].mlp.fc1.out_features
    label = f"backbone {name}{' crop dropped' if drop else ''} {_tag(dt)}"
    print(f"\n[{label}] {len(calls)} distinct gemm calls")
    fails, kinds = _replay(ops, calls, label, C=C, hidden=hidden)
    for k in ("fc2_dgrad", "fc1_dgrad", "qkv_dgrad", "proj_dgrad", "fwd_resid", "fwd_fc1"):
        assert k in kinds, f"{k} was not recorded"
    assert {c["Kd"] for c in kinds["fwd_resid"]} == {C, hidden}, "proj and fc2 with their out-of-place residual"
    if drop:
        assert {c["Kd"] for c in kinds.get("fwd_branch", ())} == {C, hidden}, "the dropped branches' f32 outputs"
        N = (img[0] // 16) * (img[1] // 16)
        assert {c["M"] for c in kinds["fc2_dgrad"]} == {B * N, (B - 1) * N}, "the compact rows' data gradient"
    else:
        assert "fwd_branch" not in kinds
    print(f"[{label}] {time.time() - t0:.0f} s")
    assert not fails, "\n".join(fails)


def test_report_worst_ratios():
    """Prints the worst max|d| / rms per section, call kind and dtype of the tests above (run with -s)."""
    for k, v in sorted(_WORST.items()):
        print(f"worst max|d|/rms {' '.join(k)}: {v:.3g}")
