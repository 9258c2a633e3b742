"""engine.VitPlan's fp8 bookkeeping against the float64 restatement of tests/fp8_walk_reference.py, stage by stage.

Every kernel of fp8 mode has its own float64 test, each taking the scales from the call's arguments.  Here the
arguments themselves are held to a restatement built from the state dict and from a recorded bf16 pass: the plan's
e4m3 weights, row scales, activation scales and column scales (calibration, recalibration, margin), the launch
sequence of one forward with the scale / column scale / weights each launch is handed, bit-identical dataflow from
producer to consumer (also for a smaller batch in the leading rows of a larger workspace), every stage's output
against the float64 value of its own recorded input inside the per-kernel bounds of gemm_reference /
attention_reference, saturation on a batch brighter than the calibration batch, and guards around the three e4m3
producers.  The free-running distance to a float64 walk that quantises at the same four points is printed, not
asserted: one flipped e4m3 rounding moves a value by a whole step and no per-element bound follows for a chain of
them; sequence + dataflow + stage values cover the chain by induction.

The models are fp8_walk_reference.MODELS (A: C 128, head dim 64, M = 60 rows; B: C 256, head dim 32, N = 15; C = 192
is refused by the fp8 GEMM, whose K comes in multiples of 128), with the conditioned states of
fp8_walk_reference.condition_state; the input condition is asserted on every restatement used."""
import pytest
import torch

from tests import fp8_walk_reference as fw
from tests import gemm_reference as gr
from tests.walk_recording import VIT_OPS, recording

pytestmark = pytest.mark.gpu

FP8, BF16 = fw.FP8, torch.bfloat16
CASES = [(m, p) for m in fw.MODELS for p in (False, True)]
CASE_IDS = [f"{m}-{'proj_fp8' if p else 'proj_bf16'}" for m, p in CASES]


@pytest.fixture(scope="module")
def ops(built_lib):
    assert torch.cuda.is_available()
    from probpose_pytorch_amd import ops as o
    return o


class Rig:
    """One model on the GPU, its conditioned state, the four batches, and the bf16 pass of each batch recorded before
    the model goes to fp8 (the kernels are deterministic: this is the pass _calibrate_fp8 runs)."""

    def __init__(self, ops, name):
        from probpose_pytorch_amd.backbone import ScratchViTBackbone
        self.ops, self.cfg = ops, fw.MODELS[name]
        cfg = self.cfg
        self.depth = cfg["depth"]
        sd = fw.model_state(cfg)
        self.model = ScratchViTBackbone(cfg["img"], cfg["patch"], embed_dim=cfg["C"], depth=cfg["depth"],
                                        num_heads=cfg["heads"])
        self.model.model.load_state_dict(sd)
        self.model = self.model.cuda().eval()
        self.sd = {k: v.cuda() for k, v in sd.items()}
        self.xs = {k: v.cuda() for k, v in fw.batches(cfg).items()}
        self.small = max(2, cfg["B"] - 2)                  # a smaller batch for the leading rows of the workspace
        self.model.set_compute_dtype(BF16)
        self.acts, self.bf16_tokens = {}, {}
        for k, x in self.xs.items():
            rec, tok = self.forward(x)
            self.acts[k] = fw.activations(rec, self.depth)
            self.bf16_tokens[k] = tok
        self.model.set_compute_dtype(FP8)

    @property
    def plan(self):
        return self.model.model._plan(self.xs["x1"].device)

    def forward(self, x):
        with recording(self.ops, VIT_OPS) as rec, torch.no_grad():
            tok = self.model.model.forward_tokens(x).clone()
        torch.cuda.synchronize()
        return rec, tok

    def restate(self, *calib, margin=None):
        R = fw.Restatement(self.sd, self.depth, [self.acts[k] for k in calib], margin)
        assert R.input_condition() == [], R.input_condition()
        return R


def plan_mismatches(plan, R):
    """Where the plan's weights, row scales, activation scales and column scales leave the restatement."""
    bad = []
    for i, (pb, rb) in enumerate(zip(plan.blocks, R.blocks)):
        for pt in fw.POINTS:
            got, want = pb.get("s_" + pt), rb["s_" + pt]
            if got is None or abs(got - want) > 1e-12 * want:
                bad.append(f"block {i} s_{pt}: {got} vs {want}")
        for lin in fw.LINEARS:
            if not torch.equal(pb[lin + "_w8"].view(torch.uint8), rb[lin + "_w8"].view(torch.uint8)):
                bad.append(f"block {i} {lin}_w8 is not bit-equal")
            for key, tol in (("_sw", 2.0 ** -23), ("_cs", 2.0 ** -22)):
                want = rb[lin + key].double()
                got = pb.get(lin + key)
                rel = float(((got.double() - want).abs() / want).max()) if got is not None else float("inf")
                if not rel <= tol:
                    bad.append(f"block {i} {lin}{key}: off by {rel:.3e} relative (bound {tol:.3e})")
    return bad


def plan_numbers(plan):
    return [(b["s_" + pt], b[lin + "_cs"].clone()) for b in plan.blocks for pt, lin in
            (("h1", "qkv"), ("ao", "proj"), ("h2", "fc1"), ("hid", "fc2"))]


@pytest.mark.parametrize("name,fp8_proj", CASES, ids=CASE_IDS)
def test_calibration_matches_restatement(ops, monkeypatch, name, fp8_proj):
    from probpose_pytorch_amd import engine
    monkeypatch.setattr(engine, "FP8_PROJ", fp8_proj)
    rig = Rig(ops, name)
    with torch.no_grad():
        rig.model.model.forward_tokens(rig.xs["x1"])          # the first forward calibrates on its own batch
    assert rig.plan.fp8 and rig.plan.fp8_calibrated
    bad = plan_mismatches(rig.plan, rig.restate("x1"))
    assert not bad, "\n".join(bad)
    implicit = plan_numbers(rig.plan)
    rig.model.model.calibrate_fp8([rig.xs["x1"]])
    for (s0, c0), (s1, c1) in zip(implicit, plan_numbers(rig.plan)):
        assert s0 == s1 and torch.equal(c0, c1), "calibrate([x]) differs from the first forward's own calibration"


@pytest.mark.parametrize("name", list(fw.MODELS))
def test_recalibration_running_maximum_reset_and_margin(ops, name):
    rig = Rig(ops, name)
    R1, R2, R12 = rig.restate("x1"), rig.restate("x2"), rig.restate("x1", "x2")
    # the check means something only if each batch holds the maximum somewhere
    s = lambda R: [b["s_" + pt] for b in R.blocks for pt in fw.POINTS]  # noqa: E731
    assert any(a > b for a, b in zip(s(R1), s(R2))) and any(a < b for a, b in zip(s(R1), s(R2)))
    x1, x2 = rig.xs["x1"], rig.xs["x2"]
    rig.model.model.calibrate_fp8([x1, x2])
    bad = plan_mismatches(rig.plan, R12)
    assert not bad, "calibrate([x1, x2]) is not the maximum over both batches:\n" + "\n".join(bad)
    rig.model.model.calibrate_fp8([x2, x1])
    bad = plan_mismatches(rig.plan, R12)
    assert not bad, "calibrate([x2, x1]) is not the maximum over both batches:\n" + "\n".join(bad)
    rig.model.model.calibrate_fp8([x1])
    bad = plan_mismatches(rig.plan, R1)
    assert not bad, "a second calibrate([x1]) did not forget x2:\n" + "\n".join(bad)
    rig.model.model.calibrate_fp8([x1, x2], margin=1.5)
    bad = plan_mismatches(rig.plan, rig.restate("x1", "x2", margin=1.5))
    assert not bad, "margin=1.5 did not reach every s and cs:\n" + "\n".join(bad)
    rig.model.model.calibrate_fp8([x2])
    bad = plan_mismatches(rig.plan, R2)
    assert not bad, "calibrate([x2]) after a margin of 1.5 is not the default-margin calibration:\n" + "\n".join(bad)


def _distance(a, b):
    d = (a.double() - b.double()).abs()
    return f"mean |d| {float(d.mean()):.4f} max |d| {float(d.max()):.3f} (rms of the reference {float(b.double().square().mean().sqrt()):.3f})"


@pytest.mark.parametrize("name,fp8_proj", CASES, ids=CASE_IDS)
def test_walk_sequence_scales_dataflow_and_stage_values(ops, monkeypatch, name, fp8_proj):
    from probpose_pytorch_amd import engine
    monkeypatch.setattr(engine, "FP8_PROJ", fp8_proj)
    rig = Rig(ops, name)
    R = rig.restate("x1", "x2")
    rig.model.model.calibrate_fp8([rig.xs["x1"], rig.xs["x2"]])
    rec, tok = rig.forward(rig.xs["x1"])
    rep = fw.check_walk(rec, R, fp8_proj)
    print(f"\n[{name} FP8_PROJ={fp8_proj}] B = {rig.cfg['B']}\n{rep.summary()}")
    assert rep.ok, str(rep)
    # a smaller batch right after: its e4m3 twins are the leading rows of the larger batch's workspace
    rec_s, _ = rig.forward(rig.xs["x2"][:rig.small].contiguous())
    assert rec_s[1]["ptrs"]["out"] == rec[1]["ptrs"]["out"] and rec_s[1]["out"].shape[0] < rec[1]["out"].shape[0]
    rep_s = fw.check_walk(rec_s, R, fp8_proj)
    print(f"[{name} FP8_PROJ={fp8_proj}] B = {rig.small} after B = {rig.cfg['B']}\n{rep_s.summary()}")
    assert rep_s.ok, str(rep_s)
    # the flag toggled after calibration: s_ao / proj_cs exist either way and must be the same restated values
    monkeypatch.setattr(engine, "FP8_PROJ", not fp8_proj)
    rec_t, _ = rig.forward(rig.xs["x1"])
    rep_t = fw.check_walk(rec_t, R, not fp8_proj)
    assert rep_t.ok, f"FP8_PROJ toggled to {not fp8_proj} after calibration:\n{rep_t}"
    # free-running distances: reported, never asserted (see the module docstring)
    free = fw.EmulatedPlan(rig.sd, rig.cfg, exact=True).adopt(R).walk(rig.xs["x1"], fp8=True, fp8_proj=fp8_proj)[-1]["out"]
    print(f"[{name} FP8_PROJ={fp8_proj}] free-running: fp8 forward vs float64 walk quantised at the same points: "
          f"{_distance(tok, free)}\n{'':27s}fp8 forward vs bf16 forward: {_distance(tok, rig.bf16_tokens['x1'])}")


@pytest.mark.parametrize("name,fp8_proj", CASES, ids=CASE_IDS)
def test_saturation_on_a_batch_brighter_than_the_calibration(ops, monkeypatch, name, fp8_proj):
    from probpose_pytorch_amd import engine
    monkeypatch.setattr(engine, "FP8_PROJ", fp8_proj)
    rig = Rig(ops, name)
    R = rig.restate("flat")
    rig.model.model.calibrate_fp8([rig.xs["flat"]])
    rec, tok = rig.forward(rig.xs["bright"])
    sat = fw.saturation(rec)
    print(f"\n[{name} FP8_PROJ={fp8_proj}] {sat}")
    assert sat["nan"] == 0 and sat["saturated"] > 0, sat          # a saturated element stores exactly +-448 (0x7E / 0xFE)
    assert bool(torch.isfinite(tok.float()).all())
    for e in rec:
        if e["out"].dtype == FP8:
            assert float(e["out"].float().abs().max()) <= 448.0
    rep = fw.check_walk(rec, R, fp8_proj)
    print(rep.summary())
    assert rep.ok, str(rep)


def test_e4m3_producers_write_nothing_outside_their_output(ops, monkeypatch):
    """LayerNorm -> e4m3, attention -> e4m3 and fc1 (GELU, e4m3 out) at model A's shapes, each into a NaN-filled
    buffer with guards on both sides, on the inputs and scales of a recorded walk."""
    from probpose_pytorch_amd import engine
    monkeypatch.setattr(engine, "FP8_PROJ", True)
    rig = Rig(ops, "A")
    R = rig.restate("x1")
    rig.model.model.calibrate_fp8([rig.xs["x1"]])
    rec, _ = rig.forward(rig.xs["x1"])
    by = {r: e for e, r in zip(rec, fw.roles(rig.depth))}
    b = R.blocks[0]
    lead, tail = 256, 1024
    for role in ("ln1", "attention", "fc1"):
        e = by[(role, 0)]
        a, sc = e["args"], e["scalars"]
        n = e["out"].numel()
        buf = gr.nan_like_bits(lead + n + tail, FP8, "cuda")
        before = buf.clone()
        out = buf[lead:lead + n].view(e["out"].shape)
        assert out.data_ptr() % 16 == 0
        if role == "ln1":
            ops.layernorm(a["x"], a["gamma"], a["beta"], sc["eps"], out, out_scale=b["s_h1"])
        elif role == "attention":
            ops.attention(a["qkv"], out, sc["B"], sc["N"], sc["heads"], sc["hd"], out_scale=b["s_ao"])
        else:
            ops.linear(a["x"], a["w"], a["bias"], out=out, epilogue=sc["epilogue"], colscale=a["colscale"],
                       out_scale=b["s_hid"])
        torch.cuda.synchronize()
        u8, b8 = buf.view(torch.uint8), before.view(torch.uint8)
        assert torch.equal(u8[:lead], b8[:lead]) and torch.equal(u8[lead + n:], b8[lead + n:]), f"{role}: a guard changed"
        assert int(((u8[lead:lead + n] & 0x7F) == 0x7F).sum()) == 0, f"{role}: an output element was left unwritten"
        assert torch.equal(out.view(torch.uint8), e["out"].view(torch.uint8)), f"{role}: differs from the walk's launch"
