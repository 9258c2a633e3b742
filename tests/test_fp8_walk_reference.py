"""The fp8 walk restatement on the CPU (tests/fp8_walk_reference.py): the comparator accepts the torch emulation of
the walk for both FP8_PROJ settings and rejects each planted bookkeeping fault, ops.quantize_rows_fp8 has the
properties the restatement states, and the model states the GPU test uses meet the input condition.

The synthetic ViT state gives LN1 and LN2 outputs of one amax and weight rows of nearly one scale, so the states here
are conditioned (fp8_walk_reference.condition_state: LN2 gamma x 0.5, fc1 weight x 4, the v rows of qkv x 0.3, every 16th row of each
linear x 0.25; proj x 0.25 and fc2 x 0.05 keep each block's update small against the stream); the condition (activation scales >= 5 % apart, row scales spread >= 2x) is asserted on
the float64 side."""
import pytest
import torch

from tests import fp8_walk_reference as fw

FP8 = fw.FP8
MODELS, model_state, batches = fw.MODELS, fw.model_state, fw.batches       # the GPU test's models and batches


def restate(sd, cfg, calib, margin=None):
    """The restatement from a fault-free bf16 emulation of the calibration batches."""
    clean = fw.EmulatedPlan(sd, cfg)
    acts = [fw.activations(clean.walk(x, fp8=False), cfg["depth"]) for x in calib]
    return fw.Restatement(sd, cfg["depth"], acts, margin)


@pytest.fixture(scope="module")
def setup():
    out = {}
    for name, cfg in MODELS.items():
        out[name] = (cfg, model_state(cfg), batches(cfg))
    return out


@pytest.mark.parametrize("name", list(MODELS))
def test_chosen_states_meet_the_input_condition(setup, name):
    cfg, sd, xs = setup[name]
    for calib in (["x1"], ["x1", "x2"], ["flat"], ["flat", "bright"]):
        R = restate(sd, cfg, [xs[k] for k in calib])
        assert R.input_condition() == [], (calib, R.input_condition())
        for i, b in enumerate(R.blocks):
            print(f"  {name} {calib} block {i}: s " + " ".join(f"{p} {b['s_' + p]:.4g}" for p in fw.POINTS))


@pytest.mark.parametrize("fp8_proj", [False, True], ids=["proj_bf16", "proj_fp8"])
@pytest.mark.parametrize("name", list(MODELS))
def test_comparator_accepts_the_emulation(setup, name, fp8_proj):
    cfg, sd, xs = setup[name]
    R = restate(sd, cfg, [xs["x1"], xs["x2"]])
    plan = fw.EmulatedPlan(sd, cfg).calibrate([xs["x1"], xs["x2"]])
    rec = plan.walk(xs["x1"], fp8=True, fp8_proj=fp8_proj)
    rep = fw.check_walk(rec, R, fp8_proj)
    print(f"\n[{name} FP8_PROJ={fp8_proj}]\n{rep.summary()}")
    assert rep.ok, str(rep)
    small = plan.walk(xs["x2"][:2], fp8=True, fp8_proj=fp8_proj)       # a smaller batch after a larger one
    rep = fw.check_walk(small, R, fp8_proj)
    assert rep.ok, str(rep)
    # a saturating batch: calibrated flat, run black / white; the clamped restatement still holds
    Rf = restate(sd, cfg, [xs["flat"]])
    rec = fw.EmulatedPlan(sd, cfg).calibrate([xs["flat"]]).walk(xs["bright"], fp8=True, fp8_proj=fp8_proj)
    sat = fw.saturation(rec)
    assert sat["nan"] == 0 and sat["saturated"] > 0, sat
    rep = fw.check_walk(rec, Rf, fp8_proj)
    assert rep.ok, str(rep)


# fault -> (calibrations the plan runs in order, batch of the forward, what the restatement is calibrated on, FP8_PROJ,
#           tags the comparator must raise)
SCENARIOS = {
    "swap_s_h1_s_h2": ([["x1"]], "x1", ["x1"], False, {"scale", "value"}),
    "cs_without_sw": ([["x1"]], "x1", ["x1"], False, {"scale", "value"}),
    "cs_from_previous_amax": ([["bright"], ["flat"]], "flat", ["flat"], False, {"scale", "value"}),
    "margin_1": ([["x1"]], "x1", ["x1"], False, {"scale", "value"}),
    "margin_twice": ([["x1"]], "x1", ["x1"], False, {"scale", "value"}),
    "last_batch_amax": ([["bright", "flat"]], "flat", ["bright", "flat"], False, {"scale", "value"}),
    "calibrate_keeps_old_max": ([["bright"], ["flat"]], "flat", ["flat"], False, {"scale", "value"}),
    "fc2_reads_other_rows": ([["x1"]], "x1", ["x1"], False, {"dataflow"}),
    "no_clamp": ([["flat"]], "bright", ["flat"], False, {"value"}),
    "proj_gets_s_ao_after_bf16_attention": ([["x1"]], "x1", ["x1"], False, {"scale", "weight", "dataflow"}),
}


def test_every_fault_has_a_scenario():
    assert set(SCENARIOS) == set(fw.FAULTS)


@pytest.mark.parametrize("fault", list(fw.FAULTS))
def test_comparator_rejects_planted_fault(setup, fault):
    cfg, sd, xs = setup["A"]
    calibs, run, restated, fp8_proj, tags = SCENARIOS[fault]
    R = restate(sd, cfg, [xs[k] for k in restated])
    assert R.input_condition() == []
    for planted in (None, fault):
        plan = fw.EmulatedPlan(sd, cfg, fault=planted)
        for c in calibs:
            plan.calibrate([xs[k] for k in c])
        if fault == "fc2_reads_other_rows":
            plan.walk(xs[run], fp8=True, fp8_proj=fp8_proj)
            rec = plan.walk(xs[run][:3], fp8=True, fp8_proj=fp8_proj)      # B = 3 right after B = 5
        else:
            rec = plan.walk(xs[run], fp8=True, fp8_proj=fp8_proj)
        rep = fw.check_walk(rec, R, fp8_proj)
        if planted is None:
            assert rep.ok, f"the scenario fails without the fault: {rep}"
        else:
            print(f"\n[{fault}] {len(rep.failures)} findings, tags {sorted(rep.tags())}; first: {rep.failures[:1]}")
            assert not rep.ok and tags <= rep.tags(), (sorted(rep.tags()), str(rep)[:2000])


# ---------------------------------------------------------------------------------------------------------------
# ops.quantize_rows_fp8
# ---------------------------------------------------------------------------------------------------------------
def _rows():
    g = torch.Generator().manual_seed(1)
    rand = torch.randn((48, 256), generator=g) * torch.logspace(-6, 3, 48)[:, None]
    zero = torch.randn((5, 128), generator=g)
    zero[2] = 0
    huge = torch.zeros((3, 128))
    huge[0, 7], huge[1, 0], huge[2, 127] = 3e38, -1e30, 6e4
    huge[1, 5] = 1e-30
    # sw = 1 exactly (amax 448): every other element sits on the midpoint of two neighbouring e4m3 values, in every
    # binade and in the subnormal range; round-to-nearest-even decides each of them
    grid = torch.arange(0, 256, dtype=torch.uint8).view(FP8).float()
    grid = grid[:0x7F]                                                 # 0 ... 448, ascending
    mid = (grid[:-1].double() + grid[1:].double()) / 2
    mid = torch.cat([mid, -mid, torch.tensor([448.0])]).float()[None, :].repeat(2, 1)
    mid[1] *= 0.5                                                     # sw = 0.5: still exact
    mid[1, -1] = 224.0
    return dict(random=rand, zero_row=zero, one_huge_element=huge, midpoints=mid)


@pytest.mark.parametrize("kind", ["random", "zero_row", "one_huge_element", "midpoints"])
def test_quantize_rows_fp8_properties(kind):
    from probpose_pytorch_amd import ops
    w = _rows()[kind]
    w8, sw = ops.quantize_rows_fp8(w)
    assert w8.dtype == FP8 and sw.dtype == torch.float32 and w8.shape == w.shape and sw.shape == (w.shape[0],)
    assert fw.check_quantized_rows(w, w8, sw) == []
    r8, rs = fw.quantize_rows(w)
    assert torch.equal(w8.view(torch.uint8), r8.view(torch.uint8))
    assert float(((sw.double() - rs.double()).abs() / rs.double()).max()) <= 2.0 ** -23
    if kind == "zero_row":
        assert bool((w8[2].float() == 0).all()) and float(sw[2]) == pytest.approx(1e-12 / 448, rel=1e-6)
    if kind == "midpoints":
        # ties go to the even mantissa: the stored byte of every midpoint is even
        assert float(sw[0]) == 1.0 and float(sw[1]) == 0.5
        assert bool((w8[:, :-1].view(torch.uint8) & 1 == 0).all())
        y = w.double() / sw.double()[:, None]
        assert bool(((w8.float().double() - y).abs()[:, :-1] == fw.half_step(y)[:, :-1]).all())


def test_property_checker_rejects_wrong_quantisations():
    w = _rows()["random"]
    w8, sw = fw.quantize_rows(w)
    assert fw.check_quantized_rows(w, w8, sw * 1.01) != []
    trunc = (w8.view(torch.uint8) & 0xFE).view(FP8)                   # round towards zero in place of nearest
    assert fw.check_quantized_rows(w, trunc, sw) != []
    assert fw.check_quantized_rows(w, fw.e4m3(w8.float() * 0.5), sw * 2) != []       # amax no longer at 448


def test_e4m3_clamps_before_the_cast():
    t = torch.tensor([460.0, 470.0, -1e4, 1e30])
    assert bool(torch.isnan(t.to(FP8).float()[1:]).all())             # torch's cast alone: NaN above 464
    assert fw.e4m3(t).float().tolist() == [448.0, 448.0, -448.0, 448.0]
