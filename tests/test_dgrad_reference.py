"""The training step's pp_gemm calls pinned on the CPU, before any kernel runs: for every builder of
tests/dgrad_reference.py and every case, the float64 restatement of pp_gemm (tests/gemm_reference.py) on the call the
product's packers and tables form equals torch's float64 autograd result of the layer itself, bit for bit on integer
data in [-3, 3] (bf16 and f32 operand storage), and every planted packer fault makes that comparison fail."""
import pytest
import torch

from tests import dgrad_reference as DR

DTYPES = [torch.bfloat16, torch.float32]
F64_TOL = 1e-12        # relative to the largest element: float64 sums of at most a few thousand terms


def _tag(dt):
    return str(dt).replace("torch.", "")


@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("kind", DR.KINDS)
def test_restatement_equals_autograd_on_integer_data(kind, dt):
    for i, case in enumerate(DR.CASES[kind]):
        call = DR.make(kind, case, dt, True, seed=i)
        ref, written = DR.restated(call)
        assert bool(written.all()), (kind, case)
        assert float(call.truth.abs().max()) > 0, (kind, case)
        assert torch.equal(ref, call.truth), (kind, case, float((ref - call.truth).abs().max()))
        if call.kw["out"].dtype == torch.bfloat16:      # the one bf16 output: every result is a bf16 number
            assert float(call.truth.abs().max()) <= 256 and torch.equal(call.truth.bfloat16().double(), call.truth)


@pytest.mark.parametrize("kind", DR.KINDS)
def test_restatement_agrees_with_autograd_on_normal_data(kind):
    case = DR.CASES[kind][1]
    call = DR.make(kind, case, torch.bfloat16, False, seed=7)
    ref, written = DR.restated(call)
    assert bool(written.all())
    assert float((ref - call.truth).abs().max()) <= F64_TOL * float(call.truth.abs().max()), (kind, case)


def test_in_place_residual_call_is_built_in_place():
    call = DR.make("aux0_resid", DR.CASES["aux0_resid"][0], torch.float32, True)
    assert call.in_place and call.kw["residual"] is call.kw["out"]
    plain = DR.make("aux0", DR.CASES["aux0"][0], torch.float32, True)
    assert not plain.in_place and "residual" not in plain.kw
    resid = DR.make("fwd_resid", DR.CASES["fwd_resid"][0], torch.float32, True)
    assert not resid.in_place and resid.kw["residual"] is not resid.kw["out"]


def test_deconv_case_with_one_pixel_has_twelve_taps_out_of_the_map():
    call = DR.make("deconv", (1, 1, 1, 8, 64), torch.float32, True)
    assert int((call.kw["rowoff"] < 0).sum()) == 12 and call.kw["rowoff"].numel() == 16


FAULT_PARAMS = [(name, kind) for name, f in DR.FAULTS.items() for kind in f[4]]


@pytest.mark.parametrize("dt", DTYPES, ids=_tag)
@pytest.mark.parametrize("name,kind", FAULT_PARAMS, ids=[f"{n}-{k}" for n, k in FAULT_PARAMS])
def test_planted_fault_fails_the_comparison(name, kind, dt):
    case = DR.FAULT_CASES[kind]
    assert DR.equals_truth(DR.make(kind, case, dt, True, seed=3)), "the case itself must pass"
    with DR.planted(name):
        bad = DR.make(kind, case, dt, True, seed=3)
    assert not DR.equals_truth(bad), (name, kind)
    # and the packer is the product's again
    assert DR.equals_truth(DR.make(kind, case, dt, True, seed=3))


def test_every_issue_fault_is_listed():
    for name in ("conv3x3 taps not flipped", "conv3x3 ky and kx swapped", "deconv ky and kx swapped",
                 "conv3x3 Cin and Cout swapped", "deconv Cin and Cout swapped", "deconv table pad off by one",
                 "deconv table -1 as offset 0", "conv table -1 as offset 0", "aux-0 table -1 as offset 0",
                 "aux-0 branch order reversed", "_wt not transposed"):
        assert name in DR.FAULTS
    # a missing flip cannot be seen on a 1 x 1 map (only the centre tap is in range): the fault cases are larger
    with DR.planted("conv3x3 taps not flipped"):
        assert DR.equals_truth(DR.make("aux_stage", (2, 1, 1, 64), torch.float32, True))
    for kind, case in DR.FAULT_CASES.items():
        if kind != "proj_dgrad":
            geo = case[0] if kind.startswith("aux0") else case
            assert geo[1] >= 2 and geo[2] >= 2


def test_every_head_descriptor_the_builders_use_has_a_planted_fault():
    """The builders take their dimension keywords from head_calls: a wrong descriptor must fail the comparison, or
    the tests would hold the product to itself."""
    from probpose_pytorch_amd import head_calls
    planted = {f[1]: f[4] for f in DR.FAULTS.values() if f[0] is head_calls}
    assert planted == {"final_dgrad": ("final",), "deconv_dgrad": ("deconv",), "aux_stage": ("aux_stage",),
                       "aux0_dgrad": ("aux0", "aux0_resid")}
