"""CPU checks of the float64 loss restatement (tests/loss_reference.py) against tests/golden/loss.npz, minted from the
unmodified reference (tests/golden/make_goldens_loss.py), and of its comparator against planted faults."""
import os

import numpy as np
import pytest

from tests import loss_reference as LR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss.npz")
# golden tag -> (input case, freeze_error, keypoint weights, learn_heatmaps_from_zeros)
PROBPOSE_CASES = {"G1": ("G1", True, False, False), "G2": ("G1", False, True, True), "G3": ("G3", True, False, False),
                  "G3e": ("G3", False, False, False)}
LOSS_KEYS = ("kpt", "probability", "visibility", "oks", "error")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def restate(g, tag, fault=None, nan_gt=False):
    case, freeze, use_kw, zeros = PROBPOSE_CASES[tag]
    inp = LR.case_inputs(case)
    gt_kpts = g[f"{tag}_gt_kpts"].copy()
    if nan_gt:
        # the reference decodes G3's all-zero map to (0, 0): a decoder that returns NaN there instead must give the
        # same OKS targets once NaN is zeroed (loss.py:588)
        assert (gt_kpts[1, 3] == 0).all()
        gt_kpts[1, 3] = np.nan
    return LR.probpose_loss(inp["gt"], inp["pred"], gt_kpts, g[f"{tag}_dt_kpts"], inp["sigmas"],
                            freeze_error=freeze, keypoint_weights=inp["keypoint_weights"] if use_kw else None,
                            learn_heatmaps_from_zeros=zeros, fault=fault)


def probpose_ratios(g, tag, R):
    """d/bound of every quantity the golden holds for one ProbPoseLoss case."""
    q = {k: LR.ratio(g[f"{tag}_loss_{k}"], *R[k]) for k in LOSS_KEYS}
    for k in ("gt_oks", "gt_err", "vis_weight"):
        B, K = g[f"{tag}_gt_kpts"].shape[:2]
        q[k] = LR.ratio(g[f"{tag}_{k}"].reshape(B, K), *R[k])
    q["mae_oks"] = LR.ratio(g[f"{tag}_acc_oks"], *R["mae_oks"])
    q["mae_err"] = LR.ratio(g[f"{tag}_acc_error"], *R["mae_err"])
    return q


@pytest.mark.parametrize("case", ["G1", "G3"])
def test_inputs_are_the_reference_maps(golden, case):
    inp = LR.case_inputs(case)
    for tag in [t for t, c in PROBPOSE_CASES.items() if c[0] == case]:
        assert LR.sha(inp["gt"]["heatmaps"]) == str(golden[f"{tag}_gt_hm_sha"])
        assert LR.sha(inp["pred"][0]) == str(golden[f"{tag}_dt_hm_sha"])


def test_golden_cases_cover_the_quirks(golden):
    # G3: the all-zero gt channel of an annotated in-image keypoint decodes to (0, 0) in the reference, and crop 2
    # has no annotated keypoint (oks_weight = 0: its OKS targets are all zero)
    assert (golden["G3_gt_kpts"][1, 3] == 0).all()
    assert (golden["G3_gt_oks"].reshape(4, 20)[2] == 0).all()
    inp = LR.case_inputs("G3")
    assert not inp["gt"]["keypoints_visible"][2].any() and inp["gt"]["in_image"][1, 0, 3]
    g1 = LR.case_inputs("G1")["gt"]
    assert (~g1["in_image"]).any() and (~g1["keypoints_visible"]).any()
    assert np.isfinite(golden["G3e_gt_err"]).all()


@pytest.mark.parametrize("tag", list(PROBPOSE_CASES))
def test_probpose_restatement_reproduces_reference(golden, tag):
    R = restate(golden, tag)
    q = probpose_ratios(golden, tag, R)
    assert max(q.values()) <= 1.0, q


def test_nan_gt_coordinate_is_zeroed(golden):
    q = probpose_ratios(golden, "G3", restate(golden, "G3", nan_gt=True))
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("i", range(len(LR.heatmap_options())))
def test_oks_heatmap_restatement_reproduces_reference(golden, i):
    hi = LR.heatmap_case_inputs()
    ot, skip, wk, mk, sw, gw, lw = LR.heatmap_options()[i]
    R = LR.oks_heatmap_loss(hi["output"], hi["target"], hi[wk] if wk else None, hi[mk] if mk else None, skip, ot,
                            sw, gw, lw)
    for red in ("pixel", "keypoint", "mean"):
        LR.assert_within(golden[f"hm{i}_{red}"], *R[red], what=f"hm{i} {red}")


def test_small_losses_restatement_reproduces_reference(golden):
    S = LR.small_inputs()
    for sig in (True, False):
        for red in ("mean", "sum", "none"):
            for wn in ("none", "w1", "w2"):
                R = LR.bce_loss(S["x"] if sig else S["logits"], S["y"], None if wn == "none" else S[wn], sig,
                                wn != "none", red, 1.5)
                LR.assert_within(golden[f"bce_{int(sig)}_{red}_{wn}"], *R, what=f"bce {sig} {red} {wn}")
    LR.assert_within(golden["mse_w"], *LR.mse_loss(S["a"], S["b"], S["wm"], True), what="mse_w")
    LR.assert_within(golden["mse_now"], *LR.mse_loss(S["a"], S["b"], loss_weight=0.7), what="mse_now")
    for D in (1, 2):
        LR.assert_within(golden[f"l1log_D{D}"], *LR.l1log_loss(S[f"eo{D}"], S[f"et{D}"], S[f"wl{D}"], True),
                         what=f"l1log D{D}")
        LR.assert_within(golden[f"l1log_D{D}_now"], *LR.l1log_loss(S[f"eo{D}"], S[f"et{D}"]), what=f"l1log D{D}")


# ----------------------------------------------------------------------------------------------- planted faults
@pytest.mark.parametrize("fault,tag,key", [
    ("reflect", "G1", "kpt"),               # Sobel with reflect instead of zero padding
    ("drop_weights", "G2", "kpt"),          # the keypoint mask of the heatmap loss dropped
    ("unnormalised_vis", "G1", "vis_weight"),
    ("nan_gt", "G3", "gt_oks"),             # a NaN gt coordinate not zeroed
])
def test_comparator_rejects_planted_fault(golden, fault, tag, key):
    q = probpose_ratios(golden, tag, restate(golden, tag, fault, nan_gt=fault == "nan_gt"))
    assert q[key] > 1.0, q


def test_comparator_rejects_planted_faults_in_the_heatmap_loss(golden):
    hi = LR.heatmap_case_inputs()
    ot, skip, wk, mk, sw, gw, lw = LR.heatmap_options()[2]      # minus, keypoint weights, no mask
    assert wk == "w2" and mk is None
    for fault in ("reflect", "drop_weights"):
        R = LR.oks_heatmap_loss(hi["output"], hi["target"], hi[wk], None, skip, ot, sw, gw, lw, fault=fault)
        assert LR.ratio(golden["hm2_pixel"], *R["pixel"]) > 1.0, fault
        assert LR.ratio(golden["hm2_mean"], *R["mean"]) > 1.0, fault


def test_comparator_rejects_log1p_in_l1log(golden):
    """log1p(x) in place of log(1 + x) in float32: visible where the operands are small (the G cases' losses are
    dominated by errors of tens of pixels, where the difference is far below rounding)."""
    S = LR.small_inputs()
    for D in (1, 2):
        R = LR.l1log_loss(S[f"eo{D}"], S[f"et{D}"], S[f"wl{D}"], True, fault="log1p")
        assert LR.ratio(golden[f"l1log_D{D}"], *R) > 1.0
