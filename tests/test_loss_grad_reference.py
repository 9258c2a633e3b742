"""CPU checks of tests/loss_grad_reference.py: the float64 gradient restatement against the reference's own gradients
(tests/golden/loss_grad.npz) and against torch autograd in float64, and its comparator against planted kernel faults."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_grad_reference as LG
from tests import loss_reference as LR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "loss_grad.npz")
GOLDEN_FWD = os.path.join(HERE, "golden", "loss.npz")
CASES = {"G1": ("G1", True, False, False), "G2": ("G1", False, True, True), "G3": ("G3", True, False, False),
         "G3e": ("G3", False, False, False)}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def golden_fwd():
    return np.load(GOLDEN_FWD)


def tie_map(H, W, r=1, c=1):
    """A map whose masked Sobel energy has exactly two maxima (6.5 at (r-1, c+1) and (r+1, c+1)), all values powers of
    two, so every energy is exact in float32."""
    o = np.zeros((H, W), np.float32)
    o[r, c], o[r, c + 1] = 0.5, 1.0
    return o


# ----------------------------------------------------------------------------------------------- float64 autograd
def torch_heatmap_loss(o, t, w, mask, skip, ot, sw, gw, lw):
    """loss.py:55-191 in torch float64: returns (per-pixel, per-keypoint, mean) of the leaf ``o``."""
    B, K, H, W = o.shape
    m = None
    if mask is not None:
        m = torch.tensor(mask, dtype=torch.float64)
    if w is not None:
        ww = torch.tensor(w, dtype=torch.float64)
        ww = ww.view(ww.shape + (1,) * (4 - ww.ndim))
        m = ww if m is None else m * ww
    if skip:
        ne = (t != 0).flatten(2).any(dim=2)[..., None, None].double()
        m = ne if m is None else m * ne
    om, op = o * (1 - t), (1 - o) * t
    oks = {"minus": om, "plus": op, "both": (om + op) / 2}[ot]
    mse = (o - t) ** 2
    sx = torch.tensor(LG.SOBEL_X).view(1, 1, 3, 3)
    sy = torch.tensor(LG.SOBEL_Y).view(1, 1, 3, 3)
    x = o.reshape(B * K, 1, H, W)
    g = (F.conv2d(x, sx, padding="same") ** 2 + F.conv2d(x, sy, padding="same") ** 2).reshape(B, K, H, W)
    if m is not None:
        oks, mse, g = oks * m, mse * m, g * m
    ow = 1 - sw - gw
    pix = (sw * g + ow * oks + gw * mse) * lw
    kp = (ow * oks.sum(dim=(2, 3)) + sw * g.reshape(B, K, -1).max(dim=-1)[0] + gw * mse.mean(dim=(2, 3))) * lw
    return pix, kp, kp.mean()


def test_heatmap_grad_matches_torch_float64_autograd():
    hi = LR.heatmap_case_inputs()
    B, K, H, W = hi["output"].shape
    worst = 0.0
    for i, (ot, skip, wk, mk, sw, gw, lw) in enumerate(LR.heatmap_options()):
        rng = np.random.default_rng(i)
        args = (hi["output"], hi["target"], hi[wk] if wk else None, hi[mk] if mk else None, skip, ot, sw, gw, lw)
        for red, u in (("pixel", rng.normal(size=(B, K, H, W))), ("keypoint", rng.normal(size=(B, K))),
                       ("mean", 1.7), ("pixel_mean", 0.9)):
            o = torch.tensor(hi["output"], dtype=torch.float64, requires_grad=True)
            pix, kp, mean = torch_heatmap_loss(o, torch.tensor(hi["target"], dtype=torch.float64), *args[2:])
            L = {"pixel": lambda: (pix * torch.tensor(u)).sum(), "keypoint": lambda: (kp * torch.tensor(u)).sum(),
                 "mean": lambda: mean * u, "pixel_mean": lambda: pix.mean() * u}[red]()
            L.backward()
            v, mag, _ = LG.oks_heatmap_loss_grad(*args, reduction=red, upstream=u)
            assert np.all(np.abs(v - o.grad.numpy()) <= 1e-12 * (mag + 1e-300)), (i, red)
            worst = max(worst, float(np.abs(v - o.grad.numpy()).max()))
    assert worst < 1e-12


def _torch_heads(inp, gt_oks, gt_err, upstream):
    """The four small losses of ProbPoseLoss in torch float64 (1 + x rounded to float32 as the reference's float32
    log(1 + x) sees it), differentiated by autograd."""
    B, K = inp["B"], inp["K"]
    gt = inp["gt"]
    probs = torch.tensor(np.asarray(gt["in_image"]).reshape(B, K).astype(np.float64))
    ann = np.asarray(gt["keypoints_visible"]).reshape(B, K).astype(np.int64)
    vis = torch.tensor(np.asarray(gt["keypoints_visibility"]).reshape(B, K).astype(np.float64))
    w = torch.tensor((ann & (probs.numpy() > 0.5)).astype(np.float64))
    x = [torch.tensor(p.reshape(B, K).astype(np.float64), requires_grad=True) for p in inp["pred"][1:]]
    loss = upstream["probability"] * F.binary_cross_entropy(x[0], probs)
    loss = loss + upstream["visibility"] * F.binary_cross_entropy(x[1], vis)
    loss = loss + upstream["oks"] * F.mse_loss(x[2] * w, torch.tensor(gt_oks, dtype=torch.float64) * w)

    def log1x(v, v32):
        delta = torch.tensor((np.float32(1) + v32).astype(np.float64)) - (1 + v.detach())
        return torch.log(1 + v + delta)
    la = log1x(x[3], inp["pred"][4].reshape(B, K))
    lb = torch.log(torch.tensor((np.float32(1) + gt_err).astype(np.float64)))
    loss = loss + upstream["error"] * F.smooth_l1_loss(la * w, lb * w)
    loss.backward()
    return [t.grad.numpy() for t in x]


@pytest.mark.parametrize("tag", list(CASES))
def test_head_grads_match_torch_float64_autograd(golden_fwd, tag):
    case, freeze, use_kw, zeros = CASES[tag]
    inp = LR.case_inputs(case)
    gt_oks = golden_fwd[f"{tag}_gt_oks"].astype(np.float32)
    gt_err = golden_fwd[f"{tag}_gt_err"].astype(np.float32)
    for up in ({"kpt": 1.0, "probability": 0.7, "visibility": -1.3, "oks": 2.0, "error": 0.4}, LG.LOSS_WEIGHTS):
        want = _torch_heads(inp, gt_oks, gt_err, up)
        R = LG.probpose_loss_grads(inp["gt"], inp["pred"], gt_oks, gt_err, inp["keypoint_weights"] if use_kw else None,
                                   zeros, up)
        for key, w in zip(LG.PRED_KEYS[1:], want):
            v, mag, _ = R[key]
            assert np.all(np.abs(v - w) <= 1e-12 * (mag + 1e-300)), (tag, key)


# ----------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("tag", list(CASES))
def test_probpose_grads_against_reference_goldens(golden, golden_fwd, tag):
    """The reference's float32 autograd gradients lie within twice the restatement's bound (its own float32
    rounding plus the kernel's), for each loss alone and for train.py's weighted sum."""
    case, freeze, use_kw, zeros = CASES[tag]
    inp = LR.case_inputs(case)
    B, K, H, W = inp["B"], inp["K"], inp["H"], inp["W"]
    gt_oks = golden_fwd[f"{tag}_gt_oks"].astype(np.float32)      # the reference's float32 targets
    gt_err = golden_fwd[f"{tag}_gt_err"].astype(np.float32)
    kw = inp["keypoint_weights"] if use_kw else None
    for name in (*LG.LOSS_KEYS, "weighted"):
        up = LG.LOSS_WEIGHTS if name == "weighted" else LG.one_hot(name)
        R = LG.probpose_loss_grads(inp["gt"], inp["pred"], gt_oks, gt_err, kw, zeros, up)
        for key in LG.PRED_KEYS[1:]:
            LR.assert_within(golden[f"{tag}_{name}_{key}"], R[key][0], R[key][1], 2 * R[key][2], f"{tag} {name} {key}")
        v, mag, c = R["heatmaps"]
        if name in ("kpt", "weighted"):
            idx = golden[f"{tag}_hm_map_index"]
            if f"{tag}_kpt_hm_maps" in golden:
                LR.assert_within(golden[f"{tag}_kpt_hm_maps"], v.reshape(B * K, H, W)[idx],
                                 mag.reshape(B * K, H, W)[idx], 2 * c, f"{tag} {name} heatmap maps")
            vm, mm = v.reshape(B * K, -1), mag.reshape(B * K, -1)
            LR.assert_within(golden[f"{tag}_kpt_hm_sum"], vm.sum(1), mm.sum(1), 2 * c, f"{tag} heatmap map sums")
            LR.assert_within(golden[f"{tag}_kpt_hm_abs"], np.abs(vm).sum(1), mm.sum(1), 2 * c, f"{tag} |heatmap| sums")
        else:
            assert not v.any()


def test_oks_heatmap_grads_against_reference_goldens(golden):
    hi = LR.heatmap_case_inputs()
    assert str(golden["input_sha"]) == LR.sha(hi["output"])
    B, K, H, W = hi["output"].shape
    for i, (ot, skip, wk, mk, sw, gw, lw) in enumerate(LR.heatmap_options()):
        rng = np.random.default_rng(int(golden["upstream_seed"]) + i)
        ups = dict(pixel=rng.normal(size=(B, K, H, W)).astype(np.float32),
                   keypoint=rng.normal(size=(B, K)).astype(np.float32), mean=np.float32(rng.normal()))
        for red, u in ups.items():
            R = LG.oks_heatmap_loss_grad(hi["output"], hi["target"], hi[wk] if wk else None, hi[mk] if mk else None,
                                         skip, ot, sw, gw, lw, red, u)
            LR.assert_within(golden[f"hm{i}_{red}_grad"], R[0], R[1], 2 * R[2], f"option {i} {red}")


# ----------------------------------------------------------------------------------------------- planted faults
def _heat_case(H, W, seed=3):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.2, 1.2, (2, 3, H, W)).astype(np.float32)
    t = rng.random((2, 3, H, W), dtype=np.float32)
    u = rng.normal(size=(2, 3, H, W)).astype(np.float32)
    return o, t, u


@pytest.mark.parametrize("fault", ["unflipped", "border", ("seam", 9)])
def test_comparator_rejects_sobel_faults(fault):
    o, t, u = _heat_case(20, 11)
    good = LG.oks_heatmap_loss_grad(o, t, reduction="pixel", upstream=u)
    bad = LG.oks_heatmap_loss_grad(o, t, reduction="pixel", upstream=u, fault=fault)
    assert LR.ratio(good[0], *good) == 0.0
    assert LR.ratio(bad[0], *good) > 1.0, fault
    if fault == "border":       # only the border moves
        inner = (slice(None), slice(None), slice(1, -1), slice(1, -1))
        assert np.array_equal(bad[0][inner], good[0][inner])


@pytest.mark.parametrize("red", ["keypoint", "mean"])
def test_comparator_rejects_last_maximal_pixel(red):
    o = np.stack([tie_map(9, 7), tie_map(9, 7, 4, 2)])[None]
    t = np.zeros_like(o)
    e = LG.energy_f32(o, np.ones_like(o))
    assert ((e == e.reshape(1, 2, -1).max(-1)[..., None, None]).sum(axis=(2, 3)) == 2).all()     # exact 2-way ties
    good = LG.oks_heatmap_loss_grad(o, t, reduction=red, upstream=np.ones((1, 2)) if red == "keypoint" else 1.0)
    bad = LG.oks_heatmap_loss_grad(o, t, reduction=red, upstream=np.ones((1, 2)) if red == "keypoint" else 1.0,
                                   fault="last_max")
    assert LR.ratio(bad[0], *good) > 1.0
    # and the first maximum is torch's choice on the CPU
    ot = torch.tensor(o, dtype=torch.float64, requires_grad=True)
    _, kp, mean = torch_heatmap_loss(ot, torch.tensor(t, dtype=torch.float64), None, None, False, "minus", 0.2, 0.0,
                                     1.0)
    (kp.sum() if red == "keypoint" else mean).backward()
    assert LR.ratio(ot.grad.numpy(), *good) <= 1.0


@pytest.mark.parametrize("fault", ["bce_noclamp", "l1log_nodiv", "vis_weighted"])
def test_comparator_rejects_head_faults(golden_fwd, fault):
    inp = LR.case_inputs("G1")
    pred = list(inp["pred"])
    if fault == "bce_noclamp":      # a probability of exactly 0 and 1: the clamp decides the gradient
        pred[1] = pred[1].copy()
        pred[1].reshape(-1)[:4] = (0.0, 1.0, 0.0, 1.0)
    gt_oks = golden_fwd["G1_gt_oks"].astype(np.float32)
    gt_err = golden_fwd["G2_gt_err"].astype(np.float32)     # nonzero error targets
    up = {k: 1.0 for k in LG.LOSS_KEYS}
    good = LG.probpose_loss_grads(inp["gt"], pred, gt_oks, gt_err, upstream=up)
    bad = LG.probpose_loss_grads(inp["gt"], pred, gt_oks, gt_err, upstream=up, fault=fault)
    key = {"bce_noclamp": "probs", "l1log_nodiv": "errs", "vis_weighted": "vis"}[fault]
    assert np.isfinite(good[key][0]).all()
    assert LR.ratio(bad[key][0], *good[key]) > 1.0, fault
    for other in LG.PRED_KEYS:
        if other != key:
            assert LR.ratio(bad[other][0], *good[other]) == 0.0
