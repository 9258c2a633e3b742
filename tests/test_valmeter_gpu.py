"""ValidationMeter on an MI355X (csrc/pp_valmeter.hip through probpose_pytorch_amd.valmeter) against the gauge of
tests/valmeter_reference.py: the integer state for equality, the report within a bound counted in float64 roundings.

The gauge forms every report field as an exact rational of the integer state, rounded once.  The device forms it from
the same integers with a handful of float64 operations; U = 2^-53 per rounding:

* quotients of two integers (bal_acc, best_bal_acc, auroc, brier, ece, mce, mean_conf, base_rate, the reliability
  entries, the OKS and error mae / bias, pck, mean_prob): int -> double of the numerator (1, when it exceeds 2^53), the
  product forming the denominator (1), the division (1), the gauge's own rounding (1): 4 U, relative.
* rmse: that quotient (3), the square root (1) and the gauge's two (2): 6 U, relative.
* pearson = cov / sqrt(vx vt): each of vx, vt, cov is a quotient (3) minus a product (1) of two means (3 each, entering
  with a factor <= 1) with the subtraction's rounding (1): 3 + 1 + 6 + 1 = 11 U absolute on values <= 1; through
  r = cov / sqrt(vx vt) that is 11 U / sqrt(vx vt) + |r| 11 U (1 / vx + 1 / vt) / 2, with |r| <= 1, plus the product,
  root and division (3) and the gauge's own three (3): absolute, and meaningful where the variances are not degenerate.
* the per-batch means (losses, MAEs, acc_kpt): float64 sums in update order on both sides, one division: 2 U relative
  against the gauge, (batches + 1) U against a host mean of the same float32 values.
"""
import math

import numpy as np
import pytest
import torch

from tests import loss_reference as LR
from tests import valmeter_reference as vr

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
THR = np.arange(0.1, 1.0, 0.05)
QUOTIENT, RMSE, MEANS = 4, 6, 2


def _meter(thr=None, ece_bins=16, loss_fn=None):
    from probpose_pytorch_amd import ValidationMeter
    return ValidationMeter(loss_fn, thresholds=thr, ece_bins=ece_bins)


def _dev(batch):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch]


def _state_np(meter):
    return {k: v.cpu().numpy() for k, v in meter.state.items()}


def _assert_state(meter, want, scalars=True):
    got = _state_np(meter)
    assert list(got) == list(want)
    for name in want:
        if name == "scalars" and not scalars:
            continue
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), name


def _close(got, want, c, what, absolute=False):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    scale = 1.0 if absolute else np.abs(want[ok])
    worst = np.abs(got[ok] - want[ok]) - c * U * scale
    assert (worst <= 0).all(), f"{what}: off by {np.max(worst):.3g} beyond {c} U"


def _pearson_bound(state, K):
    """The absolute bound of the module docstring, per row, from the gauge's exact moments (inf where undefined)."""
    out = []
    for r in [slice(k, k + 1) for k in range(K)] + [slice(0, K)]:
        n = int(state["oks_hist"][r].sum())
        if n == 0:
            out.append(math.inf)
            continue
        vx, vt, _ = vr.oks_moments(n, int(state["oks_sx"][r].sum()), int(state["oks_st"][r].sum()),
                                   state["oks_sums"][r].sum(0))
        if vx <= 0 or vt <= 0:
            out.append(math.inf)
            continue
        vx, vt = float(vx), float(vt)
        out.append((11 / math.sqrt(vx * vt) + 5.5 * (1 / vx + 1 / vt) + 6) * U)
    return np.array(out)


def _assert_report(got, want, state, K):
    assert np.array_equal(got["thresholds"], want["thresholds"])
    for head in ("probability", "visibility"):
        for name in vr.BINARY + ("bal_acc", "reliability"):
            _close(got[head][name], want[head][name], 0 if name in ("n_pos", "n_neg", "best_thr") else QUOTIENT,
                   f"{head}.{name}")
    for name in ("n", "mae", "bias", "reliability"):
        _close(got["oks"][name], want["oks"][name], 0 if name == "n" else QUOTIENT, f"oks.{name}")
    _close(got["oks"]["rmse"], want["oks"]["rmse"], RMSE, "oks.rmse")
    g, w, bound = got["oks"]["pearson"], want["oks"]["pearson"], _pearson_bound(state, K)
    sure = np.isfinite(bound) & (bound < 1e-9)           # rows whose variances are not degenerate
    assert np.array_equal(np.isnan(g[sure]), np.isnan(w[sure])) and not np.isnan(w[sure]).any()
    assert (np.abs(g[sure] - w[sure]) <= bound[sure]).all(), "oks.pearson"
    for name in ("n", "mae", "bias"):
        _close(got["error"][name], want["error"][name], 0 if name == "n" else QUOTIENT, f"error.{name}")
    _close(got["pck"], want["pck"], QUOTIENT + K, "pck")        # the pool row adds up to K quotients
    for name, v in want["reference"].items():
        _close(got["reference"][name], v, MEANS, name)
    _close(got["max_heatmap"], want["max_heatmap"], 0, "max_heatmap")
    _close(got["mean_prob"], want["mean_prob"], QUOTIENT, "mean_prob")
    for name in ("batches", "flagged_batches", "flags", "rejected"):
        assert got[name] == want[name], name


def _same_report(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same_report(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _run(batches, K, thr=THR, ece_bins=16):
    meter = _meter(thr, ece_bins)
    want = vr.empty_state(K, len(thr))
    for b in batches:
        meter.update_heads(*_dev(b))
        vr.update(want, thr, *b)
    _assert_state(meter, want)
    _assert_report(meter.compute(), vr.report(want, thr, ece_bins), want, K)
    return meter, want


# ----------------------------------------------------------------------------------------------- update_heads
@pytest.mark.parametrize("B,K", [(1, 1), (3, 17), (40, 133)])
def test_shapes(built_lib, B, K):
    rng = np.random.default_rng(B * 1000 + K)
    _run([vr.random_batch(rng, B, K), vr.random_batch(rng, B, K)], K)


def test_maximal_contention(built_lib):
    """2048 samples of one keypoint, every prediction 0.5: every atomic of the launch lands on the same few words."""
    B = 2048
    half = np.full((B, 1), 0.5, np.float32)
    ones = np.ones((B, 1), np.int64)
    label = (np.arange(B).reshape(B, 1) % 2).astype(np.int64)
    meter, want = _run([[half, half, half, half, label, ones, label, half, half]], 1)
    assert want["hist"][0, 0, :, 512].tolist() == [1024, 1024] and want["oks_hist"][0, 512] == 1024
    rep = meter.compute()
    assert rep["probability"]["auroc"][0] == 0.5 and math.isnan(rep["oks"]["pearson"][0])


@pytest.mark.parametrize("thr", [np.array([0.5]), np.concatenate([np.arange(1, 63) / 65, [0.25, 0.5]]), THR],
                         ids=["J1", "J64", "J18"])
def test_edge_values_and_thresholds(built_lib, thr):
    """0, 1, k/1024 and both float32 neighbours, float32(0.15) (above the float64 0.15000000000000002), values equal to
    a threshold (not above), in every head and keypoint."""
    e = vr.edge_values()
    rng = np.random.default_rng(3)
    B, K = len(e), 3
    cols = [np.stack([e, e[::-1], rng.permutation(e)], axis=1) for _ in range(4)]
    prob, vis, oks, gt_oks = (np.ascontiguousarray(c) for c in cols)
    err = np.ascontiguousarray((cols[0] * 7).astype(np.float32))
    label = (rng.random((B, K)) < 0.5).astype(np.int64)
    ones = np.ones((B, K), np.int64)
    meter, want = _run([[prob, vis, oks, err, label, ones, label, gt_oks, err[::-1].copy()]], K, thr, ece_bins=64)
    if len(thr) != len(THR):
        j = int(np.argmin(np.abs(thr - 0.5)))
        assert thr[j] == 0.5
        # column 0 holds each edge value once: exactly those strictly above 0.5 are counted, 0.5 itself is not
        half = np.float32(0.5)
        assert want["above"][0, 0, :, j].sum() == int((e > half).sum()) < int((e >= half).sum())
    else:
        assert want["above"][0, 0, :, 1].sum() == int((e >= np.float32(0.15)).sum())


@pytest.mark.parametrize("head", [0, 1, 2, 3])
def test_invalid_values_reject_one_head_only(built_lib, head):
    rng = np.random.default_rng(40 + head)
    B, K = 6, 4
    batch = vr.random_batch(rng, B, K, ties=False)
    batch[4][:] = 1
    batch[5][:] = 1
    bad = [np.nan, -0.1, 1.5, np.inf]
    batch[head][0, :] = bad
    meter, want = _run([batch], K)
    rej = meter.compute()["rejected"]
    n_bad = 3 if head == 3 else 4            # 1.5 is a legal error
    assert rej == {**{k: 0 for k in vr.REJECTED}, vr.REJECTED[1 + head]: n_bad}
    sizes = [want["hist"][0].sum(), want["hist"][1].sum(), want["oks_hist"].sum(), want["err"][:, 0].sum()]
    assert sizes == [B * K - (n_bad if i == head else 0) for i in range(4)]


def test_masks_and_error_range(built_lib):
    rng = np.random.default_rng(9)
    B, K = 5, 3
    batch = vr.random_batch(rng, B, K, ties=False)
    batch[4][:] = 1
    batch[5][:] = 1
    batch[4][1, 1] = 2                       # a mask value of 2: out of every head
    batch[5][2, 0] = -1
    batch[3][0, 0] = 2.0 ** 20               # accepted
    batch[3][0, 1] = np.nextafter(np.float32(2 ** 20), np.float32(np.inf))      # rejected
    meter, want = _run([batch], K)
    rej = meter.compute()["rejected"]
    assert rej["mask"] == 2 and rej["error"] == 1 and rej["probability"] == rej["oks"] == 0
    assert want["hist"][0].sum() == B * K - 2 and want["err"][:, 0].sum() == B * K - 3 and want["all"][0] == B * K


def test_empty_populations(built_lib):
    """Keypoint 0 has no positives, 1 no negatives, 2 nobody annotated, 3 is ordinary; then a batch with nothing
    annotated at all."""
    rng = np.random.default_rng(12)
    B, K = 16, 4
    batch = vr.random_batch(rng, B, K)
    batch[5][:] = 1
    batch[4][:, 0], batch[4][:, 1] = 0, 1
    batch[5][:, 2] = 0
    nothing = vr.random_batch(rng, 3, K)
    nothing[5][:] = 0
    meter, want = _run([batch, nothing], K)
    rep = meter.compute()
    p = rep["probability"]
    for k in (0, 1, 2):
        assert p["best_bal_acc"][k] == 0.0 and p["best_thr"][k] == 0.0
        assert math.isnan(p["auroc"][k]) and np.isnan(p["bal_acc"][k]).all()
    assert math.isnan(p["brier"][2]) and not math.isnan(p["brier"][0]) and p["n_pos"][0] == 0 and p["n_neg"][1] == 0
    assert math.isnan(rep["oks"]["mae"][0]) and rep["oks"]["n"][0] == 0          # not in the image: no OKS sample
    assert p["best_bal_acc"][K] > 0 and 0 <= p["auroc"][K] <= 1                  # the pool row is still right
    assert rep["batches"] == 2 and want["all"][0] == (B + 3) * K
    fresh = _meter(THR)
    fresh.update_heads(*_dev(nothing))
    rep = fresh.compute()
    assert rep["probability"]["n_pos"][K] == 0 and math.isnan(rep["error"]["mae"][K]) and rep["batches"] == 1


def test_algebra_on_the_device(built_lib):
    rng = np.random.default_rng(21)
    K = 17
    a, b = vr.random_batch(rng, 9, K), vr.random_batch(rng, 4, K)
    both = [np.concatenate([x, y]) for x, y in zip(a, b)]
    m_ab, m_ba, m_cat = _meter(THR), _meter(THR), _meter(THR)
    for m, seq in ((m_ab, (a, b)), (m_ba, (b, a)), (m_cat, (both,))):
        for batch in seq:
            m.update_heads(*_dev(batch))
    for name in m_ab.state:
        assert torch.equal(m_ab.state[name], m_ba.state[name]), name            # order
        if name != "scalars":                                                    # the batch count differs
            assert torch.equal(m_ab.state[name], m_cat.state[name]), name        # split
    first = m_ab.compute()
    assert _same_report(first, m_ab.compute())          # compute() changes nothing
    m_ab.reset()
    assert all(int(v.abs().sum()) == 0 for v in m_ab.state.values())
    m_ab.update_heads(*_dev(both))
    assert all(torch.equal(m_ab.state[n], m_cat.state[n]) for n in m_cat.state)


# ----------------------------------------------------------------------------------------------- update(gt, pred)
def _case(name):
    from probpose.codec import Codec, ProbMap
    from probpose.loss import ProbPoseLoss
    inp = LR.case_inputs(name)
    loss_fn = ProbPoseLoss(Codec(ProbMap(inp["input_size"], (inp["W"], inp["H"]), inp["sigmas"])), freeze_error=False)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp["gt"].items()}
    pred = tuple(torch.from_numpy(p).cuda() for p in inp["pred"])
    flip = lambda d: {k: v.flip(0) for k, v in d.items()}      # noqa: E731
    batches = [(gt, pred), (flip(gt), tuple(p.flip(0).contiguous() for p in pred))]
    return inp, loss_fn, batches


def _gauge_of_update(loss_fn, batches, K, thr):
    """The gauge fed with what the meter's launches produce for each batch (the loss terms are tested elsewhere)."""
    from probpose_pytorch_amd.metrics import _argmax_device, pck_counts
    want, counts, maxima = vr.empty_state(K, len(thr)), [], []
    for gt, pred in batches:
        with torch.no_grad():
            T = loss_fn.terms(gt, pred)
        B, _, H, W = pred[0].shape
        p, vals, _ = _argmax_device(T["hm"])
        g, _, _ = _argmax_device(T["gt_hm"])
        c = np.stack(pck_counts(p, g, (T["kw"] > 0.5), 0.05, np.tile(np.array([[H, W]]), (B, 1))))
        counts.append(c)
        maxima.append(vals.cpu().numpy())
        heads = [h.cpu().numpy().reshape(B, K) for h in T["heads"]]
        vr.update(want, thr, *heads, T["probs"], T["annotated"], T["vis"], T["gt_oks"].cpu().numpy(),
                  T["gt_err"].cpu().numpy(), pck_counts=c, map_max=maxima[-1], res=T["res"].cpu().numpy())
    return want, counts, maxima


@pytest.mark.parametrize("name", ["G1", "G3"])
def test_update_matches_the_loss_and_the_metrics(built_lib, name):
    inp, loss_fn, batches = _case(name)
    K = inp["K"]
    meter = _meter(THR, loss_fn=loss_fn)
    for gt, pred in batches:
        meter.update(gt, pred)
    want, counts, maxima = _gauge_of_update(loss_fn, batches, K, THR)
    _assert_state(meter, want)
    rep = meter.compute()
    _assert_report(rep, vr.report(want, THR), want, K)
    # PCK hits / valid are the sums of metrics.pck_counts
    assert np.array_equal(meter.state["pck"].cpu().numpy(), np.sum(counts, axis=0))
    assert rep["max_heatmap"] == max(float(p[0].max()) for _, p in batches)
    # the reference view: means of ProbPoseLoss.forward(compute_acc=True) over the same batches
    np.random.seed(0)
    with torch.no_grad():
        outs = [loss_fn(gt, pred, compute_acc=True) for gt, pred in batches]
    n = len(outs)
    for key in ("kpt", "probability", "visibility", "oks", "error"):
        host = sum(float(o[0][key]) for o in outs) / n
        _close(rep["reference"][f"loss_{key}"], host, n + 1, f"loss_{key}")
    for key in ("oks", "error"):
        host = sum(float(o[1][key]) for o in outs) / n
        _close(rep["reference"][f"acc_{key}"], host, n + 1, f"acc_{key}")
    # acc_kpt: each batch's average is np.mean over at most K quotients there, a running sum here
    host = sum(float(o[1]["kpt"]) for o in outs) / n
    _close(rep["reference"]["acc_kpt"], host, n + 1 + 2 * K, "acc_kpt")
    assert rep["batches"] == n and rep["flagged_batches"] == 0 and rep["flags"] == 0


def test_flagged_batches_and_nan_maps(built_lib):
    """The fault cases of test_loss_gpu.py::test_reference_errors_are_raised: counted, left out of the means, never
    raised; a NaN in a predicted map makes max_heatmap NaN."""
    inp, loss_fn, batches = _case("G1")
    gt, pred = batches[0]
    meter = _meter(THR, loss_fn=loss_fn)
    meter.update(gt, pred)
    clean = meter.compute()
    none = dict(gt, keypoints_visible=torch.zeros_like(gt["keypoints_visible"]))
    meter.update(none, pred)                                        # loss.py:448 would raise
    twice = dict(gt, heatmaps=gt["heatmaps"] * 2)
    meter.update(twice, pred)                                       # 'target should be normalized'
    rep = meter.compute()
    assert rep["batches"] == 3 and rep["flagged_batches"] == 2
    assert rep["flags"] & 1 and rep["flags"] & vr.FLAG_TARGET_RANGE
    assert _same_report(rep["reference"], clean["reference"])
    assert rep["probability"]["n_pos"][-1] + rep["probability"]["n_neg"][-1] > \
        clean["probability"]["n_pos"][-1] + clean["probability"]["n_neg"][-1]      # their samples still count
    assert rep["max_heatmap"] == clean["max_heatmap"]
    hm = pred[0].clone()
    hm[1, 2, 3, 4] = float("nan")
    meter.update(gt, (hm, *pred[1:]))
    assert math.isnan(meter.compute()["max_heatmap"])


def test_updates_do_not_synchronise(built_lib):
    inp, loss_fn, batches = _case("G1")
    meter, heads = _meter(THR, loss_fn=loss_fn), _meter(THR)
    arrays = _dev(vr.random_batch(np.random.default_rng(5), 8, 17))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gt, pred in batches:
            meter.update(gt, pred)
        heads.update_heads(*arrays)
        heads.update_heads(*arrays)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert meter.compute()["batches"] == 2 and heads.compute()["batches"] == 2


def test_run_over_a_loader(built_lib):
    from oracle import probpose_oracle as orc
    from probpose.codec import Codec, ProbMap
    from probpose.loss import ProbPoseLoss
    from probpose_pytorch_amd import ValidationMeter
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.model import ProbPoseModel
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_model_state
    img, C, depth, heads, pools, K = (64, 48), 128, 2, 2, [(4, 3)], 17
    model = ProbPoseModel(ScratchViTBackbone(img, 16, embed_dim=C, depth=depth, num_heads=heads),
                          ProbMapHead(C, K, pools, (64, 64), (4, 4), final_layer_kernel_size=1))
    model.load_state_dict(synthetic_model_state(img, 16, C, depth, K, len(pools), (64, 64), seed=0))
    model = model.cuda()
    loss_fn = ProbPoseLoss(Codec(ProbMap((48, 64), (12, 16), orc.COCO17_SIGMAS)))
    rng = np.random.default_rng(8)
    loader = []
    for i in range(3):
        B = 2 + i
        kps = rng.uniform((-4, -4), (52, 68), (B, K, 2)).astype(np.float32)
        annotated = rng.random((B, K)) > 0.2
        gt_hm, in_image = LR.encode_probmaps(kps, annotated.astype(np.float32), (48, 64), (12, 16))
        gt = dict(heatmaps=gt_hm, in_image=in_image[:, None, :], keypoints_visible=annotated[:, None, :],
                  keypoints_visibility=(rng.random((B, 1, K)) > 0.4).astype(np.float32))
        loader.append((synthetic_crops(B, *img, seed=i).cuda(),
                       {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in gt.items()}))
    for mode in (True, False):
        model.train(mode)
        rep = ValidationMeter.run(model, loader, loss_fn, ece_bins=8)
        assert model.training is mode
    model.eval()
    meter = ValidationMeter(loss_fn, ece_bins=8)
    with torch.no_grad():
        for x, gt in loader:
            meter.update(gt, model(x))
    assert _same_report(rep, meter.compute())
    assert rep["batches"] == 3 and rep["flagged_batches"] == 0 and rep["oks"]["n"][-1] > 0
