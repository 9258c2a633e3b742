"""The ProbPose losses on an MI355X (csrc/pp_loss.hip through probpose.loss) against the reference's goldens
(tests/golden/loss.npz) and the float64 restatement of tests/loss_reference.py."""
import os

import numpy as np
import pytest
import torch

from tests import loss_reference as LR

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss.npz")
PROBPOSE_CASES = {"G1": ("G1", True, False, False), "G2": ("G1", False, True, True), "G3": ("G3", True, False, False),
                  "G3e": ("G3", False, False, False)}
LOSS_KEYS = ("kpt", "probability", "visibility", "oks", "error")
WORST = {}      # quantity -> worst d/bound seen (printed at the end of the module)


def _note(what, q):
    WORST[what] = max(WORST.get(what, 0.0), q)
    assert q <= 1.0, f"{what}: d/bound = {q:.3g}"


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst d/bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})


@pytest.fixture(scope="module")
def golden(built_lib):
    return np.load(GOLDEN)


def _gt(gt, how):
    """The collated ground truth as numpy, host tensors or device tensors."""
    if how == "numpy":
        return gt
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in gt.items()}
    return t if how == "host" else {k: v.cuda() for k, v in t.items()}


def _restate(T, inp, sigmas, freeze, kw, zeros, fault=None):
    pred = tuple(p if isinstance(p, np.ndarray) else p.cpu().numpy() for p in inp["pred"])
    return LR.probpose_loss(inp["gt"], pred, T["gt_kpts"].cpu().numpy(), T["dt_kpts"].cpu().numpy(), sigmas,
                            freeze_error=freeze, keypoint_weights=kw, learn_heatmaps_from_zeros=zeros, fault=fault)


def _check_terms(T, losses, R, accs=None, tag=""):
    for k in LOSS_KEYS:
        _note(f"ProbPoseLoss {k}", LR.ratio(losses[k].cpu().numpy(), *R[k]))
    for k in ("gt_oks", "gt_err", "vis_weight", "oks_weight"):
        _note(f"ProbPoseLoss {k}", LR.ratio(T[k].cpu().numpy(), *R[k]))
    if accs is not None:
        _note("ProbPoseLoss acc oks (MAE)", LR.ratio(accs["oks"].cpu().numpy(), *R["mae_oks"]))
        _note("ProbPoseLoss acc error (MAE)", LR.ratio(accs["error"].cpu().numpy(), *R["mae_err"]))


@pytest.mark.parametrize("tag,how", [("G1", "numpy"), ("G2", "host"), ("G3", "device"), ("G3e", "numpy")])
def test_probpose_loss_golden(golden, tag, how):
    from probpose.codec import Codec, ProbMap
    from probpose.loss import ProbPoseLoss
    case, freeze, use_kw, zeros = PROBPOSE_CASES[tag]
    inp = LR.case_inputs(case)
    B, K, H, W = inp["B"], inp["K"], inp["H"], inp["W"]
    loss_fn = ProbPoseLoss(Codec(ProbMap(inp["input_size"], (W, H), inp["sigmas"])), freeze_error=freeze)
    pred = tuple(torch.from_numpy(p).cuda() for p in inp["pred"])
    kw = torch.from_numpy(inp["keypoint_weights"]).cuda() if use_kw else None
    np.random.seed(int(golden[f"{tag}_acc_seed"]))
    with torch.no_grad():
        losses, accs = loss_fn(_gt(inp["gt"], how), pred, keypoint_weights=kw, learn_heatmaps_from_zeros=zeros,
                               compute_acc=True)
        T = loss_fn.terms(_gt(inp["gt"], how), pred, kw, zeros)
    assert set(losses) == set(accs) == set(LOSS_KEYS)
    for v in list(losses.values()) + list(accs.values()):
        assert v.is_cuda and v.ndim == 0
    # the batched decodes equal the reference's per-crop decodes
    np.testing.assert_allclose(T["gt_kpts"].cpu().numpy(), golden[f"{tag}_gt_kpts"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(T["dt_kpts"].cpu().numpy(), golden[f"{tag}_dt_kpts"], rtol=0, atol=1e-4)
    R = _restate(T, inp, inp["sigmas"], freeze, inp["keypoint_weights"] if use_kw else None, zeros)
    _check_terms(T, losses, R, accs)
    # the reference's own numbers, within the restatement's bounds (the decodes agree to 1e-4 px)
    for k in ("kpt", "probability", "visibility"):
        _note(f"ProbPoseLoss {k} vs reference", LR.ratio(losses[k].cpu().numpy(), golden[f"{tag}_loss_{k}"],
                                                         R[k][1], R[k][2] * 2))
    for k in ("kpt", "probability", "visibility"):
        a = accs[k].cpu()
        assert a.dtype == getattr(torch, str(golden[f"{tag}_accdtype_{k}"]).replace("torch.", ""))
        assert a.double().numpy() == golden[f"{tag}_acc_{k}"], k


def test_probpose_loss_argmax_codec_against_restatement(golden):
    """ArgMaxProbMap (train.py's fast_codec): the DARK decode of the repo feeds the restatement (cv2 parity of that
    decode stays unpinned, as in test_decode_gpu)."""
    from probpose.codec import ArgMaxProbMap, Codec
    from probpose.loss import ProbPoseLoss
    inp = LR.case_inputs("G3")
    codec = Codec(ArgMaxProbMap(inp["input_size"], (inp["W"], inp["H"]), inp["sigmas"]))
    pred = tuple(torch.from_numpy(p).cuda() for p in inp["pred"])
    for freeze in (True, False):
        loss_fn = ProbPoseLoss(codec, freeze_error=freeze)
        with torch.no_grad():
            losses = loss_fn(_gt(inp["gt"], "device"), pred)
            T = loss_fn.terms(_gt(inp["gt"], "device"), pred)
        _check_terms(T, losses, _restate(T, inp, inp["sigmas"], freeze, None, False))


def test_probpose_loss_is_deterministic():
    from probpose.codec import Codec, ProbMap
    from probpose.loss import ProbPoseLoss
    inp = LR.case_inputs("G1")
    loss_fn = ProbPoseLoss(Codec(ProbMap(inp["input_size"], (inp["W"], inp["H"]), inp["sigmas"])), freeze_error=False)
    pred = tuple(torch.from_numpy(p).cuda() for p in inp["pred"])
    with torch.no_grad():
        a = loss_fn(inp["gt"], pred)
        b = loss_fn(inp["gt"], pred)
    for k in LOSS_KEYS:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def test_requires_grad_is_refused():
    from probpose.codec import Codec, ProbMap
    from probpose.loss import OKSHeatmapLoss, ProbPoseLoss
    inp = LR.case_inputs("G1")
    loss_fn = ProbPoseLoss(Codec(ProbMap(inp["input_size"], (inp["W"], inp["H"]), inp["sigmas"])))
    pred = [torch.from_numpy(p).cuda() for p in inp["pred"]]
    pred[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward only"):
        loss_fn(inp["gt"], tuple(pred))
    with pytest.raises(RuntimeError, match="forward only"):
        OKSHeatmapLoss()(pred[0], torch.from_numpy(inp["gt"]["heatmaps"]).cuda())
    with torch.no_grad():
        loss_fn(inp["gt"], tuple(pred))           # grad mode off: accepted


def test_reference_errors_are_raised():
    from probpose.codec import Codec, ProbMap
    from probpose.loss import OKSHeatmapLoss, ProbPoseLoss
    inp = LR.case_inputs("G1")
    loss_fn = ProbPoseLoss(Codec(ProbMap(inp["input_size"], (inp["W"], inp["H"]), inp["sigmas"])))
    pred = tuple(torch.from_numpy(p).cuda() for p in inp["pred"])
    gt = dict(inp["gt"])
    gt["keypoints_visible"] = np.zeros_like(gt["keypoints_visible"])
    with torch.no_grad(), pytest.raises(RuntimeError, match="min"):
        loss_fn(gt, pred)                                            # loss.py:448 on a batch with nothing annotated
    with torch.no_grad(), pytest.raises(AssertionError, match="normalized"):
        OKSHeatmapLoss()(pred[0], pred[0] * 2)


def test_reexports_are_the_metric_objects():
    import probpose
    from probpose_pytorch_amd import loss, metrics
    assert probpose.loss is loss
    for name in ("compute_oks", "oks_batch", "pck_counts", "keypoint_pck_accuracy", "pose_pck_accuracy",
                 "pose_pck_accuracy_expected", "get_heatmap_maximum", "get_heatmap_expected_value"):
        assert getattr(probpose.loss, name) is getattr(metrics, name)
    assert probpose.metrics is metrics


# ----------------------------------------------------------------------------------------------- OKSHeatmapLoss
def _heat_inputs(B, K, H, W, seed):
    rng = np.random.default_rng(seed)
    out = rng.uniform(-0.2, 1.2, (B, K, H, W)).astype(np.float32)
    tgt = rng.random((B, K, H, W), dtype=np.float32)
    tgt[0, -1] = 0.0                                                  # an empty channel
    w2 = np.where(rng.random((B, K)) < 0.3, 0.0, rng.random((B, K))).astype(np.float32)
    w4 = np.where(rng.random((B, K, H, W)) < 0.3, 0.0, rng.random((B, K, H, W))).astype(np.float32)
    mask = (rng.random((B, 1, H, W)) > 0.3).astype(np.float32)
    return dict(output=out, target=tgt, w2=w2, w4=w4, mask=mask)


def _guarded(n, dev, guard=4099):
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[guard:guard + n]


def _run_heat(hi, opts):
    """pp_oks_heatmap_loss with NaN-filled guarded outputs: (per-pixel, per-keypoint, scalars) as numpy."""
    from probpose_pytorch_amd.loss import _oks_heatmap_loss
    ot, skip, wk, mk, sw, gw, lw = opts
    d = {k: torch.from_numpy(v).cuda() for k, v in hi.items()}
    B, K, H, W = hi["output"].shape
    pix_buf, pix = _guarded(B * K * H * W, "cuda")
    kp_buf, kp = _guarded(B * K, "cuda")
    sc_buf, sc = _guarded(3, "cuda")
    _oks_heatmap_loss(d["output"], d["target"], d[wk] if wk else None, d[mk] if mk else None, skip, ot, sw, gw, lw,
                      pix, kp, sc)
    torch.cuda.synchronize()
    for buf, view in zip((pix_buf, kp_buf, sc_buf), (pix, kp, sc)):     # every guard element still the NaN fill
        assert buf[:4099].isnan().all() and buf[4099 + view.numel():].isnan().all()
    assert float(sc[2]) == 0
    return pix.view(B, K, H, W).cpu().numpy(), kp.view(B, K).cpu().numpy(), sc.cpu().numpy()


def _check_heat(hi, opts, shape_tag):
    pix, kp, sc = _run_heat(hi, opts)
    ot, skip, wk, mk, sw, gw, lw = opts
    B, K = hi["output"].shape[:2]
    step = max(1, 4096 // (hi["output"].shape[2] * hi["output"].shape[3]))     # maps per restated chunk
    s_kp = a_kp = s_px = a_px = 0.0
    for k0 in range(0, K, step):
        sl = (slice(None), slice(k0, k0 + step))
        sub = lambda key: (None if key is None else (hi[key][sl] if hi[key].shape[1] > 1 else hi[key]))  # noqa: E731
        R = LR.oks_heatmap_loss(hi["output"][sl], hi["target"][sl], sub(wk), sub(mk), skip, ot, sw, gw, lw)
        _note(f"OKSHeatmapLoss per-pixel {shape_tag}", LR.ratio(pix[sl], *R["pixel"]))
        _note(f"OKSHeatmapLoss per-keypoint {shape_tag}", LR.ratio(kp[sl], *R["keypoint"]))
        s_kp, a_kp = s_kp + R["keypoint"][0].sum(), a_kp + R["keypoint"][1].sum()
        s_px, a_px = s_px + R["pixel"][0].sum(), a_px + R["pixel"][1].sum()
    H, W = hi["output"].shape[2:]
    c = LR.C_PIX + LR.c_sum(H * W) + 2
    _note(f"OKSHeatmapLoss mean {shape_tag}", LR.ratio(sc[0], s_kp / (B * K), a_kp / (B * K), c))
    _note(f"OKSHeatmapLoss pixel mean {shape_tag}", LR.ratio(sc[1], s_px / (B * K * H * W), a_px / (B * K * H * W), c))


@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (2, 3, 3, 5), (2, 3, 65, 49), (2, 3, 256, 256), (64, 17, 64, 48)])
def test_oks_heatmap_loss_every_option(shape):
    hi = _heat_inputs(*shape, seed=sum(shape))
    tag = "x".join(map(str, shape))
    for opts in LR.heatmap_options():
        _check_heat(hi, opts, tag)


def test_oks_heatmap_loss_large_benchmark_shape():
    """B=128, K=133, 96x72 (vit_h_wholebody's maps): the ProbPoseLoss setting and the all-options corner."""
    hi = _heat_inputs(128, 133, 96, 72, seed=5)
    for opts in [("minus", False, "w2", None, 0.05, 0.0, 1.0), ("both", True, "w4", "mask", 0.05, 0.3, 2.5),
                 ("plus", True, "w2", "mask", 0.2, 0.1, 1.0), ("minus", False, None, None, 0.2, 0.0, 1.0)]:
        _check_heat(hi, opts, "128x133x96x72")


def test_oks_heatmap_loss_golden(golden):
    from probpose.loss import OKSHeatmapLoss
    hi = LR.heatmap_case_inputs()
    d = {k: torch.from_numpy(v).cuda() for k, v in hi.items()}
    for i, (ot, skip, wk, mk, sw, gw, lw) in enumerate(LR.heatmap_options()):
        m = OKSHeatmapLoss(use_target_weight=wk is not None, skip_empty_channel=skip, smoothing_weight=sw,
                           gaussian_weight=gw, loss_weight=lw, oks_type=ot)
        R = LR.oks_heatmap_loss(hi["output"], hi["target"], hi[wk] if wk else None, hi[mk] if mk else None, skip,
                                ot, sw, gw, lw)
        args = (d["output"], d["target"], d[wk] if wk else None, d[mk] if mk else None)
        with torch.no_grad():
            got = dict(pixel=m(*args, per_pixel=True), keypoint=m(*args, per_keypoint=True), mean=m(*args))
        for red in ("pixel", "keypoint", "mean"):
            _note(f"OKSHeatmapLoss {red} golden", LR.ratio(got[red].cpu().numpy(), *R[red]))
            _note(f"OKSHeatmapLoss {red} vs reference",
                  LR.ratio(got[red].cpu().numpy(), golden[f"hm{i}_{red}"], R[red][1], R[red][2] * 2))


def test_small_losses_golden(golden):
    from probpose.loss import BCELoss, L1LogLoss, MSELoss
    S = LR.small_inputs()
    t = {k: torch.from_numpy(v).cuda() for k, v in S.items()}
    with torch.no_grad():
        for sig in (True, False):
            for red in ("mean", "sum", "none"):
                for wn in ("none", "w1", "w2"):
                    m = BCELoss(use_target_weight=wn != "none", reduction=red, use_sigmoid=sig, loss_weight=1.5)
                    got = m(t["x"] if sig else t["logits"], t["y"], None if wn == "none" else t[wn])
                    R = LR.bce_loss(S["x"] if sig else S["logits"], S["y"], None if wn == "none" else S[wn], sig,
                                    wn != "none", red, 1.5)
                    _note("BCELoss", LR.ratio(got.cpu().numpy(), *R))
        _note("MSELoss", LR.ratio(MSELoss(True)(t["a"], t["b"], t["wm"]).cpu().numpy(),
                                  *LR.mse_loss(S["a"], S["b"], S["wm"], True)))
        for D in (1, 2):
            got = L1LogLoss(True)(t[f"eo{D}"], t[f"et{D}"], t[f"wl{D}"]).cpu().numpy()
            _note("L1LogLoss", LR.ratio(got, *LR.l1log_loss(S[f"eo{D}"], S[f"et{D}"], S[f"wl{D}"], True)))


def test_end_to_end_vit_b():
    """ProbMap.encode_device targets, a 4-crop vit_b forward, ProbPoseLoss(compute_acc=True), and the restatement on
    the same heatmaps."""
    import bench
    from probpose.loss import ProbPoseLoss
    from probpose_pytorch_amd import synthetic as syn
    cfg = dict(bench.CONFIGS["vit_b"])
    model, codec, _ = bench.build(cfg, torch.bfloat16, torch.device("cuda", 0))
    B, K = 4, cfg["K"]
    x = syn.synthetic_crops(B, 256, 192, seed=3).cuda()
    rng = np.random.default_rng(4)
    kps = rng.uniform(-10, 200, (B, K, 2)).astype(np.float32)
    annotated = rng.random((B, K)) > 0.2
    heat, _ = codec.probmap.encode_device(kps, annotated.astype(np.float32))
    w_in, h_in = codec.probmap.input_size
    in_image = (kps[..., 0] >= 0) & (kps[..., 0] < w_in) & (kps[..., 1] >= 0) & (kps[..., 1] < h_in)
    gt = dict(heatmaps=heat, in_image=in_image[:, None], keypoints_visible=annotated[:, None],
              keypoints_visibility=(rng.random((B, 1, K)) > 0.5).astype(np.float32))
    loss_fn = ProbPoseLoss(codec, freeze_error=False)
    with torch.no_grad():
        pred = model(x)
        np.random.seed(0)
        losses, accs = loss_fn(gt, pred, compute_acc=True)
        T = loss_fn.terms(gt, pred)
    gt_np = dict(gt, heatmaps=heat.cpu().numpy())
    R = LR.probpose_loss(gt_np, tuple(p.float().cpu().numpy() for p in pred), T["gt_kpts"].cpu().numpy(),
                         T["dt_kpts"].cpu().numpy(), codec.probmap.sigmas, freeze_error=False)
    _check_terms(T, losses, R, accs)
    for v in accs.values():
        assert torch.isfinite(v).all()
