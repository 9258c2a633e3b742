"""The ProbPose loss gradients on an MI355X (pp_oks_heatmap_loss_backward and pp_probpose_loss_grads through
probpose.loss with differentiable=True) against the float64 restatement of tests/loss_grad_reference.py and the
reference's gradients (tests/golden/loss_grad.npz)."""
import os

import numpy as np
import pytest
import torch

from tests import loss_grad_reference as LG
from tests import loss_reference as LR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"G1": ("G1", True, False, False), "G2": ("G1", False, True, True), "G3": ("G3", True, False, False),
         "G3e": ("G3", False, False, False)}
WORST = {}


def _note(what, q):
    WORST[what] = max(WORST.get(what, 0.0), q)
    assert q <= 1.0, f"{what}: d/bound = {q:.3g}"


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst d/bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})


@pytest.fixture(scope="module")
def golden(built_lib):
    return np.load(os.path.join(HERE, "golden", "loss_grad.npz"))


def _loss_fn(inp, freeze, codec_cls=None, differentiable=True):
    from probpose.codec import Codec, ProbMap
    from probpose.loss import ProbPoseLoss
    codec = (codec_cls or ProbMap)(inp["input_size"], (inp["W"], inp["H"]), inp["sigmas"])
    return ProbPoseLoss(Codec(codec), freeze_error=freeze, differentiable=differentiable)


def _leaves(inp):
    return tuple(torch.from_numpy(p).cuda().requires_grad_(True) for p in inp["pred"])


def _check_probpose_grads(grads, R, what):
    for key, g in zip(LG.PRED_KEYS, grads):
        _note(f"{what} {key}", LR.ratio(g.detach().cpu().numpy().reshape(R[key][0].shape), *R[key]))


@pytest.mark.parametrize("tag", list(CASES))
def test_probpose_loss_grads_golden(golden, tag):
    """Each loss alone and train.py's weighted sum: every prediction's gradient against the restatement (fed the
    forward's own targets) and against the reference's gradients."""
    case, freeze, use_kw, zeros = CASES[tag]
    inp = LR.case_inputs(case)
    B, K, H, W = inp["B"], inp["K"], inp["H"], inp["W"]
    loss_fn = _loss_fn(inp, freeze)
    kw_np = inp["keypoint_weights"] if use_kw else None
    kw = torch.from_numpy(kw_np).cuda() if use_kw else None
    pred = _leaves(inp)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp["gt"].items()}
    losses = loss_fn(gt, pred, keypoint_weights=kw, learn_heatmaps_from_zeros=zeros)
    for v in losses.values():
        assert v.grad_fn is not None and v.ndim == 0 and v.is_cuda
    with torch.no_grad():
        T = loss_fn.terms(gt, pred, kw, zeros)
    gt_oks, gt_err = T["gt_oks"].cpu().numpy(), T["gt_err"].cpu().numpy()
    total = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
    fwd = np.load(os.path.join(HERE, "golden", "loss.npz"))
    for name, L in [*losses.items(), ("weighted", total)]:
        up = LG.LOSS_WEIGHTS if name == "weighted" else LG.one_hot(name)
        grads = torch.autograd.grad(L, pred, retain_graph=True)
        R = LG.probpose_loss_grads(inp["gt"], inp["pred"], gt_oks, gt_err, kw_np, zeros, up)
        _check_probpose_grads(grads, R, "ProbPoseLoss grad")
        # the reference's numbers, within twice the bound of the restatement fed the reference's targets
        Rg = LG.probpose_loss_grads(inp["gt"], inp["pred"], fwd[f"{tag}_gt_oks"].astype(np.float32),
                                    fwd[f"{tag}_gt_err"].astype(np.float32), kw_np, zeros, up)
        for key, g in zip(LG.PRED_KEYS[1:], grads[1:]):
            _note(f"ProbPoseLoss grad {key} vs reference",
                  LR.ratio(g.cpu().numpy().reshape(B, K), golden[f"{tag}_{name}_{key}"], Rg[key][1], 2 * Rg[key][2]))
        gh = grads[0].cpu().numpy().reshape(B * K, H, W)
        v, mag, c = Rg["heatmaps"]
        if name in ("kpt", "weighted"):
            idx = golden[f"{tag}_hm_map_index"]
            if f"{tag}_kpt_hm_maps" in golden:
                _note("ProbPoseLoss grad heatmaps vs reference",
                      LR.ratio(gh[idx], golden[f"{tag}_kpt_hm_maps"], mag.reshape(B * K, H, W)[idx], 2 * c))
            _note("ProbPoseLoss grad heatmap sums vs reference",
                  LR.ratio(gh.astype(np.float64).sum((1, 2)), golden[f"{tag}_kpt_hm_sum"],
                           mag.reshape(B * K, -1).sum(1), 2 * c))
        else:
            assert not gh.any()
    # backward fills .grad of every prediction, in its shape, dtype and device
    total.backward()
    for p in pred:
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.is_cuda


def test_probpose_loss_grads_argmax_codec():
    """ArgMaxProbMap, train.py's fast_codec, at train.py's map size with both freeze_error settings."""
    from probpose.codec import ArgMaxProbMap
    inp = LR.case_inputs("G3")
    for freeze in (True, False):
        loss_fn = _loss_fn(inp, freeze, ArgMaxProbMap)
        pred = _leaves(inp)
        losses = loss_fn(inp["gt"], pred)
        total = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
        grads = torch.autograd.grad(total, pred)
        with torch.no_grad():
            T = loss_fn.terms(inp["gt"], pred)
        R = LG.probpose_loss_grads(inp["gt"], inp["pred"], T["gt_oks"].cpu().numpy(), T["gt_err"].cpu().numpy())
        _check_probpose_grads(grads, R, "ProbPoseLoss grad argmax codec")


def test_probpose_loss_compute_acc_and_partial_grads():
    """compute_acc: the accuracies carry no gradient; a heatmap that needs no grad gets none (its launch skipped)."""
    inp = LR.case_inputs("G1")
    loss_fn = _loss_fn(inp, False)
    pred = [torch.from_numpy(p).cuda() for p in inp["pred"]]
    for p in pred[1:]:
        p.requires_grad_(True)
    np.random.seed(3)
    losses, accs = loss_fn(inp["gt"], tuple(pred), compute_acc=True)
    assert all(not a.requires_grad for a in accs.values())
    with torch.no_grad():
        np.random.seed(3)
        l0, a0 = _loss_fn(inp, False, differentiable=False)(inp["gt"], tuple(pred), compute_acc=True)
    for k in LG.LOSS_KEYS:
        assert torch.equal(accs[k], a0[k]) and torch.equal(losses[k].detach(), l0[k]), k
    sum(losses.values()).backward()
    assert pred[0].grad is None and all(p.grad is not None for p in pred[1:])


def test_differentiable_without_grad_is_the_forward_path():
    """differentiable=True without grad (no_grad, or nothing requires grad) gives the default path's bits."""
    from probpose.loss import OKSHeatmapLoss
    inp = LR.case_inputs("G1")
    pred = tuple(torch.from_numpy(p).cuda() for p in inp["pred"])
    with torch.no_grad():
        a = _loss_fn(inp, False)(inp["gt"], pred)
        b = _loss_fn(inp, False, differentiable=False)(inp["gt"], pred)
    c = _loss_fn(inp, False)(inp["gt"], pred)          # grad mode on, nothing requires grad
    for k in LG.LOSS_KEYS:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() == c[k].cpu().numpy().tobytes()
        assert c[k].grad_fn is None
    # and with grad, the forward values are the same bits
    d = _loss_fn(inp, False)(inp["gt"], _leaves(inp))
    for k in LG.LOSS_KEYS:
        assert d[k].detach().cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes()
    t = torch.from_numpy(inp["gt"]["heatmaps"]).cuda()
    for kw in (dict(per_pixel=True), dict(per_keypoint=True), {}):
        with torch.no_grad():
            x = OKSHeatmapLoss(differentiable=True)(pred[0], t, **kw)
        y = OKSHeatmapLoss(differentiable=True)(pred[0].clone().requires_grad_(True), t, **kw)
        assert torch.equal(x, y.detach()) and y.grad_fn is not None


def test_backward_is_deterministic_and_syncs_nothing():
    inp = LR.case_inputs("G3")
    loss_fn = _loss_fn(inp, False)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp["gt"].items()}
    out = []
    for _ in range(2):
        pred = _leaves(inp)
        losses = loss_fn(gt, pred)
        total = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")      # any host sync inside backward raises
        try:
            total.backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        out.append([p.grad.cpu().numpy().tobytes() for p in pred])
    assert out[0] == out[1]


def test_refusals_and_double_backward():
    from probpose.loss import BCELoss, L1LogLoss, MSELoss, OKSHeatmapLoss
    inp = LR.case_inputs("G1")
    loss_fn = _loss_fn(inp, True)
    pred = _leaves(inp)
    gt = dict(inp["gt"], heatmaps=torch.from_numpy(inp["gt"]["heatmaps"]).cuda().requires_grad_(True))
    with pytest.raises(RuntimeError, match="gt_heatmaps requires grad"):
        loss_fn(gt, pred)
    kw = torch.ones(inp["B"], inp["K"], device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="keypoint_weights requires grad"):
        loss_fn(inp["gt"], pred, keypoint_weights=kw)
    o = pred[0]
    t = torch.from_numpy(inp["gt"]["heatmaps"]).cuda()
    with pytest.raises(RuntimeError, match="target requires grad"):
        OKSHeatmapLoss(differentiable=True)(o, t.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="target_weights requires grad"):
        OKSHeatmapLoss(use_target_weight=True, differentiable=True)(o, t, kw)
    with pytest.raises(RuntimeError, match="mask requires grad"):
        OKSHeatmapLoss(differentiable=True)(o, t, None, torch.ones_like(t[:, :1]).requires_grad_(True))
    x, y = pred[1].view(-1), torch.rand(pred[1].numel(), device="cuda")
    for m in (BCELoss(use_sigmoid=True, differentiable=True), MSELoss(differentiable=True),
              L1LogLoss(differentiable=True)):
        with pytest.raises(RuntimeError, match="target requires grad"):
            m(x, y.clone().requires_grad_(True))
        m(x, y).backward()                                         # output only: autograd through torch ops
    with pytest.raises(RuntimeError, match="forward only"):
        BCELoss(use_sigmoid=True)(x, y)                             # the default still refuses
    # double backward through the once-differentiable nodes
    losses = loss_fn(inp["gt"], pred)
    g = torch.autograd.grad(losses["kpt"], pred[0], grad_outputs=torch.ones((), device="cuda", requires_grad=True),
                            create_graph=True)[0]
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    L = OKSHeatmapLoss(differentiable=True)(o, t)
    g = torch.autograd.grad(L, o, grad_outputs=torch.ones((), device="cuda", requires_grad=True), create_graph=True)[0]
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_prediction_dtypes_and_shapes():
    """bf16 heatmaps and flat heads: each gradient comes back in its prediction's shape and dtype."""
    inp = LR.case_inputs("G1")
    B, K = inp["B"], inp["K"]
    pred = [torch.from_numpy(inp["pred"][0]).cuda().bfloat16().requires_grad_(True)]
    pred += [torch.from_numpy(p).cuda().view(B, K).requires_grad_(True) for p in inp["pred"][1:]]
    losses = _loss_fn(inp, False)(inp["gt"], tuple(pred))
    sum(losses.values()).backward()
    for p in pred:
        assert p.grad.shape == p.shape and p.grad.dtype == p.dtype


# ----------------------------------------------------------------------------------------------- OKSHeatmapLoss
def _heat_inputs(B, K, H, W, seed):
    rng = np.random.default_rng(seed)
    out = rng.uniform(-0.2, 1.2, (B, K, H, W)).astype(np.float32)
    tgt = rng.random((B, K, H, W), dtype=np.float32)
    tgt[0, -1] = 0.0
    w2 = np.where(rng.random((B, K)) < 0.3, 0.0, rng.random((B, K))).astype(np.float32)
    w4 = np.where(rng.random((B, K, H, W)) < 0.3, 0.0, rng.random((B, K, H, W))).astype(np.float32)
    mask = (rng.random((B, 1, H, W)) > 0.3).astype(np.float32)
    return dict(output=out, target=tgt, w2=w2, w4=w4, mask=mask)


def _heat_grad(hi, opts, red, u, expand=False):
    from probpose.loss import OKSHeatmapLoss
    ot, skip, wk, mk, sw, gw, lw = opts
    d = {k: torch.from_numpy(v).cuda() for k, v in hi.items()}
    m = OKSHeatmapLoss(use_target_weight=wk is not None, skip_empty_channel=skip, smoothing_weight=sw,
                       gaussian_weight=gw, loss_weight=lw, oks_type=ot, differentiable=True)
    o = d["output"].clone().requires_grad_(True)
    L = m(o, d["target"], d[wk] if wk else None, d[mk] if mk else None, per_pixel=red == "pixel",
          per_keypoint=red == "keypoint")
    ut = torch.as_tensor(u).cuda()
    if expand:      # a broadcast upstream gradient (stride 0)
        ut = ut[:, :, :1].expand(L.shape) if red == "pixel" else ut[:, :1].expand(L.shape)
        u = ut.cpu().numpy()
    L.backward(ut)
    return o.grad.cpu().numpy(), u


def _check_heat_grad(hi, opts, tag):
    B, K, H, W = hi["output"].shape
    rng = np.random.default_rng(B * K + H * W)
    ups = dict(pixel=rng.normal(size=(B, K, H, W)).astype(np.float32),
               keypoint=rng.normal(size=(B, K)).astype(np.float32), mean=np.float32(rng.normal()))
    ot, skip, wk, mk, sw, gw, lw = opts
    for red, u in ups.items():
        for expand in ((False, True) if red != "mean" else (False,)):
            g, u_used = _heat_grad(hi, opts, red, u, expand)
            R = LG.oks_heatmap_loss_grad(hi["output"], hi["target"], hi[wk] if wk else None, hi[mk] if mk else None,
                                         skip, ot, sw, gw, lw, red, u_used)
            _note(f"OKSHeatmapLoss grad {red} {tag}", LR.ratio(g, *R))


SHAPES = [(2, 3, 64, 48), (2, 3, 96, 72), (2, 3, 96, 96), (2, 3, 3, 3), (2, 3, 1, 37), (2, 3, 41, 1), (2, 3, 13, 11),
          (2, 2, 1, 1), (1, 2, 256, 256), (1, 2, 5, 600), (1, 2, 23, 300)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oks_heatmap_loss_grad_shapes(shape):
    """Single- and multi-tile maps (the backward's tile is at most 256 columns and 9..57 rows), 1xW and Hx1."""
    hi = _heat_inputs(*shape, seed=sum(shape))
    opts = LR.heatmap_options()
    if shape[2] * shape[3] > 20000:
        opts = [opts[i] for i in (0, 13, 35)]
    for o in opts:
        _check_heat_grad(hi, o, "x".join(map(str, shape)))


def test_oks_heatmap_loss_grad_golden(golden):
    hi = LR.heatmap_case_inputs()
    B, K, H, W = hi["output"].shape
    for i, opts in enumerate(LR.heatmap_options()):
        ot, skip, wk, mk, sw, gw, lw = opts
        rng = np.random.default_rng(int(golden["upstream_seed"]) + i)
        ups = dict(pixel=rng.normal(size=(B, K, H, W)).astype(np.float32),
                   keypoint=rng.normal(size=(B, K)).astype(np.float32), mean=np.float32(rng.normal()))
        for red, u in ups.items():
            g, _ = _heat_grad(hi, opts, red, u)
            R = LG.oks_heatmap_loss_grad(hi["output"], hi["target"], hi[wk] if wk else None, hi[mk] if mk else None,
                                         skip, ot, sw, gw, lw, red, u)
            _note(f"OKSHeatmapLoss grad {red} golden", LR.ratio(g, *R))
            _note(f"OKSHeatmapLoss grad {red} vs reference", LR.ratio(g, golden[f"hm{i}_{red}_grad"], R[1], 2 * R[2]))


@pytest.mark.parametrize("H,W", [(3, 4), (9, 7), (64, 48), (300, 11), (7, 300)])
def test_oks_heatmap_loss_grad_tie_and_zero_maps(H, W):
    """An exact two-way energy tie (power-of-two maps) takes the subgradient at the first maximum; an all-zero map
    and an all-zero target too."""
    from tests.test_loss_grad_reference import tie_map
    o = np.zeros((2, 2, H, W), np.float32)
    o[0, 0] = tie_map(H, W)
    o[1, 1] = tie_map(H, W, H - 2, W - 3)
    t = np.zeros_like(o)
    t[0, 1] = 0.5
    hi = dict(output=o, target=t)
    for red, u in (("keypoint", np.ones((2, 2), np.float32)), ("mean", np.float32(1.0))):
        opts = ("minus", False, None, None, 0.2, 0.0, 1.0)
        g, _ = _heat_grad(hi, opts, red, u)
        R = LG.oks_heatmap_loss_grad(o, t, reduction=red, upstream=u)
        _note("OKSHeatmapLoss grad tie", LR.ratio(g, *R))
        bad = LG.oks_heatmap_loss_grad(o, t, reduction=red, upstream=u, fault="last_max")
        assert LR.ratio(bad[0], *R) > 1.0


# ----------------------------------------------------------------------------------------------- training
class _TinyPoseNet(torch.nn.Module):
    """Five-tuple out of a fixed batch: heatmaps from a 3x3 conv, the four heads from pooled features."""

    def __init__(self, K):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 16, 3, padding=1)
        self.hm = torch.nn.Conv2d(16, K, 3, padding=1)
        self.heads = torch.nn.Linear(16, 4 * K)
        self.K = K

    def forward(self, x):
        f = torch.relu(self.conv(x))
        hm = torch.sigmoid(self.hm(f))
        h = self.heads(f.mean(dim=(2, 3))).view(x.shape[0], 4, self.K, 1, 1)
        return hm, torch.sigmoid(h[:, 0]), torch.sigmoid(h[:, 1]), torch.sigmoid(h[:, 2]), \
            torch.nn.functional.softplus(h[:, 3])


def test_training_loop_loss_falls():
    """train.py's loop on a fixed batch: 30 AdamW steps with ProbPoseLoss(differentiable=True) and LOSS_WEIGHTS; the
    weighted loss falls and every step's prediction gradients meet the restatement's bound."""
    torch.manual_seed(0)
    inp = LR.case_inputs("G1")
    B, K, H, W = inp["B"], inp["K"], inp["H"], inp["W"]
    x = torch.randn(B, 3, H, W, device="cuda")
    model = _TinyPoseNet(K).cuda()
    opt = torch.optim.AdamW(model.parameters(), lr=3e-3)
    loss_fn = _loss_fn(inp, False)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp["gt"].items()}
    hist = []
    for step in range(30):
        opt.zero_grad()
        pred = model(x)
        for p in pred:
            p.retain_grad()
        losses = loss_fn(gt, pred)
        loss = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
        loss.backward()
        hist.append(float(loss.detach()))
        with torch.no_grad():
            T = loss_fn.terms(gt, pred)
        pn = [p.detach().cpu().numpy() for p in pred]
        R = LG.probpose_loss_grads(inp["gt"], pn, T["gt_oks"].cpu().numpy(), T["gt_err"].cpu().numpy())
        _check_probpose_grads([p.grad for p in pred], R, "training step grad")
        opt.step()
    assert hist[-1] < 0.8 * hist[0], hist
