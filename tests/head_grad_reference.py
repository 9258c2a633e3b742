"""Float64 CPU restatement of the reference ProbMapHead in train mode (probpose/head.py:174-405, 487-594), forward and
backward, for the heads the HIP training path supports (stride-2 k4 deconvolutions, no conv stack, a 1x1 final layer,
``normalize`` None or a float).

The convolutions and the affine pieces are differentiated by torch's float64 autograd; the pieces whose gradient
convention matters are written out as explicit autograd functions: train-mode BatchNorm (batch mean, BIASED variance
in the normalisation, UNBIASED variance in the running update), MaxPool with torch's first-maximum rule, torch.clamp's
inclusive gradient mask, and Sparsemax (the oracle's sort-based forward; backward g_in = s (g - sum(g s) / sum(s)),
s = the support, as sparsemax==0.1.9).

``fault`` plants what the comparators must reject: 'unbiased_norm' (unbiased variance in the normalisation),
'biased_running' (biased variance in the running update), 'last_max' (pooling ties to the last maximum),
'exclusive_clamp' (no gradient at the clamp bounds), 'no_prob_detach' (the probability branch not detached),
'sparsemax_nomean' (the Sparsemax backward without the mean subtraction).

Bounds: every gradient and output is compared as |got - want| <= c * u * magnitude(tensor), with u the unit roundoff
of the compute dtype and magnitude the largest |want| of that tensor (a norm-wise bound; the reductions behind each
value are sums of thousands of terms whose rounding grows with sqrt(depth), c states it per class below).
"""
from __future__ import annotations

import math

import numpy as np

import torch
import torch.nn.functional as F

try:
    from oracle.probpose_oracle import sparsemax_lastdim
except ImportError:      # loaded by path from tests/golden/make_goldens_head_grad.py
    sparsemax_lastdim = None

AUX = ("probability", "visibility", "oks", "error")
U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
SAMPLE_STEP = 251      # make_goldens_head_grad.py: every 251st element of an array over 256 elements


class _Clamp01(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, exclusive):
        ctx.save_for_backward(v)
        ctx.exclusive = exclusive
        return v.clamp(0, 1)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        m = ((v > 0) & (v < 1)) if ctx.exclusive else ((v >= 0) & (v <= 1))
        return g * m, None


class _Sparsemax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, nomean):
        p = sparsemax_lastdim(z) if sparsemax_lastdim is not None else _sparsemax_sort(z)
        ctx.save_for_backward(p)
        ctx.nomean = nomean
        return p

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        s = (p > 0).to(g.dtype)
        if ctx.nomean:
            return s * g, None
        return s * (g - (g * s).sum(-1, keepdim=True) / s.sum(-1, keepdim=True)), None


def _sparsemax_sort(z):
    zs = z - z.max(-1, keepdim=True).values
    srt = zs.sort(-1, descending=True).values
    k = torch.arange(1, z.shape[-1] + 1, dtype=z.dtype)
    cs = srt.cumsum(-1)
    kk = ((1 + k * srt) > cs).to(z.dtype) * k
    kmax = kk.max(-1, keepdim=True).values
    tau = (cs.gather(-1, kmax.long() - 1) - 1) / kmax
    return (zs - tau).clamp(min=0)


def bn_train(x, gamma, beta, rm, rv, eps, momentum, fault=None):
    """Train-mode BatchNorm2d on (B, C, h, w): returns (y, new running mean, new running var)."""
    n = x.shape[0] * x.shape[2] * x.shape[3]
    if n <= 1:
        raise ValueError("Expected more than 1 value per channel when training")
    mean = x.mean((0, 2, 3))
    d = x - mean.view(1, -1, 1, 1)
    var_b = (d * d).mean((0, 2, 3))
    var_u = var_b * n / (n - 1)
    var_n = var_u if fault == "unbiased_norm" else var_b
    y = d / torch.sqrt(var_n + eps).view(1, -1, 1, 1)
    if gamma is not None:
        y = y * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    var_r = var_b if fault == "biased_running" else var_u
    new_rm = (1 - momentum) * rm + momentum * mean.detach()
    new_rv = (1 - momentum) * rv + momentum * var_r.detach()
    return y, new_rm, new_rv


def maxpool(x, kh, kw, fault=None, decide=None):
    """MaxPool2d(kernel = stride = (kh, kw)), floor mode, ties to the first maximum in scan order (torch).
    ``decide`` (B, C, oh, ow) int64: the winning window position (ky * kw + kx) to take instead, where >= 0 -- a
    float32 forward's own pick, so that near-ties (values closer than its rounding) route the gradient alike; -1
    marks a window whose ReLU passed nothing there (head_forward then blocks it too)."""
    B, C, h, w = x.shape
    oh, ow = h // kh, w // kw
    win = x[:, :, :oh * kh, :ow * kw].reshape(B, C, oh, kh, ow, kw).permute(0, 1, 2, 4, 3, 5).reshape(B, C, oh, ow,
                                                                                                       kh * kw)
    if fault == "last_max":
        idx = kh * kw - 1 - win.detach().flip(-1).argmax(-1, keepdim=True)
    else:
        idx = win.detach().argmax(-1, keepdim=True)
    if decide is not None:      # the window positions a float32 forward picked (-1: keep this one's own pick)
        idx = torch.where(decide.unsqueeze(-1) >= 0, decide.unsqueeze(-1), idx)
    return win.gather(-1, idx).squeeze(-1)


def head_forward(sd, cfg, x, fault=None, inter=None):
    """sd: name -> float64 tensor (parameters with requires_grad as wanted, running buffers); cfg: dict(pools, n_deconv,
    normalize, detach_probability, detach_visibility, momentum, eps).  Returns (outputs, new running buffers);
    ``inter`` (a dict) receives, under their bias names, the outputs of the convolutions whose bias gradient is zero
    up to rounding (ahead of a train-mode BN; the final layer under Sparsemax)."""
    eps, mom = cfg.get("eps", 1e-5), cfg.get("momentum", 0.1)
    run = {}
    inter = {} if inter is None else inter

    def bn(prefix, t):
        y, rm, rv = bn_train(t, sd.get(prefix + "weight"), sd.get(prefix + "bias"), sd[prefix + "running_mean"],
                             sd[prefix + "running_var"], eps, mom, fault)
        run[prefix + "running_mean"], run[prefix + "running_var"] = rm, rv
        run[prefix + "num_batches_tracked"] = sd[prefix + "num_batches_tracked"] + 1
        return y

    t = x
    for i in range(cfg["n_deconv"]):
        t = F.conv_transpose2d(t, sd[f"deconv_layers.{3 * i}.weight"], stride=2, padding=1)
        t = torch.relu(bn(f"deconv_layers.{3 * i + 1}.", t))
    t = F.conv2d(t, sd["final_layer.weight"], sd["final_layer.bias"])
    if cfg.get("normalize") is not None:
        inter["final_layer.bias"] = t        # Sparsemax's backward sums to 0 over a map: so does this bias gradient
    B, K, H, W = t.shape
    t = t.reshape(B, K, H * W) / 0.5
    if cfg.get("normalize") is not None:
        t = _Sparsemax.apply(t, fault == "sparsemax_nomean") * cfg["normalize"]
    heat = _Clamp01.apply(t, fault == "exclusive_clamp").reshape(B, K, H, W)
    outs = [heat]
    for name in AUX:
        detach = {"probability": cfg.get("detach_probability", True) and fault != "no_prob_detach",
                  "visibility": cfg.get("detach_visibility", True)}.get(name, True)
        a = x.detach() if detach else x
        for i, (kh, kw) in enumerate(cfg["pools"]):
            a = F.conv2d(a, sd[f"{name}_layers.{4 * i}.weight"], sd[f"{name}_layers.{4 * i}.bias"], padding=1)
            inter[f"{name}_layers.{4 * i}.bias"] = a
            a = bn(f"{name}_layers.{4 * i + 1}.", a)
            decide = cfg.get("pool_decide", {}).get((name, i))
            a = maxpool(a, kh, kw, fault, decide)
            # the ReLU passes where the float32 forward's did (a maximum within its rounding of 0 decides alike)
            a = torch.relu(a) if decide is None else torch.where(decide >= 0, a, torch.zeros_like(a))
        n = len(cfg["pools"])
        a = F.conv2d(a, sd[f"{name}_layers.{4 * n}.weight"], sd[f"{name}_layers.{4 * n}.bias"])
        outs.append(torch.relu(a) if name == "error" else torch.sigmoid(a))
    return tuple(outs), run


def head_step(state, cfg, x, upstream, trainable=None, x_requires_grad=False, fault=None):
    """One train-mode forward + backward in float64.  state: name -> tensor (a state_dict); upstream: five upstream
    gradients (None = no gradient); trainable(name) -> bool.  Returns dict(outputs, grads {name: tensor}, x_grad,
    running {name: tensor})."""
    sd = {}
    for k, v in state.items():
        v = v.detach().clone()
        if v.is_floating_point():
            v = v.double()
            if not any(k.endswith(s) for s in ("running_mean", "running_var")) and (trainable is None or trainable(k)):
                v.requires_grad_(True)
        sd[k] = v
    xd = x.detach().double().clone().requires_grad_(x_requires_grad)
    inter = {}
    outs, run = head_forward(sd, cfg, xd, fault, inter)
    inter = {k: v for k, v in inter.items() if v.requires_grad}
    pairs = [(o, g.double()) for o, g in zip(outs, upstream) if g is not None and o.requires_grad]
    names = [k for k, v in sd.items() if v.requires_grad]
    leaves = [sd[k] for k in names] + ([xd] if x_requires_grad else []) + list(inter.values())
    if pairs:
        gr = torch.autograd.grad([o for o, _ in pairs], leaves, [g for _, g in pairs], allow_unused=True)
    else:
        gr = [None] * len(leaves)
    grads = {k: (g if g is not None else torch.zeros_like(sd[k])) for k, g in zip(names, gr)}
    xg = None
    if x_requires_grad:
        xg = gr[len(names)] if gr[len(names)] is not None else torch.zeros_like(xd)
    gi = gr[len(names) + (1 if x_requires_grad else 0):]
    # sum over rows of |dY| per channel: the absolute scale of a conv bias gradient ahead of a train-mode BN
    dy_mag = {k: (g.abs().sum((0, 2, 3)) if g is not None else torch.zeros(v.shape[1], dtype=torch.float64))
              for (k, v), g in zip(inter.items(), gi)}
    return dict(outputs=[o.detach() for o in outs], grads=grads, x_grad=xg, running=run, dy_mag=dy_mag)


def grad_class(name: str) -> str:
    if name.endswith("running_mean") or name.endswith("running_var"):
        return "stats"
    if "layers." in name and (name.endswith(".weight") or name.endswith(".bias")):
        idx = int(name.split(".")[1])
        if name.startswith("deconv_layers"):
            return "bn" if idx % 3 == 1 else "conv"
        if name.startswith("final_layer"):
            return "conv"
        return "bn" if idx % 4 == 1 else "conv"
    return "conv"


def ratio(got, want, u, c) -> float:
    """max |got - want| / (c u max|want|): <= 1 passes."""
    got, want = got.double().cpu(), want.double().cpu()
    mag = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    if not math.isfinite(err):
        return math.inf
    return err / max(c * u * mag, 1e-300) if mag > 0 else (0.0 if err == 0 else math.inf)


# ---- the golden cases (tests/golden/make_goldens_head_grad.py), rebuilt from their seeds with this package's head
CASES = {
    "T1": (64, 5, [(4, 3), (2, 2)], (8, 6), (64, 64), 41, {}, True, False),
    "T2": (64, 5, [(4, 3), (2, 2)], (8, 6), (64, 64), 42, {"detach_probability": False}, True, True),
    "T3": (64, 5, [(4, 3), (2, 2)], (8, 6), (64, 64), 43, {"freeze_error": True}, False, False),
    "T4": (64, 5, [(4, 3), (2, 2)], (8, 6), (64, 64), 44, {}, True, True),
}


def case(name, **extra):
    """(head (CPU, float32, this package's ProbMapHead), feats (B, C, h, w), upstream gradients, cfg,
    x_requires_grad) of a golden case: the upstream gradients are make_goldens_head_grad.py's float64 torch.randn of
    the five outputs' shapes, in order, from torch.Generator().manual_seed(seed + 200)."""
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.synthetic import synthetic_features, synthetic_head_state
    C, K, pools, (h, w), dec, seed, kw, synthetic, xg = CASES[name]
    kw = dict(kw, **extra)
    torch.manual_seed(seed)
    head = ProbMapHead(C, K, pools, dec, (4,) * len(dec), final_layer_kernel_size=1, **kw)
    if synthetic:
        head.load_state_dict(synthetic_head_state(C, K, n_pools=len(pools), deconv_out=dec, seed=seed), strict=False)
    feats = synthetic_features(2, C, h, w, seed=seed + 100)
    g = torch.Generator().manual_seed(seed + 200)
    H, W = h * 2 ** len(dec), w * 2 ** len(dec)
    ups = [torch.randn(shape, generator=g, dtype=torch.float64)
           for shape in [(2, K, H, W)] + [(2, K, 1, 1)] * 4]
    cfg = dict(pools=pools, n_deconv=len(dec), normalize=kw.get("normalize"),
               detach_probability=kw.get("detach_probability", True),
               detach_visibility=kw.get("detach_visibility", True))
    return head, feats, ups, cfg, xg


def trainable_of(head):
    req = {k: p.requires_grad for k, p in head.named_parameters()}
    return lambda k: req.get(k, False)


def golden_ratio(golden, key, t, tol=1e-9):
    """max relative deviation of t from a golden entry (whole array, or sum / abs sum / sample)."""
    a = t.detach().double().reshape(-1).numpy()
    if key in golden:
        want = golden[key].reshape(-1)
        return float(abs(a - want).max()) / (tol * max(float(abs(want).max()), 1e-30))
    s, asum, smp = golden[key + "#sum"], golden[key + "#abssum"], golden[key + "#sample"]
    r = abs(a.sum() - s) / (tol * max(asum, 1e-30))
    r = max(r, abs(abs(a).sum() - asum) / (tol * max(asum, 1e-30)))
    return float(max(r, abs(a[::SAMPLE_STEP] - smp).max() / (tol * max(float(abs(smp).max()), 1e-30))))


def golden_abs_ratio(golden, key, t, dy_mag, tol=1e-12):
    """A gradient that is zero up to rounding (a conv bias ahead of a train-mode BN): max |t - golden| against
    tol * sum over rows of |dY|, channel by channel."""
    a = t.detach().double().reshape(-1).numpy()
    want = golden[key].reshape(-1)
    return float((abs(a - want) / (tol * np.maximum(dy_mag.double().numpy(), 1e-30))).max())


def pool_decisions(saved, C, pools, B, h, w):
    """The window picks of the HIP training forward, {(branch name, stage): (B, C, oh, ow) int64} from the autograd
    node's saved state (pp_bn_pool_relu's argmax: element index into the stage's [B*h*w, 4C] rows, -1 where the ReLU
    passes nothing)."""
    out = {}
    ah, aw = h, w
    for i, (kh, kw) in enumerate(pools):
        am = saved["aux"][i]["argmax"].long().cpu()
        oh, ow = ah // kh, aw // kw
        row = torch.div(am, 4 * C, rounding_mode="floor")
        yy = torch.div(row, aw, rounding_mode="floor") % ah
        xx = row % aw
        oy = torch.arange(oh).view(1, oh, 1, 1).expand(B, oh, ow, 1).reshape(-1, 1)
        ox = torch.arange(ow).view(1, 1, ow, 1).expand(B, oh, ow, 1).reshape(-1, 1)
        pos = (yy - oy * kh) * kw + (xx - ox * kw)
        pos = torch.where(am >= 0, pos, torch.full_like(pos, -1)).view(B, oh, ow, 4, C)
        for bi, name in enumerate(AUX):
            out[(name, i)] = pos[..., bi, :].permute(0, 3, 1, 2).contiguous()
        ah, aw = oh, ow
    return out
