"""Float64 restatement of the fp8 compute mode of the ViT walk (engine.VitPlan with fp8=True), a comparator for the
record of one forward, and a torch emulation of the walk that produces the same record on the CPU.

What fp8 mode means, restated from the model's state dict and from recorded bf16 activations only (nothing the plan
stores is read here):

  weights   per output row of qkv / proj / fc1 / fc2:  sw = max(amax_row, 1e-12) / 448  (f32),
            w8 = e4m3(w / sw), the division in f32, round to nearest even;
  scales    for each of the four quantised activations of a block (h1 = LN1 output, ao = attention output, h2 = LN2
            output, hid = GELU output), from a bf16 pass over every calibration batch:
            amax = max(max |t| over all batches, 1e-6),  s = amax * margin / 448,  cs = sw * s for the linear that reads
            the point (engine._FP8_POINTS);
  stages    LN1 / LN2:   e4m3(clamp(LN(x) / s, +-448));
            qkv:         (h8 . w8^T) * cs + b -> bf16;
            attention:   softmax(q k^T hd^-0.5) v from the bf16 qkv -> bf16, or e4m3(clamp(. / s_ao, +-448)) with FP8_PROJ;
            proj:        bf16 GEMM (FP8_PROJ off) or (ao8 . w8^T) * cs + b, + the f32 residual -> f32;
            fc1:         e4m3(clamp(gelu((h8 . w8^T) * cs + b) / s_hid, +-448));
            fc2:         (hid8 . w8^T) * cs + b + the f32 residual -> f32;
            final LN:    bf16.
The clamp comes before the cast: torch's own cast turns anything above 464 into NaN, the kernels saturate.

A record is the list of launches of one forward, one dict per launch:
  op       "patch_embed" | "layernorm" | "linear" | "attention"
  args     name -> tensor as the launch read it (cloned before the call): x / gamma / beta; x / w / bias / residual /
           colscale; qkv
  scalars  eps, out_scale, epilogue, headmajor, B, N, heads, hd as passed
  out      the output after the call (cloned)
  ptrs     name -> address of every tensor argument and of "out"
`check_walk` holds a record to the restatement: the launch sequence and dtypes, the scale / column-scale / weights
each launch was handed, bit-identical dataflow between producer and consumer, and every stage's output against the
float64 value computed from that stage's recorded input, inside the bounds of gemm_reference / attention_reference."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

from tests import attention_reference as ar
from tests import gemm_reference as gr

FP8, FP8_MAX = gr.FP8, gr.FP8_MAX
BF16, F32 = torch.bfloat16, torch.float32
POINTS = ("h1", "ao", "h2", "hid")
LINEARS = dict(qkv="attn.qkv", proj="attn.proj", fc1="mlp.fc1", fc2="mlp.fc2")
BLOCK_ROLES = ("ln1", "qkv", "attention", "proj", "ln2", "fc1", "fc2")
LN_EPS = 1e-6                   # backbone.Block / VisionTransformer.norm
MIN_SCALE_GAP = 1.05            # input condition: the four activation scales of a block differ pairwise by >= 5 %
MIN_ROW_SPREAD = 2.0            # input condition: max sw / min sw of every linear


def e4m3(t: torch.Tensor, clamp: bool = True) -> torch.Tensor:
    """Round to e4m3 (nearest even) after saturating at +-448."""
    if clamp:
        t = t.clamp(-FP8_MAX, FP8_MAX)
    return t.float().to(FP8)


def half_step(y: torch.Tensor) -> torch.Tensor:
    """Half an e4m3 step at the magnitude of y (float64, stored domain): 2^-10 in the subnormal range (|y| < 2^-6)."""
    return torch.exp2(torch.floor(torch.log2(y.abs().clamp(min=2.0 ** -6))) - 4)


def quantize_rows(w: torch.Tensor):
    """[N, K] weights -> (w8 e4m3 [N, K], sw f32 [N])."""
    w32 = w.detach().float()
    sw = torch.clamp(w32.abs().amax(dim=1), min=1e-12) / FP8_MAX
    return e4m3(w32 / sw[:, None]), sw


def check_quantized_rows(w: torch.Tensor, w8: torch.Tensor, sw: torch.Tensor) -> list:
    """The properties of a per-row quantisation (w8, sw) of w; returns the list of violations."""
    bad = []
    wd, q, s = w.detach().double(), w8.float().double(), sw.double()
    if not bool(torch.isfinite(s).all()) or not bool((s > 0).all()) or not bool(torch.isfinite(q).all()):
        bad.append("a scale or a stored value is not finite / positive")
    amax, arg = wd.abs().max(dim=1)
    live = amax >= 1e-12
    top = q.abs().gather(1, arg[:, None])[:, 0]
    if not bool((top[live] == FP8_MAX).all()):
        bad.append(f"{int((top[live] != FP8_MAX).sum())} rows do not store their amax element as +-448")
    if not bool((q[amax == 0] == 0).all()):
        bad.append("an all-zero row stores a non-zero value")
    # half an e4m3 step at the stored magnitude; the f32 division adds up to 2^-24 |y|, doubled for the f32 scale
    y = wd / s[:, None]
    bound = (half_step(y) + y.abs() * 2.0 ** -23) * s[:, None]
    err = (q * s[:, None] - wd).abs()
    if not bool((err <= bound).all()):
        bad.append(f"{int((err > bound).sum())} elements are further than half an e4m3 step from w (worst "
                   f"{float((err / bound).max()):.3f} of the bound)")
    return bad


def roles(depth: int):
    seq = [("patch_embed", None)]
    for i in range(depth):
        seq += [(r, i) for r in BLOCK_ROLES]
    return seq + [("final_ln", None)]


_OP = dict(patch_embed="patch_embed", ln1="layernorm", ln2="layernorm", final_ln="layernorm", qkv="linear",
           proj="linear", fc1="linear", fc2="linear", attention="attention")
_POINT_OF = dict(ln1="h1", attention="ao", ln2="h2", fc1="hid")       # the role that writes each quantised activation


def activations(record, depth: int):
    """The four _FP8_POINTS activations of every block of a recorded walk: [block] -> {point: tensor}."""
    assert len(record) == len(roles(depth)), f"{len(record)} launches recorded, {len(roles(depth))} expected"
    acts = [dict() for _ in range(depth)]
    for e, (role, i) in zip(record, roles(depth)):
        if role in _POINT_OF:
            acts[i][_POINT_OF[role]] = e["out"]
    return acts


def condition_state(sd, depth: int):
    """A copy of a ViT state dict whose fp8 scales are told apart: the synthetic state gives LN1 and LN2 outputs of one
    amax and weight rows of nearly one scale, so a swapped activation scale or a dropped row scale would hide inside
    the bf16 bound.  LN2's gamma is scaled by 0.5, fc1's weight by 4, the v rows of qkv by 0.3 and every 16th row of
    each linear by 0.25: amax of about 4 (h1), 0.8 (ao), 1.8 (h2) and 8 (hid).  proj's weight is scaled by 0.25 and
    fc2's by 0.05 (a uniform factor leaves w8 as it is and goes into sw).

    The last two keep each block's update a small part of the residual stream (rms about 0.06 and 0.07 against a
    stream of rms 0.55), as it is in the deep blocks of a real pre-LN ViT.  The f32-output bound of
    gemm_reference.tolerance is 1e-4 of the OUTPUT's rms and presumes that the accumulation error of the product is
    negligible against it.  For e4m3 operands it is not once the product term carries the output: the scaled fp8 MFMA
    sums its 128 products at less than f32 precision, and its error follows sum_k |a_k w_k| cs, measured at 2^-15 to
    2^-17 of that sum on every tile form, with or without the residual.  With that sum at 10 - 15 times
    the output's rms (terms of the size the plain synthetic state gives them) single elements reach 1.1 - 1.4 of the
    bound; with rows x 4, LN2 x 1.7, fc1 x 1.5 (fc2's term 7 times the stream) 3.9."""
    sd = {k: v.clone() for k, v in sd.items()}
    for i in range(depth):
        p = f"blocks.{i}."
        sd[p + "norm2.weight"] *= 0.5
        sd[p + "mlp.fc1.weight"] *= 4.0
        sd[p + "mlp.fc2.weight"] *= 0.05
        sd[p + "attn.proj.weight"] *= 0.25
        for key in LINEARS.values():
            sd[p + key + ".weight"][::16] *= 0.25
        C = sd[p + "attn.proj.weight"].shape[0]
        sd[p + "attn.qkv.weight"][2 * C:] *= 0.3
    return sd


# The smallest models that still take every path.  A: M = 60 rows, ragged against every tile, head dim 64.  B: head dim
# 32 and N = 15 tokens (no multiple of 4); C = 256 with 8 heads, since the fp8 GEMM takes K in multiples of 128 only
# (C = 192 with 6 heads is refused).
MODELS = dict(A=dict(img=(64, 48), patch=16, C=128, heads=2, depth=2, B=5),
              B=dict(img=(80, 48), patch=16, C=256, heads=8, depth=2, B=3))


def model_state(cfg, seed: int = 0):
    from probpose_pytorch_amd.synthetic import synthetic_vit_state
    return condition_state(synthetic_vit_state(cfg["img"], cfg["patch"], cfg["C"], cfg["depth"], seed=seed), cfg["depth"])


def batches(cfg):
    """x1, x2 (plain crops), flat (low contrast) and bright (black / white pixels), cfg["B"] crops each."""
    from probpose_pytorch_amd.synthetic import synthetic_crops
    (H, W), B = cfg["img"], cfg["B"]
    g = torch.Generator().manual_seed(9)
    return dict(x1=synthetic_crops(B, H, W, seed=3), x2=synthetic_crops(B, H, W, seed=4) * 0.7,
                flat=synthetic_crops(B, H, W, seed=3) * 0.2 + 0.4,
                bright=(torch.rand((B, 3, H, W), generator=g) > 0.5).float())


class Restatement:
    """Weights, scales and column scales of fp8 mode from a state dict (timm names) and the recorded bf16 activations
    of the calibration batches (calib_acts[batch][block][point])."""

    def __init__(self, sd, depth: int, calib_acts, margin: float = None, device=None):
        from probpose_pytorch_amd import engine
        self.depth = depth
        self.margin = float(engine.FP8_MARGIN if margin is None else margin)
        self.reader = dict(engine._FP8_POINTS)
        dev = calib_acts[0][0]["h1"].device if device is None else device
        g = lambda k: sd[k].detach().to(dev)  # noqa: E731
        self.blocks = []
        for i in range(depth):
            p = f"blocks.{i}."
            b = dict(n1w=g(p + "norm1.weight").float(), n1b=g(p + "norm1.bias").float(),
                     n2w=g(p + "norm2.weight").float(), n2b=g(p + "norm2.bias").float())
            for lin, key in LINEARS.items():
                w = g(p + key + ".weight")
                b[lin + "_w"], b[lin + "_b"] = w.to(BF16), g(p + key + ".bias").float()
                b[lin + "_w8"], b[lin + "_sw"] = quantize_rows(w)
            for pt in POINTS:
                amax = max(max(float(batch[i][pt].double().abs().max()) for batch in calib_acts), 1e-6)
                b["amax_" + pt] = amax
                b["s_" + pt] = amax * self.margin / FP8_MAX
                lin = self.reader[pt]
                b[lin + "_cs"] = b[lin + "_sw"].double() * b["s_" + pt]
            self.blocks.append(b)
        self.nw, self.nb = g("norm.weight").float(), g("norm.bias").float()

    def input_condition(self) -> list:
        """Violations of the condition under which a swapped or dropped scale cannot hide."""
        bad = []
        for i, b in enumerate(self.blocks):
            s = sorted(b["s_" + pt] for pt in POINTS)
            gap = min(hi / lo for lo, hi in zip(s, s[1:]))
            if gap < MIN_SCALE_GAP:
                bad.append(f"block {i}: two activation scales differ by {gap:.3f}x only ({[b['s_' + p] for p in POINTS]})")
            for lin in LINEARS:
                sw = b[lin + "_sw"].double()
                if float(sw.max() / sw.min()) < MIN_ROW_SPREAD:
                    bad.append(f"block {i} {lin}: row scales spread by {float(sw.max() / sw.min()):.2f}x only")
        return bad


# ---------------------------------------------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Report:
    failures: list = field(default_factory=list)          # (tag, message); tags: sequence, scale, weight, dataflow, value
    worst: dict = field(default_factory=dict)             # stage kind -> max |d| / bound
    off: dict = field(default_factory=dict)               # e4m3 stage kind -> [outputs != rounded float64, outputs]
    mass: dict = field(default_factory=dict)              # fp8 GEMM -> f32: max sum_k |a w| cs / rms(out)
    err_per_mass: dict = field(default_factory=dict)      # fp8 GEMM -> f32: max |d| / max sum_k |a w| cs

    @property
    def ok(self):
        return not self.failures

    def tags(self):
        return {t for t, _ in self.failures}

    def fail(self, tag, msg):
        self.failures.append((tag, msg))

    def note(self, kind, ratio, got=None, y=None):
        self.worst[kind] = max(self.worst.get(kind, 0.0), ratio)
        if got is not None:
            n = self.off.setdefault(kind, [0, 0])
            n[0] += int((got.double().reshape(-1) != e4m3(y).double().reshape(-1)).sum())
            n[1] += got.numel()

    def summary(self) -> str:
        rows = [f"    {k:22s} worst d/bound {v:.3f}" +
                (f"   {self.off[k][0] / max(1, self.off[k][1]):.2%} of the e4m3 outputs differ from the rounded float64"
                 if k in self.off else "") +
                (f"   max sum|a w| cs = {self.mass[k]:.1f} rms(out), max |d| = 2^{math.log2(max(self.err_per_mass[k], 1e-30)):.1f} of it"
                 if k in self.mass else "") for k, v in sorted(self.worst.items())]
        return "\n".join(rows)

    def __str__(self):
        return "\n".join(f"[{t}] {m}" for t, m in self.failures) or "ok"


def _close(got, want, tol):
    return got is not None and abs(float(got) - want) <= tol * abs(want)


def _bits_equal(a, b):
    if a is None or b is None or a.dtype != b.dtype or a.shape != b.shape:
        return False
    bits = gr._BITS[a.dtype]
    return torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def linear_expected(x, w, bias, residual, colscale, out_scale, epilogue, out):
    """gemm_reference.expected_output of an ops.linear launch: (ref, written), 1-D like out."""
    M, Kd = x.shape
    N = w.shape[0]
    kw = dict(A=x, W=w, out=out, M=M, N=N, Kd=Kd, lda=Kd, ldw=Kd, ldc=N, bias=bias, residual=residual,
              epilogue=epilogue, colscale=colscale, out_scale=out_scale)
    return gr.expected_output(kw, torch.zeros(out.numel(), dtype=out.dtype, device=out.device))


def check_layernorm(rep, kind, e, gamma, beta, s):
    x, out = e["args"]["x"], e["out"]
    ref, term = ar.expected_layernorm(x, gamma, beta, LN_EPS)
    y, bound, band = ar.layernorm_target(ref, term, out.dtype, None if s is None else 1.0 / s)
    v = ar.compare(out.reshape(-1), torch.zeros_like(out).reshape(-1), 0, y, bound, band)
    rep.note(kind, v.worst, *((out, y) if out.dtype == FP8 else ()))
    if not v.ok:
        rep.fail("value", f"{kind}: {v}")


def check_attention(rep, kind, e, s):
    sc, out = e["scalars"], e["out"]
    ref, ref_abs = ar.expected_attention(e["args"]["qkv"], sc["B"], sc["N"], sc["heads"], sc["hd"])
    y, bound, band = ar.attention_target(ref, ref_abs, out.dtype, None if s is None else 1.0 / s)
    v = ar.compare(out.reshape(-1), torch.zeros_like(out).reshape(-1), 0, y, bound, band)
    rep.note(kind, v.worst, *((out, y) if out.dtype == FP8 else ()))
    if not v.ok:
        rep.fail("value", f"{kind}: {v}")


def check_linear(rep, kind, e, w, bias, colscale, out_scale):
    a, out = e["args"], e["out"]
    if a["x"].dtype != w.dtype:
        rep.fail("value", f"{kind}: the input is {a['x'].dtype}, the restated weight {w.dtype}: no product to compare")
        return
    ref, written = linear_expected(a["x"], w, bias, a.get("residual"), colscale, out_scale, e["scalars"]["epilogue"], out)
    got = out.reshape(-1)
    v = gr.compare(got, torch.zeros_like(got), ref, written, BF16)      # an fp8 GEMM is held to the bf16 bound
    rtol, atol = gr.tolerance(BF16, out.dtype, v.rms)
    d = (got.double() - ref).abs()
    ratio = d / (rtol * ref.abs() + atol)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    rep.note(kind, float(ratio.max()), *((out, ref) if out.dtype == FP8 else ()))
    if colscale is not None and out.dtype == F32:
        # a figure, not a check: the fp8 MFMA's error grows with sum_k |a_k w_k| cs, the bound with the output's rms
        mass = float(((a["x"].double().abs() @ w.double().abs().t()) * colscale.double()).max())
        rep.mass[kind] = max(rep.mass.get(kind, 0.0), mass / v.rms if v.rms else math.inf)
        rep.err_per_mass[kind] = max(rep.err_per_mass.get(kind, 0.0), float(d.max()) / mass)
    if not v.ok:
        rep.fail("value", f"{kind}: {v}")


def check_walk(record, R: Restatement, fp8_proj: bool, values: bool = True) -> Report:
    """Hold the record of one fp8 forward to the restatement R."""
    rep = Report()
    seq = roles(R.depth)
    if [e["op"] for e in record] != [_OP[r] for r, _ in seq]:
        rep.fail("sequence", f"launches {[e['op'] for e in record]} are not patch embed, {R.depth} x "
                             f"{BLOCK_ROLES}, final LayerNorm")
        return rep
    by = {(r, i): e for e, (r, i) in zip(record, seq)}

    def dtype_is(name, e, key, want):
        t = e["out"] if key == "out" else e["args"].get(key)
        got = None if t is None else t.dtype
        if got != want:
            rep.fail("sequence", f"{name}: {key} is {got}, expected {want}")

    def scale_is(name, e, want):
        got = e["scalars"].get("out_scale")
        if (want is None) != (got is None) or (want is not None and not _close(got, want, 1e-12)):
            rep.fail("scale", f"{name}: out_scale {got} passed, the restatement gives {want}")

    def colscale_is(name, e, want):
        got = e["args"].get("colscale")
        if (want is None) != (got is None):
            rep.fail("scale", f"{name}: colscale {'missing' if got is None else 'passed'}, the restatement says otherwise")
        elif want is not None:
            if got.shape != want.shape:
                rep.fail("scale", f"{name}: colscale of shape {tuple(got.shape)}")
                return
            rel = float(((got.double() - want).abs() / want.abs()).max())
            if not rel <= 2.0 ** -22:
                rep.fail("scale", f"{name}: colscale differs from sw * s by {rel:.3e} relative (bound 2^-22)")

    def weight_is(name, e, want):
        if not _bits_equal(e["args"].get("w"), want):
            rep.fail("weight", f"{name}: the weight operand is not the restated {want.dtype} matrix")

    def flows(name, e, key, src, src_key="out"):
        t = e["args"].get(key)
        u = src["out"] if src_key == "out" else src["args"].get(src_key)
        if not _bits_equal(t, u):
            rep.fail("dataflow", f"{name}: {key} is not bit-identical to what its producer left")
        pa, pb = e["ptrs"].get(key), src["ptrs"].get(src_key)
        if pa is not None and pb is not None and pa != pb:
            rep.fail("dataflow", f"{name}: {key} is read at {pa:#x}, its producer wrote {pb:#x}")

    p8 = FP8 if fp8_proj else BF16
    res = by[("patch_embed", None)]                  # the launch that last wrote the residual stream
    dtype_is("patch embed", res, "out", F32)
    for i, b in enumerate(R.blocks):
        n = lambda r: f"block {i} {r}"  # noqa: E731
        ln1, qkv, att, proj, ln2, fc1, fc2 = (by[(r, i)] for r in BLOCK_ROLES)
        # dtypes
        for e, r, xd, od in ((ln1, "ln1", F32, FP8), (qkv, "qkv", FP8, BF16), (proj, "proj", p8, F32), (ln2, "ln2", F32, FP8),
                             (fc1, "fc1", FP8, FP8), (fc2, "fc2", FP8, F32)):
            dtype_is(n(r), e, "x", xd)
            dtype_is(n(r), e, "out", od)
        dtype_is(n("attention"), att, "qkv", BF16)
        dtype_is(n("attention"), att, "out", p8)
        for e, r, g_, b_ in ((ln1, "ln1", "n1w", "n1b"), (ln2, "ln2", "n2w", "n2b")):
            if not (_bits_equal(e["args"]["gamma"], b[g_]) and _bits_equal(e["args"]["beta"], b[b_])
                    and e["scalars"]["eps"] == LN_EPS):
                rep.fail("weight", f"{n(r)}: gamma / beta / eps are not the block's")
        for e, r in ((qkv, "qkv"), (proj, "proj"), (fc1, "fc1"), (fc2, "fc2")):
            if not _bits_equal(e["args"].get("bias"), b[r + "_b"]):
                rep.fail("weight", f"{n(r)}: the bias is not the layer's")
        gelu = {r: bool(e["scalars"].get("epilogue", 0) & gr.EPI_GELU) for e, r in ((qkv, "qkv"), (proj, "proj"), (fc1, "fc1"), (fc2, "fc2"))}
        if gelu != dict(qkv=False, proj=False, fc1=True, fc2=False):
            rep.fail("sequence", f"block {i}: GELU epilogues {gelu}")
        # scales, column scales, weights handed to each launch
        scale_is(n("ln1"), ln1, b["s_h1"])
        scale_is(n("ln2"), ln2, b["s_h2"])
        scale_is(n("attention"), att, b["s_ao"] if fp8_proj else None)
        scale_is(n("fc1"), fc1, b["s_hid"])
        for e, r in ((qkv, "qkv"), (proj, "proj"), (fc2, "fc2")):
            scale_is(n(r), e, None)
        for e, r in ((qkv, "qkv"), (fc1, "fc1"), (fc2, "fc2")):
            colscale_is(n(r), e, b[r + "_cs"])
            weight_is(n(r), e, b[r + "_w8"])
        colscale_is(n("proj"), proj, b["proj_cs"] if fp8_proj else None)
        weight_is(n("proj"), proj, b["proj_w8"] if fp8_proj else b["proj_w"])
        # dataflow
        flows(n("ln1"), ln1, "x", res)
        flows(n("qkv"), qkv, "x", ln1)
        flows(n("attention"), att, "qkv", qkv)
        flows(n("proj"), proj, "x", att)
        flows(n("proj"), proj, "residual", res)
        flows(n("ln2"), ln2, "x", proj)
        flows(n("fc1"), fc1, "x", ln2)
        flows(n("fc2"), fc2, "x", fc1)
        flows(n("fc2"), fc2, "residual", proj)
        for e, r in ((proj, "proj"), (fc2, "fc2")):
            if e["ptrs"].get("residual") != e["ptrs"].get("out"):
                rep.fail("dataflow", f"{n(r)}: the residual is not added in place")
        res = fc2
        if not values:
            continue
        # stage values from each launch's own recorded input
        check_layernorm(rep, "LayerNorm -> e4m3", ln1, b["n1w"], b["n1b"], b["s_h1"])
        check_linear(rep, "fp8 GEMM -> bf16", qkv, b["qkv_w8"], b["qkv_b"], b["qkv_cs"], None)
        if fp8_proj:
            check_attention(rep, "attention -> e4m3", att, b["s_ao"])
            check_linear(rep, "fp8 GEMM + res -> f32", proj, b["proj_w8"], b["proj_b"], b["proj_cs"], None)
        else:
            check_attention(rep, "attention -> bf16", att, None)
            check_linear(rep, "bf16 GEMM + res -> f32", proj, b["proj_w"], b["proj_b"], None, None)
        check_layernorm(rep, "LayerNorm -> e4m3", ln2, b["n2w"], b["n2b"], b["s_h2"])
        check_linear(rep, "fp8 GEMM gelu -> e4m3", fc1, b["fc1_w8"], b["fc1_b"], b["fc1_cs"], b["s_hid"])
        check_linear(rep, "fp8 GEMM + res -> f32", fc2, b["fc2_w8"], b["fc2_b"], b["fc2_cs"], None)
    fin = by[("final_ln", None)]
    dtype_is("final LayerNorm", fin, "x", F32)
    dtype_is("final LayerNorm", fin, "out", BF16)
    scale_is("final LayerNorm", fin, None)
    if not (_bits_equal(fin["args"]["gamma"], R.nw) and _bits_equal(fin["args"]["beta"], R.nb)):
        rep.fail("weight", "final LayerNorm: gamma / beta are not the model's")
    flows("final LayerNorm", fin, "x", res)
    if values:
        check_layernorm(rep, "LayerNorm -> bf16", fin, R.nw, R.nb, None)
    return rep


def saturation(record) -> dict:
    """Over the e4m3 outputs of a record: NaN bytes (0x7F / 0xFF), elements at +-448, elements in all."""
    nan = sat = n = 0
    for e in record:
        if e["out"].dtype == FP8:
            b = e["out"].view(torch.uint8)
            nan += int(((b & 0x7F) == 0x7F).sum())
            sat += int(((b & 0x7F) == 0x7E).sum())
            n += b.numel()
    return dict(nan=nan, saturated=sat, elements=n)


# ---------------------------------------------------------------------------------------------------------------
# torch emulation of the walk
# ---------------------------------------------------------------------------------------------------------------
FAULTS = ("swap_s_h1_s_h2", "cs_without_sw", "cs_from_previous_amax", "margin_1", "margin_twice", "last_batch_amax",
          "calibrate_keeps_old_max", "fc2_reads_other_rows", "no_clamp", "proj_gets_s_ao_after_bf16_attention")


class EmulatedPlan:
    """engine.VitPlan's fp8 bookkeeping and launch sequence in plain torch: every stage computed in float64 from the
    stage's input and rounded once to the dtype the kernel stores (`exact`: only the e4m3 quantisations round, every
    other stage stays float64: the free-running float64 walk).  `fault` plants one of FAULTS."""

    def __init__(self, sd, cfg, fault: str = None, exact: bool = False):
        from probpose_pytorch_amd import ops
        assert fault is None or fault in FAULTS
        self.fault, self.exact = fault, exact
        self.patch, self.C, self.heads, self.depth = cfg["patch"], cfg["C"], cfg["heads"], cfg["depth"]
        H, W = cfg["img"]
        self.gh, self.gw = H // self.patch, W // self.patch
        self.N = self.gh * self.gw
        self.dev = sd["pos_embed"].device
        self.pe = (sd["patch_embed.proj.weight"].reshape(self.C, -1).to(BF16), sd["patch_embed.proj.bias"].float(),
                   sd["pos_embed"].reshape(-1, self.C).float())
        self.blocks = []
        for i in range(self.depth):
            p = f"blocks.{i}."
            b = dict(n1w=sd[p + "norm1.weight"].float(), n1b=sd[p + "norm1.bias"].float(),
                     n2w=sd[p + "norm2.weight"].float(), n2b=sd[p + "norm2.bias"].float(), amax={}, old_amax={})
            for lin, key in LINEARS.items():
                w = sd[p + key + ".weight"]
                b[lin + "_w"], b[lin + "_b"] = w.to(BF16), sd[p + key + ".bias"].float()
                b[lin + "_w8"], b[lin + "_sw"] = ops.quantize_rows_fp8(w)
            self.blocks.append(b)
        self.nw, self.nb = sd["norm.weight"].float(), sd["norm.bias"].float()
        self.stale = {}                  # what an earlier, larger batch left in the e4m3 twins

    # -- calibration ---------------------------------------------------------------------------------------------
    def calibrate(self, batches, margin: float = None):
        from probpose_pytorch_amd import engine
        for b in self.blocks:
            b["old_amax"] = dict(b["amax"])
            if self.fault != "calibrate_keeps_old_max":
                b["amax"] = {}
        margin = engine.FP8_MARGIN if margin is None else margin
        if self.fault == "margin_1":
            margin = 1.0
        for x in batches:
            acts = activations(self.walk(x, fp8=False), self.depth)
            for b, act in zip(self.blocks, acts):
                for pt in POINTS:
                    prev = 0.0 if self.fault == "last_batch_amax" else b["amax"].get(pt, 0.0)
                    a = b["amax"][pt] = max(float(act[pt].float().abs().max()), 1e-6, prev)
                    s = a * margin / FP8_MAX
                    if self.fault == "margin_twice":
                        s *= margin
                    b["s_" + pt] = s
                    lin = engine._FP8_POINTS[pt]
                    if self.fault == "cs_from_previous_amax":
                        s = b["old_amax"].get(pt, a) * margin / FP8_MAX
                    b[lin + "_cs"] = torch.full_like(b[lin + "_sw"], s) if self.fault == "cs_without_sw" \
                        else (b[lin + "_sw"] * s).contiguous()
        return self

    def adopt(self, R: "Restatement"):
        """Take the restatement's scales and column scales instead of calibrating (the free-running float64 walk)."""
        for b, rb in zip(self.blocks, R.blocks):
            for pt in POINTS:
                b["s_" + pt] = rb["s_" + pt]
            for lin in LINEARS:
                b[lin + "_cs"] = rb[lin + "_cs"]
        return self

    # -- stages --------------------------------------------------------------------------------------------------
    def _store(self, v, dtype, s=None):
        if dtype == FP8:
            return e4m3(v / s, clamp=self.fault != "no_clamp")
        return v if self.exact else v.to(dtype)

    def _entry(self, rec, op, args, scalars, out, names):
        ptrs = {k: hash(v) & 0xFFFFFFF0 for k, v in names.items()}
        rec.append(dict(op=op, args={k: v for k, v in args.items() if v is not None}, scalars=scalars, out=out, ptrs=ptrs))
        return out

    def _ln(self, rec, x, gamma, beta, dtype, s, xname, oname):
        ref, _ = ar.expected_layernorm(x, gamma, beta, LN_EPS)
        return self._entry(rec, "layernorm", dict(x=x, gamma=gamma, beta=beta), dict(eps=LN_EPS, out_scale=s),
                           self._store(ref, dtype, s), dict(x=xname, out=oname))

    def _linear(self, rec, x, w, bias, dtype, xname, oname, residual=None, colscale=None, out_scale=None, epilogue=0):
        v = x.double() @ w.double().t()
        if colscale is not None:
            v = v * colscale.double()
        v = v + bias.double()
        if epilogue & gr.EPI_GELU:
            v = gr._gelu(v)
        if residual is not None:
            v = v + residual.double()
        names = dict(x=xname, out=oname, **({"residual": oname} if residual is not None else {}))
        return self._entry(rec, "linear", dict(x=x, w=w, bias=bias, residual=residual, colscale=colscale),
                           dict(epilogue=epilogue, out_scale=out_scale, headmajor=None), self._store(v, dtype, out_scale),
                           names)

    def _attention(self, rec, qkv, B, dtype, s, oname):
        ref, _ = ar.expected_attention(qkv, B, self.N, self.heads, self.C // self.heads)
        return self._entry(rec, "attention", dict(qkv=qkv),
                           dict(B=B, N=self.N, heads=self.heads, hd=self.C // self.heads, out_scale=s, headmajor=False),
                           self._store(ref, dtype, s), dict(qkv="qkv", out=oname))

    def walk(self, x, fp8: bool = True, fp8_proj: bool = False):
        """The record of one forward of x (B, 3, H, W): bf16 (the calibration pass) or fp8."""
        B, p = x.shape[0], self.patch
        rec = []
        a0 = x.reshape(B, 3, self.gh, p, self.gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * self.N, 3 * p * p).to(BF16)
        w, bias, pos = self.pe
        xres = a0.double() @ w.double().t() + bias.double() + pos.double().repeat(B, 1)
        xres = self._entry(rec, "patch_embed", {}, {}, self._store(xres, F32), dict(out="xres"))
        q8 = "8" if fp8 else ""
        p8 = "8" if fp8 and fp8_proj else ""
        act, pact = (FP8 if fp8 else BF16), (FP8 if p8 else BF16)
        M = B * self.N
        for b in self.blocks:
            s = b if fp8 else {}
            sp = s if p8 else {}
            s_h1, s_h2 = s.get("s_h1"), s.get("s_h2")
            if fp8 and self.fault == "swap_s_h1_s_h2":
                s_h1, s_h2 = s_h2, s_h1
            h = self._ln(rec, xres, b["n1w"], b["n1b"], act, s_h1, "xres", "h" + q8)
            qkv = self._linear(rec, h, b["qkv_w" + q8], b["qkv_b"], BF16, "h" + q8, "qkv", colscale=s.get("qkv_cs"))
            ao = self._attention(rec, qkv, B, pact, sp.get("s_ao"), "ao" + p8)
            if fp8 and self.fault == "proj_gets_s_ao_after_bf16_attention":
                stale = torch.zeros((M, self.C), device=self.dev).to(FP8)        # the e4m3 twin nobody wrote
                xres = self._linear(rec, stale, b["proj_w8"], b["proj_b"], F32, "ao8", "xres", residual=xres,
                                    colscale=b["proj_cs"])
            else:
                xres = self._linear(rec, ao, b["proj_w" + p8], b["proj_b"], F32, "ao" + p8, "xres", residual=xres,
                                    colscale=sp.get("proj_cs"))
            h = self._ln(rec, xres, b["n2w"], b["n2b"], act, s_h2, "xres", "h" + q8)
            hid = self._linear(rec, h, b["fc1_w" + q8], b["fc1_b"], act, "h" + q8, "hid" + q8, colscale=s.get("fc1_cs"),
                               out_scale=s.get("s_hid"), epilogue=gr.EPI_GELU)
            read = hid
            if fp8 and self.fault == "fc2_reads_other_rows" and id(b) in self.stale and self.stale[id(b)].shape[0] > M:
                read = self.stale[id(b)][-M:].clone()        # rows of the larger batch that ran before
            if fp8:
                self.stale[id(b)] = hid
            xres = self._linear(rec, read, b["fc2_w" + q8], b["fc2_b"], F32, "hid" + q8, "xres", residual=xres,
                                colscale=s.get("fc2_cs"))
        self._ln(rec, xres, self.nw, self.nb, BF16, None, "xres", "feats")
        return rec
