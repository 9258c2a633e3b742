"""Float64 restatement of the bf16 and fp32 forward walks (engine.VitPlan without fp8, engine.HeadPlan), comparators
for the record of one forward (tests/walk_recording.py), and torch emulations of both walks that produce the same
record on the CPU, clean or with one planted bookkeeping fault.

Everything is restated from the state dict (timm / reference parameter names) and from the recorded activations:
nothing a plan stores is read, and no pack.* function restates an operand.  (The emulations play the plan's part, so
they do build derived operands with pack.*, the way fp8_walk_reference.EmulatedPlan uses ops.quantize_rows_fp8.)

ViT walk (`check_vit_walk`), tags as in fp8_walk_reference.check_walk plus `layer`:
  sequence  the ops in order, the dtype of every operand and output, GELU on fc1 only, the headmajor scalars, no
            out_scale / colscale anywhere;
  weight    bit equality of every operand with the state-dict tensor cast to the compute dtype (LayerNorm parameters
            and biases f32), the patch-embed operand [C, 3 p p], rowbias = pos_embed with period N, and for the fused
            launch w_hm / b_hm = the head-major permutation as an index formula (row 192 h + 64 t + j <- t C + 64 h + j);
  dataflow  every stage reads, at the same address, bit for bit what its producer left; proj / fc2 add in place;
  value     every stage against float64 of its own recorded input inside the per-kernel bounds of gemm_reference /
            attention_reference; patchify bit-exact against an unfold;
  layer     the patch-embed GEMM output against float64 F.conv2d(x, w, stride=p) + bias + pos of the recorded crops.

Head walk (`check_head_walk`): the GEMM operands are derived state (BN fold, taps-major layout, deconvolution parities,
the 4C concatenation of the aux branches) and are not restated bit for bit.  Each GEMM stage gets two holds: `value`
(gemm_reference.expected_output of the launch's own arguments) and `layer` (the float64 layer, evaluated with
torch.nn.functional from the state-dict parameters on the recorded input re-laid from channels-last rows to NCHW).

The `layer` bound, per element:   rtol |ref| + atol   +   (u_w + c 2^-24) (|x| * |w64|)
  * rtol, atol = gemm_reference.tolerance(compute dtype, output dtype, rms(ref)): the kernel term;
  * u_w = 2^-8 for bf16 operands, 0 for f32.  bf16 keeps 8 significant bits; round to nearest moves w by at most half
    a unit in the last place, 2^-8 2^e for w in [2^e, 2^(e+1)), which is 2^-8 |w| at the bottom of a binade (1 + 2^-8
    rounds to 1: 2^-8 / (1 + 2^-8) of it).  2^-9, the figure this bound was specified with, is the mean case and not a
    bound: the exactly rounded emulation leaves it on short sums (K = 64: 1.02; tests/test_walk_reference.py pins
    that).  Every layer hold also reports its worst ratio under 2^-9, as "... [u_w 2^-9]";
  * c = the float32 roundings an operand element has been through in pack.fold_bn.  That function computes in float64
    and rounds twice, `wf = (w * scale).float()` and `bf = ((b0 - mean) * scale + beta).float()`: one rounding per
    weight element and one per bias element, so c = 1 for a layer with a BatchNorm and c = 0 for the final layer and
    the aux 1x1 layers (their f32 parameters are only cast to the compute dtype);
  * |x| * |w64| is the same layer on absolute values: |x| against |w scale| plus |folded bias| (float64, eps included),
    divided by T where the layer divides.  ReLU, clamp and max pooling are 1-Lipschitz and keep the bound.
  The patch embedding rounds both operands (the patch matrix and the weight): (2 u_w + u_w^2) (|x| * |w|), c = 0.
  The fused final layer (PP_EPI_FUSE_FINAL) is two layers in one launch with a bf16 map between them: the first
  layer's bound e1 goes through the 1x1 layer as (e1 * |wf|) / T, plus u_w ((|y| + e1) * |wf|) / T for the rounding of wf,
  plus the kernel term of the second layer.  e1's kernel term is that of an f32 output (the map is accumulated in f32)
  plus its one rounding to bf16, u_w |y|.  The `value` hold has the same form on the launch's own operands.
  A split-K aux stage is held after its pooling: the kernel terms of the S partials added, max-pooled, plus (S + 1)
  float32 additions (S - 1 of partials, the bias; one to spare for the order) of at most 2^-24 (|x| * |w64|) each, plus
  one rounding of the output, 2^-8 |ref| (bf16) or 2^-24 |ref| (f32).
There is no share of elements and no mean anywhere."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import attention_reference as ar
from tests import fp8_walk_reference as fw
from tests import gemm_reference as gr
from tests import head_forward_reference as hr
from tests.walk_recording import gemm_kw

BF16, F32 = torch.bfloat16, torch.float32
LN_EPS = fw.LN_EPS
BN_EPS = 1e-5                    # nn.BatchNorm2d's default: the head never passes another
TEMPERATURE = 0.5                # head.py: self.temperature
LINEARS = fw.LINEARS
AUX_NAMES = ("probability", "visibility", "oks", "error")
TWO_KERNEL = ("ln1", "qkv", "attention", "proj", "ln2", "fc1", "fc2")
FUSED = ("ln1", "qkv_attention", "proj", "ln2", "fc1", "fc2")
_OP = dict(patchify="patchify", patch_embed="patch_embed", ln1="layernorm", ln2="layernorm", final_ln="layernorm",
           qkv="linear", proj="linear", fc1="linear", fc2="linear", attention="attention", qkv_attention="qkv_attention")
_bits_equal = fw._bits_equal


def u_of(dtype) -> float:
    """The unit roundoff of an operand in `dtype` against its f32 value: 2^-8 for bf16, 0 for f32 (module docstring)."""
    return 2.0 ** -8 if dtype == BF16 else 0.0


U_ISSUE = 2.0 ** -9              # the bf16 figure the walk tests were first specified with; reported next to every layer hold


# ---------------------------------------------------------------------------------------------------------------
# input condition
# ---------------------------------------------------------------------------------------------------------------
MIN_EPS_SHARE = 1e-4             # some channel of every BatchNorm has eps / (2 var) above this


def _norm_role(key, sd):
    """"weight" | "bias" | "running_mean" | "running_var" if `key` is a LayerNorm / BatchNorm tensor, else None."""
    prefix, _, leaf = key.rpartition(".")
    if prefix + ".running_mean" in sd:
        return leaf if leaf in ("weight", "bias", "running_mean", "running_var") else None
    last = prefix.rpartition(".")[2]
    return leaf if last in ("norm", "norm1", "norm2") and leaf in ("weight", "bias") else None


def input_condition(sd) -> list:
    """Violations of the condition under which an exchanged or an untouched parameter cannot hide: no two same-shaped
    tensors of the state are bit-equal, no LayerNorm / BatchNorm tensor is at its 0 / 1 initial value, and every
    BatchNorm has a channel where eps is at least MIN_EPS_SHARE of 2 var (a fold without eps moves that channel by
    that share, above the fp32 kernel bound of 2e-5)."""
    bad, seen = [], {}
    for k, v in sd.items():
        for k2, v2 in seen.setdefault((v.dtype, tuple(v.shape)), []):
            if torch.equal(v, v2):
                bad.append(f"{k} and {k2} are bit-equal")
        seen[(v.dtype, tuple(v.shape))].append((k, v))
        role = _norm_role(k, sd)
        if role in ("weight", "running_var") and bool((v == 1).all()):
            bad.append(f"{k} is all ones")
        if role in ("bias", "running_mean") and bool((v == 0).all()):
            bad.append(f"{k} is all zeros")
        if role == "running_var" and float((BN_EPS / (2 * v.double())).max()) < MIN_EPS_SHARE:
            bad.append(f"{k}: eps is at most {float((BN_EPS / (2 * v.double())).max()):.1e} of 2 var in every channel")
    return bad


def condition_head_state(sd):
    """A copy of a synthetic head state that meets input_condition: the synthetic recipe leaves every
    num_batches_tracked at 0 (equal tensors) and draws running_var from [0.5, 1.5], where eps = 1e-5 is 3e-6 to 1e-5 of
    2 var, inside the fp32 kernel bound.  Every BatchNorm's num_batches_tracked becomes its own number, and every
    8th channel (from 3) gets running_var x 0.02 and gamma x sqrt(0.02): the channel's output is as before, eps is now
    2e-4 to 5e-4 of 2 var."""
    sd = {k: v.clone() for k, v in sd.items()}
    n = 0
    for k in list(sd):
        if k.endswith(".running_var"):
            p = k[: -len("running_var")]
            n += 1
            sd[p + "num_batches_tracked"] = torch.tensor(n, dtype=torch.long)
            sd[k][3::8] *= 0.02
            sd[p + "weight"][3::8] *= math.sqrt(0.02)
    return sd


# ---------------------------------------------------------------------------------------------------------------
# models, states and inputs of the tests
# ---------------------------------------------------------------------------------------------------------------
DT = {"bf16": BF16, "fp32": F32}
# The smallest models that still take each path, depth 2 everywhere (the cases of tests/test_walk_gpu.py).  V1 and V4 are
# the geometries of fp8_walk_reference.MODELS; the heads A, B, C are test_oracle_goldens.HEAD_VARIANTS.
VIT = dict(V1=dict(img=(64, 48), patch=16, C=128, heads=2, depth=2, B=5),
           V2=dict(img=(256, 192), patch=16, C=128, heads=2, depth=2, B=2),
           V3=dict(img=(384, 288), patch=16, C=320, heads=4, depth=2, B=1),
           V4=dict(img=(80, 48), patch=16, C=256, heads=8, depth=2, B=3))
POOLS = [(4, 3), (2, 2), (2, 2)]
HEADS = dict(A=dict(C=128, K=17, pools=POOLS, hw=(16, 12), dec=(64, 64), conv=(64,), ck=(3,), fk=3, seed=21),
             B=dict(C=128, K=17, pools=POOLS, hw=(16, 12), dec=(64,), conv=(64, 17), ck=(3, 1), fk=None, seed=22),
             C=dict(C=64, K=5, pools=[(4, 3), (2, 2)], hw=(8, 6), dec=(), conv=(64,), ck=(1,), fk=1, seed=23),
             default=dict(C=128, K=17, pools=POOLS, hw=(16, 12), dec=(256, 256), conv=(), ck=(), fk=1, seed=24))
HEADS["normalize"] = dict(HEADS["default"], normalize=1.0)


def vit_state(cfg, seed=0):
    from probpose_pytorch_amd.synthetic import synthetic_vit_state
    sd = dict(synthetic_vit_state(cfg["img"], cfg["patch"], cfg["C"], cfg["depth"], seed=seed))
    assert input_condition(sd) == [], input_condition(sd)
    return sd


def crops(cfg, B=None):
    from probpose_pytorch_amd.synthetic import synthetic_crops
    return synthetic_crops(B or cfg["B"], *cfg["img"], seed=3)


def head_state(spec, condition=True):
    from probpose_pytorch_amd.synthetic import synthetic_head_state
    sd = dict(synthetic_head_state(spec["C"], spec["K"], n_pools=len(spec["pools"]), deconv_out=spec["dec"],
                                   seed=spec["seed"], final_kernel=spec["fk"], conv_out=spec["conv"],
                                   conv_kernels=spec["ck"]))
    if not condition:
        return sd
    sd = condition_head_state(sd)
    assert input_condition(sd) == [], input_condition(sd)
    return sd


def head_feats(spec, dtype, B=2):
    from probpose_pytorch_amd.synthetic import synthetic_features
    h, w = spec["hw"]
    f = synthetic_features(B, spec["C"], h, w, seed=spec["seed"] + 100)
    return f.permute(0, 2, 3, 1).reshape(B * h * w, spec["C"]).to(dtype).contiguous(), B, h, w



# ---------------------------------------------------------------------------------------------------------------
# report
# ---------------------------------------------------------------------------------------------------------------
class Report(fw.Report):
    """fp8_walk_reference.Report that also keeps the stage of each failure: failures are (tag, message), stages the
    parallel list of stage names ("block 1 qkv", "aux stage 0", ...)."""

    def __init__(self):
        super().__init__()
        self.stages = []

    def fail(self, tag, msg, stage=None):
        self.failures.append((tag, msg))
        self.stages.append(stage if stage is not None else msg.split(":")[0])

    def failed_stages(self):
        return set(self.stages)


def _ratio(d, bound):
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)


def _hold(rep, tag, kind, stage, got, ref, bound):
    """|got - ref| <= bound for every element (a NaN never passes); notes the worst ratio under `kind`."""
    d = (got.double().reshape(-1) - ref.reshape(-1)).abs()
    bound = bound.reshape(-1)
    bad = int((~(d <= bound)).sum())
    worst = float(_ratio(d, bound).max()) if d.numel() else 0.0
    rep.note(kind, worst)
    if bad:
        rep.fail(tag, f"{stage}: {kind}: {bad} of {d.numel()} elements outside the bound, worst d / bound {worst:.3g}", stage)


def _gemm_value(rep, kind, stage, kw, out, compute):
    """gemm_reference.expected_output of the keyword set kw against `out`, through gemm_reference.compare."""
    got = out.reshape(-1)
    before = torch.zeros_like(got)
    ref, written = gr.expected_output(kw, before)
    if not bool(written.all()):
        rep.fail("value", f"{stage}: the launch writes {int(written.sum())} of the {got.numel()} elements of its output", stage)
        return
    v = gr.compare(got, before, ref, written, compute)
    rtol, atol = gr.tolerance(compute, out.dtype, v.rms)
    rep.note(kind, float(_ratio((got.double() - ref).abs(), rtol * ref.abs() + atol).max()))
    if not v.ok:
        rep.fail("value", f"{stage}: {kind}: {v}", stage)


def _rms(t):
    return float(t.double().square().mean().sqrt()) if t.numel() else 0.0


def _kernel_term(ref, compute, out_dtype):
    rtol, atol = gr.tolerance(compute, out_dtype, _rms(ref))
    return rtol * ref.abs() + atol


def linear_kw(x, w, bias, out, residual=None, epilogue=0, headmajor=None):
    M, Kd = x.shape
    N = w.shape[0]
    if residual is not None:
        epilogue |= gr.EPI_OUT_F32
    return dict(A=x, W=w, out=out, M=M, N=N, Kd=Kd, lda=Kd, ldw=Kd, ldc=N, bias=bias, residual=residual,
                epilogue=epilogue, headmajor=headmajor)


# ---------------------------------------------------------------------------------------------------------------
# ViT: restatement
# ---------------------------------------------------------------------------------------------------------------
def headmajor_index(C: int, heads: int) -> torch.Tensor:
    """idx with w_hm[r] = w[idx[r]]: row 192 h + 64 t + j of the head-major copy is row t C + 64 h + j of qkv.weight."""
    idx = torch.empty(3 * C, dtype=torch.long)
    for h in range(heads):
        for t in range(3):
            for j in range(64):
                idx[192 * h + 64 * t + j] = t * C + 64 * h + j
    return idx


class VitRestatement:
    """The operands of the bf16 / fp32 ViT walk from a state dict.  cfg: img (H, W), patch, C, heads, depth."""

    def __init__(self, sd, cfg, dtype, device=None):
        self.cfg, self.dtype, self.depth = cfg, dtype, cfg["depth"]
        self.patch, self.C, self.heads = cfg["patch"], cfg["C"], cfg["heads"]
        self.hd = self.C // self.heads
        (H, W), p = cfg["img"], cfg["patch"]
        self.gh, self.gw = H // p, W // p
        self.N = self.gh * self.gw
        dev = sd["pos_embed"].device if device is None else device
        g = lambda k: sd[k].detach().to(dev)  # noqa: E731
        self.conv_w, self.conv_b = g("patch_embed.proj.weight"), g("patch_embed.proj.bias")
        self.pe_w = self.conv_w.reshape(self.C, 3 * p * p).to(dtype).contiguous()
        self.pe_b = self.conv_b.float()
        self.pos = g("pos_embed").reshape(self.N, self.C).float()
        self.blocks = []
        for i in range(self.depth):
            q = f"blocks.{i}."
            b = dict(n1w=g(q + "norm1.weight").float(), n1b=g(q + "norm1.bias").float(),
                     n2w=g(q + "norm2.weight").float(), n2b=g(q + "norm2.bias").float())
            for lin, key in LINEARS.items():
                b[lin + "_w"], b[lin + "_b"] = g(q + key + ".weight").to(dtype), g(q + key + ".bias").float()
            if self.hd == 64:
                idx = headmajor_index(self.C, self.heads).to(dev)
                b["qkv_w_hm"], b["qkv_b_hm"] = b["qkv_w"][idx].contiguous(), b["qkv_b"][idx].contiguous()
            self.blocks.append(b)
        self.nw, self.nb = g("norm.weight").float(), g("norm.bias").float()
        # engine.VitPlan: bf16 models whose head rows are not whole 128-byte lines and that run the streaming attention
        self.headmajor = dtype == BF16 and (self.hd == 80 or (self.hd == 32 and self.N > 192))

    def patch_layer(self, x):
        """(ref, |x| * |w|) of the patch embedding as rows [B N, C] float64: conv2d(stride p) + bias + pos."""
        p, B = self.patch, x.shape[0]
        w, b, pos = self.conv_w.double(), self.conv_b.double(), self.pos.double()
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * self.N, self.C)  # noqa: E731
        ref = rows(F.conv2d(x.double(), w, b, stride=p)) + pos.repeat(B, 1)
        mass = rows(F.conv2d(x.double().abs(), w.abs(), None, stride=p))
        return ref, mass


def vit_roles(depth: int, mode: str):
    blk = dict(two_kernel=TWO_KERNEL, fused=FUSED)[mode]
    return ([("patchify", None), ("patch_embed", None)] + [(r, i) for i in range(depth) for r in blk]
            + [("final_ln", None)])


def _check_ln(rep, stage, e, gamma, beta):
    x, out = e["args"]["x"], e["out"]
    ref, term = ar.expected_layernorm(x, gamma, beta, LN_EPS)
    y, bound, band = ar.layernorm_target(ref, term, out.dtype, None)
    v = ar.compare(out.reshape(-1), torch.zeros_like(out).reshape(-1), 0, y, bound, band)
    rep.note(f"LayerNorm -> {_dt(out.dtype)}", v.worst)
    if not v.ok:
        rep.fail("value", f"{stage}: {v}", stage)


def _check_att(rep, stage, kind, out, qkv, B, N, heads, hd, headmajor):
    ref, ref_abs = ar.expected_attention(qkv, B, N, heads, hd, headmajor)
    y, bound, band = ar.attention_target(ref, ref_abs, out.dtype, None)
    v = ar.compare(out.reshape(-1), torch.zeros_like(out).reshape(-1), 0, y, bound, band)
    rep.note(kind, v.worst)
    if not v.ok:
        rep.fail("value", f"{stage}: {v}", stage)


def _dt(d):
    return str(d)[6:]


def check_vit_walk(record, R: VitRestatement, mode: str, values: bool = True) -> Report:
    """Hold the record of one bf16 / fp32 ViT forward (mode "two_kernel" or "fused") to the restatement R."""
    rep = Report()
    seq = vit_roles(R.depth, mode)
    if [e["op"] for e in record] != [_OP[r] for r, _ in seq]:
        rep.fail("sequence", f"launches {[e['op'] for e in record]} are not patchify, patch embed, {R.depth} x "
                             f"{dict(two_kernel=TWO_KERNEL, fused=FUSED)[mode]}, final LayerNorm", "walk")
        return rep
    by = {(r, i): e for e, (r, i) in zip(record, seq)}
    dt, C, N, heads, hd = R.dtype, R.C, R.N, R.heads, R.hd
    cdt = _dt(dt)

    def dtype_is(stage, e, key, want):
        t = e["out"] if key == "out" else e["args"].get(key)
        got = None if t is None else t.dtype
        if got != want:
            rep.fail("sequence", f"{stage}: {key} is {got}, expected {want}", stage)

    def plain(stage, e):
        if e["scalars"].get("out_scale") is not None or e["args"].get("colscale") is not None:
            rep.fail("sequence", f"{stage}: an out_scale or a colscale in a {cdt} walk", stage)

    def operand_is(stage, e, key, want, what):
        if not _bits_equal(e["args"].get(key), want):
            rep.fail("weight", f"{stage}: {what}", stage)

    def flows(stage, e, key, src, src_key="out"):
        t = e["args"].get(key)
        u = src["out"] if src_key == "out" else src["args"].get(src_key)
        if not _bits_equal(t, u):
            rep.fail("dataflow", f"{stage}: {key} is not bit-identical to what its producer left", stage)
        pa, pb = e["ptrs"].get(key), src["ptrs"].get(src_key)
        if pa is not None and pb is not None and pa != pb:
            rep.fail("dataflow", f"{stage}: {key} is read at {pa:#x}, its producer wrote {pb:#x}", stage)

    # ---- patchify and the patch embedding
    pf, pe = by[("patchify", None)], by[("patch_embed", None)]
    x = pf["args"]["x"]
    B = x.shape[0]
    M = B * N
    dtype_is("patchify", pf, "out", dt)
    if pf["scalars"]["patch"] != R.patch or tuple(pf["out"].shape) != (M, 3 * R.patch ** 2):
        rep.fail("sequence", f"patchify: patch {pf['scalars']['patch']}, output {tuple(pf['out'].shape)}", "patchify")
    sc = pe["scalars"]
    K0 = 3 * R.patch ** 2
    want = dict(M=M, N=C, Kd=K0, lda=K0, ldw=K0, ldc=C, epilogue=gr.EPI_OUT_F32)
    if {k: sc.get(k) for k in want} != want or set(pe["args"]) != {"A", "W", "bias", "rowbias"}:
        rep.fail("sequence", f"patch embed: called with {sc} and operands {sorted(pe['args'])}", "patch embed")
    dtype_is("patch embed", pe, "out", F32)
    operand_is("patch embed", pe, "W", R.pe_w, f"W is not patch_embed.proj.weight as [C, 3 p p] in {cdt}")
    operand_is("patch embed", pe, "bias", R.pe_b, "the bias is not patch_embed.proj.bias")
    operand_is("patch embed", pe, "rowbias", R.pos, "rowbias is not pos_embed [N, C]")
    if sc.get("rowbias_period") != N:
        rep.fail("weight", f"patch embed: pos_embed applied with period {sc.get('rowbias_period')}, N = {N}", "patch embed")
    flows("patch embed", pe, "A", pf)
    if values:
        if not _bits_equal(pf["out"], hr.patchify_ref(x, R.patch, dt)):
            rep.fail("value", "patchify: the patch matrix is not the unfold of the crops", "patchify")
        if sc.get("rowbias_period") == N:                 # another period reads past pos_embed: reported above
            _gemm_value(rep, f"{cdt} GEMM rowbias -> f32", "patch embed", gemm_kw(pe), pe["out"], dt)
        ref, mass = R.patch_layer(x)
        u = u_of(dt)
        _hold(rep, "layer", f"layer: patch embed {cdt}", "patch embed", pe["out"], ref,
              _kernel_term(ref, dt, F32) + (2 * u + u * u) * mass)

    # ---- the blocks
    res = pe                                          # the launch that last wrote the residual stream
    hm = (heads, hd) if R.headmajor else None
    for i, b in enumerate(R.blocks):
        n = lambda r: f"block {i} {r}"  # noqa: E731
        g = {r: by[(r, i)] for r in (TWO_KERNEL if mode == "two_kernel" else FUSED)}
        ln1, proj, ln2, fc1, fc2 = g["ln1"], g["proj"], g["ln2"], g["fc1"], g["fc2"]
        lins = [(proj, "proj"), (fc1, "fc1"), (fc2, "fc2")]
        if mode == "two_kernel":
            qkv, att = g["qkv"], g["attention"]
            lins.insert(0, (qkv, "qkv"))
        else:
            qa = g["qkv_attention"]
        for e, r in ((ln1, "ln1"), (ln2, "ln2")):
            dtype_is(n(r), e, "x", F32)
            dtype_is(n(r), e, "out", dt)
            plain(n(r), e)
        for e, r in lins:
            dtype_is(n(r), e, "x", dt)
            dtype_is(n(r), e, "w", dt)
            dtype_is(n(r), e, "out", F32 if r in ("proj", "fc2") else dt)
            plain(n(r), e)
            want_epi = gr.EPI_GELU if r == "fc1" else 0
            if e["scalars"].get("epilogue", 0) != want_epi:
                rep.fail("sequence", f"{n(r)}: epilogue {e['scalars'].get('epilogue')}, expected {want_epi} (GELU on fc1 "
                                     "only)", n(r))
            want_hm = hm if r == "qkv" else None
            got_hm = e["scalars"].get("headmajor")
            if (None if got_hm is None else tuple(got_hm)) != want_hm:
                rep.fail("sequence", f"{n(r)}: headmajor {got_hm}, expected {want_hm}", n(r))
            if (e["args"].get("residual") is not None) != (r in ("proj", "fc2")):
                rep.fail("sequence", f"{n(r)}: residual {'passed' if r not in ('proj', 'fc2') else 'missing'}", n(r))
            operand_is(n(r), e, "w", b[r + "_w"], f"the weight operand is not {LINEARS[r]}.weight in {cdt}")
            operand_is(n(r), e, "bias", b[r + "_b"], "the bias is not the layer's")
        for e, r, gk, bk in ((ln1, "ln1", "n1w", "n1b"), (ln2, "ln2", "n2w", "n2b")):
            if not (_bits_equal(e["args"]["gamma"], b[gk]) and _bits_equal(e["args"]["beta"], b[bk])
                    and e["scalars"]["eps"] == LN_EPS):
                rep.fail("weight", f"{n(r)}: gamma / beta / eps are not the block's", n(r))
        flows(n("ln1"), ln1, "x", res)
        if mode == "two_kernel":
            dtype_is(n("attention"), att, "qkv", dt)
            dtype_is(n("attention"), att, "out", dt)
            plain(n("attention"), att)
            sa = att["scalars"]
            if (sa["B"], sa["N"], sa["heads"], sa["hd"], bool(sa["headmajor"])) != (B, N, heads, hd, R.headmajor):
                rep.fail("sequence", f"{n('attention')}: called with {sa}", n("attention"))
            flows(n("qkv"), qkv, "x", ln1)
            flows(n("attention"), att, "qkv", qkv)
            flows(n("proj"), proj, "x", att)
        else:
            for key in ("h", "w_hm", "out"):
                dtype_is(n("qkv_attention"), qa, key, BF16)
            if (qa["scalars"]["B"], qa["scalars"]["heads"]) != (B, heads):
                rep.fail("sequence", f"{n('qkv_attention')}: called with {qa['scalars']}", n("qkv_attention"))
            operand_is(n("qkv_attention"), qa, "w_hm", b.get("qkv_w_hm"), "w_hm is not the head-major permutation of "
                       "attn.qkv.weight (row 192 h + 64 t + j <- row t C + 64 h + j)")
            operand_is(n("qkv_attention"), qa, "b_hm", b.get("qkv_b_hm"), "b_hm is not the head-major permutation of "
                       "attn.qkv.bias")
            flows(n("qkv_attention"), qa, "h", ln1)
            flows(n("proj"), proj, "x", qa)
        flows(n("proj"), proj, "residual", res)
        flows(n("ln2"), ln2, "x", proj)
        flows(n("fc1"), fc1, "x", ln2)
        flows(n("fc2"), fc2, "x", fc1)
        flows(n("fc2"), fc2, "residual", proj)
        for e, r in ((proj, "proj"), (fc2, "fc2")):
            if e["ptrs"].get("residual") != e["ptrs"].get("out"):
                rep.fail("dataflow", f"{n(r)}: the residual is not added in place", n(r))
        res = fc2
        if not values:
            continue
        _check_ln(rep, n("ln1"), ln1, b["n1w"], b["n1b"])
        _check_ln(rep, n("ln2"), ln2, b["n2w"], b["n2b"])
        for e, r in lins:
            a = e["args"]
            if a["x"].dtype != b[r + "_w"].dtype:
                continue                                  # reported under sequence
            kind = f"{cdt} GEMM" + dict(qkv=" headmajor" if hm else "", proj=" + res", fc1=" gelu", fc2=" + res")[r] + \
                f" -> {_dt(e['out'].dtype)}"
            kw = linear_kw(a["x"], b[r + "_w"], b[r + "_b"], e["out"], a.get("residual"), e["scalars"].get("epilogue", 0),
                           e["scalars"].get("headmajor"))
            _gemm_value(rep, kind, n(r), kw, e["out"], dt)
        if mode == "two_kernel":
            _check_att(rep, n("attention"), f"attention{' headmajor' if R.headmajor else ''} -> {cdt}", att["out"],
                       att["args"]["qkv"], B, N, heads, hd, bool(att["scalars"]["headmajor"]))
        else:
            # float64 qkv from the recorded h and the restated ROW-MAJOR weight, rounded to bf16 where the kernel rounds
            q64 = (qa["args"]["h"].double() @ b["qkv_w"].double().t() + b["qkv_b"].double()).to(BF16)
            _check_att(rep, n("qkv_attention"), "qkv + attention -> bf16", qa["out"], q64, B, N, heads, hd, False)
    fin = by[("final_ln", None)]
    dtype_is("final LayerNorm", fin, "x", F32)
    dtype_is("final LayerNorm", fin, "out", dt)
    plain("final LayerNorm", fin)
    if not (_bits_equal(fin["args"]["gamma"], R.nw) and _bits_equal(fin["args"]["beta"], R.nb)
            and fin["scalars"]["eps"] == LN_EPS):
        rep.fail("weight", "final LayerNorm: gamma / beta / eps are not the model's", "final LayerNorm")
    flows("final LayerNorm", fin, "x", res)
    if values:
        _check_ln(rep, "final LayerNorm", fin, R.nw, R.nb)
    return rep


# ---------------------------------------------------------------------------------------------------------------
# head: restatement
# ---------------------------------------------------------------------------------------------------------------
def rows_to_nchw(x, B, h, w):
    return x.reshape(B, h, w, -1).permute(0, 3, 1, 2).double()


def nchw_to_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def final_heatmap_fits(cin, K, dtype):
    """include/probpose_hip.h: pp_final_heatmap takes a 1x1 final layer when 64 padded rows and the weight fit 150 KiB."""
    es = 2 if dtype == BF16 else 4
    return 64 * (cin * es + 16) + K * cin * es <= 150 * 1024


class HeadRestatement:
    """The float64 layers of a ProbMapHead from its state dict.  spec: C, K, pools, dec, conv, ck, fk, normalize (the
    constructor arguments); geometry (B, h, w) of the features; the engine switches the forward ran under."""

    def __init__(self, sd, spec, dtype, B, h, w, splitk_aux=True, fuse_final=True, device=None):
        self.spec, self.dtype, self.B, self.h, self.w = spec, dtype, B, h, w
        self.C, self.K = spec["C"], spec["K"]
        self.pools = [tuple(p) for p in spec["pools"]]
        self.dec, self.conv, self.ck, self.fk = tuple(spec["dec"]), tuple(spec["conv"]), tuple(spec["ck"]), spec["fk"]
        self.normalize = spec.get("normalize")
        self.splitk_aux, self.fuse_final = splitk_aux, fuse_final
        dev = next(iter(sd.values())).device if device is None else device
        self.sd = {k: v.detach().to(dev).double() for k, v in sd.items() if v.is_floating_point()}

    # -- what the walk must look like --------------------------------------------------------------------------
    def ending(self) -> str:
        """Which form ends the heatmap branch."""
        widths = [self.C] + list(self.dec) + list(self.conv)
        if self.fk is None:
            return "heatmap"                        # Identity final layer: the last layer's epilogue stores the maps
        if (self.fuse_final and self.dec and not self.conv and self.dtype == BF16 and self.dec[-1] == 256
                and self.fk == 1 and self.K <= 32):
            return "fuse_final"
        if self.fk == 1 and final_heatmap_fits(widths[-1], self.K, self.dtype):
            return "final_heatmap"
        return "final_gemm"

    def split_of(self, stage: int) -> int:
        from probpose_pytorch_amd import head_calls
        return head_calls.aux_split(stage) if stage > 0 and self.splitk_aux else 1

    def sequence(self):
        """[(op, stage name)] in host order: the aux branch, then the heatmap branch."""
        seq = []
        for i in range(len(self.pools)):
            seq += [("gemm", f"aux stage {i}"), ("maxpool_relu_sum" if self.split_of(i) > 1 else "maxpool_relu", f"aux pool {i}")]
        seq.append(("aux_tail", "aux tail"))
        seq += [("gemm", f"deconv {i}") for i in range(len(self.dec))] + [("gemm", f"conv {i}") for i in range(len(self.conv))]
        end = self.ending()
        if end == "final_heatmap":
            seq.append(("final_heatmap", "final"))
        elif end == "final_gemm":
            seq.append(("gemm", "final"))
        if self.normalize is not None:
            seq.append(("sparsemax_rows", "sparsemax"))
        return seq

    # -- float64 layers: (ref, |x| * |w64|), NCHW ---------------------------------------------------------------
    def _bn(self, prefix, y):
        s = self.sd
        return F.batch_norm(y, s[prefix + "running_mean"], s[prefix + "running_var"], s[prefix + "weight"],
                            s[prefix + "bias"], False, 0.0, BN_EPS)

    def _fold_abs(self, prefix, conv_bias):
        """(|scale|, |folded bias|) of the BatchNorm at `prefix`, float64."""
        s = self.sd
        scale = s[prefix + "weight"] / torch.sqrt(s[prefix + "running_var"] + BN_EPS)
        b0 = conv_bias if conv_bias is not None else torch.zeros_like(scale)
        return scale.abs(), ((b0 - s[prefix + "running_mean"]) * scale + s[prefix + "bias"]).abs()

    def deconv_layer(self, i, x):
        w = self.sd[f"deconv_layers.{3 * i}.weight"]
        ref = torch.relu(self._bn(f"deconv_layers.{3 * i + 1}.", F.conv_transpose2d(x, w, stride=2, padding=1)))
        sa, ba = self._fold_abs(f"deconv_layers.{3 * i + 1}.", None)
        mass = F.conv_transpose2d(x.abs(), w.abs() * sa[None, :, None, None], stride=2, padding=1) + ba[None, :, None, None]
        return ref, mass

    def conv_layer(self, i, x):
        w, b = self.sd[f"conv_layers.{3 * i}.weight"], self.sd[f"conv_layers.{3 * i}.bias"]
        pad = (self.ck[i] - 1) // 2
        ref = torch.relu(self._bn(f"conv_layers.{3 * i + 1}.", F.conv2d(x, w, b, padding=pad)))
        sa, ba = self._fold_abs(f"conv_layers.{3 * i + 1}.", b)
        mass = F.conv2d(x.abs(), w.abs() * sa[:, None, None, None], None, padding=pad) + ba[None, :, None, None]
        return ref, mass

    def heat_tail(self, ref, mass):
        """/ T and the clamp (off when the Sparsemax normalisation follows)."""
        ref, mass = ref / TEMPERATURE, mass / TEMPERATURE
        return (ref.clamp(0.0, 1.0) if self.normalize is None else ref), mass

    def final_layer(self, x):
        w, b = self.sd["final_layer.weight"], self.sd["final_layer.bias"]
        ref = F.conv2d(x, w, b, padding=self.fk // 2)
        mass = F.conv2d(x.abs(), w.abs(), None, padding=self.fk // 2) + b.abs()[None, :, None, None]
        return self.heat_tail(ref, mass)

    def aux_layer(self, i, x):
        """conv3x3 + BN of the four branches in AUX_NAMES order: x [B, C, h, w] (stage 0, shared) or [B, 4C, h, w]."""
        C = self.C
        refs, masses = [], []
        for br, name in enumerate(AUX_NAMES):
            xb = x if i == 0 else x[:, br * C:(br + 1) * C]
            w, b = self.sd[f"{name}_layers.{4 * i}.weight"], self.sd[f"{name}_layers.{4 * i}.bias"]
            refs.append(self._bn(f"{name}_layers.{4 * i + 1}.", F.conv2d(xb, w, b, padding=1)))
            sa, ba = self._fold_abs(f"{name}_layers.{4 * i + 1}.", b)
            masses.append(F.conv2d(xb.abs(), w.abs() * sa[:, None, None, None], None, padding=1) + ba[None, :, None, None])
        return torch.cat(refs, 1), torch.cat(masses, 1)

    def aux_tail_layer(self, x):
        """x [B, 4C] rows -> (ref [4, B, K], mass): the four 1x1 layers and their activations."""
        C, n = self.C, len(self.pools)
        refs, masses = [], []
        for br, name in enumerate(AUX_NAMES):
            w = self.sd[f"{name}_layers.{4 * n}.weight"].reshape(self.K, C)
            b = self.sd[f"{name}_layers.{4 * n}.bias"]
            xb = x[:, br * C:(br + 1) * C].double()
            pre = xb @ w.t() + b
            refs.append(torch.relu(pre) if name == "error" else torch.sigmoid(pre))
            masses.append(xb.abs() @ w.abs().t() + b.abs())
        return torch.stack(refs), torch.stack(masses)


def _pool_nchw(t, p):
    return F.max_pool2d(t, kernel_size=p, stride=p)


def fuse_final_value(e, compute):
    """(ref [B, K, HW] float64, bound) of a PP_EPI_FUSE_FINAL launch from its own arguments: the deconvolution by
    gemm_reference.expected_output into a virtual [4M, 256] map, its kernel term e1 carried through the 1x1 layer,
    plus the kernel term of that layer (module docstring)."""
    kw = gemm_kw(e)
    K, HW, T, clamp = e["scalars"]["fuse_final"]
    M4, cout = 4 * kw["M"], kw["N"]
    dev = e["out"].device
    kw["out"] = torch.zeros((M4, cout), dtype=compute, device=dev)
    y, written = gr.expected_output(kw, torch.zeros(M4 * cout, dtype=compute, device=dev))
    assert bool(written.all())
    y = y.reshape(M4, cout)
    e1 = _kernel_term(y, compute, F32) + u_of(compute) * y.abs()
    wf, bf = e["args"]["final_w"].double(), e["args"]["final_b"].double()
    z, ez = (y @ wf.t() + bf) / T, (e1 @ wf.abs().t()) / abs(T)
    if clamp:
        z = z.clamp(0.0, 1.0)
    lay = lambda t: t.reshape(M4 // HW, HW, K).permute(0, 2, 1).contiguous()  # noqa: E731
    z, ez = lay(z), lay(ez)
    stored = (y.to(compute).double() @ wf.t() + bf) / T              # what a launch with an exact first layer stores
    return z, ez + _kernel_term(z, compute, F32), lay(stored.clamp(0.0, 1.0) if clamp else stored)


def check_head_walk(record, R: HeadRestatement, outputs=None, values: bool = True) -> Report:
    """Hold the record of one bf16 / fp32 ProbMapHead forward to the restatement R.  outputs: the forward's 5-tuple
    (heatmaps, prob, vis, oks, err), when the caller has it."""
    from probpose_pytorch_amd import head_calls
    rep = Report()
    seq = R.sequence()
    if [e["op"] for e in record] != [op for op, _ in seq]:
        rep.fail("sequence", f"launches {[e['op'] for e in record]}, expected {seq} (the heatmap branch ends with "
                             f"{R.ending()})", "walk")
        return rep
    by = {name: e for e, (_, name) in zip(record, seq)}
    dt, B, C, K = R.dtype, R.B, R.C, R.K
    cdt, u = _dt(dt), u_of(dt)
    clamp = R.normalize is None
    end = R.ending()

    def flows(stage, e, key, src, src_key="out"):
        t = e["args"].get(key)
        s = src["out"] if src_key == "out" else src["args"].get(src_key)
        if t is not None and s is not None and t.numel() == s.numel():
            t, s = t.reshape(-1), s.reshape(-1)             # sparsemax_rows sees the maps as [B K, H W]
        if not _bits_equal(t, s):
            rep.fail("dataflow", f"{stage}: {key} is not bit-identical to what its producer left", stage)
        pa, pb = e["ptrs"].get(key), src["ptrs"].get(src_key)
        if pa is not None and pb is not None and pa != pb:
            rep.fail("dataflow", f"{stage}: {key} is read at {pa:#x}, its producer wrote {pb:#x}", stage)

    def call_is(stage, e, want, epilogue, operands):
        sc = e["scalars"]
        got = {k: sc.get(k) for k in want}
        if got != want:
            rep.fail("sequence", f"{stage}: called with {got}, expected {want}", stage)
        if sc.get("epilogue", 0) != epilogue:
            rep.fail("sequence", f"{stage}: epilogue {sc.get('epilogue', 0)}, expected {epilogue}", stage)
        if sc.get("splitk", 1) != want.get("splitk", 1):
            rep.fail("sequence", f"{stage}: splitk {sc.get('splitk', 1)}, expected {want.get('splitk', 1)}", stage)
        if set(e["args"]) != set(operands):
            rep.fail("sequence", f"{stage}: operands {sorted(e['args'])}, expected {sorted(operands)}", stage)
        for k in ("A", "W"):
            if e["args"][k].dtype != dt:
                rep.fail("sequence", f"{stage}: {k} is {e['args'][k].dtype}, expected {dt}", stage)

    def layer_hold(stage, kind, got, ref, mass, out_dtype, c):
        _hold(rep, "layer", f"layer: {kind}", stage, got, ref, _kernel_term(ref, dt, out_dtype) + (u + c * 2.0 ** -24) * mass)
        if u:
            d = (got.double().reshape(-1) - ref.reshape(-1)).abs()
            rep.note(f"layer: {kind} [u_w 2^-9]", float(_ratio(d, (_kernel_term(ref, dt, out_dtype)
                                                                    + (U_ISSUE + c * 2.0 ** -24) * mass).reshape(-1)).max()))

    # ---- aux branch
    feats = by["aux stage 0"]["args"]["A"]
    ah, aw = R.h, R.w
    prev = None
    for i, p in enumerate(R.pools):
        st, ps = f"aux stage {i}", f"aux pool {i}"
        ge, pe = by[st], by[ps]
        M = B * ah * aw
        S = R.split_of(i)
        if i == 0:
            call_is(st, ge, head_calls.aux_stage0(M, C), 0, ("A", "W", "bias", "rowoff"))
        elif S > 1:
            call_is(st, ge, head_calls.aux_stage(M, C, split=S), gr.EPI_OUT_F32, ("A", "W", "rowoff"))
        else:
            call_is(st, ge, head_calls.aux_stage(M, C), 0, ("A", "W", "bias", "rowoff"))
        want_out = F32 if S > 1 else dt
        if ge["out"].dtype != want_out or pe["out"].dtype != dt:
            rep.fail("sequence", f"{st}: writes {ge['out'].dtype}, its pooling {pe['out'].dtype}", st)
        geo = dict(B=B, h=ah, w=aw, Cc=4 * C, kh=p[0], kw=p[1])
        if pe["scalars"] != geo:
            rep.fail("sequence", f"{ps}: called with {pe['scalars']}, expected {geo}", ps)
        if prev is not None:
            flows(st, ge, "A", prev)
        flows(ps, pe, "parts" if S > 1 else "x", ge)
        oh, ow = ah // p[0], aw // p[1]
        if values:
            x = rows_to_nchw(ge["args"]["A"], B, ah, aw)
            ref, mass = R.aux_layer(i, x)
            if S > 1:
                kw = gemm_kw(ge)
                _gemm_value(rep, f"{cdt} GEMM split-K -> f32", st, kw, ge["out"], dt)
                parts, bias = pe["args"]["parts"], pe["args"]["bias"]
                want = hr.maxpool_relu_sum_ref(parts.reshape(S, -1), bias, B, ah, aw, 4 * C, p[0], p[1], dt)
                if not _bits_equal(pe["out"], want.reshape(pe["out"].shape)):
                    rep.fail("value", f"{ps}: not the sequential float32 sum of the partials + bias, pooled", ps)
                # layer, after the pooling (module docstring)
                pref, _ = gr.expected_output(kw, torch.zeros(ge["out"].numel(), dtype=F32, device=ge["out"].device))
                pref = pref.reshape(S, M, 4 * C)
                term = sum(_kernel_term(pref[s], dt, F32) for s in range(S))
                bound = rows_to_nchw(term, B, ah, aw) + (u + (1 + S + 1) * 2.0 ** -24) * mass
                lref = torch.relu(_pool_nchw(ref, p))
                lbound = _pool_nchw(bound, p) + (u if dt == BF16 else 2.0 ** -24) * lref.abs()
                _hold(rep, "layer", f"layer: aux conv3x3 + BN split-K, pooled {cdt}", ps, pe["out"], nchw_to_rows(lref),
                      nchw_to_rows(lbound))
            else:
                _gemm_value(rep, f"{cdt} GEMM gather -> {cdt}", st, gemm_kw(ge), ge["out"], dt)
                layer_hold(st, f"aux conv3x3 + BN {cdt}", ge["out"], nchw_to_rows(ref), nchw_to_rows(mass), dt, 1)
                xin = pe["args"]["x"]
                want = nchw_to_rows(torch.relu(_pool_nchw(rows_to_nchw(xin, B, ah, aw), p))).to(dt)
                if not _bits_equal(pe["out"], want.reshape(pe["out"].shape)):
                    rep.fail("value", f"{ps}: not relu(max_pool2d) of its input", ps)
        prev, ah, aw = pe, oh, ow
    te = by["aux tail"]
    if te["scalars"] != dict(B=B, Cc=C, K=K) or tuple(te["out"].shape) != (4, B, K) or te["out"].dtype != F32:
        rep.fail("sequence", f"aux tail: called with {te['scalars']}, output {tuple(te['out'].shape)}", "aux tail")
    flows("aux tail", te, "x", prev)
    if values:
        a = te["args"]
        want = hr.aux_tail_ref(a["x"], a["w"], a["bias"])
        _hold(rep, "value", "aux tail", "aux tail", te["out"], want, 1e-5 + 1e-5 * want.abs())
        ref, mass = R.aux_tail_layer(a["x"])
        _hold(rep, "layer", f"layer: aux 1x1 + activation {cdt}", "aux tail", te["out"], ref,
              1e-5 + 1e-5 * ref.abs() + u * mass)
    if outputs is not None:
        base = te["ptrs"]["out"]
        for i, t in enumerate(outputs[1:]):
            if t.data_ptr() != base + 4 * i * B * K or not torch.equal(t.reshape(B, K), te["out"][i]):
                rep.fail("dataflow", f"aux tail: output {AUX_NAMES[i]} is not row {i} of the [4, B, K] tensor", "aux tail")

    # ---- heatmap branch
    heat_stages = [f"deconv {i}" for i in range(len(R.dec))] + [f"conv {i}" for i in range(len(R.conv))]
    if "final" in by:
        heat_stages.append("final")
    first = by[heat_stages[0]]
    flows(heat_stages[0], first, "x" if first["op"] == "final_heatmap" else "A", by["aux stage 0"], "A")
    hh, ww, cin = R.h, R.w, C
    prev = None
    last = heat_stages[-1]
    for st in heat_stages:
        e = by[st]
        kind_, _, idx = st.partition(" ")
        idx = int(idx) if idx else None
        x_key = "x" if e["op"] == "final_heatmap" else "A"
        if prev is not None:
            flows(st, e, x_key, prev)
        x = rows_to_nchw(e["args"][x_key], B, hh, ww) if values else None
        M = B * hh * ww
        ends = st == last and end in ("fuse_final", "heatmap")          # this layer's epilogue stores the maps
        if kind_ == "deconv":
            cout = R.dec[idx]
            ops_ = ("A", "W", "bias", "rowoff", "out_rowmap") + (("final_w", "final_b") if ends and end == "fuse_final" else ())
            call_is(st, e, head_calls.deconv(M, cin, cout), gr.EPI_RELU, ops_)
            HWo = 4 * hh * ww
            if values:
                ref, mass = R.deconv_layer(idx, x)
        elif kind_ == "conv":
            cout, k = R.conv[idx], R.ck[idx]
            call_is(st, e, head_calls.conv(M, cin, cout, k), gr.EPI_RELU, ("A", "W", "bias") + (("rowoff",) if k > 1 else ()))
            HWo = hh * ww
            if values:
                ref, mass = R.conv_layer(idx, x)
        else:
            cout, HWo = K, hh * ww
            if values:
                ref, mass = R.final_layer(x)
            if e["op"] == "gemm":
                call_is(st, e, head_calls.conv(M, cin, K, R.fk), 0, ("A", "W", "bias") + (("rowoff",) if R.fk > 1 else ()))
            else:
                want = dict(B=B, HW=HWo, Cin=cin, K=K, temperature=e["scalars"].get("temperature"), clamp=clamp)
                if e["scalars"] != want:
                    rep.fail("sequence", f"{st}: called with {e['scalars']}, expected {want}", st)
        sc = e["scalars"]
        ff, hmp = sc.get("fuse_final"), sc.get("heatmap")
        want_ff = ends and end == "fuse_final"
        want_hm = (ends and end == "heatmap") or (kind_ == "final" and e["op"] == "gemm")
        if (ff is not None) != want_ff or (hmp is not None) != want_hm:
            rep.fail("sequence", f"{st}: fuse_final {ff}, heatmap {hmp}; the branch ends with {end}", st)
        for tail in (ff, hmp):
            if tail is not None and (tuple(tail[:2]) != (K, HWo) or bool(tail[3]) != clamp):
                rep.fail("sequence", f"{st}: epilogue tail {tail}, expected K {K}, HW {HWo}, clamp {clamp} (the clamp is "
                                     "off exactly when the Sparsemax normalisation follows)", st)
        to_heat = ff is not None or hmp is not None or e["op"] == "final_heatmap"
        if e["out"].dtype != (F32 if to_heat else dt):
            rep.fail("sequence", f"{st}: writes {e['out'].dtype}", st)
        if values:
            if ff is not None:
                z, zb, _ = fuse_final_value(e, dt)
                _hold(rep, "value", f"{cdt} GEMM fuse_final -> f32", st, e["out"], z, zb)
                # layer: e1 = the first layer's whole bound, through the 1x1 layer, + the rounding of its weight
                e1 = _kernel_term(ref, dt, F32) + u * ref.abs() + (u + 2.0 ** -24) * mass
                wf, bf = R.sd["final_layer.weight"], R.sd["final_layer.bias"]
                z64, _ = R.heat_tail(F.conv2d(ref, wf, bf), ref)
                ez = (F.conv2d(e1, wf.abs()) + u * (F.conv2d(ref.abs() + e1, wf.abs()) + bf.abs()[None, :, None, None])) / TEMPERATURE
                _hold(rep, "layer", f"layer: deconv + BN + ReLU + final 1x1 {cdt}", st, e["out"], z64,
                      ez + _kernel_term(z64, dt, F32))
            elif e["op"] == "final_heatmap":
                a = e["args"]
                want = hr.final_heatmap_f64(a["x"], a["w"], a["bias"], B, HWo, K, sc["temperature"], sc["clamp"])
                _hold(rep, "value", f"final_heatmap {cdt}", st, e["out"], want, _kernel_term(
                    hr.final_heatmap_f64(a["x"], a["w"], a["bias"], B, HWo, K, sc["temperature"], False), dt, F32))
                layer_hold(st, f"final 1x1 / T, clamp {cdt}", e["out"], ref, mass, F32, 0)
            else:
                suffix = " heatmap -> f32" if hmp is not None else f" -> {cdt}"
                _gemm_value(rep, f"{cdt} GEMM {'deconv' if kind_ == 'deconv' else 'conv'}{suffix}", st, gemm_kw(e), e["out"], dt)
                if hmp is not None and kind_ != "final":
                    ref, mass = R.heat_tail(ref, mass)
                got = e["out"] if hmp is not None else rows_to_nchw(e["out"], B, *ref.shape[2:])
                layer_hold(st, dict(deconv="deconv + BN + ReLU", conv="conv + BN + ReLU", final="final conv / T, clamp")[kind_]
                           + (" heatmap" if hmp is not None and kind_ != "final" else "") + f" {cdt}", got, ref, mass,
                           F32 if hmp is not None else dt, 0 if kind_ == "final" else 1)
        if kind_ == "deconv":
            hh, ww = 2 * hh, 2 * ww
        cin, prev = cout, e
    if (R.normalize is not None) != ("sparsemax" in by):
        rep.fail("sequence", "sparsemax_rows runs exactly when normalize is set", "sparsemax")
    heat_e = by[last]
    if "sparsemax" in by:
        se = by["sparsemax"]
        flows("sparsemax", se, "x", heat_e)
        if float(se["scalars"]["scale"]) != float(R.normalize) or tuple(se["out"].shape) != (B * K, hh * ww):
            rep.fail("sequence", f"sparsemax: scale {se['scalars']['scale']} on {tuple(se['out'].shape)}", "sparsemax")
        if values:
            from oracle import probpose_oracle as orc
            want = torch.clamp(orc.sparsemax_lastdim(se["args"]["x"].double()) * R.normalize, 0.0, 1.0)
            # tests/test_sparsemax.py: 1e-6 * scale against the float64 projection
            _hold(rep, "value", "sparsemax_rows", "sparsemax", se["out"], want,
                  torch.full_like(want, 1e-6 * max(1.0, R.normalize)))
        heat_e = se
    if tuple(heat_e["out"].reshape(B, K, -1).shape) != (B, K, hh * ww):
        rep.fail("sequence", f"the heatmaps are {tuple(heat_e['out'].shape)}", last)
    if outputs is not None:
        if outputs[0].data_ptr() != heat_e["ptrs"]["out"] or not torch.equal(outputs[0].reshape(-1), heat_e["out"].reshape(-1)):
            rep.fail("dataflow", "the returned heatmaps are not what the last launch of the heatmap branch left", last)
    return rep


# ---------------------------------------------------------------------------------------------------------------
# torch emulations of the two walks
# ---------------------------------------------------------------------------------------------------------------
VIT_FAULTS = ("block1_gets_block0_qkv", "ln2_gets_ln1_gamma", "final_ln_gets_last_n2w", "b_hm_row_major",
              "fc1_without_gelu", "fc2_residual_from_patch_embed", "pos_period_n_plus_1")
HEAD_FAULTS = ("bn_without_eps", "bn_mean_added", "parities_exchanged", "gather_border_row_off_by_one",
               "aux_order_vis_prob", "temperature_dropped", "clamp_kept_with_normalize")
FAULTS = VIT_FAULTS + HEAD_FAULTS


def _entry(rec, op, args, scalars, out, names):
    ptrs = {k: hash(v) & 0xFFFFFFF0 for k, v in names.items()}
    args = {k: v for k, v in args.items() if v is not None}
    rec.append(dict(op=op, args=args, scalars=scalars, out=out, ptrs=ptrs,
                    meta={k: (t.dtype, tuple(t.shape)) for k, t in dict(args, out=out).items()}))
    return out


def _emulated_gemm(kw):
    """gemm_reference.expected_output of kw, rounded to the dtype of kw["out"] (shaped like it)."""
    out = kw["out"]
    ref, written = gr.expected_output(kw, torch.zeros(out.numel(), dtype=out.dtype))
    assert bool(written.all())
    return ref.to(out.dtype).reshape(out.shape)


class EmulatedVit:
    """engine.VitPlan's bf16 / fp32 bookkeeping and launch sequence in plain torch: every stage computed in float64
    from the stage's input and rounded once to the dtype the kernel stores.  `fault` plants one of VIT_FAULTS."""

    def __init__(self, sd, cfg, dtype, fault: str = None):
        assert fault is None or fault in VIT_FAULTS
        self.R = R = VitRestatement(sd, cfg, dtype)
        self.fault, self.dtype = fault, dtype
        self.blocks = [dict(b) for b in R.blocks]
        self.nw, self.nb = R.nw, R.nb
        if fault == "block1_gets_block0_qkv":
            self.blocks[1]["qkv_w"] = self.blocks[0]["qkv_w"]
            if "qkv_w_hm" in self.blocks[1]:
                self.blocks[1]["qkv_w_hm"] = self.blocks[0]["qkv_w_hm"]
        if fault == "ln2_gets_ln1_gamma":
            self.blocks[0]["n2w"] = self.blocks[0]["n1w"]
        if fault == "final_ln_gets_last_n2w":
            self.nw = self.blocks[-1]["n2w"]
        if fault == "b_hm_row_major":
            self.blocks[0]["qkv_b_hm"] = self.blocks[0]["qkv_b"]

    def _ln(self, rec, x, gamma, beta, xname, oname):
        ref, _ = ar.expected_layernorm(x, gamma, beta, LN_EPS)
        return _entry(rec, "layernorm", dict(x=x, gamma=gamma, beta=beta), dict(eps=LN_EPS, out_scale=None),
                      ref.to(self.dtype), dict(x=xname, out=oname))

    def _linear(self, rec, x, w, bias, odt, xname, oname, residual=None, epilogue=0, headmajor=None, resname=None):
        out = torch.zeros((x.shape[0], w.shape[0]), dtype=odt)
        out = _emulated_gemm(linear_kw(x, w, bias, out, residual, epilogue, headmajor))
        names = dict(x=xname, out=oname, **({"residual": resname or oname} if residual is not None else {}))
        return _entry(rec, "linear", dict(x=x, w=w, bias=bias, residual=residual),
                      dict(epilogue=epilogue, out_scale=None, headmajor=headmajor, tile=0), out, names)

    def walk(self, x, mode="two_kernel"):
        R, dt = self.R, self.dtype
        B, N, C, heads, hd = x.shape[0], R.N, R.C, R.heads, R.hd
        rec = []
        a0 = _entry(rec, "patchify", dict(x=x), dict(patch=R.patch), hr.patchify_ref(x, R.patch, dt).contiguous(),
                    dict(x="x", out="a0"))
        K0 = a0.shape[1]
        period = N + 1 if self.fault == "pos_period_n_plus_1" else N
        kw = dict(A=a0, W=R.pe_w, out=torch.zeros((B * N, C), dtype=F32), M=B * N, N=C, Kd=K0, lda=K0, ldw=K0, ldc=C,
                  bias=R.pe_b, rowbias=R.pos, rowbias_period=period, epilogue=gr.EPI_OUT_F32)
        if period != N:
            kw["rowbias"] = torch.cat([R.pos, R.pos[:1]])        # room for the row the longer period reads
        xres = _emulated_gemm(kw)
        sc = {k: v for k, v in kw.items() if not isinstance(v, torch.Tensor)}
        pe_out = xres = _entry(rec, "patch_embed", dict(A=a0, W=R.pe_w, bias=R.pe_b, rowbias=R.pos), sc, xres,
                               dict(A="a0", out="xres"))
        hm = (heads, hd) if R.headmajor else None
        for i, b in enumerate(self.blocks):
            h = self._ln(rec, xres, b["n1w"], b["n1b"], "xres", "h")
            if mode == "fused":
                q = (h.double() @ b["qkv_w"].double().t() + b["qkv_b"].double()).to(BF16)
                ref, _ = ar.expected_attention(q, B, N, heads, hd)
                ao = _entry(rec, "qkv_attention", dict(h=h, w_hm=b["qkv_w_hm"], b_hm=b["qkv_b_hm"]), dict(B=B, heads=heads),
                            ref.to(dt), dict(h="h", out="ao"))
            else:
                qkv = self._linear(rec, h, b["qkv_w"], b["qkv_b"], dt, "h", "qkv", headmajor=hm)
                ref, _ = ar.expected_attention(qkv, B, N, heads, hd, R.headmajor)
                ao = _entry(rec, "attention", dict(qkv=qkv), dict(B=B, N=N, heads=heads, hd=hd, out_scale=None,
                                                                  headmajor=R.headmajor), ref.to(dt), dict(qkv="qkv", out="ao"))
            xres = self._linear(rec, ao, b["proj_w"], b["proj_b"], F32, "ao", "xres", residual=xres)
            h = self._ln(rec, xres, b["n2w"], b["n2b"], "xres", "h")
            epi = 0 if self.fault == "fc1_without_gelu" and i == 0 else gr.EPI_GELU
            hid = self._linear(rec, h, b["fc1_w"], b["fc1_b"], dt, "h", "hid", epilogue=epi)
            if self.fault == "fc2_residual_from_patch_embed" and i == 0:
                xres = self._linear(rec, hid, b["fc2_w"], b["fc2_b"], F32, "hid", "xres", residual=pe_out, resname="xres0")
            else:
                xres = self._linear(rec, hid, b["fc2_w"], b["fc2_b"], F32, "hid", "xres", residual=xres)
        self._ln(rec, xres, self.nw, self.nb, "xres", "feats")
        return rec


class EmulatedHead:
    """engine.HeadPlan's bookkeeping and launch sequence in plain torch: BN fold, taps-major and parity packing, the
    gather / scatter tables and the 4C concatenation built the way the plan builds them, every GEMM output
    gemm_reference.expected_output rounded to the output dtype.  `fault` plants one of HEAD_FAULTS."""

    def __init__(self, sd, spec, dtype, fault: str = None, splitk_aux=True, fuse_final=True):
        from probpose_pytorch_amd import pack
        assert fault is None or fault in HEAD_FAULTS
        self.sd, self.spec, self.dtype, self.fault = sd, spec, dtype, fault
        self.splitk_aux, self.fuse_final = splitk_aux, fuse_final
        self.C, self.K = spec["C"], spec["K"]
        self.order = ("visibility", "probability", "oks", "error") if fault == "aux_order_vis_prob" else AUX_NAMES
        C, K, dt = self.C, self.K, dtype

        def fold(w, b, prefix, out_dim=0):
            eps = 0.0 if fault == "bn_without_eps" else BN_EPS
            scale = sd[prefix + "weight"].double() / torch.sqrt(sd[prefix + "running_var"].double() + eps)
            shape = [1] * w.dim()
            shape[out_dim] = -1
            b0 = b.double() if b is not None else torch.zeros_like(scale)
            mean = sd[prefix + "running_mean"].double()
            shift = (b0 + mean) if fault == "bn_mean_added" else (b0 - mean)
            return (w.double() * scale.reshape(shape)).float(), (shift * scale + sd[prefix + "bias"].double()).float()

        self.deconvs, self.convs = [], []
        for i, cout in enumerate(spec["dec"]):
            wf, bf = fold(sd[f"deconv_layers.{3 * i}.weight"], None, f"deconv_layers.{3 * i + 1}.", 1)
            wp = pack.pack_deconv_parities(wf, 4)
            if fault == "parities_exchanged" and i == 0:
                wp = wp[[0, 2, 1, 3]].contiguous()
            self.deconvs.append(dict(w=wp.to(dt), b=bf, cout=cout))
        for i, (cout, k) in enumerate(zip(spec["conv"], spec["ck"])):
            wf, bf = fold(sd[f"conv_layers.{3 * i}.weight"], sd[f"conv_layers.{3 * i}.bias"], f"conv_layers.{3 * i + 1}.")
            self.convs.append(dict(w=pack.conv_taps_major(wf).to(dt), b=bf, cout=cout, k=k))
        self.final = None
        if spec["fk"] is not None:
            self.final = dict(w=pack.conv_taps_major(sd["final_layer.weight"].float()).to(dt), b=sd["final_layer.bias"].float(),
                              k=spec["fk"])
        n = len(spec["pools"])
        sw, sb = [[] for _ in range(n)], [[] for _ in range(n)]
        tw, tb = [], []
        for name in self.order:
            for i in range(n):
                wf, bf = fold(sd[f"{name}_layers.{4 * i}.weight"], sd[f"{name}_layers.{4 * i}.bias"], f"{name}_layers.{4 * i + 1}.")
                sw[i].append(pack.conv_taps_major(wf))
                sb[i].append(bf)
            tw.append(sd[f"{name}_layers.{4 * n}.weight"].float().reshape(K, C))
            tb.append(sd[f"{name}_layers.{4 * n}.bias"].float())
        self.aux_w = [torch.cat(sw[0], 0).to(dt)] + [torch.stack(sw[i]).to(dt) for i in range(1, n)]
        self.aux_b = [torch.cat(sb[0], 0)] + [torch.stack(sb[i]) for i in range(1, n)]
        self.tail_w, self.tail_b = torch.stack(tw).to(dt), torch.stack(tb)

    def _gemm(self, rec, A, W, out, call, names, **extra):
        kw = dict(A=A, W=W, out=out, **call, **extra)
        ff = kw.pop("fuse_final", None)
        args = {k: kw[k] for k in ("A", "W", "bias", "rowoff", "out_rowmap") if kw.get(k) is not None}
        scalars = {k: v for k, v in kw.items() if not isinstance(v, torch.Tensor)}
        if ff is not None:
            args["final_w"], args["final_b"] = ff[:2]
            scalars["fuse_final"] = tuple(ff[2:])
            e = dict(args=args, scalars=scalars, out=out)
            o = fuse_final_value(e, self.dtype)[2].to(F32).reshape(out.shape)
        else:
            o = _emulated_gemm(kw)
        return _entry(rec, "gemm", args, scalars, o, names)

    def walk(self, feats, B, h, w):
        """feats: channels-last rows [B h w, C] in the compute dtype -> the record of one forward."""
        from probpose_pytorch_amd import head_calls, pack
        R_ = HeadRestatement(self.sd, self.spec, self.dtype, B, h, w, self.splitk_aux, self.fuse_final)
        dt, C, K, spec = self.dtype, self.C, self.K, self.spec
        T = 1.0 if self.fault == "temperature_dropped" else TEMPERATURE
        normalize = spec.get("normalize")
        clamp = normalize is None or self.fault == "clamp_kept_with_normalize"
        rec = []
        # ---- aux branch
        a, ah, aw, aname = feats, h, w, "feats"
        for i, p in enumerate(spec["pools"]):
            M = B * ah * aw
            ro = pack.conv_gather_table(B, ah, aw, 3, 3, 1, 1, C if i == 0 else 4 * C)
            if self.fault == "gather_border_row_off_by_one" and i == 0:
                ro = ro.clone()
                ro[0, M - 1] += C                 # the last row's first tap reads the pixel to the right
            kh, kw_, oh, ow = pack.pool_out(ah, aw, p)
            S = R_.split_of(i)
            geo = dict(B=B, h=ah, w=aw, Cc=4 * C, kh=kh, kw=kw_)
            if S > 1:
                parts = self._gemm(rec, a, self.aux_w[i], torch.zeros((S, M, 4 * C), dtype=F32),
                                   head_calls.aux_stage(M, C, split=S), dict(A=aname, out=f"part{i}"), rowoff=ro,
                                   epilogue=gr.EPI_OUT_F32)
                bias = self.aux_b[i].reshape(-1)
                pooled = hr.maxpool_relu_sum_ref(parts.reshape(S, -1), bias, B, ah, aw, 4 * C, kh, kw_, dt)
                _entry(rec, "maxpool_relu_sum", dict(parts=parts, bias=bias), geo, pooled, dict(parts=f"part{i}", out=f"pool{i}"))
            else:
                call = head_calls.aux_stage0(M, C) if i == 0 else head_calls.aux_stage(M, C)
                conv = self._gemm(rec, a, self.aux_w[i], torch.zeros((M, 4 * C), dtype=dt), call,
                                  dict(A=aname, out=f"conv{i}"), bias=self.aux_b[i], rowoff=ro)
                pooled = hr.maxpool_relu_ref(conv, B, ah, aw, 4 * C, kh, kw_)
                _entry(rec, "maxpool_relu", dict(x=conv), geo, pooled, dict(x=f"conv{i}", out=f"pool{i}"))
            a, ah, aw, aname = pooled, oh, ow, f"pool{i}"
        out = hr.aux_tail_ref(a, self.tail_w, self.tail_b).to(F32)
        _entry(rec, "aux_tail", dict(x=a, w=self.tail_w, bias=self.tail_b), dict(B=B, Cc=C, K=K), out, dict(x=aname, out="aux"))
        # ---- heatmap branch
        end = R_.ending()
        x, hh, ww, cin, xname = feats, h, w, C, "feats"
        f = self.final
        nd = len(self.deconvs)
        for li, d in enumerate(self.deconvs):
            M = B * hh * ww
            ro, rm = pack.deconv_tables(B, hh, ww, 4, cin)
            ends = li == nd - 1 and not self.convs
            extra, out, oname = {}, torch.zeros((4 * M, d["cout"]), dtype=dt), f"deconv{li}"
            if ends and end == "fuse_final":
                extra = dict(fuse_final=(f["w"], f["b"], K, 4 * hh * ww, T, clamp))
                out, oname = torch.zeros((B, K, 2 * hh, 2 * ww), dtype=F32), "heat"
            elif ends and end == "heatmap":
                extra = dict(heatmap=(K, 4 * hh * ww, T, clamp))
                out, oname = torch.zeros((B, K, 2 * hh, 2 * ww), dtype=F32), "heat"
            x = self._gemm(rec, x, d["w"], out, head_calls.deconv(M, cin, d["cout"]), dict(A=xname, out=oname), bias=d["b"],
                           rowoff=ro, out_rowmap=rm, epilogue=gr.EPI_RELU, **extra)
            hh, ww, cin, xname = 2 * hh, 2 * ww, d["cout"], oname
        for li, c in enumerate(self.convs):
            M = B * hh * ww
            ro = pack.conv_gather_table(B, hh, ww, c["k"], c["k"], (c["k"] - 1) // 2, (c["k"] - 1) // 2, cin) if c["k"] > 1 else None
            extra, out, oname = {}, torch.zeros((M, c["cout"]), dtype=dt), f"conv{li}"
            if end == "heatmap" and li == len(self.convs) - 1:
                extra = dict(heatmap=(K, hh * ww, T, clamp))
                out, oname = torch.zeros((B, K, hh, ww), dtype=F32), "heat"
            x = self._gemm(rec, x, c["w"], out, head_calls.conv(M, cin, c["cout"], c["k"]), dict(A=xname, out=oname),
                           bias=c["b"], rowoff=ro, epilogue=gr.EPI_RELU, **extra)
            cin, xname = c["cout"], oname
        if end == "final_heatmap":
            v = hr.final_heatmap_f64(x, f["w"], f["b"], B, hh * ww, K, T, clamp).to(F32).reshape(B, K, hh, ww)
            x = _entry(rec, "final_heatmap", dict(x=x, w=f["w"], bias=f["b"]),
                       dict(B=B, HW=hh * ww, Cin=cin, K=K, temperature=T, clamp=clamp), v, dict(x=xname, out="heat"))
        elif end == "final_gemm":
            ro = pack.conv_gather_table(B, hh, ww, f["k"], f["k"], f["k"] // 2, f["k"] // 2, cin) if f["k"] > 1 else None
            x = self._gemm(rec, x, f["w"], torch.zeros((B, K, hh, ww), dtype=F32), head_calls.conv(B * hh * ww, cin, K, f["k"]),
                           dict(A=xname, out="heat"), bias=f["b"], rowoff=ro, heatmap=(K, hh * ww, T, clamp))
        if normalize is not None:
            from oracle import probpose_oracle as orc
            z = x.reshape(B * K, hh * ww)
            v = torch.clamp(orc.sparsemax_lastdim(z.double()) * normalize, 0.0, 1.0).to(F32)
            _entry(rec, "sparsemax_rows", dict(x=z), dict(scale=normalize), v, dict(x="heat", out="heat"))
        return rec
