"""The bf16 / fp32 walk restatement on the CPU (tests/walk_reference.py): the comparators accept the torch emulations
of the ViT walk (two-kernel, head-major, fused) and of the head walk (every form that ends the heatmap branch, split-K
on and off, the Sparsemax normalisation), reject each planted bookkeeping fault with the tag named for it and in the
stage it touches only, and the input condition holds on every state used and rejects the unperturbed head state."""
import pytest
import torch

from tests import walk_reference as wr

BF16, F32, DT = wr.BF16, wr.F32, wr.DT

VIT, HEADS, vit_state, crops, head_state, head_feats = wr.VIT, wr.HEADS, wr.vit_state, wr.crops, wr.head_state, wr.head_feats


def test_input_condition_rejects_the_unperturbed_head_state():
    """The synthetic head state leaves every num_batches_tracked at 0 (same-shaped, bit-equal) and no BatchNorm channel
    where eps shows; the ViT state has neither defect."""
    bad = wr.input_condition(head_state(HEADS["A"], condition=False))
    assert any("bit-equal" in m for m in bad) and any("eps" in m for m in bad), bad
    sd = vit_state(VIT["V1"])
    sd["blocks.1.norm1.weight"] = sd["blocks.0.norm1.weight"].clone()
    sd["norm.bias"] = torch.zeros_like(sd["norm.bias"])
    bad = wr.input_condition(sd)
    assert any("bit-equal" in m for m in bad) and any("all zeros" in m for m in bad), bad


@pytest.mark.parametrize("name,mode,dtype", [("V1", "two_kernel", "bf16"), ("V1", "two_kernel", "fp32"),
                                             ("V2", "fused", "bf16"), ("V2", "two_kernel", "bf16"),
                                             ("V3", "two_kernel", "bf16"), ("V4", "two_kernel", "bf16"),
                                             ("V4", "two_kernel", "fp32")])
def test_vit_comparator_accepts_the_emulation(name, mode, dtype):
    cfg = VIT[name]
    sd = vit_state(cfg)
    B = 1 if name in ("V2", "V3") else cfg["B"]
    rec = wr.EmulatedVit(sd, cfg, DT[dtype]).walk(crops(cfg, B), mode)
    R = wr.VitRestatement(sd, cfg, DT[dtype])
    assert R.headmajor == (name == "V3")
    rep = wr.check_vit_walk(rec, R, mode)
    print(f"\n[{name} {mode} {dtype}]\n{rep.summary()}")
    assert rep.ok, str(rep)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name,splitk", [("A", True), ("B", True), ("C", True), ("default", True), ("default", False),
                                         ("normalize", True)])
def test_head_comparator_accepts_the_emulation(name, splitk, dtype):
    spec, dt = HEADS[name], DT[dtype]
    sd = head_state(spec)
    feats, B, h, w = head_feats(spec, dt)
    rec = wr.EmulatedHead(sd, spec, dt, splitk_aux=splitk).walk(feats, B, h, w)
    R = wr.HeadRestatement(sd, spec, dt, B, h, w, splitk_aux=splitk)
    want_end = dict(A="final_gemm", B="heatmap", C="final_heatmap", default="fuse_final" if dt == BF16 else "final_heatmap",
                    normalize="fuse_final" if dt == BF16 else "final_heatmap")[name]
    assert R.ending() == want_end
    rep = wr.check_head_walk(rec, R)
    print(f"\n[head {name} splitk={splitk} {dtype}] ends with {R.ending()}\n{rep.summary()}")
    assert rep.ok, str(rep)


# fault -> (model / head, mode, dtypes, tag, the stages the fault touches: prefixes of stage names)
ANY_BN = ("aux stage", "aux pool", "deconv", "conv")
SCENARIOS = {
    "block1_gets_block0_qkv": ("V1", "two_kernel", ("bf16", "fp32"), "weight", ("block 1 qkv",)),
    "ln2_gets_ln1_gamma": ("V1", "two_kernel", ("bf16",), "weight", ("block 0 ln2",)),
    "final_ln_gets_last_n2w": ("V1", "two_kernel", ("bf16",), "weight", ("final LayerNorm",)),
    "b_hm_row_major": ("V2", "fused", ("bf16",), "weight", ("block 0 qkv_attention",)),
    "fc1_without_gelu": ("V1", "two_kernel", ("bf16",), "sequence", ("block 0 fc1",)),
    "fc2_residual_from_patch_embed": ("V1", "two_kernel", ("bf16",), "dataflow", ("block 0 fc2",)),
    "pos_period_n_plus_1": ("V1", "two_kernel", ("bf16", "fp32"), "layer", ("patch embed",)),
    "bn_without_eps": ("A", None, ("fp32",), "layer", ANY_BN),
    "bn_mean_added": ("A", None, ("bf16", "fp32"), "layer", ANY_BN),
    "parities_exchanged": ("A", None, ("bf16", "fp32"), "layer", ("deconv 0",)),
    "gather_border_row_off_by_one": ("A", None, ("bf16", "fp32"), "layer", ("aux stage 0",)),
    "aux_order_vis_prob": ("A", None, ("bf16", "fp32"), "layer", ("aux stage", "aux pool", "aux tail")),
    "temperature_dropped": ("default", None, ("bf16", "fp32"), "layer", ("deconv 1", "final")),
    "clamp_kept_with_normalize": ("normalize", None, ("bf16", "fp32"), "sequence", ("deconv 1", "final")),
}


def test_every_fault_has_a_scenario():
    assert set(SCENARIOS) == set(wr.FAULTS)


def _run(fault, planted, dtype):
    name, mode, _, _, _ = SCENARIOS[fault]
    dt = DT[dtype]
    if fault in wr.VIT_FAULTS:
        cfg = VIT[name]
        sd = vit_state(cfg)
        rec = wr.EmulatedVit(sd, cfg, dt, fault=planted).walk(crops(cfg, 1 if name == "V2" else cfg["B"]), mode)
        return wr.check_vit_walk(rec, wr.VitRestatement(sd, cfg, dt), mode)
    spec = HEADS[name]
    sd = head_state(spec)
    feats, B, h, w = head_feats(spec, dt)
    rec = wr.EmulatedHead(sd, spec, dt, fault=planted).walk(feats, B, h, w)
    return wr.check_head_walk(rec, wr.HeadRestatement(sd, spec, dt, B, h, w))


@pytest.mark.parametrize("fault,dtype", [(f, d) for f in wr.FAULTS for d in SCENARIOS[f][2]])
def test_comparator_rejects_planted_fault(fault, dtype):
    _, _, _, tag, touched = SCENARIOS[fault]
    rep = _run(fault, fault, dtype)
    print(f"\n[{fault} {dtype}] {len(rep.failures)} findings, tags {sorted(rep.tags())}, stages "
          f"{sorted(rep.failed_stages())}; first: {rep.failures[:1]}")
    assert not rep.ok and tag in rep.tags(), (sorted(rep.tags()), str(rep)[:2000])
    stray = {s for s in rep.failed_stages() if not s.startswith(touched)}
    assert not stray, f"the fault also fails {sorted(stray)}:\n{str(rep)[:2000]}"


def test_bn_without_eps_in_bf16_stays_inside_the_bound():
    """A fold without eps moves a conditioned channel by eps / (2 var) <= 5e-4 of its pre-bias value; the bf16 kernel
    term alone is 2^-7 = 7.8e-3 of the output.  It trips in fp32 (test_comparator_rejects_planted_fault) and cannot in
    bf16: stated here so that nobody takes the bf16 walk to cover it."""
    rep = _run("bn_without_eps", "bn_without_eps", "bf16")
    print(f"\n[bn_without_eps bf16]\n{rep.summary()}")
    assert rep.ok, str(rep)


def test_bf16_rounding_reaches_two_to_the_minus_eight():
    """Why u_w is 2^-8 and not 2^-9: 1 + 2^-8 lies half-way between the bf16 values 1 and 1 + 2^-7 and rounds to the
    even one, 1, an error of 2^-8 / (1 + 2^-8) of the operand, almost twice 2^-9."""
    w = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)
    rel = ((w.float().to(BF16).double() - w).abs() / w).max()
    assert 2.0 ** -9 < float(rel) <= wr.u_of(BF16)


def test_two_to_the_minus_nine_is_left_by_the_exact_emulation():
    """Head variant B in bf16 ends with a 1x1 layer of 64 terms.  The emulation rounds each operand once and computes in
    float64, and still one element of that layer lies outside the layer bound taken with u_w = 2^-9 (1.02 of it; the
    MI355X gives 1.02 as well), inside with 2^-8 (0.51): the excess is operand rounding, not a kernel's error."""
    spec = HEADS["B"]
    sd = head_state(spec)
    feats, B, h, w = head_feats(spec, BF16)
    rep = wr.check_head_walk(wr.EmulatedHead(sd, spec, BF16).walk(feats, B, h, w), wr.HeadRestatement(sd, spec, BF16, B, h, w))
    kind = "layer: conv + BN + ReLU heatmap bfloat16"
    print(f"\n{kind}: {rep.worst[kind]:.3f} with 2^-8, {rep.worst[kind + ' [u_w 2^-9]']:.3f} with 2^-9")
    assert rep.ok and rep.worst[kind] < 1.0 < rep.worst[kind + " [u_w 2^-9]"]


def test_recording_clones_before_and_after_and_restores_the_module():
    """tests/walk_recording.py on a stand-in for the ops module: arguments are cloned before the call and the output
    after it, a GEMM inside ops.linear is not a launch of its own, gemm_kw gives back the keyword set, and the
    module's attributes are the originals again afterwards (also after an exception)."""
    import types

    from tests import walk_recording as rec_mod

    def gemm(A, W, out, **kw):
        out.copy_(A @ W.t() + (kw["bias"] if kw.get("bias") is not None else 0))
        A.zero_()                                              # what the record holds must be from before this
        return out

    def linear(x, w, bias=None, *, out=None, **kw):
        return fake.gemm(x, w, out, M=x.shape[0], N=w.shape[0], Kd=x.shape[1], bias=bias)

    fake = types.SimpleNamespace(gemm=gemm, linear=linear, patchify=None)
    orig = dict(vars(fake))
    x, w, b = torch.randn(3, 4), torch.randn(5, 4), torch.randn(5)
    want = x @ w.t() + b
    with rec_mod.recording(fake, ("gemm", "linear", "patchify")) as rec:
        o1 = fake.linear(x.clone(), w, b, out=torch.zeros(3, 5))
        o2 = fake.gemm(x.clone(), w, torch.zeros(3, 5), M=3, N=5, Kd=4, lda=4, ldw=4, ldc=5, bias=b, epilogue=0)
    assert vars(fake) == orig and [e["op"] for e in rec] == ["linear", "gemm"]
    assert torch.equal(rec[0]["args"]["x"], x) and torch.equal(rec[0]["out"], want) and torch.equal(o1, want)
    kw = rec_mod.gemm_kw(rec[1])
    assert torch.equal(kw["A"], x) and torch.equal(kw["out"], o2) and kw["bias"] is not None and kw["ldc"] == 5
    assert rec[1]["meta"]["out"] == (torch.float32, (3, 5)) and set(rec[1]["ptrs"]) == {"A", "W", "bias", "out"}
    with pytest.raises(ZeroDivisionError):
        with rec_mod.recording(fake, ("gemm", "linear", "patchify")):
            1 / 0
    assert vars(fake) == orig
