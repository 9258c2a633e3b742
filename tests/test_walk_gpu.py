"""The bf16 and fp32 walks of engine.VitPlan and engine.HeadPlan against the float64 restatement of
tests/walk_reference.py, stage by stage.

Every forward kernel has its own float64 test that takes the launch's arguments as given.  Here the arguments are held:
the record of one forward (tests/walk_recording.py) must be the restated launch sequence, every operand the
state-dict tensor it should be (ViT) or an operand whose product is the float64 layer of the state-dict parameters
(head), every stage must read bit for bit and at the same address what its producer left, and every stage's output
must lie inside the per-kernel bound of the float64 value of its own recorded input.

The models are the smallest that still take each path, depth 2:
  V1  img 64x48, C 128, 2 heads, B 5: N = 12, M = 60 ragged against every tile; the two-kernel walk, bf16 and fp32
  V2  img 256x192, C 128, 2 heads, B 2: the fused qkv + attention walk (bf16); the first forward also carries the
      plan's own check
  V3  img 384x288 (N = 432), C 320, 4 heads of 80, B 1: head-major qkv and the streaming attention (bf16)
  V4  img 80x48, C 256, 8 heads of 32, N = 15, B 3: bf16 and fp32
  V5  V1 at B 16 with engine.DUAL_CHAIN: two walks on two streams over row halves of the same buffers
and the heads of walk_reference.HEADS (the three HEAD_VARIANTS of test_oracle_goldens.py and the default
head, also with normalize, without split-K, serialised), B 2, bf16 and fp32, with the conditioned states of
walk_reference.condition_head_state.  No geometry had to be replaced.  Every test prints its worst d / bound per stage
kind."""
import pytest
import torch

from tests import walk_reference as wr
from tests.walk_reference import DT, HEADS, VIT, crops, head_feats, head_state, vit_state
from tests.walk_recording import recording

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops(built_lib):
    assert torch.cuda.is_available()
    from probpose_pytorch_amd import ops as o
    return o


def _vit(cfg, sd, dtype):
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    m = ScratchViTBackbone(cfg["img"], cfg["patch"], embed_dim=cfg["C"], depth=cfg["depth"], num_heads=cfg["heads"])
    m.model.load_state_dict(sd)
    return m.cuda().eval().set_compute_dtype(dtype)


def _head(spec, sd, dtype):
    from probpose_pytorch_amd.head import ProbMapHead
    dec = spec["dec"]
    head = ProbMapHead(spec["C"], spec["K"], spec["pools"], dec, (4,) * len(dec), conv_out_channels=spec["conv"] or None,
                       conv_kernel_sizes=spec["ck"] or None, final_layer_kernel_size=spec["fk"],
                       normalize=spec.get("normalize"))
    head.load_state_dict(sd)
    return head.cuda().eval().set_compute_dtype(dtype)


def _record(ops, fn):
    with recording(ops) as rec, torch.no_grad():
        out = fn()
    torch.cuda.synchronize()             # once, after the forward and before anything is read
    return rec, out


def _on_gpu(sd):
    return {k: v.cuda() for k, v in sd.items()}


def _same_bits(a, b):
    return wr._bits_equal(a.reshape(-1), b.reshape(-1))


# ---------------------------------------------------------------------------------------------------------------
# ViT
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("V1", "bf16"), ("V1", "fp32"), ("V3", "bf16"), ("V4", "bf16"), ("V4", "fp32")])
def test_vit_two_kernel_walk(ops, name, dtype):
    cfg, dt = VIT[name], DT[dtype]
    sd = vit_state(cfg)
    vit = _vit(cfg, sd, dt)
    x = crops(cfg).cuda()
    rec, tok = _record(ops, lambda: vit.model.forward_tokens(x))
    plan = vit.model._plan(x.device)
    R = wr.VitRestatement(_on_gpu(sd), cfg, dt)
    assert not plan.qkv_fused and plan.headmajor == R.headmajor == (name == "V3")
    rep = wr.check_vit_walk(rec, R, "two_kernel")
    print(f"\n[{name} {dtype}] B = {cfg['B']}, headmajor {R.headmajor}\n{rep.summary()}")
    assert rep.ok, str(rep)
    assert tok.data_ptr() == rec[-1]["ptrs"]["out"] and _same_bits(tok, rec[-1]["out"])


def test_vit_fused_walk_and_the_first_forwards_own_check(ops):
    """V2.  The first forward is the fused sequence plus, per block, the plan's own check: ops.linear on tile 14 and
    ops.attention on the same h, whose output is the fused launch's bit for bit.  The second forward (qkv_checked) is
    the fused sequence alone and is held in full."""
    from probpose_pytorch_amd import engine
    assert engine.FUSE_QKV_ATTENTION
    cfg = VIT["V2"]
    sd = vit_state(cfg)
    vit = _vit(cfg, sd, BF16)
    x = crops(cfg).cuda()
    plan = vit.model._plan(x.device)
    assert plan.qkv_fused and not plan.qkv_checked
    first, _ = _record(ops, lambda: vit.model.forward_tokens(x))
    assert plan.qkv_checked
    R = wr.VitRestatement(_on_gpu(sd), cfg, BF16)
    roles = wr.vit_roles(cfg["depth"], "fused")
    want, at = [], []
    for r, i in roles:
        if r == "qkv_attention":
            at.append(len(want))
            want += ["linear", "attention"]
        want.append(wr._OP[r])
    assert [e["op"] for e in first] == want
    for i, j in enumerate(at):
        lin, att, qa = first[j], first[j + 1], first[j + 2]
        assert lin["scalars"]["tile"] == 14 and lin["scalars"]["headmajor"] is None
        assert _same_bits(lin["args"]["x"], qa["args"]["h"]) and lin["ptrs"]["x"] == qa["ptrs"]["h"]
        assert _same_bits(lin["args"]["w"], R.blocks[i]["qkv_w"]) and _same_bits(lin["args"]["bias"], R.blocks[i]["qkv_b"])
        assert _same_bits(att["args"]["qkv"], lin["out"]) and att["ptrs"]["qkv"] == lin["ptrs"]["out"]
        assert _same_bits(att["out"], qa["out"]), f"block {i}: the check's attention output is not the fused launch's"
        assert att["ptrs"]["out"] != qa["ptrs"]["out"]
    skip = {j for a in at for j in (a, a + 1)}
    rep = wr.check_vit_walk([e for j, e in enumerate(first) if j not in skip], R, "fused")
    assert rep.ok, f"the first forward without its check launches:\n{rep}"
    second, tok = _record(ops, lambda: vit.model.forward_tokens(x))
    rep = wr.check_vit_walk(second, R, "fused")
    print(f"\n[V2 bf16 fused] B = {cfg['B']}\n{rep.summary()}")
    assert rep.ok, str(rep)
    assert tok.data_ptr() == second[-1]["ptrs"]["out"]
    for a, b in zip([e for j, e in enumerate(first) if j not in skip], second):
        assert _same_bits(a["out"], b["out"]) and a["ptrs"] == b["ptrs"]


def test_vit_dual_chain_is_two_walks_over_row_halves(ops, monkeypatch):
    """V5.  The record is two complete walks in host order, each held on its own; launch by launch the second walk's
    activations lie one half-batch of rows behind the first's in the same buffers, both read the same parameters, and
    the two halves together are the single-chain record bit for bit."""
    from probpose_pytorch_amd import engine
    cfg = dict(VIT["V1"], B=16)
    assert cfg["B"] >= engine.DUAL_CHAIN_MIN_BATCH
    sd = vit_state(cfg)
    vit = _vit(cfg, sd, BF16)
    x = crops(cfg).cuda()
    single, _ = _record(ops, lambda: vit.model.forward_tokens(x))
    monkeypatch.setattr(engine, "DUAL_CHAIN", True)
    dual, tok = _record(ops, lambda: vit.model.forward_tokens(x))
    monkeypatch.setattr(engine, "DUAL_CHAIN", False)
    R = wr.VitRestatement(_on_gpu(sd), cfg, BF16)
    L = len(wr.vit_roles(cfg["depth"], "two_kernel"))
    assert len(single) == L and len(dual) == 2 * L
    for half, walk in enumerate((dual[:L], dual[L:])):
        rep = wr.check_vit_walk(walk, R, "two_kernel")
        print(f"\n[V5 bf16 dual chain, walk {half}] B = {cfg['B'] // 2}\n{rep.summary()}")
        assert rep.ok, f"walk {half}:\n{rep}"
    rep = wr.check_vit_walk(single, R, "two_kernel")
    assert rep.ok, str(rep)
    params = {"gamma", "beta", "w", "bias", "W", "rowbias"}
    for s, a, b in zip(single, dual[:L], dual[L:]):
        assert s["op"] == a["op"] == b["op"]
        for k in a["ptrs"]:
            if k in params:
                assert a["ptrs"][k] == b["ptrs"][k] == s["ptrs"][k]
                continue
            t = a["out"] if k == "out" else a["args"][k]
            assert s["ptrs"][k] == a["ptrs"][k], f"{s['op']} {k}: the first walk does not start at the buffer"
            assert b["ptrs"][k] == a["ptrs"][k] + t.numel() * t.element_size(), f"{s['op']} {k}: not the next row half"
            whole = s["out"] if k == "out" else s["args"][k]
            u = b["out"] if k == "out" else b["args"][k]
            assert _same_bits(torch.cat([t, u]), whole), f"{s['op']} {k}: the halves are not the single-chain tensor"
    assert tok.data_ptr() == dual[L - 1]["ptrs"]["out"]


# ---------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------
HEAD_CASES = [("A", {}), ("B", {}), ("C", {}), ("default", {}), ("normalize", {}), ("default", dict(SPLITK_AUX=False)),
              ("default", dict(SERIALIZE_HEAD=True))]


def _head_walk(ops, monkeypatch, name, switches, dtype, feats=None):
    from probpose_pytorch_amd import engine
    for k, v in switches.items():
        monkeypatch.setattr(engine, k, v)
    spec, dt = HEADS[name], DT[dtype]
    sd = head_state(spec)
    head = _head(spec, sd, dt)
    rows, B, h, w = head_feats(spec, dt)
    rows = rows.cuda()
    rec, out = _record(ops, lambda: head.forward_tokens(rows, B, h, w))
    R = wr.HeadRestatement(_on_gpu(sd), spec, dt, B, h, w, splitk_aux=engine.SPLITK_AUX, fuse_final=engine.FUSE_FINAL)
    return rec, out, R, rows


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name,switches", HEAD_CASES, ids=[n + "".join(f"-{k}={v}" for k, v in s.items()) for n, s in HEAD_CASES])
def test_head_walk(ops, monkeypatch, name, switches, dtype):
    rec, out, R, rows = _head_walk(ops, monkeypatch, name, switches, dtype)
    want_end = dict(A="final_gemm", B="heatmap", C="final_heatmap")
    assert R.ending() == want_end.get(name, "fuse_final" if dtype == "bf16" else "final_heatmap")
    assert rec[0]["ptrs"]["A"] == rows.data_ptr()
    rep = wr.check_head_walk(rec, R, outputs=out)
    print(f"\n[head {name} {switches} {dtype}] B = 2, the heatmap branch ends with {R.ending()}, split-K "
          f"{[R.split_of(i) for i in range(len(R.pools))]}\n{rep.summary()}")
    assert rep.ok, str(rep)


# ---------------------------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------------------------
def test_model_backbone_feeds_the_head_and_graph_replay(ops):
    """V2's backbone feeding the default head, bf16: the head's first launches read the final LayerNorm's output bit
    for bit at its address, both walks hold, and a captured graph replays the eager outputs bit for bit."""
    from probpose_pytorch_amd.model import ProbPoseModel
    cfg, spec = VIT["V2"], HEADS["default"]
    vsd, hsd = vit_state(cfg), head_state(spec)
    model = ProbPoseModel(_vit(cfg, vsd, BF16), _head(spec, hsd, BF16)).eval()
    x = crops(cfg).cuda()
    B = cfg["B"]
    with torch.no_grad():
        model(x)                                             # the fused walk's own check runs here
    rec, out = _record(ops, lambda: model(x))
    eager = [t.clone() for t in out]
    nv = len(wr.vit_roles(cfg["depth"], "fused"))
    vrec, hrec = rec[:nv], rec[nv:]
    rep = wr.check_vit_walk(vrec, wr.VitRestatement(_on_gpu(vsd), cfg, BF16), "fused")
    assert rep.ok, str(rep)
    R = wr.HeadRestatement(_on_gpu(hsd), spec, BF16, B, *spec["hw"])
    hrep = wr.check_head_walk(hrec, R, outputs=out)
    print(f"\n[model V2 + default head bf16]\n{rep.summary()}\n{hrep.summary()}")
    assert hrep.ok, str(hrep)
    fin = vrec[-1]
    firsts = [hrec[0]] + [e for e, (_, st) in zip(hrec, R.sequence()) if st == "deconv 0"]
    assert len(firsts) == 2
    for e in firsts:
        assert e["ptrs"]["A"] == fin["ptrs"]["out"] and _same_bits(e["args"]["A"], fin["out"])
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(x)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out_g = model(x)
        g.replay()
        torch.cuda.synchronize()
    for a, b in zip(eager, out_g):
        assert _same_bits(a, b)
