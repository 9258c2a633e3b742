"""pp_qkv_attention_bf16 (qkv_attention_kernel in pp_attention.hip): attn.qkv and the attention of a ViT block in one
launch, q / k / v kept in LDS.

1. bit identity with the path it replaces: ops.linear (tiles 14, 19, 3) followed by ops.attention;
2. the float64 restatement of tests/attention_reference.py on q / k / v rounded to bf16 after the bias, through that
   module's per-element bound;
3. the hand-over exactly: one-hot rows of h pick columns of w_hm that hold the digit-coded q / k and small-integer v of
   the one-hot attention construction, so the output must equal V[winner] bit for bit;
4. the head-major permutation of qkv.weight / qkv.bias (CPU);
5. the entry point's refusals (CPU);
6. a depth-2 ViT: the fused walk is bit-equal to the two-kernel walk, eagerly and under graph replay, and fp8 / head_dim 32
   plans keep the two-kernel walk; the plan's first eager forward checks the one launch against the two and refuses a
   wrong head-major copy.

Shapes (B, heads, C): (1, 2, 128) 4 K-tiles, the ring's fill and drain edge; (3, 12, 768) 36 tiles, a partially filled
XCD block; (1, 16, 1024) ViT-L's geometry; (5, 3, 192) an odd head count and 6 K-tiles.  The bit-identity test also runs
the two launches of the benchmark steps, (64, 12, 768) and (256, 16, 1024): whole groups of XCD blocks.  Outputs go into
NaN buffers with guards on both sides, 16-byte aligned."""
import pytest
import torch

from tests import attention_reference as ar
from tests import gemm_reference as gr
from tests.test_attention_layernorm_forms_gpu import one_hot_problem

BF16, F32 = torch.bfloat16, torch.float32
NTOK, HD = 192, 64
SHAPES = [(1, 2, 128), (3, 12, 768), (1, 16, 1024), (5, 3, 192)]
QSCALES = [1.0, 3.0]
CASES = [(s, q) for s in SHAPES for q in QSCALES]
_ID = lambda c: f"B{c[0][0]}-heads{c[0][1]}-C{c[0][2]}-q{c[1]:g}"   # noqa: E731


@pytest.fixture(scope="module")
def ops(built_lib):
    assert torch.cuda.is_available()
    from probpose_pytorch_amd import ops as o
    return o


def _guarded(numel):
    """NaN bf16 buffer: 64-byte front guard, numel output elements at a 16-byte aligned address, 256-byte trailing guard."""
    lead = 32
    buf = gr.nan_like_bits(lead + numel + 128, BF16, "cuda")
    assert buf[lead:].data_ptr() % 16 == 0
    return buf, lead


def _guards_intact(buf, before, lead, n):
    a, b = buf.view(torch.int16), before.view(torch.int16)
    return int((a[:lead] != b[:lead]).sum() + (a[lead + n:] != b[lead + n:]).sum()) == 0


_INPUTS = {}


def _inputs(ops, case):
    """h [B*192, C] ~ N(0, 1), qkv.weight [3C, C] ~ N(0, 1 / C) with the q rows (and q bias) times qscale, qkv.bias
    ~ N(0, 1 / 4); their head-major packing; the two-kernel result on tile 14.  Built once per case, never modified."""
    if case not in _INPUTS:
        (B, heads, C), qscale = case
        gen = torch.Generator().manual_seed(1000 * B + heads + C + int(10 * qscale))
        h = torch.randn((B * NTOK, C), generator=gen).to(BF16).cuda()
        w = torch.randn((3 * C, C), generator=gen) * C ** -0.5
        b = torch.randn((3 * C,), generator=gen) * 0.5
        w[:C] *= qscale
        b[:C] *= qscale
        w, b = w.to(BF16).cuda(), b.cuda()
        w_hm, b_hm = ops.pack_qkv_headmajor(w, b, heads)
        d = dict(h=h, w=w, b=b, w_hm=w_hm, b_hm=b_hm)
        d["qkv14"], d["two14"] = _two_kernels(ops, d, B, heads, 14)
        _INPUTS[case] = d
    return _INPUTS[case]


def _two_kernels(ops, d, B, heads, tile):
    qkv = ops.linear(d["h"], d["w"], d["b"], tile=tile)
    out = torch.empty((B * NTOK, heads * HD), dtype=BF16, device="cuda")
    ops.attention(qkv, out, B, NTOK, heads, HD)
    torch.cuda.synchronize()
    return qkv, out


def _fused(ops, d, B, heads):
    n = B * NTOK * heads * HD
    buf, lead = _guarded(n)
    before = buf.clone()
    ops.qkv_attention(d["h"], d["w_hm"], d["b_hm"], buf[lead:lead + n].view(B * NTOK, heads * HD), B, heads)
    torch.cuda.synchronize()
    return buf, before, lead, n


# ---------------------------------------------------------------------------------------------------------------
# 1. bit identity with ops.linear + ops.attention
# ---------------------------------------------------------------------------------------------------------------
BENCH_CASES = [((64, 12, 768), 1.0), ((256, 16, 1024), 1.0)]       # the launches of the vit_b / vit_l benchmark steps


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + BENCH_CASES, ids=_ID)
def test_bit_identical_to_linear_then_attention(ops, case):
    (B, heads, C), _ = case
    d = _inputs(ops, case)
    buf, before, lead, n = _fused(ops, d, B, heads)
    got = buf[lead:lead + n].view(torch.int16)
    assert _guards_intact(buf, before, lead, n)
    diff14 = int((got != d["two14"].reshape(-1).view(torch.int16)).sum())
    print(f"  {_ID(case)}: {diff14} of {n} elements differ from tile 14 + attention")
    assert diff14 == 0
    for tile in (19, 3):
        if tile == 19 and (C < 512 or (3 * C) % 288):
            continue            # tile 19 (192 x 288 stream) takes whole tiles and K >= 512; pp_gemm refuses the rest
        qkv, two = _two_kernels(ops, d, B, heads, tile)
        q_diff = int((qkv.view(torch.int16) != d["qkv14"].view(torch.int16)).sum())
        o_diff = int((got != two.reshape(-1).view(torch.int16)).sum())
        print(f"  {_ID(case)}: tile {tile}: qkv differs from tile 14 in {q_diff} elements, the output in {o_diff}")
        assert q_diff == 0 and o_diff == 0
    if case in BENCH_CASES:
        del _INPUTS[case]           # hundreds of MB: not kept for the session


# ---------------------------------------------------------------------------------------------------------------
# 2. against float64
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_within_bound_of_float64(ops, case):
    (B, heads, C), _ = case
    d = _inputs(ops, case)
    qkv = (d["h"].double() @ d["w"].double().t() + d["b"].double()).to(BF16)     # rounded where the kernel rounds
    ref, ref_abs = ar.expected_attention(qkv, B, NTOK, heads, HD)
    buf, before, lead, n = _fused(ops, d, B, heads)
    v = ar.compare(buf, before, lead, *ar.attention_target(ref, ref_abs, BF16))
    print(f"  {_ID(case)}: {v}")
    assert v.ok, str(v)


# ---------------------------------------------------------------------------------------------------------------
# 3. the hand-over, exactly
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}-heads{s[1]}-C{s[2]}")
def test_hand_over_one_hot_exact(ops, shape):
    """Token i of crop b is the one-hot row e_c, c = cols_b[i % P], so its q / k / v are column c of w_hm exactly (one
    product, the rest zeros); the columns hold a one-hot attention problem over P = min(C, 192) distinct tokens.  Where
    C < 192, tokens i and i + P are equal: two equal winners with equal V, still V[winner] exactly.  The v bias is a
    multiple of 32 (v + bias stays an integer below 256, never 0): a shifted bias index changes the result."""
    B, heads, C = shape
    gen = torch.Generator().manual_seed(7 + C)
    P = min(C, NTOK)
    w = torch.zeros((heads, 3, HD, C), dtype=torch.float64)
    bias = torch.zeros((heads, 3, HD), dtype=torch.float64)
    exp = torch.empty((heads, P, HD), dtype=torch.float64)           # by column
    for h in range(heads):
        q, k, v, _ = one_hot_problem(P, HD, 96, "perm", gen)
        bias[h, 2] = torch.randint(-3, 4, (HD,), generator=gen).double() * 32
        w[h, 0, :, :P], w[h, 1, :, :P], w[h, 2, :, :P] = q.t(), k.t(), v.t()
        # the winner of column c is the key whose code equals the query's: recompute from the scores
        win = (q @ k.t()).argmax(dim=1)
        exp[h] = v[win] + bias[h, 2]
    hmat = torch.zeros((B * NTOK, C), dtype=torch.float64)
    want = torch.empty((B, NTOK, heads, HD), dtype=torch.float64)
    for b in range(B):
        cols = torch.randperm(P, generator=gen)[torch.arange(NTOK) % P]
        hmat[b * NTOK + torch.arange(NTOK), cols] = 1.0
        want[b] = exp[:, cols].transpose(0, 1)
    w_hm = w.reshape(heads * 3 * HD, C)
    assert torch.equal(w_hm.to(BF16).double(), w_hm)
    d = dict(h=hmat.to(BF16).cuda(), w_hm=w_hm.to(BF16).cuda(), b_hm=bias.reshape(-1).float().cuda())
    buf, before, lead, n = _fused(ops, d, B, heads)
    got = buf[lead:lead + n].cpu().view(torch.int16)
    wrong = got != want.reshape(-1).to(BF16).view(torch.int16)
    rows = sorted({int(i) // (heads * HD) for i in torch.nonzero(wrong).reshape(-1)[:4096]})
    print(f"  B{B} heads{heads} C{C}: {int(wrong.sum())} wrong of {n}")
    assert _guards_intact(buf, before, lead, n)
    assert int(wrong.sum()) == 0, f"wrong elements in rows {rows[:24]} (row = b * 192 + token)"


# ---------------------------------------------------------------------------------------------------------------
# 4. the permutation (CPU)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 2, 12])
def test_headmajor_permutation(heads):
    from probpose_pytorch_amd import ops
    Cc = 64 * heads
    w = torch.arange(3 * Cc, dtype=torch.float32)[:, None].expand(3 * Cc, Cc).contiguous()     # entry (r, c) = r
    b = torch.arange(3 * Cc, dtype=torch.float32)
    w_hm, b_hm = ops.pack_qkv_headmajor(w, b, heads)
    assert w_hm.shape == (heads * 192, Cc) and b_hm.shape == (heads * 192,) and w_hm.is_contiguous()
    for h in range(heads):
        for t in range(3):
            src = t * Cc + 64 * h + torch.arange(64, dtype=torch.float32)
            rows = slice(192 * h + 64 * t, 192 * h + 64 * t + 64)
            assert torch.equal(b_hm[rows], src)
            assert torch.equal(w_hm[rows], src[:, None].expand(64, Cc))
    with pytest.raises(ValueError):
        ops.pack_qkv_headmajor(w, b, heads + 1)


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals (no GPU: every check comes before the launch)
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_without_gpu(built_lib):
    f = built_lib.pp_qkv_attention_bf16
    h, w, b, out = 0x10000, 0x20000, 0x30000, 0x40000

    def refused(*args):
        rc = f(*args, None)
        msg = built_lib.pp_last_error()
        assert rc != 0 and b"pp_qkv_attention_bf16" in msg, (args, rc, msg)
        return msg

    assert b"head_dim 64" in refused(h, w, b, out, 2, 4, 128)          # head_dim 32
    assert b"head_dim 64" in refused(h, w, b, out, 2, 2, 160)          # head_dim 80, C % 64 != 0
    assert b"head_dim 64" in refused(h, w, b, out, 2, 3, 160)          # C % 64 != 0
    assert b"C >= 128" in refused(h, w, b, out, 2, 1, 64)              # C = 64: two K-tiles do not fill the ring
    assert b"aligned" in refused(h, w, b, out + 8, 2, 2, 128)
    assert b"aligned" in refused(h + 2, w, b, out, 2, 2, 128)
    for args in ((None, w, b, out), (h, None, b, out), (h, w, None, out), (h, w, b, None)):
        assert b"null" in refused(*args, 2, 2, 128)
    assert b"bad shape" in refused(h, w, b, out, -1, 2, 128)
    assert b"too large" in refused(h, w, b, out, 1 << 24, 128, 8192)
    assert f(None, None, None, None, 0, 2, 128, None) == 0             # B = 0: nothing to do


# ---------------------------------------------------------------------------------------------------------------
# 6. model level
# ---------------------------------------------------------------------------------------------------------------
def _vit(C, heads, dtype):
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    torch.manual_seed(C + heads)
    m = ScratchViTBackbone((256, 192), 16, embed_dim=C, depth=2, num_heads=heads)
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim == 1:
                p.add_(torch.randn_like(p) * 0.1)         # biases and LayerNorm parameters off their 0 / 1 start
    return m.cuda().eval().set_compute_dtype(dtype).model


def _labels(ops, fn):
    prof = []
    ops.set_profile(prof)
    try:
        out = fn()
    finally:
        ops.set_profile(None)
    torch.cuda.synchronize()
    return out, [p[0] for p in prof]


@pytest.mark.gpu
def test_model_fused_walk_bit_equal_eager_and_graph(ops, monkeypatch):
    from probpose_pytorch_amd import engine
    from probpose_pytorch_amd.synthetic import synthetic_crops
    assert engine.FUSE_QKV_ATTENTION
    vit = _vit(128, 2, BF16)
    x = synthetic_crops(2, 256, 192, seed=5).cuda()
    with torch.no_grad():
        # the plan's first eager forward runs the one launch AND, as its check, the two launches it replaces
        plan = vit._plan(x.device)
        assert plan.qkv_fused and not plan.qkv_checked
        _, names = _labels(ops, lambda: vit.forward_tokens(x))
        assert names.count("qkv_attention") == 2 and names.count("attention") == 2 and names.count("gemm") == 1 + 2 * 4
        assert plan.qkv_checked
        t_on, names = _labels(ops, lambda: vit.forward_tokens(x))
        assert names.count("qkv_attention") == 2 and "attention" not in names and names.count("gemm") == 1 + 2 * 3
        ptr, on = t_on.data_ptr(), t_on.clone()
        monkeypatch.setattr(engine, "FUSE_QKV_ATTENTION", False)
        t_off, names = _labels(ops, lambda: vit.forward_tokens(x))
        assert names.count("attention") == 2 and "qkv_attention" not in names and names.count("gemm") == 1 + 2 * 4
        off = t_off.clone()
        monkeypatch.setattr(engine, "FUSE_QKV_ATTENTION", True)
        assert torch.equal(on.view(torch.int16), off.view(torch.int16))
        # no allocation in the call, stable pointers
        torch.cuda.synchronize()
        mem = torch.cuda.memory_allocated()
        assert vit.forward_tokens(x).data_ptr() == ptr and torch.cuda.memory_allocated() == mem
        # capture, replay twice
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            vit.forward_tokens(x)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            t_g = vit.forward_tokens(x)
        assert t_g.data_ptr() == ptr
        for _ in range(2):
            t_g.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(t_g.view(torch.int16), off.view(torch.int16))


@pytest.mark.gpu
def test_first_forward_check_refuses_a_wrong_packing(ops):
    """Two rows of block 1's head-major weight copy exchanged (q row 0 and k row 0 of head 0): the first forward raises,
    and the plan stays unchecked."""
    from probpose_pytorch_amd import _lib
    from probpose_pytorch_amd.synthetic import synthetic_crops
    vit = _vit(128, 2, BF16)
    x = synthetic_crops(2, 256, 192, seed=5).cuda()
    plan = vit._plan(x.device)
    w = plan.blocks[1]["qkv_w_hm"]
    w[[0, 64]] = w[[64, 0]]
    with torch.no_grad(), pytest.raises(_lib.HipExtensionError, match="differ from linear"):
        vit.forward_tokens(x)
    assert not plan.qkv_checked


@pytest.mark.gpu
@pytest.mark.parametrize("C,heads,dtype", [(128, 2, torch.float8_e4m3fn), (64, 2, BF16)], ids=["fp8", "hd32"])
def test_other_plans_keep_the_two_kernel_walk(ops, C, heads, dtype):
    from probpose_pytorch_amd.synthetic import synthetic_crops
    vit = _vit(C, heads, dtype)
    x = synthetic_crops(2, 256, 192, seed=6).cuda()
    with torch.no_grad():
        vit.forward_tokens(x)                              # fp8: the calibrating forward
        _, names = _labels(ops, lambda: vit.forward_tokens(x))
    assert names.count("attention") == 2 and "qkv_attention" not in names
    assert not vit._plan(x.device).qkv_fused
