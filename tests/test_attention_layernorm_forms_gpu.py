"""Every attention and LayerNorm kernel form, exactly and against float64, and the benchmark configurations' real calls.

Attention (pp_attention.hip, attention_valu_kernel in pp_ops.hip): `attention_form` restates the host dispatch and
the case list reaches all 16 instantiations, with e4m3 output on every MFMA form and head-major qkv on every streaming
form.  Each form runs
  - one-hot inputs whose exact result is known: digit-coded q / k make P exactly one-hot (every loser trails the
    winner by >= 160 log2 units after the scale * log2(e) multiply, so its exp2 underflows to 0), V holds small
    integers, and the output must equal V[w(i)] bit for bit (bf16, e4m3 of V * inv_scale) or within 1 ulp (f32);
  - the online-softmax rescale exactly: a decoy that is the running max of an earlier key block (or a later one), and
    two equal winners in different key blocks, placed against the form's key-block size;
  - random inputs at q scales 0.1 and 3 through the per-element bound of tests/attention_reference.py.
LayerNorm (pp_ops.hip): the multi-row kernel is bit-identical to the one-row kernel for every T x RPW x NV, the
dispatch edges hold against float64, and e4m3 saturates.
The real calls: one forward of each benchmarked configuration, every distinct attention / LayerNorm call re-run into
a guarded NaN buffer and checked against the float64 restatement.

Outputs go into NaN-filled buffers with guards, keeping their 16-byte alignment (it selects the store form)."""
import math

import pytest
import torch

from tests import attention_reference as ar
from tests import gemm_reference as gr

pytestmark = pytest.mark.gpu

BF16, F32, FP8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
_CT = {F32: "float", BF16: "unsigned short", FP8: "unsigned char"}      # kernel template argument T


@pytest.fixture(scope="module")
def ops(built_lib):
    assert torch.cuda.is_available()
    from probpose_pytorch_amd import ops as o
    return o


# ---------------------------------------------------------------------------------------------------------------
# attention dispatch
# ---------------------------------------------------------------------------------------------------------------
def attention_form(N, hd, qkv_dtype, out_dtype, headmajor=False, qkv_mod16=0, out_mod16=0, B=1, heads=1):
    """The kernel instantiation a call runs: attention_dispatch, launch_stream and pp_attention_headmajor
    (pp_attention.hip) restated.  None: the call is refused."""
    fp8 = out_dtype == FP8

    def stream():
        waste128, waste144 = -(-N // 128) * 128 - N, -(-N // 144) * 144 - N
        return f"attention_stream_kernel<{hd}, {'3, 3, 32' if waste144 < waste128 else '4, 2, 64'}>"
    if headmajor:
        ok = hd in (32, 64, 80) and qkv_mod16 == 0 and out_mod16 == 0 and not fp8
        return stream() if ok else None
    if qkv_dtype == BF16:
        if hd in (64, 32) and N <= 192 and qkv_mod16 == 0 and out_mod16 % 8 == 0:
            full = N == 192 and (hd != 64 or fp8 or out_mod16 == 0)
            return f"attention_mfma_kernel<{hd}, {'true' if full else 'false'}>"
        if (hd in (32, 64, 80) and qkv_mod16 == 0 and out_mod16 % (8 if fp8 else 16) == 0
                and (B * heads + 8) * -(-N // 128) < 2 ** 31):
            return stream()
        return None if fp8 else f"attention_valu_kernel<unsigned short, {hd}>"
    return None if fp8 else f"attention_valu_kernel<float, {hd}>"


def key_block(form, hd):
    """Keys per online-softmax step of a form (the VALU kernel: its LDS chunk KC, pp_ops.hip launch_attention_valu)."""
    if form.startswith("attention_mfma"):
        return 96
    if form.startswith("attention_stream"):
        return 32 if "3, 3, 32" in form else 64
    return (64 * 1024 // (2 * hd * 4)) // 8 * 8


ATT_FORMS = ([f"attention_mfma_kernel<{hd}, {f}>" for hd in (64, 32) for f in ("true", "false")]
             + [f"attention_stream_kernel<{hd}, {c}>" for hd in (32, 64, 80) for c in ("3, 3, 32", "4, 2, 64")]
             + [f"attention_valu_kernel<{t}, {hd}>" for t in ("float", "unsigned short") for hd in (32, 64, 80)])
FP8_FORMS = [f for f in ATT_FORMS if not f.startswith("attention_valu")]
HEADMAJOR_FORMS = [f for f in ATT_FORMS if f.startswith("attention_stream")]


def _case(N, hd, dtype=BF16, out=None, headmajor=False, qkv_shift=0, out_shift=0, B=2, heads=3):
    """qkv_shift: elements the qkv pointer is moved off 16-byte alignment; out_shift: bytes for the output."""
    return dict(B=B, N=N, heads=heads, hd=hd, dtype=dtype, out=out or dtype, headmajor=headmajor, qkv_shift=qkv_shift,
                out_shift=out_shift)


def _att_cases():
    cs = []
    for hd in (64, 32):
        for N in (192, 150):
            cs += [_case(N, hd), _case(N, hd, out=FP8)]
    cs += [_case(192, 64, out_shift=8), _case(70, 32)]
    for hd in (32, 64, 80):
        for N in (432, 1000, 433, 577):
            cs += [_case(N, hd), _case(N, hd, out=FP8), _case(N, hd, headmajor=True)]
    for hd in (32, 64, 80):
        cs += [_case(433, hd, dtype=F32), _case(192, hd, dtype=F32), _case(433, hd, qkv_shift=1)]
    cs += [_case(432, 80, out_shift=8)]
    for c in cs:
        c["form"] = attention_form(c["N"], c["hd"], c["dtype"], c["out"], c["headmajor"], 2 * c["qkv_shift"] % 16,
                                   c["out_shift"], c["B"], c["heads"])
    return cs


ATT_CASES = _att_cases()


def _case_id(c):
    s = f"N{c['N']}-hd{c['hd']}-{str(c['dtype'])[6:]}"
    s += "-e4m3" if c["out"] == FP8 else ""
    s += "-headmajor" if c["headmajor"] else ""
    s += f"-qkv+{c['qkv_shift']}" if c["qkv_shift"] else ""
    s += f"-out+{c['out_shift']}B" if c["out_shift"] else ""
    return s


def test_attention_cases_reach_every_form():
    forms = {c["form"] for c in ATT_CASES}
    assert None not in forms
    assert forms == set(ATT_FORMS), sorted(set(ATT_FORMS) ^ forms)
    assert {c["form"] for c in ATT_CASES if c["out"] == FP8} == set(FP8_FORMS)
    assert {c["form"] for c in ATT_CASES if c["headmajor"]} == set(HEADMAJOR_FORMS)
    # the (q & 0x14) == 0x10 rows are stored by every shipped 16-byte-store form
    wide = {c["form"] for c in ATT_CASES if c["out"] == BF16 and c["out_shift"] == 0
            and ("<64, true>" in c["form"] or c["form"].startswith(("attention_stream_kernel<64", "attention_stream_kernel<80")))}
    assert len(wide) == 5


# ---------------------------------------------------------------------------------------------------------------
# launching into guarded buffers
# ---------------------------------------------------------------------------------------------------------------
def _guarded(numel, dtype, mod16):
    """NaN buffer: front guard, numel output elements starting at an address = mod16 (mod 16), trailing guard."""
    esz = torch.empty((), dtype=dtype).element_size()
    lead = (64 + mod16) // esz
    buf = gr.nan_like_bits(lead + numel + 256 // esz, dtype, "cuda")
    assert buf[lead:].data_ptr() % 16 == mod16
    return buf, lead


def _layout(qkv_rm, B, N, heads, hd, headmajor, shift):
    """qkv [B*N, 3C] row-major -> the buffer a call reads (head-major permuted, or moved `shift` elements)."""
    t = qkv_rm
    if headmajor:
        t = t.reshape(B * N, 3, heads, hd).permute(1, 2, 0, 3).contiguous().reshape(B * N, 3 * heads * hd)
    if shift:
        raw = torch.empty(t.numel() + shift, dtype=t.dtype, device=t.device)
        raw[shift:] = t.reshape(-1)
        t = raw[shift:].view(t.shape)
    return t


def _run_attention(ops, c, qkv, out_scale=None):
    B, N, heads, hd = c["B"], c["N"], c["heads"], c["hd"]
    buf, lead = _guarded(B * N * heads * hd, c["out"], c["out_shift"])
    before = buf.clone()
    out = buf[lead:lead + B * N * heads * hd].view(B * N, heads * hd)
    assert attention_form(N, hd, qkv.dtype, out.dtype, c["headmajor"], qkv.data_ptr() % 16, out.data_ptr() % 16,
                          B, heads) == c["form"]
    ops.attention(qkv, out, B, N, heads, hd, out_scale=out_scale, headmajor=c["headmajor"])
    torch.cuda.synchronize()
    return buf, before, lead


# ---------------------------------------------------------------------------------------------------------------
# one-hot attention
# ---------------------------------------------------------------------------------------------------------------
ALPHA = 1024.0      # score unit: >= 160 log2 units after * log2(e) / sqrt(hd) for hd <= 80 (1024 * 1.4427 / 8.94 = 165)
DIGITS = 6          # base-4 digits of a code, 3 dims each: 4096 distinct codes


def _digits(code):
    """code [...] int -> [..., DIGITS] digit values 4 * (base-4 digit) (spacing 4: a decoy at +1 is unambiguous)."""
    return torch.stack([(code >> (2 * d)) & 3 for d in range(DIGITS)], dim=-1) * 4


def one_hot_problem(N, hd, kb, pattern, gen):
    """Keys and queries of one (crop, head): (q, k, v float64 [N, hd], expected [N, hd] float64, checks).

    Score S(i, j) = -ALPHA * sum_d (t_i,d - t_j,d)^2 from q dims (2 A t_i, -A, -A t_i^2) and k dims (t_j, t_j^2, 1) per
    digit d, the 3 * DIGITS dims at random positions of the head; every other dim is 0.  Key j's digits are a code,
    query i's digits are the code of its winner, so S = 0 for a winner and <= -ALPHA for every other key; a decoy's
    code is its winner's with digit 0 + 1 (S = -ALPHA, every other key <= -9 ALPHA).
      perm:         winner w(i), a random permutation (every query row has its own winner);
      decoy_first:  keys k < n decoys of winners k + s (s >= kb: a later key block), queries pick k at random;
      winner_first: the same with the roles exchanged (the decoy comes after its winner);
      pairs:        keys k and k + s share a code: two equal winners, result (V[k] + V[k + s]) / 2."""
    dims = torch.randperm(hd, generator=gen)[:3 * DIGITS]
    s = max(kb, -(-N // 2)) if N > kb else -(-N // 2)
    n = N - s
    code = torch.arange(N)
    bump = torch.zeros(N, dtype=torch.long)                 # +1 on digit 0 of decoy keys
    if pattern == "perm":
        w = torch.randperm(N, generator=gen)
        qcode, win = w, [w]
    else:
        pick = torch.randint(0, n, (N,), generator=gen)
        qcode = pick
        lo, hi = torch.arange(n), torch.arange(n) + s
        if pattern == "decoy_first":
            code[hi] = lo
            bump[lo] = 1
            win = [pick + s]
        elif pattern == "winner_first":
            code[hi] = lo
            bump[hi] = 1
            win = [pick]
        else:
            code[hi] = lo
            win = [pick, pick + s]
    tq = _digits(qcode).double()
    tk = _digits(code).double()
    tk[:, 0] += bump.double()
    q = torch.zeros((N, hd), dtype=torch.float64)
    k = torch.zeros((N, hd), dtype=torch.float64)
    q[:, dims[0::3]] = 2 * ALPHA * tq
    q[:, dims[1::3]] = -ALPHA
    q[:, dims[2::3]] = -ALPHA * tq * tq
    k[:, dims[0::3]] = tk
    k[:, dims[1::3]] = tk * tk
    k[:, dims[2::3]] = 1.0
    sign = torch.where(torch.rand(hd, generator=gen) < 0.5, -1.0, 1.0).double()
    v = torch.randint(1, 17, (N, hd), generator=gen).double() * sign      # never 0: no signed zeros in the results
    exp = sum(v[wi] for wi in win) / len(win)
    # the construction, checked in float64: exact in bf16, the winners' score 0, every loser >= 160 log2 units behind,
    # and every partial sum an integer below 2^24 (exact in f32 in any order)
    assert torch.equal(q.to(BF16).double(), q) and torch.equal(k.to(BF16).double(), k)
    S = q @ k.t()
    for wi in win:
        assert bool((S[torch.arange(N), wi] == 0).all())
    lose = torch.ones((N, N), dtype=torch.bool)
    for wi in win:
        lose[torch.arange(N), wi] = False
    c = math.log2(math.e) / math.sqrt(hd)
    assert float(S[lose].max()) * c <= -160.0
    assert float((q.abs() @ k.abs().t()).max()) < 2 ** 24
    if pattern in ("decoy_first", "winner_first"):
        dec = pick if pattern == "decoy_first" else pick + s
        assert bool((S[torch.arange(N), dec] == -ALPHA).all())
        assert bool(((dec // kb) != (win[0] // kb)).all()) or N <= kb
    if pattern == "pairs" and N > kb:
        assert bool(((win[0] // kb) != (win[1] // kb)).all())
    return q, k, v, exp


def _one_hot_inputs(c, pattern, seed):
    B, N, heads, hd = c["B"], c["N"], c["heads"], c["hd"]
    gen = torch.Generator().manual_seed(seed)
    kb = key_block(c["form"], hd)
    qkv = torch.empty((B, N, 3, heads, hd), dtype=torch.float64)
    exp = torch.empty((B, N, heads, hd), dtype=torch.float64)
    for b in range(B):
        for h in range(heads):
            q, k, v, e = one_hot_problem(N, hd, kb, pattern, gen)
            qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h] = q, k, v
            exp[b, :, h] = e
    qkv = qkv.reshape(B * N, 3 * heads * hd).to(c["dtype"]).cuda()
    return _layout(qkv, B, N, heads, hd, c["headmajor"], c["qkv_shift"]), exp.reshape(B * N, heads * hd)


PATTERNS = ["perm", "decoy_first", "winner_first", "pairs"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("c", ATT_CASES, ids=_case_id)
def test_attention_one_hot_exact(ops, c, pattern):
    qkv, exp = _one_hot_inputs(c, pattern, seed=11 + PATTERNS.index(pattern))
    out_scale = 1.0 / 13.37 if c["out"] == FP8 else None
    buf, before, lead = _run_attention(ops, c, qkv, out_scale)
    n = exp.numel()
    bits = gr._BITS[c["out"]]
    got = buf[lead:lead + n].cpu()
    if c["out"] == FP8:
        inv = torch.tensor(1.0 / out_scale, dtype=F32)
        if pattern == "pairs":
            want = ((exp * 2).float() * (inv * 0.5)).to(FP8)
        else:
            want = (exp.float() * inv).to(FP8)
        assert float(exp.abs().max()) * float(inv) < 448
    else:
        want = exp.reshape(-1).to(c["out"])
    want = want.reshape(-1)
    if c["out"] == F32:
        ulps = (got.view(torch.int32).long() - want.view(torch.int32).long()).abs()
        wrong = ~(ulps <= 1) | torch.isnan(got)
    else:
        wrong = got.view(bits) != want.view(bits)
    guards = int((buf[:lead].view(bits) != before[:lead].view(bits)).sum()
                 + (buf[lead + n:].view(bits) != before[lead + n:].view(bits)).sum())
    rows = sorted({int(i) // (c["heads"] * c["hd"]) for i in torch.nonzero(wrong).reshape(-1)[:4096]})
    print(f"  {c['form']:42s} {_case_id(c):32s} {pattern:12s}: {int(wrong.sum())} wrong, {guards} guards written")
    assert int(wrong.sum()) == 0 and guards == 0, f"wrong elements in rows {rows[:24]} (row = b * N + q)"


# ---------------------------------------------------------------------------------------------------------------
# random inputs through the per-element bound
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qscale", [0.1, 3.0])
@pytest.mark.parametrize("c", ATT_CASES, ids=_case_id)
def test_attention_random_within_bound(ops, c, qscale):
    B, N, heads, hd = c["B"], c["N"], c["heads"], c["hd"]
    gen = torch.Generator().manual_seed(int(1000 * qscale) + N + hd)
    t = torch.randn((B * N, 3, heads * hd), generator=gen)
    t[:, 0] *= qscale
    qkv_rm = t.reshape(B * N, 3 * heads * hd).to(c["dtype"]).cuda()
    ref, ref_abs = ar.expected_attention(qkv_rm, B, N, heads, hd)
    qkv = _layout(qkv_rm, B, N, heads, hd, c["headmajor"], c["qkv_shift"])
    out_scale = 1.25 * float(ref.abs().max()) / ar.FP8_MAX if c["out"] == FP8 else None
    buf, before, lead = _run_attention(ops, c, qkv, out_scale)
    inv = 1.0 / out_scale if out_scale else None
    v = ar.compare(buf, before, lead, *ar.attention_target(ref, ref_abs, c["out"], inv))
    print(f"  {c['form']:42s} {_case_id(c):32s} q*{qscale:<4}: {v}")
    assert v.ok, str(v)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------
def layernorm_form(rows, C, out_dtype):
    """The kernel a call runs: pp_layernorm / pp_layernorm_fp8 and layernorm_rows_launch (pp_ops.hip)
    restated."""
    if C % 4 == 0 and 512 < C <= 1280 and rows >= 2048:
        want = (rows + 4095) // 4096
        rpw = 3 if want >= 3 else (2 if want >= 2 else 1)
        return f"layernorm_rows_kernel<{_CT[out_dtype]}, {rpw}, {3 if C <= 768 else 5}>"
    return f"layernorm_kernel<{_CT[out_dtype]}>"


LN_DTYPES = [F32, BF16, FP8]
LN_ROWS = [3001, 6150, 8195]             # RPW 1 / 2 / 3, none a multiple of 4 * RPW: the last wave re-reads tail rows
LN_WIDTHS = [516, 768, 772, 1024, 1280]  # NV 3 / 5 at both ends of each range


def _ln_inputs(rows, C, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, C), generator=gen) * 3 + torch.randn((rows, 1), generator=gen) * 4 + 0.5
    gam, bet = torch.randn((C,), generator=gen), torch.randn((C,), generator=gen)
    return x.cuda(), gam.cuda(), bet.cuda()


def _run_layernorm(ops, x, gam, bet, out_dtype, out_scale, slices=None):
    rows, C = x.shape
    buf, lead = _guarded(rows * C, out_dtype, 0)
    before = buf.clone()
    out = buf[lead:lead + rows * C].view(rows, C)
    step = slices or rows
    for r0 in range(0, rows, step):
        ops.layernorm(x[r0:r0 + step], gam, bet, 1e-6, out[r0:r0 + step], out_scale=out_scale)
    torch.cuda.synchronize()
    return buf, before, lead


def test_layernorm_cases_reach_every_form():
    forms = {layernorm_form(r, C, t) for r in LN_ROWS for C in LN_WIDTHS for t in LN_DTYPES}
    want = {f"layernorm_rows_kernel<{_CT[t]}, {rpw}, {nv}>" for t in LN_DTYPES for rpw in (1, 2, 3) for nv in (3, 5)}
    assert forms == want
    assert ({layernorm_form(r, C, t) for r in (1, 1000, 2047) for C in LN_WIDTHS for t in LN_DTYPES}
            == {f"layernorm_kernel<{_CT[t]}>" for t in LN_DTYPES})


@pytest.mark.parametrize("dtype", LN_DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("C", LN_WIDTHS)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_rows_kernel_bit_identical_to_one_row_kernel(ops, rows, C, dtype):
    x, gam, bet = _ln_inputs(rows, C, rows + C)
    ref, term = ar.expected_layernorm(x, gam, bet, 1e-6)
    out_scale = 1.25 * float(ref.abs().max()) / ar.FP8_MAX if dtype == FP8 else None
    form = layernorm_form(rows, C, dtype)
    assert form.startswith("layernorm_rows_kernel") and layernorm_form(1000, C, dtype).startswith("layernorm_kernel<")
    buf, before, lead = _run_layernorm(ops, x, gam, bet, dtype, out_scale)
    one, _, _ = _run_layernorm(ops, x, gam, bet, dtype, out_scale, slices=1000)
    inv = 1.0 / out_scale if out_scale else None
    v = ar.compare(buf, before, lead, *ar.layernorm_target(ref, term, dtype, inv))
    bits = gr._BITS[dtype]
    diff = int((buf.view(bits) != one.view(bits)).sum())
    print(f"  {form:42s} rows {rows} C {C}: {diff} elements differ from the one-row kernel; {v}")
    assert diff == 0, f"{form}: {diff} elements differ from layernorm_kernel"
    assert v.ok, str(v)


LN_EDGES = [(rows, C, t) for rows in (2047, 2048) for C in (512, 768, 1282, 1284, 2052) for t in LN_DTYPES
            if not (t == FP8 and (C % 4 or C > 2048))]


@pytest.mark.parametrize("rows,C,dtype", LN_EDGES, ids=[f"{r}x{C}-{str(t)[6:]}" for r, C, t in LN_EDGES])
def test_layernorm_dispatch_edges_against_float64(ops, rows, C, dtype):
    x, gam, bet = _ln_inputs(rows, C, 7 * rows + C)
    ref, term = ar.expected_layernorm(x, gam, bet, 1e-6)
    out_scale = 1.25 * float(ref.abs().max()) / ar.FP8_MAX if dtype == FP8 else None
    buf, before, lead = _run_layernorm(ops, x, gam, bet, dtype, out_scale)
    inv = 1.0 / out_scale if out_scale else None
    v = ar.compare(buf, before, lead, *ar.layernorm_target(ref, term, dtype, inv))
    print(f"  {layernorm_form(rows, C, dtype):42s} rows {rows} C {C}: {v}")
    assert v.ok, str(v)


@pytest.mark.parametrize("rows,C", [(3001, 768), (8195, 1024), (6150, 1280), (300, 1024)])
def test_layernorm_e4m3_saturates(ops, rows, C):
    x, gam, bet = _ln_inputs(rows, C, 5 * rows + C)
    ref, term = ar.expected_layernorm(x, gam, bet, 1e-6)
    out_scale = float(ref.abs().max()) / ar.FP8_MAX / 4
    buf, before, lead = _run_layernorm(ops, x, gam, bet, FP8, out_scale)
    v = ar.compare(buf, before, lead, *ar.layernorm_target(ref, term, FP8, 1.0 / out_scale))
    got = buf[lead:lead + rows * C].float()
    print(f"  {layernorm_form(rows, C, FP8):42s} rows {rows} C {C} saturating: {v}")
    assert v.ok, str(v)
    assert torch.isfinite(got).all() and float(got.abs().max()) == 448.0


# ---------------------------------------------------------------------------------------------------------------
# the benchmark configurations' real calls
# ---------------------------------------------------------------------------------------------------------------
CONFIGS = [("vit_b", BF16), ("vit_b", F32), ("vit_l", BF16), ("vit_l", FP8), ("vit_h_wholebody", BF16)]


def _describe(v):
    if isinstance(v, torch.Tensor):
        return ("T", tuple(v.shape), tuple(v.stride()), str(v.dtype), v.data_ptr() % 16)
    return v


def _record(ops, monkeypatch, model, x):
    """One forward with ops.attention and ops.layernorm wrapped: one call per distinct argument set, inputs cloned."""
    real_att, real_ln = ops.attention, ops.layernorm
    seen, calls = set(), []

    def attention(qkv, out, B, N, heads, hd, out_scale=None, headmajor=False):
        sig = ("attention", _describe(qkv), _describe(out), B, N, heads, hd, out_scale, headmajor)
        if sig not in seen:
            seen.add(sig)
            assert qkv.is_contiguous() and out.is_contiguous() and qkv.data_ptr() % 16 == 0   # as its clone will be
            calls.append(dict(op="attention", qkv=qkv.clone(), out_like=(tuple(out.shape), out.dtype, out.data_ptr() % 16),
                              B=B, N=N, heads=heads, hd=hd, out_scale=out_scale, headmajor=headmajor))
        return real_att(qkv, out, B, N, heads, hd, out_scale=out_scale, headmajor=headmajor)

    def layernorm(x, gamma, beta, eps, out, out_scale=None):
        sig = ("layernorm", _describe(x), _describe(out), eps, out_scale)
        if sig not in seen:
            seen.add(sig)
            assert x.is_contiguous() and out.is_contiguous()
            calls.append(dict(op="layernorm", x=x.clone(), gamma=gamma.clone(), beta=beta.clone(), eps=eps,
                              out_like=(tuple(out.shape), out.dtype, out.data_ptr() % 16), out_scale=out_scale))
        return real_ln(x, gamma, beta, eps, out, out_scale=out_scale)

    monkeypatch.setattr(ops, "attention", attention)
    monkeypatch.setattr(ops, "layernorm", layernorm)
    with torch.no_grad():
        model(x)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "attention", real_att)
    monkeypatch.setattr(ops, "layernorm", real_ln)
    return calls


def _check_call(ops, c):
    shape, odt, mod16 = c["out_like"]
    numel = math.prod(shape)
    buf, lead = _guarded(numel, odt, mod16)
    before = buf.clone()
    out = buf[lead:lead + numel].view(shape)
    inv = 1.0 / float(c["out_scale"]) if c["out_scale"] is not None else None
    if c["op"] == "attention":
        B, N, heads, hd = c["B"], c["N"], c["heads"], c["hd"]
        form = attention_form(N, hd, c["qkv"].dtype, odt, c["headmajor"], c["qkv"].data_ptr() % 16, mod16, B, heads)
        ops.attention(c["qkv"], out, B, N, heads, hd, out_scale=c["out_scale"], headmajor=c["headmajor"])
        torch.cuda.synchronize()
        ref, scale = ar.expected_attention(c["qkv"], B, N, heads, hd, c["headmajor"])
        target = ar.attention_target(ref, scale, odt, inv)
        name = f"attention B{B} N{N} heads{heads} hd{hd}{' headmajor' if c['headmajor'] else ''}"
    else:
        rows, C = c["x"].shape
        form = layernorm_form(rows, C, odt)
        ops.layernorm(c["x"], c["gamma"], c["beta"], c["eps"], out, out_scale=c["out_scale"])
        torch.cuda.synchronize()
        ref, scale = ar.expected_layernorm(c["x"], c["gamma"], c["beta"], c["eps"])
        target = ar.layernorm_target(ref, scale, odt, inv)
        name = f"layernorm {rows}x{C}"
    del ref, scale
    v = ar.compare(buf, before, lead, *target)
    name += f" ->{str(odt)[6:]}" + (f" scale {c['out_scale']:.3g}" if c["out_scale"] is not None else "")
    return form, name, v


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=[f"{n}-{str(d)[6:]}" for n, d in CONFIGS])
def test_benchmark_attention_and_layernorm_calls(ops, monkeypatch, name, dtype):
    import time

    import bench
    from probpose_pytorch_amd import engine
    from probpose_pytorch_amd.synthetic import synthetic_crops
    t0 = time.time()
    if dtype == FP8:
        monkeypatch.setattr(engine, "FP8_PROJ", True)      # e4m3 attention output; the calibration pass runs bf16
    cfg = dict(bench.CONFIGS[name])
    model, _, _ = bench.build(cfg, dtype, torch.device("cuda", 0))
    H, W = cfg["img"]
    x = synthetic_crops(cfg["batch"], H, W, seed=1234).cuda()
    calls = _record(ops, monkeypatch, model, x)
    del model, x
    torch.cuda.empty_cache()
    assert {c["op"] for c in calls} == {"attention", "layernorm"}
    if dtype == FP8:
        assert {c["out_like"][1] for c in calls if c["op"] == "attention"} == {BF16, FP8}
    print(f"\n[{name} {str(dtype)[6:]}] {len(calls)} distinct calls")
    failures, worst = [], {}
    while calls:
        c = calls.pop(0)
        form, nm, v = _check_call(ops, c)
        key = (form, nm.split(" scale")[0])
        w = worst.get(key)
        if w is None or v.worst > w[0].worst:
            worst[key] = (v, nm)
        if not v.ok:
            failures.append(f"{form} {nm}: {v}")
        del c
        torch.cuda.empty_cache()
    for (form, _), (v, nm) in sorted(worst.items()):
        print(f"  {form:42s} {nm:56s}: {v}")
    print(f"[{name}] {time.time() - t0:.0f} s")
    assert not failures, "\n".join(failures)
