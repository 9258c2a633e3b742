"""Float64 CPU references of the kernels of csrc/pp_vit_grad.hip, one operation each, with the element-wise magnitudes
("companions") their rounding bounds are stated against, and the faults the bounds must reject.

Every bound here is local to an element: |got - want| <= c u companion, the companion being the same sum as `want` with
every term replaced by its magnitude.  A companion is never 0 where a rounding residue can appear, unlike |want| (with
N = 1 the exact dQ and dK are 0).  u = 2^-24 (f32 arithmetic) or 2^-8 (one bf16 rounding).

Attention backward (row layout: qkv [B N, 3 C] = [3][heads][hd] along a row, O / dO [B N, C]), scale = hd^-1/2:
    S = scale Q K^T, P = softmax(S), dP = dO V^T, D = rowsum(dO o O), dS = P (dP - D),
    dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO.
``attention_backward`` is the exact float64 value of these from the O it is given, with the companions
    b_ij = sum_d |dO_id| |v_jd|,  e_i = sum_d |dO_id| |O_id|,
    comp dQ_i = scale sum_j P_ij (b_ij + e_i) |k_j|, comp dK_j = scale sum_i P_ij (b_ij + e_i) |q_i|,
    comp dV_j = sum_i P_ij |dO_i|.
The f32 (VALU) kernels are held to c = 4 (sqrt(N) + sqrt(hd)) + 16 (``c_attention_f32``, the constant of
tests/test_vit_grad_ops_gpu.py) against these.

The bf16 model (``attention_backward_bf16_model``) takes the same bf16 inputs and the forward's bf16 O, rounds P (for dV)
and dS (for dQ, dK) to bf16 before the second products as the MFMA kernels do, and keeps every sum in float64; its
results x are rounded once to bf16.  The kernel differs from it by its f32 arithmetic only, and that reaches the output
in three ways, each bounded per element:

1. The f32 error of P_ij and dS_ij ahead of their bf16 rounding.  Count the f32 roundings on the path, c u each with
       c = c_model(N, hd) = hd / 32 + N / 32 + 24:
   hd / 32 chained MFMA accumulations per dot product; N / 32 chained accumulations of the row sum l and of the second
   products; and 24 for what does not grow: 8 for the 32 products summed inside one MFMA (their order and internal
   width are not documented; 8 roundings cover a tree of depth 5 and a chain of 8), 4 each for expf and logf, 1 each
   for the scale multiply, s - lse, dP - D, P (dP - D), the rounding of lse and of D, and 2 for the lane exchanges.
   An absolute error t of the exponent s_ij - lse_i is a relative error t of P_ij.  The exponent's error is counted
   against the magnitudes that are rounded on the way to it:
       A_ij = a_ij + max_j a_ij + |s_ij| + |lse_i| + 1,  a_ij = scale sum_d |q_id| |k_jd|
   (the second term is the error lse inherits from the largest score), so
       |dP_ij| <= c u A_ij P_ij =: eP_ij,    |d dS_ij| <= c u P_ij (A_ij |dP_ij - D_i| + b_ij + e_i) =: eS_ij.
2. A flip of the bf16 rounding of P_ij or dS_ij.  This needs no allowance of its own kind: rounding is monotone, so the
   kernel's bf16 dS_ij lies between rn(dS_ij - eS_ij) and rn(dS_ij + eS_ij), and
       fS_ij = max |rn(dS_ij +- eS_ij) - rn(dS_ij)|
   is 0 unless the float64 dS_ij lies within eS_ij of a rounding boundary; then it is one bf16 ulp of that term.
   Likewise fP_ij.  The pre-rounding result therefore lies within
       E(dQ_id) = scale sum_j (fS_ij + c u (|rn dS_ij| + fS_ij)) |k_jd|
   of the model's (the second part: the f32 accumulation of the second product and the final scale multiply); E(dK)
   with q_i for k_j and the sum over i; E(dV_jd) = sum_i (fP_ij + c u (|rn P_ij| + fP_ij)) |dO_id|.
3. The final bf16 rounding, again by monotonicity: got must lie in [rn(x - E), rn(x + E)] (``inside_model``).  Where
   E is below the distance of x to its nearest rounding boundary, that is equality of the bits.

Nothing in c_model or E is taken from a kernel's output.  The allowance is of the order of c 2^-24 times the
companion plus a few single-term bf16 ulps, against c 2^-8 times the tensor's maximum in the float64 comparison:
an error of 10^-3 of an element (one spurious key among 577) falls outside it.

``fault`` plants what the bounds must reject (ATTENTION_FAULTS): 'unmasked_key' (one zero key, k = v = 0, joins the
softmax: `<= N` for `< N` in the key mask; it adds nothing to dQ but takes its share of every P), 'dropped_last_key'
(dQ misses key N - 1), 'dropped_last_query' (dK / dV miss query N - 1), 'D_zero' (D = 0).  With N = 1 the exact dQ is
0 with or without its only key (dS = P (dO . v - dO . O) and O = v), so 'dropped_last_key' computes the same function
there: tests/test_vit_grad_ops_reference.py asserts that identity in place of a rejection.

LayerNorm backward, y = xhat gamma + beta, xhat = (x - mean) rstd, gx = gamma dy:
    dx = rstd (gx - mean(gx) - xhat mean(gx xhat)), dgamma = sum_rows dy xhat, dbeta = sum_rows dy,
    comp dx = rstd (|gx| + mean|gx| + |xhat| mean|gx xhat|), comp dgamma = sum_rows |dy xhat|, comp dbeta = sum_rows |dy|.
The f32 row mean carries an error of about u (|mean| + sigma), so x - mean, of size sigma, carries the RELATIVE error
u kappa, kappa = (|mean| + sigma) / sigma per row, and so do xhat, rstd and both projections: the dx constant is
    c_ln_dx(C) kappa_row,  c_ln_dx(C) = 4 sqrt(C) + 16
(the constant of tests/test_vit_grad_ops_gpu.py; kappa = 1.25 for its x = 0.5 + 2 randn, 51 for x = 50 + randn).  The
error of xhat is absolute, (C / 64 + 8) u kappa (C / 64 lane additions, 6 exchange steps, the division and x - mean),
not relative to |xhat|: in the column sums, which run in float64 over f32 products, it leaves
    |d dgamma_c| <= u (4 sum_r |dy xhat| + (C / 64 + 8) sum_r kappa_r |dy|)     (``shift_dgamma`` is the second sum)
(4: the relative part of xhat's error, 3 u, and the final rounding), and dbeta, a float64 sum of f32 values rounded
once, |d dbeta_c| <= u |dbeta_c| + 2^-45 comp.  LN_FAULTS: 'last_row_skipped' (the column sums miss the last row),
'last_column_skipped' (the row means of gx and gx xhat miss the last column), 'boundary_row_twice' (the last row of
the first chunk of the column sums counted twice).

GELU, y = x Phi(x), dx = g (Phi(x) + x phi(x)), computed as 0.5 x (1 + erf(x / sqrt 2)): 1 + erff is quantised at
2^-24 of 1, not of Phi(x), so the magnitude of the computed cdf is 0.5 (1 + |erf|) = Phi(|x|) <= 1.  Forward:
|dy| <= 8 u |x| (erff to 4 ulps, its argument, 1 + erf and the two products one each, halved by the 0.5).  Backward:
|d dx| <= u |g| (8 Phi(|x|) + (8 + x^2) |x| phi(x)): the exponent -x^2 / 2 carries two roundings of size u x^2 / 2.
A bf16 output adds one rounding, 2^-8 |want|.

rows_period_sum: B - 1 f32 additions, |d| <= B u sum_b |x|.
"""
from __future__ import annotations

import math

import torch

U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
TINY = 2.0 ** -126          # f32 / bf16 smallest normal: the floor of every allowance (expf flushes below it)

ATTENTION_FAULTS = ("unmasked_key", "dropped_last_key", "dropped_last_query", "D_zero")
LN_FAULTS = ("last_row_skipped", "last_column_skipped", "boundary_row_twice")

ATTN_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 577)
ATTN_HD = (32, 64)
ATTN_BH = ((1, 1), (2, 3))
PEAKED_N = 97
LN_LARGE_MEAN_SHAPE = (7, 100)          # x = 50 + randn
LN_SHAPES = ((1, 8), (3, 63), (5, 65), (7, 100), (1023, 64), (1025, 36), (262151, 8))


def c_attention_f32(N: int, hd: int) -> float:
    return 4 * (math.sqrt(N) + math.sqrt(hd)) + 16


def c_attention_f64_vs_bf16(N: int) -> float:
    """The per-tensor constant of the bf16 kernels against float64 (tests/test_vit_grad_ops_gpu.py)."""
    return 2 * math.sqrt(N) + 4


def c_model(N: int, hd: int) -> float:
    return hd / 32 + N / 32 + 24


def c_ln_dx(C: int) -> float:
    return 4 * math.sqrt(C) + 16


def rn_bf16(x: torch.Tensor) -> torch.Tensor:
    """The nearest bf16 value (ties to even) of float64 x, as float64: one rounding, no detour through f32."""
    _, e = torch.frexp(x)
    q = torch.ldexp(torch.ones_like(x), e.clamp_min(-125) - 8)
    return torch.round(x / q) * q


def within(got, want, bound):
    """(all |got - want| <= bound, worst |got - want| / bound); a NaN never passes."""
    d = (got.double().cpu() - want.double().cpu()).abs()
    bound = bound.double().cpu()
    if d.numel() == 0:
        return True, 0.0
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return bool((d <= bound).all()), float(r.max())


def inside_model(got, x, E):
    """got (bf16 values) against the model's pre-rounding x and allowance E: (all rn(x - E) <= got <= rn(x + E),
    worst share of E that got needs: (|got - x| - half an ulp of got) / E)."""
    got = got.double().cpu()
    ok = bool(((got >= rn_bf16(x - E)) & (got <= rn_bf16(x + E))).all())
    _, e = torch.frexp(got)
    half = torch.ldexp(torch.ones_like(got), e.clamp_min(-125) - 9)
    need = ((got - x).abs() - half).clamp_min(0)
    r = torch.where(need == 0, torch.zeros_like(need), need / E.clamp_min(1e-300))
    r = torch.where(torch.isnan(got), torch.full_like(r, math.inf), r)
    return ok, (float(r.max()) if r.numel() else 0.0)


# ---------------------------------------------------------------------------------------------------------------
# attention backward
# ---------------------------------------------------------------------------------------------------------------
def attention_inputs(B, N, heads, hd, seed, peaked=False, dtype=torch.bfloat16):
    """(qkv [B N, 3 C], dO [B N, C]) f32 CPU, every value a value of ``dtype``; peaked: q and k times 4, so that |s|
    reaches about 50 and the rows of P are nearly one-hot."""
    C = heads * hd
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn((B * N, 3 * C), generator=gen).to(dtype).float()
    dO = torch.randn((B * N, C), generator=gen).to(dtype).float()
    if peaked:
        qkv[:, :2 * C] *= 4
    return qkv, dO


def _heads(t, B, N, heads, hd):
    return t.double().reshape(B, N, heads, hd).permute(0, 2, 1, 3)


def _rows(t, B, N, heads, hd):
    return t.permute(0, 2, 1, 3).reshape(B * N, heads * hd)


def _split(qkv, B, N, heads, hd):
    C = heads * hd
    return tuple(_heads(qkv[:, i * C:(i + 1) * C], B, N, heads, hd) for i in range(3))


def attention_forward(qkv, B, N, heads, hd):
    """O [B N, C] in float64."""
    q, k, v = _split(qkv.cpu(), B, N, heads, hd)
    P = torch.softmax(hd ** -0.5 * (q @ k.transpose(-1, -2)), -1)
    return _rows(P @ v, B, N, heads, hd)


def _attention(qkv, O, dO, B, N, heads, hd, fault, model):
    assert fault is None or fault in ATTENTION_FAULTS, fault
    q, k, v = _split(qkv.cpu(), B, N, heads, hd)
    o, g = _heads(O.cpu(), B, N, heads, hd), _heads(dO.cpu(), B, N, heads, hd)
    scale = hd ** -0.5
    T = lambda t: t.transpose(-1, -2)  # noqa: E731
    s = scale * (q @ T(k))
    se = torch.cat([s, torch.zeros_like(s[..., :1])], -1) if fault == "unmasked_key" else s
    lse = torch.logsumexp(se, -1, keepdim=True)
    P = torch.exp(s - lse)
    dP = g @ T(v)
    D = (g * o).sum(-1, keepdim=True)
    if fault == "D_zero":
        D = torch.zeros_like(D)
    dS = P * (dP - D)
    Pb, dSb = (rn_bf16(P), rn_bf16(dS)) if model else (P, dS)
    dSq, dSk, Pk = dSb, dSb, Pb
    if fault == "dropped_last_key":
        dSq = dSb.clone()
        dSq[..., :, N - 1] = 0
    if fault == "dropped_last_query":
        dSk, Pk = dSb.clone(), Pb.clone()
        dSk[..., N - 1, :] = 0
        Pk[..., N - 1, :] = 0
    cat = lambda a, b, c: torch.cat([_rows(t, B, N, heads, hd) for t in (a, b, c)], 1)  # noqa: E731
    x = cat(scale * (dSq @ k), scale * (T(dSk) @ q), T(Pk) @ g)
    b = g.abs() @ T(v.abs())
    e = (g.abs() * o.abs()).sum(-1, keepdim=True)
    if model and fault is not None:          # a planted fault is judged by the fault-free model's allowance
        return x, None
    if not model:
        w = P * (b + e)
        return x, cat(scale * (w @ k.abs()), scale * (T(w) @ q.abs()), T(P) @ g.abs())
    a = scale * (q.abs() @ T(k.abs()))
    A = a + a.amax(-1, keepdim=True) + s.abs() + lse.abs() + 1
    cu = c_model(N, hd) * U_F32
    eP = cu * A * P + TINY
    eS = cu * P * (A * (dP - D).abs() + b + e) + TINY
    fP = torch.maximum(rn_bf16(P + eP) - Pb, Pb - rn_bf16(P - eP))
    fS = torch.maximum(rn_bf16(dS + eS) - dSb, dSb - rn_bf16(dS - eS))
    wS = fS + cu * (dSb.abs() + fS)
    wP = fP + cu * (Pb.abs() + fP)
    E = cat(scale * (wS @ k.abs()), scale * (T(wS) @ q.abs()), T(wP) @ g.abs()) + TINY
    return x, E


def attention_backward(qkv, O, dO, B, N, heads, hd, fault=None):
    """(dqkv, companion), both [B N, 3 C] float64: the exact backward from row-layout qkv / O / dO."""
    return _attention(qkv, O, dO, B, N, heads, hd, fault, False)


def attention_backward_bf16_model(qkv, O, dO, B, N, heads, hd, fault=None):
    """(x, E) [B N, 3 C] float64: the bf16 MFMA kernels' roundings in float64 ahead of the final one (the model's dqkv is
    rn_bf16(x)), and the allowance of the module docstring (None with a ``fault``: a fault is judged by the fault-free
    model's allowance)."""
    return _attention(qkv, O, dO, B, N, heads, hd, fault, True)


def ratio_per_tensor(got, want, u, c) -> float:
    """max |got - want| / (c u max|want|), 0 where both vanish (head_grad_reference.ratio)."""
    got, want = got.double().cpu(), want.double().cpu()
    mag, err = float(want.abs().max()), float((got - want).abs().max())
    if not math.isfinite(err):
        return math.inf
    return err / (c * u * mag) if mag > 0 else (0.0 if err == 0 else math.inf)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------
def ln_chunk_rows(rows: int) -> int:
    """Rows per chunk of the column sums: ceil(rows / 1024) chunks, at most 256."""
    P = min(max((rows + 1023) // 1024, 1), 256)
    return (rows + P - 1) // P


def ln_inputs(rows, C, seed, mean=0.5, std=2.0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, C), generator=gen) * std + mean
    gamma = 0.8 + 0.4 * torch.rand(C, generator=gen)
    dy = torch.randn((rows, C), generator=gen)
    dres0 = torch.randn((rows, C), generator=gen)
    return x, gamma, dy, dres0


def layernorm_backward(x, gamma, dy, eps, fault=None):
    """dict(dx, dgamma, dbeta, comp_dx, comp_dgamma, comp_dbeta, kappa [rows, 1], shift_dgamma) in float64."""
    assert fault is None or fault in LN_FAULTS, fault
    x, gamma, dy = x.double().cpu(), gamma.double().cpu(), dy.double().cpu()
    rows, C = x.shape
    mean = x.mean(1, keepdim=True)
    sigma = torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    rstd = 1.0 / sigma
    xhat = (x - mean) * rstd
    gx = gamma * dy
    n = C - 1 if fault == "last_column_skipped" else C
    m1 = gx[:, :n].sum(1, keepdim=True) / C
    m2 = (gx * xhat)[:, :n].sum(1, keepdim=True) / C
    dx = rstd * (gx - m1 - xhat * m2)
    w = torch.ones((rows, 1), dtype=torch.float64)
    if fault == "last_row_skipped":
        w[rows - 1] = 0
    if fault == "boundary_row_twice":
        w[min(ln_chunk_rows(rows), rows) - 1] = 2
    kappa = (mean.abs() + sigma) / sigma
    return dict(dx=dx, dgamma=(w * dy * xhat).sum(0), dbeta=(w * dy).sum(0),
                comp_dx=rstd * (gx.abs() + gx.abs().mean(1, keepdim=True)
                                + xhat.abs() * (gx * xhat).abs().mean(1, keepdim=True)),
                comp_dgamma=(dy * xhat).abs().sum(0), comp_dbeta=dy.abs().sum(0), kappa=kappa,
                shift_dgamma=(kappa * dy.abs()).sum(0))


def ln_bounds(ref, C):
    """(dx, dgamma, dbeta) element-wise bounds of the module docstring."""
    return (c_ln_dx(C) * ref["kappa"] * U_F32 * ref["comp_dx"],
            U_F32 * (4 * ref["comp_dgamma"] + (C / 64 + 8) * ref["shift_dgamma"]),
            U_F32 * ref["dbeta"].abs() + 2.0 ** -45 * ref["comp_dbeta"])


# ---------------------------------------------------------------------------------------------------------------
# GELU, rows_period_sum
# ---------------------------------------------------------------------------------------------------------------
def gelu(x, g=None):
    """Forward (g None): (y, bound) with bound = 8 u |x|; backward: (dx, bound).  Float64; Phi from erfc, so the
    negative tail keeps its digits."""
    x = x.double().cpu()
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    if g is None:
        return x * cdf, 8 * U_F32 * x.abs()
    g = g.double().cpu()
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    cdf_abs = 0.5 * torch.special.erfc(-x.abs() / math.sqrt(2.0))
    return g * (cdf + x * pdf), U_F32 * g.abs() * (8 * cdf_abs + (8 + x * x) * x.abs() * pdf)


def gelu_inputs(n, seed):
    """x of n elements over [-8, 8] with the special values +-0, +-40, 1e-30 and a run inside [-8, -4] planted at
    the front (as many as fit), and g."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, generator=gen) * 16 - 8
    g = torch.randn(n, generator=gen)
    special = torch.tensor([0.0, -0.0, 40.0, -40.0, 1e-30, -8.0, -4.0, -5.0, -6.25, -7.5, -4.5])
    m = min(n, special.numel())
    x[:m] = special[:m]
    return x, g


def rows_period_sum(x, B, N, C):
    """(sum over b, bound B u sum_b |x|)."""
    x = x.double().cpu().reshape(B, N, C)
    return x.sum(0), B * U_F32 * x.abs().sum(0)
