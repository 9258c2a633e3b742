"""Tensor-level wrappers over the C ABI (include/probpose_hip.h).

Every function takes torch tensors that already live on the GPU, launches on
torch's current stream and returns immediately (no sync, no hidden copies), so
a whole forward can be captured into a HIP graph.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_FUSE_FINAL, EPI_GELU, EPI_HEATMAP, EPI_NOCLAMP, EPI_OUT_F32, EPI_OUT_FP8, EPI_RELU,  # noqa: F401
                   EPI_RESIDUAL, EPI_ROWBIAS, PP_BF16, PP_F32, PP_FP8)

FP8 = torch.float8_e4m3fn          # OCP e4m3: what gfx950's fp8 MFMA and conversions use
FP8_MAX = 448.0
_DT = {torch.float32: PP_F32, torch.bfloat16: PP_BF16, FP8: PP_FP8}


_PROFILE = None  # bench.py's kernel-level timing hook: list of (name, work, start_event, end_event)


def set_profile(sink):
    """sink = list to append (name, algorithmic_work, start, end) records to, or None to disable."""
    global _PROFILE
    _PROFILE = sink


def _timed(name, work, fn, info=""):
    if _PROFILE is None:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = fn()
    e.record()
    _PROFILE.append((name, work, s, e, info))
    return r


def _run(label, work, name, *args, info=""):
    """One launch of the library entry ``name`` on the current stream, under ``label`` in the profile."""
    return _timed(label, work, lambda: _lib.launch(name, *args), info)


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DT[dt]
    except KeyError:
        raise TypeError(f"compute dtype must be torch.float32, torch.bfloat16 or torch.float8_e4m3fn, got {dt}") from None


def _p(t):
    return _lib.ptr(t)


# Tile autotuning ("measure, don't guess"): the best output-tile configuration of pp_gemm depends on the
# shape (tile quantisation against 256 CUs, K length, epilogue) and varies by several percent between
# devices.  With AUTOTUNE on, the first call of every distinct GEMM signature times the candidate
# configurations on scratch outputs (HIP events, outside any graph capture) and caches the winner.
AUTOTUNE = False
_TUNE_CACHE: dict = {}
_TUNE_CANDIDATES = (2, 3, 4, 5, 6, 7, 9, 10, 13, 14, 18, 19, 20)


def save_tune_cache(path: str) -> None:
    """Persist the per-shape winners (JSON) so that a later process (e.g. a profiled run) starts tuned."""
    import json
    rows = [[*(str(v) if isinstance(v, torch.dtype) else v for v in k), best] for k, best in _TUNE_CACHE.items()]
    with open(path, "w") as f:
        json.dump(rows, f)


def load_tune_cache(path: str) -> int:
    import json
    with open(path) as f:
        rows = json.load(f)
    names = {str(d): d for d in (torch.bfloat16, torch.float32)}
    for r in rows:
        _TUNE_CACHE[tuple(names.get(v, v) if isinstance(v, str) else v for v in r[:-1])] = int(r[-1])
    return len(rows)


def _tune(a, key, out, residual):
    L = _lib.lib()
    stream = _lib.stream_ptr()
    scratch = torch.empty_like(out)
    c_saved, r_saved = a.C, a.residual
    a.C = _p(scratch)
    if residual is not None:
        a.residual = _p(scratch)
    # interleaved rounds in one process, median per candidate (a single 5-launch sample ranked tiles wrongly:
    # clocks drift by several percent between back-to-back launches)
    ok = []
    for cand in _TUNE_CANDIDATES:
        a.tile = cand
        if L.pp_gemm(C.byref(a), stream) == 0:      # configuration applicable to this problem
            ok.append(cand)
    times = {c: [] for c in ok}
    for _ in range(4):
        for cand in ok:
            a.tile = cand
            L.pp_gemm(C.byref(a), stream)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(6):
                L.pp_gemm(C.byref(a), stream)
            e.record()
            e.synchronize()
            times[cand].append(s.elapsed_time(e))
    best, best_t = 0, float("inf")
    for cand in ok:
        t = sorted(times[cand])[len(times[cand]) // 2]
        if t < best_t:
            best, best_t = cand, t
    a.C, a.residual = c_saved, r_saved
    _TUNE_CACHE[key] = best
    return best


def gemm(A, W, out, *, M, N, Kd, lda, ldw, ldc, bias=None, residual=None, rowbias=None,
         rowbias_period=0, rowoff=None, seg_len=0, out_rowmap=None, batch=1, strideA=0, strideW=0,
         strideC=0, strideBias=0, strideRowoff=0, strideRowmap=0, epilogue=0, heatmap=None, tile=0,
         colscale=None, out_scale=None, splitk=1, strideA_k=0, strideW_k=0,
         strideC_k=0, strideRowoff_k=0, fuse_final=None, headmajor=None):
    """C = epilogue(A @ W^T) on MFMA; see pp_gemm in include/probpose_hip.h.
    fp8 (A, W torch.float8_e4m3fn): ``colscale`` [N] f32 = activation scale x weight-row scale; ``out`` may be
    bf16, f32 (with residual) or fp8 (then ``out_scale`` = the scale of the output tensor)."""
    a = _lib.GemmArgs()
    a.A, a.W, a.C = _p(A), _p(W), _p(out)
    a.bias, a.residual, a.rowbias = _p(bias), _p(residual), _p(rowbias)
    a.rowoff, a.out_rowmap = _p(rowoff), _p(out_rowmap)
    a.M, a.N, a.Kd, a.lda, a.ldw, a.ldc = M, N, Kd, lda, ldw, ldc
    a.seg_len, a.rowbias_period, a.batch = seg_len, rowbias_period, batch
    a.strideA, a.strideW, a.strideC, a.strideBias = strideA, strideW, strideC, strideBias
    a.strideRowoff, a.strideRowmap = strideRowoff, strideRowmap
    a.splitk, a.strideA_k, a.strideW_k, a.strideC_k, a.strideRowoff_k = splitk, strideA_k, strideW_k, strideC_k, strideRowoff_k
    a.dtype = dtype_code(W.dtype)
    if bias is not None:
        epilogue |= EPI_BIAS
    if residual is not None:
        epilogue |= EPI_RESIDUAL
    if rowbias is not None:
        epilogue |= EPI_ROWBIAS
    if heatmap is not None:       # (K, HW, temperature[, clamp])
        epilogue |= EPI_HEATMAP
        a.hm_K, a.hm_HW, a.hm_temperature = heatmap[:3]
        if len(heatmap) > 3 and not heatmap[3]:
            epilogue |= EPI_NOCLAMP
    if fuse_final is not None:    # (final_w [K, 256], final_b [K], K, HW, temperature, clamp): out = heat [B, K, HW] f32
        fw, fb, fk, fhw, ftemp, fclamp = fuse_final
        epilogue |= EPI_FUSE_FINAL | (0 if fclamp else EPI_NOCLAMP)
        a.final_w, a.final_b = _p(fw), _p(fb)
        a.hm_K, a.hm_HW, a.hm_temperature = fk, fhw, ftemp
        tile = 9
    if headmajor is not None:     # (heads, head_dim): out is written [3][heads][M][head_dim] (the qkv projection)
        epilogue |= _lib.EPI_HEADMAJOR
        a.hm_K, a.hm_HW = headmajor
    if a.dtype == PP_FP8:
        if colscale is None or A.dtype != FP8:
            raise TypeError("fp8 GEMM: A and W must both be float8_e4m3fn and colscale [N] f32 is required")
        a.colsum = _p(colscale)
        if out.dtype == FP8:
            epilogue |= EPI_OUT_FP8
            a.out_scale = 1.0 / float(out_scale)
        elif out.dtype == torch.float32:
            epilogue |= EPI_OUT_F32
    a.epilogue = epilogue
    a.tile = tile
    if tile == 0 and AUTOTUNE and M * N * Kd >= (1 << 24):
        key = (M, N, Kd, batch * max(1, splitk), a.dtype, rowoff is not None, out_rowmap is not None, epilogue, lda, ldw, ldc)
        best = _TUNE_CACHE.get(key)
        if best is None and not torch.cuda.is_current_stream_capturing():
            best = _tune(a, key, out, residual)
        if best:
            a.tile = best
    _run("gemm", 2.0 * M * N * Kd * batch * max(1, splitk), "pp_gemm", C.byref(a),
         info=f"M={M} N={N} K={Kd} batch={batch} splitk={splitk} gather={rowoff is not None} epi={epilogue}")
    return out


def linear(x, w, bias=None, *, out=None, epilogue=0, residual=None, out_dtype=None, tile=0, colscale=None,
           out_scale=None, headmajor=None):
    """x [M,K] @ w[N,K]^T (+bias, activation / fp32 residual add)."""
    M, Kd = x.shape
    N = w.shape[0]
    if residual is not None or out_dtype == torch.float32:
        epilogue |= EPI_OUT_F32
    if out is None:
        dt = torch.float32 if (epilogue & EPI_OUT_F32) else (out_dtype or (torch.bfloat16 if w.dtype == FP8 else w.dtype))
        out = torch.empty((M, N), dtype=dt, device=x.device)
    return gemm(x, w, out, M=M, N=N, Kd=Kd, lda=x.stride(0), ldw=w.stride(0), ldc=out.stride(0),
                bias=bias, residual=residual, epilogue=epilogue, tile=tile, colscale=colscale, out_scale=out_scale,
                headmajor=headmajor)


def quantize_rows_fp8(w: torch.Tensor):
    """[N,K] float weights -> (float8_e4m3fn [N,K], scale [N] f32): per-output-channel symmetric scaling,
    amax -> 448, round-to-nearest-even (torch's cast)."""
    w32 = w.detach().float()
    scale = (w32.abs().amax(dim=1).clamp_min(1e-12) / FP8_MAX).contiguous()
    return (w32 / scale[:, None]).to(FP8).contiguous(), scale


def layernorm(x, gamma, beta, eps, out, out_scale=None):
    rows, Cc = x.shape
    if out.dtype == FP8:     # static per-tensor scale: out = e4m3(LN(x) / out_scale)
        _run("layernorm", float(rows * Cc * 5), "pp_layernorm_fp8", x, gamma, beta, float(eps), rows, Cc, out,
             1.0 / float(out_scale))
    else:
        _run("layernorm", float(rows * Cc * (4 + out.element_size())), "pp_layernorm", x, gamma, beta, float(eps),
             rows, Cc, out, dtype_code(out.dtype))
    return out


def attention(qkv, out, B, N, heads, hd, out_scale=None, headmajor=False):
    work = 4.0 * B * heads * N * N * hd
    if headmajor:            # qkv [3][heads][B*N][hd] as linear(..., headmajor=(heads, hd)) wrote it
        _run("attention", work, "pp_attention_headmajor", qkv, out, B, N, heads, hd)
    elif out.dtype == FP8:   # e4m3 output with a static per-tensor scale (fp8 mode)
        _run("attention", work, "pp_attention_fp8out", qkv, out, B, N, heads, hd, 1.0 / float(out_scale))
    else:
        _run("attention", work, "pp_attention", qkv, out, B, N, heads, hd, dtype_code(qkv.dtype))
    return out


def pack_qkv_headmajor(qkv_w, qkv_b, heads):
    """qkv.weight [3C, C] / qkv.bias [3C] -> (w_hm [heads*192, C], b_hm [heads*192]) for ``qkv_attention``: row
    192 h + 64 t + d is row t C + 64 h + d of the original (t = 0, 1, 2 for q, k, v; head_dim 64), so the q, k and v
    rows of one head are one contiguous panel of 192 rows."""
    C = qkv_w.shape[1]
    if qkv_w.shape[0] != 3 * C or C != 64 * heads:
        raise ValueError(f"qkv.weight {tuple(qkv_w.shape)} is not [3C, C] with C = 64 * heads (heads = {heads})")
    w_hm = qkv_w.reshape(3, heads, 64, C).permute(1, 0, 2, 3).reshape(3 * C, C).contiguous()
    b_hm = qkv_b.reshape(3, heads, 64).permute(1, 0, 2).reshape(3 * C).contiguous()
    return w_hm, b_hm


def qkv_attention(h, w_hm, b_hm, out, B, heads):
    """out [B*192, C] = attention(h @ qkv.weight^T + qkv.bias) per crop of 192 tokens and head of 64 dims, in one launch
    (pp_qkv_attention_bf16); w_hm / b_hm from ``pack_qkv_headmajor``.  q, k and v are never written to memory."""
    M, C = h.shape
    if h.dtype != torch.bfloat16 or w_hm.dtype != torch.bfloat16 or out.dtype != torch.bfloat16 or \
            b_hm.dtype != torch.float32:
        raise TypeError("qkv_attention: h, w_hm and out are bf16, b_hm is f32")
    if M != B * 192 or tuple(w_hm.shape) != (heads * 192, C) or b_hm.numel() != heads * 192 or h.stride(0) != C or \
            out.stride(0) != C or not w_hm.is_contiguous():
        raise ValueError("qkv_attention: h / out [B*192, C] and w_hm [heads*192, C] contiguous, b_hm [heads*192]")
    _run("qkv_attention", 2.0 * M * 3 * C * C + 4.0 * B * heads * 192 * 192 * 64, "pp_qkv_attention_bf16", h, w_hm,
         b_hm, out, B, heads, C)
    return out


def patchify(x, out, patch):
    B, _, H, W = x.shape
    _lib.launch("pp_patchify", x, out, B, H, W, patch, dtype_code(out.dtype))
    return out


def maxpool_relu(x, out, B, h, w, Cc, kh, kw):
    _lib.launch("pp_maxpool_relu", x, out, B, h, w, Cc, kh, kw, dtype_code(x.dtype))
    return out


def maxpool_relu_sum(parts, bias, out, B, h, w, Cc, kh, kw):
    """parts [S, B*h*w, Cc] f32 split-K partials -> out = ReLU(MaxPool(sum_s parts[s] + bias))."""
    _lib.launch("pp_maxpool_relu_sum", parts, parts.shape[0], parts.stride(0), bias, out, B, h, w, Cc, kh, kw,
                dtype_code(out.dtype))
    return out


def final_heatmap(x, w, bias, out, B, HW, Cin, K, temperature, clamp=True):
    """clamp=False: the unclamped logits z / T that the Sparsemax normalisation takes (head.py:526-528)."""
    _run("final_heatmap", float(B * HW * (Cin * x.element_size() + 4 * K)),
         "pp_final_heatmap" if clamp else "pp_final_logits", x, w, bias, out, B, HW, Cin, K, float(temperature),
         dtype_code(w.dtype))
    return out


def sparsemax_rows(x, scale):
    """In place on x [..., n] f32 contiguous: clamp(sparsemax(x, dim=-1) * scale, 0, 1)  (head.py:528-531)."""
    n = x.shape[-1]
    _run("sparsemax", float(x.numel() * 8), "pp_sparsemax_rows", x, x.numel() // n, n, float(scale))
    return x


def aux_tail(x, w, bias, out, B, Cc, K):
    _lib.launch("pp_aux_tail", x, w, bias, out, B, Cc, K, dtype_code(w.dtype))
    return out


def tokens_to_nchw(x, out, B, N, Cc):
    _lib.launch("pp_tokens_to_nchw", x, out, B, N, Cc, dtype_code(x.dtype))
    return out


def nchw_to_tokens(x, out, B, Cc, HW):
    _lib.launch("pp_nchw_to_tokens", x, out, B, Cc, HW, dtype_code(out.dtype))
    return out


# ---- flip test (pp_flip.hip) ------------------------------------------------------------------------------------
def hflip_pair(x, out):
    """x [B,C,H,W] f32 -> out [2B,C,H,W] f32: the batch followed by its mirror image (columns reversed)."""
    B, Cc, H, W = x.shape
    _run("hflip_pair", float(x.numel() * 12), "pp_hflip_pair", x, out, B, Cc, H, W)
    return out


def flip_merge(heat2, aux2, perm, heat_out, aux_out):
    """heat2 [2B,K,H,W], aux2 [4,2B,K] f32, perm [K] int32 -> heat_out [B,K,H,W], aux_out [4,B,K]: the average of the
    straight half and the un-mirrored, left/right-swapped second half (pp_flip_merge in include/probpose_hip.h)."""
    B, K, H, W = heat_out.shape
    _run("flip_merge", float((heat_out.numel() + aux_out.numel()) * 12), "pp_flip_merge", heat2, aux2, perm, B, K, H,
         W, heat_out, aux_out)
    return heat_out, aux_out


# ---- visualisation (pp_viz.hip) -------------------------------------------------------------------------------------
def viz_render(image, out, heat=None, lut=None, draw=None):
    """image uint8 [B,H,W,3] or f32 [B,3,H,W] -> out uint8 [B,H,W,3]: the overlay of heat [B,K,h,w] through lut [256,3]
    f64, then the primitives of ``draw`` = (kpts [N,Kp,2] f64, probs [N,Kp] f64, inst [N] i32, img_off [B+1] i32,
    style i32, N, Kp, L, threshold, radius, line_width); either half may be None (pp_viz_render in
    include/probpose_hip.h)."""
    B, H, W = out.shape[:3]
    K, h, w = heat.shape[1:] if heat is not None else (0, 0, 0)
    kpts, probs, inst, img_off, style, N, Kp, L, threshold, radius, line_width = draw or (None,) * 5 + (0, 0, 0, 0.0, 0, 1)
    _run("viz_render", float(out.numel() * (2 if image.dtype == torch.uint8 else 5) + B * K * H * W * 4),
         "pp_viz_render", image, int(image.dtype != torch.uint8), out, B, H, W, heat, K, h, w, lut, kpts, probs, inst,
         img_off, N, Kp, style, L, float(threshold), radius, line_width)
    return out


def viz_colorize(maps, lut, out, normalize=False):
    """maps f32 [..., h, w] -> out uint8 [..., h, w, 4] through lut [256,3] f64 (pp_viz_colorize)."""
    h, w = maps.shape[-2:]
    M = maps.numel() // (h * w)
    _run("viz_colorize", float(maps.numel() * (12 if normalize else 8)), "pp_viz_colorize", maps, out, M, h, w, lut,
         int(bool(normalize)))
    return out


# ---- training ProbMapHead (pp_head_grad.hip) ------------------------------------------------------------------
def wgrad_workspace_floats(M, N, Kd, batch=1) -> int:
    return int(_lib.call("pp_wgrad_workspace_floats", M, N, Kd, batch))


def wgrad(dY, A, dW, *, M, N, Kd, ldd, lda=0, rowoff=None, seg_len=0, dy_rowmap=None, dB=None, batch=1, lddw=None,
          strideDY=0, strideA=0, strideRowoff=0, strideRowmap=0, strideDW=0, strideDB=0, parts=None):
    """dW[n, k] = sum_m dY(m, n) A(m, k) (+ dB[n] = sum_m dY(m, n)); see pp_wgrad_gemm in include/probpose_hip.h."""
    a = _lib.WgradArgs()
    a.dY, a.dy_rowmap, a.ldd = _p(dY), _p(dy_rowmap), ldd
    a.A, a.rowoff, a.seg_len, a.lda = _p(A), _p(rowoff), seg_len, lda
    a.dW, a.lddw, a.dB, a.parts = _p(dW), Kd if lddw is None else lddw, _p(dB), _p(parts)
    a.M, a.N, a.Kd, a.batch = M, N, Kd, batch
    a.strideDY, a.strideA, a.strideRowoff, a.strideRowmap = strideDY, strideA, strideRowoff, strideRowmap
    a.strideDW, a.strideDB = strideDW, strideDB
    a.dtype = dtype_code(dY.dtype)
    if A.dtype != dY.dtype:
        raise TypeError(f"wgrad: dY ({dY.dtype}) and A ({A.dtype}) must share the compute dtype")
    need = wgrad_workspace_floats(M, N, Kd, batch)
    if need and (parts is None or parts.numel() < need or parts.dtype != torch.float32):
        raise ValueError(f"wgrad: this shape needs a float32 parts workspace of {need} elements")
    _run("wgrad", 2.0 * M * N * Kd * batch, "pp_wgrad_gemm", C.byref(a), info=f"M={M} N={N} K={Kd} batch={batch}")
    return dW


def bn_workspace_bytes(M, Cc) -> int:
    return int(_lib.call("pp_bn_workspace_bytes", M, Cc))


def bn_train_stats(y, M, Cc, gamma, beta, eps, momentum, running_mean, running_var, mean, rstd, scale, shift, ws):
    _run("bn_stats", float(M * Cc * 4), "pp_bn_train_stats", y, y.stride(0), M, Cc, gamma, beta, float(eps),
         float(momentum), running_mean, running_var, mean, rstd, scale, shift, ws)


def bn_apply_relu(y, M, Cc, scale, shift, out, relu=True):
    _run("bn_apply", float(M * Cc * (4 + out.element_size())), "pp_bn_apply_relu", y, y.stride(0), M, Cc, scale, shift,
         out, out.stride(0), int(relu), dtype_code(out.dtype))
    return out


def bn_pool_relu(y, B, h, w, Cc, kh, kw, scale, shift, out, argmax):
    _run("bn_pool", float(B * h * w * Cc * 4), "pp_bn_pool_relu", y, B, h, w, Cc, kh, kw, scale, shift, out, argmax,
         dtype_code(out.dtype))
    return out


def bn_train_backward(g, y, M, Cc, mean, rstd, gamma, dx, ws, *, mode=0, scale=None, shift=None, argmax=None,
                      pool=(0, 0, 0, 0, 0), dgamma=None, dbeta=None):
    """mode 0: g is the gradient of the BN output; 1: ReLU follows the BN; 2: MaxPool + ReLU follow it (g is the
    pooled gradient, pool = (B, h, w, kh, kw))."""
    _run("bn_backward", float(M * Cc * 12), "pp_bn_train_backward", g, g.stride(0), y, y.stride(0), M, Cc, mean, rstd,
         scale, shift, gamma, mode, argmax, *pool, dgamma, dbeta, dx, dx.stride(0), dtype_code(dx.dtype), ws)
    return dx


def aux_tail_backward(x, w, out, gout, B, Cc, K, dW=None, dB=None, dx=None):
    _run("aux_tail_backward", float(4 * B * K * Cc * 4), "pp_aux_tail_backward", x, w, out, gout, B, Cc, K, dW, dB, dx,
         dtype_code(w.dtype))


def heat_clamp(p, out, scale=1.0):
    _run("heat_clamp", float(p.numel() * 8), "pp_heat_clamp", p, out, p.numel(), float(scale))
    return out


def heat_tail_backward(p, g, B, K, HW, scale, sparse, temperature, dz):
    _run("heat_tail_backward", float(B * K * HW * 12), "pp_heat_tail_backward", p, g, B, K, HW, float(scale),
         int(sparse), float(temperature), dz, dz.stride(0), dtype_code(dz.dtype))
    return dz


# ---- training ViT backbone (pp_vit_grad.hip) ------------------------------------------------------------------
def layernorm_backward(x, gamma, eps, dy, dres, dres_c, accumulate, dgamma=None, dbeta=None, ws=None):
    """dres (+)= the LayerNorm input gradient of x [rows, C] f32 given dy [rows, C] f32; dres_c = dres in its dtype;
    dgamma / dbeta [C] f32 (optional)."""
    rows, Cc = x.shape
    if ws is None:
        ws = torch.empty(int(_lib.call("pp_layernorm_backward_workspace_bytes", rows, Cc)), dtype=torch.uint8,
                         device=x.device)
    _run("ln_backward", float(rows * Cc * 20), "pp_layernorm_backward", x, gamma, float(eps), rows, Cc, dy,
         dy.stride(0), dres, int(accumulate), dres_c, dtype_code(dres_c.dtype), dgamma, dbeta, ws)
    return dres


def gelu_forward(x, out):
    """out = GELU(x) (exact erf) in out's dtype; x f32 contiguous."""
    _run("gelu", float(x.numel() * (4 + out.element_size())), "pp_gelu_forward", x, x.numel(), out,
         dtype_code(out.dtype))
    return out


def gelu_backward(x, g, dx):
    """dx = g * GELU'(x) in dx's dtype; x, g f32 contiguous."""
    _run("gelu_backward", float(x.numel() * (8 + dx.element_size())), "pp_gelu_backward", x, g, x.numel(), dx,
         dtype_code(dx.dtype))
    return dx


def attention_backward(qkv, out, dout, dqkv, B, N, heads, hd, ws=None):
    """dqkv [B*N, 3C] = the gradient of pp_attention (row-layout qkv) given its output and the output's gradient."""
    if ws is None:
        ws = torch.empty(int(_lib.call("pp_attention_backward_workspace_bytes", B, N, heads)), dtype=torch.uint8,
                         device=qkv.device)
    _run("attention_backward", 10.0 * B * heads * N * N * hd, "pp_attention_backward", qkv, out, dout, dqkv, B, N,
         heads, hd, dtype_code(qkv.dtype), ws)
    return dqkv


def rows_period_sum(x, B, N, Cc, out):
    """out [N, C] = sum over b of x [B*N, C] (f32, fixed order): the pos_embed gradient."""
    _lib.launch("pp_rows_period_sum", x, B, N, Cc, out)
    return out


# ---- stochastic depth in the training backbone (pp_droppath.hip) -----------------------------------------------
def crop_rows_gather(src, idx, B, N, Cc, out, scale=1.0):
    """out [kept*N, C] (f32 or bf16) = scale * the crops idx [kept] (int32) of src [B*N, C] f32."""
    kept = idx.numel()
    _run("crop_rows_gather", float(kept * N * Cc * (4 + out.element_size())), "pp_crop_rows_gather", src, idx, B, kept,
         N, Cc, float(scale), out, dtype_code(out.dtype))
    return out


def droppath_add(r, branch, slot, B, kept, N, Cc, scale, out):
    """out [B*N, C] = r + scale * branch[slot[b]] for the kept crops (slot [B] int32 >= 0), r's bits for the others;
    r, out f32 [B*N, C], branch f32 [kept*N, C]."""
    _run("droppath_add", float((2 * B + kept) * N * Cc * 4), "pp_droppath_add", r, branch, slot, B, kept, N, Cc,
         float(scale), out)
    return out


def crop_rows_scatter_add(dx, idx, B, N, Cc, dres, dres_c):
    """dres[idx[j]] += dx[j] (crops of N rows, f32) in place; the same rows of dres_c = the new dres in its dtype."""
    kept = idx.numel()
    _run("crop_rows_scatter_add", float(kept * N * Cc * (12 + dres_c.element_size())), "pp_crop_rows_scatter_add", dx,
         idx, B, kept, N, Cc, dres, dres_c, dtype_code(dres_c.dtype))
    return dres
