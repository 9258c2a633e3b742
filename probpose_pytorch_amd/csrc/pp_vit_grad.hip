// Backward of the ViT backbone (timm VisionTransformer blocks as probpose/backbone.py:23-40 builds them): LayerNorm
// backward, exact-erf GELU forward / backward on the fc1 pre-activation, multi-head attention backward and the
// pos_embed gradient (a sum over crops).  The linear layers' gradients run on pp_gemm (data) and pp_wgrad_gemm
// (weights).
//
// Every reduction runs in a fixed order (no float atomics), so repeated calls give the same bits.
#include "pp_common.h"

namespace pp {

inline int vg_grid(long long n) {
  long long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// ============================================================================================================
// LayerNorm backward.  y = (x - mean) rstd gamma + beta over each row of C; with gx = gamma dy:
//   dx = rstd (gx - mean(gx) - xhat mean(gx xhat)),  dgamma = sum_rows dy xhat,  dbeta = sum_rows dy.
// Row kernel: one wave per row recomputes the statistics (two-pass, as pp_layernorm) and writes dx into the f32
// residual gradient (added to it, or replacing it) and its copy in the compute dtype; the row statistics go to the
// workspace for the column sums, which run as fixed-order float64 partials over row chunks and a finishing pass.
// ============================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void ln_bwd_rows_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                          float eps, int rows, int C, const float *__restrict__ dy,
                                                          long long ldy, float *__restrict__ dres, int accumulate,
                                                          T *__restrict__ dres_c, float *__restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float *xr = x + (long long)row * C;
  const float *gr = dy + (long long)row * ldy;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = xr[c] - mean;
    q += d * d;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
  float a1 = 0.f, a2 = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float gx = gamma[c] * gr[c];
    a1 += gx;
    a2 += gx * ((xr[c] - mean) * rstd);
  }
  const float m1 = wave_sum(a1) / (float)C, m2 = wave_sum(a2) / (float)C;
  float *dr = dres + (long long)row * C;
  T *dc = dres_c + (long long)row * C;
  for (int c = lane; c < C; c += 64) {
    const float xhat = (xr[c] - mean) * rstd;
    const float d = rstd * (gamma[c] * gr[c] - m1 - xhat * m2);
    const float v = accumulate ? dr[c] + d : d;
    dr[c] = v;
    Store<T>::st(dc + c, v);
  }
  if (lane == 0) {
    stats[2 * row] = mean;
    stats[2 * row + 1] = rstd;
  }
}

constexpr int LN_CH = 64, LN_RL = 4;

__host__ __device__ inline int ln_chunks(int rows) {
  int p = (rows + 1023) / 1024;
  return p < 1 ? 1 : (p > 256 ? 256 : p);
}

__global__ __launch_bounds__(256) void ln_bwd_partial_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                             long long ldy, int rows, int C, int chunk_rows,
                                                             const float *__restrict__ stats,
                                                             double *__restrict__ parts) {
  __shared__ double red[2][LN_RL][LN_CH];
  const int cl = threadIdx.x % LN_CH, rl = threadIdx.x / LN_CH;
  const int c = blockIdx.x * LN_CH + cl, p = blockIdx.y;
  const int P = gridDim.y;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    const int r1 = min(rows, (p + 1) * chunk_rows);
    for (int r = p * chunk_rows + rl; r < r1; r += LN_RL) {
      const float g = dy[(long long)r * ldy + c];
      const float xhat = (x[(long long)r * C + c] - stats[2 * r]) * stats[2 * r + 1];
      s1 += g;
      s2 += (double)g * xhat;
    }
  }
  red[0][rl][cl] = s1;
  red[1][rl][cl] = s2;
  __syncthreads();
  if (rl == 0 && c < C) {
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int i = 0; i < LN_RL; ++i) {
      t1 += red[0][i][cl];
      t2 += red[1][i][cl];
    }
    parts[(long long)p * C + c] = t1;
    parts[(long long)(P + p) * C + c] = t2;
  }
}

__global__ __launch_bounds__(256) void ln_bwd_final_kernel(int C, int P, const double *__restrict__ parts,
                                                           float *dgamma, float *dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double t1 = 0.0, t2 = 0.0;
  for (int p = 0; p < P; ++p) {
    t1 += parts[(long long)p * C + c];
    t2 += parts[(long long)(P + p) * C + c];
  }
  if (dbeta) dbeta[c] = (float)t1;
  if (dgamma) dgamma[c] = (float)t2;
}

// ============================================================================================================
// GELU (timm Mlp act, nn.GELU(): exact erf, the same expression as pp_gemm's f32 GELU epilogue) on the f32 fc1
// pre-activation, and its derivative d/dx [x Phi(x)] = Phi(x) + x phi(x).  Four elements per thread.
// ============================================================================================================
__device__ __forceinline__ float vg_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float vg_gelu_grad(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
  return cdf + x * pdf;
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void gelu_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                   long long n, T *__restrict__ out) {
  const long long n4 = n / 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4 *>(x)[i];
    float r[4] = {v.x, v.y, v.z, v.w};
    if constexpr (BWD) {
      const float4 gv = reinterpret_cast<const float4 *>(g)[i];
      r[0] = gv.x * vg_gelu_grad(r[0]); r[1] = gv.y * vg_gelu_grad(r[1]);
      r[2] = gv.z * vg_gelu_grad(r[2]); r[3] = gv.w * vg_gelu_grad(r[3]);
    } else {
      r[0] = vg_gelu(r[0]); r[1] = vg_gelu(r[1]); r[2] = vg_gelu(r[2]); r[3] = vg_gelu(r[3]);
    }
    if constexpr (sizeof(T) == 4) {
      reinterpret_cast<float4 *>(out)[i] = make_float4(r[0], r[1], r[2], r[3]);
    } else {
      uint2 pk;
      pk.x = pack_bf16x2(r[0], r[1]);
      pk.y = pack_bf16x2(r[2], r[3]);
      reinterpret_cast<uint2 *>(out)[i] = pk;
    }
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = BWD ? g[i] * vg_gelu_grad(x[i]) : vg_gelu(x[i]);
    Store<T>::st(out + i, v);
  }
}

// ============================================================================================================
// Attention backward, FlashAttention-2 split, exact f32 arithmetic on the VALU (the fp32 mode; bf16 runs the MFMA
// kernels below).
// qkv [B*N, 3C] in timm's row layout ([3][heads][hd] along the row, C = heads * hd), O / dO [B*N, C], dqkv [B*N, 3C].
// With s_ij = scale q_i . k_j, P = softmax_j(s), dP_ij = dO_i . v_j, D_i = dO_i . O_i, dS = P (dP - D):
//   dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO.
// (a) dq kernel, per (crop, head, query block): one query row per thread (head_dim 64: two lanes per row, 32 dims
//     each, the dot products joined by one lane exchange); keys stream through LDS; the row's log-sum-exp is
//     recomputed (pass 1), then dQ accumulates in registers (pass 2); lse and D go to the workspace.
// (b) dk / dv kernel, per (crop, head, key block): one key row per thread; the queries, dO, lse and D
//     stream through LDS; P and dS are recomputed from the saved statistics.
// Every sum runs in key / query order: no atomics, deterministic.
// The score s_ij is the argument of an exponential: an absolute error t of it is a relative error t of P_ij, and an f32
// chain over hd products of a score of size 50 (peaked rows) is off by 100 u and more.  So the score alone is summed as
// a compensated dot product (Ogita, Rump, Oishi: Dot2, the result as if accumulated in twice the precision) of the
// unscaled q and k and then scaled by hd^-1/2 held as two floats: it carries one rounding of its own size.
// ============================================================================================================
constexpr int AB_THREADS = 128;
constexpr int AB_CHUNK = 64;      // rows per LDS chunk

template <int SPLIT>
__device__ __forceinline__ float ab_join(float v) {
  if constexpr (SPLIT == 2) v += __shfl_xor(v, 1, 64);
  return v;
}

// hi + lo += a b, exactly but for second-order terms (TwoProduct by fma, Knuth's TwoSum; -ffp-contract=off)
__device__ __forceinline__ void ab_dot2(float a, float b, float &hi, float &lo) {
  const float p = a * b;
  const float ep = fmaf(a, b, -p);
  const float t = hi + p;
  const float z = t - hi;
  const float es = (hi - (t - z)) + (p - z);
  hi = t;
  lo += ep + es;
}

// the 32 dims of a lane: q in registers against a row of 8 float4
__device__ __forceinline__ void ab_dot2_row(const float (&q)[32], const float4 *kr, float &hi, float &lo) {
  hi = 0.f;
  lo = 0.f;
#pragma unroll
  for (int d4 = 0; d4 < 8; ++d4) {
    const float4 kv = kr[d4];
    ab_dot2(q[4 * d4], kv.x, hi, lo); ab_dot2(q[4 * d4 + 1], kv.y, hi, lo);
    ab_dot2(q[4 * d4 + 2], kv.z, hi, lo); ab_dot2(q[4 * d4 + 3], kv.w, hi, lo);
  }
}

// scale (sc_hi + sc_lo) times the dot product hi + lo, the two half rows of head_dim 64 joined first (TwoSum's error
// term is exact, so both lanes of a pair hold the same bits)
template <int SPLIT>
__device__ __forceinline__ float ab_score(float hi, float lo, float sc_hi, float sc_lo) {
  if constexpr (SPLIT == 2) {
    const float h2 = __shfl_xor(hi, 1, 64), l2 = __shfl_xor(lo, 1, 64);
    const float t = hi + h2;
    const float z = t - hi;
    lo = ((hi - (t - z)) + (h2 - z)) + (lo + l2);
    hi = t;
  }
  const float p = hi * sc_hi;
  const float e = fmaf(hi, sc_hi, -p);
  return p + (e + (hi * sc_lo + lo * sc_hi));
}

template <typename T, int HD>
__global__ __launch_bounds__(AB_THREADS) void attn_bwd_dq_kernel(const T *__restrict__ qkv, const T *__restrict__ o,
                                                                 const T *__restrict__ dout, T *__restrict__ dqkv,
                                                                 float *__restrict__ ws, int N, int heads,
                                                                 float scale, float scale_lo) {
  constexpr int SPLIT = HD / 32, ROWS = AB_THREADS / SPLIT;
  __shared__ __attribute__((aligned(16))) float Ks[AB_CHUNK * HD];
  __shared__ __attribute__((aligned(16))) float Vs[AB_CHUNK * HD];
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int C = heads * HD, ld = 3 * C;
  const int part = threadIdx.x % SPLIT, r = threadIdx.x / SPLIT;
  const int i = blockIdx.y * ROWS + r;
  const bool active = i < N;
  const T *base = qkv + (long long)b * N * ld;
  const int d0 = part * 32;
  float q[32], dob[32], dq[32];
  float Dp = 0.f;
#pragma unroll
  for (int d = 0; d < 32; ++d) {
    const long long orow = ((long long)b * N + i) * C + h * HD + d0 + d;
    q[d] = active ? Store<T>::ld(base + (long long)i * ld + h * HD + d0 + d) : 0.f;
    dob[d] = active ? Store<T>::ld(dout + orow) : 0.f;
    Dp = fmaf(dob[d], active ? Store<T>::ld(o + orow) : 0.f, Dp);
    dq[d] = 0.f;
  }
  const float D = ab_join<SPLIT>(Dp);
  // pass 1: the row's log-sum-exp
  float m = -__builtin_inff(), l = 0.f;
  for (int k0 = 0; k0 < N; k0 += AB_CHUNK) {
    const int kc = min(AB_CHUNK, N - k0);
    __syncthreads();
    for (int e = threadIdx.x; e < kc * HD; e += AB_THREADS) {
      const int kk = e / HD, d = e - kk * HD;
      Ks[e] = Store<T>::ld(base + (long long)(k0 + kk) * ld + C + h * HD + d);
    }
    __syncthreads();
    for (int j = 0; j < kc; ++j) {
      float a, al;
      ab_dot2_row(q, reinterpret_cast<const float4 *>(Ks + j * HD + d0), a, al);
      const float sc = ab_score<SPLIT>(a, al, scale, scale_lo);
      const float mn = fmaxf(m, sc);
      l = l * expf(m - mn) + expf(sc - mn);
      m = mn;
    }
  }
  const float lse = m + logf(l);
  // pass 2: dQ = sum_j dS_ij k_j (scale applied at the end)
  for (int k0 = 0; k0 < N; k0 += AB_CHUNK) {
    const int kc = min(AB_CHUNK, N - k0);
    __syncthreads();
    for (int e = threadIdx.x; e < kc * HD; e += AB_THREADS) {
      const int kk = e / HD, d = e - kk * HD;
      const T *row = base + (long long)(k0 + kk) * ld + h * HD + d;
      Ks[e] = Store<T>::ld(row + C);
      Vs[e] = Store<T>::ld(row + 2 * C);
    }
    __syncthreads();
    for (int j = 0; j < kc; ++j) {
      const float4 *kr = reinterpret_cast<const float4 *>(Ks + j * HD + d0);
      const float4 *vr = reinterpret_cast<const float4 *>(Vs + j * HD + d0);
      float a, al, dp = 0.f;
      ab_dot2_row(q, kr, a, al);
#pragma unroll
      for (int d4 = 0; d4 < 8; ++d4) {
        const float4 vv = vr[d4];
        dp = fmaf(dob[4 * d4], vv.x, dp); dp = fmaf(dob[4 * d4 + 1], vv.y, dp);
        dp = fmaf(dob[4 * d4 + 2], vv.z, dp); dp = fmaf(dob[4 * d4 + 3], vv.w, dp);
      }
      const float p = expf(ab_score<SPLIT>(a, al, scale, scale_lo) - lse);
      const float ds = p * (ab_join<SPLIT>(dp) - D);
#pragma unroll
      for (int d4 = 0; d4 < 8; ++d4) {
        const float4 kv = kr[d4];
        dq[4 * d4] = fmaf(ds, kv.x, dq[4 * d4]); dq[4 * d4 + 1] = fmaf(ds, kv.y, dq[4 * d4 + 1]);
        dq[4 * d4 + 2] = fmaf(ds, kv.z, dq[4 * d4 + 2]); dq[4 * d4 + 3] = fmaf(ds, kv.w, dq[4 * d4 + 3]);
      }
    }
  }
  if (active) {
    T *out = dqkv + ((long long)b * N + i) * ld + h * HD + d0;
#pragma unroll
    for (int d = 0; d < 32; ++d) Store<T>::st(out + d, dq[d] * scale);
    if (part == 0) {
      ws[(long long)bh * 2 * N + i] = lse;
      ws[(long long)bh * 2 * N + N + i] = D;
    }
  }
}

template <typename T, int HD>
__global__ __launch_bounds__(AB_THREADS) void attn_bwd_dkv_kernel(const T *__restrict__ qkv, const T *__restrict__ dout,
                                                                  T *__restrict__ dqkv, const float *__restrict__ ws,
                                                                  int N, int heads, float scale, float scale_lo) {
  constexpr int SPLIT = HD / 32, ROWS = AB_THREADS / SPLIT;
  __shared__ __attribute__((aligned(16))) float Qs[AB_CHUNK * HD];
  __shared__ __attribute__((aligned(16))) float Gs[AB_CHUNK * HD];
  __shared__ float Ls[AB_CHUNK], Dd[AB_CHUNK];
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int C = heads * HD, ld = 3 * C;
  const int part = threadIdx.x % SPLIT, r = threadIdx.x / SPLIT;
  const int j = blockIdx.y * ROWS + r;
  const bool active = j < N;
  const T *base = qkv + (long long)b * N * ld;
  const int d0 = part * 32;
  float k[32], v[32], dk[32], dv[32];
#pragma unroll
  for (int d = 0; d < 32; ++d) {
    const T *row = base + (long long)j * ld + h * HD + d0 + d;
    k[d] = active ? Store<T>::ld(row + C) : 0.f;
    v[d] = active ? Store<T>::ld(row + 2 * C) : 0.f;
    dk[d] = 0.f;
    dv[d] = 0.f;
  }
  const float *lse = ws + (long long)bh * 2 * N, *Dv = lse + N;
  for (int i0 = 0; i0 < N; i0 += AB_CHUNK) {
    const int qc = min(AB_CHUNK, N - i0);
    __syncthreads();
    for (int e = threadIdx.x; e < qc * HD; e += AB_THREADS) {
      const int ii = e / HD, d = e - ii * HD;
      Qs[e] = Store<T>::ld(base + (long long)(i0 + ii) * ld + h * HD + d);
      Gs[e] = Store<T>::ld(dout + ((long long)b * N + i0 + ii) * C + h * HD + d);
    }
    for (int e = threadIdx.x; e < qc; e += AB_THREADS) {
      Ls[e] = lse[i0 + e];
      Dd[e] = Dv[i0 + e];
    }
    __syncthreads();
    for (int ii = 0; ii < qc; ++ii) {
      const float4 *qr = reinterpret_cast<const float4 *>(Qs + ii * HD + d0);
      const float4 *gr = reinterpret_cast<const float4 *>(Gs + ii * HD + d0);
      float a, al, dp = 0.f;
      ab_dot2_row(k, qr, a, al);          // the products and their order are the dq kernel's: the same bits
#pragma unroll
      for (int d4 = 0; d4 < 8; ++d4) {
        const float4 gv = gr[d4];
        dp = fmaf(gv.x, v[4 * d4], dp); dp = fmaf(gv.y, v[4 * d4 + 1], dp);
        dp = fmaf(gv.z, v[4 * d4 + 2], dp); dp = fmaf(gv.w, v[4 * d4 + 3], dp);
      }
      const float p = expf(ab_score<SPLIT>(a, al, scale, scale_lo) - Ls[ii]);
      const float ds = p * (ab_join<SPLIT>(dp) - Dd[ii]);
#pragma unroll
      for (int d4 = 0; d4 < 8; ++d4) {
        const float4 qv = qr[d4], gv = gr[d4];
        dv[4 * d4] = fmaf(p, gv.x, dv[4 * d4]); dv[4 * d4 + 1] = fmaf(p, gv.y, dv[4 * d4 + 1]);
        dv[4 * d4 + 2] = fmaf(p, gv.z, dv[4 * d4 + 2]); dv[4 * d4 + 3] = fmaf(p, gv.w, dv[4 * d4 + 3]);
        dk[4 * d4] = fmaf(ds, qv.x, dk[4 * d4]); dk[4 * d4 + 1] = fmaf(ds, qv.y, dk[4 * d4 + 1]);
        dk[4 * d4 + 2] = fmaf(ds, qv.z, dk[4 * d4 + 2]); dk[4 * d4 + 3] = fmaf(ds, qv.w, dk[4 * d4 + 3]);
      }
    }
  }
  if (active) {
    T *out = dqkv + ((long long)b * N + j) * ld + h * HD + d0;
#pragma unroll
    for (int d = 0; d < 32; ++d) {
      Store<T>::st(out + C + d, dk[d] * scale);
      Store<T>::st(out + 2 * C + d, dv[d]);
    }
  }
}

template <typename T, int HD>
static int attn_bwd_launch(const void *qkv, const void *o, const void *dout, void *dqkv, int B, int N, int heads,
                           float *ws, hipStream_t s) {
  constexpr int ROWS = AB_THREADS / (HD / 32);
  const float scale = 1.0f / sqrtf((float)HD);
  const float scale_lo = (float)(1.0 / sqrt((double)HD) - (double)scale);
  const dim3 grid(B * heads, cdiv(N, ROWS));
  hipLaunchKernelGGL((attn_bwd_dq_kernel<T, HD>), grid, dim3(AB_THREADS), 0, s, (const T *)qkv, (const T *)o,
                     (const T *)dout, (T *)dqkv, ws, N, heads, scale, scale_lo);
  PP_CHECK_LAUNCH("attn_bwd_dq_kernel");
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, HD>), grid, dim3(AB_THREADS), 0, s, (const T *)qkv, (const T *)dout,
                     (T *)dqkv, (const float *)ws, N, heads, scale, scale_lo);
  PP_CHECK_LAUNCH("attn_bwd_dkv_kernel");
  return 0;
}

// ============================================================================================================
// bf16 attention backward on MFMA (v_mfma_f32_16x16x32_bf16, f32 accumulate): the same FA2 split.  A workgroup is 4
// waves; each wave owns 16 rows (queries in (a), keys in (b)) whose operands stay in registers, and the other side
// streams through LDS in blocks of 32 rows, stored row-major and (where a product reduces over those rows) also
// transposed at the write.  Fragment layout (lane = 16 g + i): A lane holds A[i][8 g .. 8 g + 7], B lane holds
// B[8 g .. 8 g + 7][i], the accumulator lane holds C[4 g + r][i].  The score and dP tiles are formed with the
// streamed rows on the MFMA row axis, so one lane holds the 4 x 2 scores of 8 streamed rows against its own row; the
// second products reduce over the streamed rows and take those accumulators straight back as the B operand, slot j of
// lane group g standing for streamed row 4 g + j (j < 4) or 16 + 4 g + j - 4 (the transposed LDS image is read in the
// same order).  P and dS are rounded to bf16 for the second products, as the forward rounds P.
//   (a) per (crop, head, 64 queries): S^T = K Q^T and dP^T = V dO^T per 32-key block; pass 1 the row log-sum-exp,
//       pass 2 dQ^T += K^T dS^T; lse and D = rowsum(dO o O) go to the workspace.
//   (b) per (crop, head, 64 keys): S = Q K^T and dP = dO V^T per 32-query block, P and dS from the saved statistics,
//       dV^T += dO^T P and dK^T += Q^T dS.
// ============================================================================================================
typedef __bf16 vg_bf16x8 __attribute__((ext_vector_type(8)));
typedef float vg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int MB_ROWS = 32;           // streamed rows per LDS block
constexpr int MB_TP = MB_ROWS + 4;    // transposed image pitch (elements): 72 B, 8-B aligned reads

__device__ __forceinline__ vg_f32x4 vg_mfma(uint4 a, uint4 b, vg_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const vg_bf16x8 *>(&a),
                                                 *reinterpret_cast<const vg_bf16x8 *>(&b), c, 0, 0, 0);
}

// rows [r0, r0 + 32) of src (row pitch ld elements, head offset applied) -> R [32][HD + 8] and (TRANS) T [HD][MB_TP];
// rows >= N are zero
template <int HD, bool TRANS>
__device__ __forceinline__ void mb_stage(const bf16_t *__restrict__ src, long long ld, int r0, int N, bf16_t *R,
                                         bf16_t *T) {
  constexpr int CH = HD / 8, RP = HD + 8;
  for (int c = threadIdx.x; c < MB_ROWS * CH; c += blockDim.x) {
    const int row = c / CH, c8 = c - row * CH;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r0 + row < N) v = *reinterpret_cast<const uint4 *>(src + (long long)(r0 + row) * ld + c8 * 8);
    *reinterpret_cast<uint4 *>(R + row * RP + c8 * 8) = v;
    if constexpr (TRANS) {
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        T[(c8 * 8 + 2 * e) * MB_TP + row] = (bf16_t)(w[e] & 0xffffu);
        T[(c8 * 8 + 2 * e + 1) * MB_TP + row] = (bf16_t)(w[e] >> 16);
      }
    }
  }
}

// A / B fragment of row `row` of a row-major LDS block, K-step s
template <int HD>
__device__ __forceinline__ uint4 mb_rowfrag(const bf16_t *R, int row, int s, int g) {
  return *reinterpret_cast<const uint4 *>(R + row * (HD + 8) + 32 * s + 8 * g);
}

// A fragment of row `d` of a transposed block over the 32 streamed rows, in the accumulator slot order
__device__ __forceinline__ uint4 mb_transfrag(const bf16_t *T, int d, int g) {
  const uint2 lo = *reinterpret_cast<const uint2 *>(T + d * MB_TP + 4 * g);
  const uint2 hi = *reinterpret_cast<const uint2 *>(T + d * MB_TP + 16 + 4 * g);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

__device__ __forceinline__ uint4 mb_pack(const float (&v)[2][4]) {
  return make_uint4(pack_bf16x2(v[0][0], v[0][1]), pack_bf16x2(v[0][2], v[0][3]), pack_bf16x2(v[1][0], v[1][1]),
                    pack_bf16x2(v[1][2], v[1][3]));
}

__device__ __forceinline__ float mb_dot8(uint4 a, uint4 b) {
  const unsigned x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s = fmaf(bf16_to_f32((bf16_t)(x[e] & 0xffffu)), bf16_to_f32((bf16_t)(y[e] & 0xffffu)), s);
    s = fmaf(bf16_to_f32((bf16_t)(x[e] >> 16)), bf16_to_f32((bf16_t)(y[e] >> 16)), s);
  }
  return s;
}

__device__ __forceinline__ void mb_store4(bf16_t *p, vg_f32x4 v, float sc) {
  *reinterpret_cast<uint2 *>(p) = make_uint2(pack_bf16x2(v[0] * sc, v[1] * sc), pack_bf16x2(v[2] * sc, v[3] * sc));
}

template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_dq_mfma_kernel(const bf16_t *__restrict__ qkv,
                                                               const bf16_t *__restrict__ o,
                                                               const bf16_t *__restrict__ dout,
                                                               bf16_t *__restrict__ dqkv, float *__restrict__ ws,
                                                               int N, int heads, float scale) {
  constexpr int KS = HD / 32, DT = HD / 16, RP = HD + 8;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[MB_ROWS * RP];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[MB_ROWS * RP];
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int C = heads * HD, ld = 3 * C;
  const bf16_t *base = qkv + (long long)b * N * ld + h * HD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int qi = blockIdx.y * 64 + wave * 16 + i;       // this lane's query (B column, accumulator column)
  const bool qok = qi < N;
  uint4 qf[KS], df[KS];
  float Dp = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    qf[s] = df[s] = make_uint4(0, 0, 0, 0);
    if (qok) {
      const long long orow = ((long long)b * N + qi) * C + h * HD + 32 * s + 8 * g;
      qf[s] = *reinterpret_cast<const uint4 *>(base + (long long)qi * ld + 32 * s + 8 * g);
      df[s] = *reinterpret_cast<const uint4 *>(dout + orow);
      Dp += mb_dot8(df[s], *reinterpret_cast<const uint4 *>(o + orow));
    }
  }
  Dp += __shfl_xor(Dp, 16, 64);
  const float D = Dp + __shfl_xor(Dp, 32, 64);
  // pass 1: the row's log-sum-exp
  float m = -__builtin_inff(), l = 0.f;
  for (int k0 = 0; k0 < N; k0 += MB_ROWS) {
    __syncthreads();
    mb_stage<HD, false>(base + C, ld, k0, N, Ks, nullptr);
    __syncthreads();
    float sv[2][4];
    float mb = -__builtin_inff();
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      vg_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) acc = vg_mfma(mb_rowfrag<HD>(Ks, 16 * kt + i, s, g), qf[s], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sv[kt][r] = (k0 + 16 * kt + 4 * g + r < N) ? acc[r] * scale : -__builtin_inff();
        mb = fmaxf(mb, sv[kt][r]);
      }
    }
    mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
    mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
    const float mn = fmaxf(m, mb);              // finite: key k0 < N
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += expf(sv[kt][r] - mn);
    l = l * expf(m - mn) + sum;
    m = mn;
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float lse = m + logf(l);
  // pass 2: dQ += dS K (the dS^T accumulators are the A operand as they stand: lane (query i, g), slot j = key
  // 4 g + j / 16 + 4 g + j - 4; the B operand gathers the same keys of K for dim column i)
  vg_f32x4 dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = vg_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < N; k0 += MB_ROWS) {
    __syncthreads();
    mb_stage<HD, false>(base + C, ld, k0, N, Ks, nullptr);
    mb_stage<HD, false>(base + 2 * C, ld, k0, N, Vs, nullptr);
    __syncthreads();
    float ds[2][4];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      vg_f32x4 sa = {0.f, 0.f, 0.f, 0.f}, pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        sa = vg_mfma(mb_rowfrag<HD>(Ks, 16 * kt + i, s, g), qf[s], sa);
        pa = vg_mfma(mb_rowfrag<HD>(Vs, 16 * kt + i, s, g), df[s], pa);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = (k0 + 16 * kt + 4 * g + r < N) ? expf(sa[r] * scale - lse) : 0.f;
        ds[kt][r] = p * (pa[r] - D);
      }
    }
    const uint4 dsf = mb_pack(ds);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const bf16_t *kc = Ks + 16 * dt + i;
      unsigned kw[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k0e = 2 * e < 4 ? 4 * g + 2 * e : 16 + 4 * g + 2 * e - 4;
        kw[e] = (unsigned)kc[k0e * RP] | ((unsigned)kc[(k0e + 1) * RP] << 16);
      }
      dq[dt] = vg_mfma(dsf, make_uint4(kw[0], kw[1], kw[2], kw[3]), dq[dt]);
    }
  }
  {   // dq rows: lane (dim column i, g) holds queries 4 g + r of the wave's 16
    const int qw = blockIdx.y * 64 + wave * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = qw + 4 * g + r;
      if (q < N) {
        bf16_t *out = dqkv + ((long long)b * N + q) * ld + h * HD + i;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) out[16 * dt] = f32_to_bf16(dq[dt][r] * scale);
      }
    }
  }
  if (qok) {
    if (g == 0) {
      ws[(long long)bh * 2 * N + qi] = lse;
      ws[(long long)bh * 2 * N + N + qi] = D;
    }
  }
}

template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_dkv_mfma_kernel(const bf16_t *__restrict__ qkv,
                                                                const bf16_t *__restrict__ dout,
                                                                bf16_t *__restrict__ dqkv,
                                                                const float *__restrict__ ws, int N, int heads,
                                                                float scale) {
  constexpr int KS = HD / 32, DT = HD / 16, RP = HD + 8;
  __shared__ __attribute__((aligned(16))) bf16_t Qs[MB_ROWS * RP];
  __shared__ __attribute__((aligned(16))) bf16_t Gs[MB_ROWS * RP];
  __shared__ __attribute__((aligned(16))) bf16_t Qt[HD * MB_TP];
  __shared__ __attribute__((aligned(16))) bf16_t Gt[HD * MB_TP];
  __shared__ float Ls[MB_ROWS], Dd[MB_ROWS];
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int C = heads * HD, ld = 3 * C;
  const bf16_t *base = qkv + (long long)b * N * ld + h * HD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int kj = blockIdx.y * 64 + wave * 16 + i;       // this lane's key (B column, accumulator column)
  const bool kok = kj < N;
  uint4 kf[KS], vf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    kf[s] = vf[s] = make_uint4(0, 0, 0, 0);
    if (kok) {
      kf[s] = *reinterpret_cast<const uint4 *>(base + (long long)kj * ld + C + 32 * s + 8 * g);
      vf[s] = *reinterpret_cast<const uint4 *>(base + (long long)kj * ld + 2 * C + 32 * s + 8 * g);
    }
  }
  const float *lse = ws + (long long)bh * 2 * N, *Dv = lse + N;
  vg_f32x4 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = vg_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < N; q0 += MB_ROWS) {
    __syncthreads();
    mb_stage<HD, true>(base, ld, q0, N, Qs, Qt);
    mb_stage<HD, true>(dout + (long long)b * N * C + h * HD, C, q0, N, Gs, Gt);
    if (threadIdx.x < MB_ROWS) {
      const bool ok = q0 + threadIdx.x < N;
      Ls[threadIdx.x] = ok ? lse[q0 + threadIdx.x] : 0.f;
      Dd[threadIdx.x] = ok ? Dv[q0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    float pv[2][4], ds[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      vg_f32x4 sa = {0.f, 0.f, 0.f, 0.f}, pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        sa = vg_mfma(mb_rowfrag<HD>(Qs, 16 * qt + i, s, g), kf[s], sa);
        pa = vg_mfma(mb_rowfrag<HD>(Gs, 16 * qt + i, s, g), vf[s], pa);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qq = 16 * qt + 4 * g + r;
        const float p = (q0 + qq < N) ? expf(sa[r] * scale - Ls[qq]) : 0.f;
        pv[qt][r] = p;
        ds[qt][r] = p * (pa[r] - Dd[qq]);
      }
    }
    const uint4 pf = mb_pack(pv), dsf = mb_pack(ds);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      dv[dt] = vg_mfma(mb_transfrag(Gt, 16 * dt + i, g), pf, dv[dt]);
      dk[dt] = vg_mfma(mb_transfrag(Qt, 16 * dt + i, g), dsf, dk[dt]);
    }
  }
  if (kok) {
    bf16_t *out = dqkv + ((long long)b * N + kj) * ld + h * HD + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      mb_store4(out + C + 16 * dt, dk[dt], scale);
      mb_store4(out + 2 * C + 16 * dt, dv[dt], 1.0f);
    }
  }
}

template <int HD>
static int attn_bwd_mfma_launch(const void *qkv, const void *o, const void *dout, void *dqkv, int B, int N,
                                int heads, float *ws, hipStream_t s) {
  const float scale = 1.0f / sqrtf((float)HD);
  const dim3 grid(B * heads, cdiv(N, 64));
  hipLaunchKernelGGL((attn_bwd_dq_mfma_kernel<HD>), grid, dim3(256), 0, s, (const bf16_t *)qkv, (const bf16_t *)o,
                     (const bf16_t *)dout, (bf16_t *)dqkv, ws, N, heads, scale);
  PP_CHECK_LAUNCH("attn_bwd_dq_mfma_kernel");
  hipLaunchKernelGGL((attn_bwd_dkv_mfma_kernel<HD>), grid, dim3(256), 0, s, (const bf16_t *)qkv,
                     (const bf16_t *)dout, (bf16_t *)dqkv, (const float *)ws, N, heads, scale);
  PP_CHECK_LAUNCH("attn_bwd_dkv_mfma_kernel");
  return 0;
}

// pos_embed gradient: out[n, c] = sum_b x[(b N + n) C + c], b ascending.
__global__ __launch_bounds__(256) void rows_period_sum_kernel(const float *__restrict__ x, int B, int N, int C,
                                                              float *__restrict__ out) {
  const long long total = (long long)N * C;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += x[(long long)b * total + e];
    out[e] = acc;
  }
}

}  // namespace pp

using namespace pp;

extern "C" long long pp_layernorm_backward_workspace_bytes(int rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  return 2LL * rows * (long long)sizeof(float) + 2LL * ln_chunks(rows) * C * (long long)sizeof(double);
}

extern "C" int pp_layernorm_backward(const float *x, const float *gamma, float eps, int rows, int C, const float *dy,
                                     long long ldy, float *dres, int accumulate, void *dres_c, int dtype,
                                     float *dgamma, float *dbeta, void *ws, void *stream) {
  PP_REQUIRE(rows > 0 && C > 0 && ldy >= C, "pp_layernorm_backward: bad shape rows=%d C=%d ldy=%lld", rows, C, ldy);
  PP_REQUIRE(x && gamma && dy && dres && dres_c && ws, "pp_layernorm_backward: null pointer");
  PP_REQUIRE(dtype == PP_F32 || dtype == PP_BF16, "pp_layernorm_backward: bad dtype %d", dtype);
  PP_REQUIRE(((uintptr_t)ws & 7) == 0, "pp_layernorm_backward: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float *stats = (float *)ws;
  double *parts = (double *)(stats + 2LL * rows);
  if (dtype == PP_BF16)
    hipLaunchKernelGGL(ln_bwd_rows_kernel<bf16_t>, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, gamma, eps, rows, C, dy,
                       ldy, dres, accumulate, (bf16_t *)dres_c, stats);
  else
    hipLaunchKernelGGL(ln_bwd_rows_kernel<float>, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, gamma, eps, rows, C, dy, ldy,
                       dres, accumulate, (float *)dres_c, stats);
  PP_CHECK_LAUNCH("ln_bwd_rows_kernel");
  if (dgamma || dbeta) {
    const int P = ln_chunks(rows);
    hipLaunchKernelGGL(ln_bwd_partial_kernel, dim3(cdiv(C, LN_CH), P), dim3(256), 0, s, x, dy, ldy, rows, C,
                       cdiv(rows, P), (const float *)stats, parts);
    PP_CHECK_LAUNCH("ln_bwd_partial_kernel");
    hipLaunchKernelGGL(ln_bwd_final_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, C, P, (const double *)parts, dgamma,
                       dbeta);
    PP_CHECK_LAUNCH("ln_bwd_final_kernel");
  }
  return 0;
}

static int gelu_launch(const float *x, const float *g, long long n, void *out, int dtype, bool bwd, void *stream) {
  PP_REQUIRE(n >= 0, "pp_gelu: bad length %lld", n);
  if (n == 0) return 0;
  PP_REQUIRE(x && out && (!bwd || g), "pp_gelu: null pointer");
  PP_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0 && (!bwd || ((uintptr_t)g & 15) == 0),
             "pp_gelu: buffers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int grid = vg_grid((n + 3) / 4);
  if (dtype == PP_BF16) {
    if (bwd) hipLaunchKernelGGL((gelu_kernel<bf16_t, true>), dim3(grid), dim3(256), 0, s, x, g, n, (bf16_t *)out);
    else hipLaunchKernelGGL((gelu_kernel<bf16_t, false>), dim3(grid), dim3(256), 0, s, x, g, n, (bf16_t *)out);
  } else if (dtype == PP_F32) {
    if (bwd) hipLaunchKernelGGL((gelu_kernel<float, true>), dim3(grid), dim3(256), 0, s, x, g, n, (float *)out);
    else hipLaunchKernelGGL((gelu_kernel<float, false>), dim3(grid), dim3(256), 0, s, x, g, n, (float *)out);
  } else {
    return fail("pp_gelu: bad dtype %d", dtype);
  }
  PP_CHECK_LAUNCH("gelu_kernel");
  return 0;
}

extern "C" int pp_gelu_forward(const float *x, long long n, void *out, int dtype, void *stream) {
  return gelu_launch(x, nullptr, n, out, dtype, false, stream);
}

extern "C" int pp_gelu_backward(const float *x, const float *g, long long n, void *dx, int dtype, void *stream) {
  return gelu_launch(x, g, n, dx, dtype, true, stream);
}

extern "C" long long pp_attention_backward_workspace_bytes(int B, int N, int heads) {
  if (B <= 0 || N <= 0 || heads <= 0) return 0;
  return 2LL * B * heads * N * (long long)sizeof(float);
}

extern "C" int pp_attention_backward(const void *qkv, const void *out, const void *dout, void *dqkv, int B, int N,
                                     int heads, int hd, int dtype, void *ws, void *stream) {
  PP_REQUIRE(B > 0 && N > 0 && heads > 0, "pp_attention_backward: bad shape B=%d N=%d heads=%d", B, N, heads);
  PP_REQUIRE(hd == 32 || hd == 64, "pp_attention_backward: head_dim %d not supported (32, 64)", hd);
  PP_REQUIRE(qkv && out && dout && dqkv && ws, "pp_attention_backward: null pointer");
  PP_REQUIRE((long long)B * heads <= 0x7fffffffLL && cdiv(N, 64) <= 65535, "pp_attention_backward: grid too large");
  hipStream_t s = (hipStream_t)stream;
  float *w = (float *)ws;
  if (dtype == PP_BF16) {
    PP_REQUIRE((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dqkv) & 15) == 0,
               "pp_attention_backward: bf16 buffers must be 16-byte aligned");
    return hd == 32 ? attn_bwd_mfma_launch<32>(qkv, out, dout, dqkv, B, N, heads, w, s)
                    : attn_bwd_mfma_launch<64>(qkv, out, dout, dqkv, B, N, heads, w, s);
  }
  if (dtype == PP_F32)
    return hd == 32 ? attn_bwd_launch<float, 32>(qkv, out, dout, dqkv, B, N, heads, w, s)
                    : attn_bwd_launch<float, 64>(qkv, out, dout, dqkv, B, N, heads, w, s);
  return fail("pp_attention_backward: bad dtype %d", dtype);
}

extern "C" int pp_rows_period_sum(const float *x, int B, int N, int C, float *out, void *stream) {
  PP_REQUIRE(B > 0 && N > 0 && C > 0, "pp_rows_period_sum: bad shape B=%d N=%d C=%d", B, N, C);
  PP_REQUIRE(x && out, "pp_rows_period_sum: null pointer");
  hipLaunchKernelGGL(rows_period_sum_kernel, dim3(vg_grid((long long)N * C)), dim3(256), 0, (hipStream_t)stream, x, B,
                     N, C, out);
  PP_CHECK_LAUNCH("rows_period_sum_kernel");
  return 0;
}
