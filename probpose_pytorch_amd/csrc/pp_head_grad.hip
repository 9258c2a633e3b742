// Training (train-mode BatchNorm) forward pieces and the backward of ProbMapHead (reference probpose/head.py:174-405,
// 487-594): the weight-gradient GEMM of every (de)convolution, train-mode BatchNorm statistics / apply / backward,
// the aux branches' arg-max pooling and its scatter, the 1x1 aux tail backward, and the heatmap tail (clamp,
// /temperature, Sparsemax) backward.  Input gradients of the convolutions run on pp_gemm with transposed weights and
// the gather tables of pack.py.
//
// Every reduction runs in a fixed order (row chunks summed chunk by chunk, no float atomics), so repeated calls give
// the same bits.
#include "pp_common.h"

typedef __bf16 hg_bf16x8 __attribute__((ext_vector_type(8)));
typedef float hg_f32x4 __attribute__((ext_vector_type(4)));

namespace pp {

// ============================================================================================================
// Weight-gradient GEMM: dW[n, k] = sum_m dY(m, n) * A(m, k)
//
// One workgroup (4 waves) owns a 64 (n) x 64 (k) tile of dW and a range of rows m.  Per step it stages a 32-row slab
// of dY and of A through LDS, TRANSPOSED at the write ([n][m] and [k][m]): the reduction runs over m, so an MFMA
// operand needs consecutive m of one column, which the transposed image gives as one contiguous 16-byte read (bf16:
// 8 m per lane for v_mfma_f32_16x16x32_bf16; fp32: one m per lane for v_mfma_f32_16x16x4_f32).  The rows come
// straight from the channels-last activations through the forward's gather tables -- no im2col, no transposed copy
// in HBM.  Each wave computes a 32 x 32 quarter of the tile as 2 x 2 MFMA blocks.
// ============================================================================================================
constexpr int WG_T = 64;     // tile edge (n and k)
constexpr int WG_M = 32;     // rows per LDS slab
constexpr int WG_THREADS = 256;

template <typename T> struct WgLds {
  // row pitch in elements: bf16 40 (80 B: 16-B aligned rows for the b128 operand reads), fp32 33 (odd: no conflicts)
  static constexpr int P = sizeof(T) == 2 ? WG_M + 8 : WG_M + 1;
};

template <typename T>
__device__ __forceinline__ T zero_of() {
  if constexpr (sizeof(T) == 2) return (T)0;
  else return 0.f;
}

template <typename T>
__device__ __forceinline__ void load8(const T *p, T *v) {
  if constexpr (sizeof(T) == 2) {
    const uint4 q = *reinterpret_cast<const uint4 *>(p);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = (T)(w[i] & 0xffffu);
      v[2 * i + 1] = (T)(w[i] >> 16);
    }
  } else {
    const float4 q0 = *reinterpret_cast<const float4 *>(p), q1 = *reinterpret_cast<const float4 *>(p + 4);
    v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w;
    v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
  }
}

template <typename T>
__global__ __launch_bounds__(WG_THREADS) void wgrad_kernel(pp_wgrad_args a, int split, int rows_per_split) {
  constexpr int P = WgLds<T>::P;
  __shared__ __attribute__((aligned(16))) T sY[WG_T * P];
  __shared__ __attribute__((aligned(16))) T sA[WG_T * P];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int k0 = blockIdx.x * WG_T, n0 = blockIdx.y * WG_T;
  const int b = blockIdx.z / split, s = blockIdx.z % split;
  const int m_begin = s * rows_per_split;
  const int m_end = min(a.M, m_begin + rows_per_split);
  const T *dY = reinterpret_cast<const T *>(a.dY) + (long long)b * a.strideDY;
  const T *A = reinterpret_cast<const T *>(a.A) + (long long)b * a.strideA;
  const int *rowmap = a.dy_rowmap ? a.dy_rowmap + (long long)b * a.strideRowmap : nullptr;
  const int *rowoff = a.rowoff ? a.rowoff + (long long)b * a.strideRowoff : nullptr;
  const bool do_bias = a.dB != nullptr && blockIdx.x == 0;

  // staging: thread t loads row r = t / 8 of the slab, 8 consecutive columns c8 .. c8 + 7 of both operands
  const int lr = tid >> 3, lc = (tid & 7) * 8;
  const int wn = (wave >> 1) * 32, wk = (wave & 1) * 32;     // this wave's 32 x 32 quarter
  hg_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = hg_f32x4{0.f, 0.f, 0.f, 0.f};
  float bias_acc = 0.f;

  for (int mb = m_begin; mb < m_end; mb += WG_M) {
    const int m = mb + lr;
    T yv[8], av[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) yv[e] = av[e] = zero_of<T>();
    if (m < m_end) {
      // 8 consecutive columns: one 16-byte (bf16) or two 16-byte (fp32) loads when whole, aligned and in one segment
      const long long yrow = (long long)(rowmap ? rowmap[m] : m) * a.ldd + n0 + lc;
      if (n0 + lc + 8 <= a.N && ((yrow | (long long)((uintptr_t)dY & 15) / (long long)sizeof(T)) & 7) == 0) {
        load8(dY + yrow, yv);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (n0 + lc + e < a.N) yv[e] = dY[yrow + e];
      }
      const int kb = k0 + lc;
      long long off0 = -1;
      bool whole = false;
      if (kb < a.Kd) {
        if (rowoff) {
          const int seg = kb / a.seg_len;
          const int r = rowoff[(long long)seg * a.M + m];
          whole = kb + 8 <= a.Kd && (kb - seg * a.seg_len) + 8 <= a.seg_len;
          off0 = r < 0 ? -2 : (long long)r + (kb - seg * a.seg_len);
        } else {
          whole = kb + 8 <= a.Kd;
          off0 = (long long)m * a.lda + kb;
        }
      }
      if (whole && off0 >= 0 && ((off0 | (long long)((uintptr_t)A & 15) / (long long)sizeof(T)) & 7) == 0) {
        load8(A + off0, av);
      } else if (!(whole && off0 == -2)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = kb + e;
          if (k < a.Kd) {
            long long off;
            if (rowoff) {
              const int seg = k / a.seg_len;
              const int r = rowoff[(long long)seg * a.M + m];
              off = r < 0 ? -1 : (long long)r + (k - seg * a.seg_len);
            } else {
              off = (long long)m * a.lda + k;
            }
            if (off >= 0) av[e] = A[off];
          }
        }
      }
    }
    __syncthreads();     // the previous slab's readers are done
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sY[(lc + e) * P + lr] = yv[e];
      sA[(lc + e) * P + lr] = av[e];
    }
    __syncthreads();
    if (do_bias && tid < WG_T) {      // the bias gradient: column sums of dY, in row order
#pragma unroll 8
      for (int r = 0; r < WG_M; ++r) bias_acc += Store<T>::ld(&sY[tid * P + r]);
    }
    const int col = lane & 15, grp = lane >> 4;
    if constexpr (sizeof(T) == 2) {
      hg_bf16x8 fy[2], fa[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fy[i] = *reinterpret_cast<const hg_bf16x8 *>(&sY[(wn + 16 * i + col) * P + 8 * grp]);
        fa[i] = *reinterpret_cast<const hg_bf16x8 *>(&sA[(wk + 16 * i + col) * P + 8 * grp]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fy[i], fa[j], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
      for (int kk = 0; kk < WG_M; kk += 4) {
        float fy[2], fa[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fy[i] = sY[(wn + 16 * i + col) * P + kk + grp];
          fa[i] = sA[(wk + 16 * i + col) * P + kk + grp];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fy[i], fa[j], acc[i][j], 0, 0, 0);
      }
    }
  }
  // D[i][j] of a 16 x 16 block: lane holds rows 4 * (lane / 16) + r (n), column lane % 16 (k)
  float *out;
  long long ld;
  if (split > 1) {
    out = a.parts + ((long long)b * split + s) * a.N * a.Kd;
    ld = a.Kd;
  } else {
    out = a.dW + (long long)b * a.strideDW;
    ld = a.lddw;
  }
  const int col = lane & 15, grp = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + 16 * i + 4 * grp + r, k = k0 + wk + 16 * j + col;
        if (n < a.N && k < a.Kd) out[(long long)n * ld + k] = acc[i][j][r];
      }
  if (do_bias && tid < WG_T && n0 + tid < a.N) {
    if (split > 1)
      a.parts[(long long)a.batch * split * a.N * a.Kd + ((long long)b * split + s) * a.N + n0 + tid] = bias_acc;
    else
      a.dB[(long long)b * a.strideDB + n0 + tid] = bias_acc;
  }
}

// split partials -> dW (and dB), summed in split order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(pp_wgrad_args a, int split) {
  const long long per = (long long)a.N * a.Kd;
  const long long total = (long long)a.batch * per;
  const long long nb = a.dB ? (long long)a.batch * a.N : 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total + nb;
       i += (long long)gridDim.x * blockDim.x) {
    if (i < total) {
      const long long b = i / per, r = i % per, n = r / a.Kd, k = r % a.Kd;
      const float *p = a.parts + b * split * per + r;
      float v = 0.f;
      for (int s = 0; s < split; ++s) v += p[s * per];
      a.dW[b * a.strideDW + n * a.lddw + k] = v;
    } else {
      const long long j = i - total, b = j / a.N, n = j % a.N;
      const float *p = a.parts + (long long)a.batch * split * per + b * split * a.N + n;
      float v = 0.f;
      for (int s = 0; s < split; ++s) v += p[(long long)s * a.N];
      a.dB[b * a.strideDB + n] = v;
    }
  }
}

// Rows per split: the split is a function of the problem shape only.  Enough workgroups to cover the CUs twice over,
// at least 512 rows per split (below that the partials cost more than the parallelism buys).
static int wgrad_split(int M, int N, int Kd, int batch) {
  const long long tiles = (long long)cdiv(N, WG_T) * cdiv(Kd, WG_T) * batch;
  long long split = cdiv(512, tiles);
  const long long max_split = cdiv(M, 512);
  if (split > max_split) split = max_split;
  if (split < 1) split = 1;
  if (split > 64) split = 64;
  return (int)split;
}

static int wgrad_rows_per_split(int M, int split) {
  int r = cdiv(M, split);
  return (r + WG_M - 1) / WG_M * WG_M;
}

}  // namespace pp

using namespace pp;

extern "C" long long pp_wgrad_workspace_floats(int M, int N, int Kd, int batch) {
  if (M <= 0 || N <= 0 || Kd <= 0 || batch <= 0) return 0;
  const int split = wgrad_split(M, N, Kd, batch);
  if (split == 1) return 0;
  return (long long)batch * split * ((long long)N * Kd + N);
}

extern "C" int pp_wgrad_gemm(const pp_wgrad_args *a, void *stream) {
  PP_REQUIRE(a, "pp_wgrad_gemm: null args");
  PP_REQUIRE(a->dtype == PP_F32 || a->dtype == PP_BF16, "pp_wgrad_gemm: dtype must be PP_F32 or PP_BF16, got %d",
             a->dtype);
  PP_REQUIRE(a->M > 0 && a->N > 0 && a->Kd > 0 && a->batch >= 1 && a->batch <= 65535 / 64,
             "pp_wgrad_gemm: bad shape M=%d N=%d K=%d batch=%d", a->M, a->N, a->Kd, a->batch);
  PP_REQUIRE(a->dY && a->A && a->dW, "pp_wgrad_gemm: null operand");
  PP_REQUIRE(a->ldd >= a->N && a->lddw >= a->Kd, "pp_wgrad_gemm: ldd=%lld < N or lddw=%lld < K", a->ldd, a->lddw);
  if (a->rowoff)
    PP_REQUIRE(a->seg_len > 0 && a->Kd % a->seg_len == 0, "pp_wgrad_gemm: K=%d not a multiple of seg_len=%d", a->Kd,
               a->seg_len);
  else
    PP_REQUIRE(a->lda >= a->Kd, "pp_wgrad_gemm: lda=%d < K=%d", a->lda, a->Kd);
  const int split = wgrad_split(a->M, a->N, a->Kd, a->batch);
  if (split > 1) PP_REQUIRE(a->parts, "pp_wgrad_gemm: this shape splits M %d ways: parts (pp_wgrad_workspace_floats) "
                            "is required", split);
  hipStream_t s = (hipStream_t)stream;
  const int rps = wgrad_rows_per_split(a->M, split);
  dim3 grid(cdiv(a->Kd, WG_T), cdiv(a->N, WG_T), a->batch * split);
  PP_REQUIRE(grid.y <= 65535, "pp_wgrad_gemm: N too large");
  if (a->dtype == PP_BF16)
    hipLaunchKernelGGL(wgrad_kernel<bf16_t>, grid, dim3(WG_THREADS), 0, s, *a, split, rps);
  else
    hipLaunchKernelGGL(wgrad_kernel<float>, grid, dim3(WG_THREADS), 0, s, *a, split, rps);
  PP_CHECK_LAUNCH("wgrad_kernel");
  if (split > 1) {
    const long long work = (long long)a->batch * a->N * a->Kd;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)std::min<long long>(cdiv(work, 256), 4096)), dim3(256), 0,
                       s, *a, split);
    PP_CHECK_LAUNCH("wgrad_reduce_kernel");
  }
  return 0;
}

namespace pp {

// ============================================================================================================
// Train-mode BatchNorm over channels-last f32 rows [M, C] (row pitch ld).
// Statistics: thread (channel c, row lane r) accumulates rows r, r + 4, ... of its chunk in float64, shifted by the
// channel's first value (no cancellation of a large mean); the four row lanes and then the chunks are combined in a
// fixed order.
// ============================================================================================================
constexpr int BN_CH = 64, BN_RL = 4;

__host__ __device__ inline int bn_chunks(int M) {
  int p = (M + 2047) / 2048;
  return p < 1 ? 1 : (p > 256 ? 256 : p);
}

__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float *__restrict__ y, long long ld, int M, int C,
                                                               int chunk_rows, double *__restrict__ ws) {
  __shared__ double red[2][BN_RL][BN_CH];
  const int cl = threadIdx.x % BN_CH, rl = threadIdx.x / BN_CH;
  const int c = blockIdx.x * BN_CH + cl, p = blockIdx.y;
  const int P = gridDim.y;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    const double pivot = y[c];
    const int r1 = min(M, (p + 1) * chunk_rows);
    for (int r = p * chunk_rows + rl; r < r1; r += BN_RL) {
      const double d = (double)y[(long long)r * ld + c] - pivot;
      s1 += d;
      s2 += d * d;
    }
  }
  red[0][rl][cl] = s1;
  red[1][rl][cl] = s2;
  __syncthreads();
  if (rl == 0 && c < C) {
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int i = 0; i < BN_RL; ++i) {
      t1 += red[0][i][cl];
      t2 += red[1][i][cl];
    }
    ws[(long long)p * C + c] = t1;
    ws[(long long)(P + p) * C + c] = t2;
  }
}

__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float *__restrict__ y, int M, int C, int P,
                                                             const double *__restrict__ ws, const float *gamma,
                                                             const float *beta, float eps, float momentum,
                                                             float *running_mean, float *running_var, float *mean_out,
                                                             float *rstd_out, float *scale_out, float *shift_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double t1 = 0.0, t2 = 0.0;
  for (int p = 0; p < P; ++p) {
    t1 += ws[(long long)p * C + c];
    t2 += ws[(long long)(P + p) * C + c];
  }
  const double dm = t1 / M;
  const double mean = (double)y[c] + dm;
  double var = t2 / M - dm * dm;
  if (var < 0.0) var = 0.0;
  const float meanf = (float)mean, varf = (float)var;
  const float rstd = 1.f / sqrtf(varf + eps);
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  mean_out[c] = meanf;
  rstd_out[c] = rstd;
  scale_out[c] = g * rstd;
  shift_out[c] = bt - meanf * (g * rstd);
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * meanf;
  if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(var * M / (M - 1));
}

template <typename T>
__global__ __launch_bounds__(256) void bn_apply_relu_kernel(const float *__restrict__ y, long long ldy, int M, int C,
                                                            const float *__restrict__ scale,
                                                            const float *__restrict__ shift, T *__restrict__ out,
                                                            long long ldo, int relu) {
  const long long total = (long long)M * C;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / C;
    const int c = (int)(i % C);
    float z = y[r * ldy + c] * scale[c] + shift[c];
    if (relu && z <= 0.f) z = 0.f;          // torch.relu: a NaN stays a NaN
    Store<T>::st(&out[r * ldo + c], z);
  }
}

// MaxPool (kernel = stride = (kh, kw), no padding, floor mode) of z = y * scale + shift, then ReLU.  The window is
// scanned row by row; a value replaces the running maximum when it is greater or NaN (torch's CPU max_pool2d rule:
// the first maximum, a NaN winning).  argmax = the element index of the winner in y, or -1 where the ReLU blocks the
// gradient (maximum <= 0).
template <typename T>
__global__ __launch_bounds__(256) void bn_pool_relu_kernel(const float *__restrict__ y, int B, int h, int w, int C,
                                                           int kh, int kw, const float *__restrict__ scale,
                                                           const float *__restrict__ shift, T *__restrict__ out,
                                                           int *__restrict__ argmax) {
  const int oh = h / kh, ow = w / kw;
  const long long total = (long long)B * oh * ow * C;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long long o = i / C;
    const int ox = (int)(o % ow), oy = (int)((o / ow) % oh), b = (int)(o / ((long long)ow * oh));
    const float sc = scale[c], sh = shift[c];
    float best = -INFINITY;
    long long bi = (((long long)b * h + oy * kh) * w + ox * kw) * C + c;
    for (int dy = 0; dy < kh; ++dy)
      for (int dx = 0; dx < kw; ++dx) {
        const long long e = (((long long)b * h + oy * kh + dy) * w + ox * kw + dx) * C + c;
        const float z = y[e] * sc + sh;
        if (z > best || isnan(z)) {
          best = z;
          bi = e;
        }
      }
    const bool pass = !(best <= 0.f);
    Store<T>::st(&out[i], pass ? best : 0.f);
    argmax[i] = pass ? (int)bi : -1;
  }
}

// The upstream gradient of the BN output z at (r, c):
//   mode 0: g[r, c];  mode 1 (ReLU after BN): g[r, c] where z > 0 (recomputed as in the forward), else 0;
//   mode 2 (MaxPool + ReLU after BN): dpool[o, c] if (r, c) is the recorded winner of its window o, else 0.
struct BnGrad {
  const float *g;
  long long ldg;
  const float *y;
  long long ldy;
  const float *scale, *shift;
  int mode;
  const int *argmax;
  int h, w, kh, kw, C;
  __device__ __forceinline__ float operator()(long long r, int c) const {
    if (mode == 2) {
      const int x = (int)(r % w), yy = (int)((r / w) % h), b = (int)(r / ((long long)w * h));
      const int oh = h / kh, ow = w / kw, oy = yy / kh, ox = x / kw;
      if (oy >= oh || ox >= ow) return 0.f;
      const long long o = ((long long)b * oh + oy) * ow + ox;
      return argmax[o * C + c] == (int)(r * C + c) ? g[o * ldg + c] : 0.f;
    }
    const float v = g[r * ldg + c];
    if (mode == 1) {
      const float z = y[r * ldy + c] * scale[c] + shift[c];
      return z <= 0.f ? 0.f : v;
    }
    return v;
  }
};

__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(BnGrad G, int M, int C, int chunk_rows,
                                                             const float *__restrict__ mean,
                                                             const float *__restrict__ rstd, double *__restrict__ ws) {
  __shared__ double red[2][BN_RL][BN_CH];
  const int cl = threadIdx.x % BN_CH, rl = threadIdx.x / BN_CH;
  const int c = blockIdx.x * BN_CH + cl, p = blockIdx.y;
  const int P = gridDim.y;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    const float mu = mean[c], rs = rstd[c];
    const int r1 = min(M, (p + 1) * chunk_rows);
    for (int r = p * chunk_rows + rl; r < r1; r += BN_RL) {
      const float g = G(r, c);
      const float xhat = (G.y[(long long)r * G.ldy + c] - mu) * rs;
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
    for (int i = 0; i < BN_RL; ++i) {
      t1 += red[0][i][cl];
      t2 += red[1][i][cl];
    }
    ws[(long long)p * C + c] = t1;
    ws[(long long)(P + p) * C + c] = t2;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_final_kernel(int M, int C, int P, const double *__restrict__ ws,
                                                           float *dgamma, float *dbeta, float *coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double t1 = 0.0, t2 = 0.0;
  for (int p = 0; p < P; ++p) {
    t1 += ws[(long long)p * C + c];
    t2 += ws[(long long)(P + p) * C + c];
  }
  if (dbeta) dbeta[c] = (float)t1;
  if (dgamma) dgamma[c] = (float)t2;
  coef[c] = (float)(t1 / M);
  coef[C + c] = (float)(t2 / M);
}

// dx = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat))
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(BnGrad G, int M, int C, const float *__restrict__ mean,
                                                        const float *__restrict__ rstd, const float *__restrict__ gamma,
                                                        const float *__restrict__ coef, T *__restrict__ dx,
                                                        long long ldx) {
  const long long total = (long long)M * C;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / C;
    const int c = (int)(i % C);
    const float g = G(r, c);
    const float xhat = (G.y[r * G.ldy + c] - mean[c]) * rstd[c];
    const float gm = gamma ? gamma[c] : 1.f;
    Store<T>::st(&dx[r * ldx + c], gm * rstd[c] * (g - coef[c] - xhat * coef[C + c]));
  }
}

inline int grid_1d(long long n) {
  long long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace pp

extern "C" long long pp_bn_workspace_bytes(int M, int C) {
  if (M <= 0 || C <= 0) return 0;
  return 2LL * bn_chunks(M) * C * (long long)sizeof(double) + 2LL * C * (long long)sizeof(float);
}

extern "C" int pp_bn_train_stats(const float *y, long long ldy, int M, int C, const float *gamma, const float *beta,
                                 float eps, float momentum, float *running_mean, float *running_var, float *mean,
                                 float *rstd, float *scale, float *shift, void *ws, void *stream) {
  PP_REQUIRE(M > 1 && C > 0 && ldy >= C, "pp_bn_train_stats: expected more than 1 value per channel (M=%d), C=%d, "
             "ld=%lld", M, C, ldy);
  PP_REQUIRE(y && mean && rstd && scale && shift && ws, "pp_bn_train_stats: null pointer");
  PP_REQUIRE(momentum >= 0.f && momentum <= 1.f && eps >= 0.f, "pp_bn_train_stats: bad momentum / eps");
  hipStream_t s = (hipStream_t)stream;
  const int P = bn_chunks(M);
  const int chunk = cdiv(M, P);
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(cdiv(C, BN_CH), P), dim3(256), 0, s, y, ldy, M, C, chunk,
                     (double *)ws);
  PP_CHECK_LAUNCH("bn_stats_partial_kernel");
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, y, M, C, P, (const double *)ws,
                     gamma, beta, eps, momentum, running_mean, running_var, mean, rstd, scale, shift);
  PP_CHECK_LAUNCH("bn_stats_final_kernel");
  return 0;
}

extern "C" int pp_bn_apply_relu(const float *y, long long ldy, int M, int C, const float *scale, const float *shift,
                                void *out, long long ldo, int relu, int dtype, void *stream) {
  PP_REQUIRE(M >= 0 && C > 0 && ldy >= C && ldo >= C, "pp_bn_apply_relu: bad shape");
  if (M == 0) return 0;
  PP_REQUIRE(y && scale && shift && out, "pp_bn_apply_relu: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_1d((long long)M * C);
  if (dtype == PP_BF16)
    hipLaunchKernelGGL(bn_apply_relu_kernel<bf16_t>, dim3(g), dim3(256), 0, s, y, ldy, M, C, scale, shift,
                       (bf16_t *)out, ldo, relu);
  else if (dtype == PP_F32)
    hipLaunchKernelGGL(bn_apply_relu_kernel<float>, dim3(g), dim3(256), 0, s, y, ldy, M, C, scale, shift,
                       (float *)out, ldo, relu);
  else
    return fail("pp_bn_apply_relu: bad dtype %d", dtype);
  PP_CHECK_LAUNCH("bn_apply_relu_kernel");
  return 0;
}

extern "C" int pp_bn_pool_relu(const float *y, int B, int h, int w, int C, int kh, int kw, const float *scale,
                               const float *shift, void *out, int *argmax, int dtype, void *stream) {
  PP_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0 && kh > 0 && kw > 0, "pp_bn_pool_relu: bad shape");
  PP_REQUIRE(h / kh > 0 && w / kw > 0, "pp_bn_pool_relu: window %dx%d larger than input %dx%d", kh, kw, h, w);
  PP_REQUIRE((long long)B * h * w * C < (1LL << 31), "pp_bn_pool_relu: input too large for int32 arg-max indices");
  PP_REQUIRE(y && scale && shift && out && argmax, "pp_bn_pool_relu: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_1d((long long)B * (h / kh) * (w / kw) * C);
  if (dtype == PP_BF16)
    hipLaunchKernelGGL(bn_pool_relu_kernel<bf16_t>, dim3(g), dim3(256), 0, s, y, B, h, w, C, kh, kw, scale, shift,
                       (bf16_t *)out, argmax);
  else if (dtype == PP_F32)
    hipLaunchKernelGGL(bn_pool_relu_kernel<float>, dim3(g), dim3(256), 0, s, y, B, h, w, C, kh, kw, scale, shift,
                       (float *)out, argmax);
  else
    return fail("pp_bn_pool_relu: bad dtype %d", dtype);
  PP_CHECK_LAUNCH("bn_pool_relu_kernel");
  return 0;
}

extern "C" int pp_bn_train_backward(const float *g, long long ldg, const float *y, long long ldy, int M, int C,
                                    const float *mean, const float *rstd, const float *scale, const float *shift,
                                    const float *gamma, int mode, const int *argmax, int B, int h, int w, int kh,
                                    int kw, float *dgamma, float *dbeta, void *dx, long long ldx, int dtype, void *ws,
                                    void *stream) {
  PP_REQUIRE(M > 1 && C > 0 && ldy >= C && ldx >= C && ldg >= C, "pp_bn_train_backward: bad shape M=%d C=%d", M, C);
  PP_REQUIRE(g && y && mean && rstd && dx && ws, "pp_bn_train_backward: null pointer");
  PP_REQUIRE(mode >= 0 && mode <= 2, "pp_bn_train_backward: bad mode %d", mode);
  if (mode == 1) PP_REQUIRE(scale && shift, "pp_bn_train_backward: mode 1 needs scale and shift");
  if (mode == 2) {
    PP_REQUIRE(argmax && B > 0 && h > 0 && w > 0 && kh > 0 && kw > 0 && (long long)B * h * w == M && ldy == C,
               "pp_bn_train_backward: mode 2 needs argmax and the pooling geometry (B*h*w == M, ldy == C)");
  }
  PP_REQUIRE(dtype == PP_F32 || dtype == PP_BF16, "pp_bn_train_backward: bad dtype %d", dtype);
  hipStream_t s = (hipStream_t)stream;
  BnGrad G{g, ldg, y, ldy, scale, shift, mode, argmax, h, w, kh, kw, C};
  const int P = bn_chunks(M);
  const int chunk = cdiv(M, P);
  double *wsd = (double *)ws;
  float *coef = (float *)(wsd + 2LL * P * C);
  hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(cdiv(C, BN_CH), P), dim3(256), 0, s, G, M, C, chunk, mean, rstd, wsd);
  PP_CHECK_LAUNCH("bn_bwd_partial_kernel");
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, M, C, P, (const double *)wsd, dgamma,
                     dbeta, coef);
  PP_CHECK_LAUNCH("bn_bwd_final_kernel");
  const int gr = grid_1d((long long)M * C);
  if (dtype == PP_BF16)
    hipLaunchKernelGGL(bn_bwd_dx_kernel<bf16_t>, dim3(gr), dim3(256), 0, s, G, M, C, mean, rstd, gamma, coef,
                       (bf16_t *)dx, ldx);
  else
    hipLaunchKernelGGL(bn_bwd_dx_kernel<float>, dim3(gr), dim3(256), 0, s, G, M, C, mean, rstd, gamma, coef,
                       (float *)dx, ldx);
  PP_CHECK_LAUNCH("bn_bwd_dx_kernel");
  return 0;
}

namespace pp {

// ============================================================================================================
// Aux tail backward: out[br, b, k] = act(sum_c x[b, br*C + c] w[br, k, c] + bias[br, k]), act = sigmoid for branches
// 0-2, ReLU for branch 3.  dl = gout * s (1 - s) (sigmoid, from the saved output) or gout * (out > 0) (ReLU).
//   dW[br, k, c] = sum_b dl[br, b, k] x[b, br*C + c]      dB[br, k] = sum_b dl[br, b, k]
//   dx[b, br*C + c] = sum_k dl[br, b, k] w[br, k, c]
// ============================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void aux_tail_bwd_kernel(const T *__restrict__ x, const T *__restrict__ w,
                                                           const float *__restrict__ out,
                                                           const float *__restrict__ gout, int B, int C, int K,
                                                           float *dW, float *dB, float *dx) {
  const long long nW = dW ? 4LL * K * C : 0, nB = dB ? 4LL * K : 0, nX = dx ? 4LL * B * C : 0;
  auto dl = [&](int br, int b, int k) {
    const long long i = ((long long)br * B + b) * K + k;
    const float o = out[i], g = gout[i];
    return br < 3 ? g * (o * (1.f - o)) : (o > 0.f ? g : 0.f);
  };
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nW + nB + nX;
       i += (long long)gridDim.x * blockDim.x) {
    if (i < nW) {
      const int c = (int)(i % C), k = (int)((i / C) % K), br = (int)(i / ((long long)C * K));
      float acc = 0.f;
      for (int b = 0; b < B; ++b) acc += dl(br, b, k) * Store<T>::ld(&x[(long long)b * 4 * C + br * C + c]);
      dW[i] = acc;
    } else if (i < nW + nB) {
      const long long j = i - nW;
      const int k = (int)(j % K), br = (int)(j / K);
      float acc = 0.f;
      for (int b = 0; b < B; ++b) acc += dl(br, b, k);
      dB[j] = acc;
    } else {
      const long long j = i - nW - nB;
      const int c4 = (int)(j % (4 * C)), b = (int)(j / (4 * C));
      const int br = c4 / C, c = c4 % C;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc += dl(br, b, k) * Store<T>::ld(&w[((long long)br * K + k) * C + c]);
      dx[j] = acc;
    }
  }
}

// ============================================================================================================
// Heatmap tail.  Forward: out = clamp(p * scale, 0, 1) (p = the logits / T, or their Sparsemax; scale = normalize or
// 1).  Backward, one workgroup per (crop, keypoint) map:
//   gp = g * scale where 0 <= p * scale <= 1 (torch.clamp passes the gradient at both bounds), else 0
//   Sparsemax (sparsemax==0.1.9):  gv = s * (gp - sum(gp * s) / sum(s)),  s = (p > 0)
//   gz = gv / T, written channels-last into dz[(b * HW + pixel) * ldz + k]; columns K .. ldz - 1 are zeroed.
// ============================================================================================================
__global__ __launch_bounds__(256) void heat_clamp_kernel(const float *__restrict__ p, float *__restrict__ out,
                                                         long long n, float scale) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float v = p[i] * scale;
    out[i] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void heat_tail_bwd_kernel(const float *__restrict__ p, const float *__restrict__ g,
                                                            int K, int HW, float scale, int sparse, float temperature,
                                                            T *__restrict__ dz, int ldz) {
  __shared__ double red_s[4];
  __shared__ int red_c[4];
  const int row = blockIdx.x, b = row / K, k = row % K;
  const float *pr = p + (long long)row * HW;
  const float *gr = g + (long long)row * HW;
  auto gp_at = [&](int i) {
    const float v = pr[i] * scale;
    return (v >= 0.f && v <= 1.f) ? gr[i] * scale : 0.f;
  };
  double mean = 0.0;
  if (sparse) {
    double s = 0.0;
    int cnt = 0;
    for (int i = threadIdx.x; i < HW; i += 256)
      if (pr[i] > 0.f) {
        s += gp_at(i);
        ++cnt;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s += __shfl_xor(s, o, 64);
      cnt += __shfl_xor(cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      red_s[threadIdx.x >> 6] = s;
      red_c[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    double ts = 0.0;
    int tc = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ts += red_s[i];
      tc += red_c[i];
    }
    mean = tc > 0 ? ts / tc : 0.0;
  }
  const float meanf = (float)mean;
  for (int i = threadIdx.x; i < HW; i += 256) {
    float gv = gp_at(i);
    if (sparse) gv = pr[i] > 0.f ? gv - meanf : 0.f;
    T *d = dz + ((long long)b * HW + i) * ldz;
    Store<T>::st(&d[k], gv / temperature);
    if (k == K - 1)
      for (int j = K; j < ldz; ++j) d[j] = zero_of<T>();
  }
}

}  // namespace pp

extern "C" int pp_aux_tail_backward(const void *x, const void *w, const float *out, const float *gout, int B, int C,
                                    int K, float *dW, float *dB, float *dx, int dtype, void *stream) {
  PP_REQUIRE(B > 0 && C > 0 && K > 0, "pp_aux_tail_backward: bad shape");
  PP_REQUIRE(x && w && out && gout, "pp_aux_tail_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const long long n = (dW ? 4LL * K * C : 0) + (dB ? 4LL * K : 0) + (dx ? 4LL * B * C : 0);
  if (n == 0) return 0;
  if (dtype == PP_BF16)
    hipLaunchKernelGGL(aux_tail_bwd_kernel<bf16_t>, dim3(grid_1d(n)), dim3(256), 0, s, (const bf16_t *)x,
                       (const bf16_t *)w, out, gout, B, C, K, dW, dB, dx);
  else if (dtype == PP_F32)
    hipLaunchKernelGGL(aux_tail_bwd_kernel<float>, dim3(grid_1d(n)), dim3(256), 0, s, (const float *)x,
                       (const float *)w, out, gout, B, C, K, dW, dB, dx);
  else
    return fail("pp_aux_tail_backward: bad dtype %d", dtype);
  PP_CHECK_LAUNCH("aux_tail_bwd_kernel");
  return 0;
}

extern "C" int pp_heat_clamp(const float *p, float *out, long long n, float scale, void *stream) {
  PP_REQUIRE(n >= 0, "pp_heat_clamp: bad size");
  if (n == 0) return 0;
  PP_REQUIRE(p && out, "pp_heat_clamp: null pointer");
  hipLaunchKernelGGL(heat_clamp_kernel, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, p, out, n, scale);
  PP_CHECK_LAUNCH("heat_clamp_kernel");
  return 0;
}

extern "C" int pp_heat_tail_backward(const float *p, const float *g, int B, int K, int HW, float scale, int sparse,
                                     float temperature, void *dz, int ldz, int dtype, void *stream) {
  PP_REQUIRE(B > 0 && K > 0 && HW > 0 && ldz >= K && temperature != 0.f, "pp_heat_tail_backward: bad shape");
  PP_REQUIRE(p && g && dz, "pp_heat_tail_backward: null pointer");
  PP_REQUIRE((long long)B * K <= 0x7fffffffLL, "pp_heat_tail_backward: too many maps");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == PP_BF16)
    hipLaunchKernelGGL(heat_tail_bwd_kernel<bf16_t>, dim3(B * K), dim3(256), 0, s, p, g, K, HW, scale, sparse,
                       temperature, (bf16_t *)dz, ldz);
  else if (dtype == PP_F32)
    hipLaunchKernelGGL(heat_tail_bwd_kernel<float>, dim3(B * K), dim3(256), 0, s, p, g, K, HW, scale, sparse,
                       temperature, (float *)dz, ldz);
  else
    return fail("pp_heat_tail_backward: bad dtype %d", dtype);
  PP_CHECK_LAUNCH("heat_tail_bwd_kernel");
  return 0;
}
