// Stochastic depth (timm DropPath, scale_by_keep) around the ViT blocks' branches in training: a branch runs on the
// kept crops' rows only.  Three memory-bound kernels move whole crops (N rows of C, contiguous) between the full
// residual stream [B*N, C] and a compact buffer [B'*N, C]:
//   crop_rows_gather       compact <- scale * full[idx]       (the branch's input; the branch's output gradient)
//   droppath_add           out = r + scale * branch[slot]     (the new residual buffer; dropped crops copy r)
//   crop_rows_scatter_add  full[idx] += compact               (the branch's input gradient into dR, dR_c refreshed)
// One workgroup column per crop (blockIdx.y), a grid-stride loop over the crop's N*C elements, four per thread as one
// 128-bit access where C % 4 == 0 and the buffers are 16-byte aligned.  Every output element has one writer (idx holds
// each crop at most once), no atomics: repeated calls give the same bits.  A table entry outside [0, B) (idx) or
// [0, B') (slot, other than "dropped") is skipped / taken as dropped, never followed.
#include "pp_common.h"

namespace pp {

constexpr int DP_THREADS = 256;

inline dim3 dp_grid(long long per_crop, int crops) {
  long long g = (per_crop + DP_THREADS - 1) / DP_THREADS;
  return dim3((unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g)), (unsigned)crops);
}

template <typename T>
__device__ __forceinline__ void dp_store4(T *p, float a, float b, float c, float d) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<float4 *>(p) = make_float4(a, b, c, d);
  } else {
    *reinterpret_cast<uint2 *>(p) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(DP_THREADS) void crop_rows_gather_kernel(const float *__restrict__ src,
                                                                      const int *__restrict__ idx, int B, long long L,
                                                                      float scale, T *__restrict__ dst) {
  const int j = blockIdx.y;
  const int b = idx[j];
  if (b < 0 || b >= B) return;
  const float *s = src + (long long)b * L;
  T *d = dst + (long long)j * L;
  const long long stride = (long long)gridDim.x * DP_THREADS;
  const long long t0 = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if constexpr (VEC) {
    for (long long i = t0; i < L / 4; i += stride) {
      const float4 v = reinterpret_cast<const float4 *>(s)[i];
      dp_store4<T>(d + 4 * i, scale * v.x, scale * v.y, scale * v.z, scale * v.w);
    }
  } else {
    for (long long i = t0; i < L; i += stride) Store<T>::st(d + i, scale * s[i]);
  }
}

// fma form: out = fmaf(scale, branch, r), one rounding
template <bool VEC>
__global__ __launch_bounds__(DP_THREADS) void droppath_add_kernel(const float *__restrict__ r,
                                                                  const float *__restrict__ branch,
                                                                  const int *__restrict__ slot, int Bk, long long L,
                                                                  float scale, float *__restrict__ out) {
  const int b = blockIdx.y;
  const int j = slot[b];
  const bool kept = j >= 0 && j < Bk;
  const float *x = r + (long long)b * L;
  const float *y = branch + (long long)(kept ? j : 0) * L;
  float *o = out + (long long)b * L;
  const long long stride = (long long)gridDim.x * DP_THREADS;
  const long long t0 = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if constexpr (VEC) {
    for (long long i = t0; i < L / 4; i += stride) {
      float4 v = reinterpret_cast<const float4 *>(x)[i];
      if (kept) {
        const float4 w = reinterpret_cast<const float4 *>(y)[i];
        v.x = fmaf(scale, w.x, v.x); v.y = fmaf(scale, w.y, v.y);
        v.z = fmaf(scale, w.z, v.z); v.w = fmaf(scale, w.w, v.w);
      }
      reinterpret_cast<float4 *>(o)[i] = v;
    }
  } else {
    for (long long i = t0; i < L; i += stride) o[i] = kept ? fmaf(scale, y[i], x[i]) : x[i];
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(DP_THREADS) void crop_rows_scatter_add_kernel(const float *__restrict__ dx,
                                                                           const int *__restrict__ idx, int B,
                                                                           long long L, float *__restrict__ dres,
                                                                           T *__restrict__ dres_c) {
  const int j = blockIdx.y;
  const int b = idx[j];
  if (b < 0 || b >= B) return;
  const float *s = dx + (long long)j * L;
  float *d = dres + (long long)b * L;
  T *c = dres_c + (long long)b * L;
  const long long stride = (long long)gridDim.x * DP_THREADS;
  const long long t0 = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if constexpr (VEC) {
    for (long long i = t0; i < L / 4; i += stride) {
      const float4 a = reinterpret_cast<const float4 *>(s)[i];
      float4 v = reinterpret_cast<float4 *>(d)[i];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
      reinterpret_cast<float4 *>(d)[i] = v;
      dp_store4<T>(c + 4 * i, v.x, v.y, v.z, v.w);
    }
  } else {
    for (long long i = t0; i < L; i += stride) {
      const float v = d[i] + s[i];
      d[i] = v;
      Store<T>::st(c + i, v);
    }
  }
}

static bool dp_aligned16(const void *a, const void *b, const void *c) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace pp

using namespace pp;

#define DP_REQUIRE_SHAPE(name)                                                                                      \
  PP_REQUIRE(B > 0 && B <= 65535 && Bk > 0 && Bk <= B && N > 0 && C > 0,                                            \
             name ": bad shape B=%d kept=%d N=%d C=%d (0 < kept <= B <= 65535)", B, Bk, N, C)

extern "C" int pp_crop_rows_gather(const float *src, const int *idx, int B, int Bk, int N, int C, float scale,
                                   void *dst, int dtype, void *stream) {
  DP_REQUIRE_SHAPE("pp_crop_rows_gather");
  PP_REQUIRE(src && idx && dst, "pp_crop_rows_gather: null pointer");
  PP_REQUIRE(dtype == PP_F32 || dtype == PP_BF16, "pp_crop_rows_gather: bad dtype %d", dtype);
  PP_REQUIRE((const void *)src != (const void *)dst, "pp_crop_rows_gather: dst must not alias src");
  hipStream_t s = (hipStream_t)stream;
  const long long L = (long long)N * C;
  const bool vec = C % 4 == 0 && dp_aligned16(src, dst, nullptr);
  const dim3 grid = dp_grid(vec ? L / 4 : L, Bk), block(DP_THREADS);
  if (dtype == PP_BF16) {
    if (vec) hipLaunchKernelGGL((crop_rows_gather_kernel<bf16_t, true>), grid, block, 0, s, src, idx, B, L, scale, (bf16_t *)dst);
    else hipLaunchKernelGGL((crop_rows_gather_kernel<bf16_t, false>), grid, block, 0, s, src, idx, B, L, scale, (bf16_t *)dst);
  } else {
    if (vec) hipLaunchKernelGGL((crop_rows_gather_kernel<float, true>), grid, block, 0, s, src, idx, B, L, scale, (float *)dst);
    else hipLaunchKernelGGL((crop_rows_gather_kernel<float, false>), grid, block, 0, s, src, idx, B, L, scale, (float *)dst);
  }
  PP_CHECK_LAUNCH("crop_rows_gather_kernel");
  return 0;
}

extern "C" int pp_droppath_add(const float *r, const float *branch, const int *slot, int B, int Bk, int N, int C,
                               float scale, float *out, void *stream) {
  DP_REQUIRE_SHAPE("pp_droppath_add");
  PP_REQUIRE(r && branch && slot && out, "pp_droppath_add: null pointer");
  PP_REQUIRE(out != r && out != branch, "pp_droppath_add: out must not alias r or branch");
  const long long L = (long long)N * C;
  const bool vec = C % 4 == 0 && dp_aligned16(r, branch, out);
  const dim3 grid = dp_grid(vec ? L / 4 : L, B), block(DP_THREADS);
  if (vec) hipLaunchKernelGGL(droppath_add_kernel<true>, grid, block, 0, (hipStream_t)stream, r, branch, slot, Bk, L, scale, out);
  else hipLaunchKernelGGL(droppath_add_kernel<false>, grid, block, 0, (hipStream_t)stream, r, branch, slot, Bk, L, scale, out);
  PP_CHECK_LAUNCH("droppath_add_kernel");
  return 0;
}

extern "C" int pp_crop_rows_scatter_add(const float *dx, const int *idx, int B, int Bk, int N, int C, float *dres,
                                        void *dres_c, int dtype, void *stream) {
  DP_REQUIRE_SHAPE("pp_crop_rows_scatter_add");
  PP_REQUIRE(dx && idx && dres && dres_c, "pp_crop_rows_scatter_add: null pointer");
  PP_REQUIRE(dtype == PP_F32 || dtype == PP_BF16, "pp_crop_rows_scatter_add: bad dtype %d", dtype);
  PP_REQUIRE(dx != dres && (const void *)dres != (const void *)dres_c && (const void *)dx != (const void *)dres_c,
             "pp_crop_rows_scatter_add: dx, dres and dres_c must be three buffers");
  hipStream_t s = (hipStream_t)stream;
  const long long L = (long long)N * C;
  const bool vec = C % 4 == 0 && dp_aligned16(dx, dres, dres_c);
  const dim3 grid = dp_grid(vec ? L / 4 : L, Bk), block(DP_THREADS);
  if (dtype == PP_BF16) {
    if (vec) hipLaunchKernelGGL((crop_rows_scatter_add_kernel<bf16_t, true>), grid, block, 0, s, dx, idx, B, L, dres, (bf16_t *)dres_c);
    else hipLaunchKernelGGL((crop_rows_scatter_add_kernel<bf16_t, false>), grid, block, 0, s, dx, idx, B, L, dres, (bf16_t *)dres_c);
  } else {
    if (vec) hipLaunchKernelGGL((crop_rows_scatter_add_kernel<float, true>), grid, block, 0, s, dx, idx, B, L, dres, (float *)dres_c);
    else hipLaunchKernelGGL((crop_rows_scatter_add_kernel<float, false>), grid, block, 0, s, dx, idx, B, L, dres, (float *)dres_c);
  }
  PP_CHECK_LAUNCH("crop_rows_scatter_add_kernel");
  return 0;
}
