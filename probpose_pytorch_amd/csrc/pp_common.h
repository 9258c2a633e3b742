// Shared helpers for the gfx950 kernels of libprobpose_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/probpose_hip.h"

namespace pp {

// thread-local error string behind pp_last_error()
char *err_buf();
int fail(const char *fmt, ...);

#define PP_CHECK_HIP(expr)                                                            \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) return pp::fail("%s: %s", #expr, hipGetErrorString(_e));    \
  } while (0)

#define PP_CHECK_LAUNCH(name)                                                         \
  do {                                                                                \
    hipError_t _e = hipGetLastError();                                                \
    if (_e != hipSuccess) return pp::fail("launch %s: %s", name, hipGetErrorString(_e)); \
  } while (0)

#define PP_REQUIRE(cond, ...)                                                         \
  do {                                                                                \
    if (!(cond)) return pp::fail(__VA_ARGS__);                                        \
  } while (0)

// ---- storage types -------------------------------------------------------
typedef unsigned short bf16_t;  // raw bf16 bits

__device__ __forceinline__ float bf16_to_f32(bf16_t v) {
  return __uint_as_float(((unsigned)v) << 16);
}
// round-to-nearest-even; plain cast keeps NaN a NaN (v_cvt_pk_bf16_f32 on gfx950)
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<bf16_t *>(&h);
}

// two floats -> one packed bf16 pair by ONE v_cvt_pk_bf16_f32 (the same rounding as f32_to_bf16, which the compiler
// lowers to that instruction with one live input, a shift and an or around it)
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// OCP e4m3 (gfx950): 4 floats -> 4 bytes, round-to-nearest-even, saturating at +-448 (NaN stays NaN).  The fp8 mode's
// producers: the GEMM epilogue, LayerNorm (value * static per-tensor scale) and attention (its output feeds the fp8 proj
// GEMM).
__device__ __forceinline__ unsigned pack_fp8x4(float a, float b, float c, float d) {
  a = __builtin_amdgcn_fmed3f(a, -448.0f, 448.0f);
  b = __builtin_amdgcn_fmed3f(b, -448.0f, 448.0f);
  c = __builtin_amdgcn_fmed3f(c, -448.0f, 448.0f);
  d = __builtin_amdgcn_fmed3f(d, -448.0f, 448.0f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (unsigned)w;
}

// LDS-DMA of 16 B per lane: LDS destination = wave-uniform byte offset (M0) + lane * 16.  Issued
// from inline asm on purpose: hipcc cannot tell that the DMA into buffer t+1 never aliases the
// ds_reads of buffer t and would drain vmcnt(0) in front of every fragment read, serialising the
// prefetch behind the MFMAs.  The asm DMA is invisible to its wait-count bookkeeping; completion is
// enforced by the caller's explicit s_waitcnt vmcnt + barrier.
__device__ __forceinline__ void glds16(const void *gsrc, unsigned lds_off_uniform) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_off_uniform)
      : "memory");
}

template <typename T> struct Store;
template <> struct Store<float> {
  static __device__ __forceinline__ float ld(const float *p) { return *p; }
  static __device__ __forceinline__ void st(float *p, float v) { *p = v; }
};
template <> struct Store<bf16_t> {
  static __device__ __forceinline__ float ld(const bf16_t *p) { return bf16_to_f32(*p); }
  static __device__ __forceinline__ void st(bf16_t *p, float v) { *p = f32_to_bf16(v); }
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// every lane gets the wave's smallest v and the smallest i among the lanes that hold it: one butterfly over the pair
__device__ __forceinline__ void wave_argmin_i64(long long &v, int &i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov < v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

// ---- np.argmax order -------------------------------------------------------
// The running result of a flat arg-max with numpy's semantics: the first maximum in row-major order wins; a NaN is the
// maximum, and the first NaN wins.
struct ArgmaxBest {
  float v;
  int i;
  // "nothing seen yet": every real (v, i) -- NaN included -- is ahead of it, so it never wins a reduction
  static __device__ __forceinline__ ArgmaxBest none() { return ArgmaxBest{-__builtin_inff(), 0x7fffffff}; }
};

// is (av, ai) strictly ahead of (bv, bi) in np.argmax's order?
__device__ __forceinline__ bool argmax_ahead(float av, int ai, float bv, int bi) {
  bool an = av != av, bn = bv != bv;
  if (an || bn) {
    if (an && bn) return ai < bi;
    return an;
  }
  return av > bv || (av == bv && ai < bi);
}

__device__ __forceinline__ void argmax_take(ArgmaxBest &b, float v, int i) {
  if (argmax_ahead(v, i, b.v, b.i)) {
    b.v = v;
    b.i = i;
  }
}

// every thread of the workgroup (whole waves) returns the workgroup's best
__device__ __forceinline__ ArgmaxBest block_argmax(ArgmaxBest mine, ArgmaxBest *red /* [waves] in LDS */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float ov = __shfl_down(mine.v, o, 64);
    int oi = __shfl_down(mine.i, o, 64);
    if (argmax_ahead(ov, oi, mine.v, mine.i)) {
      mine.v = ov;
      mine.i = oi;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) red[wave] = mine;
  __syncthreads();
  ArgmaxBest r = red[0];
  for (int w = 1; w < nw; ++w)
    if (argmax_ahead(red[w].v, red[w].i, r.v, r.i)) r = red[w];
  return r;
}

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Raise a kernel's dynamic-LDS limit to `bytes` on the calling thread's current device, once per (kernel, device): the
// attribute is per device, and a device is marked only after hipFuncSetAttribute has succeeded there.
template <typename K>
inline int ensure_dynamic_lds(K *kernel, size_t bytes) {
  struct Raised { const void *kernel; int dev; size_t bytes; };
  static thread_local std::vector<Raised> raised;
  int dev = 0;
  PP_CHECK_HIP(hipGetDevice(&dev));
  Raised *r = nullptr;
  for (Raised &e : raised)
    if (e.kernel == (const void *)kernel && e.dev == dev) r = &e;
  if (r && r->bytes >= bytes) return 0;
  PP_CHECK_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (r) r->bytes = bytes;
  else raised.push_back({(const void *)kernel, dev, bytes});
  return 0;
}

// Compute units of the calling thread's current device, cached per device ordinal.
inline int cu_count(int *out) {
  static thread_local int cached[64] = {};
  int dev = 0;
  PP_CHECK_HIP(hipGetDevice(&dev));
  int &n = cached[dev & 63];
  if (n == 0) {
    PP_CHECK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    if (n <= 0) n = 256;
  }
  *out = n;
  return 0;
}

}  // namespace pp
