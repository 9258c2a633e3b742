// The ValidationMeter's int64 state as device and host C++ see it: the one statement of its layout, of the fine bin a
// sample is counted in and of the K / J limits, for the meter (pp_valmeter.hip) and for the calibration that reads the
// state (pp_calib.hip), with the 256-thread tree sum.  include/probpose_hip.h documents the sections; valmeter.py's
// state_layout and tests/valmeter_reference.py restate them and are held to this by the tests.
//
// Not here, on purpose: the reliability-row writer and the max-of-256 finish of an MCE.  As shared helpers they changed
// the instruction streams of the report and score kernels, and the report measured slower
// (profiles/valmeter_state_refactor.txt).
#pragma once
#include "pp_common.h"

namespace pp {

constexpr int VM_BINS = 1024;
constexpr int VM_MAX_J = 64;
constexpr int VM_OKS_SUMS = 5, VM_ERR_SUMS = 4, VM_ALL = 3, VM_REJECTED = 5, VM_SCALARS = 15;
constexpr double VM_Q30 = 1073741824.0, VM_Q20 = 1048576.0;

typedef unsigned long long u64;

// word offsets of the sections of the state
struct VmLayout {
  long long hist, conf, above, sum_p, sum_p2, oks_hist, oks_sx, oks_st, oks_sums, err, pck, all, rejected, scalars,
      words;
};

__host__ __device__ inline VmLayout vm_layout(int K, int J) {
  VmLayout L;
  const long long k = K;
  long long o = 0;
  L.hist = o, o += 2 * k * 2 * VM_BINS;
  L.conf = o, o += 2 * k * VM_BINS;
  L.above = o, o += 2 * k * 2 * J;
  L.sum_p = o, o += 2 * k * 2;
  L.sum_p2 = o, o += 2 * k * 2;
  L.oks_hist = o, o += k * VM_BINS;
  L.oks_sx = o, o += k * VM_BINS;
  L.oks_st = o, o += k * VM_BINS;
  L.oks_sums = o, o += k * VM_OKS_SUMS;
  L.err = o, o += k * VM_ERR_SUMS;
  L.pck = o, o += 2 * k;
  L.all = o, o += VM_ALL;
  L.rejected = o, o += VM_REJECTED;
  L.scalars = o, o += VM_SCALARS;
  L.words = o;
  return L;
}

inline int vm_check_shape(const char *who, int K, int J) {
  PP_REQUIRE(K > 0 && K <= 65535, "%s: bad K=%d (1 .. 65535 keypoints)", who, K);
  PP_REQUIRE(J >= 1 && J <= VM_MAX_J, "%s: bad J=%d (1 .. %d thresholds)", who, J, VM_MAX_J);
  return 0;
}

__device__ __forceinline__ bool vm_unit_ok(float p) { return p >= 0.0f && p <= 1.0f; }         // NaN: false
__device__ __forceinline__ int vm_fine_bin(float p) { return min(VM_BINS - 1, (int)floorf(p * 1024.0f)); }
__device__ __forceinline__ double vm_nan() { return __builtin_nan(""); }

// the keypoints k0 .. k1-1 of a report row: row < K is that keypoint, row K the pool of all
struct VmRows {
  int k0, k1;
};
__device__ __forceinline__ VmRows vm_row_range(int row, int K) {
  return VmRows{row < K ? row : 0, row < K ? row + 1 : K};
}

// (weight n, numerator P) of fine bin b of keypoint k for head h; h = 2: the OKS head, P the Q30 sum of the achieved OKS
__device__ __forceinline__ void vm_bin(const long long *__restrict__ state, const VmLayout &L, int K, int h, int k,
                                       int b, long long &n, long long &p) {
  if (h < 2) {
    const long long at = L.hist + (((long long)h * K + k) * 2) * VM_BINS + b;
    const long long neg = state[at], pos = state[at + VM_BINS];
    n = neg + pos, p = pos;
  } else {
    n = state[L.oks_hist + (long long)k * VM_BINS + b];
    p = state[L.oks_st + (long long)k * VM_BINS + b];
  }
}

// the sum of v over the 256 threads, to every thread, as a tree in red[256]; begins and ends with a barrier
template <typename T>
__device__ __forceinline__ T vm_block_sum(T v, T *red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

}  // namespace pp
