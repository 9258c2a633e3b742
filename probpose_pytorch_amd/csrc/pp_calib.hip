// HeadCalibration: isotonic recalibration of the probability, visibility and OKS heads from a ValidationMeter state.
//
// pp_calib_fit takes, per head h and row r (a keypoint, or r = K: the integer state summed over the keypoints), the
// weighted isotonic least-squares regression over the meter's 1024 fine bins by pool-adjacent-violators, exactly:
// blocks are (P, N) integer pairs and two neighbours pool while P_l N_r >= P_r N_l, compared as 128-bit products.  With
// ">=" the final blocks are the maximal runs of equal fitted value, so the result does not depend on the pooling order
// and tests/calibration_reference.py (a stack PAV in Python integers) must reproduce it bit for bit.  pp_calib_apply
// maps decoded head values through the fitted table; pp_calib_score says what the table makes of the samples of any
// meter state.  The definitions are in include/probpose_hip.h, the reasoning in DESIGN §4.5j.
#include "pp_valmeter_state.h"

namespace pp {

constexpr int CB_HEADS = 3;
constexpr int CB_BINARY_FIXED = 6, CB_OKS_FIXED = 3;

// value(l) >= value(r), exactly: P_l N_r >= P_r N_l as 128-bit products (P < 2^61, N < 2^31)
__device__ __forceinline__ bool cb_ge(u64 pl, u64 nl, u64 pr, u64 nr) {
  const u64 ah = __umul64hi(pl, nr), al = pl * nr, bh = __umul64hi(pr, nl), bl = pr * nl;
  return ah > bh || (ah == bh && al >= bl);
}

// Do the neighbours l, r pool?  An empty right block always joins its left neighbour (an empty bin carries the block to
// its left); an empty left block -- only the first block of a list can be one -- waits: the leading empty bins take the
// first block at the very end.
__device__ __forceinline__ bool cb_pool(long long pl, long long nl, long long pr, long long nr) {
  if (nr == 0) return true;
  if (nl == 0) return false;
  return cb_ge((u64)pl, (u64)nl, (u64)pr, (u64)nr);
}

__device__ __forceinline__ float cb_value(int h, long long P, long long N) {
  if (N <= 0) return 0.0f;
  const double q = (double)P / (double)N;
  return h < 2 ? (float)q : (float)(q * (1.0 / VM_Q30));
}

// grid (K + 1, 3): workgroup (r, h) fits row r of head h.  256 threads.
//
// The blocks of a list live in place: a block that covers the bins [s, e) keeps P[s], N[s], nxt[s] = e and
// beg[e - 1] = s; head[s] says that s still starts a block.  Every bin starts as its own block; level j of a merge tree
// joins the lists of the segments [2m 2^j, (2m+1) 2^j) and [(2m+1) 2^j, (2m+2) 2^j), one thread per pair: both lists are
// strictly increasing, so only the junction can violate, and the junction block grows to the left and to the right
// until both of its neighbours are strictly on their side.  A merge touches its own segment only.
__global__ __launch_bounds__(256) void calib_fit_kernel(const long long *__restrict__ state, int K, int J,
                                                        long long min_count, long long *__restrict__ blocks,
                                                        float *__restrict__ table, int *__restrict__ row_of) {
  __shared__ long long P[VM_BINS], N[VM_BINS];
  __shared__ short nxt[VM_BINS], beg[VM_BINS];
  __shared__ unsigned char head[VM_BINS];
  __shared__ long long red[256];
  __shared__ int scan[256];
  const VmLayout L = vm_layout(K, J);
  const int tid = threadIdx.x, row = blockIdx.x, h = blockIdx.y;
  const auto [k0, k1] = vm_row_range(row, K);

  long long mine = 0;
  for (int b = tid; b < VM_BINS; b += 256) {
    long long n = 0, p = 0;
    for (int k = k0; k < k1; ++k) {
      long long nk, pk;
      vm_bin(state, L, K, h, k, b, nk, pk);
      n += nk, p += pk;
    }
    P[b] = p, N[b] = n;
    nxt[b] = (short)(b + 1), beg[b] = (short)b, head[b] = 1;
    mine += n;
  }
  const long long total = vm_block_sum(mine, red, tid);     // ends with a barrier: the lists are in place

  for (int half = 1; half < VM_BINS; half <<= 1) {
    const int merges = VM_BINS / (2 * half);
    for (int m = tid; m < merges; m += 256) {
      const int lo = m * 2 * half, mid = lo + half, hi = mid + half;
      int cs = beg[mid - 1], ce = nxt[mid];
      long long cp = P[cs], cn = N[cs];
      if (cb_pool(cp, cn, P[mid], N[mid])) {
        cp += P[mid], cn += N[mid], head[mid] = 0;
        bool grew;
        do {
          grew = false;
          if (cs > lo) {
            const int s = beg[cs - 1];
            if (cb_pool(P[s], N[s], cp, cn)) cp += P[s], cn += N[s], head[cs] = 0, cs = s, grew = true;
          }
          if (ce < hi && cb_pool(cp, cn, P[ce], N[ce])) cp += P[ce], cn += N[ce], head[ce] = 0, ce = nxt[ce], grew = true;
        } while (grew);
        P[cs] = cp, N[cs] = cn, nxt[cs] = (short)ce, beg[ce - 1] = (short)cs;
      }
    }
    __syncthreads();
  }
  // the leading empty bins carry the first block
  if (tid == 0 && N[0] == 0 && nxt[0] < VM_BINS) {
    const int e = nxt[0];
    P[0] = P[e], N[0] = N[e], head[e] = 0;
  }
  __syncthreads();

  // the block that covers a bin starts at the last head at or before it: thread t owns the bins 4t .. 4t+3
  int last = -1;
  for (int i = 0; i < 4; ++i)
    if (head[4 * tid + i]) last = 4 * tid + i;
  scan[tid] = last;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = tid >= off ? scan[tid - off] : -1;
    __syncthreads();
    scan[tid] = max(scan[tid], v);
    __syncthreads();
  }
  int cur = tid > 0 ? scan[tid - 1] : 0;      // bin 0 always starts a block
  const long long out = ((long long)h * (K + 1) + row) * VM_BINS;
  for (int i = 0; i < 4; ++i) {
    const int b = 4 * tid + i;
    if (head[b]) cur = b;
    const long long p = P[cur], n = N[cur];
    blocks[(out + b) * 2] = p;
    blocks[(out + b) * 2 + 1] = n;
    table[out + b] = cb_value(h, p, n);
  }

  // row_of, by the pool's workgroup (it knows whether the pool holds a sample): wave w counts the rows w, w + 4, ...
  if (row != K) return;
  const int lane = tid & 63;
  for (int k = tid >> 6; k < K; k += 4) {
    long long n = 0;
    for (int b = lane; b < VM_BINS; b += 64) {
      long long nk, pk;
      vm_bin(state, L, K, h, k, b, nk, pk);
      n += nk;
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if (lane == 0) row_of[(long long)h * K + k] = n >= min_count ? k : (total >= 1 ? K : -1);
  }
}

// grid (ceil(B K / 256), 3): one value each.  Reads its element before it writes it, so in place is safe.
__global__ __launch_bounds__(256) void calib_apply_kernel(const float *__restrict__ in, float *__restrict__ out, int BK,
                                                          int K, const float *__restrict__ table,
                                                          const int *__restrict__ row_of) {
  const int i = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
  if (i >= BK) return;
  const long long at = (long long)h * BK + i;
  float p = in[at];
  const int r = row_of[h * K + i % K];
  if (vm_unit_ok(p) && r >= 0 && r <= K)
    p = table[((long long)h * (K + 1) + r) * VM_BINS + vm_fine_bin(p)];
  out[at] = p;
}

// grid (K + 1, 3): workgroup (r, h) scores row r of head h; row K pools the keypoints, each through its own table.
// Thread t takes the fine bins t, t + 256, ... of every keypoint of the row; the samples of a bin are regrouped by the
// float32 value y the apply emits for it into E bins kept in LDS (integer counts, float64 sum of n y).
__global__ __launch_bounds__(256) void calib_score_kernel(const long long *__restrict__ state, int K, int J,
                                                          const float *__restrict__ table,
                                                          const int *__restrict__ row_of, int E, int F,
                                                          double *__restrict__ report) {
  __shared__ u64 cnt[VM_BINS], num[VM_BINS];      // per E bin: samples; positives, or the Q30 sum of the achieved OKS
  __shared__ double conf[VM_BINS];                // per E bin: the sum of n_b y_b
  __shared__ double redf[256];
  __shared__ long long red[256];
  const VmLayout L = vm_layout(K, J);
  const int tid = threadIdx.x, row = blockIdx.x, h = blockIdx.y;
  const auto [k0, k1] = vm_row_range(row, K);
  for (int e = tid; e < E; e += 256) cnt[e] = 0, num[e] = 0, conf[e] = 0.0;
  __syncthreads();

  long long my_n = 0, my_skipped = 0;
  double my_brier = 0.0, my_conf = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int r = row_of[h * K + k];
    const bool use = r >= 0 && r <= K;
    const float *t = table + ((long long)h * (K + 1) + (use ? r : 0)) * VM_BINS;
    for (int b = tid; b < VM_BINS; b += 256) {
      long long n, p;
      vm_bin(state, L, K, h, k, b, n, p);
      if (n == 0) continue;
      if (!use) {
        my_skipped += n;
        continue;
      }
      const float y = t[b];
      const int e = min(E - 1, max(0, (int)(y * (float)E)));
      const double yd = (double)y, c = (double)n * yd;
      my_n += n, my_conf += c;
      atomicAdd(&cnt[e], (u64)n);
      atomicAdd(&num[e], (u64)p);
      atomicAdd(&conf[e], c);
      if (h < 2) {
        const double w = 1.0 - yd;
        my_brier += (double)p * (w * w) + (double)(n - p) * (yd * yd);
      }
    }
  }
  const long long n = vm_block_sum(my_n, red, tid);
  const long long skipped = vm_block_sum(my_skipped, red, tid);
  const double brier = vm_block_sum(my_brier, redf, tid), sconf = vm_block_sum(my_conf, redf, tid);

  const int fixed = h < 2 ? CB_BINARY_FIXED : CB_OKS_FIXED;
  double *o = report + (long long)row * F + (h < 2 ? h * (CB_BINARY_FIXED + 3 * E) : 2 * (CB_BINARY_FIXED + 3 * E));
  double my_abs = 0.0, my_mce = -1.0;
  for (int e = tid; e < E; e += 256) {
    const double c = (double)cnt[e];
    const double target = h < 2 ? (double)num[e] : (double)num[e] / VM_Q30;
    const double d = fabs(conf[e] - target);
    double *t = o + fixed + 3 * e;
    t[0] = c;
    if (cnt[e] > 0) {
      my_abs += d;
      my_mce = fmax(my_mce, d / c);
      t[1] = conf[e] / c;
      t[2] = target / c;
    } else {
      t[1] = t[2] = vm_nan();
    }
  }
  const double abs_sum = vm_block_sum(my_abs, redf, tid);
  __syncthreads();
  redf[tid] = my_mce;
  __syncthreads();
  if (tid != 0) return;
  double mce = -1.0;
  for (int i = 0; i < 256; ++i) mce = fmax(mce, redf[i]);
  o[0] = (double)n;
  o[1] = (double)skipped;
  const bool any = n > 0;
  if (h < 2) {
    o[2] = any ? brier / (double)n : vm_nan();
    o[3] = any ? sconf / (double)n : vm_nan();
    o[4] = any ? abs_sum / (double)n : vm_nan();
    o[5] = any ? mce : vm_nan();
  } else {
    o[2] = any ? abs_sum / (double)n : vm_nan();
  }
}

}  // namespace pp

extern "C" int pp_calib_fit(const long long *state, int K, int J, long long min_count, long long *blocks, float *table,
                            int *row_of, void *stream) {
  using namespace pp;
  if (int rc = vm_check_shape("pp_calib_fit", K, J)) return rc;
  PP_REQUIRE(min_count >= 1, "pp_calib_fit: bad min_count=%lld (at least 1)", min_count);
  PP_REQUIRE(state, "pp_calib_fit: null state");
  PP_REQUIRE(blocks && table && row_of, "pp_calib_fit: null output");
  hipLaunchKernelGGL(calib_fit_kernel, dim3(K + 1, CB_HEADS), dim3(256), 0, (hipStream_t)stream, state, K, J, min_count,
                     blocks, table, row_of);
  PP_CHECK_LAUNCH("calib_fit_kernel");
  return 0;
}

extern "C" int pp_calib_apply(const float *aux_in, float *aux_out, int B, int K, const float *table, const int *row_of,
                              void *stream) {
  using namespace pp;
  PP_REQUIRE(K > 0 && K <= 65535, "pp_calib_apply: bad K=%d (1 .. 65535 keypoints)", K);
  PP_REQUIRE(B > 0 && (long long)B * K * CB_HEADS < (1ll << 31), "pp_calib_apply: bad B=%d (B > 0, 3*B*K < 2^31)", B);
  PP_REQUIRE(aux_in && aux_out, "pp_calib_apply: null aux");
  PP_REQUIRE(table && row_of, "pp_calib_apply: null calibration");
  const long long count = (long long)CB_HEADS * B * K;
  const float *in_end = aux_in + count;
  const float *out_end = aux_out + count;
  PP_REQUIRE(aux_in == aux_out || in_end <= aux_out || out_end <= aux_in,
             "pp_calib_apply: aux_in and aux_out overlap in part (in place means the same address)");
  const int BK = B * K;
  hipLaunchKernelGGL(calib_apply_kernel, dim3(cdiv(BK, 256), CB_HEADS), dim3(256), 0, (hipStream_t)stream, aux_in,
                     aux_out, BK, K, table, row_of);
  PP_CHECK_LAUNCH("calib_apply_kernel");
  return 0;
}

extern "C" int pp_calib_score(const long long *state, int K, int J, const float *table, const int *row_of, int ece_bins,
                              double *report, void *stream) {
  using namespace pp;
  if (int rc = vm_check_shape("pp_calib_score", K, J)) return rc;
  PP_REQUIRE(ece_bins >= 1 && ece_bins <= VM_BINS && VM_BINS % ece_bins == 0,
             "pp_calib_score: ece_bins=%d does not divide %d", ece_bins, VM_BINS);
  PP_REQUIRE(state, "pp_calib_score: null state");
  PP_REQUIRE(table && row_of, "pp_calib_score: null calibration");
  PP_REQUIRE(report, "pp_calib_score: null report");
  const int F = 2 * (CB_BINARY_FIXED + 3 * ece_bins) + CB_OKS_FIXED + 3 * ece_bins;
  hipLaunchKernelGGL(calib_score_kernel, dim3(K + 1, CB_HEADS), dim3(256), 0, (hipStream_t)stream, state, K, J, table,
                     row_of, ece_bins, F, report);
  PP_CHECK_LAUNCH("calib_score_kernel");
  return 0;
}
