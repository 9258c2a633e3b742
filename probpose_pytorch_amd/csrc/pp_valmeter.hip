// ValidationMeter: whole-set validation and head calibration statistics, accumulated on the device.
//
// Replaces the per-batch host work of the reference's validation loop (train.py:124-168) around
// ProbPoseLoss.forward(compute_acc=True): get_binary_accuracy (loss.py:653-697), get_mae (loss.py:699-712), the
// averaging of the losses and accuracies (train.py:146-167).  pp_valmeter_update adds one batch to an INTEGER state
// (counts and fixed-point sums, 64-bit atomics), so the state does not depend on batch order, batch split or atomic
// order; pp_valmeter_report turns the state into float64 statistics per keypoint and pooled.  The state layout
// (pp_valmeter_state.h) and the report fields are documented in include/probpose_hip.h; tests/valmeter_reference.py
// restates both.
//
// Compiled -ffp-contract=off: Q30 / Q20 round one float64 product, exactly as numpy does.
#include <algorithm>

#include "pp_valmeter_state.h"

namespace pp {

constexpr int VM_GLOBALS = 18;
constexpr int VM_BINARY_FIXED = 10, VM_OKS_FIXED = 5, VM_ERR_FIELDS = 3;
// flag bits the meter adds to those of pp_probpose_loss_terms
constexpr long long VM_FLAG_TARGET_RANGE = 256, VM_FLAG_NONFINITE = 512;

struct VmBatch {
  const float *dt_prob, *dt_vis, *dt_oks, *dt_err, *gt_oks, *gt_err;
  const int *in_image, *annotated, *visibility;
  const double *thresholds;
  const int *pck_counts;
  const float *map_max, *res;
};

__device__ __forceinline__ u64 q_fixed(double z, double scale) { return (u64)(long long)__builtin_rint(z * scale); }
__device__ __forceinline__ bool err_ok(float x) { return x >= 0.0f && x <= 1048576.0f; }    // NaN, inf: false

// the workgroup's private counters: above[2][2][J], sum_p[2][2], sum_p2[2][2], oks sums, err, all, rejected
constexpr int VM_LOCAL_FIXED = 4 + 4 + VM_OKS_SUMS + VM_ERR_SUMS + VM_ALL + VM_REJECTED;

// grid (K, chunks + 1): workgroup (k, c < chunks) takes the samples b = c * 256 + t, + chunks * 256, ... of keypoint k;
// the workgroups (k, chunks) add keypoint k's PCK counts, and (0, chunks) reduces map_max and adds the batch scalars.
__global__ __launch_bounds__(256) void valmeter_update_kernel(VmBatch in, int B, int K, int J, int chunks,
                                                              long long *__restrict__ state_) {
  __shared__ u64 lc[4 * VM_MAX_J + VM_LOCAL_FIXED];
  __shared__ double thr[VM_MAX_J];
  __shared__ float red_v[256];
  __shared__ int red_nan[256];
  u64 *state = reinterpret_cast<u64 *>(state_);
  const VmLayout L = vm_layout(K, J);
  const int tid = threadIdx.x, k = blockIdx.x;

  if ((int)blockIdx.y == chunks) {
    if (in.pck_counts && tid == 0) {
      atomicAdd(&state[L.pck + k], (u64)(long long)in.pck_counts[k]);
      atomicAdd(&state[L.pck + K + k], (u64)(long long)in.pck_counts[K + k]);
    }
    if (k != 0) return;
    // the batch's maximum of map_max; a NaN wins (pred[0].max())
    float m = -__builtin_inff();
    int any_nan = 0;
    if (in.map_max) {
      const long long total = (long long)B * K;
      for (long long i = tid; i < total; i += 256) {
        const float v = in.map_max[i];
        if (v != v) any_nan = 1;
        else m = fmaxf(m, v);
      }
    }
    red_v[tid] = m;
    red_nan[tid] = any_nan;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) {
        red_v[tid] = fmaxf(red_v[tid], red_v[tid + o]);
        red_nan[tid] |= red_nan[tid + o];
      }
      __syncthreads();
    }
    if (tid != 0) return;
    // the per-batch scalars: one thread, float64, in the order of the updates
    long long *S = state_ + L.scalars;
    double *D = reinterpret_cast<double *>(S + 6);
    S[0] += 1;
    bool flagged = false;
    if (in.res) {
      float r[11];
      for (int i = 0; i < 11; ++i) r[i] = in.res[i];
      long long word = 0;
      if (r[9] == r[9] && fabsf(r[9]) < 2147483648.0f) word = (long long)(int)r[9];
      else word = VM_FLAG_NONFINITE;
      if (r[2] != 0.0f) word |= VM_FLAG_TARGET_RANGE;
      bool finite = isfinite(r[1]);
      for (int i = 3; i <= 8; ++i) finite = finite && isfinite(r[i]);
      if (!finite) word |= VM_FLAG_NONFINITE;
      flagged = r[9] != 0.0f || r[2] != 0.0f || !finite;
      S[2] |= word;
      if (flagged) {
        S[1] += 1;
      } else {
        S[3] += 1;
        D[0] += (double)r[1];
        for (int i = 3; i <= 8; ++i) D[i - 2] += (double)r[i];
      }
    }
    if (in.pck_counts && !flagged) {     // _accuracy_from_counts of this batch, summed in keypoint order
      double s = 0.0;
      int cnt = 0;
      for (int j = 0; j < K; ++j) {
        const int v = in.pck_counts[K + j];
        if (v > 0) {
          s += (double)in.pck_counts[j] / (double)v;
          ++cnt;
        }
      }
      S[4] += 1;
      D[7] += cnt ? s / (double)cnt : 0.0;
    }
    if (in.map_max) {
      const double bm = red_nan[0] ? (double)__builtin_nanf("") : (double)red_v[0];
      const double cur = D[8];
      if (S[5] == 0 || bm != bm || (cur == cur && bm > cur)) D[8] = bm;
      S[5] += 1;
    }
    return;
  }

  const int nlocal = 4 * J + VM_LOCAL_FIXED;
  for (int i = tid; i < nlocal; i += 256) lc[i] = 0;
  if (tid < J) thr[tid] = in.thresholds[tid];
  __syncthreads();
  u64 *l_above = lc, *l_sp = lc + 4 * J, *l_sp2 = l_sp + 4, *l_oks = l_sp2 + 4, *l_err = l_oks + 5, *l_all = l_err + 4,
      *l_rej = l_all + 3;

  for (long long b = (long long)blockIdx.y * 256 + tid; b < B; b += (long long)chunks * 256) {
    const long long idx = b * K + k;
    const float prob = in.dt_prob[idx];
    atomicAdd(&l_all[0], 1ull);
    if (vm_unit_ok(prob)) {
      atomicAdd(&l_all[1], 1ull);
      atomicAdd(&l_all[2], q_fixed((double)prob, VM_Q30));
    }
    const int im = in.in_image[idx], an = in.annotated[idx];
    if ((im != 0 && im != 1) || (an != 0 && an != 1)) {
      atomicAdd(&l_rej[0], 1ull);
      continue;
    }
    if (!an) continue;
    // the two binary heads: probability over the annotated samples, visibility over the annotated ones in the image
    for (int h = 0; h < 2; ++h) {
      if (h == 1 && !im) break;
      const float p = h == 0 ? prob : in.dt_vis[idx];
      const int label = h == 0 ? im : (in.visibility[idx] != 0);
      if (!vm_unit_ok(p)) {
        atomicAdd(&l_rej[1 + h], 1ull);
        continue;
      }
      const double pd = (double)p;
      const int bin = vm_fine_bin(p);
      const long long hk = (long long)h * K + k;
      atomicAdd(&state[L.hist + (hk * 2 + label) * VM_BINS + bin], 1ull);
      atomicAdd(&state[L.conf + hk * VM_BINS + bin], q_fixed(pd, VM_Q30));
      atomicAdd(&l_sp[h * 2 + label], q_fixed(pd, VM_Q30));
      atomicAdd(&l_sp2[h * 2 + label], q_fixed(pd * pd, VM_Q30));
      for (int j = 0; j < J; ++j)
        if (pd > thr[j]) atomicAdd(&l_above[(h * 2 + label) * J + j], 1ull);
    }
    if (!im) continue;
    {
      const float x = in.dt_oks[idx], t = in.gt_oks[idx];
      if (!vm_unit_ok(x) || !vm_unit_ok(t)) {
        atomicAdd(&l_rej[3], 1ull);
      } else {
        const double xd = (double)x, td = (double)t, d = xd - td;
        const int bin = vm_fine_bin(x);
        atomicAdd(&state[L.oks_hist + (long long)k * VM_BINS + bin], 1ull);
        atomicAdd(&state[L.oks_sx + (long long)k * VM_BINS + bin], q_fixed(xd, VM_Q30));
        atomicAdd(&state[L.oks_st + (long long)k * VM_BINS + bin], q_fixed(td, VM_Q30));
        atomicAdd(&l_oks[0], q_fixed(fabs(d), VM_Q30));
        atomicAdd(&l_oks[1], q_fixed(d * d, VM_Q30));
        atomicAdd(&l_oks[2], q_fixed(xd * xd, VM_Q30));
        atomicAdd(&l_oks[3], q_fixed(td * td, VM_Q30));
        atomicAdd(&l_oks[4], q_fixed(xd * td, VM_Q30));
      }
    }
    {
      const float x = in.dt_err[idx], t = in.gt_err[idx];
      if (!err_ok(x) || !err_ok(t)) {
        atomicAdd(&l_rej[4], 1ull);
      } else {
        const double xd = (double)x, td = (double)t;
        atomicAdd(&l_err[0], 1ull);
        atomicAdd(&l_err[1], q_fixed(xd, VM_Q20));
        atomicAdd(&l_err[2], q_fixed(td, VM_Q20));
        atomicAdd(&l_err[3], q_fixed(fabs(xd - td), VM_Q20));
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < nlocal; i += 256) {
    const u64 v = lc[i];
    if (!v) continue;
    long long at;
    if (i < 4 * J) {
      const int h = i / (2 * J), rem = i - h * 2 * J;
      at = L.above + ((long long)h * K + k) * 2 * J + rem;
    } else {
      const int f = i - 4 * J;
      if (f < 4) at = L.sum_p + ((long long)(f >> 1) * K + k) * 2 + (f & 1);
      else if (f < 8) at = L.sum_p2 + ((long long)((f - 4) >> 1) * K + k) * 2 + (f & 1);
      else if (f < 13) at = L.oks_sums + (long long)k * VM_OKS_SUMS + (f - 8);
      else if (f < 17) at = L.err + (long long)k * VM_ERR_SUMS + (f - 13);
      else if (f < 20) at = L.all + (f - 17);
      else at = L.rejected + (f - 20);
    }
    atomicAdd(&state[at], v);
  }
}

// sum over the keypoints k0 .. k1-1 of state[base + k * stride]
__device__ __forceinline__ long long vm_sum_k(const long long *state, long long base, long long stride, int k0,
                                              int k1) {
  long long s = 0;
  for (int k = k0; k < k1; ++k) s += state[base + k * stride];
  return s;
}

// grid (K + 1, 4): row = keypoint (K = the pool, summed from the integer state); part 0 / 1 = the probability /
// visibility head, 2 = the OKS head, 3 = the error head, PCK and the whole-set fields.  256 threads.
__global__ __launch_bounds__(256) void valmeter_report_kernel(const long long *__restrict__ state,
                                                              const double *__restrict__ thresholds, int K, int J,
                                                              int E, int F, double *__restrict__ out) {
  __shared__ long long a[VM_BINS], b[VM_BINS], c[VM_BINS];
  __shared__ long long scan[256];
  __shared__ long long tot[4];
  __shared__ long long vals[VM_MAX_J];
  __shared__ double mx[256];
  const VmLayout L = vm_layout(K, J);
  const int tid = threadIdx.x, row = blockIdx.x, part = blockIdx.y;
  const auto [k0, k1] = vm_row_range(row, K);
  const int bin_fields = VM_BINARY_FIXED + J + 3 * E, oks_fields = VM_OKS_FIXED + 3 * E;
  double *o = out + (long long)row * F;
  const int width = VM_BINS / E;
  if (tid < 4) tot[tid] = 0;

  if (part < 2) {
    const int h = part;
    o += h * bin_fields;
    for (int i = tid; i < VM_BINS; i += 256) {
      a[i] = vm_sum_k(state, L.hist + ((long long)h * K * 2 + 0) * VM_BINS + i, 2 * VM_BINS, k0, k1);   // negatives
      b[i] = vm_sum_k(state, L.hist + ((long long)h * K * 2 + 1) * VM_BINS + i, 2 * VM_BINS, k0, k1);   // positives
      c[i] = vm_sum_k(state, L.conf + (long long)h * K * VM_BINS + i, VM_BINS, k0, k1);
    }
    __syncthreads();
    // suffix scan of the positives over the fine bins: thread t owns bins 4t .. 4t+3
    long long p4 = 0, n4 = 0;
    for (int i = 0; i < 4; ++i) p4 += b[4 * tid + i], n4 += a[4 * tid + i];
    scan[tid] = p4;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const long long v = tid + off < 256 ? scan[tid + off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    long long above = scan[tid] - p4, num = 0;     // positives in the bins above this thread's
    for (int i = 3; i >= 0; --i) {
      const int bin = 4 * tid + i;
      num += a[bin] * (2 * above + b[bin]);
      above += b[bin];
    }
    atomicAdd(reinterpret_cast<u64 *>(&tot[0]), (u64)num);
    atomicAdd(reinterpret_cast<u64 *>(&tot[1]), (u64)n4);
    __syncthreads();
    const long long n_pos = scan[0], n_neg = tot[1], n = n_pos + n_neg;
    // balanced accuracy per threshold, as an integer cross product (exact ordering for the arg-max)
    if (tid < J) {
      const long long hk = (long long)h * K;
      const long long a0 = vm_sum_k(state, L.above + hk * 2 * J + tid, 2 * J, k0, k1);
      const long long a1 = vm_sum_k(state, L.above + hk * 2 * J + J + tid, 2 * J, k0, k1);
      const long long v = a1 * n_neg + (n_neg - a0) * n_pos;
      vals[tid] = v;
      o[VM_BINARY_FIXED + tid] =
          (n_pos > 0 && n_neg > 0) ? (double)v / (2.0 * (double)n_pos * (double)n_neg) : vm_nan();
    }
    // coarse bins: |conf_c - pos_c 2^30| summed for the ECE, its largest quotient for the MCE, the reliability table
    double my_mce = -1.0;
    long long my_abs = 0;
    for (int cb = tid; cb < E; cb += 256) {
      long long nc = 0, pc = 0, cc = 0;
      for (int i = cb * width; i < (cb + 1) * width; ++i) nc += a[i] + b[i], pc += b[i], cc += c[i];
      long long d = cc - pc * (1ll << 30);
      if (d < 0) d = -d;
      my_abs += d;
      double *t = o + VM_BINARY_FIXED + J + 3 * cb;
      t[0] = (double)nc;
      if (nc > 0) {
        const double den = (double)nc * VM_Q30;
        my_mce = fmax(my_mce, (double)d / den);
        t[1] = (double)cc / den;
        t[2] = (double)pc / (double)nc;
      } else {
        t[1] = t[2] = vm_nan();
      }
    }
    atomicAdd(reinterpret_cast<u64 *>(&tot[2]), (u64)my_abs);
    mx[tid] = my_mce;
    __syncthreads();
    if (tid != 0) return;
    double mce = -1.0;
    for (int i = 0; i < 256; ++i) mce = fmax(mce, mx[i]);
    const long long hk = (long long)h * K;
    const long long sp0 = vm_sum_k(state, L.sum_p + hk * 2 + 0, 2, k0, k1);
    const long long sp1 = vm_sum_k(state, L.sum_p + hk * 2 + 1, 2, k0, k1);
    const long long sq = vm_sum_k(state, L.sum_p2 + hk * 2 + 0, 2, k0, k1) +
                         vm_sum_k(state, L.sum_p2 + hk * 2 + 1, 2, k0, k1);
    o[0] = (double)n_pos;
    o[1] = (double)n_neg;
    if (n_pos > 0 && n_neg > 0) {
      int best = 0;
      for (int j = 1; j < J; ++j)
        if (vals[j] > vals[best]) best = j;
      o[2] = (double)vals[best] / (2.0 * (double)n_pos * (double)n_neg);
      o[3] = thresholds[best];
      o[4] = (double)tot[0] / (2.0 * (double)n_pos * (double)n_neg);
    } else {
      o[2] = o[3] = 0.0;      // loss.py:670-673
      o[4] = vm_nan();
    }
    if (n > 0) {
      const double den = (double)n * VM_Q30;
      o[5] = (double)(sq - 2 * sp1 + n_pos * (1ll << 30)) / den;     // Brier
      o[6] = (double)tot[2] / den;                                  // ECE
      o[7] = mce;
      o[8] = (double)(sp0 + sp1) / den;
      o[9] = (double)n_pos / (double)n;
    } else {
      for (int i = 5; i < 10; ++i) o[i] = vm_nan();
    }
    return;
  }

  if (part == 2) {
    o += 2 * bin_fields;
    for (int i = tid; i < VM_BINS; i += 256) {
      a[i] = vm_sum_k(state, L.oks_hist + i, VM_BINS, k0, k1);
      b[i] = vm_sum_k(state, L.oks_sx + i, VM_BINS, k0, k1);
      c[i] = vm_sum_k(state, L.oks_st + i, VM_BINS, k0, k1);
    }
    __syncthreads();
    long long mn = 0, msx = 0, mst = 0;
    for (int cb = tid; cb < E; cb += 256) {
      long long nc = 0, sx = 0, st = 0;
      for (int i = cb * width; i < (cb + 1) * width; ++i) nc += a[i], sx += b[i], st += c[i];
      mn += nc, msx += sx, mst += st;
      double *t = o + VM_OKS_FIXED + 3 * cb;
      t[0] = (double)nc;
      if (nc > 0) {
        const double den = (double)nc * VM_Q30;
        t[1] = (double)sx / den;
        t[2] = (double)st / den;
      } else {
        t[1] = t[2] = vm_nan();
      }
    }
    atomicAdd(reinterpret_cast<u64 *>(&tot[0]), (u64)mn);
    atomicAdd(reinterpret_cast<u64 *>(&tot[1]), (u64)msx);
    atomicAdd(reinterpret_cast<u64 *>(&tot[2]), (u64)mst);
    __syncthreads();
    if (tid != 0) return;
    const long long n = tot[0], sx = tot[1], st = tot[2];
    o[0] = (double)n;
    if (n == 0) {
      for (int i = 1; i < 5; ++i) o[i] = vm_nan();
      return;
    }
    long long s[5];
    for (int i = 0; i < 5; ++i) s[i] = vm_sum_k(state, L.oks_sums + i, 5, k0, k1);
    const double den = (double)n * VM_Q30;
    o[1] = (double)s[0] / den;
    o[2] = sqrt((double)s[1] / den);
    o[3] = (double)(sx - st) / den;
    const double mx_ = (double)sx / den, mt = (double)st / den;
    const double vx = (double)s[2] / den - mx_ * mx_, vt = (double)s[3] / den - mt * mt;
    const double cov = (double)s[4] / den - mx_ * mt;
    o[4] = (vx > 0.0 && vt > 0.0) ? cov / sqrt(vx * vt) : vm_nan();
    return;
  }

  // part 3: the error head, PCK and the whole-set fields, one thread
  if (tid != 0) return;
  o += 2 * bin_fields + oks_fields;
  {
    long long s[4];
    for (int i = 0; i < 4; ++i) s[i] = vm_sum_k(state, L.err + i, 4, k0, k1);
    o[0] = (double)s[0];
    if (s[0] > 0) {
      const double den = (double)s[0] * VM_Q20;
      o[1] = (double)s[3] / den;
      o[2] = (double)(s[1] - s[2]) / den;
    } else {
      o[1] = o[2] = vm_nan();
    }
  }
  o += VM_ERR_FIELDS;
  if (row < K) {
    const long long hits = state[L.pck + row], valid = state[L.pck + K + row];
    o[0] = valid > 0 ? (double)hits / (double)valid : -1.0;
    for (int i = 1; i <= VM_GLOBALS; ++i) o[i] = vm_nan();
    return;
  }
  {
    double s = 0.0;
    int cnt = 0;
    for (int k = 0; k < K; ++k) {
      const long long valid = state[L.pck + K + k];
      if (valid > 0) s += (double)state[L.pck + k] / (double)valid, ++cnt;
    }
    o[0] = cnt ? s / (double)cnt : vm_nan();
  }
  o += 1;
  const long long *S = state + L.scalars;
  const double *D = reinterpret_cast<const double *>(S + 6);
  // kpt, probability, visibility, oks, error losses, acc_kpt, acc_oks, acc_error
  for (int i = 0; i < 5; ++i) o[i] = S[3] > 0 ? D[i] / (double)S[3] : vm_nan();
  o[5] = S[4] > 0 ? D[7] / (double)S[4] : vm_nan();
  o[6] = S[3] > 0 ? D[5] / (double)S[3] : vm_nan();
  o[7] = S[3] > 0 ? D[6] / (double)S[3] : vm_nan();
  o[8] = S[5] > 0 ? D[8] : vm_nan();
  const long long *A = state + L.all;
  o[9] = A[1] > 0 ? (double)A[2] / ((double)A[1] * VM_Q30) : vm_nan();
  o[10] = (double)S[0];
  o[11] = (double)S[1];
  o[12] = (double)S[2];
  for (int i = 0; i < 5; ++i) o[13 + i] = (double)state[L.rejected + i];
}

}  // namespace pp

extern "C" long long pp_valmeter_state_words(int K, int J) {
  using namespace pp;
  if (vm_check_shape("pp_valmeter_state_words", K, J)) return -1;
  return vm_layout(K, J).words;
}

extern "C" int pp_valmeter_update(const float *dt_prob, const float *dt_vis, const float *dt_oks, const float *dt_err,
                                  const float *gt_oks, const float *gt_err, const int *in_image, const int *annotated,
                                  const int *visibility, const double *thresholds, int J, const int *pck_counts,
                                  const float *map_max, const float *res, int B, int K, long long *state,
                                  void *stream) {
  using namespace pp;
  if (int rc = vm_check_shape("pp_valmeter_update", K, J)) return rc;
  PP_REQUIRE(B > 0 && (long long)B * K < (1ll << 31), "pp_valmeter_update: bad B=%d (B > 0, B*K < 2^31)", B);
  PP_REQUIRE(thresholds, "pp_valmeter_update: thresholds not given");
  PP_REQUIRE(dt_prob && dt_vis && dt_oks && dt_err, "pp_valmeter_update: null prediction");
  PP_REQUIRE(gt_oks && gt_err, "pp_valmeter_update: null target");
  PP_REQUIRE(in_image && annotated && visibility, "pp_valmeter_update: null mask");
  PP_REQUIRE(state, "pp_valmeter_update: null state");
  const VmBatch in{dt_prob, dt_vis, dt_oks, dt_err, gt_oks, gt_err, in_image, annotated, visibility, thresholds,
                   pck_counts, map_max, res};
  const int chunks = std::min(cdiv(B, 256), 256);
  hipLaunchKernelGGL(valmeter_update_kernel, dim3(K, chunks + 1), dim3(256), 0, (hipStream_t)stream, in, B, K, J,
                     chunks, state);
  PP_CHECK_LAUNCH("valmeter_update_kernel");
  return 0;
}

extern "C" int pp_valmeter_report(const long long *state, const double *thresholds, int K, int J, int ece_bins,
                                  double *report, void *stream) {
  using namespace pp;
  if (int rc = vm_check_shape("pp_valmeter_report", K, J)) return rc;
  PP_REQUIRE(ece_bins >= 1 && ece_bins <= VM_BINS && VM_BINS % ece_bins == 0,
             "pp_valmeter_report: ece_bins=%d does not divide %d", ece_bins, VM_BINS);
  PP_REQUIRE(thresholds, "pp_valmeter_report: thresholds not given");
  PP_REQUIRE(state, "pp_valmeter_report: null state");
  PP_REQUIRE(report, "pp_valmeter_report: null report");
  const int F = 2 * (VM_BINARY_FIXED + J + 3 * ece_bins) + VM_OKS_FIXED + 3 * ece_bins + VM_ERR_FIELDS + 1 + VM_GLOBALS;
  hipLaunchKernelGGL(valmeter_report_kernel, dim3(K + 1, 4), dim3(256), 0, (hipStream_t)stream, state, thresholds, K, J,
                     ece_bins, F, report);
  PP_CHECK_LAUNCH("valmeter_report_kernel");
  return 0;
}
