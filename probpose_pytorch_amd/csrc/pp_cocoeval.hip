// CocoKeypointEval: COCO keypoint AP / AR on the device (probpose_pytorch_amd/cocoeval.py), three launches.
//
// A ragged batch is three CSR offset rows of n_img + 1 int64 each, kept in one array `offs`:
//   offs[0 .. n_img]                   det_off: image i owns detections det_off[i] .. det_off[i+1], already in
//                                      descending score order and cut to max_dets
//   offs[n_img+1 .. 2 n_img+1]         gt_off:  image i owns ground truths gt_off[i] .. gt_off[i+1]
//   offs[2 n_img+2 .. 3 n_img+2]       oks_off: image i's D_i x G_i row-major float64 OKS matrix starts at oks_off[i]
// The entry points take the offsets twice: a HOST copy, which they check (start at 0, monotone, oks_off the running
// sum of D_i G_i, totals) before anything is launched, and the DEVICE copy the kernels read.
//
//   cocoeval_oks_kernel         one wave per image, one lane per (detection, ground truth) pair, pairs looped in
//                               steps of 64.  A lane walks its K keypoints in order with the operations of
//                               tests/cocoeval_reference.py's compute_oks one for one (compiled -ffp-contract=off), so
//                               the exponent e is the gauge's bit for bit and the only differences are exp() and the
//                               roundings of a K-term sum of terms that differ by exp()'s error
//                               (tests/test_cocoeval_gpu.py counts them).  Its second form, <true>, is Ex-OKS
//                               (pp_cocoeval_exoks): per annotated keypoint the ground truth is inside its activation
//                               window or not and the detection's presence probability reaches the threshold or not;
//                               both: the plain term, same operations; inside but reported absent: 0; outside and
//                               reported absent: 1; outside but reported present: exp(-e) of the depth b of the
//                               prediction inside the window.  The 0 and 1 terms are exact, so the plain bound holds
//                               (tests/test_exoks_gpu.py).  The four cases diverge per keypoint within a wave; the
//                               kernel is 2 % of an evaluation, so they are left to.
//   cocoeval_match_kernel      one wave per (image, area range, threshold), four waves to a workgroup.
//                               Detections are visited one after the other; for one detection the 64 lanes stride
//                               over the ground truths, each lane keeping its best candidate of the non-ignored
//                               and of the ignored ground truths with a >=
//                               update (the later index wins), and a wave max-reduction that prefers the larger index
//                               on equal OKS picks the winner.  Non-ignored ground truths come first in the gauge's
//                               walk and the walk stops at the first ignored one once a non-ignored match is held, so:
//                               a non-ignored candidate wins whenever there is one, otherwise the ignored candidate.
//                               The ignore-first order of an area range is never materialised.  Lane g % 64 owns the
//                               matched byte of ground truth g: it clears it, reads it and sets it, no other lane does.
//   cocoeval_accumulate_kernel  one workgroup per (area range, threshold): a forward block scan of tp / fp over the
//                               globally score-sorted detections, the right-to-left maximum envelope of precision as a
//                               backward block scan, and 101 binary searches on the integer tp counts.
//
// No float atomics: the only atomic is the int32 count of non-ignored ground truths per area range (integer addition
// is exact in any order).  No host synchronisation; every kernel writes plain vector stores; the same bits on every
// call.
#include <float.h>

#include "pp_common.h"

namespace pp {

constexpr int kCocoAccThreads = 1024;
constexpr int kCocoMatchWaves = 4;

// EX = false: plain OKS (det_presence and gt_window are not read).  EX = true: Ex-OKS, the same loop with the four
// presence cases of the header per annotated keypoint; the both-present case is the plain term, operation for operation.
template <bool EX>
__global__ __launch_bounds__(64) void cocoeval_oks_kernel(
    int n_img, int K, const long long *__restrict__ offs, const double *__restrict__ det_kpts,
    const double *__restrict__ gt_kpts, const double *__restrict__ gt_bbox, const double *__restrict__ gt_area,
    const unsigned char *__restrict__ gt_flags, const double *__restrict__ vars,
    const double *__restrict__ det_presence, const double *__restrict__ gt_window, double presence_thr,
    double *__restrict__ oks) {
  const int img = blockIdx.x;
  if (img >= n_img) return;
  const long long d0 = offs[img], D = offs[img + 1] - d0;
  const long long g0 = offs[n_img + 1 + img], G = offs[n_img + 2 + img] - g0;
  const long long o0 = offs[2 * n_img + 2 + img];
  const long long pairs = D * G;
  for (long long p = threadIdx.x; p < pairs; p += 64) {
    const long long d = p / G, g = p - d * G;
    const double *dk = det_kpts + (d0 + d) * (long long)K * 2;
    const double *gk = gt_kpts + (g0 + g) * (long long)K * 3;
    const double size = gt_area[g0 + g] + DBL_EPSILON;
    double sum = 0.0;
    int cnt = 0;
    if (!(gt_flags[g0 + g] & PP_COCO_GT_NO_VISIBLE)) {
      double wx0 = 0.0, wy0 = 0.0, wx1 = 0.0, wy1 = 0.0;
      const double *pr = nullptr;
      if constexpr (EX) {
        const double *w = gt_window + (g0 + g) * 4;
        wx0 = w[0], wy0 = w[1], wx1 = w[2], wy1 = w[3];
        pr = det_presence + (d0 + d) * (long long)K;
      }
      for (int k = 0; k < K; ++k) {
        if (gk[3 * k + 2] > 0.0) {
          bool gin = true, pin = true;
          if constexpr (EX) {
            const double xg = gk[3 * k], yg = gk[3 * k + 1];
            gin = wx0 <= xg && xg < wx1 && wy0 <= yg && yg < wy1;
            pin = pr[k] >= presence_thr;
          }
          if (gin && pin) {
            const double dx = dk[2 * k] - gk[3 * k], dy = dk[2 * k + 1] - gk[3 * k + 1];
            const double e = (dx * dx + dy * dy) / vars[k] / size / 2.0;
            sum += exp(-e);
          } else if (!gin && !pin) {        // correctly reported absent
            sum += 1.0;
          } else if (!gin) {                // a false positive: charged by its depth inside the window
            const double xd = dk[2 * k], yd = dk[2 * k + 1];
            const double b = fmax(0.0, fmin(fmin(xd - wx0, wx1 - xd), fmin(yd - wy0, wy1 - yd)));
            const double e = b * b / vars[k] / size / 2.0;
            sum += exp(-e);
          }                                 // gin && !pin: missed, the term is 0
          ++cnt;
        }
      }
    } else {
      const double *bb = gt_bbox + (g0 + g) * 4;
      const double x0 = bb[0] - bb[2], x1 = bb[0] + bb[2] * 2.0;
      const double y0 = bb[1] - bb[3], y1 = bb[1] + bb[3] * 2.0;
      for (int k = 0; k < K; ++k) {
        const double xd = dk[2 * k], yd = dk[2 * k + 1];
        const double dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1);
        const double dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        const double e = (dx * dx + dy * dy) / vars[k] / size / 2.0;
        sum += exp(-e);
      }
      cnt = K;
    }
    oks[o0 + p] = sum / (double)cnt;
  }
}

// the better of two (OKS, ground truth) candidates: larger OKS, on equal OKS the larger index; idx < 0 = none
__device__ __forceinline__ void coco_take_better(double &v, long long &i, double ov, long long oi) {
  if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi > i))) {
    v = ov;
    i = oi;
  }
}
__device__ __forceinline__ void coco_wave_best(double &v, long long &i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const long long oi = __shfl_xor(i, o, 64);
    coco_take_better(v, i, ov, oi);
  }
}

__global__ __launch_bounds__(64 * kCocoMatchWaves) void cocoeval_match_kernel(
    int n_img, int A, int T, long long Dtot, long long Gtot, const long long *__restrict__ offs,
    const double *__restrict__ oks, const unsigned char *__restrict__ gt_flags, const double *__restrict__ gt_area,
    const double *__restrict__ det_area, const double *__restrict__ area_ranges, const double *__restrict__ thr,
    unsigned char *__restrict__ gt_matched, unsigned char *__restrict__ dt_matched,
    unsigned char *__restrict__ dt_ignore, int *__restrict__ npig) {
  // four independent waves per workgroup, consecutive triples of (mostly) one image: they share its OKS rows in L1
  const long long triple = (long long)blockIdx.x * kCocoMatchWaves + (threadIdx.x >> 6);
  if (triple >= (long long)n_img * A * T) return;
  const int img = (int)(triple / (A * T)), at = (int)(triple - (long long)img * (A * T));
  const int a = at / T, t = at - a * T, lane = threadIdx.x & 63;
  const long long d0 = offs[img], D = offs[img + 1] - d0;
  const long long g0 = offs[n_img + 1 + img], G = offs[n_img + 2 + img] - g0;
  const double *M = oks + offs[2 * n_img + 2 + img];
  const double lo = area_ranges[2 * a], hi = area_ranges[2 * a + 1];
  unsigned char *gm = gt_matched + (long long)at * Gtot + g0;
  const unsigned char *gf = gt_flags + g0;
  const double *ga = gt_area + g0;

  int live = 0;
  for (long long g = lane; g < G; g += 64) {
    gm[g] = 0;
    const bool ig = (gf[g] & (PP_COCO_GT_CROWD | PP_COCO_GT_NO_VISIBLE)) || ga[g] < lo || ga[g] > hi;
    live += ig ? 0 : 1;
  }
  if (t == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) live += __shfl_xor(live, o, 64);
    if (lane == 0 && live) atomicAdd(npig + a, live);
  }

  const double start = fmin(thr[t], 1.0 - 1e-10);
  for (long long d = 0; d < D; ++d) {
    const double *row = M + d * G;
    double v_live = 0.0, v_ign = 0.0;
    long long i_live = -1, i_ign = -1;
    for (long long g = lane; g < G; g += 64) {
      const unsigned char f = gf[g];
      const bool crowd = f & PP_COCO_GT_CROWD;
      if (gm[g] && !crowd) continue;
      const double v = row[g];
      if (v < start) continue;
      const bool ig = (f & (PP_COCO_GT_CROWD | PP_COCO_GT_NO_VISIBLE)) || ga[g] < lo || ga[g] > hi;
      if (ig) {
        if (i_ign < 0 || v >= v_ign) { v_ign = v; i_ign = g; }
      } else {
        if (i_live < 0 || v >= v_live) { v_live = v; i_live = g; }
      }
    }
    coco_wave_best(v_live, i_live);
    coco_wave_best(v_ign, i_ign);
    const long long m = i_live >= 0 ? i_live : i_ign;
    if (m >= 0 && (m & 63) == lane) gm[m] = 1;
    if (lane == 0) {
      const double da = det_area[d0 + d];
      const long long o = (long long)at * Dtot + d0 + d;
      dt_matched[o] = m >= 0;
      dt_ignore[o] = m >= 0 ? (i_live < 0) : (da < lo || da > hi);
    }
  }
}

// inclusive scans over the threads of a workgroup; `carry` holds the running total across calls
__device__ __forceinline__ int2 coco_block_scan_add(int2 v, int2 *wave_tot, int2 &carry) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int x = __shfl_up(v.x, o, 64), y = __shfl_up(v.y, o, 64);
    if (lane >= o) { v.x += x; v.y += y; }
  }
  __syncthreads();                       // the previous call's readers are done with wave_tot
  if (lane == 63) wave_tot[w] = v;
  __syncthreads();
  int2 base = carry, total = carry;
  for (int j = 0; j < kCocoAccThreads / 64; ++j) {
    const int2 s = wave_tot[j];
    if (j < w) { base.x += s.x; base.y += s.y; }
    total.x += s.x;
    total.y += s.y;
  }
  carry = total;
  v.x += base.x;
  v.y += base.y;
  return v;
}
// inclusive maximum from the RIGHT: thread i gets max(v[i .. last], carry)
__device__ __forceinline__ double coco_block_scan_max_right(double v, double *wave_max, double &carry) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double x = __shfl_down(v, o, 64);
    if (lane + o < 64) v = fmax(v, x);
  }
  __syncthreads();
  if (lane == 0) wave_max[w] = v;
  __syncthreads();
  double total = carry;
  for (int j = kCocoAccThreads / 64 - 1; j >= 0; --j) {
    const double s = wave_max[j];
    if (j > w) v = fmax(v, s);
    total = fmax(total, s);
  }
  v = fmax(v, carry);
  carry = total;
  return v;
}

__global__ __launch_bounds__(kCocoAccThreads) void cocoeval_accumulate_kernel(
    long long Dtot, int A, int T, int R, const long long *__restrict__ order,
    const unsigned char *__restrict__ dt_matched, const unsigned char *__restrict__ dt_ignore,
    const int *__restrict__ npig, const double *__restrict__ rec_thr, double *__restrict__ ws_env,
    int *__restrict__ ws_tp, double *__restrict__ precision, double *__restrict__ recall) {
  __shared__ int2 s_tot[kCocoAccThreads / 64];
  __shared__ double s_max[kCocoAccThreads / 64];
  const int at = blockIdx.x, a = at / T, t = at - a * T, tid = threadIdx.x;
  if (a >= A) return;
  const int n_gt = npig[a];
  if (n_gt == 0) {        // nothing to find in this area range: the entries are marked absent
    for (int r = tid; r < R; r += kCocoAccThreads) precision[((long long)t * R + r) * A + a] = -1.0;
    if (tid == 0) recall[t * A + a] = -1.0;
    return;
  }
  const unsigned char *dm = dt_matched + (long long)at * Dtot, *di = dt_ignore + (long long)at * Dtot;
  double *env = ws_env + (long long)at * Dtot;
  int *tps = ws_tp + (long long)at * Dtot;
  const long long padded = (Dtot + kCocoAccThreads - 1) / kCocoAccThreads * kCocoAccThreads;

  // forward: cumulative tp / fp over the non-ignored detections.  An ignored detection repeats the counts in front of
  // it, so it repeats their precision and recall: it adds no new value to the envelope or to the sampled curve.
  int2 carry = make_int2(0, 0);
  for (long long p0 = 0; p0 < padded; p0 += kCocoAccThreads) {
    const long long p = p0 + tid;
    int2 v = make_int2(0, 0);
    if (p < Dtot) {
      const long long i = order[p];
      if (i >= 0 && i < Dtot && !di[i]) v = dm[i] ? make_int2(1, 0) : make_int2(0, 1);
    }
    v = coco_block_scan_add(v, s_tot, carry);
    if (p < Dtot) {
      tps[p] = v.x;
      env[p] = (double)v.x / ((double)(v.x + v.y) + DBL_EPSILON);
    }
  }
  const int tp_last = carry.x;
  // backward: precision made non-increasing from the right (a maximum: exact in any order)
  double mcarry = 0.0;
  for (long long p0 = padded - kCocoAccThreads; p0 >= 0; p0 -= kCocoAccThreads) {
    const long long p = p0 + tid;
    double v = p < Dtot ? env[p] : 0.0;
    v = coco_block_scan_max_right(v, s_max, mcarry);
    if (p < Dtot) env[p] = v;
  }
  __syncthreads();        // env and tps of every thread are visible to the searches below
  // recall thresholds: the first position whose recall tp / n_gt reaches r
  for (int r = tid; r < R; r += kCocoAccThreads) {
    const double want = rec_thr[r];
    long long lo = 0, hi = Dtot;
    while (lo < hi) {
      const long long mid = lo + (hi - lo) / 2;
      if ((double)tps[mid] / (double)n_gt >= want) hi = mid;
      else lo = mid + 1;
    }
    precision[((long long)t * R + r) * A + a] = lo < Dtot ? env[lo] : 0.0;
  }
  if (tid == 0) recall[t * A + a] = Dtot > 0 ? (double)tp_last / (double)n_gt : 0.0;
}

// the host copy of the offsets: [det_off | gt_off | oks_off], n_img + 1 entries each
static int coco_check_offsets(const char *who, int n_img, const long long *h, long long Dtot, long long Gtot,
                              long long oks_total) {
  PP_REQUIRE(n_img >= 0, "%s: n_img=%d", who, n_img);
  PP_REQUIRE(h, "%s: null host offsets", who);
  const long long *d = h, *g = h + n_img + 1, *o = h + 2 * (n_img + 1);
  PP_REQUIRE(d[0] == 0 && g[0] == 0 && o[0] == 0, "%s: offsets do not start at 0 (det %lld, gt %lld, oks %lld)", who,
             d[0], g[0], o[0]);
  for (int i = 0; i < n_img; ++i) {
    PP_REQUIRE(d[i + 1] >= d[i], "%s: detection offsets are not monotone at image %d (%lld after %lld)", who, i,
               d[i + 1], d[i]);
    PP_REQUIRE(g[i + 1] >= g[i], "%s: ground-truth offsets are not monotone at image %d (%lld after %lld)", who, i,
               g[i + 1], g[i]);
  }
  for (int i = 0; i < n_img; ++i)
    PP_REQUIRE(o[i + 1] - o[i] == (d[i + 1] - d[i]) * (g[i + 1] - g[i]),
               "%s: OKS offsets of image %d span %lld entries, expected D x G = %lld x %lld", who, i, o[i + 1] - o[i],
               d[i + 1] - d[i], g[i + 1] - g[i]);
  PP_REQUIRE(d[n_img] == Dtot && g[n_img] == Gtot && o[n_img] == oks_total,
             "%s: offsets end at (det %lld, gt %lld, oks %lld), the arrays hold (%lld, %lld, %lld)", who, d[n_img],
             g[n_img], o[n_img], Dtot, Gtot, oks_total);
  return 0;
}

// both OKS entries: the checks they share, then the launch of one form of the kernel
template <bool EX>
static int coco_oks_launch(const char *who, int n_img, int K, long long Dtot, long long Gtot, long long oks_total,
                           const long long *host_offs, const void *offs, const void *det_kpts, const void *gt_kpts,
                           const void *gt_bbox, const void *gt_area, const void *gt_flags, const void *vars,
                           const void *det_presence, const void *gt_window, double presence_thr, void *oks,
                           void *stream) {
  PP_REQUIRE(K > 0, "%s: K=%d", who, K);
  PP_REQUIRE(offs && det_kpts && gt_kpts && gt_bbox && gt_area && gt_flags && vars && oks &&
                 (!EX || (det_presence && gt_window)),
             "%s: null argument", who);
  if constexpr (EX)       // written so that a NaN fails it
    PP_REQUIRE(presence_thr >= 0.0 && presence_thr <= 1.0, "%s: presence_thr=%g is not in [0, 1]", who, presence_thr);
  if (int rc = coco_check_offsets(who, n_img, host_offs, Dtot, Gtot, oks_total)) return rc;
  if (n_img == 0 || oks_total == 0) return 0;
  hipLaunchKernelGGL(cocoeval_oks_kernel<EX>, dim3(n_img), dim3(64), 0, (hipStream_t)stream, n_img, K,
                     (const long long *)offs, (const double *)det_kpts, (const double *)gt_kpts,
                     (const double *)gt_bbox, (const double *)gt_area, (const unsigned char *)gt_flags,
                     (const double *)vars, (const double *)det_presence, (const double *)gt_window, presence_thr,
                     (double *)oks);
  PP_CHECK_LAUNCH(EX ? "cocoeval_oks_kernel<ex>" : "cocoeval_oks_kernel");
  return 0;
}

}  // namespace pp

extern "C" int pp_cocoeval_oks(int n_img, int K, long long Dtot, long long Gtot, long long oks_total,
                               const long long *host_offs, const void *offs, const void *det_kpts,
                               const void *gt_kpts, const void *gt_bbox, const void *gt_area, const void *gt_flags,
                               const void *vars, void *oks, void *stream) {
  return pp::coco_oks_launch<false>("pp_cocoeval_oks", n_img, K, Dtot, Gtot, oks_total, host_offs, offs, det_kpts,
                                    gt_kpts, gt_bbox, gt_area, gt_flags, vars, nullptr, nullptr, 0.0, oks, stream);
}

extern "C" int pp_cocoeval_exoks(int n_img, int K, long long Dtot, long long Gtot, long long oks_total,
                                 const long long *host_offs, const void *offs, const void *det_kpts,
                                 const void *gt_kpts, const void *gt_bbox, const void *gt_area, const void *gt_flags,
                                 const void *vars, const void *det_presence, const void *gt_window,
                                 double presence_thr, void *oks, void *stream) {
  return pp::coco_oks_launch<true>("pp_cocoeval_exoks", n_img, K, Dtot, Gtot, oks_total, host_offs, offs, det_kpts,
                                   gt_kpts, gt_bbox, gt_area, gt_flags, vars, det_presence, gt_window, presence_thr,
                                   oks, stream);
}

extern "C" int pp_cocoeval_match(int n_img, int A, int T, long long Dtot, long long Gtot, long long oks_total,
                                 const long long *host_offs, const void *offs, const void *oks, const void *gt_flags,
                                 const void *gt_area, const void *det_area, const void *area_ranges, const void *thr,
                                 void *gt_matched, void *dt_matched, void *dt_ignore, void *npig, void *stream) {
  using namespace pp;
  PP_REQUIRE(A > 0 && T > 0 && (long long)A * T <= 65535, "pp_cocoeval_match: A=%d area ranges x T=%d thresholds", A,
             T);
  const long long blocks = ((long long)(n_img > 0 ? n_img : 0) * A * T + kCocoMatchWaves - 1) / kCocoMatchWaves;
  PP_REQUIRE(blocks < (1ll << 31), "pp_cocoeval_match: %d images x %d x %d triples exceed one grid", n_img, A, T);
  PP_REQUIRE(offs && oks && gt_flags && gt_area && det_area && area_ranges && thr && gt_matched && dt_matched &&
                 dt_ignore && npig,
             "pp_cocoeval_match: null argument");
  if (int rc = coco_check_offsets("pp_cocoeval_match", n_img, host_offs, Dtot, Gtot, oks_total)) return rc;
  PP_CHECK_HIP(hipMemsetAsync(npig, 0, sizeof(int) * (size_t)A, (hipStream_t)stream));
  if (n_img == 0) return 0;
  hipLaunchKernelGGL(cocoeval_match_kernel, dim3((unsigned)blocks), dim3(64 * kCocoMatchWaves), 0,
                     (hipStream_t)stream, n_img, A, T, Dtot,
                     Gtot, (const long long *)offs, (const double *)oks, (const unsigned char *)gt_flags,
                     (const double *)gt_area, (const double *)det_area, (const double *)area_ranges,
                     (const double *)thr, (unsigned char *)gt_matched, (unsigned char *)dt_matched,
                     (unsigned char *)dt_ignore, (int *)npig);
  PP_CHECK_LAUNCH("cocoeval_match_kernel");
  return 0;
}

extern "C" int pp_cocoeval_accumulate(long long Dtot, int A, int T, int R, const void *order, const void *dt_matched,
                                      const void *dt_ignore, const void *npig, const void *rec_thr, void *ws_env,
                                      void *ws_tp, void *precision, void *recall, void *stream) {
  using namespace pp;
  PP_REQUIRE(Dtot >= 0 && Dtot < (1ll << 31), "pp_cocoeval_accumulate: Dtot=%lld (the counts are int32)", Dtot);
  PP_REQUIRE(A > 0 && T > 0 && R > 0, "pp_cocoeval_accumulate: A=%d, T=%d, R=%d", A, T, R);
  PP_REQUIRE(order && dt_matched && dt_ignore && npig && rec_thr && ws_env && ws_tp && precision && recall,
             "pp_cocoeval_accumulate: null argument");
  hipLaunchKernelGGL(cocoeval_accumulate_kernel, dim3(A * T), dim3(kCocoAccThreads), 0, (hipStream_t)stream, Dtot, A,
                     T, R, (const long long *)order, (const unsigned char *)dt_matched,
                     (const unsigned char *)dt_ignore, (const int *)npig, (const double *)rec_thr, (double *)ws_env,
                     (int *)ws_tp, (double *)precision, (double *)recall);
  PP_CHECK_LAUNCH("cocoeval_accumulate_kernel");
  return 0;
}
