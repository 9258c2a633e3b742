// PoseNMS: instance rescoring and OKS-NMS of decoded poses (probpose_pytorch_amd/posenms.py), one launch each.
//
//   posenms_rescore_kernel  one lane per detection: the keypoint scores above kpt_thr are added in ascending k and
//                           divided by their number, the box score is multiplied by that mean.  The operations of
//                           tests/posenms_reference.py's rescore one for one (compiled -ffp-contract=off): the same
//                           bits.
//   posenms_kernel          one wave per image, four waves to a workgroup.  The image's detections arrive in visiting
//                           order (descending score, stable).  Lane j % 64 OWNS detection j: its live flag is bit
//                           j / 64 of a 64-bit register of that lane (64 lanes x 64 bits = PP_POSENMS_MAX_DETS), its
//                           current score is element j of the output array, and only that lane ever reads or writes
//                           either; its keep byte is written by that lane alone.  What the whole wave needs of the
//                           pivot goes through shuffles: in hard mode its live bit, in the soft modes the argmax of the
//                           lanes' best (score, index) pairs (wave_max of the scores, then wave_min of the indices that
//                           hold it: the earliest on equal scores).  The pivot's keypoints, visibilities and area are
//                           INPUTS, which every lane reads at a wave-uniform address.  So there is no cross-lane
//                           memory traffic, no atomic, no LDS, no barrier, and the result does not depend on timing.
//                           Each lane evaluates the pair OKS of the pivot and of its own live detections with the
//                           gauge's operations in the gauge's order; what differs is exp() (tests/test_posenms_gpu.py
//                           counts the roundings).  That pair OKS is pp_assoc.h's pair_oks, the function
//                           pp_track.hip's track_oks_kernel calls.
#include <limits.h>
#include <math.h>

#include "pp_assoc.h"

namespace pp {

constexpr int kNmsWaves = 4;
constexpr int kNmsRescoreThreads = 256;

__global__ __launch_bounds__(kNmsRescoreThreads) void posenms_rescore_kernel(
    long long M, int K, const double *__restrict__ kpt_scores, const double *__restrict__ box_scores, double kpt_thr,
    double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * kNmsRescoreThreads + threadIdx.x;
  if (i >= M) return;
  const double *s = kpt_scores + i * K;
  double sum = 0.0;
  int n = 0;
  for (int k = 0; k < K; ++k) {
    const double v = s[k];
    if (v > kpt_thr) {
      sum += v;
      ++n;
    }
  }
  const double mean = n ? sum / (double)n : 0.0;
  out[i] = box_scores[i] * mean;
}

__global__ __launch_bounds__(64 * kNmsWaves) void posenms_kernel(
    int n_img, int K, const long long *__restrict__ off, const double *__restrict__ kpts,
    const double *__restrict__ vis, const double *__restrict__ area, const double *__restrict__ scores,
    const double *__restrict__ vars, int mode, double oks_thr, double vis_thr, int max_dets,
    double *__restrict__ out_scores, unsigned char *__restrict__ keep, int *__restrict__ counts) {
  const long long img = (long long)blockIdx.x * kNmsWaves + (threadIdx.x >> 6);
  if (img >= n_img) return;
  const int lane = threadIdx.x & 63;
  const long long d0 = off[img], span = off[img + 1] - d0;
  if (span <= 0 || span > PP_POSENMS_MAX_DETS) {      // the host has refused the latter; nothing of it is touched
    if (lane == 0) counts[img] = 0;
    return;
  }
  const int D = (int)span, slots = (D + 63) >> 6;
  const double *kp = kpts + d0 * K * 2, *vs = vis ? vis + d0 * K : nullptr, *ar = area + d0;
  double *sc = out_scores + d0;
  unsigned char *kf = keep + d0;

  // lane-owned state: live bits, current scores; the lane's best live (score, index), the earliest on equal scores
  unsigned long long live = 0;
  double best = -INFINITY;
  int best_j = INT_MAX;
  for (int s = 0; s < slots; ++s) {
    const int j = s * 64 + lane;
    if (j < D) {
      const double v = scores[d0 + j];
      sc[j] = v;
      kf[j] = 0;
      live |= 1ull << s;
      if (v > best) {
        best = v;
        best_j = j;
      }
    }
  }

  int kept = 0;
  if (mode == PP_POSENMS_HARD) {
    for (int p = 0; p < D; ++p) {
      const int alive = __shfl((int)((live >> (p >> 6)) & 1ull), p & 63, 64);
      if (!alive) continue;                             // wave-uniform
      ++kept;
      if (lane == (p & 63)) kf[p] = 1;
      const double *kpp = kp + (long long)p * K * 2, *vsp = vs ? vs + (long long)p * K : nullptr;
      const double area_p = ar[p];
      for (int s = p >> 6; s < slots; ++s) {
        const int j = s * 64 + lane;
        if (j > p && ((live >> s) & 1ull)) {
          const double oks = pair_oks(K, kpp, kp + (long long)j * K * 2, vsp, vs ? vs + (long long)j * K : nullptr,
                                      vis_thr, area_p, ar[j], vars);
          if (oks > oks_thr) live &= ~(1ull << s);
        }
      }
    }
  } else {
    const int rounds = D < max_dets ? D : max_dets;
    for (int r = 0; r < rounds; ++r) {
      const double top = wave_max(best);
      const int p = wave_min(best_j != INT_MAX && best == top ? best_j : INT_MAX);
      if (p == INT_MAX) break;                          // nothing live (or nothing comparable): wave-uniform
      ++kept;
      if (lane == (p & 63)) {
        kf[p] = 1;
        live &= ~(1ull << (p >> 6));
      }
      const double *kpp = kp + (long long)p * K * 2, *vsp = vs ? vs + (long long)p * K : nullptr;
      const double area_p = ar[p];
      best = -INFINITY;
      best_j = INT_MAX;
      for (int s = 0; s < slots; ++s) {
        if (!((live >> s) & 1ull)) continue;
        const int j = s * 64 + lane;
        const double oks = pair_oks(K, kpp, kp + (long long)j * K * 2, vsp, vs ? vs + (long long)j * K : nullptr,
                                    vis_thr, area_p, ar[j], vars);
        double v = sc[j];
        if (mode == PP_POSENMS_SOFT_GAUSSIAN) {
          v = v * exp(-(oks * oks) / oks_thr);
          sc[j] = v;
        } else if (oks >= oks_thr) {
          v = v * (1.0 - oks);
          sc[j] = v;
        }
        if (v > best) {
          best = v;
          best_j = j;
        }
      }
    }
  }
  if (lane == 0) counts[img] = kept;
}

static int nms_check_offsets(int n_img, const long long *h, long long Dtot) {
  PP_REQUIRE(n_img >= 0, "pp_posenms: n_img=%d", n_img);
  PP_REQUIRE(Dtot >= 0, "pp_posenms: Dtot=%lld", Dtot);
  PP_REQUIRE(h, "pp_posenms: null host offsets");
  PP_REQUIRE(h[0] == 0, "pp_posenms: offsets do not start at 0 (%lld)", h[0]);
  for (int i = 0; i < n_img; ++i)
    PP_REQUIRE(h[i + 1] >= h[i], "pp_posenms: detection offsets are not monotone at image %d (%lld after %lld)", i,
               h[i + 1], h[i]);
  PP_REQUIRE(h[n_img] == Dtot, "pp_posenms: offsets end at %lld, the arrays hold %lld detections", h[n_img], Dtot);
  for (int i = 0; i < n_img; ++i)
    PP_REQUIRE(h[i + 1] - h[i] <= PP_POSENMS_MAX_DETS,
               "pp_posenms: image %d has %lld detections, more than the %d one wave's registers hold", i,
               h[i + 1] - h[i], PP_POSENMS_MAX_DETS);
  return 0;
}

}  // namespace pp

extern "C" int pp_posenms_rescore(long long M, int K, const void *kpt_scores, const void *box_scores, double kpt_thr,
                                  void *out, void *stream) {
  using namespace pp;
  PP_REQUIRE(M >= 0, "pp_posenms_rescore: M=%lld", M);
  PP_REQUIRE(K > 0, "pp_posenms_rescore: K=%d", K);
  PP_REQUIRE(kpt_thr == kpt_thr, "pp_posenms_rescore: kpt_thr is not a number");
  PP_REQUIRE(kpt_scores && box_scores && out, "pp_posenms_rescore: null argument");
  const long long blocks = (M + kNmsRescoreThreads - 1) / kNmsRescoreThreads;
  PP_REQUIRE(blocks < (1ll << 31), "pp_posenms_rescore: M=%lld detections exceed one grid", M);
  if (M == 0) return 0;
  hipLaunchKernelGGL(posenms_rescore_kernel, dim3((unsigned)blocks), dim3(kNmsRescoreThreads), 0, (hipStream_t)stream,
                     M, K, (const double *)kpt_scores, (const double *)box_scores, kpt_thr, (double *)out);
  PP_CHECK_LAUNCH("posenms_rescore_kernel");
  return 0;
}

extern "C" int pp_posenms(int n_img, int K, long long Dtot, const long long *host_off, const void *off,
                          const void *kpts, const void *vis, const void *area, const void *scores, const void *vars,
                          int mode, double oks_thr, double vis_thr, int max_dets, void *out_scores, void *keep,
                          void *counts, void *stream) {
  using namespace pp;
  PP_REQUIRE(K > 0, "pp_posenms: K=%d", K);
  PP_REQUIRE(oks_thr > 0.0 && oks_thr <= 1.0, "pp_posenms: oks_thr=%g is outside (0, 1]", oks_thr);
  PP_REQUIRE(mode == PP_POSENMS_HARD || mode == PP_POSENMS_SOFT_GAUSSIAN || mode == PP_POSENMS_SOFT_LINEAR,
             "pp_posenms: unknown mode %d", mode);
  PP_REQUIRE(max_dets > 0, "pp_posenms: max_dets=%d", max_dets);
  PP_REQUIRE(!vis || vis_thr == vis_thr, "pp_posenms: vis_thr is not a number");
  PP_REQUIRE(off && kpts && area && scores && vars && out_scores && keep && counts, "pp_posenms: null argument");
  if (int rc = nms_check_offsets(n_img, host_off, Dtot)) return rc;
  if (n_img == 0 || Dtot == 0) return 0;
  const unsigned blocks = (unsigned)((n_img + kNmsWaves - 1) / kNmsWaves);
  hipLaunchKernelGGL(posenms_kernel, dim3(blocks), dim3(64 * kNmsWaves), 0, (hipStream_t)stream, n_img, K,
                     (const long long *)off, (const double *)kpts, (const double *)vis, (const double *)area,
                     (const double *)scores, (const double *)vars, mode, oks_thr, vis_thr, max_dets,
                     (double *)out_scores, (unsigned char *)keep, (int *)counts);
  PP_CHECK_LAUNCH("posenms_kernel");
  return 0;
}
