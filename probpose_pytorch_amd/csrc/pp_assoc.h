// What the association kernels share (pp_posenms.hip, pp_track.hip, pp_trackeval.hip), each written once:
//
//   pair_oks    the pair OKS of DESIGN §4.7c, the gauges' operations in the gauges' order.  The library is compiled
//               -ffp-contract=off, which is what keeps these the gauges' bits up to exp().  pair_oks_of is the loop
//               itself, over how the second pose's coordinates are had (stored, or a track's predicted ones).
//   sap_solve   the shortest-augmenting-path solver of DESIGN §4.7f (the rule: include/probpose_hip.h,
//               tests/trackopt_reference.py): a device template over the number of columns NC a lane owns (lane j % 64
//               owns column j) and over how the weights of a row are fetched.  v, minv, way, the used bits, the held
//               row and its u are registers of the owning lane; a step is one fetch and one wave_argmin_i64.
//   sap_fetch, kSapInf, kSapRoot   its register-array shuffle and its two constants, which the tracker's loop uses too.
//
// The weights are the callers' own: track_weight (> thr, 2^40) and tev_weight (>= thr, 2^32) are different rules.
#pragma once
#include <float.h>
#include <limits.h>
#include <math.h>

#include "pp_common.h"

namespace pp {

// The pair loop: OKS of detection a (the pivot) and a second pose whose keypoint k has the coordinates b(k, 0) and
// b(k, 1); vis_a == nullptr: every keypoint counts
template <typename Second>
__device__ __forceinline__ double pair_oks_of(int K, const double *__restrict__ ka, const Second &b,
                                              const double *__restrict__ vis_a, const double *__restrict__ vis_b,
                                              double vis_thr, double area_a, double area_b,
                                              const double *__restrict__ vars) {
  const double size = (area_a + area_b) / 2.0 + DBL_EPSILON;
  double sum = 0.0;
  int n = 0;
  for (int k = 0; k < K; ++k) {
    if (vis_a && !(vis_a[k] > vis_thr && vis_b[k] > vis_thr)) continue;
    const double dx = ka[2 * k] - b(k, 0), dy = ka[2 * k + 1] - b(k, 1);
    const double e = (dx * dx + dy * dy) / vars[k] / size / 2.0;
    sum += exp(-e);
    ++n;
  }
  return n ? sum / (double)n : 0.0;
}

// OKS of detections a (the pivot) and b of one image
__device__ __forceinline__ double pair_oks(int K, const double *__restrict__ ka, const double *__restrict__ kb,
                                           const double *__restrict__ vis_a, const double *__restrict__ vis_b,
                                           double vis_thr, double area_a, double area_b,
                                           const double *__restrict__ vars) {
  return pair_oks_of(K, ka, [kb](int k, int c) { return kb[2 * k + c]; }, vis_a, vis_b, vis_thr, area_a, area_b, vars);
}

constexpr long long kSapInf = 1ll << 62;
constexpr int kSapRoot = -1;                              // the extra start column

// x[col / 64] of a lane-owned register array as lane col % 64 holds it; col is wave-uniform
template <int NC, typename V>
__device__ __forceinline__ V sap_fetch(const V (&x)[NC], int col) {
  const int s = col >> 6;
  V mine = x[0];
#pragma unroll
  for (int c = 1; c < NC; ++c)
    if (s == c) mine = x[c];
  return __shfl(mine, col & 63, 64);
}

// The assignment of largest total weight by the rule of §4.7f: rows 0 .. R-1 in order, columns 0 .. m-1 (m >= R; the
// columns the fetch gives 0 for are virtual).  fetch(i0, q) fills q[s] with the int64 weight of row i0 and the lane's
// column s * 64 + lane.  On return held[s] is the row that column holds, or -1.  Every loop bound is wave-uniform.
//
// pp_track.hip's track_assign_optimal_kernel does NOT call this: it keeps the same loop written out with its row-ahead
// load.  Calling sap_solve with a fetch that was told "this is the row's first step" gave the same results and 98
// instead of 102 VGPRs, but ran pp_track_assign_optimal 5 - 6 % slower on the MI355X (profiles/assoc_refactor_ab.txt).
// A change to the tie rule, the step bound or the walk back has to be made there too; tests/test_trackopt_gpu.py and
// tests/test_trackeval_gpu.py hold both copies to the one Python solver.
template <int NC, typename Fetch>
__device__ __forceinline__ void sap_solve(int lane, int R, int m, const Fetch &fetch, int (&held)[NC]) {
  long long v[NC], u_held[NC];                            // a row's u travels with the column that holds it
#pragma unroll
  for (int s = 0; s < NC; ++s) {
    v[s] = u_held[s] = 0;
    held[s] = -1;
  }
  for (int i = 0; i < R; ++i) {                           // one augmenting path per row
    long long minv[NC];
    int way[NC];
    unsigned used = 0;                                    // bit s: the lane's column s is on the tree
#pragma unroll
    for (int s = 0; s < NC; ++s) {
      minv[s] = kSapInf;
      way[s] = kSapRoot;
    }
    int cur = kSapRoot, i0 = i;                           // wave-uniform: the column being scanned, its row,
    long long u0 = 0, u_root = 0;                         // that row's u, and the u of row i (the root's)
    bool open = false;
    for (int step = 0; step <= m; ++step) {               // every step marks one more column: at most m + 1
      if (cur != kSapRoot && lane == (cur & 63)) used |= 1u << (cur >> 6);
      long long q[NC];
      fetch(i0, q);
      long long delta = LLONG_MAX;
      int j1 = INT_MAX;
#pragma unroll
      for (int s = 0; s < NC; ++s) {                      // ascending columns: the lowest of the lane's on equal minv
        const int j = s * 64 + lane;
        if (j < m && !((used >> s) & 1u)) {
          const long long c = -q[s] - u0 - v[s];
          if (c < minv[s]) {
            minv[s] = c;
            way[s] = cur;
          }
          if (minv[s] < delta) {
            delta = minv[s];
            j1 = j;
          }
        }
      }
      wave_argmin_i64(delta, j1);
      if (j1 == INT_MAX) break;                           // no unused column: cannot happen, rows on the tree < m
#pragma unroll
      for (int s = 0; s < NC; ++s) {
        if ((used >> s) & 1u) {
          u_held[s] += delta;
          v[s] -= delta;
        } else {
          minv[s] -= delta;
        }
      }
      u_root += delta;
      cur = j1;
      i0 = sap_fetch<NC>(held, cur);
      u0 = sap_fetch<NC>(u_held, cur);
      if (i0 < 0) {
        open = true;
        break;
      }
    }
    // walk back: every column of the path takes the row of the column before it
    for (int hop = 0; open && cur != kSapRoot && hop <= m; ++hop) {
      const int prev = sap_fetch<NC>(way, cur);
      int row_prev = i;
      long long u_prev = u_root;
      if (prev != kSapRoot) {                             // wave-uniform
        row_prev = sap_fetch<NC>(held, prev);
        u_prev = sap_fetch<NC>(u_held, prev);
      }
      if (lane == (cur & 63)) {
#pragma unroll
        for (int s = 0; s < NC; ++s)
          if (s == (cur >> 6)) {
            held[s] = row_prev;
            u_held[s] = u_prev;
          }
      }
      cur = prev;
    }
  }
}

}  // namespace pp
