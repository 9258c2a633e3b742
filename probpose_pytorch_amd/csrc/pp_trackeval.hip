// PoseTrackEval: CLEAR-MOT and identity (IDF1) metrics of tracked poses on the device (probpose_pytorch_amd/
// trackeval.py; the rule: include/probpose_hip.h, tests/trackeval_reference.py).  The similarity is
// pp_cocoeval_oks with the frames of all sequences as its images; the three launches here read its matrices.
//
// A batch is described by two offset tables, each given twice (a HOST copy that is checked before any launch and the
// DEVICE copy the kernels read):
//   offs  [3, n_frames + 1] int64   pp_cocoeval_oks's own table: prediction, ground-truth and OKS offsets per frame;
//                                   frame f's matrix is D_f x G_f row-major, s[g][d] = oks[oks_off[f] + d * G_f + g]
//   seq   [4, n_seq + 1]    int64   frame_off (sequence s owns frames frame_off[s] .. frame_off[s+1], in time order) |
//                                   gid_off (running sum of its ground-truth identities NG_s) | pid_off (of its
//                                   predicted identities NP_s) | c_off (running sum of NG_s * NP_s)
// gt_idx [Gtot] / pred_idx [Dtot] int32 are the dense identity indices within the sequence.
//
//   sap_solve                   the shortest-augmenting-path solver of §4.7f lives in pp_assoc.h: a device template over
//                               the number of columns NC a lane owns (lane j % 64 owns column j) and over how the
//                               weights of a row are fetched.  The three solver kernels here differ in their fetch
//                               alone.  (pp_track.hip's kernel keeps the loop written out: see the header.)
//   trackeval_clear_kernel      one wave per (sequence, threshold), four waves to a workgroup; the frames in order,
//                               sap_solve<4> per frame with the weights formed on the fly from the OKS column and the
//                               row's `prev`.  last / prev / matched / runs per ground-truth identity live in a global
//                               workspace this wave alone owns; the rows of a frame are distinct identities, so every
//                               element has one writer.  prev carries the frame it was set in: nothing is reset.  A
//                               frame's stores are fenced before the next frame reads them from other lanes.
//   trackeval_overlap_kernel    one lane per (OKS entry, threshold): atomicAdd of 1 into the int32 c[a][b] of its
//                               sequence where s >= thr.  Integer atomics: exact in any order.
//   trackeval_identity_kernel   one wave per (sequence, threshold): sap_solve on c; 4 columns per lane when both
//                               identity counts are at most 256, 16 otherwise.
// HOTA (PoseTrackEval(hota=True); the gauge: tests/hota_reference.py), on the same tables:
//   trackeval_hota_align_kernel    one wave per frame: the row and column sums of its OKS matrix, each one lane's
//                                  sequential sum; per pair floor(s / (R + C - s) * 2^32) into the int64 pmc[a][b]
//   trackeval_hota_weights_kernel  one lane per OKS entry: q = 1 + floor(A s 2^32), written transposed (G x D), so
//                                  that the one fp64 division per pair is paid once and the solver's fetch is a load
//   trackeval_hota_match_kernel    one wave per frame: sap_solve<4> on q, one matching for all alphas; per alpha the
//                                  frame's own TP and OKS sum (no atomics) and mc[a][b] += 1 (int32 atomics)
//   trackeval_hota_assoc_kernel    one wave per (sequence, alpha): the frames' records added, the association sums
// No float atomics, no LDS, no barrier; every result is the same on every call.
#include <limits.h>
#include <math.h>

#include "pp_assoc.h"

namespace pp {

constexpr int kTevWaves = 4;
constexpr int kTevThreads = 64 * kTevWaves;
constexpr long long kTevBonus = 1ll << 42;                // what a continued pair's weight gains
constexpr double kTwo32 = 4294967296.0;

// q of a pair without the continuation bonus: 0 = inadmissible (a NaN is)
__device__ __forceinline__ long long tev_weight(double s, double thr) {
  if (!(s >= thr)) return 0;
  return 1 + (long long)floor(fmin(s - thr, 1.0) * kTwo32);
}

// the rows of the sequence table
struct TevSeq {
  long long f0, f1, a0, NG, NP, c0;
};
__device__ __forceinline__ TevSeq tev_seq(const long long *seq, int n_seq, long long s) {
  const long long *fo = seq, *go = seq + (n_seq + 1), *po = seq + 2ll * (n_seq + 1), *co = seq + 3ll * (n_seq + 1);
  return TevSeq{fo[s], fo[s + 1], go[s], go[s + 1] - go[s], po[s + 1] - po[s], co[s]};
}

// a frame's extents in pp_cocoeval_oks's table; ok = false: refused on the host
struct TevFrame {
  long long d0, g0, o0;
  int D, G;
  bool ok;
};
__device__ __forceinline__ TevFrame tev_frame(const long long *offs, int n_frames, long long f) {
  const long long d0 = offs[f], Dl = offs[f + 1] - d0;
  const long long g0 = offs[n_frames + 1 + f], Gl = offs[n_frames + 2 + f] - g0;
  const bool ok = Dl >= 0 && Gl >= 0 && Dl <= PP_TRACKEVAL_MAX_FRAME && Gl <= PP_TRACKEVAL_MAX_FRAME;
  return TevFrame{d0, g0, offs[2ll * n_frames + 2 + f], (int)Dl, (int)Gl, ok};
}

constexpr int kClearCols = PP_TRACKEVAL_MAX_FRAME / 64;   // columns a lane owns in a frame

__global__ __launch_bounds__(kTevThreads) void trackeval_clear_kernel(
    int n_seq, int n_thr, int n_frames, long long n_gid, const long long *__restrict__ offs,
    const long long *__restrict__ seq, const double *__restrict__ thr, const double *__restrict__ oks,
    const int *__restrict__ gt_idx, const int *__restrict__ pred_idx, int *last, long long *prev, int *matched,
    int *runs, long long *__restrict__ rec, double *__restrict__ oks_sum) {
  const long long w = (long long)blockIdx.x * kTevWaves + (threadIdx.x >> 6);
  if (w >= (long long)n_seq * n_thr) return;
  const int lane = threadIdx.x & 63;
  const long long s = w / n_thr;
  const int t = (int)(w - s * n_thr);
  const TevSeq q = tev_seq(seq, n_seq, s);
  if (q.f0 < 0 || q.f1 < q.f0 || q.f1 > n_frames || q.NG < 0 || q.NG > PP_TRACKEVAL_MAX_IDS || q.a0 < 0 ||
      q.a0 + q.NG > n_gid)
    return;                                               // refused on the host
  const int NG = (int)q.NG;
  const double th = thr[t];
  const long long base = (long long)t * n_gid + q.a0;     // this wave's slice of the per-identity workspace
  // last: the predicted identity + 1 (0 = none); prev: (frame tag << 32) | predicted identity, tag 0 = never
  for (int a = lane; a < NG; a += 64) {
    last[base + a] = 0;
    prev[base + a] = 0;
    matched[base + a] = 0;
    runs[base + a] = 0;
  }
  __threadfence();
  long long tp = 0, idsw = 0, n_gt = 0, n_pr = 0;
  double sum = 0.0;
  for (long long f = q.f0; f < q.f1; ++f) {
    const TevFrame fr = tev_frame(offs, n_frames, f);
    if (!fr.ok) return;                                   // refused on the host
    const long long d0 = fr.d0, g0 = fr.g0;
    const int D = fr.D, G = fr.G;
    n_gt += G;
    n_pr += D;
    if (G == 0 || D == 0) continue;                       // nothing can match
    const long long tag = f - q.f0 + 2;                   // tag - 1 >= 1: the frame before, never the "never" tag

    // lane-owned: the prev of row r * 64 + lane (-1: none) and the predicted identity of column s * 64 + lane
    int prow[kClearCols], pcol[kClearCols];
#pragma unroll
    for (int r = 0; r < kClearCols; ++r) {
      const int i = r * 64 + lane;
      prow[r] = pcol[r] = -1;
      if (i < G) {
        const int a = gt_idx[g0 + i];
        if (a >= 0 && a < NG) {
          const long long pk = prev[base + a];
          if ((pk >> 32) == tag - 1) prow[r] = (int)(pk & 0xffffffffll);
        }
      }
      if (i < D) pcol[r] = pred_idx[d0 + i];
    }
    const double *mat = oks + fr.o0;
    const auto fetch = [&](int i0, long long (&wq)[kClearCols]) {
      const int pv = sap_fetch<kClearCols>(prow, i0);
#pragma unroll
      for (int c = 0; c < kClearCols; ++c) {
        const int j = c * 64 + lane;
        long long x = 0;
        if (j < D) {
          x = tev_weight(mat[(long long)j * G + i0], th);
          if (x > 0 && pv >= 0 && pcol[c] == pv) x += kTevBonus;
        }
        wq[c] = x;
      }
    };
    int held[kClearCols];
    sap_solve<kClearCols>(lane, G, G > D ? G : D, fetch, held);

    // a held row is matched if its column is real and the pair admissible; written by the column's lane
#pragma unroll
    for (int c = 0; c < kClearCols; ++c) {
      const int j = c * 64 + lane;
      if (j < D && held[c] >= 0 && held[c] < G) {
        const double x = mat[(long long)j * G + held[c]];
        if (tev_weight(x, th) > 0) {
          ++tp;
          sum += x;
          const int a = gt_idx[g0 + held[c]], p = pcol[c];
          if (a >= 0 && a < NG) {
            const int was = last[base + a];
            if (was != 0 && was != p + 1) ++idsw;
            last[base + a] = p + 1;
            if ((prev[base + a] >> 32) != tag - 1) runs[base + a] += 1;
            matched[base + a] += 1;
            prev[base + a] = (tag << 32) | (long long)(unsigned)p;
          }
        }
      }
    }
    __threadfence();                                      // the next frame reads these from other lanes
  }
  tp = wave_sum_i64(tp);
  idsw = wave_sum_i64(idsw);
  sum = wave_sum(sum);
  if (lane == 0) {
    rec[4 * w] = tp;
    rec[4 * w + 1] = n_gt - tp;
    rec[4 * w + 2] = n_pr - tp;
    rec[4 * w + 3] = idsw;
    oks_sum[w] = sum;
  }
}

// the last index i of a[0 .. n] (ascending, a[0] <= x < a[n]) with a[i] <= x
__device__ __forceinline__ long long tev_owner(const long long *a, long long n, long long x) {
  long long lo = 0, hi = n;
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if (a[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kTevThreads) void trackeval_overlap_kernel(
    int n_seq, int n_thr, int n_frames, long long oks_total, long long c_total, const long long *__restrict__ offs,
    const long long *__restrict__ seq, const double *__restrict__ thr, const double *__restrict__ oks,
    const int *__restrict__ gt_idx, const int *__restrict__ pred_idx, int *c) {
  const long long i = (long long)blockIdx.x * kTevThreads + threadIdx.x;
  if (i >= oks_total * n_thr) return;
  const long long e = i / n_thr;
  const int t = (int)(i - e * n_thr);
  if (!(oks[e] >= thr[t])) return;
  const long long f = tev_owner(offs + 2ll * (n_frames + 1), n_frames, e);
  const long long d0 = offs[f], D = offs[f + 1] - d0;
  const long long g0 = offs[n_frames + 1 + f], G = offs[n_frames + 2 + f] - g0;
  const long long r = e - offs[2ll * n_frames + 2 + f];
  if (G <= 0 || r < 0 || r >= D * G) return;              // refused on the host
  const long long d = r / G, g = r - d * G;
  const TevSeq q = tev_seq(seq, n_seq, tev_owner(seq, n_seq, f));
  const long long a = gt_idx[g0 + g], b = pred_idx[d0 + d];
  if (a < 0 || a >= q.NG || b < 0 || b >= q.NP) return;
  const long long at = q.c0 + a * q.NP + b;
  if (at < 0 || at >= c_total) return;
  atomicAdd(&c[(long long)t * c_total + at], 1);
}

template <int NC>
__device__ __forceinline__ long long tev_identity(int lane, int NG, int NP, const int *__restrict__ c) {
  const auto fetch = [&](int i0, long long (&wq)[NC]) {
#pragma unroll
    for (int s = 0; s < NC; ++s) {
      const int j = s * 64 + lane;
      wq[s] = j < NP ? (long long)c[(long long)i0 * NP + j] : 0;
    }
  };
  int held[NC];
  sap_solve<NC>(lane, NG, NG > NP ? NG : NP, fetch, held);
  long long sum = 0;
#pragma unroll
  for (int s = 0; s < NC; ++s) {
    const int j = s * 64 + lane;
    if (j < NP && held[s] >= 0 && held[s] < NG) sum += c[(long long)held[s] * NP + j];
  }
  return wave_sum_i64(sum);
}

constexpr int kIdentityCols = PP_TRACKEVAL_MAX_IDS / 64;  // columns a lane owns in the wide form

__global__ __launch_bounds__(kTevThreads) void trackeval_identity_kernel(
    int n_seq, int n_thr, long long c_total, const long long *__restrict__ seq, const int *__restrict__ c,
    long long *__restrict__ idtp) {
  const long long w = (long long)blockIdx.x * kTevWaves + (threadIdx.x >> 6);
  if (w >= (long long)n_seq * n_thr) return;
  const int lane = threadIdx.x & 63;
  const long long s = w / n_thr, t = w - s * n_thr;
  const TevSeq q = tev_seq(seq, n_seq, s);
  if (q.NG < 0 || q.NP < 0 || q.NG > PP_TRACKEVAL_MAX_IDS || q.NP > PP_TRACKEVAL_MAX_IDS || q.c0 < 0 ||
      q.c0 + q.NG * q.NP > c_total)
    return;                                               // refused on the host
  const int NG = (int)q.NG, NP = (int)q.NP;
  const int *mine = c + t * c_total + q.c0;
  long long total = 0;
  if (NG > 0 && NP > 0) {                                 // wave-uniform
    if (NG <= PP_TRACKEVAL_MAX_FRAME && NP <= PP_TRACKEVAL_MAX_FRAME) total = tev_identity<kClearCols>(lane, NG, NP, mine);
    else total = tev_identity<kIdentityCols>(lane, NG, NP, mine);
  }
  if (lane == 0) idtp[w] = total;
}

// ---- HOTA (the rule: include/probpose_hip.h, tests/hota_reference.py) ---------------------------------
// an OKS as the HOTA rule reads it: what is not > 0 (a NaN is not) counts as 0
__device__ __forceinline__ double hota_s(double s) { return s > 0.0 ? s : 0.0; }

// where the identities (a, b) of sequence q sit in a [c_total] array, or -1: an index out of range is passed over
__device__ __forceinline__ long long hota_at(const TevSeq &q, long long c_total, long long a, long long b) {
  if (a < 0 || a >= q.NG || b < 0 || b >= q.NP) return -1;
  const long long at = q.c0 + a * q.NP + b;
  return at >= 0 && at < c_total ? at : -1;
}

// Launch 1, one wave per frame: R_g and C_d, each one lane's sequential sum in ascending index; then pmc[a][b] +=
// floor(s / ((R_g + C_d) - s) * 2^32) for every pair with s > 0.  Lane g % 64 owns row g, lane d % 64 column d.
__global__ __launch_bounds__(kTevThreads) void trackeval_hota_align_kernel(
    int n_seq, int n_frames, long long c_total, const long long *__restrict__ offs, const long long *__restrict__ seq,
    const double *__restrict__ oks, const int *__restrict__ gt_idx, const int *__restrict__ pred_idx,
    unsigned long long *pmc) {
  const long long f = (long long)blockIdx.x * kTevWaves + (threadIdx.x >> 6);
  if (f >= n_frames) return;
  const int lane = threadIdx.x & 63;
  const TevFrame fr = tev_frame(offs, n_frames, f);
  if (!fr.ok || fr.G == 0 || fr.D == 0) return;
  const TevSeq q = tev_seq(seq, n_seq, tev_owner(seq, n_seq, f));
  const int D = fr.D, G = fr.G;
  const double *mat = oks + fr.o0;
  double R[kClearCols], C[kClearCols];
  int arow[kClearCols];
#pragma unroll
  for (int r = 0; r < kClearCols; ++r) {
    const int i = r * 64 + lane;
    R[r] = C[r] = 0.0;
    arow[r] = -1;
    if (i < G) {
      arow[r] = gt_idx[fr.g0 + i];
      for (int d = 0; d < D; ++d) R[r] += hota_s(mat[(long long)d * G + i]);
    }
    if (i < D)
      for (int g = 0; g < G; ++g) C[r] += hota_s(mat[(long long)i * G + g]);
  }
  for (int d = 0; d < D; ++d) {                           // wave-uniform: the rows of one column are one coalesced load
    const double Cd = sap_fetch<kClearCols>(C, d);
    const long long b = pred_idx[fr.d0 + d];
#pragma unroll
    for (int r = 0; r < kClearCols; ++r) {
      const int g = r * 64 + lane;
      if (g >= G) continue;
      const double s = mat[(long long)d * G + g];
      if (!(s > 0.0)) continue;
      const long long at = hota_at(q, c_total, arow[r], b);
      if (at < 0) continue;
      const double x = s / ((R[r] + Cd) - s);             // <= 1: both sums hold s
      atomicAdd(&pmc[at], (unsigned long long)(long long)floor(x * kTwo32));
    }
  }
}

// Launch 2, one lane per OKS entry: q[g][d] = 0 unless s > 0, else 1 + floor((A s) 2^32) with A = pmc / (2^32 (ng +
// np) - pmc).  q is written G x D row-major, so that the solver's row fetch is one coalesced load.
__global__ __launch_bounds__(kTevThreads) void trackeval_hota_weights_kernel(
    int n_seq, int n_frames, long long oks_total, long long c_total, const long long *__restrict__ offs,
    const long long *__restrict__ seq, const double *__restrict__ oks, const int *__restrict__ gt_idx,
    const int *__restrict__ pred_idx, const long long *__restrict__ pmc, const long long *__restrict__ gt_present,
    const long long *__restrict__ pred_present, long long *__restrict__ qw) {
  const long long e = (long long)blockIdx.x * kTevThreads + threadIdx.x;
  if (e >= oks_total) return;
  const long long f = tev_owner(offs + 2ll * (n_frames + 1), n_frames, e);
  const TevFrame fr = tev_frame(offs, n_frames, f);
  const long long r = e - fr.o0;
  if (!fr.ok || fr.G == 0 || r < 0 || r >= (long long)fr.D * fr.G) return;      // refused on the host
  const long long d = r / fr.G, g = r - d * fr.G;
  const double s = oks[e];
  long long w = 0;
  if (s > 0.0) {
    const long long sq = tev_owner(seq, n_seq, f);
    const TevSeq q = tev_seq(seq, n_seq, sq);
    const long long a = gt_idx[fr.g0 + g], b = pred_idx[fr.d0 + d];
    const long long at = hota_at(q, c_total, a, b);
    if (at >= 0) {
      const long long p = pmc[at];
      const long long den = ((gt_present[q.a0 + a] + pred_present[seq[2ll * (n_seq + 1) + sq] + b]) << 32) - p;
      const double A = den > 0 ? (double)p / (double)den : 0.0;
      w = 1 + (long long)floor((A * s) * kTwo32);
    }
  }
  qw[fr.o0 + g * fr.D + d] = w;
}

// Launch 3, one wave per frame: sap_solve<4> on q, then per alpha the counted pairs.  held_row [Dtot]: the row every
// prediction is matched to, or -1.  ftp / floc [n_frames, n_alpha]: the frame's own record, per-lane sums in ascending
// columns and one butterfly.  mc[i][a][b] += 1 by an integer atomic.
__global__ __launch_bounds__(kTevThreads) void trackeval_hota_match_kernel(
    int n_seq, int n_alpha, int n_frames, long long c_total, const long long *__restrict__ offs,
    const long long *__restrict__ seq, const double *__restrict__ alpha, const double *__restrict__ oks,
    const long long *__restrict__ qw, const int *__restrict__ gt_idx, const int *__restrict__ pred_idx, int *mc,
    int *__restrict__ held_row, long long *__restrict__ ftp, double *__restrict__ floc) {
  const long long f = (long long)blockIdx.x * kTevWaves + (threadIdx.x >> 6);
  if (f >= n_frames) return;
  const int lane = threadIdx.x & 63;
  const TevFrame fr = tev_frame(offs, n_frames, f);
  if (!fr.ok) return;                                     // refused on the host
  const int D = fr.D, G = fr.G;
  double sp[kClearCols];                                  // the OKS of the lane's matched pairs, 0 = none
  long long at[kClearCols];
#pragma unroll
  for (int c = 0; c < kClearCols; ++c) {
    sp[c] = 0.0;
    at[c] = -1;
  }
  if (G > 0 && D > 0) {                                   // wave-uniform
    const TevSeq q = tev_seq(seq, n_seq, tev_owner(seq, n_seq, f));
    const double *mat = oks + fr.o0;
    const long long *qm = qw + fr.o0;
    const auto fetch = [&](int i0, long long (&wq)[kClearCols]) {
#pragma unroll
      for (int c = 0; c < kClearCols; ++c) {
        const int j = c * 64 + lane;
        wq[c] = j < D ? qm[(long long)i0 * D + j] : 0;
      }
    };
    int held[kClearCols];
    sap_solve<kClearCols>(lane, G, G > D ? G : D, fetch, held);
#pragma unroll
    for (int c = 0; c < kClearCols; ++c) {
      const int j = c * 64 + lane;
      if (j >= D) continue;
      int h = -1;
      if (held[c] >= 0 && held[c] < G && qm[(long long)held[c] * D + j] > 0) {
        h = held[c];
        sp[c] = mat[(long long)j * G + h];
        at[c] = hota_at(q, c_total, gt_idx[fr.g0 + h], pred_idx[fr.d0 + j]);
      }
      held_row[fr.d0 + j] = h;
    }
  } else {
    for (int j = lane; j < D; j += 64) held_row[fr.d0 + j] = -1;
  }
  for (int i = 0; i < n_alpha; ++i) {
    const double al = alpha[i];
    long long tp = 0;
    double loc = 0.0;
#pragma unroll
    for (int c = 0; c < kClearCols; ++c)
      if (sp[c] > 0.0 && sp[c] >= al) {
        ++tp;
        loc += sp[c];
        if (at[c] >= 0) atomicAdd(&mc[(long long)i * c_total + at[c]], 1);
      }
    tp = wave_sum_i64(tp);
    loc = wave_sum(loc);
    if (lane == 0) {
      ftp[f * n_alpha + i] = tp;
      floc[f * n_alpha + i] = loc;
    }
  }
}

// Launch 4, one wave per (sequence, alpha): the frames' records added up, and the association sums over the NG x NP
// entries of mc.  Every sum: each lane a fixed stride, ascending, then one butterfly.
__global__ __launch_bounds__(kTevThreads) void trackeval_hota_assoc_kernel(
    int n_seq, int n_alpha, int n_frames, long long c_total, const long long *__restrict__ seq,
    const int *__restrict__ mc, const long long *__restrict__ gt_present, const long long *__restrict__ pred_present,
    const long long *__restrict__ ftp, const double *__restrict__ floc, long long *__restrict__ tp_out,
    double *__restrict__ sums) {
  const long long w = (long long)blockIdx.x * kTevWaves + (threadIdx.x >> 6);
  if (w >= (long long)n_seq * n_alpha) return;
  const int lane = threadIdx.x & 63;
  const long long s = w / n_alpha, i = w - s * n_alpha;
  const TevSeq q = tev_seq(seq, n_seq, s);
  if (q.f0 < 0 || q.f1 < q.f0 || q.f1 > n_frames || q.NG < 0 || q.NP < 0 || q.NG > PP_TRACKEVAL_MAX_IDS ||
      q.NP > PP_TRACKEVAL_MAX_IDS || q.c0 < 0 || q.c0 + q.NG * q.NP > c_total)
    return;                                               // refused on the host
  long long tp = 0;
  double loc = 0.0, assa = 0.0, assre = 0.0, asspr = 0.0;
  for (long long f = q.f0 + lane; f < q.f1; f += 64) {
    tp += ftp[f * n_alpha + i];
    loc += floc[f * n_alpha + i];
  }
  const int *mine = mc + i * c_total + q.c0;
  const long long *ng = gt_present + q.a0, *np = pred_present + seq[2ll * (n_seq + 1) + s];
  const long long n = q.NG * q.NP;
  for (long long e = lane; e < n; e += 64) {
    const long long m = mine[e];
    if (m <= 0) continue;
    const long long a = e / q.NP, b = e - a * q.NP;
    const double mm = (double)(m * m);
    const long long either = ng[a] + np[b] - m;
    if (either > 0) assa += mm / (double)either;
    if (ng[a] > 0) assre += mm / (double)ng[a];
    if (np[b] > 0) asspr += mm / (double)np[b];
  }
  tp = wave_sum_i64(tp);
  loc = wave_sum(loc);
  assa = wave_sum(assa);
  assre = wave_sum(assre);
  asspr = wave_sum(asspr);
  if (lane == 0) {
    tp_out[w] = tp;
    sums[4 * w] = loc;
    sums[4 * w + 1] = assa;
    sums[4 * w + 2] = assre;
    sums[4 * w + 3] = asspr;
  }
}

// ---- host checks: everything an entry refuses, before any launch ---------------------------------------------------
static int tev_check_counts(const char *who, int n_seq, int n_thr) {
  PP_REQUIRE(n_seq >= 0, "%s: n_seq=%d", who, n_seq);
  PP_REQUIRE(n_thr >= 1, "%s: n_thr=%d", who, n_thr);
  return 0;
}

static int tev_check_thr(const char *who, int n_thr, const double *h) {
  PP_REQUIRE(h, "%s: null host thresholds", who);
  for (int i = 0; i < n_thr; ++i)                         // written so that a NaN fails it
    PP_REQUIRE(h[i] > 0.0 && h[i] <= 1.0, "%s: threshold %d = %g is outside (0, 1]", who, i, h[i]);
  return 0;
}

// the host copy of the sequence table; n_frames < 0: the caller has no frames to hold it against
static int tev_check_seq(const char *who, int n_seq, const long long *h, long long n_frames, long long n_gid,
                         long long c_total) {
  PP_REQUIRE(h, "%s: null host sequence table", who);
  const long long *fo = h, *go = h + (n_seq + 1), *po = h + 2ll * (n_seq + 1), *co = h + 3ll * (n_seq + 1);
  PP_REQUIRE(fo[0] == 0 && go[0] == 0 && po[0] == 0 && co[0] == 0,
             "%s: sequence offsets do not start at 0 (frames %lld, gt ids %lld, pred ids %lld, c %lld)", who, fo[0],
             go[0], po[0], co[0]);
  for (int i = 0; i < n_seq; ++i) {
    PP_REQUIRE(fo[i + 1] >= fo[i], "%s: frame offsets are not monotone at sequence %d (%lld after %lld)", who, i,
               fo[i + 1], fo[i]);
    const long long ng = go[i + 1] - go[i], np = po[i + 1] - po[i];
    PP_REQUIRE(ng >= 0 && np >= 0, "%s: identity offsets are not monotone at sequence %d", who, i);
    PP_REQUIRE(ng <= PP_TRACKEVAL_MAX_IDS && np <= PP_TRACKEVAL_MAX_IDS,
               "%s: sequence %d has %lld ground-truth and %lld predicted identities, more than "
               "PP_TRACKEVAL_MAX_IDS = %d", who, i, ng, np, PP_TRACKEVAL_MAX_IDS);
    PP_REQUIRE(co[i + 1] - co[i] == ng * np, "%s: c offsets of sequence %d span %lld entries, expected %lld x %lld",
               who, i, co[i + 1] - co[i], ng, np);
  }
  PP_REQUIRE(n_frames < 0 || fo[n_seq] == n_frames, "%s: frame offsets end at %lld, there are %lld frames", who,
             fo[n_seq], n_frames);
  PP_REQUIRE(n_gid < 0 || go[n_seq] == n_gid, "%s: ground-truth identity offsets end at %lld, the workspace holds %lld",
             who, go[n_seq], n_gid);
  PP_REQUIRE(co[n_seq] == c_total, "%s: c offsets end at %lld, c holds %lld per threshold", who, co[n_seq], c_total);
  return 0;
}

// the host copy of pp_cocoeval_oks's table, and the frame limit
static int tev_check_frames(const char *who, int n_frames, const long long *h, long long Dtot, long long Gtot,
                            long long oks_total) {
  PP_REQUIRE(n_frames >= 0, "%s: n_frames=%d", who, n_frames);
  PP_REQUIRE(h, "%s: null host offsets", who);
  const long long *d = h, *g = h + n_frames + 1, *o = h + 2ll * (n_frames + 1);
  PP_REQUIRE(d[0] == 0 && g[0] == 0 && o[0] == 0, "%s: offsets do not start at 0 (pred %lld, gt %lld, oks %lld)", who,
             d[0], g[0], o[0]);
  for (int i = 0; i < n_frames; ++i) {
    const long long D = d[i + 1] - d[i], G = g[i + 1] - g[i];
    PP_REQUIRE(D >= 0 && G >= 0, "%s: offsets are not monotone at frame %d", who, i);
    PP_REQUIRE(D <= PP_TRACKEVAL_MAX_FRAME && G <= PP_TRACKEVAL_MAX_FRAME,
               "%s: frame %d has %lld ground truths and %lld predictions, more than PP_TRACKEVAL_MAX_FRAME = %d", who,
               i, G, D, PP_TRACKEVAL_MAX_FRAME);
    PP_REQUIRE(o[i + 1] - o[i] == D * G, "%s: OKS offsets of frame %d span %lld entries, expected D x G = %lld x %lld",
               who, i, o[i + 1] - o[i], D, G);
  }
  PP_REQUIRE(d[n_frames] == Dtot && g[n_frames] == Gtot && o[n_frames] == oks_total,
             "%s: offsets end at (pred %lld, gt %lld, oks %lld), the arrays hold (%lld, %lld, %lld)", who, d[n_frames],
             g[n_frames], o[n_frames], Dtot, Gtot, oks_total);
  return 0;
}

static int tev_check_alphas(const char *who, int n_alpha, const double *h) {
  PP_REQUIRE(n_alpha >= 1 && n_alpha <= PP_TRACKEVAL_HOTA_MAX_ALPHAS, "%s: n_alpha=%d is outside [1, %d]", who, n_alpha,
             PP_TRACKEVAL_HOTA_MAX_ALPHAS);
  if (!h) return 0;                                       // the entry reads no alpha
  for (int i = 0; i < n_alpha; ++i)                       // written so that a NaN fails it
    PP_REQUIRE(h[i] > 0.0 && h[i] <= 1.0, "%s: alpha %d = %g is outside (0, 1]", who, i, h[i]);
  return 0;
}

// the sequence table of a HOTA entry: tev_check_seq, the predicted identities' total, the frames a sequence may have
static int tev_check_hota_seq(const char *who, int n_seq, const long long *h, long long n_frames, long long n_gid,
                              long long n_pid, long long c_total) {
  PP_REQUIRE(n_seq >= 0, "%s: n_seq=%d", who, n_seq);
  PP_REQUIRE(c_total >= 0, "%s: c_total=%lld", who, c_total);
  if (int rc = tev_check_seq(who, n_seq, h, n_frames, n_gid, c_total)) return rc;
  const long long *fo = h, *po = h + 2ll * (n_seq + 1);
  PP_REQUIRE(n_pid < 0 || po[n_seq] == n_pid, "%s: predicted identity offsets end at %lld, the table holds %lld", who,
             po[n_seq], n_pid);
  for (int i = 0; i < n_seq; ++i)
    PP_REQUIRE(fo[i + 1] - fo[i] <= PP_TRACKEVAL_HOTA_MAX_FRAMES,
               "%s: sequence %d has %lld frames, more than PP_TRACKEVAL_HOTA_MAX_FRAMES = %d", who, i,
               fo[i + 1] - fo[i], PP_TRACKEVAL_HOTA_MAX_FRAMES);
  return 0;
}

static int tev_frame_grid(const char *who, int n_frames, long long *grid) {
  *grid = ((long long)n_frames + kTevWaves - 1) / kTevWaves;
  PP_REQUIRE(*grid < (1ll << 31), "%s: %d frames exceed one grid", who, n_frames);
  return 0;
}

}  // namespace pp

extern "C" int pp_trackeval_hota_align(int n_seq, int n_frames, long long Dtot, long long Gtot, long long oks_total,
                                       long long c_total, const long long *host_offs, const long long *host_seq,
                                       const void *offs, const void *seq, const void *oks, const void *gt_idx,
                                       const void *pred_idx, void *pmc, void *stream) {
  using namespace pp;
  const char *who = "pp_trackeval_hota_align";
  PP_REQUIRE(n_seq >= 0, "%s: n_seq=%d", who, n_seq);
  PP_REQUIRE(offs && seq && oks && gt_idx && pred_idx && pmc, "%s: null argument", who);
  if (int rc = tev_check_frames(who, n_frames, host_offs, Dtot, Gtot, oks_total)) return rc;
  if (int rc = tev_check_hota_seq(who, n_seq, host_seq, n_frames, -1, -1, c_total)) return rc;
  if (n_seq == 0 || oks_total == 0) return 0;
  long long grid;
  if (int rc = tev_frame_grid(who, n_frames, &grid)) return rc;
  hipLaunchKernelGGL(trackeval_hota_align_kernel, dim3((unsigned)grid), dim3(kTevThreads), 0, (hipStream_t)stream, n_seq,
                     n_frames, c_total, (const long long *)offs, (const long long *)seq, (const double *)oks,
                     (const int *)gt_idx, (const int *)pred_idx, (unsigned long long *)pmc);
  PP_CHECK_LAUNCH("trackeval_hota_align_kernel");
  return 0;
}

extern "C" int pp_trackeval_hota_weights(int n_seq, int n_frames, long long Dtot, long long Gtot, long long oks_total,
                                         long long c_total, long long n_gid, long long n_pid,
                                         const long long *host_offs, const long long *host_seq, const void *offs,
                                         const void *seq, const void *oks, const void *gt_idx, const void *pred_idx,
                                         const void *pmc, const void *gt_present, const void *pred_present, void *q,
                                         void *stream) {
  using namespace pp;
  const char *who = "pp_trackeval_hota_weights";
  PP_REQUIRE(n_seq >= 0, "%s: n_seq=%d", who, n_seq);
  PP_REQUIRE(n_gid >= 0 && n_pid >= 0, "%s: n_gid=%lld, n_pid=%lld", who, n_gid, n_pid);
  PP_REQUIRE(offs && seq && oks && gt_idx && pred_idx && pmc && gt_present && pred_present && q, "%s: null argument",
             who);
  if (int rc = tev_check_frames(who, n_frames, host_offs, Dtot, Gtot, oks_total)) return rc;
  if (int rc = tev_check_hota_seq(who, n_seq, host_seq, n_frames, n_gid, n_pid, c_total)) return rc;
  if (n_seq == 0 || oks_total == 0) return 0;
  const long long grid = (oks_total + kTevThreads - 1) / kTevThreads;
  PP_REQUIRE(grid < (1ll << 31), "%s: %lld OKS entries exceed one grid", who, oks_total);
  hipLaunchKernelGGL(trackeval_hota_weights_kernel, dim3((unsigned)grid), dim3(kTevThreads), 0, (hipStream_t)stream,
                     n_seq, n_frames, oks_total, c_total, (const long long *)offs, (const long long *)seq,
                     (const double *)oks, (const int *)gt_idx, (const int *)pred_idx, (const long long *)pmc,
                     (const long long *)gt_present, (const long long *)pred_present, (long long *)q);
  PP_CHECK_LAUNCH("trackeval_hota_weights_kernel");
  return 0;
}

extern "C" int pp_trackeval_hota_match(int n_seq, int n_alpha, int n_frames, long long Dtot, long long Gtot,
                                       long long oks_total, long long c_total, const long long *host_offs,
                                       const long long *host_seq, const double *host_alpha, const void *offs,
                                       const void *seq, const void *alpha, const void *oks, const void *q,
                                       const void *gt_idx, const void *pred_idx, void *mc, void *held_row,
                                       void *frame_tp, void *frame_loc, void *stream) {
  using namespace pp;
  const char *who = "pp_trackeval_hota_match";
  PP_REQUIRE(n_seq >= 0, "%s: n_seq=%d", who, n_seq);
  PP_REQUIRE(host_alpha, "%s: null host alphas", who);
  if (int rc = tev_check_alphas(who, n_alpha, host_alpha)) return rc;
  PP_REQUIRE(offs && seq && alpha && oks && q && gt_idx && pred_idx && mc && held_row && frame_tp && frame_loc,
             "%s: null argument", who);
  if (int rc = tev_check_frames(who, n_frames, host_offs, Dtot, Gtot, oks_total)) return rc;
  if (int rc = tev_check_hota_seq(who, n_seq, host_seq, n_frames, -1, -1, c_total)) return rc;
  if (n_seq == 0 || n_frames == 0) return 0;
  long long grid;
  if (int rc = tev_frame_grid(who, n_frames, &grid)) return rc;
  hipLaunchKernelGGL(trackeval_hota_match_kernel, dim3((unsigned)grid), dim3(kTevThreads), 0, (hipStream_t)stream, n_seq,
                     n_alpha, n_frames, c_total, (const long long *)offs, (const long long *)seq, (const double *)alpha,
                     (const double *)oks, (const long long *)q, (const int *)gt_idx, (const int *)pred_idx, (int *)mc,
                     (int *)held_row, (long long *)frame_tp, (double *)frame_loc);
  PP_CHECK_LAUNCH("trackeval_hota_match_kernel");
  return 0;
}

extern "C" int pp_trackeval_hota_assoc(int n_seq, int n_alpha, int n_frames, long long c_total, long long n_gid,
                                       long long n_pid, const long long *host_seq, const void *seq, const void *mc,
                                       const void *gt_present, const void *pred_present, const void *frame_tp,
                                       const void *frame_loc, void *tp, void *sums, void *stream) {
  using namespace pp;
  const char *who = "pp_trackeval_hota_assoc";
  PP_REQUIRE(n_seq >= 0, "%s: n_seq=%d", who, n_seq);
  if (int rc = tev_check_alphas(who, n_alpha, nullptr)) return rc;
  PP_REQUIRE(n_frames >= 0, "%s: n_frames=%d", who, n_frames);
  PP_REQUIRE(n_gid >= 0 && n_pid >= 0, "%s: n_gid=%lld, n_pid=%lld", who, n_gid, n_pid);
  PP_REQUIRE(seq && mc && gt_present && pred_present && frame_tp && frame_loc && tp && sums, "%s: null argument", who);
  if (int rc = tev_check_hota_seq(who, n_seq, host_seq, n_frames, n_gid, n_pid, c_total)) return rc;
  if (n_seq == 0) return 0;
  const long long grid = ((long long)n_seq * n_alpha + kTevWaves - 1) / kTevWaves;
  PP_REQUIRE(grid < (1ll << 31), "%s: %lld (sequence, alpha) pairs exceed one grid", who, (long long)n_seq * n_alpha);
  hipLaunchKernelGGL(trackeval_hota_assoc_kernel, dim3((unsigned)grid), dim3(kTevThreads), 0, (hipStream_t)stream, n_seq,
                     n_alpha, n_frames, c_total, (const long long *)seq, (const int *)mc, (const long long *)gt_present,
                     (const long long *)pred_present, (const long long *)frame_tp, (const double *)frame_loc,
                     (long long *)tp, (double *)sums);
  PP_CHECK_LAUNCH("trackeval_hota_assoc_kernel");
  return 0;
}

extern "C" int pp_trackeval_clear(int n_seq, int n_thr, int n_frames, long long Dtot, long long Gtot,
                                  long long oks_total, long long n_gid, const long long *host_offs,
                                  const long long *host_seq, const double *host_thr, const void *offs, const void *seq,
                                  const void *thr, const void *oks, const void *gt_idx, const void *pred_idx,
                                  void *last, void *prev, void *matched, void *runs, void *rec, void *oks_sum,
                                  void *stream) {
  using namespace pp;
  const char *who = "pp_trackeval_clear";
  if (int rc = tev_check_counts(who, n_seq, n_thr)) return rc;
  PP_REQUIRE(n_gid >= 0, "%s: n_gid=%lld", who, n_gid);
  PP_REQUIRE(offs && seq && thr && oks && gt_idx && pred_idx && last && prev && matched && runs && rec && oks_sum,
             "%s: null argument", who);
  if (int rc = tev_check_thr(who, n_thr, host_thr)) return rc;
  if (int rc = tev_check_frames(who, n_frames, host_offs, Dtot, Gtot, oks_total)) return rc;
  PP_REQUIRE(host_seq, "%s: null host sequence table", who);
  if (int rc = tev_check_seq(who, n_seq, host_seq, n_frames, n_gid, host_seq[4ll * (n_seq + 1) - 1])) return rc;
  if (n_seq == 0) return 0;
  const long long grid = ((long long)n_seq * n_thr + kTevWaves - 1) / kTevWaves;
  PP_REQUIRE(grid < (1ll << 31), "%s: %lld (sequence, threshold) pairs exceed one grid", who, (long long)n_seq * n_thr);
  hipLaunchKernelGGL(trackeval_clear_kernel, dim3((unsigned)grid), dim3(kTevThreads), 0, (hipStream_t)stream, n_seq,
                     n_thr, n_frames, n_gid, (const long long *)offs, (const long long *)seq, (const double *)thr,
                     (const double *)oks, (const int *)gt_idx, (const int *)pred_idx, (int *)last, (long long *)prev,
                     (int *)matched, (int *)runs, (long long *)rec, (double *)oks_sum);
  PP_CHECK_LAUNCH("trackeval_clear_kernel");
  return 0;
}

extern "C" int pp_trackeval_overlap(int n_seq, int n_thr, int n_frames, long long Dtot, long long Gtot,
                                    long long oks_total, long long c_total, const long long *host_offs,
                                    const long long *host_seq, const double *host_thr, const void *offs,
                                    const void *seq, const void *thr, const void *oks, const void *gt_idx,
                                    const void *pred_idx, void *c, void *stream) {
  using namespace pp;
  const char *who = "pp_trackeval_overlap";
  if (int rc = tev_check_counts(who, n_seq, n_thr)) return rc;
  PP_REQUIRE(c_total >= 0, "%s: c_total=%lld", who, c_total);
  PP_REQUIRE(offs && seq && thr && oks && gt_idx && pred_idx && c, "%s: null argument", who);
  if (int rc = tev_check_thr(who, n_thr, host_thr)) return rc;
  if (int rc = tev_check_frames(who, n_frames, host_offs, Dtot, Gtot, oks_total)) return rc;
  if (int rc = tev_check_seq(who, n_seq, host_seq, n_frames, -1, c_total)) return rc;
  if (n_seq == 0 || oks_total == 0) return 0;
  const long long lanes = oks_total * n_thr, grid = (lanes + kTevThreads - 1) / kTevThreads;
  PP_REQUIRE(grid < (1ll << 31), "%s: %lld (OKS entry, threshold) pairs exceed one grid", who, lanes);
  hipLaunchKernelGGL(trackeval_overlap_kernel, dim3((unsigned)grid), dim3(kTevThreads), 0, (hipStream_t)stream, n_seq,
                     n_thr, n_frames, oks_total, c_total, (const long long *)offs, (const long long *)seq,
                     (const double *)thr, (const double *)oks, (const int *)gt_idx, (const int *)pred_idx, (int *)c);
  PP_CHECK_LAUNCH("trackeval_overlap_kernel");
  return 0;
}

extern "C" int pp_trackeval_identity(int n_seq, int n_thr, long long c_total, const long long *host_seq,
                                     const void *seq, const void *c, void *idtp, void *stream) {
  using namespace pp;
  const char *who = "pp_trackeval_identity";
  if (int rc = tev_check_counts(who, n_seq, n_thr)) return rc;
  PP_REQUIRE(c_total >= 0, "%s: c_total=%lld", who, c_total);
  PP_REQUIRE(seq && c && idtp, "%s: null argument", who);
  if (int rc = tev_check_seq(who, n_seq, host_seq, -1, -1, c_total)) return rc;
  if (n_seq == 0) return 0;
  const long long grid = ((long long)n_seq * n_thr + kTevWaves - 1) / kTevWaves;
  PP_REQUIRE(grid < (1ll << 31), "%s: %lld (sequence, threshold) pairs exceed one grid", who, (long long)n_seq * n_thr);
  hipLaunchKernelGGL(trackeval_identity_kernel, dim3((unsigned)grid), dim3(kTevThreads), 0, (hipStream_t)stream, n_seq,
                     n_thr, c_total, (const long long *)seq, (const int *)c, (long long *)idtp);
  PP_CHECK_LAUNCH("trackeval_identity_kernel");
  return 0;
}
