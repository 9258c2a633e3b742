// PoseTracker: greedy OKS track association and One-Euro smoothing of decoded poses (probpose_pytorch_amd/tracker.py,
// DESIGN §4.7d), three launches per update.
//
//   track_oks_kernel     one lane per (detection, slot): the pair OKS of §4.7c (pp_assoc.h's pair_oks, the function
//                        posenms_kernel calls) with the slot's stored raw keypoints, area and visibilities as the
//                        second detection; a free slot writes 0.  This is the arithmetic (K exp per pair) and it is
//                        spread over the whole chip.
//   track_assign_kernel  one wave per stream, four waves to a workgroup.  Lane j % 64 OWNS slot j: its live and taken
//                        bits are bit j / 64 of two 64-bit registers of that lane (64 lanes x 64 bits =
//                        PP_TRACK_MAX_TRACKS), and its id, age, t_last and area are written by that lane alone.  The
//                        stream's detections arrive in visiting order.  A detection's pick is wave_max of the lanes' best
//                        OKS among their live, untaken slots, then wave_min of the slots that hold it (the lowest on
//                        equal OKS); whether detection p is still unmatched is bit p / 64 of a register of lane p % 64.
//                        Ageing and freeing follow, then the births, each through wave_min of the lanes' lowest free
//                        slot.  What a detection gets (id, OKS, born, slot, te) is written by the lane that owns its
//                        slot, or by lane 0 when it has none.  No atomics, no LDS, no barrier, plain vector stores: the
//                        result does not depend on timing.
//   track_assign_optimal_kernel  the same launch shape, phases and outputs with the association replaced by the
//                        assignment of largest total weight: shortest augmenting paths with potentials
//                        in int64, at most PP_TRACK_OPT_MAX rows and columns.  Lane j % 64 owns column j (at most four):
//                        its v, minv, way, used bit, the row it holds and that row's u are registers of that lane; a
//                        step is one coalesced load of the scanned row's OKS (a row's first step: loaded a row ahead)
//                        and one wave_argmin_i64.  The loop is pp_assoc.h's sap_solve statement for statement, kept
//                        written out here, in track_optimal_rows, for the row-ahead load (the header says what calling
//                        sap_solve cost; the function takes a row range, a column mask and a threshold, so that the
//                        staged kernel runs the same statements once per stage); the
//                        shuffle sap_fetch and the constants are the header's.  Ageing, births and the matched pair's
//                        stores are the greedy kernel's own functions.
//   track_oks_predicted_kernel   track_oks_kernel with the slot's pose moved to the call's time by its One-Euro speed
//                        (DESIGN §4.7i): both are track_oks_lane, the pair loop is pp_assoc.h's pair_oks_of.
//   track_assign_staged_kernel   the launch shape, layout and outputs of track_assign_kernel with the association in
//                        two stages by score and births gated by score (§4.7i).  A stage is track_greedy_rows, the
//                        greedy kernel's own walk, or track_optimal_rows, the optimal kernel's own loop on the stage's
//                        rows and column mask; ageing and births are track_age_and_bear.
//   track_filter_kernel  one lane per (detection, keypoint): reads the slot the assign kernel gave the detection, applies
//                        the One-Euro step (or initialises, or passes the raw value through) and writes the output, the
//                        filter state and the slot's raw keypoint and visibility.  A slot belongs to at most one
//                        detection of a call, so every state element has one writer.  The operations of
//                        tests/track_reference.py one for one (compiled -ffp-contract=off): the same bits.
//
// State of one stream: one block of pp_track_state_bytes(max_tracks, K) bytes, laid out by TrackState below.
#include <limits.h>
#include <math.h>

#include "pp_assoc.h"

namespace pp {

constexpr int kTrackWaves = 4;
constexpr int kTrackThreads = 256;

// the sections of a stream's block, each a multiple of 8 bytes (T = max_tracks):
//   id int64 [T] | t_last f64 [T] | area f64 [T] | kp f64 [T, K, 2] | vis f64 [T, K] | xhat f64 [T, K, 2] |
//   dxhat f64 [T, K, 2] | next_id int64 | overflow int64 | age int32 [T] | init uint8 [T, K]
struct TrackState {
  long long *id;
  double *t_last, *area, *kp, *vis, *xhat, *dxhat;
  long long *next_id, *overflow;
  int *age;
  unsigned char *init;
};

__host__ __device__ inline long long track_pad8(long long n) { return (n + 7) & ~7ll; }

__host__ __device__ inline long long track_state_bytes(long long T, long long K) {
  return 8 * (3 * T + 7 * T * K + 2) + track_pad8(4 * T) + track_pad8(T * K);
}

__device__ __forceinline__ TrackState track_state(long long base, int T, int K) {
  TrackState s;
  const long long TK = (long long)T * K;
  double *w = (double *)base;
  s.id = (long long *)w;
  s.t_last = w + T;
  s.area = w + 2ll * T;
  s.kp = w + 3ll * T;
  s.vis = s.kp + 2 * TK;
  s.xhat = s.vis + TK;
  s.dxhat = s.xhat + 2 * TK;
  s.next_id = (long long *)(s.dxhat + 2 * TK);
  s.overflow = s.next_id + 1;
  s.age = (int *)(s.overflow + 1);
  s.init = (unsigned char *)s.age + track_pad8(4ll * T);
  return s;
}

// The lane of pair i = (detection d, slot j) of both OKS kernels.  kPredict: the slot's pose is where its One-Euro
// filter expects it at time t (the two statements of track_boxes_kernel for dt, then one multiply and one add per
// coordinate), the stored raw keypoint where the filter holds nothing for it; otherwise the stored raw keypoints.
template <bool kPredict>
__device__ __forceinline__ void track_oks_lane(int K, int T, long long Dtot, const long long *__restrict__ det_stream,
                                               const long long *__restrict__ blocks, const double *__restrict__ kpts,
                                               const double *__restrict__ vis, const double *__restrict__ area,
                                               const double *__restrict__ vars, double vis_thr, double t, double max_dt,
                                               double *__restrict__ oks) {
  const long long i = (long long)blockIdx.x * kTrackThreads + threadIdx.x;
  if (i >= Dtot * T) return;
  const long long d = i / T;
  const int j = (int)(i - d * T);
  const TrackState st = track_state(blocks[det_stream[d]], T, K);
  if (st.id[j] < 0) {
    oks[i] = 0.0;
    return;
  }
  const long long e0 = (long long)j * K;
  const double *ka = kpts + d * K * 2, *kb = st.kp + e0 * 2;
  const double *va = vis ? vis + d * K : nullptr, *vb = st.vis + e0;
  if constexpr (kPredict) {
    double dt = t - st.t_last[j];
    if (dt > max_dt) dt = max_dt;
    const double *xh = st.xhat + e0 * 2, *dxh = st.dxhat + e0 * 2;
    const unsigned char *init = st.init + e0;
    const auto expected = [=](int k, int c) {
      return init[k] ? xh[2 * k + c] + dxh[2 * k + c] * dt : kb[2 * k + c];
    };
    oks[i] = pair_oks_of(K, ka, expected, va, vb, vis_thr, area[d], st.area[j], vars);
  } else {
    oks[i] = pair_oks(K, ka, kb, va, vb, vis_thr, area[d], st.area[j], vars);   // the detection as the pivot
  }
}

__global__ __launch_bounds__(kTrackThreads) void track_oks_kernel(
    int K, int T, long long Dtot, const long long *__restrict__ det_stream, const long long *__restrict__ blocks,
    const double *__restrict__ kpts, const double *__restrict__ vis, const double *__restrict__ area,
    const double *__restrict__ vars, double vis_thr, double *__restrict__ oks) {
  track_oks_lane<false>(K, T, Dtot, det_stream, blocks, kpts, vis, area, vars, vis_thr, 0.0, 0.0, oks);
}

__global__ __launch_bounds__(kTrackThreads) void track_oks_predicted_kernel(
    int K, int T, long long Dtot, const long long *__restrict__ det_stream, const long long *__restrict__ blocks,
    const double *__restrict__ kpts, const double *__restrict__ vis, const double *__restrict__ area,
    const double *__restrict__ vars, double vis_thr, double t, double max_dt, double *__restrict__ oks) {
  track_oks_lane<true>(K, T, Dtot, det_stream, blocks, kpts, vis, area, vars, vis_thr, t, max_dt, oks);
}

// What the lanes of a stream's wave share between the association modes.  The per-detection outputs of the assign
// launch, and the call's constants they are written with:
struct TrackOut {
  const double *area;
  double t;
  long long *ids;
  double *match_oks;
  unsigned char *born;
  int *slot_of;
  double *te;
};

// detection d continues slot j with pair OKS v: called by the lane that owns j
__device__ __forceinline__ void track_take(const TrackState &st, const TrackOut &o, long long d, int j, double v) {
  o.ids[d] = st.id[j];
  o.match_oks[d] = v;
  o.born[d] = 0;
  o.slot_of[d] = j;
  o.te[d] = o.t - st.t_last[j];
  st.age[j] = 0;
  st.t_last[j] = o.t;
  st.area[j] = o.area[d];
}

// After the association: ageing of every live slot not taken (freed above max_age), then the births of the unmatched
// detections in visiting order, each through wave_min of the lanes' lowest free slot.  valid / live / taken: bit s of
// a lane is its slot s * 64 + lane; unmatched: bit p / 64 of lane p % 64 is detection p.
__device__ __forceinline__ void track_age_and_bear(const TrackState &st, const TrackOut &o, int lane, long long d0,
                                                   int D, int max_age, unsigned long long valid,
                                                   unsigned long long live, unsigned long long taken,
                                                   unsigned long long unmatched) {
  // ageing: every live slot not taken; freed above max_age
  for (unsigned long long m = live & ~taken; m;) {
    const int s = __builtin_ctzll(m);
    m &= m - 1;
    const int j = s * 64 + lane;
    const int a = st.age[j] + 1;
    st.age[j] = a;
    if (a > max_age) {
      st.id[j] = -1;
      live &= ~(1ull << s);
    }
  }

  // births: the unmatched detections in visiting order, each into the lowest free slot
  long long next = *st.next_id, over = 0;                 // wave-uniform
  bool any = false;
  for (int p = 0; p < D; ++p) {
    if (!__shfl((int)((unmatched >> (p >> 6)) & 1ull), p & 63, 64)) continue;   // wave-uniform
    const unsigned long long free_slots = valid & ~live;
    const int j = wave_min(free_slots ? __builtin_ctzll(free_slots) * 64 + lane : INT_MAX);
    const long long d = d0 + p;
    any = true;
    if (j != INT_MAX) {
      if (lane == (j & 63)) {
        live |= 1ull << (j >> 6);
        st.id[j] = next;
        st.age[j] = 0;
        st.t_last[j] = o.t;
        st.area[j] = o.area[d];
        o.ids[d] = next;
        o.match_oks[d] = 0.0;
        o.born[d] = 1;
        o.slot_of[d] = j;
        o.te[d] = 0.0;
      }
      ++next;
    } else {
      if (lane == 0) {
        o.ids[d] = -1;
        o.match_oks[d] = 0.0;
        o.born[d] = 0;
        o.slot_of[d] = -1;
        o.te[d] = 0.0;
      }
      ++over;
    }
  }
  if (any && lane == 0) {
    *st.next_id = next;
    *st.overflow += over;
  }
}

// which of the lane's slots exist and which are live when the call begins
__device__ __forceinline__ void track_slot_masks(const TrackState &st, int lane, int T, unsigned long long &valid,
                                                 unsigned long long &live) {
  valid = live = 0;
  for (int s = 0, slots = (T + 63) >> 6; s < slots; ++s) {
    const int j = s * 64 + lane;
    if (j < T) {
      valid |= 1ull << s;
      if (st.id[j] >= 0) live |= 1ull << s;
    }
  }
}

// The greedy walk of §4.7d over the stream's detections p0 .. p1-1 in visiting order: each takes, among the lane-owned
// slots of `cols` not yet taken, the one with the largest OKS (the lowest on equal OKS) if that OKS is > thr, and is
// marked unmatched otherwise.
__device__ __forceinline__ void track_greedy_rows(const TrackState &st, const TrackOut &out, int lane, long long d0,
                                                  int p0, int p1, int T, const double *__restrict__ oks,
                                                  unsigned long long cols, double thr, unsigned long long &taken,
                                                  unsigned long long &unmatched) {
  for (int p = p0; p < p1; ++p) {
    const double *row = oks + (d0 + p) * T;
    double best = -INFINITY;
    int best_j = INT_MAX;
    unsigned long long cand = cols & ~taken;
    while (cand) {                                        // ascending slots: the lowest of the lane's on equal OKS
      const int s = __builtin_ctzll(cand);
      cand &= cand - 1;
      const int j = s * 64 + lane;
      const double v = row[j];
      if (v > best) {
        best = v;
        best_j = j;
      }
    }
    const double top = wave_max(best);
    const int pick = wave_min(best_j != INT_MAX && best == top ? best_j : INT_MAX);
    if (pick != INT_MAX && top > thr) {                   // wave-uniform
      if (lane == (pick & 63)) {
        taken |= 1ull << (pick >> 6);
        track_take(st, out, d0 + p, pick, top);
      }
    } else if (lane == (p & 63)) {
      unmatched |= 1ull << (p >> 6);
    }
  }
}

__global__ __launch_bounds__(64 * kTrackWaves) void track_assign_kernel(
    int n_str, int K, int T, const long long *__restrict__ off, const long long *__restrict__ blocks,
    const double *__restrict__ oks, const double *__restrict__ area, double match_thr, int max_age, double t,
    long long *__restrict__ ids, double *__restrict__ match_oks, unsigned char *__restrict__ born,
    int *__restrict__ slot_of, double *__restrict__ te) {
  const long long str = (long long)blockIdx.x * kTrackWaves + (threadIdx.x >> 6);
  if (str >= n_str) return;
  const int lane = threadIdx.x & 63;
  const long long d0 = off[str], span = off[str + 1] - d0;
  if (span < 0 || span > PP_TRACK_MAX_DETS || T > PP_TRACK_MAX_TRACKS) return;   // refused on the host
  const int D = (int)span;
  const TrackState st = track_state(blocks[str], T, K);
  const TrackOut out{area, t, ids, match_oks, born, slot_of, te};

  // lane-owned: which of the lane's slots exist, are live (at entry) and are taken in this call; which of the
  // detections p with p % 64 == lane are unmatched
  unsigned long long valid, live, taken = 0, unmatched = 0;
  track_slot_masks(st, lane, T, valid, live);
  track_greedy_rows(st, out, lane, d0, 0, D, T, oks, live, match_thr, taken, unmatched);
  track_age_and_bear(st, out, lane, d0, D, max_age, valid, live, taken, unmatched);
}

// ---- the optimal association (the rule: include/probpose_hip.h, tests/trackopt_reference.py) ---------
constexpr int kOptCols = PP_TRACK_OPT_MAX / 64;           // columns a lane owns at most

// q of a pair whose slot is real and live at entry
__device__ __forceinline__ long long track_weight(double oks, double match_thr) {
  if (!(oks > match_thr)) return 0;                       // a NaN is inadmissible
  return 1 + (long long)floor(fmin(oks - match_thr, 1.0) * 1099511627776.0 /* 2^40 */);
}

// row[j] at the lane's columns that are slots live at entry (bit s of live: slot s * 64 + lane < T), 0 elsewhere
__device__ __forceinline__ void opt_load_row(const double *row, int lane, unsigned long long live,
                                             double (&x)[kOptCols]) {
#pragma unroll
  for (int s = 0; s < kOptCols; ++s) x[s] = ((live >> s) & 1ull) ? row[s * 64 + lane] : 0.0;
}

// The matching of largest total weight between the stream's detections p0 .. p1-1 (the rows, in visiting
// order) and the lane-owned slots of `live` (bit s: slot s * 64 + lane is a column; every other column weighs
// nothing), m = max(rows, T), with track_weight at match_thr.  Matched pairs are stored by the slot's lane and marked
// in `taken`; the rows left over are marked in `unmatched` (bit p / 64 of lane p % 64).  Returns the lane's share of
// the sum of q over the matched pairs.  track_assign_optimal_kernel runs it on every row and every live slot, the
// staged kernel once per stage.
__device__ __forceinline__ long long track_optimal_rows(const TrackState &st, const TrackOut &out, int lane,
                                                        long long d0, int p0, int p1, int T,
                                                        const double *__restrict__ oks, unsigned long long live,
                                                        double match_thr, unsigned long long &taken,
                                                        unsigned long long &unmatched) {
  const int D = p1 - p0, m = D > T ? D : T, cols = (m + 63) >> 6;
  const double *rows = oks + (d0 + p0) * T;

  // lane-owned, column s * 64 + lane in element s: the potential v, the row the column holds (-1: none) and that
  // row's potential u (a row's u travels with the column that holds it; a row not yet added has u = 0)
  long long v[kOptCols], u_held[kOptCols];
  int held[kOptCols];
#pragma unroll
  for (int s = 0; s < kOptCols; ++s) {
    v[s] = u_held[s] = 0;
    held[s] = -1;
  }

  // the OKS of the scanned row at the lane's columns.  A row's first step always scans that row itself, so its OKS are
  // loaded one row ahead, behind the previous row's path; only the later steps wait for a load their row index needs
  double x[kOptCols], ahead[kOptCols];
  if (D > 0) opt_load_row(rows, lane, live, ahead);
  for (int i = 0; i < D; ++i) {                           // the rows in visiting order, one augmenting path each
#pragma unroll
    for (int s = 0; s < kOptCols; ++s) x[s] = ahead[s];
    if (i + 1 < D) opt_load_row(rows + (long long)(i + 1) * T, lane, live, ahead);
    long long minv[kOptCols];
    int way[kOptCols];
    unsigned used = 0;                                    // bit s: the lane's column s is on the tree
#pragma unroll
    for (int s = 0; s < kOptCols; ++s) {
      minv[s] = kSapInf;
      way[s] = kSapRoot;
    }
    int cur = kSapRoot, i0 = i;                           // wave-uniform: the column being scanned, its row,
    long long u0 = 0, u_root = 0;                         // that row's u, and the u of row i (the root's)
    bool open = false;
    for (int step = 0; step <= m; ++step) {               // every step marks one more column: at most m + 1
      if (cur != kSapRoot && lane == (cur & 63)) used |= 1u << (cur >> 6);
      if (step > 0) opt_load_row(rows + (long long)i0 * T, lane, live, x);
      long long delta = LLONG_MAX;
      int j1 = INT_MAX;
#pragma unroll
      for (int s = 0; s < kOptCols; ++s) {                // ascending columns: the lowest of the lane's on equal minv
        const int j = s * 64 + lane;
        if (s < cols && j < m && !((used >> s) & 1u)) {
          const long long q = ((live >> s) & 1ull) ? track_weight(x[s], match_thr) : 0;
          const long long c = -q - u0 - v[s];
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
      for (int s = 0; s < kOptCols; ++s) {
        if ((used >> s) & 1u) {
          u_held[s] += delta;
          v[s] -= delta;
        } else {
          minv[s] -= delta;
        }
      }
      u_root += delta;
      cur = j1;
      i0 = sap_fetch<kOptCols>(held, cur);
      u0 = sap_fetch<kOptCols>(u_held, cur);
      if (i0 < 0) {
        open = true;
        break;
      }
    }
    // walk back: every column of the path takes the row of the column before it
    for (int hop = 0; open && cur != kSapRoot && hop <= m; ++hop) {
      const int prev = sap_fetch<kOptCols>(way, cur);
      int row_prev = i;
      long long u_prev = u_root;
      if (prev != kSapRoot) {                             // wave-uniform
        row_prev = sap_fetch<kOptCols>(held, prev);
        u_prev = sap_fetch<kOptCols>(u_held, prev);
      }
      if (lane == (cur & 63)) {
#pragma unroll
        for (int s = 0; s < kOptCols; ++s)
          if (s == (cur >> 6)) {
            held[s] = row_prev;
            u_held[s] = u_prev;
          }
      }
      cur = prev;
    }
  }

  // a held row is matched if its column is a slot and the pair is admissible; written by the slot's lane
  long long sum = 0;
#pragma unroll
  for (int s = 0; s < kOptCols; ++s) {
    const int j = s * 64 + lane;
    if (j < T && ((live >> s) & 1ull) && held[s] >= 0) {
      const double x = rows[(long long)held[s] * T + j];
      const long long q = track_weight(x, match_thr);
      if (q > 0) {
        sum += q;
        taken |= 1ull << s;
        track_take(st, out, d0 + p0 + held[s], j, x);
      } else {
        held[s] = -1;
      }
    } else {
      held[s] = -1;
    }
  }
  for (int p = 0; p < D; ++p) {
    bool mine = false;
#pragma unroll
    for (int s = 0; s < kOptCols; ++s) mine |= held[s] == p;
    if (!__any(mine) && lane == ((p0 + p) & 63)) unmatched |= 1ull << ((p0 + p) >> 6);
  }
  return sum;
}

__global__ __launch_bounds__(64 * kTrackWaves) void track_assign_optimal_kernel(
    int n_str, int K, int T, const long long *__restrict__ off, const long long *__restrict__ blocks,
    const double *__restrict__ oks, const double *__restrict__ area, double match_thr, int max_age, double t,
    long long *__restrict__ ids, double *__restrict__ match_oks, unsigned char *__restrict__ born,
    int *__restrict__ slot_of, double *__restrict__ te, long long *__restrict__ total) {
  const long long str = (long long)blockIdx.x * kTrackWaves + (threadIdx.x >> 6);
  if (str >= n_str) return;
  const int lane = threadIdx.x & 63;
  const long long d0 = off[str], span = off[str + 1] - d0;
  if (span < 0 || span > PP_TRACK_OPT_MAX || T < 1 || T > PP_TRACK_OPT_MAX) return;   // refused on the host
  const int D = (int)span;
  const TrackState st = track_state(blocks[str], T, K);
  const TrackOut out{area, t, ids, match_oks, born, slot_of, te};

  unsigned long long valid, live, taken = 0, unmatched = 0;
  track_slot_masks(st, lane, T, valid, live);
  const long long sum = wave_sum_i64(track_optimal_rows(st, out, lane, d0, 0, D, T, oks, live, match_thr, taken,
                                                         unmatched));
  if (total && lane == 0) total[str] = sum;
  track_age_and_bear(st, out, lane, d0, D, max_age, valid, live, taken, unmatched);
}

// ---- the staged association (the rule: include/probpose_hip.h, tests/trackstage_reference.py) ---------
// One wave per stream, the launch shape and lane-owns-slot layout of track_assign_kernel.  Stage 1: the detections
// with score >= high_thr (a prefix of the visiting order) on the slots live at entry, at match_thr.  Stage 2: the
// others on the live slots stage 1 left that had age <= low_max_age at entry, at low_match_thr.  Each stage is the
// greedy walk or (kOptimal) the optimal matching.  Then the unmatched detections below birth_thr are dropped, by the
// lane that owns their unmatched bit, and ageing and births follow for the rest.
template <bool kOptimal>
__global__ __launch_bounds__(64 * kTrackWaves) void track_assign_staged_kernel(
    int n_str, int K, int T, const long long *__restrict__ off, const long long *__restrict__ blocks,
    const double *__restrict__ oks, const double *__restrict__ area, const double *__restrict__ score,
    double match_thr, double high_thr, double low_match_thr, int low_max_age, double birth_thr, int max_age, double t,
    long long *__restrict__ ids, double *__restrict__ match_oks, unsigned char *__restrict__ born,
    int *__restrict__ slot_of, double *__restrict__ te, unsigned char *__restrict__ dropped) {
  const long long str = (long long)blockIdx.x * kTrackWaves + (threadIdx.x >> 6);
  if (str >= n_str) return;
  const int lane = threadIdx.x & 63;
  const long long d0 = off[str], span = off[str + 1] - d0;
  constexpr int kMaxD = kOptimal ? PP_TRACK_OPT_MAX : PP_TRACK_MAX_DETS;
  constexpr int kMaxT = kOptimal ? PP_TRACK_OPT_MAX : PP_TRACK_MAX_TRACKS;
  if (span < 0 || span > kMaxD || T < 1 || T > kMaxT) return;                  // refused on the host
  const int D = (int)span;
  const TrackState st = track_state(blocks[str], T, K);
  const TrackOut out{area, t, ids, match_oks, born, slot_of, te};

  unsigned long long valid, live, taken = 0, unmatched = 0, young = 0;
  track_slot_masks(st, lane, T, valid, live);
  for (unsigned long long m = live; m;) {                 // before stage 1 resets the ages of the slots it takes
    const int s = __builtin_ctzll(m);
    m &= m - 1;
    if (st.age[s * 64 + lane] <= low_max_age) young |= 1ull << s;
  }
  long long high = 0;
  for (int p = lane; p < D; p += 64) high += score[d0 + p] >= high_thr ? 1 : 0;
  const int n_high = (int)wave_sum_i64(high);              // wave-uniform

  for (int stage = 0; stage < 2; ++stage) {
    const int p0 = stage ? n_high : 0, p1 = stage ? D : n_high;
    if (p0 >= p1) continue;
    const unsigned long long cols = stage ? live & ~taken & young : live;
    const double thr = stage ? low_match_thr : match_thr;
    if constexpr (kOptimal) (void)track_optimal_rows(st, out, lane, d0, p0, p1, T, oks, cols, thr, taken, unmatched);
    else track_greedy_rows(st, out, lane, d0, p0, p1, T, oks, cols, thr, taken, unmatched);
  }

  unsigned long long bear = 0;
  for (int p = lane; p < D; p += 64) {
    const long long d = d0 + p;
    const bool un = (unmatched >> (p >> 6)) & 1ull;
    const bool drop = un && !(score[d] >= birth_thr);
    if (un && !drop) bear |= 1ull << (p >> 6);
    dropped[d] = drop ? 1 : 0;
    if (drop) {
      ids[d] = -1;
      match_oks[d] = 0.0;
      born[d] = 0;
      slot_of[d] = -1;
      te[d] = 0.0;
    }
  }
  track_age_and_bear(st, out, lane, d0, D, max_age, valid, live, taken, bear);
}

__device__ __forceinline__ double track_alpha(double te, double fc) {
  const double r = ((2.0 * M_PI) * fc) * te;
  return r / (r + 1.0);
}

__global__ __launch_bounds__(kTrackThreads) void track_filter_kernel(
    int K, int T, long long Dtot, const long long *__restrict__ det_stream, const long long *__restrict__ blocks,
    const double *__restrict__ kpts, const double *__restrict__ vis, double vis_thr,
    const int *__restrict__ slot_of, const unsigned char *__restrict__ born, const double *__restrict__ te_of,
    int smooth, double min_cutoff, double beta, double d_cutoff, double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * kTrackThreads + threadIdx.x;
  if (i >= Dtot * K) return;
  const long long d = i / K;
  const int k = (int)(i - d * K);
  const double x0 = kpts[2 * i], x1 = kpts[2 * i + 1];
  double o0 = x0, o1 = x1;
  const int j = slot_of[d];
  if (j >= 0 && j < T) {
    const TrackState st = track_state(blocks[det_stream[d]], T, K);
    const long long e = (long long)j * K + k;
    const double v = vis ? vis[i] : 1.0;
    if (smooth) {
      const bool counted = !vis || v > vis_thr;
      if (!counted) {
        st.init[e] = 0;
      } else if (born[d] || st.init[e] == 0) {
        st.xhat[2 * e] = x0;
        st.xhat[2 * e + 1] = x1;
        st.dxhat[2 * e] = 0.0;
        st.dxhat[2 * e + 1] = 0.0;
        st.init[e] = 1;
      } else {
        const double te = te_of[d];
        const double a_d = track_alpha(te, d_cutoff);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const double x = c ? x1 : x0, xh = st.xhat[2 * e + c];
          const double dx = (x - xh) / te;
          const double dxh = a_d * dx + (1.0 - a_d) * st.dxhat[2 * e + c];
          const double a = track_alpha(te, min_cutoff + beta * fabs(dxh));
          const double nx = a * x + (1.0 - a) * xh;
          st.dxhat[2 * e + c] = dxh;
          st.xhat[2 * e + c] = nx;
          if (c) o1 = nx;
          else o0 = nx;
        }
      }
    }
    st.kp[2 * e] = x0;
    st.kp[2 * e + 1] = x1;
    st.vis[e] = v;
  }
  out[2 * i] = o0;
  out[2 * i + 1] = o1;
}

static int track_check_common(const char *who, int n_str, int K, int T, long long Dtot) {
  PP_REQUIRE(n_str >= 0, "%s: n_str=%d", who, n_str);
  PP_REQUIRE(K > 0, "%s: K=%d", who, K);
  PP_REQUIRE(T >= 1 && T <= PP_TRACK_MAX_TRACKS, "%s: max_tracks=%d is outside 1..%d", who, T, PP_TRACK_MAX_TRACKS);
  PP_REQUIRE(Dtot >= 0, "%s: Dtot=%lld", who, Dtot);
  return 0;
}

static int track_check_offsets(const char *who, int n_str, const long long *h, long long Dtot) {
  PP_REQUIRE(h, "%s: null host offsets", who);
  PP_REQUIRE(h[0] == 0, "%s: offsets do not start at 0 (%lld)", who, h[0]);
  for (int i = 0; i < n_str; ++i)
    PP_REQUIRE(h[i + 1] >= h[i], "%s: detection offsets are not monotone at stream %d (%lld after %lld)", who, i,
               h[i + 1], h[i]);
  PP_REQUIRE(h[n_str] == Dtot, "%s: offsets end at %lld, the arrays hold %lld detections", who, h[n_str], Dtot);
  for (int i = 0; i < n_str; ++i)
    PP_REQUIRE(h[i + 1] - h[i] <= PP_TRACK_MAX_DETS,
               "%s: stream %d has %lld detections, more than the %d one call takes", who, i, h[i + 1] - h[i],
               PP_TRACK_MAX_DETS);
  return 0;
}

// what the assign entries check, in this order
static int track_check_assign(const char *who, int n_str, int K, int T, long long Dtot, const long long *host_off,
                              double match_thr, int max_age, double t, double t_prev, bool pointers) {
  if (int rc = track_check_common(who, n_str, K, T, Dtot)) return rc;
  PP_REQUIRE(match_thr >= 0.0 && match_thr < 1.0, "%s: match_thr=%g is outside [0, 1)", who, match_thr);
  PP_REQUIRE(max_age >= 0, "%s: max_age=%d", who, max_age);
  PP_REQUIRE(t - t_prev > 0.0 && t < INFINITY, "%s: te <= 0 (t=%g after t_prev=%g)", who, t, t_prev);
  PP_REQUIRE(pointers, "%s: null argument", who);
  return track_check_offsets(who, n_str, host_off, Dtot);
}

// the workgroups of `lanes` one-lane items; 2^31 or more are refused, the entry `who` calling the items `what`
static int track_grid(const char *who, long long lanes, const char *what, unsigned *grid) {
  const long long g = (lanes + kTrackThreads - 1) / kTrackThreads;
  PP_REQUIRE(g < (1ll << 31), "%s: %lld %s exceed one grid", who, lanes, what);
  *grid = (unsigned)g;
  return 0;
}

// pp_track_oks and (predicted: with t and max_dt) pp_track_oks_predicted
static int track_launch_oks(const char *who, bool predicted, int n_str, int K, int T, long long Dtot,
                            const long long *host_off, const void *det_stream, const void *blocks, const void *kpts,
                            const void *vis, const void *area, const void *vars, double vis_thr, double t,
                            double max_dt, void *oks, void *stream) {
  if (int rc = track_check_common(who, n_str, K, T, Dtot)) return rc;
  PP_REQUIRE(!vis || vis_thr == vis_thr, "%s: vis_thr is not a number", who);
  if (predicted) {
    PP_REQUIRE(isfinite(t), "%s: t=%g is not finite", who, t);
    PP_REQUIRE(max_dt >= 0.0, "%s: max_dt=%g is negative or not a number", who, max_dt);
  }
  PP_REQUIRE(det_stream && blocks && kpts && area && vars && oks, "%s: null argument", who);
  if (int rc = track_check_offsets(who, n_str, host_off, Dtot)) return rc;
  if (n_str == 0 || Dtot == 0) return 0;
  unsigned grid;
  if (int rc = track_grid(who, Dtot * T, "pairs", &grid)) return rc;
  const auto launch = [&](auto kernel, auto... when) {       // both kernels' arguments, `when` between vis_thr and oks
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kTrackThreads), 0, (hipStream_t)stream, K, T, Dtot,
                       (const long long *)det_stream, (const long long *)blocks, (const double *)kpts,
                       (const double *)vis, (const double *)area, (const double *)vars, vis_thr, when...,
                       (double *)oks);
  };
  if (predicted) launch(track_oks_predicted_kernel, t, max_dt);
  else launch(track_oks_kernel);
  PP_CHECK_LAUNCH(predicted ? "track_oks_predicted_kernel" : "track_oks_kernel");
  return 0;
}

// The three assign entries: pp_track_assign (optimal = 0), pp_track_assign_optimal (optimal = 1, with `total`) and
// pp_track_assign_staged (staged: with `score` .. `birth_thr` and `dropped`; `optimal` is its argument, checked here).
static int track_launch_assign(const char *who, bool staged, int optimal, int n_str, int K, int T, long long Dtot,
                               const long long *host_off, const void *off, const void *blocks, const void *oks,
                               const void *area, const void *score, double match_thr, double high_thr,
                               double low_match_thr, int low_max_age, double birth_thr, int max_age, double t,
                               double t_prev, void *ids, void *match_oks, void *born, void *slot_of, void *te,
                               void *dropped, void *total, void *stream) {
  if (int rc = track_check_assign(who, n_str, K, T, Dtot, host_off, match_thr, max_age, t, t_prev,
                                  off && blocks && oks && area && ids && match_oks && born && slot_of && te &&
                                      (!staged || (score && dropped))))
    return rc;
  if (staged) {
    PP_REQUIRE(high_thr == high_thr, "%s: high_thr is not a number", who);
    PP_REQUIRE(birth_thr == birth_thr, "%s: birth_thr is not a number", who);
    PP_REQUIRE(low_match_thr >= 0.0 && low_match_thr < 1.0, "%s: low_match_thr=%g is outside [0, 1)", who,
               low_match_thr);
    PP_REQUIRE(low_max_age >= 0, "%s: low_max_age=%d", who, low_max_age);
    PP_REQUIRE(optimal == 0 || optimal == 1, "%s: optimal=%d is neither 0 nor 1", who, optimal);
  }
  if (optimal) {
    PP_REQUIRE(T <= PP_TRACK_OPT_MAX, "%s: max_tracks=%d is above PP_TRACK_OPT_MAX = %d", who, T, PP_TRACK_OPT_MAX);
    for (int i = 0; i < n_str; ++i)
      PP_REQUIRE(host_off[i + 1] - host_off[i] <= PP_TRACK_OPT_MAX,
                 "%s: stream %d has %lld detections, more than PP_TRACK_OPT_MAX = %d", who, i,
                 host_off[i + 1] - host_off[i], PP_TRACK_OPT_MAX);
  }
  if (n_str == 0) return 0;                                // a stream without detections still ages its tracks
  const dim3 grid((unsigned)((n_str + kTrackWaves - 1) / kTrackWaves)), block(64 * kTrackWaves);
  const auto *of = (const long long *)off, *bl = (const long long *)blocks;
  const auto *ok = (const double *)oks, *ar = (const double *)area;
  auto *id = (long long *)ids;
  auto *mo = (double *)match_oks, *te_ = (double *)te;
  auto *bo = (unsigned char *)born;
  auto *sl = (int *)slot_of;
  if (staged)
    hipLaunchKernelGGL(optimal ? track_assign_staged_kernel<true> : track_assign_staged_kernel<false>, grid, block, 0,
                       (hipStream_t)stream, n_str, K, T, of, bl, ok, ar, (const double *)score, match_thr, high_thr,
                       low_match_thr, low_max_age, birth_thr, max_age, t, id, mo, bo, sl, te_,
                       (unsigned char *)dropped);
  else if (optimal)
    hipLaunchKernelGGL(track_assign_optimal_kernel, grid, block, 0, (hipStream_t)stream, n_str, K, T, of, bl, ok, ar,
                       match_thr, max_age, t, id, mo, bo, sl, te_, (long long *)total);
  else
    hipLaunchKernelGGL(track_assign_kernel, grid, block, 0, (hipStream_t)stream, n_str, K, T, of, bl, ok, ar,
                       match_thr, max_age, t, id, mo, bo, sl, te_);
  PP_CHECK_LAUNCH(staged ? "track_assign_staged_kernel" : optimal ? "track_assign_optimal_kernel"
                                                                  : "track_assign_kernel");
  return 0;
}

}  // namespace pp

extern "C" long long pp_track_state_bytes(int max_tracks, int K) {
  using namespace pp;
  if (max_tracks < 1 || max_tracks > PP_TRACK_MAX_TRACKS || K <= 0) {
    fail("pp_track_state_bytes: max_tracks=%d (1..%d), K=%d", max_tracks, PP_TRACK_MAX_TRACKS, K);
    return -1;
  }
  return track_state_bytes(max_tracks, K);
}

extern "C" int pp_track_oks(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off,
                            const void *det_stream, const void *blocks, const void *kpts, const void *vis,
                            const void *area, const void *vars, double vis_thr, void *oks, void *stream) {
  return pp::track_launch_oks("pp_track_oks", false, n_str, K, max_tracks, Dtot, host_off, det_stream, blocks, kpts,
                              vis, area, vars, vis_thr, 0.0, 0.0, oks, stream);
}

extern "C" int pp_track_oks_predicted(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off,
                                      const void *det_stream, const void *blocks, const void *kpts, const void *vis,
                                      const void *area, const void *vars, double vis_thr, double t, double max_dt,
                                      void *oks, void *stream) {
  return pp::track_launch_oks("pp_track_oks_predicted", true, n_str, K, max_tracks, Dtot, host_off, det_stream, blocks,
                              kpts, vis, area, vars, vis_thr, t, max_dt, oks, stream);
}

extern "C" int pp_track_assign(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off,
                               const void *off, const void *blocks, const void *oks, const void *area,
                               double match_thr, int max_age, double t, double t_prev, void *ids, void *match_oks,
                               void *born, void *slot_of, void *te, void *stream) {
  return pp::track_launch_assign("pp_track_assign", false, 0, n_str, K, max_tracks, Dtot, host_off, off, blocks, oks,
                                 area, nullptr, match_thr, 0.0, 0.0, 0, 0.0, max_age, t, t_prev, ids, match_oks, born,
                                 slot_of, te, nullptr, nullptr, stream);
}

extern "C" int pp_track_assign_optimal(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off,
                                       const void *off, const void *blocks, const void *oks, const void *area,
                                       double match_thr, int max_age, double t, double t_prev, void *ids,
                                       void *match_oks, void *born, void *slot_of, void *te, void *total,
                                       void *stream) {
  return pp::track_launch_assign("pp_track_assign_optimal", false, 1, n_str, K, max_tracks, Dtot, host_off, off,
                                 blocks, oks, area, nullptr, match_thr, 0.0, 0.0, 0, 0.0, max_age, t, t_prev, ids,
                                 match_oks, born, slot_of, te, nullptr, total, stream);
}

extern "C" int pp_track_assign_staged(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off,
                                      const void *off, const void *blocks, const void *oks, const void *area,
                                      const void *score, double match_thr, double high_thr, double low_match_thr,
                                      int low_max_age, double birth_thr, int optimal, int max_age, double t,
                                      double t_prev, void *ids, void *match_oks, void *born, void *slot_of, void *te,
                                      void *dropped, void *stream) {
  return pp::track_launch_assign("pp_track_assign_staged", true, optimal, n_str, K, max_tracks, Dtot, host_off, off,
                                 blocks, oks, area, score, match_thr, high_thr, low_match_thr, low_max_age, birth_thr,
                                 max_age, t, t_prev, ids, match_oks, born, slot_of, te, dropped, nullptr, stream);
}

extern "C" int pp_track_filter(int K, int max_tracks, long long Dtot, const void *det_stream, const void *blocks,
                               const void *kpts, const void *vis, double vis_thr, const void *slot_of,
                               const void *born, const void *te, int smooth, double min_cutoff, double beta,
                               double d_cutoff, void *out, void *stream) {
  using namespace pp;
  if (int rc = track_check_common("pp_track_filter", 0, K, max_tracks, Dtot)) return rc;
  PP_REQUIRE(!vis || vis_thr == vis_thr, "pp_track_filter: vis_thr is not a number");
  if (smooth)
    PP_REQUIRE(min_cutoff > 0.0 && d_cutoff > 0.0 && beta >= 0.0 && min_cutoff < INFINITY && d_cutoff < INFINITY &&
                   beta < INFINITY,
               "pp_track_filter: min_cutoff=%g, d_cutoff=%g (both > 0), beta=%g (>= 0) must be finite", min_cutoff,
               d_cutoff, beta);
  PP_REQUIRE(det_stream && blocks && kpts && slot_of && born && te && out, "pp_track_filter: null argument");
  if (Dtot == 0) return 0;
  unsigned grid;
  if (int rc = track_grid("pp_track_filter", Dtot * K, "keypoints", &grid)) return rc;
  hipLaunchKernelGGL(track_filter_kernel, dim3(grid), dim3(kTrackThreads), 0, (hipStream_t)stream, K,
                     max_tracks, Dtot, (const long long *)det_stream, (const long long *)blocks, (const double *)kpts,
                     (const double *)vis, vis_thr, (const int *)slot_of, (const unsigned char *)born,
                     (const double *)te, smooth, min_cutoff, beta, d_cutoff, (double *)out);
  PP_CHECK_LAUNCH("track_filter_kernel");
  return 0;
}

// ---- pp_track_boxes: the tracks read back out as person boxes ---------------------------------------
// One lane per (stream, slot) with a serial loop over the slot's K keypoints, as track_oks_kernel walks a pair.  Reads
// the state, writes only its four outputs: no atomics, no LDS, no barrier, plain vector stores.  Every step is one
// IEEE basic operation in the order of include/probpose_hip.h (compiled -ffp-contract=off): the bits of
// tests/trackbox_reference.py.
namespace pp {

__global__ __launch_bounds__(kTrackThreads) void track_boxes_kernel(
    int n_str, int K, int T, const long long *__restrict__ blocks, double t, int use_vis, double vis_thr, int smooth,
    int extrapolate, double max_dt, int max_age, int min_keypoints, double pad, double min_side, double aspect,
    const double *__restrict__ frame_wh, const long long *__restrict__ sup_off, const double *__restrict__ sup_boxes,
    double iou_thr, double *__restrict__ boxes, long long *__restrict__ ids, double *__restrict__ scores,
    unsigned char *__restrict__ status) {
  const long long i = (long long)blockIdx.x * kTrackThreads + threadIdx.x;
  if (i >= (long long)n_str * T) return;
  const long long s = i / T;
  const int j = (int)(i - s * T);
  const TrackState st = track_state(blocks[s], T, K);
  const long long id = st.id[j];
  double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0, score = 0.0;
  int code = PP_TRACK_BOX_FREE;
  do {
    if (id < 0) break;
    code = PP_TRACK_BOX_OLD;
    if (st.age[j] > max_age) break;
    double dt = t - st.t_last[j];
    if (dt > max_dt) dt = max_dt;
    const long long e0 = (long long)j * K;
    double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0, sum = 0.0;
    int n = 0;
    for (int k = 0; k < K; ++k) {
      const double v = st.vis[e0 + k];
      if (use_vis && !(v > vis_thr)) continue;
      const long long e = 2 * (e0 + k);
      double px, py;
      if (smooth && st.init[e0 + k]) {
        px = st.xhat[e];
        py = st.xhat[e + 1];
        if (extrapolate) {
          px = px + st.dxhat[e] * dt;
          py = py + st.dxhat[e + 1] * dt;
        }
      } else {
        px = st.kp[e];
        py = st.kp[e + 1];
      }
      if (n == 0) {
        x0 = x1 = px;
        y0 = y1 = py;
      } else {
        if (px < x0) x0 = px;
        if (px > x1) x1 = px;
        if (py < y0) y0 = py;
        if (py > y1) y1 = py;
      }
      sum += v;
      ++n;
    }
    code = PP_TRACK_BOX_FEW;
    if (n < min_keypoints) break;
    const double cx = (x0 + x1) * 0.5, cy = (y0 + y1) * 0.5;
    double w = (x1 - x0) * pad, h = (y1 - y0) * pad;
    if (!(w >= min_side)) w = min_side;
    if (!(h >= min_side)) h = min_side;
    if (aspect > 0.0) {
      const double wa = h * aspect;
      if (w < wa) w = wa;
      else h = w / aspect;
    }
    double bx = cx - w * 0.5, by = cy - h * 0.5;
    double ex = bx + w, ey = by + h;
    if (frame_wh) {
      const double fw = frame_wh[2 * s], fh = frame_wh[2 * s + 1];
      if (fw > 0.0) {
        if (bx < 0.0) bx = 0.0;
        if (by < 0.0) by = 0.0;
        if (ex > fw) ex = fw;
        if (ey > fh) ey = fh;
      }
    }
    w = ex - bx;
    h = ey - by;
    code = PP_TRACK_BOX_OUTSIDE;
    if (!(isfinite(bx) && isfinite(by) && isfinite(w) && isfinite(h)) || !(w >= min_side && h >= min_side)) break;
    code = PP_TRACK_BOX_PROPOSED;
    if (sup_off && sup_boxes) {
      const double mine = w * h;
      for (long long g = sup_off[s], g1 = sup_off[s + 1]; g < g1; ++g) {
        const double gx = sup_boxes[4 * g], gy = sup_boxes[4 * g + 1], gw = sup_boxes[4 * g + 2],
                     gh = sup_boxes[4 * g + 3];
        if (!(gw > 0.0 && gh > 0.0)) continue;
        const double gex = gx + gw, gey = gy + gh;
        const double ix = (ex < gex ? ex : gex) - (bx > gx ? bx : gx);
        const double iy = (ey < gey ? ey : gey) - (by > gy ? by : gy);
        const double inter = (ix > 0.0 && iy > 0.0) ? ix * iy : 0.0;
        const double uni = (mine + gw * gh) - inter;
        const double iou = uni > 0.0 ? inter / uni : 0.0;
        if (iou > iou_thr) {
          code = PP_TRACK_BOX_SUPPRESSED;
          break;
        }
      }
    }
    o0 = bx;
    o1 = by;
    o2 = w;
    o3 = h;
    score = sum / (double)n;
  } while (false);
  boxes[4 * i] = o0;
  boxes[4 * i + 1] = o1;
  boxes[4 * i + 2] = o2;
  boxes[4 * i + 3] = o3;
  ids[i] = id < 0 ? -1 : id;
  scores[i] = score;
  status[i] = (unsigned char)code;
}

}  // namespace pp

extern "C" int pp_track_boxes(int n_str, int K, int max_tracks, const void *blocks, double t, int use_vis,
                              double vis_thr, int smooth, int extrapolate, double max_dt, int max_age,
                              int min_keypoints, double pad, double min_side, double aspect, const void *frame_wh,
                              const long long *host_sup_off, const void *sup_off, const void *sup_boxes, double iou_thr,
                              void *boxes, void *ids, void *scores, void *status, void *stream) {
  using namespace pp;
  if (int rc = track_check_common("pp_track_boxes", n_str, K, max_tracks, 0)) return rc;
  PP_REQUIRE(isfinite(t), "pp_track_boxes: t=%g is not finite", t);
  PP_REQUIRE(!use_vis || vis_thr == vis_thr, "pp_track_boxes: vis_thr is not a number");
  PP_REQUIRE(max_dt >= 0.0, "pp_track_boxes: max_dt=%g is negative or not a number", max_dt);
  PP_REQUIRE(max_age >= 0, "pp_track_boxes: max_age=%d", max_age);
  PP_REQUIRE(min_keypoints >= 1, "pp_track_boxes: min_keypoints=%d", min_keypoints);
  PP_REQUIRE(isfinite(pad) && pad > 0.0, "pp_track_boxes: pad=%g must be finite and > 0", pad);
  PP_REQUIRE(isfinite(min_side) && min_side > 0.0, "pp_track_boxes: min_side=%g must be finite and > 0", min_side);
  PP_REQUIRE(isfinite(aspect) && aspect >= 0.0, "pp_track_boxes: aspect=%g must be finite and >= 0", aspect);
  PP_REQUIRE(iou_thr >= 0.0 && iou_thr <= 1.0, "pp_track_boxes: iou_thr=%g is outside [0, 1]", iou_thr);
  PP_REQUIRE(!host_sup_off == !sup_off, "pp_track_boxes: sup_off needs its host copy and its device copy, or neither");
  if (host_sup_off) {
    PP_REQUIRE(host_sup_off[0] == 0, "pp_track_boxes: sup_off does not start at 0 (%lld)", host_sup_off[0]);
    for (int i = 0; i < n_str; ++i)
      PP_REQUIRE(host_sup_off[i + 1] >= host_sup_off[i],
                 "pp_track_boxes: sup_off is not ascending at stream %d (%lld after %lld)", i, host_sup_off[i + 1],
                 host_sup_off[i]);
    PP_REQUIRE(host_sup_off[n_str] == 0 || sup_boxes, "pp_track_boxes: sup_off names %lld boxes, sup_boxes is null",
               host_sup_off[n_str]);
  }
  if (n_str == 0) return 0;
  PP_REQUIRE(blocks && boxes && ids && scores && status, "pp_track_boxes: null argument (blocks or an output)");
  unsigned grid;
  if (int rc = track_grid("pp_track_boxes", (long long)n_str * max_tracks, "slots", &grid)) return rc;
  hipLaunchKernelGGL(track_boxes_kernel, dim3(grid), dim3(kTrackThreads), 0, (hipStream_t)stream, n_str, K,
                     max_tracks, (const long long *)blocks, t, use_vis, vis_thr, smooth, extrapolate, max_dt, max_age,
                     min_keypoints, pad, min_side, aspect, (const double *)frame_wh, (const long long *)sup_off,
                     (const double *)sup_boxes, iou_thr, (double *)boxes, (long long *)ids, (double *)scores,
                     (unsigned char *)status);
  PP_CHECK_LAUNCH("track_boxes_kernel");
  return 0;
}
