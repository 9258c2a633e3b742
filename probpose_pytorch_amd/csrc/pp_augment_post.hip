// The pixel steps of Augment that follow the warp: a light box or median blur, then coarse dropout
// (random erasing), one launch for the batch between pp_augment_warp and the keypoint kernel.
//
// records [n, 24] int32 per sample: {kind, k, n_holes, fill (f32 bits), 4 x {x0, y0, x1, y1}, 4 x 0}; in / out are the
// warp's [n, 3, in_h, in_w] f32.  Per sample and channel, in this order:
//   1. filter (filters = 1 only): kind 1 = the mean of the k x k window in float32 (the k * k values added one after the
//      other, one division by k * k), kind 2 = the median of the k x k window (an element of it: exact), kind 0 = a
//      copy.  Borders are reflect-101: index -i reads i, index W - 1 + i reads W - 1 - i.
//   2. holes: every pixel inside any of the first n_holes half-open rectangles [x0, x1) x [y0, y1) becomes fill.
// filters = 0: the kind fields are not read, only holes are written (in == out allowed), and a workgroup whose tile
// meets no hole returns before it touches memory.
//
// augment_post_kernel: one workgroup of 256 threads per (sample, tile of TILE_W x TILE_H = 64 x 16 pixels); a thread
// holds 4 consecutive u of one row, for the three channels, as the warp's threads do.  kind, k and the holes are read
// from the sample's record through wave-uniform addresses, so every branch on them is taken by whole waves.  For a
// filter the tile plus a halo of r = k / 2 is staged in LDS for the three channels at once, the reflected index
// resolved and then clamped into the crop at the load, so no load leaves `in` whatever the record holds (a kind or k the
// kernel does not know is a copy).  The LDS image has a fixed left margin of 4 floats and rows of 72 floats, so that a
// thread's window row, columns 4 lx + 4 - r .. 4 lx + 7 + r, lies in the three aligned 16-byte pieces at 4 lx (the
// compiler narrows those reads to the columns a filter size uses: ds_read2_b32 / ds_read2_b64); the 16 lanes of one
// tile row cover 64 consecutive banks.  The box mean adds from those registers; the median is a selection in
// registers (median_select).  Stores are 128-bit along u where in_w % 4 == 0
// and the buffers are 16-byte aligned, one float at a time otherwise.  No atomics, nothing read back by the host.
#include "pp_common.h"

#include <math.h>

namespace pp {

constexpr int POST_TW = PP_AUGMENT_POST_TILE_W, POST_TH = PP_AUGMENT_POST_TILE_H;
constexpr int POST_RMAX = 3, POST_PAD = 4;                    // the largest halo; the LDS image's left and right margin
constexpr int POST_LW = POST_TW + 2 * POST_PAD, POST_LH = POST_TH + 2 * POST_RMAX;
static_assert(POST_TW == 64 && POST_TH == 16, "256 threads x 4 pixels cover the tile");
static_assert(POST_PAD >= POST_RMAX && POST_PAD % 4 == 0 && POST_LW % 4 == 0, "aligned 16-byte window pieces");

__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i > n - 1 ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);             // a tile column beyond the halo, or a record the host never checked
}

__device__ __forceinline__ void order(float &a, float &b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// The median of N values (N odd) by forgetful selection: of any N / 2 + 2 of them neither the smallest nor the largest
// can be the median (N / 2 + 1 others lie on one side of it), so both are dropped and one value that was not looked
// at yet joins; with three left and none to join, the middle one is the median.  Only comparisons and moves: the
// result is one of the inputs.
template <int N>
__device__ __forceinline__ float median_select(const float (&a)[N]) {
  constexpr int M0 = N / 2 + 2;
  float w[M0];
#pragma unroll
  for (int i = 0; i < M0; ++i) w[i] = a[i];
#pragma unroll
  for (int m = M0; m >= 3; --m) {
#pragma unroll
    for (int i = 0; i + 1 < m; ++i) order(w[i], w[i + 1]);        // the largest of w[0 .. m) to w[m - 1]: dropped
#pragma unroll
    for (int i = m - 2; i >= 1; --i) order(w[i - 1], w[i]);       // the smallest to w[0]: replaced
    if (m > 3) w[0] = a[N - (m - 3)];
  }
  return w[1];
}

struct PostHoles {
  int n;
  int r[4][4];
  __device__ __forceinline__ bool meets_tile(int u_lo, int v_lo) const {
    bool any = false;
#pragma unroll
    for (int h = 0; h < 4; ++h)
      any = any || (h < n && r[h][0] < u_lo + POST_TW && r[h][2] > u_lo && r[h][1] < v_lo + POST_TH && r[h][3] > v_lo);
    return any;
  }
  __device__ __forceinline__ bool covers(int u, int v) const {
    bool any = false;
#pragma unroll
    for (int h = 0; h < 4; ++h) any = any || (h < n && u >= r[h][0] && u < r[h][2] && v >= r[h][1] && v < r[h][3]);
    return any;
  }
};

// Stage tile + halo of the three channels, filter the thread's 4 pixels of each channel into res.
template <int KIND, int R>
__device__ __forceinline__ void post_filter(const float *__restrict__ img, int in_w, int in_h, int u_lo, int v_lo,
                                            float (*tile)[POST_LH][POST_LW], float (&res)[3][4]) {
  constexpr int K = 2 * R + 1, COLS = POST_TW + 2 * R, ROWS = POST_TH + 2 * R;
  const size_t plane = (size_t)in_h * in_w;
  for (int e = threadIdx.x; e < ROWS * COLS; e += 256) {
    const int ry = e / COLS, cx = e - ry * COLS;
    const size_t at = (size_t)reflect101(v_lo + ry - R, in_h) * in_w + reflect101(u_lo + cx - R, in_w);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) tile[ch][ry][POST_PAD - R + cx] = img[ch * plane + at];
  }
  __syncthreads();
  const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float win[K][12];
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
      const float4 *p = reinterpret_cast<const float4 *>(&tile[ch][ly + dy][4 * lx]);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float4 t = p[q];
        win[dy][4 * q] = t.x, win[dy][4 * q + 1] = t.y, win[dy][4 * q + 2] = t.z, win[dy][4 * q + 3] = t.w;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (KIND == 1) {
        float s = 0.0f;
#pragma unroll
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
          for (int dx = 0; dx < K; ++dx) s = s + win[dy][POST_PAD + j - R + dx];
        res[ch][j] = s / (float)(K * K);
      } else {
        float a[K * K];
#pragma unroll
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
          for (int dx = 0; dx < K; ++dx) a[dy * K + dx] = win[dy][POST_PAD + j - R + dx];
        res[ch][j] = median_select<K * K>(a);
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void augment_post_kernel(const float *in, const int *__restrict__ records, int in_w,
                                                           int in_h, int tiles_x, int tiles_y, int filters,
                                                           float *out) {
  __shared__ __attribute__((aligned(16))) float tile[3][POST_LH][POST_LW];
  const int bx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x, by = rest % tiles_y, b = rest / tiles_y;
  const int *rec = records + 24 * (size_t)b;
  const int u_lo = bx * POST_TW, v_lo = by * POST_TH;
  PostHoles holes;
  holes.n = min(max(rec[2], 0), 4);
  const float fill = __int_as_float(rec[3]);
#pragma unroll
  for (int h = 0; h < 4; ++h)
#pragma unroll
    for (int c = 0; c < 4; ++c) holes.r[h][c] = rec[4 + 4 * h + c];
  const bool meets = holes.meets_tile(u_lo, v_lo);
  if (!filters && !meets) return;

  const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int u0 = u_lo + 4 * lx, v = v_lo + ly;
  const size_t plane = (size_t)in_h * in_w;
  const size_t first = (size_t)b * 3 * plane;
  const bool inside = v < in_h && u0 < in_w;                  // VEC: in_w % 4 == 0, so u0 + 3 < in_w as well
  bool hole[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) hole[j] = meets && holes.covers(u0 + j, v);

  if (!filters) {                                             // holes only: nothing is read, `out` may be `in`
    if (!inside) return;
    float *o = out + first + (size_t)v * in_w + u0;
    if (VEC && hole[0] && hole[1] && hole[2] && hole[3]) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<float4 *>(o + ch * plane) = make_float4(fill, fill, fill, fill);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (hole[j] && u0 + j < in_w)
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) o[ch * plane + j] = fill;
    }
    return;
  }

  const int kind = rec[0], k = rec[1];
  float res[3][4];
  const float *img = in + first;
  if (kind == 1 && k == 3) post_filter<1, 1>(img, in_w, in_h, u_lo, v_lo, tile, res);
  else if (kind == 1 && k == 5) post_filter<1, 2>(img, in_w, in_h, u_lo, v_lo, tile, res);
  else if (kind == 1 && k == 7) post_filter<1, 3>(img, in_w, in_h, u_lo, v_lo, tile, res);
  else if (kind == 2 && k == 3) post_filter<2, 1>(img, in_w, in_h, u_lo, v_lo, tile, res);
  else if (kind == 2 && k == 5) post_filter<2, 2>(img, in_w, in_h, u_lo, v_lo, tile, res);
  else if (inside) {                                          // a copy
    const float *p = img + (size_t)v * in_w + u0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if constexpr (VEC) {
        const float4 t = *reinterpret_cast<const float4 *>(p + ch * plane);
        res[ch][0] = t.x, res[ch][1] = t.y, res[ch][2] = t.z, res[ch][3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) res[ch][j] = u0 + j < in_w ? p[ch * plane + j] : 0.0f;
      }
    }
  }
  if (!inside) return;
  float *o = out + first + (size_t)v * in_w + u0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
    for (int j = 0; j < 4; ++j) res[ch][j] = hole[j] ? fill : res[ch][j];
    if constexpr (VEC) {
      *reinterpret_cast<float4 *>(o + ch * plane) = make_float4(res[ch][0], res[ch][1], res[ch][2], res[ch][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (u0 + j < in_w) o[ch * plane + j] = res[ch][j];
    }
  }
}

}  // namespace pp

extern "C" int pp_augment_post_check(int n, const int *records, int in_w, int in_h, int filters) {
  using namespace pp;
  const char *who = "pp_augment_post_check";
  PP_REQUIRE(n >= 1 && records && in_w >= 1 && in_h >= 1 && (filters == 0 || filters == 1), "%s: bad arguments", who);
  for (int c = 0; c < n; ++c) {
    const int *r = records + 24 * (size_t)c;
    const int kind = r[0], k = r[1], nh = r[2];
    PP_REQUIRE(kind >= 0 && kind <= 2, "%s: sample %d has kind %d, outside 0..2", who, c, kind);
    PP_REQUIRE(kind == 0 || filters == 1, "%s: sample %d has kind %d, but filters = 0 writes holes only", who, c, kind);
    if (kind == 0) {
      PP_REQUIRE(k == 0, "%s: sample %d has no filter (kind 0) but a kernel size k = %d", who, c, k);
    } else {
      PP_REQUIRE(k == 3 || k == 5 || (k == 7 && kind == 1),
                 "%s: sample %d has kernel size k = %d; the box blur takes 3, 5, 7 and the median 3, 5", who, c, k);
      PP_REQUIRE(k <= in_w && k <= in_h, "%s: sample %d has kernel size k = %d, larger than the %d x %d crop", who, c,
                 k, in_w, in_h);
    }
    PP_REQUIRE(nh >= 0 && nh <= 4, "%s: sample %d has %d holes, outside 0..4", who, c, nh);
    float fill;
    memcpy(&fill, r + 3, sizeof fill);
    PP_REQUIRE(isfinite(fill), "%s: sample %d has a fill that is not finite", who, c);
    for (int h = 0; h < nh; ++h) {
      const int *q = r + 4 + 4 * h;
      PP_REQUIRE(q[0] < q[2] && q[1] < q[3], "%s: hole %d of sample %d, [%d, %d) x [%d, %d), is empty", who, h, c,
                 q[0], q[2], q[1], q[3]);
      PP_REQUIRE(q[0] >= 0 && q[1] >= 0 && q[2] <= in_w && q[3] <= in_h,
                 "%s: hole %d of sample %d, [%d, %d) x [%d, %d), leaves the %d x %d crop", who, h, c, q[0], q[2], q[1],
                 q[3], in_w, in_h);
    }
    for (int j = 20; j < 24; ++j)
      PP_REQUIRE(r[j] == 0, "%s: sample %d has a non-zero reserved word (%d at %d)", who, c, r[j], j);
  }
  return 0;
}

extern "C" int pp_augment_post(const float *in, const int *records, int n, int in_w, int in_h, int filters, float *out,
                               void *stream) {
  using namespace pp;
  const char *who = "pp_augment_post";
  PP_REQUIRE(n >= 1 && in_w >= 1 && in_h >= 1 && (filters == 0 || filters == 1), "%s: bad shape or mode", who);
  PP_REQUIRE(in && records && out, "%s: null pointer", who);
  const uintptr_t a = reinterpret_cast<uintptr_t>(in), o = reinterpret_cast<uintptr_t>(out);
  PP_REQUIRE(a % 4 == 0 && o % 4 == 0 && reinterpret_cast<uintptr_t>(records) % 4 == 0,
             "%s: a buffer is not 4-byte aligned (misaligned)", who);
  const long long tiles_x = cdiv(in_w, POST_TW), tiles_y = cdiv(in_h, POST_TH);
  PP_REQUIRE((long long)n * 3 * in_w * in_h < (1ll << 31) && (long long)n * tiles_x * tiles_y < (1ll << 31),
             "%s: more than 2^31 elements or workgroups", who);
  const uintptr_t bytes = (uintptr_t)n * 3 * in_w * in_h * sizeof(float);
  if (filters)
    PP_REQUIRE(a + bytes <= o || o + bytes <= a, "%s: with filters = 1, out must not overlap in", who);
  else
    PP_REQUIRE(a == o || a + bytes <= o || o + bytes <= a, "%s: with filters = 0, out is in or does not overlap it", who);
  const dim3 grid((unsigned)(n * tiles_x * tiles_y));
  if (in_w % 4 == 0 && a % 16 == 0 && o % 16 == 0) {
    hipLaunchKernelGGL(augment_post_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, records, in_w, in_h,
                       (int)tiles_x, (int)tiles_y, filters, out);
  } else {
    hipLaunchKernelGGL(augment_post_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, records, in_w, in_h,
                       (int)tiles_x, (int)tiles_y, filters, out);
  }
  PP_CHECK_LAUNCH("augment_post_kernel");
  return 0;
}
