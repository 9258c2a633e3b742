// Visualisation on the device (probpose_pytorch_amd/viz.py): heat overlays and pose drawing on uint8 RGB
// images, and heat maps as RGBA pictures.  Two memory-bound kernels, no atomics, the same bytes on every call.
//
// viz_render_kernel    out[b, y, x, :] = draw(overlay(image[b, y, x, :])): one pass, every image byte read once and
//                      written once; either half can be switched off (heat == NULL, kpts == NULL).  A workgroup owns
//                      1024 consecutive pixels of one image, a thread 4 consecutive pixels = 12 bytes = three dwords,
//                      loaded and stored as dwords in the <true> instance (every image 4-byte aligned); the <false>
//                      instance and the last, partly filled group of an image move bytes.
//   overlay            per pixel the K maps of its image are read in ascending k (the inner loop; a crop's maps stay in
//                      L2): the map's own element when the map has the image's size, else the bilinear value of its 4
//                      taps in float64 rounded to float32; matplotlib's Colormap.__call__ picks a row of the float64
//                      [256, 3] table (in LDS, 6 KB); values below float32(0.01) add nothing; the float64 sum times 255
//                      is saturated at 255, truncated and added to the pixel with saturation.
//   draw               the primitives of the image (limbs first, then discs; instances ascending) are visited in order,
//                      256 candidates at a time, one a thread: a candidate whose bounding box meets the tile's is
//                      appended to an LDS list by an ordered compaction (ballot + popcount, wave totals through LDS).
//                      When the list could not take 256 more, or at the end, every thread resolves its 4 pixels against
//                      the list in order (all lanes read the same entry: a broadcast), the last primitive that covers a
//                      pixel wins, and the list starts again: nothing is ever dropped.  Integer arithmetic only.
//
// viz_colorize_kernel  one workgroup a map: with `normalize` numpy's NaN-propagating maximum first (wave shuffles, then
//                      LDS) and v / max in float32; the colormap row as one RGBA dword from a 256-entry LDS table.
#include "pp_common.h"

namespace pp {

constexpr int VIZ_THREADS = 256, VIZ_PPT = 4, VIZ_TILE = VIZ_THREADS * VIZ_PPT, VIZ_CAP = 1024;
constexpr unsigned VIZ_LIMB = 1u << 24;       // in VizPrim::color, above the packed r | g << 8 | b << 16

struct VizPrim {
  int ax, ay, bx, by;        // a disc: its centre twice
  unsigned color;
};

struct VizRender {
  const void *image;
  unsigned char *out;
  int f32chw, B, H, W;
  const float *heat;
  int K, h, w;
  const double *lut;
  const double *kpts, *probs;
  const int *inst, *img_off, *style;
  int N, Kp, L;
  double threshold;
  int radius, line_width;
};

// matplotlib's Colormap.__call__ on a float32 value: the row of the table, -1 for NaN (the "bad" colour, all zeros)
__device__ __forceinline__ int viz_lut_row(float v) {
  const float xa = v * 256.0f;
  if (xa != xa) return -1;
  if (xa < 0.0f) return 0;
  if (xa >= 256.0f) return 255;
  return (int)xa;
}

// the reference's `if prob < thr: continue; x, y = int(kp[0]), int(kp[1]); if 0 <= x < W and 0 <= y < H`
__device__ __forceinline__ bool viz_centre(const VizRender &a, long long idx, int &x, int &y) {
  if (a.probs[idx] < a.threshold) return false;
  const double fx = a.kpts[2 * idx], fy = a.kpts[2 * idx + 1];
  if (!(fabs(fx) < 2147483648.0) || !(fabs(fy) < 2147483648.0)) return false;      // NaN, inf, 2^31 and beyond
  x = (int)fx;
  y = (int)fy;
  return x >= 0 && x < a.W && y >= 0 && y < a.H;
}

__device__ __forceinline__ bool viz_covers(const VizPrim &q, int px, int py, int r2, long long lw2) {
  const int ex = px - q.ax, ey = py - q.ay;
  if (!(q.color & VIZ_LIMB)) return ex * ex + ey * ey <= r2;
  const long long dx = q.bx - q.ax, dy = q.by - q.ay, L2 = dx * dx + dy * dy;
  const long long t = ex * dx + ey * dy;
  if (t <= 0) return 4ll * ((long long)ex * ex + (long long)ey * ey) <= lw2;
  if (t >= L2) {
    const long long fx = px - q.bx, fy = py - q.by;
    return 4ll * (fx * fx + fy * fy) <= lw2;
  }
  const long long cr = ex * dy - ey * dx;
  return 4ll * cr * cr <= lw2 * L2;
}

template <bool VEC>
__global__ __launch_bounds__(VIZ_THREADS) void viz_render_kernel(const VizRender a, const int tiles) {
  __shared__ double s_lut[768];
  __shared__ VizPrim s_prim[VIZ_CAP];
  __shared__ int s_wave[VIZ_THREADS / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int HW = a.H * a.W;
  const int p0 = tile * VIZ_TILE + tid * VIZ_PPT;
  const int nvalid = min(VIZ_PPT, HW - p0);           // <= 0: a thread past the image; it still meets every barrier
  if (a.heat)
    for (int i = tid; i < 768; i += VIZ_THREADS) s_lut[i] = a.lut[i];

  int px[VIZ_PPT], py[VIZ_PPT];
  {
    int y = p0 / a.W, x = p0 - y * a.W;
#pragma unroll
    for (int j = 0; j < VIZ_PPT; ++j) {
      px[j] = x;
      py[j] = y;
      if (++x == a.W) x = 0, ++y;
    }
  }

  // ---- draw: which primitive, if any, each of the 4 pixels shows -------------------------------------------------
  unsigned covered = 0, col[VIZ_PPT] = {0, 0, 0, 0};
  if (a.kpts) {
    const int t0 = tile * VIZ_TILE, t1 = min(t0 + VIZ_TILE, HW) - 1;
    const int ty0 = t0 / a.W, ty1 = t1 / a.W;
    const int tx0 = ty0 == ty1 ? t0 - ty0 * a.W : 0, tx1 = ty0 == ty1 ? t1 - ty1 * a.W : a.W - 1;
    const int i0 = min(max(a.img_off[b], 0), a.N), i1 = min(max(a.img_off[b + 1], i0), a.N);
    const long long n_limb = (long long)(i1 - i0) * a.L, n_all = n_limb + (long long)(i1 - i0) * a.Kp;
    const int r2 = a.radius * a.radius + a.radius, pad = (a.line_width + 1) / 2;
    const long long lw2 = (long long)a.line_width * a.line_width;
    const int lane = tid & 63, wv = tid >> 6;
    int cnt = 0;
    for (long long c0 = 0; c0 < n_all; c0 += VIZ_THREADS) {
      const long long c = c0 + tid;
      bool keep = false;
      VizPrim q = {0, 0, 0, 0, 0};
      if (c < n_limb) {
        const int ii = (int)(c / a.L), l = (int)(c - (long long)ii * a.L);
        const int n = a.inst[i0 + ii];
        const int ki = a.style[a.Kp + 3 * l], kj = a.style[a.Kp + 3 * l + 1];
        if ((unsigned)n < (unsigned)a.N && (unsigned)ki < (unsigned)a.Kp && (unsigned)kj < (unsigned)a.Kp &&
            viz_centre(a, (long long)n * a.Kp + ki, q.ax, q.ay) &&
            viz_centre(a, (long long)n * a.Kp + kj, q.bx, q.by) && (q.ax != q.bx || q.ay != q.by)) {
          q.color = (unsigned)a.style[a.Kp + 3 * l + 2] | VIZ_LIMB;
          keep = min(q.ax, q.bx) - pad <= tx1 && max(q.ax, q.bx) + pad >= tx0 && min(q.ay, q.by) - pad <= ty1 &&
                 max(q.ay, q.by) + pad >= ty0;
        }
      } else if (c < n_all) {
        const long long d = c - n_limb;
        const int ii = (int)(d / a.Kp), k = (int)(d - (long long)ii * a.Kp);
        const int n = a.inst[i0 + ii];
        if ((unsigned)n < (unsigned)a.N && viz_centre(a, (long long)n * a.Kp + k, q.ax, q.ay)) {
          q.bx = q.ax;
          q.by = q.ay;
          q.color = (unsigned)a.style[k] & 0xffffffu;
          keep = q.ax - a.radius <= tx1 && q.ax + a.radius >= tx0 && q.ay - a.radius <= ty1 && q.ay + a.radius >= ty0;
        }
      }
      // ordered compaction: a kept candidate goes behind every kept candidate of a smaller index
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) s_wave[wv] = __popcll(bal);
      __syncthreads();
      int base = cnt, total = 0;
#pragma unroll
      for (int v = 0; v < VIZ_THREADS / 64; ++v) {
        if (v < wv) base += s_wave[v];
        total += s_wave[v];
      }
      if (keep) s_prim[base + __popcll(bal & ((1ull << lane) - 1ull))] = q;
      cnt += total;
      __syncthreads();
      if (cnt + VIZ_THREADS > VIZ_CAP || c0 + VIZ_THREADS >= n_all) {         // the same decision in every thread
        for (int e = 0; e < cnt; ++e) {
          const VizPrim s = s_prim[e];
#pragma unroll
          for (int j = 0; j < VIZ_PPT; ++j)
            if (j < nvalid && viz_covers(s, px[j], py[j], r2, lw2)) {
              covered |= 1u << j;
              col[j] = s.color;
            }
        }
        cnt = 0;
        __syncthreads();
      }
    }
  }
  __syncthreads();                                   // s_lut is filled
  if (nvalid <= 0) return;

  // ---- the image's 12 bytes --------------------------------------------------------------------------------------
  const size_t pix = (size_t)b * HW + p0;
  unsigned rgb[3 * VIZ_PPT];                         // bytes, one a register
  const bool whole = VEC && nvalid == VIZ_PPT;
  if (a.f32chw) {
    const float *src = (const float *)a.image + (size_t)b * 3 * HW + p0;
#pragma unroll
    for (int j = 0; j < VIZ_PPT; ++j)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float t = j < nvalid ? src[(size_t)ch * HW + j] : 0.0f;
        t = t * 255.0f + 0.5f;
        t = t > 0.0f ? t : 0.0f;                       // NaN -> 0
        t = t < 255.0f ? t : 255.0f;
        rgb[3 * j + ch] = (unsigned)(int)t;
      }
  } else {
    const unsigned char *src = (const unsigned char *)a.image + pix * 3;
    if (whole) {
      const unsigned *s4 = reinterpret_cast<const unsigned *>(src);
      const unsigned w0 = s4[0], w1 = s4[1], w2 = s4[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        rgb[i] = w0 >> (8 * i) & 255u;
        rgb[4 + i] = w1 >> (8 * i) & 255u;
        rgb[8 + i] = w2 >> (8 * i) & 255u;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 3 * VIZ_PPT; ++i) rgb[i] = i < 3 * nvalid ? src[i] : 0;
    }
  }

  // ---- overlay ---------------------------------------------------------------------------------------------------
  if (a.heat) {
    const bool same = a.h == a.H && a.w == a.W;
    int x0[VIZ_PPT], x1[VIZ_PPT], y0[VIZ_PPT], y1[VIZ_PPT];
    double fx[VIZ_PPT], fy[VIZ_PPT], acc[VIZ_PPT][3];
#pragma unroll
    for (int j = 0; j < VIZ_PPT; ++j) {
      acc[j][0] = acc[j][1] = acc[j][2] = 0.0;
      const double u = a.W == 1 ? 0.0 : (double)(px[j] * (a.w - 1)) / (double)(a.W - 1);
      const double v = a.H == 1 ? 0.0 : (double)(py[j] * (a.h - 1)) / (double)(a.H - 1);
      x0[j] = min((int)floor(u), a.w - 1);
      y0[j] = min((int)floor(v), a.h - 1);
      x1[j] = min(x0[j] + 1, a.w - 1);
      y1[j] = min(y0[j] + 1, a.h - 1);
      fx[j] = u - (double)x0[j];
      fy[j] = v - (double)y0[j];
    }
    const size_t hw = (size_t)a.h * a.w;
    const float *map = a.heat + (size_t)b * a.K * hw;
    for (int k = 0; k < a.K; ++k, map += hw) {
#pragma unroll
      for (int j = 0; j < VIZ_PPT; ++j) {
        if (j >= nvalid || (covered >> j & 1u)) continue;
        float v;
        if (same) {
          v = map[p0 + j];
        } else {
          const double a00 = map[(size_t)y0[j] * a.w + x0[j]], a01 = map[(size_t)y0[j] * a.w + x1[j]];
          const double a10 = map[(size_t)y1[j] * a.w + x0[j]], a11 = map[(size_t)y1[j] * a.w + x1[j]];
          v = (float)((a00 * (1.0 - fx[j]) + a01 * fx[j]) * (1.0 - fy[j]) +
                      (a10 * (1.0 - fx[j]) + a11 * fx[j]) * fy[j]);
        }
        if (v < 0.01f) continue;                       // NaN is not less: it reaches the all-zero "bad" colour
        const int row = viz_lut_row(v);
        if (row < 0) continue;
        acc[j][0] += s_lut[3 * row];
        acc[j][1] += s_lut[3 * row + 1];
        acc[j][2] += s_lut[3 * row + 2];
      }
    }
#pragma unroll
    for (int j = 0; j < VIZ_PPT; ++j)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        double s = acc[j][ch] * 255.0;
        s = s < 255.0 ? s : 255.0;
        rgb[3 * j + ch] = (unsigned)min(255, (int)rgb[3 * j + ch] + (int)s);
      }
  }
#pragma unroll
  for (int j = 0; j < VIZ_PPT; ++j)
    if (covered >> j & 1u) {
      rgb[3 * j] = col[j] & 255u;
      rgb[3 * j + 1] = col[j] >> 8 & 255u;
      rgb[3 * j + 2] = col[j] >> 16 & 255u;
    }

  unsigned char *dst = a.out + pix * 3;
  if (whole) {
    unsigned *d4 = reinterpret_cast<unsigned *>(dst);
#pragma unroll
    for (int i = 0; i < 3; ++i)
      d4[i] = rgb[4 * i] | rgb[4 * i + 1] << 8 | rgb[4 * i + 2] << 16 | rgb[4 * i + 3] << 24;
  } else {
#pragma unroll
    for (int i = 0; i < 3 * VIZ_PPT; ++i)
      if (i < 3 * nvalid) dst[i] = (unsigned char)rgb[i];
  }
}

__global__ __launch_bounds__(VIZ_THREADS) void viz_colorize_kernel(const float *__restrict__ maps,
                                                                   unsigned char *__restrict__ out, const int hw,
                                                                   const double *__restrict__ lut, const int normalize,
                                                                   const int dwords) {
  __shared__ unsigned s_rgba[256];
  __shared__ float s_max[VIZ_THREADS / 64];
  __shared__ int s_nan[VIZ_THREADS / 64];
  const int tid = threadIdx.x;
  const float *src = maps + (size_t)blockIdx.x * hw;
  unsigned char *dst = out + (size_t)blockIdx.x * hw * 4;
  {
    unsigned word = 255u << 24;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) word |= (unsigned)(int)(lut[3 * tid + ch] * 255.0) << (8 * ch);
    s_rgba[tid] = word;
  }
  float mx = 1.0f;
  if (normalize) {                                     // numpy's max: NaN as soon as one element is NaN
    float m = -INFINITY;
    int nan = 0;
    for (int i = tid; i < hw; i += VIZ_THREADS) {
      const float v = src[i];
      nan |= v != v;
      m = v > m ? v : m;
    }
    m = wave_max(m);
    nan = __any(nan);
    if ((tid & 63) == 0) s_max[tid >> 6] = m, s_nan[tid >> 6] = nan;
  }
  __syncthreads();
  if (normalize) {
    mx = s_max[0];
    int nan = s_nan[0];
#pragma unroll
    for (int v = 1; v < VIZ_THREADS / 64; ++v) {
      mx = s_max[v] > mx ? s_max[v] : mx;
      nan |= s_nan[v];
    }
    if (nan) mx = __builtin_nanf("");
  }
  for (int i = tid; i < hw; i += VIZ_THREADS) {
    float v = src[i];
    if (normalize) v = v / mx;
    const int row = viz_lut_row(v);
    const unsigned word = row < 0 ? 0u : s_rgba[row];
    if (dwords) {
      reinterpret_cast<unsigned *>(dst)[i] = word;
    } else {
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) dst[4 * (size_t)i + ch] = (unsigned char)(word >> (8 * ch));
    }
  }
}

static bool viz_overlap(const void *a, long long a_bytes, const void *b, long long b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

static bool viz_aligned4(const void *p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace pp

extern "C" int pp_viz_render(const void *image, int image_f32chw, void *out, int B, int H, int W, const float *heat,
                             int K, int h, int w, const double *lut, const double *kpts, const double *probs,
                             const int *inst, const int *img_off, int N, int Kp, const int *style, int L,
                             double threshold, int radius, int line_width, void *stream) {
  using namespace pp;
  PP_REQUIRE(image && out, "pp_viz_render: null image or out");
  PP_REQUIRE(image_f32chw == 0 || image_f32chw == 1, "pp_viz_render: image_f32chw=%d", image_f32chw);
  PP_REQUIRE(B > 0 && H > 0 && W > 0, "pp_viz_render: sizes must be positive, got B=%d H=%d W=%d", B, H, W);
  PP_REQUIRE(H <= PP_VIZ_MAX_SIDE && W <= PP_VIZ_MAX_SIDE, "pp_viz_render: a %d x %d image is larger than %d a side", H,
             W, PP_VIZ_MAX_SIDE);
  const long long HW = (long long)H * W, tiles = cdiv(HW, VIZ_TILE);
  PP_REQUIRE(tiles * B < (1ll << 31), "pp_viz_render: %d images of %d x %d exceed one grid", B, H, W);
  const long long out_bytes = 3 * HW * B, in_bytes = image_f32chw ? 4 * out_bytes : out_bytes;
  PP_REQUIRE((!image_f32chw && image == out) || !viz_overlap(image, in_bytes, out, out_bytes),
             "pp_viz_render: out aliases the image partly (only out == a uint8 image is in-place use)");
  if (heat) {
    PP_REQUIRE(lut, "pp_viz_render: heat maps without a colour table");
    PP_REQUIRE(K > 0 && h > 0 && w > 0, "pp_viz_render: map sizes must be positive, got K=%d h=%d w=%d", K, h, w);
    PP_REQUIRE(h <= PP_VIZ_MAX_SIDE && w <= PP_VIZ_MAX_SIDE, "pp_viz_render: a %d x %d map is larger than %d a side", h,
               w, PP_VIZ_MAX_SIDE);
    PP_REQUIRE(!viz_overlap(heat, 4ll * B * K * h * w, out, out_bytes), "pp_viz_render: out aliases the heat maps");
  }
  if (kpts) {
    PP_REQUIRE(probs && inst && img_off && style, "pp_viz_render: keypoints without probabilities, instance order, "
                                                   "image offsets or style table");
    PP_REQUIRE(N >= 0 && Kp > 0 && L >= 0, "pp_viz_render: N=%d Kp=%d L=%d", N, Kp, L);
    PP_REQUIRE((long long)N * Kp < (1ll << 31) && (long long)N * L < (1ll << 31),
               "pp_viz_render: %d instances of %d keypoints and %d limbs exceed the 2^31 the index arithmetic holds", N,
               Kp, L);
    PP_REQUIRE(threshold == threshold, "pp_viz_render: threshold is not a number");
    PP_REQUIRE(radius >= 0 && radius <= PP_VIZ_MAX_SIDE, "pp_viz_render: radius=%d is outside 0..%d", radius,
               PP_VIZ_MAX_SIDE);
    PP_REQUIRE(line_width >= 1 && line_width <= PP_VIZ_MAX_SIDE, "pp_viz_render: line_width=%d is outside 1..%d",
               line_width, PP_VIZ_MAX_SIDE);
    PP_REQUIRE(!viz_overlap(kpts, 16ll * N * Kp, out, out_bytes) && !viz_overlap(probs, 8ll * N * Kp, out, out_bytes),
               "pp_viz_render: out aliases the keypoints or the probabilities");
  }
  const VizRender a = {image, (unsigned char *)out, image_f32chw, B,   H,   W,      heat,  K,         h,      w, lut,
                       kpts,  probs,                inst,         img_off, style, N,   Kp,  L,      threshold, radius,
                       line_width};
  const bool vec = viz_aligned4(out) && (image_f32chw || viz_aligned4(image)) && (B == 1 || HW % 4 == 0);
  const dim3 grid((unsigned)(tiles * B)), block(VIZ_THREADS);
  if (vec) hipLaunchKernelGGL(viz_render_kernel<true>, grid, block, 0, (hipStream_t)stream, a, (int)tiles);
  else hipLaunchKernelGGL(viz_render_kernel<false>, grid, block, 0, (hipStream_t)stream, a, (int)tiles);
  PP_CHECK_LAUNCH("viz_render_kernel");
  return 0;
}

extern "C" int pp_viz_colorize(const float *maps, void *out, long long M, int h, int w, const double *lut,
                               int normalize, void *stream) {
  using namespace pp;
  PP_REQUIRE(M >= 0, "pp_viz_colorize: M=%lld", M);
  PP_REQUIRE(h > 0 && w > 0 && (long long)h * w < (1ll << 29), "pp_viz_colorize: h=%d w=%d", h, w);
  PP_REQUIRE(M < (1ll << 31), "pp_viz_colorize: M=%lld maps exceed one grid", M);
  if (M == 0) return 0;
  PP_REQUIRE(maps && out && lut, "pp_viz_colorize: null pointer");
  PP_REQUIRE(!viz_overlap(maps, 4ll * M * h * w, out, 4ll * M * h * w), "pp_viz_colorize: out aliases the maps");
  hipLaunchKernelGGL(viz_colorize_kernel, dim3((unsigned)M), dim3(VIZ_THREADS), 0, (hipStream_t)stream, maps,
                     (unsigned char *)out, h * w, lut, normalize != 0, (int)viz_aligned4(out));
  PP_CHECK_LAUNCH("viz_colorize_kernel");
  return 0;
}
