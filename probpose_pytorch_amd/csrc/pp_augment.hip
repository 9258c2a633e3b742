// Augmented training batches on the GPU: one affine bilinear warp for the whole batch and the matching keypoint path.
// Counterpart of pp_frontend.hip's multi-source launch + pp_dataset.hip for YOLOPoseDataset(augment=Augment(...)):
// random flip, box scale, rotation, shift and a brightness / contrast step, where the un-augmented path has Pillow's
// separable LANCZOS resize (which cannot rotate).  The host folds the geometry of DESIGN §4.4c into two 2x3 matrices
// per sample; the kernels only apply them.
//
// augment_warp_kernel, per output pixel (u, v) of sample b, record m = warp[b] (8 float64: m00 m01 m02 m10 m11 m12 c b):
//   x = (m00 * u + m01 * v) + m02,  y = (m10 * u + m11 * v) + m12      float64, in this order, nothing fused:
//                                                                      the region's pixel-index coordinates (pixel
//                                                                      (i, j) has its centre at (i, j))
//   x0 = floor(x), fx = float32(x - x0), likewise y                    the four taps (x0, y0) .. (x0 + 1, y0 + 1)
//   wx1 = fx, wx0 = 1 - fx, wy1 = fy, wy0 = 1 - fy                     float32
//   top = p00 * wx0 + p01 * wx1,  bot = p10 * wx0 + p11 * wx1          float32; a tap outside the region is 0
//   val = top * wy0 + bot * wy1;  val = val / 255
//   out = min(max(float32(c) * val + float32(b), 0), 1)
// The taps are read bytewise and only inside the region's rows, so no load can leave the packed buffer whatever the
// matrix is.  A thread computes 4 consecutive u of one row for the three channels (the coordinates and weights are
// shared by the channels) and writes one 128-bit store per channel; lane i of a wave holds u = 4 i .. 4 i + 3, rows
// follow each other in NCHW, so every store instruction of a wave covers 1 KiB of consecutive addresses.
//
// dataset_gt_affine_kernel: pp_dataset.hip's dataset_gt_kernel with the box arithmetic replaced by
//   x = (a00 * kx + a01 * ky) + a02,  y = (a10 * kx + a11 * ky) + a12  float32, in this order, nothing fused
// and, for a flipped sample, output slot k reading source keypoint perm[k] (coordinates and visibility).
#include "pp_common.h"

#include <math.h>

namespace pp {

template <int V>
__global__ __launch_bounds__(256) void augment_warp_kernel(const unsigned char *__restrict__ src,
                                                           const long long *__restrict__ sources,
                                                           const double *__restrict__ warp, int n_threads, int in_w,
                                                           int in_h, float *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_threads) return;
  const int per_row = in_w / V;
  const int u0 = (i % per_row) * V, row = i / per_row, v = row % in_h, b = row / in_h;
  const long long off = sources[4 * b], sw = sources[4 * b + 1], sh = sources[4 * b + 2], st = sources[4 * b + 3];
  const double *m = warp + 8 * b;
  const double m00 = m[0], m02 = m[2], m10 = m[3], m12 = m[5];
  const float c = (float)m[6], bias = (float)m[7];
  const double rx = m[1] * (double)v, ry = m[4] * (double)v;
  const unsigned char *base = src + off;
  float res[3][V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const double du = (double)(u0 + j);
    double x = m00 * du;
    x = x + rx;
    x = x + m02;
    double y = m10 * du;
    y = y + ry;
    y = y + m12;
    const double xf = floor(x), yf = floor(y);
    const float fx = (float)(x - xf), fy = (float)(y - yf);
    const float wx1 = fx, wx0 = 1.0f - fx, wy1 = fy, wy0 = 1.0f - fy;
    // compared in float64 before any conversion: a coordinate far outside (or not a number) has no tap inside
    const bool x0in = xf >= 0.0 && xf <= (double)(sw - 1), x1in = xf >= -1.0 && xf <= (double)(sw - 2);
    const bool y0in = yf >= 0.0 && yf <= (double)(sh - 1), y1in = yf >= -1.0 && yf <= (double)(sh - 2);
    const long long c0 = x0in ? 3 * (long long)xf : 0, c1 = x1in ? 3 * ((long long)xf + 1) : 0;
    const long long r0 = y0in ? (long long)yf * st : 0, r1 = y1in ? ((long long)yf + 1) * st : 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float p00 = (x0in && y0in) ? (float)base[r0 + c0 + ch] : 0.0f;
      const float p01 = (x1in && y0in) ? (float)base[r0 + c1 + ch] : 0.0f;
      const float p10 = (x0in && y1in) ? (float)base[r1 + c0 + ch] : 0.0f;
      const float p11 = (x1in && y1in) ? (float)base[r1 + c1 + ch] : 0.0f;
      const float top = p00 * wx0 + p01 * wx1;
      const float bot = p10 * wx0 + p11 * wx1;
      float val = top * wy0 + bot * wy1;
      val = val / 255.0f;
      val = c * val + bias;
      res[ch][j] = fminf(fmaxf(val, 0.0f), 1.0f);
    }
  }
  const size_t plane = (size_t)in_h * in_w;
  float *o = out + (size_t)b * 3 * plane + (size_t)v * in_w + u0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    if constexpr (V == 4) {
      *reinterpret_cast<float4 *>(o + ch * plane) = make_float4(res[ch][0], res[ch][1], res[ch][2], res[ch][3]);
    } else {
      o[ch * plane] = res[ch][0];
    }
  }
}

__global__ __launch_bounds__(256) void dataset_gt_affine_kernel(const float *__restrict__ kpts_raw,
                                                                const float *__restrict__ affine,
                                                                const int *__restrict__ perm, int n, int K, float in_w,
                                                                float in_h, float scale_x, float scale_y,
                                                                float *__restrict__ kpts_crop,
                                                                float *__restrict__ kpts_hm,
                                                                float *__restrict__ encode_visible,
                                                                unsigned char *__restrict__ in_image,
                                                                unsigned char *__restrict__ visible,
                                                                float *__restrict__ visibility) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = i / K, k = i - b * K;
  const float *a = affine + 8 * b;
  int s = a[6] != 0.0f ? perm[k] : k;
  if ((unsigned)s >= (unsigned)K) s = k;       // the host has checked the permutation; never index outside the sample
  const float *kp = kpts_raw + 3 * ((size_t)b * K + s);
  const float kx = kp[0], ky = kp[1], v = kp[2];
  float x = a[0] * kx + a[1] * ky;
  x = x + a[2];
  float y = a[3] * kx + a[4] * ky;
  y = y + a[5];
  kpts_crop[2 * i] = x;
  kpts_crop[2 * i + 1] = y;
  kpts_hm[2 * i] = x / scale_x;
  kpts_hm[2 * i + 1] = y / scale_y;
  const bool vis = v == 2.0f;
  encode_visible[i] = vis ? 1.0f : 0.0f;
  visible[i] = vis ? 1 : 0;
  visibility[i] = v < 1.0f ? v : 1.0f;     // np.minimum(v, 1)
  in_image[i] = (x >= 0.0f && x < in_w && y >= 0.0f && y < in_h) ? 1 : 0;
}

static bool finite_all(const double *p, int n) {
  for (int i = 0; i < n; ++i)
    if (!isfinite(p[i]) || fabs(p[i]) > 1e12) return false;
  return true;
}

static bool singular(double a, double b, double c, double d) {
  const double det = a * d - b * c;
  return !(fabs(det) > 1e-12 * (fabs(a) + fabs(b)) * (fabs(c) + fabs(d)));
}

}  // namespace pp

extern "C" int pp_augment_check(int n, const long long *sources, long long src_bytes, const double *warp,
                                const float *kp_affine, int K, const int *perm) {
  using namespace pp;
  const char *who = "pp_augment_check";
  PP_REQUIRE(n >= 0 && src_bytes >= 0 && K > 0 && perm && (n == 0 || (sources && warp && kp_affine)),
             "%s: bad arguments", who);
  for (int k = 0; k < K; ++k) {
    PP_REQUIRE(perm[k] >= 0 && perm[k] < K, "%s: the permutation sends keypoint %d to %d, outside 0..%d", who, k,
               perm[k], K - 1);
    PP_REQUIRE(perm[perm[k]] == k, "%s: the permutation is not an involution (%d -> %d -> %d)", who, k, perm[k],
               perm[perm[k]]);
  }
  for (int c = 0; c < n; ++c) {
    const long long off = sources[4 * c], sw = sources[4 * c + 1], sh = sources[4 * c + 2], st = sources[4 * c + 3];
    PP_REQUIRE(sw > 0 && sh > 0 && sw < (1ll << 28) && sh < (1ll << 31) && st >= 3 * sw && st < (1ll << 40),
               "%s: source %d is %lld x %lld with a row stride of %lld bytes", who, c, sw, sh, st);
    PP_REQUIRE(off >= 0 && off % PP_FRONTEND_SRC_ALIGN == 0,
               "%s: source %d starts at byte %lld, not a multiple of %d (misaligned)", who, c, off,
               PP_FRONTEND_SRC_ALIGN);
    PP_REQUIRE(off + (sh - 1) * st + 3 * sw + PP_FRONTEND_SRC_PAD <= src_bytes,
               "%s: source %d (bytes %lld to %lld, plus %d of padding) reaches past the end of the %lld-byte buffer",
               who, c, off, off + (sh - 1) * st + 3 * sw, PP_FRONTEND_SRC_PAD, src_bytes);
    const double *m = warp + 8 * c;
    PP_REQUIRE(finite_all(m, 8), "%s: sample %d has a pixel matrix or colour term that is not finite", who, c);
    PP_REQUIRE(!singular(m[0], m[1], m[3], m[4]), "%s: sample %d has a singular pixel matrix", who, c);
    double a[6];
    for (int j = 0; j < 6; ++j) a[j] = (double)kp_affine[8 * c + j];
    PP_REQUIRE(finite_all(a, 6), "%s: sample %d has a keypoint matrix that is not finite", who, c);
    PP_REQUIRE(!singular(a[0], a[1], a[3], a[4]), "%s: sample %d has a singular keypoint matrix", who, c);
    PP_REQUIRE(kp_affine[8 * c + 6] == 0.0f || kp_affine[8 * c + 6] == 1.0f,
               "%s: sample %d has a flip flag that is neither 0 nor 1", who, c);
  }
  return 0;
}

extern "C" int pp_augment_warp(const unsigned char *src, const long long *sources, const double *warp, int n, int in_w,
                               int in_h, float *out, void *stream) {
  using namespace pp;
  PP_REQUIRE(n >= 0 && in_w > 0 && in_h > 0 && (long long)(n > 0 ? n : 1) * in_w * in_h < (1ll << 31),
             "pp_augment_warp: bad shape");
  if (n == 0) return 0;
  PP_REQUIRE(src && sources && warp && out, "pp_augment_warp: null pointer");
  PP_REQUIRE(reinterpret_cast<uintptr_t>(sources) % 8 == 0 && reinterpret_cast<uintptr_t>(warp) % 8 == 0,
             "pp_augment_warp: the source records and matrices are not 8-byte aligned");
  if (in_w % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0) {
    const int n_threads = (int)((long long)n * in_h * (in_w / 4));
    hipLaunchKernelGGL(augment_warp_kernel<4>, dim3((unsigned)cdiv(n_threads, 256)), dim3(256), 0, (hipStream_t)stream,
                       src, sources, warp, n_threads, in_w, in_h, out);
  } else {
    const int n_threads = n * in_h * in_w;
    hipLaunchKernelGGL(augment_warp_kernel<1>, dim3((unsigned)cdiv(n_threads, 256)), dim3(256), 0, (hipStream_t)stream,
                       src, sources, warp, n_threads, in_w, in_h, out);
  }
  PP_CHECK_LAUNCH("augment_warp_kernel");
  return 0;
}

extern "C" int pp_dataset_ground_truth_affine(const float *kpts_raw, const float *kp_affine, const int *perm, int B,
                                              int K, int in_w, int in_h, float scale_x, float scale_y,
                                              float *kpts_crop, float *kpts_hm, float *encode_visible,
                                              unsigned char *in_image, unsigned char *keypoints_visible,
                                              float *keypoints_visibility, void *stream) {
  using namespace pp;
  PP_REQUIRE(B >= 0 && K > 0 && in_w > 0 && in_h > 0 && in_w < (1 << 24) && in_h < (1 << 24) &&
                 (long long)B * K < (1ll << 30),
             "pp_dataset_ground_truth_affine: bad shape");
  if (B == 0) return 0;
  PP_REQUIRE(kpts_raw && kp_affine && perm && kpts_crop && kpts_hm && encode_visible && in_image &&
                 keypoints_visible && keypoints_visibility,
             "pp_dataset_ground_truth_affine: null pointer");
  const int n = B * K;
  hipLaunchKernelGGL(dataset_gt_affine_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     kpts_raw, kp_affine, perm, n, K, (float)in_w, (float)in_h, scale_x, scale_y, kpts_crop, kpts_hm,
                     encode_visible, in_image, keypoints_visible, keypoints_visibility);
  PP_CHECK_LAUNCH("dataset_gt_affine_kernel");
  return 0;
}
