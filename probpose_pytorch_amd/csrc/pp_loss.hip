// The validation loss of the reference (loss.py:18-712) on the device, forward only.
//
// pp_oks_heatmap_loss   OKSHeatmapLoss.forward (loss.py:55-143): one workgroup per (crop, keypoint) map.  The map of
//                       `output` is staged tile by tile in LDS with a one-pixel zero halo (the 'same' padding of the
//                       Sobel F.conv2d, loss.py:106-110), so every input element is read from HBM once; at the
//                       benchmark map sizes (64x48, 96x72) one tile is the whole map.  Each workgroup writes the
//                       optional per-pixel loss and five per-map partials; a one-workgroup finish kernel turns those
//                       into the per-keypoint loss and the two means.
// pp_probpose_loss_terms everything else ProbPoseLoss.forward (loss.py:360-510) computes from the B*K keypoints: the
//                       per-keypoint OKS of _oks_from_heatmaps (loss.py:550-640) in float64, the error target of
//                       _error_from_heatmaps (:512-548), the visibility weights (:436-450), the four small losses and
//                       the two MAE accuracies (:699-712).  One workgroup: the batch-wide counts the visibility
//                       weights need are block reductions, no second launch.
//
// Every reduction has a fixed shape (fixed lane -> element assignment, xor-butterfly wave sums, waves combined in
// order by one lane), and there are no float atomics: repeated calls return identical bits.
#include <math.h>

#include "pp_common.h"

namespace pp {

constexpr int HL_THREADS = 256;
constexpr int HL_TILE = 8192;        // LDS floats of one output tile incl. halo (32 KiB)
constexpr int HL_MAX_COLS = 512;     // tile width cap: (HL_TILE / (512 + 2)) - 2 = 13 rows still fit
constexpr int HL_PARTS = 5;          // per map: oks sum, max gradient, mse sum, per-pixel loss sum, #target outside [0,1]

// torch.max semantics: a NaN is the maximum and stays it
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

template <int WAVES>
__device__ __forceinline__ float block_sum_f(float v, float *lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = lds[0];
  for (int w = 1; w < WAVES; ++w) s += lds[w];
  return s;
}

template <int WAVES>
__device__ __forceinline__ double block_sum_d(double v, double *lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = lds[0];
  for (int w = 1; w < WAVES; ++w) s += lds[w];
  return s;
}

template <int WAVES>
__device__ __forceinline__ float block_max_f(float v, float *lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = lds[0];
  for (int w = 1; w < WAVES; ++w) s = nan_max(s, lds[w]);
  return s;
}

template <int WAVES>
__device__ __forceinline__ double block_min_pos_d(double v, double *lds) {   // min over v > 0; +inf when none
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = lds[0];
  for (int w = 1; w < WAVES; ++w) s = fmin(s, lds[w]);
  return s;
}

// ---------------------------------------------------------------------------------------------------- heatmap loss
// output / target [B,K,H,W]; weights [B,K] (per keypoint) or [B,K,H,W] (weights_per_pixel); mask at
// mask + b * mask_sb + k * mask_sk, [H,W] per map.  parts [B*K][HL_PARTS].
__global__ __launch_bounds__(HL_THREADS) void oks_heatmap_loss_kernel(
    const float *__restrict__ output, const float *__restrict__ target, const float *__restrict__ weights,
    int weights_per_pixel, const float *__restrict__ mask, long long mask_sb, long long mask_sk, int skip_empty,
    int oks_type, float sw, float ow, float gw, float lw, int K, int H, int W, int tile_rows, int tile_cols,
    float *__restrict__ per_pixel, float *__restrict__ parts) {
  __shared__ float tile[HL_TILE];
  __shared__ float red[HL_THREADS / 64];
  const long long map = blockIdx.x;
  const int b = (int)(map / K), k = (int)(map - (long long)b * K);
  const long long HW = (long long)H * W;
  const float *o = output + map * HW, *t = target + map * HW;
  const float *pw = (weights && weights_per_pixel) ? weights + map * HW : nullptr;
  const float kw = (weights && !weights_per_pixel) ? weights[map] : 1.0f;
  const float *sm = mask ? mask + b * mask_sb + k * mask_sk : nullptr;
  float nonempty = 1.0f;
  if (skip_empty) {    // loss.py:181-189: (target != 0).flatten(2).any(dim=2)
    int any = 0;
    for (long long i = threadIdx.x; i < HW && !any; i += HL_THREADS) any = t[i] != 0.0f;
    nonempty = __syncthreads_or(any) ? 1.0f : 0.0f;
  }
  float s_oks = 0.0f, s_mse = 0.0f, s_pix = 0.0f, g_max = -__builtin_inff(), bad = 0.0f;
  for (int r0 = 0; r0 < H; r0 += tile_rows) {
    const int br = min(tile_rows, H - r0);
    for (int c0 = 0; c0 < W; c0 += tile_cols) {
      const int bc = min(tile_cols, W - c0), pitch = bc + 2;
      // output rows r0-1 .. r0+br, columns c0-1 .. c0+bc; zero outside the map
      for (int i = threadIdx.x; i < (br + 2) * pitch; i += HL_THREADS) {
        const int r = r0 - 1 + i / pitch, c = c0 - 1 + i % pitch;
        tile[i] = (r >= 0 && r < H && c >= 0 && c < W) ? o[(long long)r * W + c] : 0.0f;
      }
      __syncthreads();
      for (int p = threadIdx.x; p < br * bc; p += HL_THREADS) {
        const int r = p / bc, c = p - r * bc;
        const long long idx = (long long)(r0 + r) * W + (c0 + c);
        const float *a = tile + r * pitch + c;        // a[dr * pitch + dc]: output[r0 + r - 1 + dr][c0 + c - 1 + dc]
        const float ov = a[pitch + 1], tv = t[idx];
        float oks;
        const float om = ov * (1.0f - tv), op = (1.0f - ov) * tv;       // loss.py:92-101
        if (oks_type == 0) oks = om;
        else if (oks_type == 1) oks = op;
        else oks = (om + op) / 2.0f;
        const float d = ov - tv;
        float mse = d * d;                                               // loss.py:103
        // cross-correlation with sobel_x = [[1,0,-1],[2,0,-2],[1,0,-1]], sobel_y = [[1,2,1],[0,0,0],[-1,-2,-1]]
        const float gx = (a[0] - a[2]) + 2.0f * (a[pitch] - a[pitch + 2]) + (a[2 * pitch] - a[2 * pitch + 2]);
        const float gy = (a[0] + 2.0f * a[1] + a[2]) - (a[2 * pitch] + 2.0f * a[2 * pitch + 1] + a[2 * pitch + 2]);
        float grad = gx * gx + gy * gy;
        // mask = spatial mask * keypoint (or pixel) weight * non-empty channel (loss.py:145-191); x * 1 == x
        float m = sm ? sm[idx] : 1.0f;
        m = m * (pw ? pw[idx] : kw);
        m = m * nonempty;
        oks = oks * m;
        mse = mse * m;
        grad = grad * m;
        const float pix = ((sw * grad + ow * oks) + gw * mse) * lw;     // loss.py:122-127, :143
        if (per_pixel) per_pixel[map * HW + idx] = pix;
        s_oks += oks;
        s_mse += mse;
        s_pix += pix;
        g_max = nan_max(g_max, grad);
        bad += (tv >= 0.0f && tv <= 1.0f) ? 0.0f : 1.0f;                // loss.py:85-86
      }
      __syncthreads();
    }
  }
  s_oks = block_sum_f<HL_THREADS / 64>(s_oks, red);
  s_mse = block_sum_f<HL_THREADS / 64>(s_mse, red);
  s_pix = block_sum_f<HL_THREADS / 64>(s_pix, red);
  bad = block_sum_f<HL_THREADS / 64>(bad, red);
  g_max = block_max_f<HL_THREADS / 64>(g_max, red);
  if (threadIdx.x == 0) {
    float *P = parts + map * HL_PARTS;
    P[0] = s_oks;
    P[1] = g_max;
    P[2] = s_mse;
    P[3] = s_pix;
    P[4] = bad;
  }
}

// per_keypoint [B*K] (optional) = lw * (ow * oks sum + sw * max gradient + gw * mse mean)   (loss.py:128-134)
// scalars[0] = mean of that (without lw) * lw  (loss.py:135-143); scalars[1] = mean of the per-pixel loss
// (ProbPoseLoss's heatmap_loss_pxl.mean(), loss.py:431); scalars[2] = #target elements outside [0, 1]
__global__ __launch_bounds__(HL_THREADS) void oks_heatmap_loss_finish_kernel(const float *__restrict__ parts, long long n,
                                                                           long long HW, float sw, float ow, float gw,
                                                                           float lw, float *__restrict__ per_keypoint,
                                                                           float *__restrict__ scalars) {
  __shared__ double red[HL_THREADS / 64];
  double s_kp = 0.0, s_pix = 0.0, bad = 0.0;
  for (long long i = threadIdx.x; i < n; i += HL_THREADS) {
    const float *P = parts + i * HL_PARTS;
    const float kp = (ow * P[0] + sw * P[1]) + gw * (P[2] / (float)HW);
    if (per_keypoint) per_keypoint[i] = kp * lw;
    s_kp += kp;
    s_pix += P[3];
    bad += P[4];
  }
  s_kp = block_sum_d<HL_THREADS / 64>(s_kp, red);
  s_pix = block_sum_d<HL_THREADS / 64>(s_pix, red);
  bad = block_sum_d<HL_THREADS / 64>(bad, red);
  if (threadIdx.x == 0) {
    scalars[0] = (float)(s_kp / (double)n) * lw;
    scalars[1] = (float)(s_pix / ((double)n * (double)HW));
    scalars[2] = (float)bad;
  }
}

// ---------------------------------------------------------------------------------------------------- B*K terms
constexpr int LT_THREADS = 1024;

// torch's binary_cross_entropy element (ATen Loss.cpp / Loss.cu): logs clamped at -100, log1p for 1 - x
__device__ __forceinline__ float bce(float x, float y) {
  const float l0 = fmaxf(logf(x), -100.0f), l1 = fmaxf(log1pf(-x), -100.0f);
  return (y - 1.0f) * l1 - y * l0;
}

// torch smooth_l1_loss element, beta = 1
__device__ __forceinline__ float smooth_l1(float a, float b) {
  const float z = fabsf(a - b);
  return z < 1.0f ? 0.5f * z * z / 1.0f : z - 0.5f * 1.0f;
}

__global__ __launch_bounds__(LT_THREADS) void probpose_loss_terms_kernel(
    const double *__restrict__ gt_kpts, const double *__restrict__ dt_kpts, const int *__restrict__ in_image,
    const int *__restrict__ annotated, const int *__restrict__ visibility, const float *__restrict__ dt_prob,
    const float *__restrict__ dt_vis, const float *__restrict__ dt_oks, const float *__restrict__ dt_err,
    const double *__restrict__ variance, double oks_area, int B, int K, int freeze_error, float *__restrict__ gt_oks,
    float *__restrict__ gt_err, float *__restrict__ vis_weight, float *__restrict__ oks_weight,
    float *__restrict__ results) {
  __shared__ double red[LT_THREADS / 64];
  const long long N = (long long)B * K;
  // (1) per crop: does it hold a keypoint with weight = in_image & annotated > 0 (loss.py:602-607); batch-wide
  //     counts of annotated invisible / visible keypoints (loss.py:437-438)
  for (int b = threadIdx.x; b < B; b += LT_THREADS) {
    int any = 0;
    for (int k = 0; k < K; ++k) any |= (in_image[(long long)b * K + k] & annotated[(long long)b * K + k]) > 0;
    oks_weight[b] = any ? 1.0f : 0.0f;
  }
  double n_inv = 0.0, n_vis = 0.0;
  for (long long i = threadIdx.x; i < N; i += LT_THREADS) {
    const bool ann = annotated[i] > 0;
    n_inv += (ann && visibility[i] == 0) ? 1.0 : 0.0;
    n_vis += (ann && visibility[i] > 0) ? 1.0 : 0.0;
  }
  n_inv = block_sum_d<LT_THREADS / 64>(n_inv, red);
  n_vis = block_sum_d<LT_THREADS / 64>(n_vis, red);     // block_sum_d's barriers also publish oks_weight
  // torch: 1 / (int_tensor.sum() + 1e-10) is float32
  const float w_inv = 1.0f / ((float)n_inv + 1e-10f), w_vis = 1.0f / ((float)n_vis + 1e-10f);

  // (2) per keypoint
  double s_prob = 0.0, s_vis = 0.0, s_oks = 0.0, s_err = 0.0, mae_oks = 0.0, mae_err = 0.0, n_ann = 0.0;
  double w_min = __builtin_inf();
  int flags = 0;
  for (long long i = threadIdx.x; i < N; i += LT_THREADS) {
    const int b = (int)(i / K), k = (int)(i - (long long)b * K);
    const int w = in_image[i] & annotated[i];
    const double wd = (double)w;
    double o = 0.0;
    if (oks_weight[b] != 0.0f && w * 2 > 0) {
      // gt NaN -> 0 (loss.py:588), both * weight (:591-592); dt is never cleaned
      double gx = gt_kpts[2 * i], gy = gt_kpts[2 * i + 1];
      gx = (gx != gx) ? 0.0 : gx;
      gy = (gy != gy) ? 0.0 : gy;
      const double dx = dt_kpts[2 * i] * wd - gx * wd, dy = dt_kpts[2 * i + 1] * wd - gy * wd;
      o = exp(-((dx * dx + dy * dy) / variance[k] / oks_area / 2.0));   // compute_oks, use_area=False (loss.py:751-752)
    }
    const float go = (float)o;
    gt_oks[i] = go;
    float ge = 0.0f;
    if (!freeze_error) {                                                 // loss.py:540-548
      double gx = gt_kpts[2 * i], gy = gt_kpts[2 * i + 1];
      gx = (gx != gx) ? -1.0 : gx;
      gy = (gy != gy) ? -1.0 : gy;
      const double ex = gx - dt_kpts[2 * i], ey = gy - dt_kpts[2 * i + 1];
      const double e = sqrt(ex * ex + ey * ey);
      if (!(e >= 0.0)) flags |= 2;
      ge = (float)e;
    }
    gt_err[i] = ge;
    const int ann_in = annotated[i] & (in_image[i] > 0);                 // loss.py:419
    const float ai = (float)ann_in;
    // visibility weights (loss.py:439-445): annotated_in, then the invisible / visible annotated overwritten
    float vw = ai;
    if (annotated[i] > 0) vw = visibility[i] == 0 ? w_inv : w_vis;
    vis_weight[i] = vw;
    if (vw > 0.0f) w_min = fmin(w_min, (double)vw);
    const float xp = dt_prob[i], xv = dt_vis[i];
    if (!(xp >= 0.0f && xp <= 1.0f) || !(xv >= 0.0f && xv <= 1.0f)) flags |= 4;
    s_prob += bce(xp, (float)in_image[i]);
    s_vis += bce(xv, (float)visibility[i]);
    const float dq = dt_oks[i] * ai - go * ai;                           // MSELoss with target weight (loss.py:288)
    s_oks += dq * dq;
    // L1LogLoss: log(1 + x) in float32, not log1p (loss.py:325-326), weighted, smooth-L1 (:335)
    const float la = logf(1.0f + dt_err[i]), lb = logf(1.0f + ge);
    s_err += smooth_l1(la * ai, lb * ai);
    if (ann_in) {                                                        // get_mae (loss.py:699-712)
      mae_oks += fabsf(dt_oks[i] - go);
      mae_err += fabsf(dt_err[i] - ge);
      n_ann += 1.0;
    }
  }
  w_min = block_min_pos_d<LT_THREADS / 64>(w_min, red);
  if (!(w_min < __builtin_inf())) flags |= 1;                            // loss.py:448: min() of an empty tensor
  // (3) normalise the visibility weights by their smallest positive value, in float64 (loss.py:446-450)
  for (long long i = threadIdx.x; i < N; i += LT_THREADS) vis_weight[i] = (float)((double)vis_weight[i] / w_min);
  s_prob = block_sum_d<LT_THREADS / 64>(s_prob, red);
  s_vis = block_sum_d<LT_THREADS / 64>(s_vis, red);
  s_oks = block_sum_d<LT_THREADS / 64>(s_oks, red);
  s_err = block_sum_d<LT_THREADS / 64>(s_err, red);
  mae_oks = block_sum_d<LT_THREADS / 64>(mae_oks, red);
  mae_err = block_sum_d<LT_THREADS / 64>(mae_err, red);
  n_ann = block_sum_d<LT_THREADS / 64>(n_ann, red);
  __shared__ int flag_bits;                                               // integer OR: order-free
  if (threadIdx.x == 0) flag_bits = 0;
  __syncthreads();
  if (flags) atomicOr(&flag_bits, flags);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = (double)N;
    results[0] = (float)(s_prob / n);
    results[1] = (float)(s_vis / n);
    results[2] = (float)(s_oks / n);
    results[3] = (float)(s_err / n);
    results[4] = (float)(mae_oks / n_ann);     // no annotated keypoint in the image: 0 / 0 = NaN, like numpy's mean
    results[5] = (float)(mae_err / n_ann);
    results[6] = (float)flag_bits;
    results[7] = (float)n_ann;
  }
}

}  // namespace pp

extern "C" int pp_oks_heatmap_loss(const float *output, const float *target, const float *weights,
                                   int weights_per_pixel, const float *mask, long long mask_sb, long long mask_sk,
                                   int skip_empty, int oks_type, float smoothing_weight, float oks_weight,
                                   float gaussian_weight, float loss_weight, int B, int K, int H, int W,
                                   float *per_pixel, float *per_keypoint, float *parts, float *scalars,
                                   void *stream) {
  using namespace pp;
  PP_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0, "pp_oks_heatmap_loss: bad shape B=%d K=%d H=%d W=%d", B, K, H, W);
  PP_REQUIRE((long long)B * K < (1ll << 31), "pp_oks_heatmap_loss: too many maps");
  PP_REQUIRE(oks_type >= 0 && oks_type <= 2, "pp_oks_heatmap_loss: oks_type %d is not minus (0), plus (1), both (2)",
             oks_type);
  PP_REQUIRE(output && target && parts && scalars, "pp_oks_heatmap_loss: null operand");
  PP_REQUIRE(mask_sb >= 0 && mask_sk >= 0, "pp_oks_heatmap_loss: negative mask stride");
  const int cols = W < HL_MAX_COLS ? W : HL_MAX_COLS;
  int rows = HL_TILE / (cols + 2) - 2;
  rows = rows < H ? rows : H;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(oks_heatmap_loss_kernel, dim3((unsigned)(B * K)), dim3(HL_THREADS), 0, s, output, target,
                     weights, weights_per_pixel, mask, mask_sb, mask_sk, skip_empty, oks_type, smoothing_weight,
                     oks_weight, gaussian_weight, loss_weight, K, H, W, rows, cols, per_pixel, parts);
  PP_CHECK_LAUNCH("oks_heatmap_loss_kernel");
  hipLaunchKernelGGL(oks_heatmap_loss_finish_kernel, dim3(1), dim3(HL_THREADS), 0, s, (const float *)parts,
                     (long long)B * K, (long long)H * W, smoothing_weight, oks_weight, gaussian_weight, loss_weight,
                     per_keypoint, scalars);
  PP_CHECK_LAUNCH("oks_heatmap_loss_finish_kernel");
  return 0;
}

extern "C" int pp_probpose_loss_terms(const double *gt_kpts, const double *dt_kpts, const int *in_image,
                                      const int *annotated, const int *visibility, const float *dt_prob,
                                      const float *dt_vis, const float *dt_oks, const float *dt_err,
                                      const double *variance, double oks_area, int B, int K, int freeze_error,
                                      float *gt_oks, float *gt_err, float *vis_weight, float *oks_weight,
                                      float *results, void *stream) {
  using namespace pp;
  PP_REQUIRE(B > 0 && K > 0 && (long long)B * K < (1ll << 31), "pp_probpose_loss_terms: bad shape B=%d K=%d", B, K);
  PP_REQUIRE(gt_kpts && dt_kpts && in_image && annotated && visibility && dt_prob && dt_vis && dt_oks && dt_err &&
                 variance && gt_oks && gt_err && vis_weight && oks_weight && results,
             "pp_probpose_loss_terms: null operand");
  hipLaunchKernelGGL(probpose_loss_terms_kernel, dim3(1), dim3(LT_THREADS), 0, (hipStream_t)stream, gt_kpts, dt_kpts,
                     in_image, annotated, visibility, dt_prob, dt_vis, dt_oks, dt_err, variance, oks_area, B, K,
                     freeze_error, gt_oks, gt_err, vis_weight, oks_weight, results);
  PP_CHECK_LAUNCH("probpose_loss_terms_kernel");
  return 0;
}
