// The losses of the reference (loss.py:18-712) on the device, and their gradients.
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
// pp_oks_heatmap_loss_backward   d/d output of the three OKSHeatmapLoss reductions for an arbitrary upstream gradient,
//                       one workgroup per map.  Per pixel, the Sobel term reaches a pixel q from the 3x3 neighbours p of
//                       q inside the map, and each needs gx[p], gy[p]: a tile stages `output` with a two-pixel zero halo,
//                       forms G*m*gx and G*m*gy on the tile plus a one-pixel ring (zero where p lies outside the map),
//                       then correlates them with the flipped Sobel kernels.  The per-keypoint and mean reductions put
//                       the max-gradient subgradient at the first maximal pixel of the masked energy (torch's max(dim)).
// pp_probpose_loss_grads d/d prediction of the four small losses of ProbPoseLoss (loss.py:419-464), elementwise.
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
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);   // not wave_sum: that call moves oks_heatmap_loss_kernel's schedule
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = lds[0];
  for (int w = 1; w < WAVES; ++w) s += lds[w];
  return s;
}

template <int WAVES>
__device__ __forceinline__ double block_sum_d(double v, double *lds) {
  v = wave_sum(v);
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


// ---------------------------------------------------------------------------------------------------- backward
constexpr int HB_THREADS = 256;
constexpr int HB_TILE_H = 3584;      // LDS floats of `output` incl. a two-pixel halo (14 KiB)
constexpr int HB_TILE_E = 3328;      // LDS floats of each of G*m*gx, G*m*gy incl. a one-pixel ring (13 KiB)
constexpr int HB_MAX_COLS = 256;     // tile width cap: 3584 / 260 - 4 = 9 rows still fit
// reductions of pp_oks_heatmap_loss_backward (include/probpose_hip.h)
constexpr int HB_PIXEL = 0, HB_KEYPOINT = 1, HB_MEAN = 2, HB_PIXEL_MEAN = 3;

// cross-correlation kernels, [dr + 1][dc + 1]: gx[p] = sum_d SX[d] * h[p + d], so d gx[p] / d h[q] = SX[q - p]
__constant__ float SOBEL_X[3][3] = {{1.0f, 0.0f, -1.0f}, {2.0f, 0.0f, -2.0f}, {1.0f, 0.0f, -1.0f}};
__constant__ float SOBEL_Y[3][3] = {{1.0f, 2.0f, 1.0f}, {0.0f, 0.0f, 0.0f}, {-1.0f, -2.0f, -1.0f}};

// (v1, i1) precedes (v2, i2) in torch's max(dim) order: a NaN beats any number, then the larger value, then the
// earlier pixel
__device__ __forceinline__ bool max_before(float v1, int i1, float v2, int i2) {
  const bool n1 = v1 != v1, n2 = v2 != v2;
  if (n1 != n2) return n1;
  if (!n1 && v1 != v2) return v1 > v2;
  return i1 < i2;
}

// d oks / d output of loss.py:92-101
__device__ __forceinline__ float d_oks(int oks_type, float tv) {
  if (oks_type == 0) return 1.0f - tv;
  if (oks_type == 1) return -tv;
  return ((1.0f - tv) - tv) / 2.0f;
}

// grad (per-pixel reductions): G at g + b * gs[0] + k * gs[1] + r * gs[2] + c * gs[3]; per keypoint: g + b * gs[0]
// + k * gs[1]; mean and pixel mean: g[0].  n_maps = B * K.
__global__ __launch_bounds__(HB_THREADS) void oks_heatmap_loss_backward_kernel(
    const float *__restrict__ output, const float *__restrict__ target, const float *__restrict__ weights,
    int weights_per_pixel, const float *__restrict__ mask, long long mask_sb, long long mask_sk, int skip_empty,
    int oks_type, float sw, float ow, float gw, float lw, int reduction, const float *__restrict__ grad,
    long long gs_b, long long gs_k, long long gs_h, long long gs_w, long long n_maps, int K, int H, int W,
    int tile_rows, int tile_cols, float *__restrict__ grad_output) {
  __shared__ float th[HB_TILE_H];
  __shared__ float tex[HB_TILE_E], tey[HB_TILE_E];
  __shared__ float rv[HB_THREADS / 64];
  __shared__ int ri[HB_THREADS / 64];
  __shared__ float star[2];
  const long long map = blockIdx.x;
  const int b = (int)(map / K), k = (int)(map - (long long)b * K);
  const long long HW = (long long)H * W;
  const float *o = output + map * HW, *t = target + map * HW;
  float *dh = grad_output + map * HW;
  const float *pw = (weights && weights_per_pixel) ? weights + map * HW : nullptr;
  const float kw = (weights && !weights_per_pixel) ? weights[map] : 1.0f;
  const float *sm = mask ? mask + b * mask_sb + k * mask_sk : nullptr;
  float nonempty = 1.0f;
  if (skip_empty) {
    int any = 0;
    for (long long i = threadIdx.x; i < HW && !any; i += HB_THREADS) any = t[i] != 0.0f;
    nonempty = __syncthreads_or(any) ? 1.0f : 0.0f;
  }
  // the forward's mask, bit for bit (oks_heatmap_loss_kernel)
  auto mask_at = [&](long long idx) {
    float m = sm ? sm[idx] : 1.0f;
    m = m * (pw ? pw[idx] : kw);
    return m * nonempty;
  };
  const float sw2 = 2.0f * sw;

  if (reduction == HB_PIXEL || reduction == HB_PIXEL_MEAN) {
    const float *gm = grad + b * gs_b + k * gs_k;
    const float gconst = reduction == HB_PIXEL_MEAN ? grad[0] / (float)((double)n_maps * (double)HW) : 0.0f;
    auto g_at = [&](int r, int c) { return reduction == HB_PIXEL_MEAN ? gconst : gm[r * gs_h + c * gs_w]; };
    for (int r0 = 0; r0 < H; r0 += tile_rows) {
      const int br = min(tile_rows, H - r0);
      for (int c0 = 0; c0 < W; c0 += tile_cols) {
        const int bc = min(tile_cols, W - c0), ph = bc + 4, pe = bc + 2;
        // output rows r0-2 .. r0+br+1, columns c0-2 .. c0+bc+1; zero outside the map (the forward's padding)
        for (int i = threadIdx.x; i < (br + 4) * ph; i += HB_THREADS) {
          const int r = r0 - 2 + i / ph, c = c0 - 2 + i % ph;
          th[i] = (r >= 0 && r < H && c >= 0 && c < W) ? o[(long long)r * W + c] : 0.0f;
        }
        __syncthreads();
        // G*lw*m*gx and G*lw*m*gy at p = rows r0-1 .. r0+br, columns c0-1 .. c0+bc: zero for p outside the map,
        // whose energy the forward never forms
        for (int i = threadIdx.x; i < (br + 2) * pe; i += HB_THREADS) {
          const int rr = i / pe, cc = i - rr * pe, r = r0 - 1 + rr, c = c0 - 1 + cc;
          float ex = 0.0f, ey = 0.0f;
          if (r >= 0 && r < H && c >= 0 && c < W) {
            const float *a = th + rr * ph + cc;        // a[dr * ph + dc]: output[r - 1 + dr][c - 1 + dc]
            const float gx = (a[0] - a[2]) + 2.0f * (a[ph] - a[ph + 2]) + (a[2 * ph] - a[2 * ph + 2]);
            const float gy = (a[0] + 2.0f * a[1] + a[2]) - (a[2 * ph] + 2.0f * a[2 * ph + 1] + a[2 * ph + 2]);
            const float s = (g_at(r, c) * lw) * mask_at((long long)r * W + c);
            ex = s * gx;
            ey = s * gy;
          }
          tex[i] = ex;
          tey[i] = ey;
        }
        __syncthreads();
        for (int p = threadIdx.x; p < br * bc; p += HB_THREADS) {
          const int r = p / bc, c = p - r * bc;
          const long long idx = (long long)(r0 + r) * W + (c0 + c);
          // sum over the neighbours p = q - d of SX[d] * ex[p] + SY[d] * ey[p]; the ring index of q is (r+1, c+1)
          float acc = 0.0f;
#pragma unroll
          for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
            for (int dc = -1; dc <= 1; ++dc) {
              const int e = (r + 1 - dr) * pe + (c + 1 - dc);
              acc += SOBEL_X[dr + 1][dc + 1] * tex[e];
              acc += SOBEL_Y[dr + 1][dc + 1] * tey[e];
            }
          const float ov = th[(r + 2) * ph + (c + 2)], tv = t[idx];
          const float s = (g_at(r0 + r, c0 + c) * lw) * mask_at(idx);
          const float local = s * (ow * d_oks(oks_type, tv) + gw * (2.0f * (ov - tv)));
          dh[idx] = local + sw2 * acc;
        }
        __syncthreads();
      }
    }
    return;
  }

  // per keypoint / mean: a = d loss / d (that map's per-keypoint loss without lw) * lw
  const float a = reduction == HB_KEYPOINT ? grad[b * gs_b + k * gs_k] * lw : (grad[0] * lw) / (float)n_maps;
  // (1) the first maximal masked energy, computed exactly as the forward does
  float best = -__builtin_inff();
  int besti = 0x7fffffff;
  for (int r0 = 0; r0 < H; r0 += tile_rows) {
    const int br = min(tile_rows, H - r0);
    for (int c0 = 0; c0 < W; c0 += tile_cols) {
      const int bc = min(tile_cols, W - c0), pitch = bc + 2;
      for (int i = threadIdx.x; i < (br + 2) * pitch; i += HB_THREADS) {
        const int r = r0 - 1 + i / pitch, c = c0 - 1 + i % pitch;
        th[i] = (r >= 0 && r < H && c >= 0 && c < W) ? o[(long long)r * W + c] : 0.0f;
      }
      __syncthreads();
      for (int p = threadIdx.x; p < br * bc; p += HB_THREADS) {
        const int r = p / bc, c = p - r * bc;
        const long long idx = (long long)(r0 + r) * W + (c0 + c);
        const float *q = th + r * pitch + c;
        const float gx = (q[0] - q[2]) + 2.0f * (q[pitch] - q[pitch + 2]) + (q[2 * pitch] - q[2 * pitch + 2]);
        const float gy = (q[0] + 2.0f * q[1] + q[2]) - (q[2 * pitch] + 2.0f * q[2 * pitch + 1] + q[2 * pitch + 2]);
        float e = gx * gx + gy * gy;
        e = e * mask_at(idx);
        if (max_before(e, (int)idx, best, besti)) {
          best = e;
          besti = (int)idx;
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float v = __shfl_xor(best, off, 64);
    const int i = __shfl_xor(besti, off, 64);
    if (max_before(v, i, best, besti)) {
      best = v;
      besti = i;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    rv[threadIdx.x >> 6] = best;
    ri[threadIdx.x >> 6] = besti;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < HB_THREADS / 64; ++w)
      if (max_before(rv[w], ri[w], rv[0], ri[0])) {
        rv[0] = rv[w];
        ri[0] = ri[w];
      }
    // gx, gy at the maximum p*, scaled by a * m[p*] * 2 sw
    const int pr = ri[0] / W, pc = ri[0] - pr * W;
    auto at = [&](int r, int c) { return (r >= 0 && r < H && c >= 0 && c < W) ? o[(long long)r * W + c] : 0.0f; };
    const float a00 = at(pr - 1, pc - 1), a01 = at(pr - 1, pc), a02 = at(pr - 1, pc + 1), a10 = at(pr, pc - 1),
                a12 = at(pr, pc + 1), a20 = at(pr + 1, pc - 1), a21 = at(pr + 1, pc), a22 = at(pr + 1, pc + 1);
    const float gx = (a00 - a02) + 2.0f * (a10 - a12) + (a20 - a22);
    const float gy = (a00 + 2.0f * a01 + a02) - (a20 + 2.0f * a21 + a22);
    const float s = (a * mask_at(ri[0])) * sw2;
    star[0] = s * gx;
    star[1] = s * gy;
  }
  __syncthreads();
  const int pstar = ri[0], pr = pstar / W, pc = pstar - pr * W;
  const float sx = star[0], sy = star[1];
  const float inv_hw = 2.0f / (float)HW;
  // (2) every pixel: the oks and mse terms, plus the Sobel term on the 3x3 neighbours of p* inside the map
  for (long long idx = threadIdx.x; idx < HW; idx += HB_THREADS) {
    const float ov = o[idx], tv = t[idx];
    const float s = a * mask_at(idx);
    float v = s * (ow * d_oks(oks_type, tv) + gw * ((ov - tv) * inv_hw));
    const int r = (int)(idx / W), c = (int)(idx - (long long)r * W), dr = r - pr, dc = c - pc;
    if (dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1)
      v = v + (sx * SOBEL_X[dr + 1][dc + 1] + sy * SOBEL_Y[dr + 1][dc + 1]);
    dh[idx] = v;
  }
}

// torch's backward of the four small losses of ProbPoseLoss.forward, each a mean over the N = B*K keypoints:
//   probability / visibility  binary_cross_entropy (ATen): g * (x - y) / max((1 - x) x, 1e-12)
//   oks                       mse_loss of (x w, y w):      2 (x w - y w) g * w
//   error                     smooth_l1 of (log(1 + x) w, log(1 + y) w), beta 1: clamp(z, -1, 1) g * w / (1 + x)
// with g = upstream / N and w = annotated & in_image.  The visibility BCE is unweighted, as in the reference
// (BCELoss(use_target_weight=False) ignores the visibility weights it is passed, loss.py:452-454).
__global__ __launch_bounds__(256) void probpose_loss_grads_kernel(
    const float *__restrict__ dt_prob, const float *__restrict__ dt_vis, const float *__restrict__ dt_oks,
    const float *__restrict__ dt_err, const float *__restrict__ gt_oks, const float *__restrict__ gt_err,
    const int *__restrict__ in_image, const int *__restrict__ annotated, const int *__restrict__ visibility,
    const float *__restrict__ u_prob, const float *__restrict__ u_vis, const float *__restrict__ u_oks,
    const float *__restrict__ u_err, long long N, float *__restrict__ d_prob, float *__restrict__ d_vis,
    float *__restrict__ d_oks, float *__restrict__ d_err) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float n = (float)N;
  const float ai = (float)(annotated[i] & (in_image[i] > 0));
  {
    const float x = dt_prob[i], y = (float)in_image[i];
    d_prob[i] = ((u_prob[0] / n) * (x - y)) / fmaxf((1.0f - x) * x, 1e-12f);
  }
  {
    const float x = dt_vis[i], y = (float)visibility[i];
    d_vis[i] = ((u_vis[0] / n) * (x - y)) / fmaxf((1.0f - x) * x, 1e-12f);
  }
  {
    const float x = dt_oks[i], y = gt_oks[i];
    d_oks[i] = ((2.0f * (x * ai - y * ai)) * (u_oks[0] / n)) * ai;
  }
  {
    const float x = dt_err[i], y = gt_err[i];
    const float x1 = 1.0f + x;                 // rounded to float32, as torch.log(1 + x) sees it
    const float z = logf(x1) * ai - logf(1.0f + y) * ai;
    const float s = z < -1.0f ? -1.0f : (z > 1.0f ? 1.0f : z);
    d_err[i] = ((s * (u_err[0] / n)) * ai) / x1;
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

extern "C" int pp_oks_heatmap_loss_backward(const float *output, const float *target, const float *weights,
                                            int weights_per_pixel, const float *mask, long long mask_sb,
                                            long long mask_sk, int skip_empty, int oks_type, float smoothing_weight,
                                            float oks_weight, float gaussian_weight, float loss_weight, int reduction,
                                            const float *grad, long long grad_sb, long long grad_sk,
                                            long long grad_sh, long long grad_sw, int B, int K, int H, int W,
                                            float *grad_output, void *stream) {
  using namespace pp;
  PP_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0, "pp_oks_heatmap_loss_backward: bad shape B=%d K=%d H=%d W=%d", B, K,
             H, W);
  PP_REQUIRE((long long)B * K < (1ll << 31) && (long long)H * W < (1ll << 31),
             "pp_oks_heatmap_loss_backward: too many maps or pixels");
  PP_REQUIRE(oks_type >= 0 && oks_type <= 2,
             "pp_oks_heatmap_loss_backward: oks_type %d is not minus (0), plus (1), both (2)", oks_type);
  PP_REQUIRE(reduction >= HB_PIXEL && reduction <= HB_PIXEL_MEAN,
             "pp_oks_heatmap_loss_backward: reduction %d is not pixel (0), keypoint (1), mean (2), pixel mean (3)",
             reduction);
  PP_REQUIRE(output && target && grad && grad_output, "pp_oks_heatmap_loss_backward: null operand");
  PP_REQUIRE(mask_sb >= 0 && mask_sk >= 0 && grad_sb >= 0 && grad_sk >= 0 && grad_sh >= 0 && grad_sw >= 0,
             "pp_oks_heatmap_loss_backward: negative stride");
  const int cols = W < HB_MAX_COLS ? W : HB_MAX_COLS;
  int rows = HB_TILE_H / (cols + 4) - 4;
  const int rows_e = HB_TILE_E / (cols + 2) - 2;
  rows = rows < rows_e ? rows : rows_e;
  rows = rows < H ? rows : H;
  hipLaunchKernelGGL(oks_heatmap_loss_backward_kernel, dim3((unsigned)(B * K)), dim3(HB_THREADS), 0,
                     (hipStream_t)stream, output, target, weights, weights_per_pixel, mask, mask_sb, mask_sk,
                     skip_empty, oks_type, smoothing_weight, oks_weight, gaussian_weight, loss_weight, reduction,
                     grad, grad_sb, grad_sk, grad_sh, grad_sw, (long long)B * K, K, H, W, rows, cols, grad_output);
  PP_CHECK_LAUNCH("oks_heatmap_loss_backward_kernel");
  return 0;
}

extern "C" int pp_probpose_loss_grads(const float *dt_prob, const float *dt_vis, const float *dt_oks,
                                      const float *dt_err, const float *gt_oks, const float *gt_err,
                                      const int *in_image, const int *annotated, const int *visibility,
                                      const float *u_prob, const float *u_vis, const float *u_oks, const float *u_err,
                                      int B, int K, float *d_prob, float *d_vis, float *d_oks, float *d_err,
                                      void *stream) {
  using namespace pp;
  PP_REQUIRE(B > 0 && K > 0 && (long long)B * K < (1ll << 31), "pp_probpose_loss_grads: bad shape B=%d K=%d", B, K);
  PP_REQUIRE(dt_prob && dt_vis && dt_oks && dt_err && gt_oks && gt_err && in_image && annotated && visibility &&
                 u_prob && u_vis && u_oks && u_err && d_prob && d_vis && d_oks && d_err,
             "pp_probpose_loss_grads: null operand");
  const long long N = (long long)B * K;
  hipLaunchKernelGGL(probpose_loss_grads_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     dt_prob, dt_vis, dt_oks, dt_err, gt_oks, gt_err, in_image, annotated, visibility, u_prob, u_vis,
                     u_oks, u_err, N, d_prob, d_vis, d_oks, d_err);
  PP_CHECK_LAUNCH("probpose_loss_grads_kernel");
  return 0;
}
