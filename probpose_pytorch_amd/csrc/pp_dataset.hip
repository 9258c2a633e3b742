// Ground truth of a training batch apart from the probability maps, on the GPU.
// Replaces, per sample (reference file:line), batched over B samples in one launch:
//   dataset.py:87-89    scale_box: kps = (kps - bbox[0]) / bbox[2] * image_size[0] (and y), on a float32 array with
//                       Python-float box components: numpy rounds each scalar to float32 and runs three float32 ops
//   dataset.py:124-126  keypoints_visible = (v == 2), keypoints_visibility = minimum(v, 1)
//   codec.py:178        heatmap_keypoints = keypoints / scale_factor (float32 / float32)
//   codec.py:195-204    in_image = (0 <= x < input_w) & (0 <= y < input_h)
// The arithmetic is plain IEEE float32 subtract, divide, multiply: the library is built with -ffp-contract=off and
// -fhip-fp32-correctly-rounded-divide-sqrt, so nothing is fused and the division is not a reciprocal multiply.
// One thread per keypoint; 12 + 32/K bytes in and 26 bytes out each: the launch is latency, not bandwidth.
#include "pp_common.h"

namespace pp {

__global__ __launch_bounds__(256) void dataset_gt_kernel(const float *__restrict__ kpts_raw,
                                                         const double *__restrict__ boxes, int n, int K, float in_w,
                                                         float in_h, float scale_x, float scale_y,
                                                         float *__restrict__ kpts_crop, float *__restrict__ kpts_hm,
                                                         float *__restrict__ encode_visible,
                                                         unsigned char *__restrict__ in_image,
                                                         unsigned char *__restrict__ visible,
                                                         float *__restrict__ visibility) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double *box = boxes + 4 * (i / K);
  const float bx = (float)box[0], by = (float)box[1], bw = (float)box[2], bh = (float)box[3];
  const float kx = kpts_raw[3 * i], ky = kpts_raw[3 * i + 1], v = kpts_raw[3 * i + 2];
  float x = kx - bx;
  x = x / bw;
  x = x * in_w;
  float y = ky - by;
  y = y / bh;
  y = y * in_h;
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

}  // namespace pp

extern "C" int pp_dataset_ground_truth(const float *kpts_raw, const double *boxes_xywh, int B, int K, int in_w,
                                       int in_h, float scale_x, float scale_y, float *kpts_crop, float *kpts_hm,
                                       float *encode_visible, unsigned char *in_image,
                                       unsigned char *keypoints_visible, float *keypoints_visibility, void *stream) {
  using namespace pp;
  PP_REQUIRE(B >= 0 && K > 0 && in_w > 0 && in_h > 0 && in_w < (1 << 24) && in_h < (1 << 24) &&
                 (long long)B * K < (1ll << 30),
             "pp_dataset_ground_truth: bad shape");
  if (B == 0) return 0;
  PP_REQUIRE(kpts_raw && boxes_xywh && kpts_crop && kpts_hm && encode_visible && in_image && keypoints_visible &&
                 keypoints_visibility,
             "pp_dataset_ground_truth: null pointer");
  PP_REQUIRE(reinterpret_cast<uintptr_t>(boxes_xywh) % 8 == 0, "pp_dataset_ground_truth: boxes are not 8-byte aligned");
  const int n = B * K;
  hipLaunchKernelGGL(dataset_gt_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, kpts_raw,
                     boxes_xywh, n, K, (float)in_w, (float)in_h, scale_x, scale_y, kpts_crop, kpts_hm, encode_visible,
                     in_image, keypoints_visible, keypoints_visibility);
  PP_CHECK_LAUNCH("dataset_gt_kernel");
  return 0;
}
