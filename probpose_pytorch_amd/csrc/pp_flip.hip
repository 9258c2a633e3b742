// Flip test at inference: the crop and its mirror image go through the model as one batch of 2B, and the
// two sets of outputs are averaged with the mirror undone and the left/right keypoint channels swapped.  Two
// memory-bound kernels, float32 only (the head's five outputs are float32 in every compute mode):
//
// hflip_pair_kernel   out[b] = x[b], out[B + b, c, y, u] = x[b, c, y, W - 1 - u]: both halves of the 2B batch in one
//                     launch.  A thread reads 4 consecutive pixels once (one 128-bit load) and issues two 128-bit
//                     stores: the group as it is, and the group reversed in registers at the mirrored address
//                     W - 4 - u0 of the same row in the second half.  Lane i of a wave holds u0 = 4 i and rows follow
//                     each other, so the load and the straight store of a wave cover 1 KiB of consecutive addresses;
//                     the mirrored store covers the same 16-byte groups of a row in descending order.
//
// flip_merge_kernel   heat_out[b, k, y, u] = (heat2[b, k, y, u] + heat2[B + b, perm[k], y, W - 1 - u]) * 0.5f
//                     aux_out[j, b, k]     = (aux2[j, b, k] + aux2[j, B + b, perm[k]]) * 0.5f        j = 0 .. 3
//                     in float32, in this order: one add, one multiply by 0.5 (exact barring underflow; the library is
//                     built without contraction).  One launch for the five outputs: the first workgroups take 4 pixels
//                     a thread (two 128-bit loads, the mirrored one at W - 4 - u0 reversed in registers, one 128-bit
//                     store), the trailing workgroups of the same grid take the 4 B K auxiliary values one a thread.
//                     No atomics, no LDS.
//
// W % 4 != 0 (or a pointer that is not 16-byte aligned) takes the one-pixel-per-thread instance of either kernel.
#include "pp_common.h"

namespace pp {

template <int V>
__global__ __launch_bounds__(256) void hflip_pair_kernel(const float *__restrict__ x, float *__restrict__ out,
                                                         int n_threads, int W, long long half) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_threads) return;
  const int per_row = W / V;
  const int row = i / per_row, u0 = (i - row * per_row) * V;
  const size_t base = (size_t)row * W;
  if constexpr (V == 4) {
    const float4 v = *reinterpret_cast<const float4 *>(x + base + u0);
    *reinterpret_cast<float4 *>(out + base + u0) = v;
    *reinterpret_cast<float4 *>(out + (size_t)half + base + (W - 4 - u0)) = make_float4(v.w, v.z, v.y, v.x);
  } else {
    const float v = x[base + u0];
    out[base + u0] = v;
    out[(size_t)half + base + (W - 1 - u0)] = v;
  }
}

template <int V>
__global__ __launch_bounds__(256) void flip_merge_kernel(const float *__restrict__ heat2,
                                                         const float *__restrict__ aux2,
                                                         const int *__restrict__ perm, int heat_blocks,
                                                         int heat_threads, int B, int K, int H, int W,
                                                         float *__restrict__ heat_out, float *__restrict__ aux_out) {
  if ((int)blockIdx.x < heat_blocks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= heat_threads) return;
    const int per_row = W / V;
    const int row = i / per_row, u0 = (i - row * per_row) * V;      // row = (b K + k) H + y
    const int y = row % H, bk = row / H, k = bk % K, b = bk / K;
    int s = perm[k];
    if ((unsigned)s >= (unsigned)K) s = k;     // the host has checked the permutation; never index outside the batch
    const size_t straight = (size_t)row * W + u0;
    const size_t mirrored = (((size_t)(B + b) * K + s) * H + y) * W + (W - V - u0);
    if constexpr (V == 4) {
      const float4 a = *reinterpret_cast<const float4 *>(heat2 + straight);
      const float4 m = *reinterpret_cast<const float4 *>(heat2 + mirrored);
      float4 r;
      r.x = (a.x + m.w) * 0.5f;
      r.y = (a.y + m.z) * 0.5f;
      r.z = (a.z + m.y) * 0.5f;
      r.w = (a.w + m.x) * 0.5f;
      *reinterpret_cast<float4 *>(heat_out + straight) = r;
    } else {
      heat_out[straight] = (heat2[straight] + heat2[mirrored]) * 0.5f;
    }
  } else {
    const int i = ((int)blockIdx.x - heat_blocks) * 256 + threadIdx.x;
    const int BK = B * K;
    if (i >= 4 * BK) return;
    const int j = i / BK, r = i - j * BK, b = r / K, k = r - b * K;
    int s = perm[k];
    if ((unsigned)s >= (unsigned)K) s = k;
    const float *a = aux2 + (size_t)j * 2 * BK;
    aux_out[i] = (a[b * K + k] + a[(B + b) * K + s]) * 0.5f;
  }
}

static bool overlap(const void *a, long long a_bytes, const void *b, long long b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

// a b c d <= limit, without overflow (every factor is positive and below 2^31)
static bool count_within(int a, int b, int c, int d, long long limit) {
  long long n = a;
  for (int f : {b, c, d}) {
    n *= f;
    if (n > limit) return false;
  }
  return true;
}

static bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace pp

extern "C" int pp_hflip_pair(const float *x, float *out, int B, int C, int H, int W, void *stream) {
  using namespace pp;
  PP_REQUIRE(x && out, "pp_hflip_pair: null pointer");
  PP_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "pp_hflip_pair: sizes must be positive, got B=%d C=%d H=%d W=%d", B, C,
             H, W);
  PP_REQUIRE(count_within(B, C, H, W, (1ll << 30) - 1),
             "pp_hflip_pair: 2 x %d x %d x %d x %d output elements exceed the 2^31 the index arithmetic holds", B, C, H,
             W);
  const long long rows = (long long)B * C * H;
  const long long half = rows * W;
  PP_REQUIRE(!overlap(x, half * 4, out, 2 * half * 4), "pp_hflip_pair: out aliases x (in-place use is refused)");
  if (W % 4 == 0 && aligned16(x) && aligned16(out)) {
    const int n_threads = (int)(rows * (W / 4));
    hipLaunchKernelGGL(hflip_pair_kernel<4>, dim3((unsigned)cdiv(n_threads, 256)), dim3(256), 0, (hipStream_t)stream, x,
                       out, n_threads, W, half);
  } else {
    const int n_threads = (int)half;
    hipLaunchKernelGGL(hflip_pair_kernel<1>, dim3((unsigned)cdiv(n_threads, 256)), dim3(256), 0, (hipStream_t)stream, x,
                       out, n_threads, W, half);
  }
  PP_CHECK_LAUNCH("hflip_pair_kernel");
  return 0;
}

extern "C" int pp_flip_merge(const float *heat2, const float *aux2, const int *perm, int B, int K, int H, int W,
                             float *heat_out, float *aux_out, void *stream) {
  using namespace pp;
  PP_REQUIRE(heat2 && aux2 && perm && heat_out && aux_out, "pp_flip_merge: null pointer");
  PP_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0, "pp_flip_merge: sizes must be positive, got B=%d K=%d H=%d W=%d", B, K,
             H, W);
  PP_REQUIRE(count_within(B, K, H, W, (1ll << 30) - 1),
             "pp_flip_merge: 2 x %d x %d x %d x %d input elements exceed the 2^31 the index arithmetic holds", B, K, H,
             W);
  const long long rows = (long long)B * K * H, n = rows * W, bk = (long long)B * K;
  PP_REQUIRE(bk < (1ll << 28), "pp_flip_merge: 8 x %d x %d auxiliary elements exceed the 2^31 the index arithmetic holds",
             B, K);
  PP_REQUIRE(!overlap(heat_out, n * 4, heat2, 2 * n * 4),
             "pp_flip_merge: heat_out aliases heat2 (in-place use is refused)");
  PP_REQUIRE(!overlap(aux_out, 4 * bk * 4, aux2, 8 * bk * 4),
             "pp_flip_merge: aux_out aliases aux2 (in-place use is refused)");
  PP_REQUIRE(!overlap(aux_out, 4 * bk * 4, heat2, 2 * n * 4) && !overlap(heat_out, n * 4, aux2, 8 * bk * 4) &&
                 !overlap(heat_out, n * 4, aux_out, 4 * bk * 4),
             "pp_flip_merge: an output aliases the other output or the other input");
  const int aux_blocks = cdiv(4 * bk, 256);
  if (W % 4 == 0 && aligned16(heat2) && aligned16(heat_out)) {
    const int heat_threads = (int)(rows * (W / 4)), heat_blocks = cdiv(heat_threads, 256);
    hipLaunchKernelGGL(flip_merge_kernel<4>, dim3((unsigned)(heat_blocks + aux_blocks)), dim3(256), 0,
                       (hipStream_t)stream, heat2, aux2, perm, heat_blocks, heat_threads, B, K, H, W, heat_out,
                       aux_out);
  } else {
    const int heat_threads = (int)n, heat_blocks = cdiv(heat_threads, 256);
    hipLaunchKernelGGL(flip_merge_kernel<1>, dim3((unsigned)(heat_blocks + aux_blocks)), dim3(256), 0,
                       (hipStream_t)stream, heat2, aux2, perm, heat_blocks, heat_threads, B, K, H, W, heat_out,
                       aux_out);
  }
  PP_CHECK_LAUNCH("flip_merge_kernel");
  return 0;
}
