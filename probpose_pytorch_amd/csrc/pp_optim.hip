// FusedAdamW: global gradient-norm clipping and torch's AdamW over ALL parameter tensors in at most three launches
// (train.py:113-115: clip_grad_norm_(max_norm=1.0), AdamW(weight_decay=0.1).step() under OneCycleLR).
//
// The work is a plain stream: read p, g, m, v and write p, m, v (28 B per parameter) plus one read of g for the norm
// (4 B).  What makes it many launches elsewhere is the number of tensors (199 trainable ones on train.py's model, from
// 20 to 1 572 864 elements); here a device table describes them all and a chunk map turns the ragged list into a flat
// grid, one workgroup per chunk of at most PP_OPTIM_CHUNK elements of ONE tensor:
//
//   [header 32 B][groups: n_groups x {lr, beta1, beta2, eps, weight_decay} f64][tensors: n_tensors x 56 B]
//   [chunk map: n_chunks x {tensor, chunk within the tensor} int32]
//
// pp_optim_table_build packs and checks it on the host (no GPU needed); the caller copies it to the device, the
// prefix up to the chunk map every step (gradient addresses and the scheduler's lr / beta1 change per step), the chunk
// map when the set of tensors changes.
//
//   grad_sqnorm_partials_kernel  partials[chunk] = sum g^2 of the chunk, squares and sums in float64 (a float32 square
//                                is exact there), fixed order: lane, wave shuffle, four waves through LDS
//   grad_norm_finish_kernel      one workgroup: the partials in a fixed order -> record {total_norm f32, clip_coef f32,
//                                finite, skipped_steps}
//   adamw_step_kernel            per chunk: lane 0 takes the tensor's step count t from the device, forms the bias
//                                corrections in float64 and hands the per-tensor scalars over in LDS; then 128-bit
//                                loads and stores where the four pointers allow, a scalar loop otherwise, tails handled
//
// Roundings per element and step (what tests/test_optim_gpu.py counts): g' = g clip_coef, the two moment updates and
// the decay multiply are evaluated in float64 and rounded ONCE each when stored as float32; sqrt, the division by
// sqrt(1 - beta2^t), + eps, step_size m, the division and the final subtraction are float32 operations (compiled
// -ffp-contract=off with correctly rounded division and sqrt).  No float atomics: the same bits on every call.  The
// only atomic is the integer arrival counter by which the LAST chunk of a tensor advances that tensor's step count
// (every chunk has read it before it arrives).  Everything is written by ordinary vector stores.
#include "pp_common.h"

namespace pp {

constexpr int kChunk = PP_OPTIM_CHUNK;
constexpr unsigned kMagic = 0x4f505431u;   // "OPT1"

struct OptHeader {
  unsigned magic;
  int n_tensors, n_groups, n_chunks, chunk_elems, pad;
  int *arrive;                             // [n_tensors] int32, zero between launches
};
struct OptGroup {
  double lr, beta1, beta2, eps, weight_decay;
};
struct OptTensor {
  float *p;
  const float *g;
  float *m, *v, *step;
  long long n;
  int group, pad;
};
struct OptRecord {
  float total_norm, clip_coef;
  int finite, skipped_steps;
};
static_assert(sizeof(OptHeader) == 32 && sizeof(OptGroup) == 40 && sizeof(OptTensor) == 56 && sizeof(OptRecord) == 16,
              "the table layout is part of the C ABI (include/probpose_hip.h)");

struct OptView {
  const OptHeader *hdr;
  const OptGroup *groups;
  const OptTensor *tensors;
  const int2 *chunks;
};
__host__ __device__ inline OptView view_of(const void *table, int n_groups, int n_tensors) {
  const char *b = reinterpret_cast<const char *>(table);
  OptView w;
  w.hdr = reinterpret_cast<const OptHeader *>(b);
  w.groups = reinterpret_cast<const OptGroup *>(b + sizeof(OptHeader));
  w.tensors = reinterpret_cast<const OptTensor *>(b + sizeof(OptHeader) + sizeof(OptGroup) * (size_t)n_groups);
  w.chunks = reinterpret_cast<const int2 *>(b + sizeof(OptHeader) + sizeof(OptGroup) * (size_t)n_groups +
                                            sizeof(OptTensor) * (size_t)n_tensors);
  return w;
}

__global__ __launch_bounds__(256) void grad_sqnorm_partials_kernel(const void *__restrict__ table,
                                                                   double *__restrict__ partials) {
  const OptHeader *hdr = reinterpret_cast<const OptHeader *>(table);
  if (hdr->magic != kMagic || (int)blockIdx.x >= hdr->n_chunks) return;
  const OptView w = view_of(table, hdr->n_groups, hdr->n_tensors);
  const int2 cm = w.chunks[blockIdx.x];
  const OptTensor T = w.tensors[cm.x];
  const long long off = (long long)cm.y * kChunk;
  const int cnt = (int)(T.n - off < kChunk ? T.n - off : kChunk);
  const float *g = T.g + off;
  double acc = 0.0;
  if ((((uintptr_t)g) & 15) == 0) {
    const int nq = cnt >> 2;
    for (int q = threadIdx.x; q < nq; q += 256) {
      const float4 t = reinterpret_cast<const float4 *>(g)[q];
      acc += (double)t.x * (double)t.x;
      acc += (double)t.y * (double)t.y;
      acc += (double)t.z * (double)t.z;
      acc += (double)t.w * (double)t.w;
    }
    const int i = 4 * nq + threadIdx.x;
    if (i < cnt) acc += (double)g[i] * (double)g[i];
  } else {
    for (int i = threadIdx.x; i < cnt; i += 256) acc += (double)g[i] * (double)g[i];
  }
  acc = wave_sum(acc);
  __shared__ double ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

__global__ __launch_bounds__(1024) void grad_norm_finish_kernel(const double *__restrict__ partials, int n, int clip,
                                                                double max_norm, int count_skips,
                                                                OptRecord *__restrict__ rec) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) acc += partials[i];
  acc = wave_sum(acc);
  __shared__ double ws[16];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < 16; ++k) s += ws[k];
    const double norm = sqrt(s);
    double c = 1.0;
    if (clip) {
      c = max_norm / (norm + 1e-6);
      c = c > 1.0 ? 1.0 : c;               // a NaN norm stays a NaN coefficient, as torch.clamp(max=1) keeps it
    }
    const int finite = s == s && s != __builtin_inf();
    rec->total_norm = (float)norm;
    rec->clip_coef = (float)c;
    rec->finite = finite;
    if (count_skips && !finite) rec->skipped_steps = rec->skipped_steps + 1;
  }
}

struct StepScalars {
  double coef, beta1, omb1, beta2, omb2, decay;
  float step_size, bc2_sqrt, eps, t;
};

__device__ inline double powi(double b, long long e) {   // b^e by squaring, e >= 0
  double r = 1.0;
  while (e > 0) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

__device__ __forceinline__ void adamw_one(float &p, float g, float &m, float &v, const StepScalars &s) {
  const double gd = (double)g * s.coef;
  m = (float)(s.beta1 * (double)m + s.omb1 * gd);
  v = (float)(s.beta2 * (double)v + s.omb2 * (gd * gd));
  const float pd = (float)((double)p * s.decay);
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = pd - s.step_size * m / denom;
}

__device__ __forceinline__ void adamw_quad(float4 &p, const float4 &g, float4 &m, float4 &v, const StepScalars &s) {
  adamw_one(p.x, g.x, m.x, v.x, s);
  adamw_one(p.y, g.y, m.y, v.y, s);
  adamw_one(p.z, g.z, m.z, v.z, s);
  adamw_one(p.w, g.w, m.w, v.w, s);
}

__global__ __launch_bounds__(256) void adamw_step_kernel(const void *__restrict__ table,
                                                         const OptRecord *__restrict__ rec, int skip_nonfinite) {
  const OptHeader *hdr = reinterpret_cast<const OptHeader *>(table);
  if (hdr->magic != kMagic || (int)blockIdx.x >= hdr->n_chunks) return;
  if (rec && skip_nonfinite && !rec->finite) return;       // p, m, v and the step counts stay as they are
  const OptView w = view_of(table, hdr->n_groups, hdr->n_tensors);
  const int2 cm = w.chunks[blockIdx.x];
  const OptTensor T = w.tensors[cm.x];
  __shared__ StepScalars sh;
  if (threadIdx.x == 0) {
    const OptGroup G = w.groups[T.group];
    const float t = *T.step + 1.0f;
    StepScalars s;
    s.coef = rec ? (double)rec->clip_coef : 1.0;
    s.beta1 = G.beta1;
    s.omb1 = 1.0 - G.beta1;
    s.beta2 = G.beta2;
    s.omb2 = 1.0 - G.beta2;
    s.decay = 1.0 - G.lr * G.weight_decay;
    s.step_size = (float)(G.lr / (1.0 - powi(G.beta1, (long long)t)));
    s.bc2_sqrt = (float)sqrt(1.0 - powi(G.beta2, (long long)t));
    s.eps = (float)G.eps;
    s.t = t;
    sh = s;
  }
  __syncthreads();
  const StepScalars s = sh;
  const long long off = (long long)cm.y * kChunk;
  const int cnt = (int)(T.n - off < kChunk ? T.n - off : kChunk);
  float *p = T.p + off, *m = T.m + off, *v = T.v + off;
  const float *g = T.g + off;
  if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0) {
    const int nq = cnt >> 2;
#pragma unroll 2
    for (int q = threadIdx.x; q < nq; q += 256) {
      float4 tp = reinterpret_cast<float4 *>(p)[q];
      const float4 tg = reinterpret_cast<const float4 *>(g)[q];
      float4 tm = reinterpret_cast<float4 *>(m)[q];
      float4 tv = reinterpret_cast<float4 *>(v)[q];
      adamw_quad(tp, tg, tm, tv, s);
      reinterpret_cast<float4 *>(p)[q] = tp;
      reinterpret_cast<float4 *>(m)[q] = tm;
      reinterpret_cast<float4 *>(v)[q] = tv;
    }
    const int i = 4 * nq + threadIdx.x;
    if (i < cnt) adamw_one(p[i], g[i], m[i], v[i], s);
  } else {
    for (int i = threadIdx.x; i < cnt; i += 256) adamw_one(p[i], g[i], m[i], v[i], s);
  }
  // the tensor's step count advances once every chunk of it has read the old one
  if (threadIdx.x == 0) {
    const int nck = (int)((T.n + kChunk - 1) / kChunk);
    if (nck == 1) {
      *T.step = s.t;
    } else {
      __threadfence();
      if (atomicAdd(&hdr->arrive[cm.x], 1) == nck - 1) {
        *T.step = s.t;
        hdr->arrive[cm.x] = 0;
      }
    }
  }
}

static long long chunks_of(int n_tensors, const long long *counts) {
  long long c = 0;
  for (int i = 0; i < n_tensors; ++i) c += (counts[i] + kChunk - 1) / kChunk;
  return c;
}

}  // namespace pp

extern "C" long long pp_optim_table_bytes(int n_tensors, const long long *counts, int n_groups) {
  using namespace pp;
  if (n_tensors <= 0 || n_groups <= 0 || !counts) {
    fail("pp_optim_table_bytes: n_tensors=%d n_groups=%d counts=%p", n_tensors, n_groups, (const void *)counts);
    return -1;
  }
  for (int i = 0; i < n_tensors; ++i)
    if (counts[i] <= 0) {
      fail("pp_optim_table_bytes: tensor %d has count %lld (every tensor needs at least one element)", i, counts[i]);
      return -1;
    }
  const long long nc = chunks_of(n_tensors, counts);
  if (nc >= (1ll << 31)) {
    fail("pp_optim_table_bytes: %lld chunks exceed one grid", nc);
    return -1;
  }
  return (long long)(sizeof(OptHeader) + sizeof(OptGroup) * (size_t)n_groups + sizeof(OptTensor) * (size_t)n_tensors +
                     sizeof(int2) * (size_t)nc);
}

extern "C" int pp_optim_table_build(int n_tensors, const void *const *p, const void *const *g, const void *const *m,
                                    const void *const *v, const void *const *step, const long long *counts,
                                    const int *group, int n_groups, const double *hyper, void *arrive, void *table,
                                    int with_chunks, int *n_chunks, long long *prefix_bytes) {
  using namespace pp;
  PP_REQUIRE(n_tensors > 0, "pp_optim_table_build: zero tensors (n_tensors=%d)", n_tensors);
  PP_REQUIRE(n_groups > 0, "pp_optim_table_build: n_groups=%d", n_groups);
  PP_REQUIRE(p && g && m && v && step && counts && group && hyper && arrive && table && n_chunks && prefix_bytes,
             "pp_optim_table_build: null argument");
  PP_REQUIRE((((uintptr_t)table) & 7) == 0, "pp_optim_table_build: table %p is not 8-byte aligned", table);
  PP_REQUIRE((((uintptr_t)arrive) & 3) == 0, "pp_optim_table_build: arrive %p is not 4-byte aligned", arrive);
  for (int i = 0; i < n_tensors; ++i) {
    PP_REQUIRE(counts[i] > 0, "pp_optim_table_build: tensor %d has count %lld", i, counts[i]);
    PP_REQUIRE(p[i] && g[i] && m[i] && v[i] && step[i], "pp_optim_table_build: tensor %d has a null pointer", i);
    PP_REQUIRE(((((uintptr_t)p[i]) | ((uintptr_t)g[i]) | ((uintptr_t)m[i]) | ((uintptr_t)v[i]) | ((uintptr_t)step[i])) &
                3) == 0,
               "pp_optim_table_build: tensor %d has a pointer that is not 4-byte aligned", i);
    PP_REQUIRE(group[i] >= 0 && group[i] < n_groups, "pp_optim_table_build: tensor %d names group %d of %d", i,
               group[i], n_groups);
  }
  for (int k = 0; k < n_groups; ++k) {
    const double *h = hyper + 5 * k;
    PP_REQUIRE(h[0] >= 0.0 && h[1] >= 0.0 && h[1] < 1.0 && h[2] >= 0.0 && h[2] < 1.0 && h[3] >= 0.0 && h[4] >= 0.0,
               "pp_optim_table_build: group %d has lr=%g betas=(%g, %g) eps=%g weight_decay=%g", k, h[0], h[1], h[2],
               h[3], h[4]);
  }
  const long long nc = chunks_of(n_tensors, counts);
  PP_REQUIRE(nc < (1ll << 31), "pp_optim_table_build: %lld chunks exceed one grid", nc);
  OptHeader *hdr = reinterpret_cast<OptHeader *>(table);
  hdr->magic = kMagic;
  hdr->n_tensors = n_tensors;
  hdr->n_groups = n_groups;
  hdr->n_chunks = (int)nc;
  hdr->chunk_elems = kChunk;
  hdr->pad = 0;
  hdr->arrive = reinterpret_cast<int *>(arrive);
  const OptView w = view_of(table, n_groups, n_tensors);
  OptGroup *G = const_cast<OptGroup *>(w.groups);
  for (int k = 0; k < n_groups; ++k) {
    const double *h = hyper + 5 * k;
    G[k] = OptGroup{h[0], h[1], h[2], h[3], h[4]};
  }
  OptTensor *T = const_cast<OptTensor *>(w.tensors);
  for (int i = 0; i < n_tensors; ++i)
    T[i] = OptTensor{(float *)p[i], (const float *)g[i], (float *)m[i], (float *)v[i], (float *)step[i], counts[i],
                     group[i], 0};
  if (with_chunks) {
    int2 *cm = const_cast<int2 *>(w.chunks);
    long long c = 0;
    for (int i = 0; i < n_tensors; ++i) {
      const int k = (int)((counts[i] + kChunk - 1) / kChunk);
      for (int j = 0; j < k; ++j) cm[c++] = make_int2(i, j);
    }
  }
  *n_chunks = (int)nc;
  *prefix_bytes = (long long)(reinterpret_cast<const char *>(w.chunks) - reinterpret_cast<const char *>(table));
  return 0;
}

static int check_table(const char *who, const void *table, int n_chunks) {
  using namespace pp;
  PP_REQUIRE(table, "%s: null table", who);
  PP_REQUIRE((((uintptr_t)table) & 7) == 0, "%s: table %p is not 8-byte aligned", who, table);
  PP_REQUIRE(n_chunks > 0, "%s: n_chunks=%d (a step needs at least one tensor)", who, n_chunks);
  return 0;
}

extern "C" int pp_grad_sqnorm_partials(const void *table, int n_chunks, double *partials, void *stream) {
  using namespace pp;
  if (int rc = check_table("pp_grad_sqnorm_partials", table, n_chunks)) return rc;
  PP_REQUIRE(partials, "pp_grad_sqnorm_partials: null partials");
  PP_REQUIRE((((uintptr_t)partials) & 7) == 0, "pp_grad_sqnorm_partials: partials %p is not 8-byte aligned",
             (void *)partials);
  hipLaunchKernelGGL(grad_sqnorm_partials_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, partials);
  PP_CHECK_LAUNCH("grad_sqnorm_partials_kernel");
  return 0;
}

extern "C" int pp_grad_norm_finish(const double *partials, int n_chunks, int clip, double max_norm, int count_skips,
                                   void *record, void *stream) {
  using namespace pp;
  PP_REQUIRE(partials && record, "pp_grad_norm_finish: null %s", partials ? "record" : "partials");
  PP_REQUIRE(((((uintptr_t)partials) & 7) | (((uintptr_t)record) & 3)) == 0,
             "pp_grad_norm_finish: partials / record are not aligned");
  PP_REQUIRE(n_chunks > 0, "pp_grad_norm_finish: n_chunks=%d", n_chunks);
  PP_REQUIRE(!clip || max_norm > 0.0, "pp_grad_norm_finish: max_norm=%g must be positive", max_norm);
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials, n_chunks, clip,
                     max_norm, count_skips, reinterpret_cast<OptRecord *>(record));
  PP_CHECK_LAUNCH("grad_norm_finish_kernel");
  return 0;
}

extern "C" int pp_adamw_step(const void *table, int n_chunks, const void *record, int skip_nonfinite, void *stream) {
  using namespace pp;
  if (int rc = check_table("pp_adamw_step", table, n_chunks)) return rc;
  PP_REQUIRE(!skip_nonfinite || record, "pp_adamw_step: skip_nonfinite needs the record of pp_grad_norm_finish");
  PP_REQUIRE((((uintptr_t)record) & 3) == 0, "pp_adamw_step: record %p is not 4-byte aligned", record);
  hipLaunchKernelGGL(adamw_step_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table,
                     reinterpret_cast<const OptRecord *>(record), skip_nonfinite);
  PP_CHECK_LAUNCH("adamw_step_kernel");
  return 0;
}
