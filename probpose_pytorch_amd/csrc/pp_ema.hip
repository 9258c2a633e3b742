// ModelEma: the exponential moving average of ALL state tensors of a model in one launch
// (timm's ModelEmaV2 / Ultralytics' ModelEMA: shadow = shadow + (1 - decay_t) (model - shadow) per float tensor, a
// plain copy of everything else, e.g. BatchNorm's int64 num_batches_tracked).
//
// The work is a stream: read src, read dst, write dst (12 B per averaged element).  What makes it many launches
// elsewhere is the number of tensors (199 parameters plus the BN buffers on train.py's model, from 1 to 1 572 864
// elements); as in pp_optim.hip a device table describes them all and a chunk map turns the ragged list into a flat
// grid, one workgroup per chunk of at most PP_OPTIM_CHUNK elements of ONE tensor:
//
//   [header 32 B][tensors: n_tensors x 32 B {src, dst, count, kind}][chunk map: n_chunks x {tensor, chunk} int32]
//
// Unlike the optimizer's table this one is static: neither the model's nor the shadow's addresses change from step to
// step (the gradients' do), so the caller uploads it once and rebuilds it only when an address, a count or a kind
// changes.  The weight 1 - decay_t is a launch argument.
//
// Roundings (what tests/test_ema_gpu.py counts): dst + weight (src - dst) is evaluated in float64 and rounded ONCE,
// when it is stored as float32 (compiled -ffp-contract=off).  No atomics at all, ordinary vector stores only: the same
// bits on every call.  src is never written.
#include "pp_common.h"

namespace pp {

constexpr int kEmaChunk = PP_OPTIM_CHUNK;
constexpr unsigned kEmaMagic = 0x454d4131u;   // "EMA1"
constexpr int kEmaBatch = 4;                  // 128-bit groups a lane has in flight before its first store

struct EmaHeader {
  unsigned magic;
  int n_tensors, n_chunks, chunk_elems;
  int pad[4];
};
struct EmaTensor {
  const void *src;
  void *dst;
  long long n;                               // float32 elements (kind 0) or 4-byte words (kind 1)
  int kind, pad;
};
static_assert(sizeof(EmaHeader) == 32 && sizeof(EmaTensor) == 32,
              "the table layout is part of the C ABI (include/probpose_hip.h)");

struct EmaView {
  const EmaHeader *hdr;
  const EmaTensor *tensors;
  const int2 *chunks;
};
__host__ __device__ inline EmaView ema_view_of(const void *table, int n_tensors) {
  const char *b = reinterpret_cast<const char *>(table);
  EmaView w;
  w.hdr = reinterpret_cast<const EmaHeader *>(b);
  w.tensors = reinterpret_cast<const EmaTensor *>(b + sizeof(EmaHeader));
  w.chunks = reinterpret_cast<const int2 *>(b + sizeof(EmaHeader) + sizeof(EmaTensor) * (size_t)n_tensors);
  return w;
}

struct Lerp {
  double w;
  __device__ __forceinline__ float operator()(float d, float s) const {
    return (float)((double)d + w * ((double)s - (double)d));
  }
};
struct CopyWord {
  __device__ __forceinline__ unsigned operator()(unsigned, unsigned s) const { return s; }
};

// the table hands the pointers over as plain (flat) addresses; they are global memory, and saying so gets global_load /
// global_store instead of the flat forms, which also wait on the LDS counter
#define PP_EMA_GLOBAL __attribute__((address_space(1)))
template <typename T> using Quad = T __attribute__((ext_vector_type(4)));

// dst[i] = op(dst[i], src[i]) over cnt elements of one chunk; src and dst do not overlap (the host checked it)
template <typename T, bool kReadsDst, typename Op>
__device__ __forceinline__ void ema_chunk(const T *src_flat, T *dst_flat, int cnt, Op op) {
  typedef Quad<T> Q;
  const PP_EMA_GLOBAL T *__restrict__ src = (const PP_EMA_GLOBAL T *)src_flat;
  PP_EMA_GLOBAL T *__restrict__ dst = (PP_EMA_GLOBAL T *)dst_flat;
  if (((((uintptr_t)src_flat) | ((uintptr_t)dst_flat)) & 15) == 0) {
    const int nq = cnt >> 2;
    const PP_EMA_GLOBAL Q *__restrict__ s4 = (const PP_EMA_GLOBAL Q *)src_flat;
    PP_EMA_GLOBAL Q *__restrict__ d4 = (PP_EMA_GLOBAL Q *)dst_flat;
    for (int q0 = threadIdx.x; q0 < nq; q0 += 256 * kEmaBatch) {
      Q s[kEmaBatch], d[kEmaBatch];
#pragma unroll
      for (int k = 0; k < kEmaBatch; ++k) {
        const int q = q0 + 256 * k;
        if (q < nq) {
          s[k] = s4[q];
          if (kReadsDst) d[k] = d4[q];
          else d[k] = s[k];
        }
      }
#pragma unroll
      for (int k = 0; k < kEmaBatch; ++k) {
        const int q = q0 + 256 * k;
        if (q < nq) {
          Q r;
          r.x = op(d[k].x, s[k].x);
          r.y = op(d[k].y, s[k].y);
          r.z = op(d[k].z, s[k].z);
          r.w = op(d[k].w, s[k].w);
          d4[q] = r;
        }
      }
    }
    const int i = 4 * nq + threadIdx.x;
    if (i < cnt) dst[i] = op(kReadsDst ? dst[i] : src[i], src[i]);
  } else {
    for (int i = threadIdx.x; i < cnt; i += 256) dst[i] = op(kReadsDst ? dst[i] : src[i], src[i]);
  }
}

__global__ __launch_bounds__(256) void ema_update_kernel(const void *__restrict__ table, double weight) {
  const EmaHeader *hdr = reinterpret_cast<const EmaHeader *>(table);
  if (hdr->magic != kEmaMagic || (int)blockIdx.x >= hdr->n_chunks) return;
  const EmaView w = ema_view_of(table, hdr->n_tensors);
  const int2 cm = w.chunks[blockIdx.x];
  const EmaTensor T = w.tensors[cm.x];
  const long long off = (long long)cm.y * kEmaChunk;
  const int cnt = (int)(T.n - off < kEmaChunk ? T.n - off : kEmaChunk);
  if (T.kind == PP_EMA_LERP_F32)
    ema_chunk<float, true>(reinterpret_cast<const float *>(T.src) + off, reinterpret_cast<float *>(T.dst) + off, cnt,
                           Lerp{weight});
  else
    ema_chunk<unsigned, false>(reinterpret_cast<const unsigned *>(T.src) + off,
                               reinterpret_cast<unsigned *>(T.dst) + off, cnt, CopyWord{});
}

static long long ema_chunks_of(int n_tensors, const long long *counts) {
  long long c = 0;
  for (int i = 0; i < n_tensors; ++i) c += (counts[i] + kEmaChunk - 1) / kEmaChunk;
  return c;
}

static int ema_check_counts(const char *who, int n_tensors, const long long *counts, long long *n_chunks) {
  PP_REQUIRE(n_tensors > 0, "%s: zero tensors (n_tensors=%d)", who, n_tensors);
  PP_REQUIRE(counts, "%s: null counts", who);
  for (int i = 0; i < n_tensors; ++i)
    PP_REQUIRE(counts[i] > 0 && counts[i] < (1ll << 60),
               "%s: tensor %d has count %lld (every tensor needs at least one element)", who, i, counts[i]);
  *n_chunks = ema_chunks_of(n_tensors, counts);
  PP_REQUIRE(*n_chunks < (1ll << 31), "%s: %lld chunks exceed one grid", who, *n_chunks);
  return 0;
}

}  // namespace pp

extern "C" long long pp_ema_table_bytes(int n_tensors, const long long *counts) {
  using namespace pp;
  long long nc = 0;
  if (ema_check_counts("pp_ema_table_bytes", n_tensors, counts, &nc)) return -1;
  return (long long)(sizeof(EmaHeader) + sizeof(EmaTensor) * (size_t)n_tensors + sizeof(int2) * (size_t)nc);
}

extern "C" int pp_ema_table_build(int n_tensors, const void *const *src, const void *const *dst,
                                  const long long *counts, const int *kinds, void *table, int *n_chunks) {
  using namespace pp;
  PP_REQUIRE(src && dst && counts && kinds && table && n_chunks, "pp_ema_table_build: null argument");
  PP_REQUIRE((((uintptr_t)table) & 7) == 0, "pp_ema_table_build: table %p is not 8-byte aligned", table);
  long long nc = 0;
  if (int rc = ema_check_counts("pp_ema_table_build", n_tensors, counts, &nc)) return rc;
  for (int i = 0; i < n_tensors; ++i) {
    PP_REQUIRE(src[i] && dst[i], "pp_ema_table_build: tensor %d has a null pointer", i);
    PP_REQUIRE(((((uintptr_t)src[i]) | ((uintptr_t)dst[i])) & 3) == 0,
               "pp_ema_table_build: tensor %d has a pointer that is not 4-byte aligned", i);
    PP_REQUIRE(kinds[i] == PP_EMA_LERP_F32 || kinds[i] == PP_EMA_COPY_WORDS,
               "pp_ema_table_build: tensor %d has kind %d (0 = lerp_f32, 1 = copy_words)", i, kinds[i]);
  }
  // every dst range must be disjoint from every src range and from every other dst range: a chunk reads and writes
  // only its own elements, so nothing else orders one workgroup's store against another's load
  for (int i = 0; i < n_tensors; ++i) {
    const uintptr_t d0 = (uintptr_t)dst[i], d1 = d0 + 4 * (uintptr_t)counts[i];
    for (int j = 0; j < n_tensors; ++j) {
      const uintptr_t s0 = (uintptr_t)src[j], s1 = s0 + 4 * (uintptr_t)counts[j];
      PP_REQUIRE(d1 <= s0 || s1 <= d0, "pp_ema_table_build: dst of tensor %d overlaps src of tensor %d", i, j);
      if (j > i) {
        const uintptr_t e0 = (uintptr_t)dst[j], e1 = e0 + 4 * (uintptr_t)counts[j];
        PP_REQUIRE(d1 <= e0 || e1 <= d0, "pp_ema_table_build: dst of tensor %d overlaps dst of tensor %d", i, j);
      }
    }
  }
  EmaHeader *hdr = reinterpret_cast<EmaHeader *>(table);
  hdr->magic = kEmaMagic;
  hdr->n_tensors = n_tensors;
  hdr->n_chunks = (int)nc;
  hdr->chunk_elems = kEmaChunk;
  for (int k = 0; k < 4; ++k) hdr->pad[k] = 0;
  const EmaView w = ema_view_of(table, n_tensors);
  EmaTensor *T = const_cast<EmaTensor *>(w.tensors);
  for (int i = 0; i < n_tensors; ++i) T[i] = EmaTensor{src[i], const_cast<void *>(dst[i]), counts[i], kinds[i], 0};
  int2 *cm = const_cast<int2 *>(w.chunks);
  long long c = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const int k = (int)((counts[i] + kEmaChunk - 1) / kEmaChunk);
    for (int j = 0; j < k; ++j) cm[c++] = make_int2(i, j);
  }
  *n_chunks = (int)nc;
  return 0;
}

extern "C" int pp_ema_update(const void *table, int n_chunks, double weight, void *stream) {
  using namespace pp;
  PP_REQUIRE(table, "pp_ema_update: null table");
  PP_REQUIRE((((uintptr_t)table) & 7) == 0, "pp_ema_update: table %p is not 8-byte aligned", table);
  PP_REQUIRE(n_chunks > 0, "pp_ema_update: n_chunks=%d (an update needs at least one tensor)", n_chunks);
  PP_REQUIRE(weight >= 0.0 && weight <= 1.0, "pp_ema_update: weight=%g is not in [0, 1]", weight);
  hipLaunchKernelGGL(ema_update_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, weight);
  PP_CHECK_LAUNCH("ema_update_kernel");
  return 0;
}
