// The K-loop of the "Duo" form (gemm_duo_kernel in pp_gemm.hip, qkv_attention_kernel in pp_attention.hip): one 192x192
// tile on FOUR waves (2 x 2, 96x96 per wave), K-tiles of 32 (64-byte rows), a ring of 3 LDS stages of 24 KB filled by
// LDS-DMA with counted vmcnt waits, ascending K.  The kernel owns the operand addressing (which rows, clamps, zero
// lines) and the accumulator's start value; staging, fragment reads, MFMAs and the pipeline are here, once.
// Swizzle for 64-byte rows: physical 16-B chunk = logical ^ perm[(row >> 2) & 3], perm = {0, 3, 2, 1}: every 16-lane
// group of a ds_read_b128 (rows r .. r+15, chunk = lane >> 4) covers all 16 bank slots of the 256-byte LDS row.
#pragma once
#include <type_traits>
#include <utility>

#include "pp_gemm_shared.h"

namespace pp {

// XCD-blocked tile order: workgroups go round-robin to the 8 XCDs, each with its own L2, so workgroup ids are dealt out
// in blocks of 8 x rn tiles per XCD (8 row tiles whose A panels are shared by the block's rn column tiles).  The grid
// is rounded up to whole groups of 8 blocks: false = this workgroup has no tile.
constexpr int DUO_XCD_RM = 8;
__device__ __forceinline__ bool duo_blocked_tile(unsigned bid, int rn, int tiles_m, int tiles_n, int &tm, int &tn) {
  constexpr int RM = DUO_XCD_RM;
  const int RN = rn, RT = RM * RN;
  const int nbm = (tiles_m + RM - 1) / RM, nbn = (tiles_n + RN - 1) / RN;
  const int x = bid & 7, j = bid >> 3;
  const int g = (j / RT) * 8 + x, idx = j % RT;
  if (g >= nbm * nbn) return false;
  const int bmi = g / nbn, bni = g - bmi * nbn;
  tm = bmi * RM + idx / RN;
  tn = bni * RN + idx % RN;
  return tm < tiles_m && tn < tiles_n;
}

struct DuoLoop {
  static constexpr int BM = 192, BN = 192, STAGES = 3, BK = 32, RB = 64;          // RB: bytes of K per staged row
  static constexpr int PA = 3, PB = 3, PIECES = PA + PB, TM = 6, TN = 6;           // 1-KiB pieces (16 rows) per wave per K-tile
  static constexpr int A_BYTES = BM * RB, STAGE_BYTES = (BM + BN) * RB, LDS_BYTES = STAGES * STAGE_BYTES;
  static_assert(PIECES == TM, "one DMA piece per MFMA group");

  char *smem;
  // staging: lane -> (row in piece = lane >> 2, physical chunk = lane & 3); logical chunk = physical ^ perm.  The
  // kernel fills a_src / w_src for its rows: piece j of this wave holds tile rows piece_row(j) (A) and the same (W),
  // each pointer already advanced by lchunk_off.  A W row with w_ok false is a fixed zero line: it is not advanced in K.
  int prow, lchunk_off;
  const char *a_src[PA];
  const char *w_src[PB];
  bool w_ok[PB];
  int wave;
  unsigned lds0, st_ldsA, st_ldsB;
  size_t st_koff;
  unsigned offA, offB;

  __device__ __forceinline__ void init(char *smem_, int lane, int wave_) {
    smem = smem_;
    wave = wave_;
    prow = lane >> 2;
    const int pchunk = lane & 3;
    const int perm_p = (0x1230 >> (4 * ((prow >> 2) & 3))) & 3;      // {0, 3, 2, 1}[(row >> 2) & 3]
    lchunk_off = (pchunk ^ perm_p) * 16;
  }
  // second half of the set-up, once the kernel has filled a_src / w_src / w_ok
  __device__ __forceinline__ void init_ring(int lane, int wm, int wn) {
    lds0 = lds_offset_of(smem);
    st_ldsA = 0, st_ldsB = 0;
    st_koff = 0;
    // fragment offsets: row (w? * 96 + 16 i + frow), chunk fq ^ perm[(frow >> 2) & 3] (i only adds multiples of 16 rows)
    const int frow = lane & 15, fq = lane >> 4;
    const int perm_f = (0x1230 >> (4 * ((frow >> 2) & 3))) & 3;
    offA = (wm * 96 + frow) * RB + ((fq ^ perm_f) << 4);
    offB = A_BYTES + (wn * 96 + frow) * RB + ((fq ^ perm_f) << 4);
  }
  __device__ __forceinline__ int piece_row(int j) const { return (wave * PA + j) * 16 + prow; }

  __device__ __forceinline__ void stage_begin(int kt, int buf) {
    st_ldsA = __builtin_amdgcn_readfirstlane(lds0 + buf * STAGE_BYTES + wave * PA * 1024);
    st_ldsB = __builtin_amdgcn_readfirstlane(lds0 + buf * STAGE_BYTES + A_BYTES + wave * PB * 1024);
    st_koff = (size_t)kt * RB;
  }
  template <int q>
  __device__ __forceinline__ void stage_piece() {
    if constexpr (q < PA) {
      glds16(a_src[q] + st_koff, st_ldsA + q * 1024);
    } else {
      constexpr int j = q - PA;
      glds16(w_ok[j] ? w_src[j] + st_koff : w_src[j], st_ldsB + j * 1024);
    }
  }
  __device__ __forceinline__ void stage_all(int kt, int buf) {
    stage_begin(kt, buf);
    [&]<int... Q>(std::integer_sequence<int, Q...>) {
      (stage_piece<Q>(), ...);
    }(std::make_integer_sequence<int, PIECES>{});
  }

  template <bool DO_STAGE>
  __device__ __forceinline__ void compute(int buf, f32x4 (&acc)[TM][TN]) {
    const char *sb = smem + buf * STAGE_BYTES;
    uint4 bf[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const uint4 *>(sb + offB + j * 16 * RB);
    [&]<int... I>(std::integer_sequence<int, I...>) {
      ([&] {
        constexpr int i = I;
        const uint4 af = *reinterpret_cast<const uint4 *>(sb + offA + i * 16 * RB);
        if constexpr (DO_STAGE) {
          __builtin_amdgcn_sched_barrier(0);
          stage_piece<i>();        // PIECES == TM: one piece per MFMA group
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8 *>(&bf[j]),
                                                              *reinterpret_cast<const bf16x8 *>(&af), acc[i][j], 0, 0, 0);
      }(), ...);
    }(std::make_integer_sequence<int, TM>{});
  }

  // pipeline fill: the first STAGES - 1 K-tiles are requested; the kernel then sets its accumulators' start value
  __device__ __forceinline__ void fill(int nkt) {
#pragma unroll
    for (int s_ = 0; s_ < STAGES - 1; ++s_)
      if (s_ < nkt) stage_all(s_, s_);
  }
  // acc += A_tile W_tile^T over nkt K-tiles.  On return every DMA piece of this wave has landed and been consumed;
  // other waves may still be reading the last stage (the caller's barrier comes before the ring is reused).
  __device__ __forceinline__ void run(int nkt, f32x4 (&acc)[TM][TN]) {
    int buf = 0, kt = 0;
    for (; kt + STAGES - 1 < nkt; ++kt) {
      wait_vmcnt<(STAGES - 2) * PIECES>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      int nb = buf + STAGES - 1;
      if (nb >= STAGES) nb -= STAGES;
      stage_begin(kt + STAGES - 1, nb);
      compute<true>(buf, acc);
      if (++buf == STAGES) buf = 0;
    }
    for (; kt < nkt; ++kt) {
      if (kt + STAGES - 1 <= nkt) {
        wait_vmcnt<(STAGES - 2) * PIECES>();
      } else {
        wait_vmcnt<0>();
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      compute<false>(buf, acc);
      if (++buf == STAGES) buf = 0;
    }
  }
};

}  // namespace pp
