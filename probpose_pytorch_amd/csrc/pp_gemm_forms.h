// The tile forms of pp_gemm (its `tile` selector), one row each.  Everything the dispatcher knows about a form is read
// from here: the tile shape, the kernel family with its wave layout, the auto cost model's terms, the XCD block width
// of the grid, and what the form accepts.  Host only; no state.
#pragma once
#include "../../include/probpose_hip.h"

namespace pp {

enum class GemmFamily { Grid, Persist, Duo, QuadStream };   // gemm_kernel / gemm_persist_kernel / gemm_duo_kernel /
                                                            // gemm_quad_stream_kernel (pp_gemm_quad.hip)
constexpr unsigned DT_F32 = 1u << PP_F32, DT_BF16 = 1u << PP_BF16, DT_FP8 = 1u << PP_FP8, DT_ALL = DT_F32 | DT_BF16 | DT_FP8;
constexpr int EPI_ACT = PP_EPI_BIAS | PP_EPI_GELU | PP_EPI_RELU;

// measured: one 8-wave 3-stage 192x192 tile per CU vs two co-resident 4-wave tiles
constexpr double CFG3_SPEEDUP = 1.3;

constexpr const char *GRID_SERVES = "per-launch tiles 1 - 7 and 10 are built for f32 and bf16 (fp8: tiles 2, 3 and 10)";
constexpr const char *WIDE_SERVES =
    "the 256-wide tiles are built for bf16 only (fp32 fragments do not fit the register file)";
constexpr const char *QUAD_SERVES =
    "of the four-wave tiles 15 - 20, tiles 18 - 20 (the stream; 15 - 17 are removed) serve plain bf16 -> bf16 GEMMs with "
    "bias / GELU / ReLU epilogues";

// The defaults are those of a per-launch (Grid) form: it takes every epilogue and operand structure.
struct GemmForm {
  int tile, bm, bn;
  GemmFamily family = GemmFamily::Grid;
  int wgm = 2, wgn = 4, stages;  // MFMA waves per workgroup (wgm x wgn) and the depth of their LDS ring
  int nwp = 0;                   // Grid: extra DMA-only producer waves (the wave-specialised form)
  bool pingpong = false;         // Grid: the two wave quartets run half a K-tile apart
  int slots = 256;               // workgroups resident on the chip per launch round: 512 (two per CU) or 256 (one)
  double auto_rate = 0;          // auto cost model: relative per-CU throughput; 0 = auto never picks this form
  int auto_max_n = 0;            //   considered only for N <= this (0 = any N)
  bool auto_wins_ties = false;   //   takes an equal cost (every other candidate must be strictly cheaper)
  int xcd_rn = 4;                // column tiles per XCD block of the blocked tile order
  unsigned dtypes = DT_F32 | DT_BF16;   // DT_* the form is built for
  int epilogues = ~0;            // PP_EPI_* bits it accepts
  bool residual_f32_only = false;   // PP_EPI_RESIDUAL / PP_EPI_ROWBIAS only together with PP_EPI_OUT_F32
  bool plain = false;            // no rowoff, no out_rowmap, no batch > 1 or split-K (grid.y)
  bool lds_epilogue = false;     // the C tile must be able to leave through LDS as whole 16-byte chunks
  bool whole_tiles = false;      // M % bm == 0 and N % bn == 0
  int k_multiple = 1, k_min = 0; // K % k_multiple == 0 (on top of the dtype's own rule), K >= k_min
  bool c_below_4g = false;       // rows leave through 32-bit buffer offsets
  const char *serves = GRID_SERVES;   // what it serves, for the refusal of anything else
};

// four-wave stream (pp_gemm_quad.hip): one wave per SIMD, 128x96 / 96x144 / 96x128 wave tiles, one workgroup per CU
// walking its tiles as one stream of 32-deep K-tiles (in pairs behind a 4-deep ring)
constexpr GemmForm quad_stream_form(int tile, int bm, int bn) {
  return {.tile = tile, .bm = bm, .bn = bn, .family = GemmFamily::QuadStream, .wgn = 2, .stages = 4, .dtypes = DT_BF16,
          .epilogues = EPI_ACT | PP_EPI_HEADMAJOR, .plain = true, .lds_epilogue = true, .whole_tiles = true,
          .k_multiple = 64, .k_min = 512, .c_below_4g = true, .serves = QUAD_SERVES};
}

constexpr GemmForm GEMM_FORMS[] = {
    // 4 waves, 2 stages, two workgroups share a CU
    {.tile = 1, .bm = 128, .bn = 128, .wgn = 2, .stages = 2, .slots = 512, .auto_rate = 0.5, .xcd_rn = 8},
    {.tile = 2, .bm = 192, .bn = 96, .wgn = 2, .stages = 2, .slots = 512, .auto_rate = 0.5, .xcd_rn = 8, .dtypes = DT_ALL},
    // 8 waves, one workgroup per CU
    {.tile = 3, .bm = 192, .bn = 192, .stages = 3, .auto_rate = CFG3_SPEEDUP, .auto_wins_ties = true, .dtypes = DT_ALL},
    {.tile = 4, .bm = 192, .bn = 128, .stages = 3, .auto_rate = CFG3_SPEEDUP * 0.9},
    // narrow outputs (the N = 256 deconvolution layers): a taller tile restores the flop/byte ratio
    {.tile = 5, .bm = 384, .bn = 128, .stages = 2, .auto_rate = CFG3_SPEEDUP, .auto_max_n = 256},
    {.tile = 6, .bm = 192, .bn = 192, .stages = 3, .nwp = 4},   // wave-specialised: 8 MFMA waves + 4 DMA waves
    {.tile = 7, .bm = 192, .bn = 384, .stages = 2},             // wide-N layers such as fc1
    {.tile = 8, .bm = 256, .bn = 256, .stages = 2, .dtypes = DT_BF16, .serves = WIDE_SERVES},
    // N = 256 layers: one column tile, A read once; the one form that holds all 256 channels of a pixel
    {.tile = 9, .bm = 192, .bn = 256, .stages = 2, .dtypes = DT_BF16, .serves = WIDE_SERVES},
    // ping-pong: one wave quartet loads fragments and issues DMA while the other runs MFMAs
    {.tile = 10, .bm = 192, .bn = 192, .stages = 3, .pingpong = true, .dtypes = DT_ALL},
    // persistent: one workgroup per CU walks its tiles as one stream of K-tiles
    {.tile = 13, .bm = 192, .bn = 192, .family = GemmFamily::Persist, .stages = 3, .dtypes = DT_BF16,
     .epilogues = EPI_ACT | PP_EPI_HEADMAJOR, .plain = true, .lds_epilogue = true, .c_below_4g = true,
     .serves = "tile 13 (persistent) serves plain bf16 -> bf16 GEMMs with bias / GELU / ReLU epilogues only"},
    // two 4-wave workgroups per CU, 96x96 wave tiles, 32-deep K-tiles
    {.tile = 14, .bm = 192, .bn = 192, .family = GemmFamily::Duo, .wgn = 2, .stages = 3, .slots = 512, .dtypes = DT_BF16,
     .epilogues = EPI_ACT | PP_EPI_RESIDUAL | PP_EPI_OUT_F32 | PP_EPI_ROWBIAS, .residual_f32_only = true, .plain = true,
     .lds_epilogue = true, .k_multiple = 64,
     .serves = "tile 14 (two workgroups per CU) serves plain bf16 GEMMs (bias / GELU / ReLU / f32 residual) whose output "
               "rows are whole 16-byte chunks (N, ldc multiples of 8 for bf16 / 4 for f32 outputs, C 16-byte aligned)"},
    quad_stream_form(18, 256, 192), quad_stream_form(19, 192, 288), quad_stream_form(20, 192, 256),
};

// Selectors that once named a form: refused, with the reason.
struct RetiredTile { int first, last; const char *reason; };
constexpr RetiredTile GEMM_RETIRED[] = {
    {11, 12, "a round-2 experiment"},
    {15, 17, "a per-launch four-wave form that only lab builds had"},
};

constexpr int GEMM_TILE_RAGGED = 1;        // the one form with an element-wise (ragged N / heatmap store) variant
constexpr int GEMM_TILE_FP8_FALLBACK = 3;  // what auto selection falls back to when it picks a form fp8 is not built for
constexpr int GEMM_TILE_FUSE_FINAL = 9;    // PP_EPI_FUSE_FINAL runs on this form only

constexpr const GemmForm *gemm_form_or_null(int tile) {
  for (const GemmForm &f : GEMM_FORMS)
    if (f.tile == tile) return &f;
  return nullptr;
}
// compile-time lookup: naming a tile that has no row does not compile
consteval GemmForm gemm_form(int tile) { return *gemm_form_or_null(tile); }

}  // namespace pp
