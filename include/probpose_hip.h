/*
 * probpose_hip.h -- C ABI of libprobpose_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the ProbPose forward + decode hot path.
 * The reference (zir-vision/ProbPose_pytorch) has no FFI layer: its boundary
 * is the Python class API (probpose.model / backbone / head / codec).  The
 * Python host in probpose_pytorch_amd/ keeps that class API and binds these
 * entry points with ctypes; every entry point below cites the reference
 * interface (file:line, relative to the reference checkout) it replaces.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  All device buffers are
 *     caller-owned (torch tensors' data_ptr()); nothing is allocated here
 *     (where an entry point needs scratch, a *_workspace_bytes query sizes it).
 *   - every launch takes an explicit hipStream_t (as void*); calls are
 *     asynchronous and capturable into a hipGraph (no sync, no malloc).
 *   - return value: 0 = ok, <0 = error; pp_last_error() gives the message
 *     (thread-local).  No exceptions cross the ABI.
 *   - dtype enum: PP_F32 = 0 (fp32 storage, exact-fp32 MFMA), PP_BF16 = 1
 *     (bf16 storage, bf16 MFMA, fp32 accumulate), PP_FP8 = 2 (OCP e4m3 storage,
 *     block-scaled fp8 MFMA, fp32 accumulate; pp_gemm / pp_layernorm_fp8 /
 *     pp_attention_fp8out only).
 */
#ifndef PROBPOSE_HIP_H
#define PROBPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_F32 0
#define PP_BF16 1
#define PP_FP8 2                        /* OCP e4m3 storage (gfx950 fp8 MFMA), fp32 accumulate: pp_gemm / pp_layernorm_fp8 only */

#define PP_MAX_RADIUS 9                 /* heatmap.py:178-179: s<=3.0 -> ceil(3s)<=9 */
#define PP_MAX_TAPS (2 * PP_MAX_RADIUS + 1)

/* epilogue flags of pp_gemm (bit-or) */
#define PP_EPI_BIAS 1                   /* + bias[n]                                  */
#define PP_EPI_GELU 2                   /* GELU (timm Mlp act): exact erf in f32 mode; bf16 mode: fitted form, abs err <= 3e-5 */
#define PP_EPI_RELU 4                   /* ReLU (head.py:120)                         */
#define PP_EPI_RESIDUAL 8               /* out_f32 = residual_f32 + (acc + bias)      */
#define PP_EPI_OUT_F32 16               /* store fp32 regardless of the storage dtype */
#define PP_EPI_ROWBIAS 32               /* + rowbias[(m % rowbias_period) * ldc + n]  (pos_embed) */
#define PP_EPI_ROWSTATS 128              /* RETIRED (refused): round-1 LayerNorm fusion, producer side */
#define PP_EPI_LNFOLD 256                /* RETIRED (refused): round-1 LayerNorm fusion, consumer side.  The fusion cost
                                           +11..16 us per fused GEMM against the 12 us LayerNorm launch it replaced. */
#define PP_EPI_OUT_FP8 512              /* fp8 GEMM only: store e4m3(value * out_scale) instead of bf16 (the next fp8 GEMM's A) */
#define PP_EPI_NOCLAMP 1024             /* with PP_EPI_HEATMAP: store v / temperature unclamped (the Sparsemax path, head.py:526-528) */
#define PP_EPI_FUSE_FINAL 2048           /* bf16, N = 256 (tile 9): the epilogue also applies the final 1x1 heatmap layer
                                           (head.py:525-532) to the ReLU'd tile: C is the f32 NCHW heat buffer [B, hm_K, hm_HW],
                                           final_w [hm_K, 256] bf16, final_b [hm_K] f32, hm_K <= 32; the 256-channel map is
                                           never stored.  out_rowmap gives each GEMM row its pixel index b * hm_HW + hw. */
#define PP_EPI_HEADMAJOR 4096            /* bf16 qkv projection (timm attn.qkv): C is written [3][heads][M][head_dim] instead of
                                           [M][3 * heads * head_dim]; heads = hm_K, head_dim = hm_HW (fields reused), N = 3 * hm_K *
                                           hm_HW.  Read by pp_attention_headmajor. */
#define PP_EPI_HEATMAP 64               /* head.py:526-532: f32 NCHW store of clamp(v / temperature, 0, 1):
                                           C[((r / hm_HW) * hm_K + n) * hm_HW + r % hm_HW], r = output row */

int pp_version(void);
const char *pp_last_error(void);
/* 1 when a gfx950 device is visible to this process, else 0 (never throws). */
int pp_device_ok(void);

/* ------------------------------------------------------------------------
 * Fused decode.  Replaces, in one launch per batch (every map that fits LDS, at batch sizes up to ~1 536 maps of 64x48 /
 * ~512 of 96x72; larger 64x48 / 96x72 batches take two launches -- one wave per map, then the few flat maps it hands
 * over -- and maps beyond LDS, e.g. 256x256, three launches through a global-memory image):
 *   Codec.decode            probpose/codec.py:249-263
 *   ProbMap.decode          probpose/codec.py:214-239
 *   get_heatmap_expected_value + _get_subpixel_maximums
 *                           probpose/heatmap.py:291-395, :114-167
 *   the D2H copy of util.to_numpy   probpose/util.py:6-12
 * (OKS kernels of heatmap.py:170-194 arrive pre-factored as normalised 1-D
 * taps; the 2-D kernel is exactly their outer product.)
 *
 * heatmaps [B,K,H,W] f32 contiguous.  prob/vis/oks/err: [B*K] f32 or NULL.
 * taps [K][PP_MAX_TAPS] f64 (entry j = offset j - radius[k]), radius [K].
 * den_x/den_y = heatmap_size-1 ([W-1,H-1] of codec.py:237), in_w/in_h = input_size.
 * Outputs (each may be NULL): kpts f64 [B,K,2] (input-image space),
 * scores f32 [B,K] (raw heatmap at the integer peak), locs f32 [B,K,2]
 * (heatmap space, = get_heatmap_expected_value's locs), aux f32 [3,B,K]
 * (prob,vis,oks passthrough), err f64 [B,K] (= err / sqrt(H^2+W^2)),
 * conv f32 [B,K,H,W] (return_heatmap=True), packed f64 [B,K,7] = (kpt x, kpt y,
 * score, prob, vis, oks, err) per keypoint: the record the multi-GPU all-gather ships.
 * workspace: pp_decode_workspace_bytes() bytes, 4-byte aligned: a (B*K + 2)-int hand-over list for 64x48 / 96x72 maps
 * (the wave-per-map path; NULL selects the workgroup-per-map kernels instead) which the caller ZEROES ONCE when it
 * allocates it (every call returns its two counters to zero itself: no memset or reset launch) and must not share
 * between calls that may run concurrently; 0 for other maps that fit in LDS; a float64 + float32 image of the batch for
 * maps that do not.
 * flags: 0 = the default form per map size and batch size (64x48 / 96x72: the all-pixel kernel up to ~1 536 / ~512
 * maps, the wave-per-map kernel above); PP_DECODE_NO_WAVE / PP_DECODE_SCREEN / PP_DECODE_ALL_PIXEL select the
 * other implementations (A/B measurements and the equivalence tests: all forms return identical numbers).
 * ---------------------------------------------------------------------- */
#define PP_DECODE_NO_WAVE 1             /* not the wave-per-map kernel (64x48 / 96x72 maps)                  */
#define PP_DECODE_SCREEN 2              /* the workgroup-per-map screened kernel on every map that fits LDS  */
#define PP_DECODE_ALL_PIXEL 4           /* float64 convolution of every pixel (the round-1 kernel)          */
#define PP_DECODE_WAVE 16               /* the wave-per-map path at any batch size (default: above two rounds of the
                                           all-pixel kernel's resident workgroups, ~1 536 maps of 64x48)      */
size_t pp_decode_workspace_bytes(int B, int K, int H, int W);
int pp_decode_f32(const float *heatmaps, const float *prob, const float *vis,
                  const float *oks, const float *err, int B, int K, int H, int W,
                  const double *taps, const int *radius, double den_x, double den_y,
                  double in_w, double in_h, double *out_kpts, float *out_scores,
                  float *out_locs, float *out_aux, double *out_err, float *out_conv,
                  double *out_packed, void *workspace, int flags, void *stream);

/* ------------------------------------------------------------------------
 * Dense contraction on MFMA:  C[M,N] = epilogue(A[M,Kd] * W[N,Kd]^T).
 * Replaces torch.nn.Linear / Conv2d-as-GEMM call sites of the backbone
 * (timm VisionTransformer via probpose/backbone.py:26-39: patch_embed.proj,
 * attn.qkv, attn.proj, mlp.fc1, mlp.fc2) and of the head (head.py:227-233
 * final_layer, :262-285 aux convs, :459-469 deconvs after im2col-free row
 * gather).  A rows are addressed through an optional gather table so 3x3
 * convolutions and the four stride-2 deconvolution parities run as implicit
 * GEMMs with no im2col buffer:
 *   A(m, k) = Abase[ rowoff[(k / seg_len) * M + m] + (k % seg_len) ]   (rowoff<0 -> 0)
 * with rowoff == NULL meaning A(m,k) = Abase[m*lda + k].
 * batch > 1 runs independent problems (strideA/W/C/bias in elements).
 * dtype selects storage+MFMA type for A, W and (unless PP_EPI_OUT_F32) C.
 * ---------------------------------------------------------------------- */
typedef struct pp_gemm_args {
  const void *A; const void *W; void *C;
  const float *bias;            /* [N] f32 or NULL                      */
  const float *residual;        /* [M,ldc] f32 (PP_EPI_RESIDUAL)        */
  const float *rowbias;         /* [rowbias_period, ldc] f32            */
  const int32_t *rowoff;        /* [segs*M] element offsets or NULL     */
  const int32_t *out_rowmap;    /* [M] output row of GEMM row m, or NULL (identity);
                                   the stride-2 deconvolution parities scatter through it */
  int M, N, Kd;
  int lda, ldw, ldc;
  int seg_len;                  /* K-segment length for the gather      */
  int rowbias_period;
  int batch;
  long long strideA, strideW, strideC, strideBias, strideRowoff, strideRowmap;
  int dtype;                    /* PP_F32 | PP_BF16 | PP_FP8 (A, W e4m3 bytes; C bf16, or f32 / e4m3 by flag;
                                   K % 128 == 0; colsum = [N] f32 dequantisation scale per output column:
                                   C = act((A8 W8^T)[m,n] * colsum[n] + bias[n]) (+ residual); tiles 2, 3) */
  int epilogue;                 /* PP_EPI_* flags                       */
  int hm_K, hm_HW;              /* PP_EPI_HEATMAP geometry              */
  float hm_temperature;         /* head.py:107 (0.5)                    */
  void *C2;                     /* reserved (retired LayerNorm fusion): must be NULL / 0; kept so the struct layout
                                   of round 1 binaries and bindings stays valid                          */
  int ldc2;
  float *stats_out;             /* reserved */
  const float *stats_in;        /* reserved */
  int stats_parts;              /* reserved */
  const float *colsum;          /* PP_FP8: [N] f32 column scales (batch stride strideBias)               */
  float ln_eps;                 /* reserved */
  int tile;                     /* the tile form, one line per row of csrc/pp_gemm_forms.h (BM x BN, waves, LDS stages):
                                    0 = auto: the cheapest of 1 - 5 by rounds of resident workgroups x padded tile area
                                    1 = 128x128, 4 waves, 2 stages, two workgroups per CU; f32 / bf16; also every ragged call
                                    2 = 192x96, 4 waves, 2 stages, two workgroups per CU; f32 / bf16 / fp8
                                    3 = 192x192, 8 waves, 3 stages, one workgroup per CU; f32 / bf16 / fp8
                                    4 = 192x128, 8 waves, 3 stages; f32 / bf16
                                    5 = 384x128, 8 waves, 2 stages; f32 / bf16; auto considers it for N <= 256
                                    6 = 192x192 wave-specialised, 8 MFMA + 4 DMA waves, 3 stages; f32 / bf16
                                    7 = 192x384, 8 waves, 2 stages; f32 / bf16
                                    8 = 256x256, 8 waves, 2 stages; bf16
                                    9 = 192x256, 8 waves, 2 stages; bf16; the form of PP_EPI_FUSE_FINAL
                                   10 = 192x192 ping-pong, 8 waves, 3 stages, wave quartets half a K-tile apart; f32 / bf16 / fp8
                                   13 = 192x192 persistent stream, 8 waves, 3 stages; plain bf16 -> bf16, bias / GELU / ReLU
                                   14 = 192x192 as two 4-wave workgroups per CU; plain bf16, bias / GELU / ReLU / f32 residual
                                   18 / 19 / 20 = 256x192 / 192x288 / 192x256 four-wave stream (pp_gemm_quad.hip); plain bf16
                                        -> bf16, bias / GELU / ReLU, M and N whole numbers of tiles, K >= 512
                                   11, 12 (round-2 experiments), 15 - 17 (per-launch four-wave forms): removed, refused. */
  float out_scale;              /* PP_EPI_OUT_FP8: 1 / (scale of the fp8 output tensor) */
  int splitk;                   /* 0 / 1 = off.  S > 1: the launch computes S partial products per batch entry, split s
                                   over the K range [s * Kd, (s + 1) * Kd) (Kd = the PER-SPLIT depth): operands advance
                                   by the *_k strides below, the f32 partials go to C + s * strideC_k and are summed by
                                   the consumer (pp_maxpool_relu_sum).  Only with epilogue == PP_EPI_OUT_F32 (no bias,
                                   activation or residual); gather segments must not straddle a split (Kd % seg_len == 0).
                                   Used for the long-K, few-row aux convolutions (head.py:255-405 stages 2, 3). */
  long long strideA_k, strideW_k, strideC_k, strideRowoff_k;   /* elements per split step */
  const void *final_w;          /* PP_EPI_FUSE_FINAL */
  const float *final_b;
} pp_gemm_args;
int pp_gemm(const pp_gemm_args *args, void *stream);

/* LayerNorm over the last dim (timm Block.norm1/norm2/final norm, eps 1e-6).
 * x [rows,C] f32 (the fp32 residual stream) -> out [rows,C] in `dtype`. */
int pp_layernorm(const float *x, const float *gamma, const float *beta, float eps,
                 int rows, int C, void *out, int dtype, void *stream);
/* Same, output quantised to OCP e4m3: out[r,c] = e4m3(LN(x)[r,c] * inv_scale) (static per-tensor scale). */
int pp_layernorm_fp8(const float *x, const float *gamma, const float *beta, float eps,
                     int rows, int C, unsigned char *out, float inv_scale, void *stream);

/* Multi-head self-attention (timm Attention.forward: softmax(q k^T * hd^-1/2) v).
 * qkv [B*N, 3*heads*hd] laid out [3][heads][hd] along the row (timm's
 * reshape(B,N,3,heads,hd)); out [B*N, heads*hd]. */
int pp_attention(const void *qkv, void *out, int B, int N, int heads, int hd,
                 int dtype, void *stream);
/* Same attention on a HEAD-MAJOR bf16 qkv, [3][heads][B*N][hd] as the qkv GEMM writes it with PP_EPI_HEADMAJOR (one
 * head's rows contiguous: whole cache lines for head_dim 80 / 32); out [B*N, heads*hd] row-major as above.
 * The streaming MFMA kernel, head_dim 32 / 64 / 80, any N. */
int pp_attention_headmajor(const void *qkv, void *out, int B, int N, int heads, int hd, void *stream);
/* Same on bf16 qkv, output quantised to OCP e4m3: out[., c] = e4m3(o * inv_scale) (fp8 mode: the A operand of
 * the fp8 proj GEMM).  MFMA kernels only (head_dim 32 / 64 / 80). */
int pp_attention_fp8out(const void *qkv, unsigned char *out, int B, int N, int heads, int hd,
                        float inv_scale, void *stream);

/* attn.qkv and the attention of one ViT block in ONE launch (timm Attention.forward: qkv = self.qkv(x), then
 * softmax(q k^T * hd^-1/2) v), for N = 192 tokens per crop (256x192 input) and head_dim 64, bf16: q, k and v stay in
 * LDS and never go to memory.  h [B*192, C] bf16 (the LayerNorm output); w_hm [heads*192, C] bf16 and b_hm
 * [heads*192] f32 = qkv.weight / qkv.bias with the rows permuted HEAD-MAJOR: row 192 h + 64 t + d is row
 * t C + 64 h + d of the original (t = 0, 1, 2 for q, k, v), so one head's q, k and v rows are one 192-row panel;
 * out [B*192, C] bf16, bit-identical to pp_gemm (tile 14, PP_EPI_BIAS) followed by pp_attention.
 * Refused: C != 64 heads, C % 64 != 0, C < 128, operands not 16-byte aligned, B * heads beyond one launch's grid. */
int pp_qkv_attention_bf16(const void *h, const void *w_hm, const float *b_hm, void *out, int B, int heads, int C,
                          void *stream);

/* Patch im2col + cast: x [B,3,H,W] f32 NCHW -> A [B*gh*gw, 3*p*p] (k = c*p*p + py*p + px),
 * the A operand of patch_embed.proj as a GEMM (timm PatchEmbed, stride = patch). */
int pp_patchify(const float *x, void *out, int B, int H, int W, int patch, int dtype,
                void *stream);

/* Split-K consumer of the aux convolutions: x = nsplit f32 partial maps [nsplit][B, h, w, C] (split stride
 * `split_stride` elements), bias [C] f32 -> out [B, h/kh, w/kw, C] in `dtype` = ReLU(MaxPool(sum_s x_s + bias))
 * (head.py:271-276 behind a conv whose K was split over workgroups). */
int pp_maxpool_relu_sum(const float *x, int nsplit, long long split_stride, const float *bias, void *out, int B, int h,
                        int w, int C, int kh, int kw, int dtype, void *stream);

/* MaxPool(kh,kw stride kh,kw) + ReLU on channels-last rows (head.py:271-276):
 * x [B, h, w, C] -> out [B, h/kh, w/kw, C]. */
int pp_maxpool_relu(const void *x, void *out, int B, int h, int w, int C, int kh, int kw,
                    int dtype, void *stream);

/* Final 1x1 conv + /temperature + clamp(0,1), channels-last rows -> NCHW float32 (head.py:525-532),
 * as a streaming (HBM-bound) kernel for small K:  x [B*HW, Cin], w [K, Cin], bias [K] ->
 * heat [B, K, HW] f32 = clamp((x w^T + bias) / temperature, 0, 1).  (K*Cin*sizeof + 64 rows must fit
 * LDS; larger final layers / k > 1 kernels go through pp_gemm with PP_EPI_HEATMAP.)
 * A NaN pre-activation gives 0 (the clamp is fminf(fmaxf(v, 0), 1), which returns the non-NaN operand), exactly as the
 * PP_EPI_HEATMAP epilogue of pp_gemm does, so the two routes of one layer agree; torch.clamp would keep the NaN.
 * +Inf gives 1, -Inf gives 0. */
int pp_final_heatmap(const void *x, const void *w, const float *bias, float *out, int B, int HW,
                     int Cin, int K, float temperature, int dtype, void *stream);

/* Same contraction without the clamp: logits = (x w^T + bias) / temperature, the input of the Sparsemax
 * normalisation (head.py:526-528 with normalize != None).  Nothing is clamped: a NaN or Inf pre-activation is
 * written as it is. */
int pp_final_logits(const void *x, const void *w, const float *bias, float *out, int B, int HW,
                    int Cin, int K, float temperature, int dtype, void *stream);

/* Sparsemax over the last axis of x [rows, n] f32 (in place), then * scale and clamp(0, 1): head.py:237-245
 * (normalize_layer = Sparsemax(dim=-1), third-party sparsemax==0.1.9: restated from the published algorithm,
 * Martins & Astudillo 2016 -- parity unpinned) + head.py:529-531 (x * normalize, clamp).  One workgroup per row.
 * A row that holds a NaN or +Inf comes back NaN in every element, as the library's max(0, input - taus) with a NaN
 * tau and torch.clamp give; every other row is unaffected by it. */
int pp_sparsemax_rows(float *x, long long rows, int n, float scale, void *stream);

/* ArgMaxProbMap.decode (codec.py:515-543): raw arg-max of every heatmap (heatmap.py:13-52 get_heatmap_maximum)
 * refined by DARK-UDP (codec.py:315-375: Gaussian blur codec.py:284-313, clip, log, 3x3 Hessian step), rescaled to
 * input pixels.  heatmaps [B,K,H,W] f32; taps_host = the ksize float32 coefficients of cv2.getGaussianKernel(ksize, 0)
 * (host memory, copied into the launch); outputs kpts [B,K,2] f64, scores [B,K] f32 (raw maxima), locs [B,K,2] f32
 * (integer arg-max, (-1,-1) where the maximum is <= 0).  cv2 is not importable here: parity unpinned. */
size_t pp_dark_decode_lds_bytes(int H, int W, int ksize);
int pp_dark_decode_f32(const float *heatmaps, int B, int K, int H, int W, const float *taps_host, int ksize,
                       double in_w, double in_h, double *out_kpts, float *out_scores, float *out_locs, void *stream);

/* Aux tail: 1x1 conv C->K on pooled 1x1 features + Sigmoid/ReLU (head.py:277-286,:391-400).
 * x [B, 4*C] (one row per crop, the four branches' C columns side by side: branch br at columns br*C ..), w [4][K][C],
 * bias [4][K] -> out [4][B,K] f32 (branches 0..2 sigmoid, 3 relu).  The ReLU is fmaxf(s, 0): a NaN pre-activation
 * of branch 3 gives 0 (torch.relu would keep it); the sigmoid branches keep a NaN. */
int pp_aux_tail(const void *x, const void *w, const float *bias, float *out, int B, int C,
                int K, int dtype, void *stream);

/* (B,N,C) tokens -> (B,C,gh,gw) f32, the permute of backbone.py:40. */
int pp_tokens_to_nchw(const void *x, float *out, int B, int N, int C, int dtype, void *stream);
/* (B,C,h,w) f32 NCHW -> (B,h*w,C) channels-last rows in `dtype` (head entry when
 * ProbMapHead.forward is called on a foreign NCHW feature map). */
int pp_nchw_to_tokens(const float *x, void *out, int B, int C, int HW, int dtype, void *stream);

/* ------------------------------------------------------------------------
 * Front end: person boxes of one RGB frame -> network input crops.  Replaces
 *   dataset.py:71-90   scale_box: image.crop(box).resize(image_size, PIL.Image.LANCZOS)
 *   inference.py:74-82 image.resize(input_size, LANCZOS), v2.ToImage(), v2.ToDtype(float32, scale=True)
 * (the arithmetic is Pillow's: Image.crop zero-pads outside the frame; ImagingResample, 8 bits per
 * channel, Lanczos-3, two passes with a uint8 intermediate, 22-bit fixed-point coefficients).
 * Bit-exact against Pillow.
 *
 * boxes_xyxy [n][4] int32: (x0, y0, x1, y1) AFTER Image.crop's rounding (int(round(v)) in Python).
 * pp_frontend_plan_bytes / pp_frontend_plan_build run on the HOST (no GPU needed): they compute, with
 * Pillow's own double-precision expressions, the per-box bounds / coefficient tables and the
 * workgroup table into `plan` (host memory); the caller copies `plan` to the device.
 * pp_frontend_crop_resize: image uint8 HWC RGB on the device (img_stride = bytes per row), plan_dev =
 * the device copy of the plan, out [n][3][out_h][out_w] f32 in [0,1] (= f32(u8) * f32(1/255)).
 * ---------------------------------------------------------------------- */
long long pp_frontend_plan_bytes(int n_boxes, const int *boxes_xyxy, int out_w, int out_h);   /* < 0: error */
int pp_frontend_plan_build(int n_boxes, const int *boxes_xyxy, int out_w, int out_h, void *plan,
                           int *n_blocks_out, long long *lds_bytes_out);
int pp_frontend_crop_resize(const unsigned char *image, int img_w, int img_h, long long img_stride,
                            const void *plan_dev, int n_boxes, int n_blocks, long long lds_bytes,
                            int out_w, int out_h, float *out, void *stream);

/* ------------------------------------------------------------------------
 * Multi-source front end: pp_frontend_crop_resize with a source image PER BOX, so that one launch resizes a training
 * batch of crops cut from different images (dataset.py:116-122 for a whole batch).  The sources lie in one packed
 * uint8 buffer; box c reads the region sources[c] = {byte offset into the buffer, width, height, row stride in bytes}
 * (int64 each, RGB, 3 bytes per pixel) and boxes_xyxy[c] is in that region's pixel frame (pixels outside the region
 * are zero, as Image.crop pads).  Several boxes may name the same region.
 *
 * Every offset must be a multiple of PP_FRONTEND_SRC_ALIGN, and every region must end at least PP_FRONTEND_SRC_PAD
 * bytes before the end of the buffer (src_bytes): the kernel loads dwords that start at any byte of a region's rows,
 * never one that starts outside them, so with that padding no load leaves the buffer, the last region's included.
 * pp_frontend_multi_plan_build (HOST, no GPU needed) checks both and emits the same bounds and 22-bit coefficient
 * tables as pp_frontend_plan_build, the source records, and one workgroup table (box, first output row) over the
 * whole batch: ONE launch.  The plan must be 8-byte aligned on the device.  Per box the result has the bits that
 * pp_frontend_crop_resize gives for the same box on the same pixels.
 * ---------------------------------------------------------------------- */
#define PP_FRONTEND_SRC_ALIGN 4
#define PP_FRONTEND_SRC_PAD 4
long long pp_frontend_multi_plan_bytes(int n_boxes, const int *boxes_xyxy, int out_w, int out_h);   /* < 0: error */
int pp_frontend_multi_plan_build(int n_boxes, const int *boxes_xyxy, const long long *sources, long long src_bytes,
                                 int out_w, int out_h, void *plan, int *n_blocks_out, long long *lds_bytes_out);
int pp_frontend_crop_resize_multi(const unsigned char *src, const void *plan_dev, int n_boxes, int n_blocks,
                                  long long lds_bytes, int out_w, int out_h, float *out, void *stream);

/* ------------------------------------------------------------------------
 * Ground truth of a training batch apart from the maps (dataset.py:87-89, :121-135; codec.py:176-178, :195-204), all
 * on the device.  kpts_raw [B,K,3] f32: (x, y, v) in image pixels, v in {0, 2} (a labelled 1 is 2 already);
 * boxes_xywh [B,4] f64: the UN-rounded boxes.  Writes
 *   kpts_crop [B,K,2] f32   (x - f32(box_x)) / f32(box_w) * f32(in_w), likewise y: three separate IEEE float32
 *                           operations, as numpy evaluates scale_box on a float32 array
 *   kpts_hm   [B,K,2] f32   kpts_crop / scale (float32 division; scale = (input - 1) / (heatmap - 1) in float32)
 *   encode_visible [B,K] f32  1 where v == 2, else 0: the `visible` input of pp_encode_probmaps
 *   in_image  [B,K] u8      0 <= x < in_w and 0 <= y < in_h on kpts_crop
 *   keypoints_visible [B,K] u8   v == 2
 *   keypoints_visibility [B,K] f32   min(v, 1)
 * ---------------------------------------------------------------------- */
int pp_dataset_ground_truth(const float *kpts_raw, const double *boxes_xywh, int B, int K, int in_w, int in_h,
                            float scale_x, float scale_y, float *kpts_crop, float *kpts_hm, float *encode_visible,
                            unsigned char *in_image, unsigned char *keypoints_visible, float *keypoints_visibility,
                            void *stream);

/* ------------------------------------------------------------------------
 * Augmented training batches (YOLOPoseDataset(augment=...); geometry: DESIGN §4.4c).  The host folds flip, scale,
 * rotation and shift into two 2x3 matrices per sample; one launch warps the batch, one moves the keypoints.
 *
 * pp_augment_warp: src and sources are the packed buffer and the {byte offset, width, height, row stride} int64
 * records of the multi-source front end, under the same alignment and padding rules.  warp [n, 8] f64 per sample:
 * m00 m01 m02 m10 m11 m12 c b.  For output pixel (u, v): x = (m00 * u + m01 * v) + m02, y likewise with m1., in
 * float64 in this order: the region's pixel-index coordinates (pixel (i, j) centred at (i, j)).  Bilinear over the
 * taps floor(x), floor(x) + 1 (and y), a tap outside the region being zero, with float32 weights fx = f32(x -
 * floor(x)) and 1 - fx: top = p00 * wx0 + p01 * wx1, bot = p10 * wx0 + p11 * wx1, val = top * wy0 + bot * wy1, then
 * val / 255 and clamp(f32(c) * val + f32(b), 0, 1).  out [n, 3, in_h, in_w] f32.  The taps are read bytewise inside
 * the region's rows only.
 *
 * pp_dataset_ground_truth_affine: pp_dataset_ground_truth with kp_affine [B, 8] f32 per sample (a00 a01 a02 a10 a11
 * a12 flip 0) in place of the boxes: kpts_crop = ((a00 * kx + a01 * ky) + a02, (a10 * kx + a11 * ky) + a12) in
 * float32 in this order.  Where flip is 1, output slot k takes coordinates and visibility of source keypoint
 * perm[k] (perm [K] int32, an involution).  Every other output is formed from kpts_crop as pp_dataset_ground_truth
 * forms it.
 *
 * pp_augment_check (HOST, no GPU needed) refuses what the launches cannot check on device memory: a region that
 * breaks the rules of pp_frontend_multi_plan_build, a matrix or colour term that is not finite (or beyond 1e12), a
 * singular matrix, a flip flag other than 0 or 1, and a permutation that leaves 0..K-1 or is not an involution.
 * ---------------------------------------------------------------------- */
int pp_augment_check(int n, const long long *sources, long long src_bytes, const double *warp,
                     const float *kp_affine, int K, const int *perm);
int pp_augment_warp(const unsigned char *src, const long long *sources, const double *warp, int n, int in_w,
                    int in_h, float *out, void *stream);
int pp_dataset_ground_truth_affine(const float *kpts_raw, const float *kp_affine, const int *perm, int B, int K,
                                   int in_w, int in_h, float scale_x, float scale_y, float *kpts_crop,
                                   float *kpts_hm, float *encode_visible, unsigned char *in_image,
                                   unsigned char *keypoints_visible, float *keypoints_visibility, void *stream);

/* ------------------------------------------------------------------------
 * The pixel steps behind the warp (Augment's blur_* / median_* / erase_* settings): a box or median
 * blur, then coarse dropout, one launch for the batch.
 *
 * records [n, 24] int32 per sample: {kind, k, n_holes, fill (f32 bits), 4 x {x0, y0, x1, y1}, 4 x 0}.  in and out are
 * [n, 3, in_h, in_w] f32, the warp's layout.  Per sample and channel, in this order:
 *   1. filter (filters = 1 only).  kind 1: the mean of the k x k window in float32 (k * k - 1 additions, one division
 *      by k * k).  kind 2: the median of the k x k window, an element of the window, so exact.  Both with reflect-101
 *      borders: index -i reads i, index W - 1 + i reads W - 1 - i.  kind 0: a copy (its k is 0).
 *   2. holes: every pixel inside any of the first n_holes half-open rectangles [x0, x1) x [y0, y1) becomes fill.
 * filters = 0: the kind fields are not read and only the holes are written; in == out is allowed, and a workgroup
 * whose PP_AUGMENT_POST_TILE_W x PP_AUGMENT_POST_TILE_H tile meets no hole writes nothing.  filters = 1 requires that
 * in and out do not overlap.  128-bit stores where in_w % 4 == 0 and both buffers are 16-byte aligned, scalar stores
 * otherwise.  No load leaves `in`, whatever the records hold.
 *
 * pp_augment_post refuses on the host, before any launch: null or misaligned (not 4-byte) buffers, n, in_w or in_h
 * below 1, a mode other than 0 and 1, 2^31 or more elements, and the overlaps above.
 *
 * pp_augment_post_check (HOST, no GPU needed) refuses what the launch cannot check on device memory: a kind outside
 * 0..2; a k that is even, not one of 3, 5, 7 (box) or 3, 5 (median), above min(in_w, in_h), or not 0 with kind 0;
 * n_holes outside 0..4; one of the first n_holes rectangles that is empty or leaves the crop; a fill that is not
 * finite; a non-zero reserved word; any kind != 0 when filters = 0.
 * ---------------------------------------------------------------------- */
#define PP_AUGMENT_POST_TILE_W 64
#define PP_AUGMENT_POST_TILE_H 16
int pp_augment_post_check(int n, const int *records, int in_w, int in_h, int filters);
int pp_augment_post(const float *in, const int *records, int n, int in_w, int in_h, int filters, float *out,
                    void *stream);

/* ------------------------------------------------------------------------
 * Flip test at inference (ProbPoseModel(..., flip_pairs=...)).  float32 only.
 *
 * pp_hflip_pair: x [B,C,H,W] -> out [2B,C,H,W]: out[b] = x[b] and out[B + b, c, y, u] = x[b, c, y, W - 1 - u], the
 * batch and its mirror image in one launch (bit copies: nothing is computed on the values).
 *
 * pp_flip_merge: heat2 [2B,K,H,W] and aux2 [4,2B,K] (the head's probability, visibility, oks and error planes) ->
 *   heat_out[b, k, y, u] = (heat2[b, k, y, u] + heat2[B + b, perm[k], y, W - 1 - u]) * 0.5f      [B,K,H,W]
 *   aux_out[j, b, k]     = (aux2[j, b, k] + aux2[j, B + b, perm[k]]) * 0.5f                      [4,B,K]
 * in float32 in exactly this order (one add, one multiply by 0.5).  perm [K] int32 on the device, an involution
 * (left <-> right keypoints); the caller validates it.  One launch for the five outputs; no atomics.
 *
 * Both refuse on the host, before any launch: null pointers, non-positive sizes, more than 2^31 elements in the
 * 2B-batch tensor, and an output that overlaps an input (no in-place use).  W % 4 == 0 with 16-byte aligned
 * pointers takes the 128-bit form (4 pixels a thread), anything else one pixel a thread.
 * ---------------------------------------------------------------------- */
int pp_hflip_pair(const float *x, float *out, int B, int C, int H, int W, void *stream);
int pp_flip_merge(const float *heat2, const float *aux2, const int *perm, int B, int K, int H, int W,
                  float *heat_out, float *aux_out, void *stream);

/* ------------------------------------------------------------------------
 * Training targets: the OKS probability maps of ProbMap.encode, batched over crops.  Replaces
 *   generate_probmaps   probpose/codec.py:11-70  (called from ProbMap.encode, codec.py:176-182)
 * kpts_hm [B,K,2] f32: keypoints in HEATMAP pixels (= keypoints / scale_factor, codec.py:178);
 * visible [B,K] f32; two_s [K] f64 = 2 * s_k with s_k the per-keypoint (or overriding) variance of
 * codec.py:61-66, computed by the caller in float64.  Outputs: heatmaps [B,K,H,W] f32 (zero for
 * visible < 0.5), weights [B,K] f32 (= visible for skipped keypoints, else map.max() > 0).
 * ---------------------------------------------------------------------- */
int pp_encode_probmaps(const float *kpts_hm, const float *visible, const double *two_s, int B, int K, int H,
                       int W, float *heatmaps, float *weights, void *stream);

/* ------------------------------------------------------------------------
 * Evaluation metric: PCK over a batch of keypoint pairs in one pass.  Replaces the per-instance host code
 *   _calc_distances        probpose/heatmap.py:55-89   (normalised distances, -1 for masked-out pairs)
 *   _distance_acc          probpose/heatmap.py:92-111  (fraction below the threshold)
 *   keypoint_pck_accuracy  probpose/loss.py:825-866    (called from pose_pck_accuracy, loss.py:767-822)
 * pred / gt [N,K,2] float32 (coord_f64 = 0) or float64 (coord_f64 = 1): the difference is formed in that type;
 * mask [N,K] u8; norm [N,2] f64 with the reference's "<= 0 -> 1e6" substitution already applied, skip[n] = 1 for an
 * instance whose normalisation factor held an exact 0 (heatmap.py:78-82); thr: the threshold as the comparison sees it
 * (a Python float compared with a float32 array is rounded to float32 by numpy 2).  Outputs: counts [2][K] int32 =
 * (pairs below thr, valid pairs) per keypoint (zeroed here by a memset node), dist [K,N] f32 or NULL.
 * ---------------------------------------------------------------------- */
/* get_heatmap_maximum (probpose/heatmap.py:13-52) for `maps` = B*K contiguous H x W float32 maps of any size: locs
 * [maps,2] f32 = (x, y) of the first maximum in row-major order (a NaN counts as the maximum, like np.argmax),
 * (-1,-1) where the maximum is <= 0; vals [maps] f32 = the maximum. */
int pp_heatmap_argmax(const float *heatmaps, long long maps, int H, int W, float *locs, float *vals, void *stream);
int pp_pck_counts(const void *pred, const void *gt, int coord_f64, const unsigned char *mask, const double *norm,
                  const unsigned char *skip, double thr, int N, int K, int *counts, float *dist, void *stream);

/* ------------------------------------------------------------------------
 * Validation loss (forward only).  Replaces
 *   OKSHeatmapLoss.forward / _get_mask  probpose/loss.py:55-191  (pp_oks_heatmap_loss)
 *   ProbPoseLoss.forward                probpose/loss.py:360-510 with _error_from_heatmaps (:512-548),
 *                                        _oks_from_heatmaps (:550-640, its per-crop host decode replaced by
 *                                        the batched decodes above), compute_oks (:715-764), get_mae (:699-712)
 *                                        (pp_probpose_loss_terms)
 *
 * pp_oks_heatmap_loss: output / target [B,K,H,W] f32.  weights: NULL, [B,K] or, with weights_per_pixel,
 * [B,K,H,W] f32; mask: NULL or f32 [H,W] maps at mask + b * mask_sb + k * mask_sk (element strides; 0
 * broadcasts, e.g. mask_sk = 0 for a [B,1,H,W] mask); skip_empty: zero channels whose target is all 0;
 * oks_type 0 = minus, 1 = plus, 2 = both.  oks_weight is 1 - smoothing_weight - gaussian_weight (the caller's
 * float64 value).  Sobel gradients of `output` with zero 'same' padding, any H, W >= 1.  Outputs: per_pixel
 * [B,K,H,W] (optional), per_keypoint [B,K] (optional), scalars[3] = (mean of the per-keypoint loss, mean of
 * the per-pixel loss, number of target elements outside [0, 1]).  parts: caller-owned scratch of
 * B*K*5 floats.  Two launches; deterministic (fixed-order reductions, no float atomics).
 *
 * pp_probpose_loss_terms: gt_kpts / dt_kpts [B,K,2] f64 decoded coordinates (input-image pixels; gt may be
 * NaN for an empty map); in_image / annotated / visibility [B,K] int32 (the reference's .to(int) values);
 * dt_prob / dt_vis / dt_oks / dt_err [B*K] f32 predictions; variance [K] f64 = (2 sigma_k)^2; oks_area =
 * 0.53 * W * H + eps (loss.py:609-620 with heatmap_size = (W, H), compute_oks use_area=False).  Outputs
 * (all required): gt_oks, gt_err (0 with freeze_error), vis_weight [B*K] f32 (the normalised weights of
 * loss.py:439-450), oks_weight [B] f32 (1 for a crop with an in-image annotated keypoint), results[8] f32 =
 * (probability BCE, visibility BCE, OKS MSE, error L1Log, OKS MAE, error MAE, flags, #annotated in-image
 * keypoints); flags bit 0: no annotated keypoint (loss.py:448 raises), bit 1: a NaN error target
 * (loss.py:546 asserts), bit 2: a probability or visibility outside [0, 1].  One launch, one workgroup.
 * ---------------------------------------------------------------------- */
int pp_oks_heatmap_loss(const float *output, const float *target, const float *weights, int weights_per_pixel,
                        const float *mask, long long mask_sb, long long mask_sk, int skip_empty, int oks_type,
                        float smoothing_weight, float oks_weight, float gaussian_weight, float loss_weight, int B,
                        int K, int H, int W, float *per_pixel, float *per_keypoint, float *parts, float *scalars,
                        void *stream);
int pp_probpose_loss_terms(const double *gt_kpts, const double *dt_kpts, const int *in_image, const int *annotated,
                           const int *visibility, const float *dt_prob, const float *dt_vis, const float *dt_oks,
                           const float *dt_err, const double *variance, double oks_area, int B, int K,
                           int freeze_error, float *gt_oks, float *gt_err, float *vis_weight, float *oks_weight,
                           float *results, void *stream);

/* ------------------------------------------------------------------------
 * Training loss gradients.  Differentiate
 *   OKSHeatmapLoss.forward  probpose/loss.py:55-143  (pp_oks_heatmap_loss_backward, all three reductions)
 *   BCELoss / MSELoss / L1LogLoss as ProbPoseLoss.forward uses them, loss.py:232-339 and :419-464
 *                                                     (pp_probpose_loss_grads)
 * The targets (the gt heatmaps, the OKS and error targets from detached decodes), weights and masks are constants:
 * no gradient flows to them.  Deterministic: no float atomics, fixed-order sums.
 *
 * pp_oks_heatmap_loss_backward: output, target, weights, weights_per_pixel, mask and its strides, skip_empty,
 * oks_type, the three weights and loss_weight exactly as pp_oks_heatmap_loss.  reduction 0 = per pixel: the upstream
 * gradient G [B,K,H,W] at grad + b * grad_sb + k * grad_sk + r * grad_sh + c * grad_sw (element strides, 0
 * broadcasts); 1 = per keypoint: G [B,K] at grad + b * grad_sb + k * grad_sk; 2 = the scalar mean: G = grad[0];
 * 3 = the mean of the per-pixel loss (ProbPoseLoss's heatmap_loss_pxl.mean(), loss.py:427-431): G = grad[0].  The
 * upstream gradient is read on the device.  Output grad_output [B,K,H,W] f32, every element written:
 *   d/dh[q] = sum_p G[p] lw sw m[p] 2 (gx[p] Sx(q-p) + gy[p] Sy(q-p)) + G[q] lw m[q] (ow d oks/dh + gw 2 (h - t))
 * with p over the 3x3 neighbours of q inside the map (the per-pixel reductions).  The per-keypoint and mean reductions
 * take the max-gradient subgradient at the first maximal pixel of the masked energy in row-major order (a NaN counts
 * as the maximum), as torch's max(dim) does, and divide the mse term by H*W.  One launch, one workgroup per map.
 *
 * pp_probpose_loss_grads: dt_prob / dt_vis / dt_oks / dt_err [B*K] f32 predictions; gt_oks / gt_err [B*K] f32 the
 * targets pp_probpose_loss_terms wrote; in_image / annotated / visibility [B*K] int32 as there; u_prob, u_vis, u_oks,
 * u_err: the upstream gradients of results[0..3] of pp_probpose_loss_terms, one float each on the device.  Outputs
 * d_prob, d_vis, d_oks, d_err [B*K] f32: with N = B*K, g = u / N and w = annotated & in_image,
 *   BCE (probability vs in_image, visibility vs visibility): g (x - y) / max((1 - x) x, 1e-12)
 *   MSE (oks, weighted):                                    2 w (x w - y w) g
 *   L1Log (error, weighted):                                clamp(z, -1, 1) g w / (1 + x), z = (log(1 + x) - log(1 + y)) w
 * with 1 + x rounded to float32 (the reference's log(1 + x)).  The visibility BCE takes no weights: the reference's
 * BCELoss(use_target_weight=False) ignores the visibility weights it is handed.  One launch.
 * ---------------------------------------------------------------------- */
int pp_oks_heatmap_loss_backward(const float *output, const float *target, const float *weights, int weights_per_pixel,
                                 const float *mask, long long mask_sb, long long mask_sk, int skip_empty, int oks_type,
                                 float smoothing_weight, float oks_weight, float gaussian_weight, float loss_weight,
                                 int reduction, const float *grad, long long grad_sb, long long grad_sk,
                                 long long grad_sh, long long grad_sw, int B, int K, int H, int W, float *grad_output,
                                 void *stream);
int pp_probpose_loss_grads(const float *dt_prob, const float *dt_vis, const float *dt_oks, const float *dt_err,
                           const float *gt_oks, const float *gt_err, const int *in_image, const int *annotated,
                           const int *visibility, const float *u_prob, const float *u_vis, const float *u_oks,
                           const float *u_err, int B, int K, float *d_prob, float *d_vis, float *d_oks, float *d_err,
                           void *stream);

/* ------------------------------------------------------------------------
 * Training ProbMapHead (train-mode BatchNorm forward, backward).  Differentiate
 *   ConvTranspose2d / Conv2d weights and biases, head.py:174-235, 255-405   (pp_wgrad_gemm; input gradients run on
 *                                                      pp_gemm with transposed weights and pack.py's tables)
 *   BatchNorm2d in train mode, head.py:190-222, 270-400                     (pp_bn_train_stats, pp_bn_apply_relu,
 *                                                      pp_bn_pool_relu, pp_bn_train_backward)
 *   nn.MaxPool2d + ReLU of the aux branches, head.py:270-400                (pp_bn_pool_relu, pp_bn_train_backward
 *                                                      mode 2)
 *   the 1x1 aux tails + Sigmoid / ReLU, head.py:270-400                     (pp_aux_tail_backward)
 *   x / temperature, Sparsemax, * normalize, torch.clamp, head.py:526-532   (pp_heat_clamp, pp_heat_tail_backward)
 * No allocation, no host sync; every reduction in a fixed order (no float atomics): repeated calls give the same bits.
 *
 * pp_wgrad_gemm: dW[n, k] = sum_m dY(m, n) A(m, k), f32 out, MFMA with f32 accumulation (dtype of dY and A: PP_F32,
 * v_mfma_f32_16x16x4_f32; PP_BF16, v_mfma_f32_16x16x32_bf16), per batch entry b:
 *   dY(m, n) = dY[b * strideDY + (dy_rowmap ? dy_rowmap[b * strideRowmap + m] : m) * ldd + n]
 *   A(m, k)  = A[b * strideA + rowoff[b * strideRowoff + (k / seg_len) * M + m] + k % seg_len]  (-1 -> 0), or
 *              A[b * strideA + m * lda + k] when rowoff is NULL (the layout of pp_gemm's A)
 *   dW[b * strideDW + n * lddw + k];  dB (optional) [b * strideDB + n] = sum_m dY(m, n)
 * Shapes with few output tiles split M; the f32 partials go to ``parts`` (pp_wgrad_workspace_floats(M, N, Kd, batch)
 * floats; 0 = no split) and are summed in split order.
 *
 * pp_bn_train_stats: y [M, C] f32 (row pitch ldy), the batch mean and biased variance per channel (float64
 * accumulation in a fixed order), mean / rstd = 1/sqrt(var + eps) / scale = gamma rstd / shift = beta - mean scale
 * [C] f32 out; running_mean / running_var (may be NULL) <- (1 - momentum) r + momentum (mean, unbiased var).  M > 1.
 * ws: pp_bn_workspace_bytes(M, C) bytes, shared with pp_bn_train_backward.
 * pp_bn_apply_relu: out[r, c] = relu?(y[r, c] scale[c] + shift[c]) in dtype.
 * pp_bn_pool_relu: y [B*h*w, C] f32 -> out [B*(h/kh)*(w/kw), C] dtype = ReLU(MaxPool_{kh x kw, stride = kernel}(y scale
 *   + shift)), the first maximum in window scan order (a NaN wins); argmax [same] int32 = the winner's element index in
 *   y, -1 where the ReLU passes no gradient.
 * pp_bn_train_backward: the gradient g of the BN output z (mode 0: g [M, C] pitch ldg; mode 1: g where z > 0, z
 *   recomputed from y, scale, shift; mode 2: the MaxPool scatter of g [B*(h/kh)*(w/kw), C] through argmax) ->
 *   dbeta = sum g, dgamma = sum g xhat (either may be NULL), dx = gamma rstd (g - mean(g) - xhat mean(g xhat)) in dtype.
 * pp_aux_tail_backward: x [B, 4C] the pooled rows, w [4, K, C], out / gout [4, B, K] f32 (the forward's outputs and
 *   their upstream gradients) -> dW [4, K, C], dB [4, K], dx [B, 4C] f32 (each may be NULL); sigmoid for branches 0-2,
 *   ReLU for branch 3.
 * pp_heat_clamp: out = clamp(p scale, 0, 1) elementwise (a NaN stays a NaN).
 * pp_heat_tail_backward: p [B*K, HW] (the logits / T, or with sparse = 1 their Sparsemax), g [B*K, HW] the upstream
 *   gradient of the heatmaps -> dz[(b*HW + i) * ldz + k] in dtype: the gradient of the final layer's output (clamp
 *   mask 0 <= p scale <= 1 inclusive, * scale, Sparsemax backward s (g - sum(g s) / sum(s)), / temperature); columns
 *   K .. ldz-1 are written 0.  One workgroup per map.
 * ---------------------------------------------------------------------- */
typedef struct pp_wgrad_args {
  const void *dY; const int32_t *dy_rowmap; long long ldd;
  const void *A; const int32_t *rowoff; int seg_len; int lda;
  float *dW; long long lddw;
  float *dB;
  float *parts;
  int M, N, Kd, batch;
  long long strideDY, strideA, strideRowoff, strideRowmap, strideDW, strideDB;
  int dtype;
} pp_wgrad_args;

long long pp_wgrad_workspace_floats(int M, int N, int Kd, int batch);
int pp_wgrad_gemm(const pp_wgrad_args *args, void *stream);
long long pp_bn_workspace_bytes(int M, int C);
int pp_bn_train_stats(const float *y, long long ldy, int M, int C, const float *gamma, const float *beta, float eps,
                      float momentum, float *running_mean, float *running_var, float *mean, float *rstd, float *scale,
                      float *shift, void *ws, void *stream);
int pp_bn_apply_relu(const float *y, long long ldy, int M, int C, const float *scale, const float *shift, void *out,
                     long long ldo, int relu, int dtype, void *stream);
int pp_bn_pool_relu(const float *y, int B, int h, int w, int C, int kh, int kw, const float *scale, const float *shift,
                    void *out, int32_t *argmax, int dtype, void *stream);
int pp_bn_train_backward(const float *g, long long ldg, const float *y, long long ldy, int M, int C, const float *mean,
                         const float *rstd, const float *scale, const float *shift, const float *gamma, int mode,
                         const int32_t *argmax, int B, int h, int w, int kh, int kw, float *dgamma, float *dbeta,
                         void *dx, long long ldx, int dtype, void *ws, void *stream);
int pp_aux_tail_backward(const void *x, const void *w, const float *out, const float *gout, int B, int C, int K,
                         float *dW, float *dB, float *dx, int dtype, void *stream);
int pp_heat_clamp(const float *p, float *out, long long n, float scale, void *stream);
int pp_heat_tail_backward(const float *p, const float *g, int B, int K, int HW, float scale, int sparse,
                          float temperature, void *dz, int ldz, int dtype, void *stream);

/* ------------------------------------------------------------------------
 * Training ScratchViTBackbone (ScratchViTBackbone(differentiable=True) in .train() mode).  Differentiate the timm
 * VisionTransformer that probpose/backbone.py:23-40 builds (reached through ScratchViTBackbone.forward, model.py:10-11):
 *   Block.norm1 / norm2 and the final norm (LayerNorm, eps 1e-6)   (pp_layernorm_backward)
 *   Mlp.act (nn.GELU, exact erf) on the f32 fc1 pre-activation       (pp_gelu_forward, pp_gelu_backward)
 *   Attention.forward: softmax(q k^T hd^-1/2) v                      (pp_attention_backward)
 *   the pos_embed add of _pos_embed                                  (pp_rows_period_sum)
 * The Linear layers' data gradients run on pp_gemm with transposed weights, their weight / bias gradients on
 * pp_wgrad_gemm.  No allocation, no host sync; every reduction in a fixed order (no float atomics).
 *
 * pp_layernorm_backward: x [rows, C] f32 the LayerNorm's input (the statistics are recomputed as pp_layernorm takes
 *   them), gamma [C] f32, dy [rows, C] f32 (row pitch ldy) the gradient of its output ->
 *   dres [rows, C] f32 (+)= rstd (gamma dy - mean(gamma dy) - xhat mean(gamma dy xhat)) (accumulate = 1 adds, 0
 *   overwrites), dres_c [rows, C] in dtype = the new dres; dgamma = sum dy xhat, dbeta = sum dy [C] f32 (either may be
 *   NULL; fixed-order float64 partials).  ws: pp_layernorm_backward_workspace_bytes(rows, C) bytes, 8-byte aligned.
 * pp_gelu_forward: out[i] = x Phi(x) in dtype (x [n] f32);  pp_gelu_backward: dx[i] = g (Phi(x) + x phi(x)) in dtype
 *   (x, g [n] f32).  16-byte aligned buffers.
 * pp_attention_backward: qkv [B*N, 3*heads*hd] in dtype laid out as pp_attention reads it, out / dout [B*N, heads*hd]
 *   (the forward's output and its gradient) -> dqkv [B*N, 3*heads*hd] (dq, dk, dv in qkv's layout).  head_dim 32 / 64,
 *   any N; PP_F32 or PP_BF16 storage, f32 arithmetic.  ws: pp_attention_backward_workspace_bytes(B, N, heads) bytes
 *   (the rows' log-sum-exp and rowsum(dout o out)).
 * pp_rows_period_sum: out[n, c] = sum_b x[(b N + n) C + c] (b ascending), x [B*N, C] f32, out [N, C] f32.
 * ---------------------------------------------------------------------- */
long long pp_layernorm_backward_workspace_bytes(int rows, int C);
int pp_layernorm_backward(const float *x, const float *gamma, float eps, int rows, int C, const float *dy,
                          long long ldy, float *dres, int accumulate, void *dres_c, int dtype, float *dgamma,
                          float *dbeta, void *ws, void *stream);
int pp_gelu_forward(const float *x, long long n, void *out, int dtype, void *stream);
int pp_gelu_backward(const float *x, const float *g, long long n, void *dx, int dtype, void *stream);
long long pp_attention_backward_workspace_bytes(int B, int N, int heads);
int pp_attention_backward(const void *qkv, const void *out, const void *dout, void *dqkv, int B, int N, int heads,
                          int hd, int dtype, void *ws, void *stream);
int pp_rows_period_sum(const float *x, int B, int N, int C, float *out, void *stream);

/* ------------------------------------------------------------------------
 * Stochastic depth in the training backbone (ScratchViTBackbone(drop_path_rate=...), timm's DropPath with
 * scale_by_keep): r_out[b] = r_in[b] + keep[b] / (1 - p) branch(r_in)[b] per crop b.  The branch (LayerNorm, GEMMs,
 * attention, GELU: the kernels above, unchanged) runs on the kept crops only, on compact buffers [kept*N, C]; these
 * three kernels move whole crops (N rows of C) between the residual stream [B*N, C] and the compact buffers.
 * idx [kept] int32: the kept crops, each at most once (ascending as vit_train.py builds it); slot [B] int32: a crop's
 * position in idx, or -1 for a dropped crop.  0 < kept <= B <= 65535.  128-bit accesses where C % 4 == 0 and every
 * buffer is 16-byte aligned, scalar accesses otherwise.  One writer per output element, no atomics: repeated calls
 * give the same bits.  A table entry out of range is skipped (idx) or taken as dropped (slot).
 *
 * pp_crop_rows_gather: dst[(j N + n) C + c] = scale src[(idx[j] N + n) C + c], j < kept; src [B*N, C] f32, dst
 *   [kept*N, C] in dtype (PP_F32 / PP_BF16), one f32 multiply, then rounded once to dtype.  scale == 1 and PP_F32: an
 *   exact copy.
 * pp_droppath_add: out[b] = fmaf(scale, branch[slot[b]], r[b]) where slot[b] >= 0 (a single fma: ONE rounding of the
 *   exact r + scale branch), else out[b] = r[b] with its bits; r, out [B*N, C] f32, branch [kept*N, C] f32.  out must
 *   not alias r or branch.
 * pp_crop_rows_scatter_add: dres[idx[j]] += dx[j] in place (one f32 add), and the same rows of dres_c = the new dres
 *   rounded to dtype; dx [kept*N, C] f32, dres [B*N, C] f32, dres_c [B*N, C] in dtype.  Rows of crops that are not in
 *   idx are not touched in either buffer.
 * ---------------------------------------------------------------------- */
int pp_crop_rows_gather(const float *src, const int *idx, int B, int kept, int N, int C, float scale, void *dst,
                        int dtype, void *stream);
int pp_droppath_add(const float *r, const float *branch, const int *slot, int B, int kept, int N, int C, float scale,
                    float *out, void *stream);
int pp_crop_rows_scatter_add(const float *dx, const int *idx, int B, int kept, int N, int C, float *dres, void *dres_c,
                             int dtype, void *stream);

/* ------------------------------------------------------------------------
 * FusedAdamW (probpose_pytorch_amd/optim.py): train.py:113-115's clip_grad_norm_ + AdamW.step() over all parameter
 * tensors in at most three launches, no host sync, no float atomics.  All tensors contiguous float32.
 *
 * The device table (8-byte aligned) that the kernels read:
 *   header  32 B  {uint32 magic, int32 n_tensors, n_groups, n_chunks, chunk_elems, pad, int32 *arrive}
 *   groups  n_groups x 40 B  {lr, beta1, beta2, eps, weight_decay} f64
 *   tensors n_tensors x 56 B {float *p, *g, *exp_avg, *exp_avg_sq, *step; int64 count; int32 group, pad}
 *   chunks  n_chunks x 8 B   {int32 tensor, chunk within the tensor}: one workgroup per chunk of at most
 *                            PP_OPTIM_CHUNK elements of one tensor
 * `step` points at the tensor's own step count t (one float32 on the device, torch's state["step"]); `arrive` at
 * n_tensors zeroed int32 on the device (left zero by every launch).
 * pp_optim_table_bytes: the table's size for these element counts, -1 (and pp_last_error) on bad arguments.
 * pp_optim_table_build: checks every argument on the host and packs the table into HOST memory `table`; hyper is
 *   [n_groups][5] f64 in the groups' order.  with_chunks = 0 leaves the chunk map unwritten (it depends on the counts
 *   only).  *prefix_bytes = the bytes ahead of the chunk map, what changes from step to step.
 * pp_grad_sqnorm_partials: partials[chunk] = sum of g^2 over the chunk in float64, fixed order.
 * pp_grad_norm_finish: one workgroup adds the partials in a fixed order -> record (16 B on the device):
 *   {f32 total_norm, f32 clip_coef = clip ? min(1, max_norm / (total_norm + 1e-6)) : 1, int32 finite,
 *    int32 skipped_steps (+1 when count_skips and the norm is inf or NaN)}.
 * pp_adamw_step: per element, with g' = g clip_coef (1 when record is NULL) and t = *step + 1:
 *     p = p (1 - lr wd);  m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g' g'
 *     p = p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps);   *step = t
 *   skip_nonfinite (needs record): a step whose record says "not finite" changes nothing.
 * ---------------------------------------------------------------------- */
#define PP_OPTIM_CHUNK 8192
long long pp_optim_table_bytes(int n_tensors, const long long *counts, int n_groups);
int pp_optim_table_build(int n_tensors, const void *const *p, const void *const *g, const void *const *m,
                         const void *const *v, const void *const *step, const long long *counts, const int *group,
                         int n_groups, const double *hyper, void *arrive, void *table, int with_chunks, int *n_chunks,
                         long long *prefix_bytes);
int pp_grad_sqnorm_partials(const void *table, int n_chunks, double *partials, void *stream);
int pp_grad_norm_finish(const double *partials, int n_chunks, int clip, double max_norm, int count_skips, void *record,
                        void *stream);
int pp_adamw_step(const void *table, int n_chunks, const void *record, int skip_nonfinite, void *stream);

/* ------------------------------------------------------------------------
 * ModelEma (probpose_pytorch_amd/ema.py): the exponential moving average of all state tensors of a model in one
 * launch, no host sync, no atomics.  All tensors contiguous and 4-byte aligned.
 *
 * The device table (8-byte aligned) that the kernel reads:
 *   header  32 B  {uint32 magic, int32 n_tensors, n_chunks, chunk_elems, 16 B zero}
 *   tensors n_tensors x 32 B {const void *src, void *dst; int64 count; int32 kind, pad}
 *   chunks  n_chunks x 8 B   {int32 tensor, chunk within the tensor}: one workgroup per chunk of at most
 *                            PP_OPTIM_CHUNK elements of one tensor
 * kind PP_EMA_LERP_F32:   dst = (float)((double)dst + weight * ((double)src - (double)dst)), count in float32
 *                         elements, evaluated in float64 and rounded once at the store
 * kind PP_EMA_COPY_WORDS: dst = src as 4-byte words, count in words (non-float state, e.g. BatchNorm's int64
 *                         num_batches_tracked: 2 words)
 * The table is static: it depends on the addresses, counts and kinds only, so it is uploaded once.
 * pp_ema_table_bytes: the table's size for these counts, -1 (and pp_last_error) on bad arguments.
 * pp_ema_table_build: checks every argument on the host (null and misaligned pointers, counts <= 0, kinds, a dst
 *   range that overlaps any src range or another dst range) and packs the table into HOST memory `table`.
 * pp_ema_update: one launch over n_chunks workgroups; weight = 1 - decay of this update, in [0, 1].  A table whose
 *   first word is not the magic word is left alone by every workgroup.
 * ---------------------------------------------------------------------- */
#define PP_EMA_LERP_F32 0
#define PP_EMA_COPY_WORDS 1
long long pp_ema_table_bytes(int n_tensors, const long long *counts);
int pp_ema_table_build(int n_tensors, const void *const *src, const void *const *dst, const long long *counts,
                       const int *kinds, void *table, int *n_chunks);
int pp_ema_update(const void *table, int n_chunks, double weight, void *stream);

/* ------------------------------------------------------------------------
 * CocoKeypointEval (probpose_pytorch_amd/cocoeval.py): COCO keypoint AP / AR on the device.  Everything is float64;
 * no host sync, no float atomics, the same bits on every call.
 *
 * A ragged batch of n_img images is one int64 array of 3 (n_img + 1) CSR offsets [det_off | gt_off | oks_off]:
 * image i owns detections det_off[i] .. det_off[i+1] (already in descending score order, cut to max_dets), ground
 * truths gt_off[i] .. gt_off[i+1], and its row-major D_i x G_i OKS matrix starts at oks_off[i].  `host_offs` is the
 * copy in HOST memory that the entry points check before any launch (start at 0, monotone, oks_off the running sum of
 * D_i G_i, ending at Dtot / Gtot / oks_total); `offs` is the same array in device memory.  D_i = 0 and G_i = 0 are
 * legal, so is n_img = 0 (nothing is launched).
 *
 * pp_cocoeval_oks: oks[oks_off[i] + d G_i + g] = OKS(detection d, ground truth g) of every image in one launch.
 *   det_kpts [Dtot, K, 2] (x, y), gt_kpts [Gtot, K, 3] (x, y, v), gt_bbox [Gtot, 4] xywh, gt_area [Gtot],
 *   vars [K] = (2 sigma_k)^2, gt_flags [Gtot] bytes (below).  Over the keypoints with v > 0:
 *   e = (dx^2 + dy^2) / vars / (area + DBL_EPSILON) / 2, OKS = mean(exp(-e)); a ground truth flagged NO_VISIBLE is
 *   scored over all K keypoints by the distance to its box grown by its own size on every side.
 * pp_cocoeval_exoks: the same matrices with Ex-OKS, the presence-aware OKS of ProbPose, in place of OKS; the other two
 *   entries run on its output unchanged.  Adds det_presence [Dtot, K] (the detection's probability that keypoint k is
 *   inside what the model saw), gt_window [Gtot, 4] xyxy (x0, y0, x1, y1: the region the model saw of that ground
 *   truth) and presence_thr in [0, 1] (anything else, NaN included, is refused; so is a null det_presence or
 *   gt_window).  Per keypoint with v > 0, gin = x0 <= xg < x1 and y0 <= yg < y1, pin = det_presence >= presence_thr
 *   (equal counts as present), and the term is
 *     gin and pin          exp(-e), e as in pp_cocoeval_oks, the same operations in the same order
 *     gin and not pin      0 (missed)
 *     not gin and not pin  1 (correctly reported absent)
 *     not gin and pin      exp(-e) with e = b b / vars / (area + DBL_EPSILON) / 2 and
 *                          b = max(0, min(xd - x0, x1 - xd, yd - y0, y1 - yd)): a false positive is charged by how far
 *                          inside the window it was placed, one on or outside the border costs nothing
 *   ExOKS = (sum of the terms, added in keypoint order) / (number of keypoints with v > 0).  A ground truth flagged
 *   NO_VISIBLE takes the grown-box branch of pp_cocoeval_oks.  With every annotated keypoint inside its window and
 *   every presence >= presence_thr the result is pp_cocoeval_oks's bit for bit.
 * pp_cocoeval_match: the greedy matching of all (image, area range, threshold) triples in one launch.
 *   area_ranges [A, 2] (lo, hi), thr [T], det_area [Dtot].  A ground truth is ignored in a range when it is CROWD or
 *   NO_VISIBLE or its area is outside [lo, hi].  Per detection, in order: the best still-free ground truth with
 *   OKS >= min(thr, 1 - 1e-10), non-ignored ones before ignored ones, the later one on equal OKS; crowd ground truths
 *   stay free.  dt_matched / dt_ignore [A, T, Dtot] bytes (an unmatched detection is ignored when its own area is
 *   outside the range), npig [A] int32 = non-ignored ground truths, gt_matched [A, T, Gtot] bytes (workspace; on
 *   return: which ground truths were taken).
 * pp_cocoeval_accumulate: per (area range, threshold), over the detections in `order` ([Dtot] int64, the stable
 *   descending score order over all images): tp / fp over the non-ignored ones, precision tp / (tp + fp + eps) made
 *   non-increasing from the right, sampled at the first position whose recall tp / npig reaches rec_thr[r].
 *   precision [T, R, A], recall [T, A]; -1 where npig[a] = 0.  ws_env [A, T, Dtot] float64 and ws_tp [A, T, Dtot]
 *   int32 are workspace.
 * ---------------------------------------------------------------------- */
#define PP_COCO_GT_CROWD 1
#define PP_COCO_GT_NO_VISIBLE 2
int pp_cocoeval_oks(int n_img, int K, long long Dtot, long long Gtot, long long oks_total, const long long *host_offs,
                    const void *offs, const void *det_kpts, const void *gt_kpts, const void *gt_bbox,
                    const void *gt_area, const void *gt_flags, const void *vars, void *oks, void *stream);
int pp_cocoeval_exoks(int n_img, int K, long long Dtot, long long Gtot, long long oks_total, const long long *host_offs,
                      const void *offs, const void *det_kpts, const void *gt_kpts, const void *gt_bbox,
                      const void *gt_area, const void *gt_flags, const void *vars, const void *det_presence,
                      const void *gt_window, double presence_thr, void *oks, void *stream);
int pp_cocoeval_match(int n_img, int A, int T, long long Dtot, long long Gtot, long long oks_total,
                      const long long *host_offs, const void *offs, const void *oks, const void *gt_flags,
                      const void *gt_area, const void *det_area, const void *area_ranges, const void *thr,
                      void *gt_matched, void *dt_matched, void *dt_ignore, void *npig, void *stream);
int pp_cocoeval_accumulate(long long Dtot, int A, int T, int R, const void *order, const void *dt_matched,
                           const void *dt_ignore, const void *npig, const void *rec_thr, void *ws_env, void *ws_tp,
                           void *precision, void *recall, void *stream);

/* ------------------------------------------------------------------------
 * PoseNMS (probpose_pytorch_amd/posenms.py): instance rescoring and OKS-NMS of decoded poses, the stage between
 * Codec.decode and CocoKeypointEval.  Everything is float64; no host sync, no atomics, plain vector stores, the same
 * bits on every call.
 *
 * pp_posenms_rescore: out[i] = box_scores[i] * mean, one lane per detection.  mean = (sum of the kpt_scores[i, k] >
 *   kpt_thr, added in ascending k) / (their number n); n = 0 gives mean 0.  kpt_scores [M, K], box_scores [M],
 *   out [M].  M = 0 launches nothing.
 *
 * pp_posenms: NMS of every image of a ragged batch in one launch.  `host_off` / `off` are the n_img + 1 int64 CSR
 *   offsets of the detections, in HOST memory (checked before any launch: start at 0, monotone, ending at Dtot, no
 *   image above PP_POSENMS_MAX_DETS) and in device memory (what the kernel reads).  Image i owns detections
 *   off[i] .. off[i+1], ALREADY in descending score order, equal scores in the order they were given.
 *   kpts [Dtot, K, 2] (x, y), vis [Dtot, K] or NULL, area [Dtot], scores [Dtot], vars [K] = (2 sigma_k)^2.
 *   OKS(a, b) = mean over the keypoints that count of exp(-e_k),
 *   e_k = (dx^2 + dy^2) / vars[k] / ((area_a + area_b) / 2 + DBL_EPSILON) / 2; with vis == NULL every keypoint counts,
 *   otherwise those with vis_a[k] > vis_thr and vis_b[k] > vis_thr; none counting gives OKS 0.
 *   PP_POSENMS_HARD: walk the order; a detection not yet suppressed is kept and suppresses every later live one whose
 *     OKS with it is > oks_thr.  out_scores = scores.  max_dets is not used (it must still be positive).
 *   PP_POSENMS_SOFT_GAUSSIAN / PP_POSENMS_SOFT_LINEAR: until nothing is live or max_dets are kept: the live detection
 *     with the largest current score (the earliest on equal scores) is kept with that score, and every other live
 *     detection's score is multiplied by exp(-OKS^2 / oks_thr), or by (1 - OKS) where OKS >= oks_thr.
 *   out_scores [Dtot] (the current scores at the end), keep [Dtot] bytes (1 = kept), counts [n_img] int32 = kept per
 *   image.  n_img = 0 or Dtot = 0 launches nothing.
 * Both refuse on the host, with pp_last_error, before any launch: null pointers, K <= 0, oks_thr outside (0, 1], an
 * unknown mode, max_dets <= 0, bad offsets.
 * ---------------------------------------------------------------------- */
#define PP_POSENMS_HARD 0
#define PP_POSENMS_SOFT_GAUSSIAN 1
#define PP_POSENMS_SOFT_LINEAR 2
#define PP_POSENMS_MAX_DETS 4096
int pp_posenms_rescore(long long M, int K, const void *kpt_scores, const void *box_scores, double kpt_thr, void *out,
                       void *stream);
int pp_posenms(int n_img, int K, long long Dtot, const long long *host_off, const void *off, const void *kpts,
               const void *vis, const void *area, const void *scores, const void *vars, int mode, double oks_thr,
               double vis_thr, int max_dets, void *out_scores, void *keep, void *counts, void *stream);

/* ------------------------------------------------------------------------
 * PoseTracker (probpose_pytorch_amd/tracker.py): greedy OKS association of a frame's poses with the
 * tracks of its stream, and One-Euro smoothing per keypoint coordinate.  Everything is float64; no host sync, no
 * atomics, plain vector stores, the same bits on every call.  One update is the three launches below, in this order.
 *
 * State of one stream: a block of pp_track_state_bytes(max_tracks, K) bytes, 8-byte aligned, T = max_tracks:
 *   id int64 [T] (-1 = free) | t_last f64 [T] | area f64 [T] | kp f64 [T, K, 2] | vis f64 [T, K] | xhat f64 [T, K, 2]
 *   | dxhat f64 [T, K, 2] | next_id int64 | overflow int64 | age int32 [T], padded to 8 bytes | init uint8 [T, K],
 *   padded to 8 bytes.  A fresh block is all zero except id = -1.
 * `blocks` is a device array of n_str int64 block addresses, one per stream of the call; `host_off` / `off` are the
 * n_str + 1 int64 CSR offsets of the detections in HOST memory (checked before any launch: start at 0, monotone,
 * ending at Dtot, no stream above PP_TRACK_MAX_DETS) and in device memory; `det_stream` [Dtot] int64 is every
 * detection's stream index.  Stream i owns detections off[i] .. off[i+1], ALREADY in descending score order, equal
 * scores in the order they were given.  kpts [Dtot, K, 2], vis [Dtot, K] or NULL, area [Dtot], vars [K] = (2 sigma)^2.
 *
 * pp_track_oks: oks [Dtot, max_tracks] = pp_posenms's pair OKS of detection d (the pivot) and slot j's stored raw
 *   keypoints, area and visibilities; a free slot gives 0.  One lane per pair.
 * pp_track_assign: one wave per stream.  In visiting order each detection takes the slot, live when the call began and
 *   not yet taken, with the largest OKS (the lowest slot on equal OKS) if that OKS is > match_thr.  Then every live
 *   slot not taken gets age += 1 and is freed when age > max_age.  Then each unmatched detection, in visiting order,
 *   takes the lowest free slot with id = next_id++, or none (overflow += 1).  Per detection: ids [Dtot] int64 (-1 =
 *   none), match_oks [Dtot] f64 (0 unless matched), born [Dtot] uint8, slot_of [Dtot] int32 (-1 = none), te [Dtot] f64
 *   = t - t_last of a matched slot (0 otherwise).  A taken or born slot gets age = 0, t_last = t, area = the
 *   detection's.  t - t_prev must be > 0 (t_prev = the previous update's t, -inf for the first).  A stream without
 *   detections still ages; n_str = 0 launches nothing.
 * pp_track_filter: one lane per (detection, keypoint) with a slot: out [Dtot, K, 2] and the slot's filter state.
 *   smooth = 0: out = raw.  Otherwise a keypoint with vis given and vis <= vis_thr: out = raw, init = 0; a born slot or
 *   init == 0: xhat = x, dxhat = 0, init = 1, out = x; else per coordinate dx = (x - xhat) / te, a_d = alpha(te,
 *   d_cutoff), dxhat = a_d dx + (1 - a_d) dxhat, a = alpha(te, min_cutoff + beta |dxhat|), xhat = a x + (1 - a) xhat =
 *   out, with alpha(te, fc) = r / (r + 1), r = ((2 pi) fc) te, unfused.  The slot's kp and vis rows take the raw values
 *   (vis 1 without visibilities).  A detection without a slot: out = raw.
 * All refuse on the host, with pp_last_error, before any launch: null pointers, K <= 0, max_tracks outside
 * 1..PP_TRACK_MAX_TRACKS, match_thr outside [0, 1), max_age < 0, te <= 0, bad offsets, bad filter constants.
 * ---------------------------------------------------------------------- */
#define PP_TRACK_MAX_TRACKS 4096
#define PP_TRACK_MAX_DETS 4096
long long pp_track_state_bytes(int max_tracks, int K);
int pp_track_oks(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off, const void *det_stream,
                 const void *blocks, const void *kpts, const void *vis, const void *area, const void *vars,
                 double vis_thr, void *oks, void *stream);
int pp_track_assign(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off, const void *off,
                    const void *blocks, const void *oks, const void *area, double match_thr, int max_age, double t,
                    double t_prev, void *ids, void *match_oks, void *born, void *slot_of, void *te, void *stream);
int pp_track_filter(int K, int max_tracks, long long Dtot, const void *det_stream, const void *blocks,
                    const void *kpts, const void *vis, double vis_thr, const void *slot_of, const void *born,
                    const void *te, int smooth, double min_cutoff, double beta, double d_cutoff, void *out,
                    void *stream);

/* ------------------------------------------------------------------------
 * Optimal track association (PoseTracker(assign="optimal")): pp_track_assign with its association
 * replaced by the matching of largest total weight; the launch shape, every other phase, the outputs and the state
 * layout are pp_track_assign's.  total: int64 [n_str] or NULL, per stream the sum of q over its matched pairs.
 *
 * Per stream: rows are its D detections in visiting order, columns 0 .. T-1 its slots (T = max_tracks), m = max(D, T);
 * columns T .. m-1 are virtual ("unmatched").  Weights q[i][j], int64:
 *   q = 0 if j >= T, or slot j is not live when the call begins, or !(oks[i][j] > match_thr) (a NaN is inadmissible);
 *   otherwise q = 1 + floor(min(oks[i][j] - match_thr, 1.0) * 2^40), each step one IEEE float64 operation.
 * Costs a = -q.  Shortest augmenting paths with potentials, all int64, INF = 2^62:
 *   1. u[i] = 0, v[j] = 0, no column holds a row.
 *   2. for rows i = 0 .. D-1 in order: minv[j] = INF, used[j] = false, way[j] = root for every j; root is an extra
 *      start column that holds row i; cur = root.  Repeat: mark cur used (the root counts); i0 = the row cur holds; for
 *      every unused column j: c = a[i0][j] - u[i0] - v[j]; if c < minv[j] then minv[j] = c, way[j] = cur.  delta = the
 *      minimum of minv over the unused columns, j1 = the LOWEST column that attains it.  For every used column (root
 *      included): u[row it holds] += delta, v[col] -= delta; for every unused column: minv[j] -= delta.  cur = j1; stop
 *      when cur holds no row.  Then walk back: while cur != root: prev = way[cur], cur takes the row prev held,
 *      cur = prev.  Every step marks one more column used: a row ends after at most m + 1 steps on any input.
 *   3. detection i is matched to slot j iff column j holds row i, j < T and q[i][j] > 0.
 * This maximises the sum of q over the matchings of admissible pairs; every admissible pair has q >= 1.  A matched pair
 * is written as pp_track_assign writes one (match_oks = oks[i][j]); ageing and births follow unchanged.
 * Refused on the host like pp_track_assign, and also, naming the limit: max_tracks > PP_TRACK_OPT_MAX, a stream with
 * more than PP_TRACK_OPT_MAX detections.
 * ---------------------------------------------------------------------- */
#define PP_TRACK_OPT_MAX 256
int pp_track_assign_optimal(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off,
                            const void *off, const void *blocks, const void *oks, const void *area, double match_thr,
                            int max_age, double t, double t_prev, void *ids, void *match_oks, void *born,
                            void *slot_of, void *te, void *total, void *stream);

/* ------------------------------------------------------------------------
 * Motion prediction and the low-score second pass (PoseTracker(predict=..., high_thr=..., birth_thr=...), DESIGN
 * §4.7i).  Each entry stands in for one of the three launches of an update; the state block does not change.
 *
 * pp_track_oks_predicted: pp_track_oks with the slot's pose moved to time t by the speed of its One-Euro filter.  For
 *   a live slot j and keypoint k, e = j K + k, float64, every step one IEEE basic operation, unfused:
 *     dt = t - t_last[j]; if dt > max_dt then dt = max_dt           (pp_track_boxes' step 3; max_dt = +inf is allowed)
 *     p_c = init[e] ? xhat[2e+c] + dxhat[2e+c] * dt : kp[2e+c]      (the product, then the sum, per coordinate c)
 *   and the pair OKS takes p in place of the slot's stored raw keypoints; the slot's stored visibilities and area are
 *   used as in pp_track_oks, a free slot gives 0.  One lane per pair, the same grid.
 *   Refused on the host like pp_track_oks, and also: t not finite, max_dt negative or NaN.
 *
 * pp_track_assign_staged: pp_track_assign in two stages by detection score, with births gated by score.  score f64
 *   [Dtot] in visiting order (descending within a stream, so the detections with score >= high_thr are a prefix of
 *   their stream: n_high of them); dropped uint8 [Dtot]; the other arguments and outputs are pp_track_assign's.
 *   Per stream, with "live" and "age" as they are when the call begins:
 *     stage 1: rows are detections 0 .. n_high-1, columns the live slots, the threshold is match_thr;
 *     stage 2: rows are detections n_high .. D-1, columns the live slots that stage 1 did not take and whose
 *       age <= low_max_age, the threshold is low_match_thr.
 *   Within a stage, optimal = 0: each row in turn takes the column not yet taken with the largest OKS (the lowest slot
 *   on equal OKS) if that OKS is > the threshold (pp_track_assign's rule).  optimal = 1: the rows take the columns by
 *   pp_track_assign_optimal's steps 1 - 3 with m = max(rows of the stage, T), q = 0 for a slot that is not a column of
 *   the stage and the stage's threshold in place of match_thr; the stages are solved one after the other.
 *   Then ageing as in pp_track_assign (every live slot taken in neither stage).  Then each unmatched detection with
 *   score >= birth_thr, in visiting order, takes the lowest free slot with id = next_id++, or none (overflow += 1).
 *   Every other unmatched detection is dropped: ids = -1, match_oks = 0, born = 0, slot_of = -1, te = 0, dropped = 1,
 *   and overflow does not count it; dropped = 0 for every other detection.  high_thr = birth_thr = -inf is
 *   pp_track_assign (optimal = 0) or pp_track_assign_optimal (optimal = 1) bit for bit.
 *   Refused on the host like pp_track_assign, and also: high_thr or birth_thr NaN, low_match_thr outside [0, 1),
 *   low_max_age < 0, optimal neither 0 nor 1, and with optimal = 1 max_tracks or a stream's detections above
 *   PP_TRACK_OPT_MAX.
 * ---------------------------------------------------------------------- */
int pp_track_oks_predicted(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off,
                           const void *det_stream, const void *blocks, const void *kpts, const void *vis,
                           const void *area, const void *vars, double vis_thr, double t, double max_dt, void *oks,
                           void *stream);
int pp_track_assign_staged(int n_str, int K, int max_tracks, long long Dtot, const long long *host_off,
                           const void *off, const void *blocks, const void *oks, const void *area, const void *score,
                           double match_thr, double high_thr, double low_match_thr, int low_max_age, double birth_thr,
                           int optimal, int max_age, double t, double t_prev, void *ids, void *match_oks, void *born,
                           void *slot_of, void *te, void *dropped, void *stream);

/* ------------------------------------------------------------------------
 * Track-driven person boxes (PoseTracker.propose_boxes): the tracker's state read back out as the box
 * each track's person is expected in at time t, one launch, one lane per (stream, slot) with a serial loop over the
 * slot's K keypoints.  It writes no state; no atomics, no LDS, no barrier, plain vector stores: the same bits on every
 * call.  `blocks` [n_str] int64 as above.  frame_wh: device f64 [n_str, 2] (w, h) or NULL; a row (0, 0) does not clamp
 * that stream.  host_sup_off / sup_off: n_str + 1 int64 CSR offsets into sup_boxes, in HOST memory (checked) and in
 * device memory, both or neither; sup_boxes: device f64 [n_sup, 4] xywh, the boxes a proposal must not duplicate.
 * Outputs, [n_str * max_tracks], row s * max_tracks + j: boxes f64 x 4 (xywh), ids int64 (the slot's id, -1 when
 * free), scores f64, status uint8 (PP_TRACK_BOX_*).
 *
 * Rule for slot j of stream s; float64, every step one IEEE basic operation, in this order, unfused:
 *    1. id[j] < 0 -> FREE.
 *    2. age[j] > max_age -> OLD.
 *    3. dt = t - t_last[j]; if dt > max_dt then dt = max_dt (max_dt = +inf is allowed).
 *    4. for k ascending, a keypoint counts if !use_vis or vis[j, k] > vis_thr.  Its point is xhat + dxhat * dt (the
 *       product, then the sum, per coordinate) when smooth && init[j, k] && extrapolate, xhat when smooth && init[j, k]
 *       without extrapolate, else the raw kp.  The first counted point starts x0, x1, y0, y1; later points update them
 *       by < / > comparisons.  sum += vis[j, k] (from 0.0); n += 1.
 *    5. n < min_keypoints -> FEW.
 *    6. cx = (x0 + x1) * 0.5, cy likewise; w = (x1 - x0) * pad, h = (y1 - y0) * pad; if !(w >= min_side) then
 *       w = min_side, the same for h.
 *    7. with aspect > 0 (w / h): if w < h * aspect then w = h * aspect, else h = w / aspect.
 *    8. bx = cx - w * 0.5, by = cy - h * 0.5, ex = bx + w, ey = by + h.
 *    9. with a frame (fw > 0): bx < 0 -> 0, by < 0 -> 0, ex > fw -> fw, ey > fh -> fh.
 *   10. always: w = ex - bx, h = ey - by.
 *   11. any of bx, by, w, h not finite, or !(w >= min_side && h >= min_side) -> OUTSIDE.
 *   12. for each given box (gx, gy, gw, gh) of stream s, in the order given, with gw > 0 && gh > 0:
 *       ix = min(ex, gx + gw) - max(bx, gx), iy likewise (min / max by one < / > comparison, the first operand when it
 *       holds); inter = (ix > 0 && iy > 0) ? ix * iy : 0; uni = (w * h + gw * gh) - inter; iou = uni > 0 ? inter /
 *       uni : 0; any iou > iou_thr -> SUPPRESSED.
 *   13. else PROPOSED.  PROPOSED and SUPPRESSED rows carry the box (bx, by, w, h) and score = sum / n; all other rows
 *       carry zeros.
 * Refused on the host, with pp_last_error naming the argument, before any launch: n_str < 0, K <= 0, max_tracks
 * outside 1..PP_TRACK_MAX_TRACKS, t not finite, vis_thr NaN with use_vis, max_dt negative or NaN, max_age < 0,
 * min_keypoints < 1, pad or min_side not finite or <= 0, aspect negative or not finite, iou_thr outside [0, 1],
 * sup_off not ascending from 0 or given on one side only, boxes expected but sup_boxes NULL, and, when n_str > 0, NULL
 * blocks or outputs.  n_str = 0 launches nothing.
 * ---------------------------------------------------------------------- */
#define PP_TRACK_BOX_FREE 0
#define PP_TRACK_BOX_PROPOSED 1
#define PP_TRACK_BOX_OLD 2
#define PP_TRACK_BOX_FEW 3
#define PP_TRACK_BOX_OUTSIDE 4
#define PP_TRACK_BOX_SUPPRESSED 5
int pp_track_boxes(int n_str, int K, int max_tracks, const void *blocks, double t, int use_vis, double vis_thr,
                   int smooth, int extrapolate, double max_dt, int max_age, int min_keypoints, double pad,
                   double min_side, double aspect, const void *frame_wh, const long long *host_sup_off,
                   const void *sup_off, const void *sup_boxes, double iou_thr, void *boxes, void *ids, void *scores,
                   void *status, void *stream);

/* ------------------------------------------------------------------------
 * PoseTrackEval (probpose_pytorch_amd/trackeval.py): CLEAR-MOT and identity (IDF1) metrics of tracked
 * poses against annotated ones.  The frames of all sequences are the "images" of pp_cocoeval_oks, which is launched
 * first and unchanged; the three entries below read its matrices.  No host sync, no float atomics, no LDS; the same
 * result on every call.
 *
 * Tables, each given in HOST memory (checked before any launch) and in device memory (what the kernels read):
 *   host_offs / offs  [3, n_frames + 1] int64: pp_cocoeval_oks's own table with the predictions as its detections:
 *     pred_off | gt_off | oks_off.  Frame f's matrix is D_f x G_f row-major: s[g][d] = oks[oks_off[f] + d * G_f + g].
 *   host_seq / seq    [4, n_seq + 1] int64: frame_off (sequence q owns frames frame_off[q] .. frame_off[q+1], in time
 *     order) | gid_off (running sum of NG_q, its ground-truth identities) | pid_off (running sum of NP_q, its predicted
 *     identities) | c_off (running sum of NG_q * NP_q).
 *   host_thr / thr    [n_thr] float64, each in (0, 1].
 * gt_idx [Gtot] and pred_idx [Dtot], int32, device: every instance's identity as a dense index within its sequence,
 * 0 <= gt_idx < NG_q, 0 <= pred_idx < NP_q, distinct within one frame (an index out of range is passed over).
 *
 * The rule.  s[g][d] is pp_cocoeval_oks of the frame, exactly.
 * CLEAR, per sequence and threshold thr, frames in order.  State per ground-truth identity: last = the predicted
 * identity it was matched to most recently, or none; prev = the one it was matched to in the frame immediately before
 * this one, none if it was absent or unmatched there.  A frame with G ground truths (rows, in the order given) and D
 * predictions (columns) has the int64 weights
 *   q[i][j] = 0 unless s[i][j] >= thr (a NaN is inadmissible); otherwise
 *   q[i][j] = 1 + floor(min(s[i][j] - thr, 1.0) * 2^32) + (2^42 if prev[gt i] == pred j else 0),
 * each step one IEEE float64 operation.  256 * (2^32 + 1) < 2^42: an admissible continued pair outweighs any set of
 * new pairs; every total stays below 2^53.  The assignment is that of pp_track_assign_optimal's steps 1 - 3 on q
 * (rows in order, int64 potentials, the lowest column on equal minv, m = max(G, D) with virtual columns, a pair
 * matched iff its column is real and q > 0).  Then TP += matches, FN += G - matches, FP += D - matches; for each
 * matched (g, p): IDSW += 1 if last[g] exists and is not p; s[g][p] is added to a float64 sum (MOTP = sum / TP);
 * last[g] = prev[g] = p for the matched, prev = none for every other identity.  Per identity, matched = the number of
 * frames it is matched in and runs = the number of maximal runs of consecutive frames OF THE SEQUENCE in which it is
 * matched; with present = the number of frames it appears in: MT iff 5 matched > 4 present, ML iff 5 matched < present,
 * PT otherwise; Frag += max(0, runs - 1); MOTA = 1 - (FN + FP + IDSW) / (TP + FN).
 * Identity, per sequence and threshold: c[a][b] = the number of frames in which ground-truth identity a and predicted
 * identity b are both present with s >= thr; IDTP = the largest total of c over one-to-one assignments (the same
 * solver; the total is unique); IDFN = ground-truth instances - IDTP, IDFP = predicted instances - IDTP; IDF1 =
 * 2 IDTP / (2 IDTP + IDFP + IDFN), IDP = IDTP / (IDTP + IDFP), IDR = IDTP / (IDTP + IDFN).
 *
 * pp_trackeval_clear: one wave per (sequence, threshold).  Workspace, [n_thr, n_gid] each (n_gid = gid_off[n_seq]),
 *   needing no initialisation: last int32, prev int64.  Outputs: matched, runs int32 [n_thr, n_gid]; rec int64
 *   [n_seq, n_thr, 4] = TP, FN, FP, IDSW; oks_sum float64 [n_seq, n_thr] (per-lane sums added in a fixed order).
 * pp_trackeval_overlap: one lane per (OKS entry, threshold): c [n_thr, c_total] int32 (c_total = c_off[n_seq]; sequence
 *   q's matrix is NG_q x NP_q row-major at c_off[q]) gets += 1 by an integer atomic.  c must be ZERO on entry.
 * pp_trackeval_identity: one wave per (sequence, threshold): idtp int64 [n_seq, n_thr].  A lane owns 4 columns when
 *   both identity counts are at most PP_TRACKEVAL_MAX_FRAME, 16 otherwise.
 * All refuse on the host, with pp_last_error naming the entry, before any launch: null pointers, n_seq < 0, n_thr < 1,
 * a threshold outside (0, 1], tables that do not start at 0, are not monotone or do not end at the totals given, a
 * frame with more than PP_TRACKEVAL_MAX_FRAME ground truths or predictions, a sequence with more than
 * PP_TRACKEVAL_MAX_IDS ground-truth or predicted identities.  n_seq = 0 (overlap: also oks_total = 0) launches nothing.
 * ---------------------------------------------------------------------- */
#define PP_TRACKEVAL_MAX_FRAME 256
#define PP_TRACKEVAL_MAX_IDS 1024
int pp_trackeval_clear(int n_seq, int n_thr, int n_frames, long long Dtot, long long Gtot, long long oks_total,
                       long long n_gid, const long long *host_offs, const long long *host_seq, const double *host_thr,
                       const void *offs, const void *seq, const void *thr, const void *oks, const void *gt_idx,
                       const void *pred_idx, void *last, void *prev, void *matched, void *runs, void *rec,
                       void *oks_sum, void *stream);
int pp_trackeval_overlap(int n_seq, int n_thr, int n_frames, long long Dtot, long long Gtot, long long oks_total,
                         long long c_total, const long long *host_offs, const long long *host_seq,
                         const double *host_thr, const void *offs, const void *seq, const void *thr, const void *oks,
                         const void *gt_idx, const void *pred_idx, void *c, void *stream);
int pp_trackeval_identity(int n_seq, int n_thr, long long c_total, const long long *host_seq, const void *seq,
                          const void *c, void *idtp, void *stream);

/* ------------------------------------------------------------------------
 * HOTA for PoseTrackEval (PoseTrackEval(hota=True)): higher order tracking accuracy (Luiten et al., IJCV
 * 2021) with OKS as the similarity, per sequence and alpha: the counts and sums from which DetA, AssA, LocA and HOTA
 * are finished on the host.  Four entries after pp_cocoeval_oks, on the tables of the entries above; the same
 * principles: no host sync, no float atomics, no LDS, the same result on every call.
 *
 * The rule.  s[g][d] is pp_cocoeval_oks's entry of the frame (in [0, 1] or NaN); an s that is not > 0 (a NaN is not)
 * counts as 0 everywhere below.  a and b are the dense identities of g and d in their sequence; every float step is
 * one IEEE float64 operation.
 *  1. Potential matches, per frame: R_g = sum over d of s[g][d] and C_d = sum over g of s[g][d], each a sequential sum
 *     from 0.0 in ascending index.  For every pair with s > 0: x = s / ((R_g + C_d) - s), w = floor(x * 2^32) as int64
 *     (x <= 1, since both sums hold s), pmc[a][b] += w (an int64 atomic: exact in any order).  ng[a] and np[b] are the
 *     numbers of frames an identity appears in, counted on the host.
 *  2. Alignment: A[a][b] = double(pmc) / double(2^32 (ng[a] + np[b]) - pmc), the denominator formed in int64 (it is
 *     at least 2^32 max(ng, np) where both identities appear; A = 0 if it is not > 0).  Both operands stay below 2^53
 *     while a sequence has at most PP_TRACKEVAL_HOTA_MAX_FRAMES = 2^20 frames.
 *  3. Matching, one per frame for all alphas: q[g][d] = 0 unless s > 0, else 1 + floor((A[a][b] * s) * 2^32); the
 *     assignment is pp_track_assign_optimal's steps 1 - 3 on q exactly as for CLEAR above: rows (ground truths) in
 *     order, int64 potentials, the lowest column on equal minv, m = max(G, D) with virtual columns, a pair matched iff
 *     its column is real and q > 0.  A matching's total / 2^32 differs from its sum of A s by less than 2^-23 (at
 *     most 256 pairs, each q / 2^32 within 2^-32 above A s, and the roundings of A s).
 *  4. Counts, per alpha_i: a matched pair counts iff s >= alpha_i.  TP_i = the counted pairs of all frames, FN_i =
 *     ground-truth instances - TP_i, FP_i = predicted instances - TP_i, loc_i = the sum of s over the counted pairs,
 *     mc_i[a][b] += 1 (an int32 atomic).  TP and loc take no atomics: every frame writes its own record (the lane of
 *     column d % 64 adds its columns in ascending order, then one butterfly over the lanes), launch 4 adds the frames.
 *  5. Association, per sequence and alpha, with m = mc_i[a][b] over the NG x NP entries: assA = sum of m m / (ng[a] +
 *     np[b] - m), assRe = sum of m m / ng[a], assPr = sum of m m / np[b]; m m is formed in int64.
 *  6. On the host, with everything summed over the sequences: DetA = TP / (TP + FN + FP), DetRe = TP / (TP + FN), DetPr
 *     = TP / (TP + FP), AssA = assA / TP, AssRe = assRe / TP, AssPr = assPr / TP, LocA = loc / TP, HOTA = sqrt(DetA
 *     AssA); a ratio whose denominator is 0 is 0, LocA is then 1.
 * A float sum of launch 4 is: lane l adds the elements l, l + 64, .. in ascending order, then one butterfly.
 *
 * gt_present [n_gid] / pred_present [n_pid] int64, device: ng and np of every identity, at gid_off / pid_off of its
 *   sequence (n_pid = pid_off[n_seq]).  host_alpha / alpha [n_alpha] float64, each in (0, 1], n_alpha <=
 *   PP_TRACKEVAL_HOTA_MAX_ALPHAS.
 * pp_trackeval_hota_align (step 1): one wave per frame, four to a workgroup.  pmc int64 [c_total], laid out like one
 *   threshold's c above; it must be ZERO on entry.
 * pp_trackeval_hota_weights (steps 2, 3): one lane per OKS entry: q int64 [oks_total]; frame f's weights are G_f x D_f
 *   row-major (the transpose of its OKS matrix): q[g][d] = q[oks_off[f] + g * D_f + d], so that the solver loads a row
 *   coalesced and no division is left in it.  Every entry is written.
 * pp_trackeval_hota_match (steps 3, 4): one wave per frame, four to a workgroup, four columns per lane.  mc int32
 *   [n_alpha, c_total] must be ZERO on entry.  Outputs: held_row int32 [Dtot] = the row (ground truth of the frame)
 *   every prediction is matched to, or -1; frame_tp int64 and frame_loc float64 [n_frames, n_alpha].
 * pp_trackeval_hota_assoc (steps 4, 5): one wave per (sequence, alpha): tp int64 [n_seq, n_alpha]; sums float64
 *   [n_seq, n_alpha, 4] = loc, assA, assRe, assPr.
 * Workspace: pmc and mc take (8 + 4 n_alpha) NG NP bytes per sequence: about 84 MB for one 1024 x 1024 sequence with 19
 * alphas; q takes 8 bytes per OKS entry.
 * All refuse on the host, with pp_last_error naming the entry, before any launch: what the entries above refuse of the
 * tables they are given, n_alpha outside [1, PP_TRACKEVAL_HOTA_MAX_ALPHAS], an alpha outside (0, 1], predicted identity
 * offsets that do not end at n_pid, a sequence of more than PP_TRACKEVAL_HOTA_MAX_FRAMES frames.  n_seq = 0 launches
 * nothing (align, weights: also oks_total = 0; match: also n_frames = 0).
 * ---------------------------------------------------------------------- */
#define PP_TRACKEVAL_HOTA_MAX_ALPHAS 32
#define PP_TRACKEVAL_HOTA_MAX_FRAMES 1048576
int pp_trackeval_hota_align(int n_seq, int n_frames, long long Dtot, long long Gtot, long long oks_total,
                            long long c_total, const long long *host_offs, const long long *host_seq, const void *offs,
                            const void *seq, const void *oks, const void *gt_idx, const void *pred_idx, void *pmc,
                            void *stream);
int pp_trackeval_hota_weights(int n_seq, int n_frames, long long Dtot, long long Gtot, long long oks_total,
                              long long c_total, long long n_gid, long long n_pid, const long long *host_offs,
                              const long long *host_seq, const void *offs, const void *seq, const void *oks,
                              const void *gt_idx, const void *pred_idx, const void *pmc, const void *gt_present,
                              const void *pred_present, void *q, void *stream);
int pp_trackeval_hota_match(int n_seq, int n_alpha, int n_frames, long long Dtot, long long Gtot, long long oks_total,
                            long long c_total, const long long *host_offs, const long long *host_seq,
                            const double *host_alpha, const void *offs, const void *seq, const void *alpha,
                            const void *oks, const void *q, const void *gt_idx, const void *pred_idx, void *mc,
                            void *held_row, void *frame_tp, void *frame_loc, void *stream);
int pp_trackeval_hota_assoc(int n_seq, int n_alpha, int n_frames, long long c_total, long long n_gid, long long n_pid,
                            const long long *host_seq, const void *seq, const void *mc, const void *gt_present,
                            const void *pred_present, const void *frame_tp, const void *frame_loc, void *tp, void *sums,
                            void *stream);

/* ------------------------------------------------------------------------
 * Visualisation (probpose_pytorch_amd/viz.py): heat overlays and pose drawing on uint8 RGB images, heat
 * maps as RGBA pictures.  No host sync, no atomics, plain vector stores, the same bytes on every call.
 *
 * pp_viz_render: out [B, H, W, 3] uint8 = draw(overlay(image)); one pass, every image byte read and written once.
 *   image: uint8 [B, H, W, 3] (image_f32chw = 0; out == image is allowed: in place) or float32 [B, 3, H, W]
 *     (image_f32chw = 1), converted as trunc(min(max(v * 255f + 0.5f, 0), 255)) in float32, NaN -> 0.
 *   overlay (heat != NULL): heat [B, K, h, w] float32, lut [256, 3] float64 (matplotlib's table of the colormap).  Per
 *     pixel and map the value is the map's own element when (h, w) == (H, W), else bilinear in float64 with
 *     u = px (w - 1) / (W - 1) (0 when W == 1), x0 = min(floor(u), w - 1), x1 = min(x0 + 1, w - 1), fx = u - x0, the
 *     same in y, (a00 (1 - fx) + a01 fx)(1 - fy) + (a10 (1 - fx) + a11 fx) fy, rounded to float32.  Colour: xa = v *
 *     256f in float32; NaN -> (0, 0, 0); xa < 0 -> row 0; xa >= 256 -> row 255; else row trunc(xa).  v < float32(0.01)
 *     adds nothing.  The colours are summed in float64 over k ascending from 0.0, times 255.0, saturated at 255,
 *     truncated, and added to the image byte with saturation at 255.
 *   draw (kpts != NULL): kpts [N, Kp, 2] and probs [N, Kp] float64; inst [N] int32 = the instances ordered by image
 *     (stable), img_off [B + 1] int32 = where each image's instances start in inst; style = Kp int32 colours
 *     (r | g << 8 | b << 16) followed by L limbs (i, j, colour).  A keypoint is drawn unless prob < threshold, when
 *     its coordinates are finite and below 2^31 in magnitude and its centre (trunc(x), trunc(y)) is inside the image:
 *     a disc dx^2 + dy^2 <= radius^2 + radius.  A limb is drawn when both its keypoints are and their centres differ:
 *     the pixels whose squared distance to the segment, times 4, is <= line_width^2, in exact integers.  Per pixel the
 *     last primitive that covers it wins, in the order: all limbs (instances ascending, then limb order), then all
 *     discs (instances ascending, then keypoints ascending).
 *   H, W, h, w, radius and line_width are at most PP_VIZ_MAX_SIDE.
 * pp_viz_colorize: maps [M, h, w] float32 -> out [M, h, w, 4] uint8: trunc(colour * 255.0) of the colour rule above
 *   with alpha 255, (0, 0, 0, 0) for NaN; with `normalize` every map is first divided, in float32, by its own maximum
 *   (NaN when any element is NaN, as numpy's max).  M = 0 launches nothing.
 * Both refuse on the host, with pp_last_error, before any launch: null pointers, sizes out of range, an out that
 * overlaps an input.
 * ---------------------------------------------------------------------- */
#define PP_VIZ_MAX_SIDE 8192
int pp_viz_render(const void *image, int image_f32chw, void *out, int B, int H, int W, const float *heat, int K, int h,
                  int w, const double *lut, const double *kpts, const double *probs, const int *inst,
                  const int *img_off, int N, int Kp, const int *style, int L, double threshold, int radius,
                  int line_width, void *stream);
int pp_viz_colorize(const float *maps, void *out, long long M, int h, int w, const double *lut, int normalize,
                    void *stream);

/* ------------------------------------------------------------------------
 * ValidationMeter (probpose_pytorch_amd/valmeter.py): a whole validation pass accumulated on the device
 * and read back once.  Replaces, per batch of the reference's validation loop (train.py:124-168),
 *   get_binary_accuracy      probpose/loss.py:653-697  (its balanced subsample by its expectation, see below)
 *   get_mae                  probpose/loss.py:699-712
 *   the populations / labels probpose/loss.py:419, :473-500
 *   the host averaging       train.py:146-167
 *
 * The state is `pp_valmeter_state_words(K, J)` int64 words, all zero when empty (a memset resets it).  It holds counts
 * and fixed-point sums only, so it does not depend on the order or the split of the batches.  Q30(z) = rint(z 2^30) in
 * float64 (ties to even), Q20 the same at 2^20; the fine bin of p in [0,1] is min(1023, floor(p * 1024)) in float32.
 * Sections, in this order (h = 0 probability, 1 visibility; label 0 / 1; in code: csrc/pp_valmeter_state.h):
 *   hist     [2][K][2][1024]  samples per (head, keypoint, label, fine bin of p)
 *   conf     [2][K][1024]     sum of Q30(p) per fine bin
 *   above    [2][K][2][J]     samples with (double)p > thresholds[j], strictly
 *   sum_p    [2][K][2]        sum of Q30(p)
 *   sum_p2   [2][K][2]        sum of Q30(p p)
 *   oks_hist [K][1024]        samples of the OKS head per fine bin of the prediction x
 *   oks_sx   [K][1024]        sum of Q30(x) per fine bin
 *   oks_st   [K][1024]        sum of Q30(t) per fine bin, t the achieved OKS
 *   oks_sums [K][5]           sums of Q30 of |x - t|, (x - t)^2, x^2, t^2, x t (formed in float64)
 *   err      [K][4]           n, sums of Q20 of x, t, |x - t| of the error head
 *   pck      [2][K]           hits, valid (the sums of pck_counts)
 *   all      [3]              samples, samples whose dt_prob is in [0,1], the sum of Q30(dt_prob) over those
 *   rejected [5]              samples refused for: a mask value, the probability, visibility, OKS, error head
 *   scalars  [15]             int64: batches, flagged batches, OR of the flag words, unflagged batches that had `res`,
 *                             those that had pck_counts, batches that had map_max; then float64 bit patterns: the sums
 *                             over the unflagged batches of res[1], res[3..8]; of the per-batch PCK average; the
 *                             running maximum of map_max (a NaN wins).
 *
 * pp_valmeter_update adds one batch of B*K samples.  dt_prob, dt_vis, dt_oks, dt_err [B*K] f32 predictions; gt_oks,
 * gt_err [B*K] f32 as pp_probpose_loss_terms writes them; in_image, annotated, visibility [B*K] int32; thresholds [J]
 * f64 on the device, 1 <= J <= 64; optional (NULL to leave out): pck_counts [2][K] int32 of pp_pck_counts, map_max
 * [B*K] f32 = the vals of pp_heatmap_argmax on the predicted maps, res [11] f32 = scalars[3] of pp_oks_heatmap_loss
 * followed by results[8] of pp_probpose_loss_terms.  in_image / annotated other than 0 or 1 reject the sample for every
 * head.  Populations: probability = annotated, label in_image; visibility, OKS and error = annotated and in the image,
 * label visibility != 0.  Within its population a head skips (and counts in `rejected`) a sample whose prediction (or
 * OKS target) is outside [0,1] or NaN, for the error head non-finite, negative or above 2^20.  A batch is flagged when
 * res[9] != 0, res[2] != 0 or one of res[1], res[3..8] is not finite; the flag word is res[9]'s integer, | 256 for
 * res[2] != 0, | 512 for a non-finite value.  A flagged batch's samples are counted like any other's; its losses, MAEs
 * and PCK average are left out of the sums.  Nothing is ever raised per batch.  One launch: a grid of (K, chunks + 1)
 * workgroups with LDS-private counters, 64-bit integer atomics on the state; the scalars are added by one thread.
 *
 * pp_valmeter_report writes report [K + 1][F] f64, F = 2 (10 + J + 3 E) + (5 + 3 E) + 3 + 1 + 18 with E = ece_bins (a
 * divisor of 1024).  Row K pools the keypoints (the integer state summed over k).  Per row:
 *   probability head, then visibility head, each: n_pos, n_neg, best_bal_acc, best_thr, auroc, brier, ece, mce,
 *     mean_conf, base_rate, bal_acc[J], reliability [E][3] = (count, mean confidence, observed frequency).
 *     bal_acc[j] = (TP_j / n_pos + TN_j / n_neg) / 2: the expectation of the reference's balanced subsample at that
 *     threshold.  best_*: the first maximal j (np.argmax); both 0.0 when a class is empty (loss.py:670-673).
 *     auroc = sum_b neg[b] (pos above b + pos[b] / 2) / (n_pos n_neg) over the fine bins.
 *   OKS head: n, mae, rmse, bias (mean x - mean t), pearson, reliability [E][3] = (count, mean predicted, mean achieved)
 *   error head: n, mae, bias
 *   pck: hits / valid, -1 where valid == 0; in the pool row the mean over the keypoints that have any
 *   whole set (pool row only, NaN elsewhere): the means over the unflagged batches of the kpt, probability,
 *     visibility, oks and error losses, acc_kpt, acc_oks, acc_error; max_heatmap; mean_prob; batches; flagged_batches;
 *     flags; rejected[5].
 * Undefined values (an empty population, a zero variance) are NaN.  One launch, one workgroup per (row, head), suffix
 * scan over the fine bins.  Integer intermediates are int64: n_pos n_neg must stay below 2^61.
 *
 * Both refuse on the host before any launch, with pp_last_error: null pointers, K <= 0, B <= 0, J outside 1..64,
 * thresholds not given, an ece_bins that does not divide 1024.  pp_valmeter_state_words returns -1 for bad K or J.
 * ---------------------------------------------------------------------- */
long long pp_valmeter_state_words(int K, int J);
int pp_valmeter_update(const float *dt_prob, const float *dt_vis, const float *dt_oks, const float *dt_err,
                       const float *gt_oks, const float *gt_err, const int *in_image, const int *annotated,
                       const int *visibility, const double *thresholds, int J, const int *pck_counts,
                       const float *map_max, const float *res, int B, int K, long long *state, void *stream);
int pp_valmeter_report(const long long *state, const double *thresholds, int K, int J, int ece_bins, double *report,
                       void *stream);

/* ------------------------------------------------------------------------
 * HeadCalibration (probpose_pytorch_amd/calibration.py): isotonic recalibration of the probability,
 * visibility and OKS heads, fitted from a ValidationMeter state.  h = 0 probability, 1 visibility, 2 OKS; rows
 * r = 0 .. K-1 are the keypoints and r = K the pool (the integer state summed over k, as in pp_valmeter_report).
 * `state` is the meter's own state of pp_valmeter_state_words(K, J) words; hist, oks_hist and oks_st below are its
 * sections as the ValidationMeter paragraph above lays them out, and the fine bin is the one stated there.
 *
 * pp_calib_fit: for each (h, r) the weighted isotonic (non-decreasing) least-squares regression over the 1024 fine
 * bins.  Binary heads: weight n_b = hist[h][k][0][b] + hist[h][k][1][b], numerator P_b = hist[h][k][1][b]; OKS head:
 * n_b = oks_hist[k][b], P_b = oks_st[k][b].  Pool-adjacent-violators over the non-empty bins: two adjacent blocks
 * pool while P_l N_r >= P_r N_l (128-bit products; equal neighbours pool too), so the blocks are the maximal runs of
 * equal fitted value and the result does not depend on the pooling order.  An empty bin carries the block of the
 * nearest non-empty bin to its left, the leading empty bins the first block.  Precondition: fewer than 2^31 samples
 * per (h, r), the pool included.  Outputs, on the device:
 *   blocks [3][K+1][1024][2] int64  (P, N) of the block that covers each bin; (0, 0) in a row with no sample
 *   table  [3][K+1][1024]    f32    binary heads (float)((double)P / (double)N), OKS (float)(((double)P / (double)N)
 *                                   * 2^-30), every conversion to nearest even; 0 in an empty row
 *   row_of [3][K]            int32  k when row (h, k) has at least min_count samples, else K when the pool row has
 *                                   at least one, else -1 (pass through)
 * One launch, one workgroup per (h, r): singleton blocks joined by a merge tree in LDS.
 *
 * pp_calib_apply: aux_in, aux_out [3][B][K] f32 (the `aux` of the decode).  A p in [0,1] becomes
 * table[h][row_of[h][k]][min(1023, floor(p * 1024))]; NaN, values outside [0,1] and entries whose row_of is -1 are
 * copied bit for bit.  aux_in == aux_out is allowed, a partial overlap is refused.  One launch, nothing allocated.
 *
 * pp_calib_score: what the calibration makes of the samples of a meter state with the same K.  Keypoint k goes through
 * table row row_of[h][k]; row K pools the keypoints, each through its own table; keypoints whose row_of is -1 are left
 * out and counted.  The samples of fine bin b take the float32 table value y_b and are regrouped into E = ece_bins
 * bins (a divisor of 1024) by e = min(E - 1, (int)(y_b * E)) in float32.  report [K+1][F] f64, F = 2 (6 + 3 E) + 3 + 3 E:
 *   probability head, then visibility head, each: n, skipped, brier = sum_b (pos_b (1 - y_b)^2 + neg_b y_b^2) / n,
 *     mean_conf = sum_b n_b y_b / n, ece, mce, reliability [E][3] = (count, mean calibrated value, observed frequency)
 *   OKS head: n, skipped, ece, reliability [E][3] = (count, mean calibrated value, mean achieved OKS)
 * Undefined values are NaN.  Sums of y are float64 sums in no fixed order (tests/test_calibration_gpu.py counts the
 * roundings).
 *
 * All three refuse on the host before any launch, with pp_last_error: null pointers, K <= 0, B <= 0, J outside 1..64,
 * min_count < 1, an ece_bins that does not divide 1024.
 * ---------------------------------------------------------------------- */
int pp_calib_fit(const long long *state, int K, int J, long long min_count, long long *blocks, float *table,
                 int *row_of, void *stream);
int pp_calib_apply(const float *aux_in, float *aux_out, int B, int K, const float *table, const int *row_of,
                   void *stream);
int pp_calib_score(const long long *state, int K, int J, const float *table, const int *row_of, int ece_bins,
                   double *report, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PROBPOSE_HIP_H */
