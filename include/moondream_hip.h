/*
 * moondream_hip.h -- C ABI of libmoondream_hip.so, the MI355X (gfx950) compute
 * library behind the Moondream inference seam.
 *
 * The reference isolates its accelerated path behind four bound methods that
 * it rebinds itself in compile() (reference: moondream/torch/moondream.py:168-204):
 *
 *     _vis_enc(x)                           moondream.py:168-169  -> md_vit_encode
 *     _vis_proj(g, r)                       moondream.py:171-172  -> md_vision_project
 *     _prefill(x, attn_mask, pos_ids, lora) moondream.py:174-181  -> md_text_forward
 *     _decode_one_tok(x, mask, pos, lora)   moondream.py:183-192  -> md_text_forward + md_lm_head
 *
 * Conventions
 *   - plain C: device pointers travel as void*, the HIP stream as void*
 *     (a hipStream_t); no torch / C++ types cross this boundary.
 *   - the caller owns every buffer (weights, KV slabs, activations, workspace);
 *     nothing here allocates, frees or synchronises.  All work is enqueued on
 *     the caller's stream, so calls are hipGraph-capturable.
 *   - bf16 tensors are raw 16-bit words, row-major, with an explicit leading
 *     dimension in ELEMENTS.
 *   - every entry point returns an md_status; 0 is success.  There is no CPU
 *     fallback: without a gfx950 device the launches fail and say so.
 */
#ifndef MOONDREAM_HIP_H
#define MOONDREAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MD_ABI_VERSION 5 /* 2: md_text_model.fp8 (trailing, optional); 3: md_vit_model.f8, md_text_model.f8 (trailing, optional), md_gemm_f8 + fp8 producers, md_decode_step_b1_supported; 4: md_linear_fp8.format (int4 group-128 weight stream; a LAYOUT BREAK: md_linear_fp8 grew 40 -> 48 bytes, which moves every md_text_block_fp8 member); 5: tile_policy in md_gemm_args / md_vit_model / md_text_model (per call; replaces the process-wide "strict" tuning key).  Every version is a layout break for some struct: callers MUST compare md_abi_version() with the header they were built against */

typedef int md_status;
enum {
  MD_OK = 0,
  MD_ERR_INVALID_ARG = 1, /* shape / alignment / null-pointer contract violated */
  MD_ERR_LAUNCH = 2,      /* the HIP runtime rejected a launch (no gfx950 device, ...) */
  MD_ERR_WORKSPACE = 3,   /* workspace smaller than md_*_workspace_bytes() */
  MD_ERR_UNSUPPORTED = 4  /* a shape outside what the kernels are built for */
};

int md_abi_version(void);
const char* md_status_string(md_status s);

/* ------------------------------------------------------------------ *
 * Dense layers                                                        *
 * ------------------------------------------------------------------ */

/* y = x W^T + b in the nn.Linear layout (reference: layers.py:34-35).
 * w: bf16 [n_pad][k_pad] row-major, packed once by the host: k_pad = k rounded
 * up to 64 with zero fill; rows n..n_pad-1 (n_pad = n rounded up to 64) zero.
 * b: bf16 [n_pad] (zero-filled tail) or NULL. */
typedef struct {
  const void* w;
  const void* b;
  int32_t n;     /* logical out features */
  int32_t k;     /* logical in features  */
  int32_t n_pad; /* allocated rows       */
  int32_t k_pad; /* allocated row length = leading dimension */
} md_linear;

/* LayerNorm affine parameters, bf16 [dim] (reference: layers.py:118-119). */
typedef struct {
  const void* w;
  const void* b;
} md_layernorm;

enum {
  MD_EPI_BIAS = 0,     /* c = bf16(acc + b)                                       */
  MD_EPI_GELU = 1,     /* c = bf16(gelu_tanh(bf16(acc + b)))    layers.py:129-138 */
  MD_EPI_RESIDUAL = 2  /* c = bf16(r + bf16(acc + b))           vision.py:68,70-71, text.py:158 */
};

/* C[m, n] = epilogue(A[m, :k_pad] . W[n, :k_pad] + b[n]), fp32 accumulate on
 * MFMA, one bf16 rounding of (acc + bias) and one more for the epilogue op --
 * the reference's rounding points.  A must have lda >= k_pad with columns
 * k..k_pad-1 readable and ZERO.  r (MD_EPI_RESIDUAL) is read at row
 * (res_row_mod ? row % res_row_mod : row); it may alias c.  Columns n..n_pad-1
 * of C are written (zeros through the zero weight rows) when ldc >= n_pad,
 * which is what lets a padded activation feed the next layer's k_pad. */
typedef struct {
  const void* a;
  int64_t lda;
  md_linear lin;
  void* c;
  int64_t ldc;
  const void* r;
  int64_t ldr;
  int32_t res_row_mod;
  int32_t m;
  int32_t epilogue;
  int32_t store_pad_cols; /* 1: also store columns [n, n_pad) */
  int32_t gelu_from_col;  /* MD_EPI_GELU only: GELU applies to columns >= this (multiple of 8; 0 = all) */
  /* Scratch for the decode regime (m <= 64), where K is split over several
   * workgroups per output tile: md_gemm_workspace_bytes() bytes, or NULL (then K
   * is not split across workgroups: slower, and a different -- still
   * deterministic -- summation tree).  Its first 8 KiB are arrival tickets:
   * they must be ZERO before the first launch that uses the buffer; every launch
   * leaves them zero, so launches that follow each other on one stream can share
   * the buffer. */
  void* splitk_ws;
  size_t splitk_ws_bytes;
  int32_t tile_policy; /* MD_TILE_BY_SHAPE / MD_TILE_PINNED (below); ABI 5 */
} md_gemm_args;

/* Tile choice of a launch with more than 64 rows -- a PER-CALL property (ABI 5; up to ABI 4 a process-wide tuning key):
 *   MD_TILE_BY_SHAPE  the config that is fastest for (m, n, k): small launches (one image: 730 / 1458 rows) take the
 *                     64x64 / 128x128 / 256x128 configs (32x32x16 MFMAs), large ones the four-wave 256x256 kernel
 *                     (16x16x32 MFMAs).  The two families sum K in different associations: equal to fp32 rounding of the
 *                     accumulator, not bitwise -- so a row's bits can depend on how many rows travel with it.
 *   MD_TILE_PINNED    the tile config is a function of the layer (n, k) alone, never of m: every launch of more than 64
 *                     rows takes the 256x256 kernel, so a sequence gets the same bits alone and in any batch.  That
 *                     kernel addresses a launch with 32-bit byte offsets (m * lda * 2 < 4 GiB, (m + 256) * ldc * 2 <
 *                     0xfffff000: ~150 000 rows of the 2B fused qkv|fc1 layer); a larger launch is cut into row blocks
 *                     of the same kernel (same bits), and one that cannot be cut -- a broadcast residual
 *                     (res_row_mod != 0), the RoPE epilogue -- returns MD_ERR_UNSUPPORTED instead of changing family.
 *   MD_TILE_DECODE_TALL  (round 6; set by md_decode_step / md_text_forward themselves for a decode step of 65 .. 128 sequences, accepted
 *                     from a caller of md_gemm_bf16 too) a launch of 65 .. 128 rows is a WEIGHT STREAM like the <= 64-row regime: one
 *                     128 x 64 tile per weight panel (four compute waves + two DMA waves), the same K order per output element as
 *                     the 64-row configs -- a sequence gets the same bits in a decode step of 128 as in one of 64; layers of
 *                     >= 16384 output columns (lm_head) take the by-shape config (same MFMA family, same K order).  Other row
 *                     counts: as MD_TILE_BY_SHAPE.
 *   MD_TILE_PINNED_ANY_ROWS  MD_TILE_PINNED for launches of <= 64 rows as well: the 256x256 kernel with the rows past m dropped
 *                     by its range checks, not the split-K weight-streaming configs.  For recomputing a few rows of a pinned
 *                     launch with the bits that launch gives them (md_text_forward_trim's last block); slower than the
 *                     decode regime for anything else.
 * md_vit_model.tile_policy / md_text_model.tile_policy apply it to every GEMM of md_vit_encode / md_vision_project* /
 * md_text_forward* / md_lm_head / md_decode_step made with that struct.  Launches of <= 64 rows (the decode regime) are
 * not affected: they always take the split-K weight-streaming configs, except under MD_TILE_PINNED_ANY_ROWS. */
enum { MD_TILE_BY_SHAPE = 0, MD_TILE_PINNED = 1, MD_TILE_DECODE_TALL = 2, MD_TILE_PINNED_ANY_ROWS = 3 };

md_status md_gemm_bf16(const md_gemm_args* args, void* stream);
size_t md_gemm_workspace_bytes(const md_linear* lin, int32_t m, int32_t store_pad_cols);

/* Decode regime (m <= 64), launch-boundary split-K: instead of combining the K slices inside
 * the launch (tickets + an agent-scope release/acquire per tile), every slice stores its
 * fp32 partial products, partial[s][row][ld_partial] for s < md_gemm_partial_slices(lin)
 * (slice_stride floats apart; no bias), and the consumer kernel below sums them in slice
 * order.  Used for the two linears that feed the residual stream in a decode step
 * (proj: text.py:53, fc2: layers.py:139). */
int32_t md_gemm_partial_slices(const md_linear* lin);
md_status md_gemm_partial_f32(const void* a, int64_t lda, const md_linear* lin, int32_t m, float* partial,
                              int64_t ld_partial, int64_t slice_stride, void* stream);
/* The same for two independent layers over the same rows in ONE launch (a decode block's proj and
 * fc2): partial0 / partial1 get md_gemm_partial_slices(lin0) / (lin1) slices. */
md_status md_gemm_partial_f32_pair(const void* a0, int64_t lda0, const md_linear* lin0, float* partial0,
                                   const void* a1, int64_t lda1, const md_linear* lin1, float* partial1,
                                   int32_t m, int64_t ld_partial, int64_t slice_stride, void* stream);

/* Block tail of a decode step, one launch (text.py:53,157-158 and the next block's text.py:145):
 *   x = bf16(bf16(x + bf16(sum_s A[s] + bias_a)) + bf16(sum_s B[s] + bias_b));  y = layer_norm(x)
 * -- the same roundings, in the same order, as two md_gemm_bf16 MD_EPI_RESIDUAL launches
 * followed by md_layernorm_bf16.  y == NULL skips the layer norm (last block). */
md_status md_reduce_residual_layernorm(void* x, int64_t ldx, const float* partial_a, int32_t slices_a,
                                       const void* bias_a, const float* partial_b, int32_t slices_b,
                                       const void* bias_b, int64_t ld_partial, int64_t slice_stride,
                                       void* y, int64_t ldy, const md_layernorm* ln, int32_t rows,
                                       int32_t dim, float eps, void* stream);

/* ---- FP8 weights for the decode regime (opt-in numerical mode; BASELINE configs[4]) -------------------------------
 * w: OCP e4m3fn bytes in MFMA-fragment order: block (nb, kb) of 32 channels x 32 features is 1 KiB at
 * ((nb * k_pad / 32 + kb) * 1024); inside it lane l (0..63) owns 16 bytes: channel 32 nb + (l & 31), bytes 0..7 =
 * features 32 kb + 8 (l >> 5) + j, bytes 8..15 = features 32 kb + 16 + 8 (l >> 5) + j.  scale: fp32 [n_pad],
 * weight[n][k] ~= scale[n] * fp8[n][k].  b: bf16 [n_pad] or NULL.  n_pad % 64 == 0, k_pad % 128 == 0, zero padded.
 * The same op as md_gemm_bf16 at m <= 64 (F.linear of text.py:30,53, layers.py:130,139, text.py:166 at q_len 1):
 * bf16 activations, exact fp8 -> bf16 products, fp32 accumulation, epilogue(scale * acc + bias) with the bf16
 * kernels' rounding points.  MD_EPI_BIAS / MD_EPI_GELU (GELU on columns >= gelu_from_col). */
/* format MD_WSTREAM_INT4_G128 (ABI 4): the reference's own quantised checkpoint format as the weight stream (layers.py:38-74,
 * QuantizedLinear: 4-bit weights in groups of 128 input features, one (scale, zero_point) pair per group).  w: nibbles in
 * MFMA-fragment order: block (nb, step, kh) of 32 channels x 64 features (the kh-th half of the 128-wide K step = of the
 * group) is 1 KiB at (((nb * k_pad / 128 + step) * 2 + kh) * 1024); lane l owns 16 bytes: channel 32 nb + (l & 31), dword t =
 * features 128 step + 64 kh + 16 t + 8 (l >> 5) + j as nibble j (bits 4 j .. 4 j + 3).  scale: fp32 pairs (scale, zero_point)
 * at [k_pad / 128][n_pad].  Every weight is rebuilt as bf16(bf16(q - zero_point) * scale), the reference's dequantize_tensor
 * (layers.py:38-44) with its two roundings: the operand is bit for bit the bf16 weight the bf16 path multiplies with, so this is
 * NOT a numerical mode -- the same layer at a quarter of the weight bytes.  k_pad == k (k % 128 == 0). */
#define MD_WSTREAM_E4M3 0
#define MD_WSTREAM_INT4_G128 1
typedef struct {
  const void* w;
  const float* scale;
  const void* b;
  int32_t n, k, n_pad, k_pad;
  int32_t format; /* MD_WSTREAM_E4M3 | MD_WSTREAM_INT4_G128.  Added in ABI 4 -- a LAYOUT BREAK: the struct grew from 40 to 48
                   * bytes, which also moves every member of md_text_block_fp8; a caller built against ABI <= 3 does not pass
                   * 0 here, it passes garbage.  Only the md_abi_version() check protects against that. */
} md_linear_fp8;
md_status md_gemm_fp8w(const void* a, int64_t lda, const md_linear_fp8* lin, void* c, int64_t ldc, int32_t m,
                       int32_t epilogue, int32_t store_pad_cols, int32_t gelu_from_col, void* stream);
/* K-slice partial products of two layers in one launch, the fp8 form of md_gemm_partial_f32_pair (already scaled,
 * no bias); md_gemm_fp8w_partial_slices(lin) slices each. */
int32_t md_gemm_fp8w_partial_slices(const md_linear_fp8* lin);
md_status md_gemm_fp8w_partial_f32_pair(const void* a0, int64_t lda0, const md_linear_fp8* lin0, float* partial0,
                                        const void* a1, int64_t lda1, const md_linear_fp8* lin1, float* partial1,
                                        int32_t m, int64_t ld_partial, int64_t slice_stride, void* stream);

/* ---- FP8 operands for the MFMA-bound linears (opt-in numerical mode; BASELINE configs[4] "CDNA4 fp8 MFMA") ---------
 * Both operands OCP e4m3fn, ROW-MAJOR with K contiguous (the layout v_mfma_f32_32x32x64_f8f6f4 consumes: a lane's
 * operand is 32 consecutive bytes of a row), fp32 accumulation:
 *   value[m][n] = a_scale * scale[n] * sum_k a8[m][k] * w8[n][k] + b[n]
 * then the bf16 kernels' rounding points (ONE rounding of value to bf16, then GELU / residual add).  The reference has
 * no fp8 path (its only quantised format is int4, layers.py:38-109): this mode is judged by tolerance against the
 * bf16 path, never by bit parity.
 * w: [n_pad][k_pad] bytes, zero padded, k_pad % 64 == 0, n_pad % 64 == 0; scale: fp32 [n_pad] (weight[n][k] ~=
 * scale[n] * fp8[n][k]); b: bf16 [n_pad] or NULL. */
typedef struct {
  const void* w;
  const float* scale;
  const void* b;
  int32_t n, k, n_pad, k_pad;
} md_linear_f8;

typedef struct {
  const void* a;      /* e4m3fn [m][lda] bytes, lda >= k_pad, lda % 16 == 0, columns k..k_pad-1 ZERO (0x00) */
  int64_t lda;
  float a_scale;      /* activation[m][k] ~= a_scale * fp8 (one scale per tensor) */
  md_linear_f8 lin;
  void* c;            /* bf16 result [m][ldc] (columns < f8_from_col when c8 is given); may be NULL if everything goes to c8 */
  int64_t ldc;
  void* c8;           /* optional e4m3fn result of columns >= f8_from_col: c8[m][n - f8_from_col] = fp8(sat(value * c8_inv_scale)) */
  int64_t ldc8;       /* bytes between rows of c8 (% 8 == 0) */
  float c8_inv_scale;
  int32_t f8_from_col; /* multiple of 64 */
  const void* r;      /* MD_EPI_RESIDUAL operand (bf16), may alias c */
  int64_t ldr;
  int32_t res_row_mod;
  int32_t m;
  int32_t epilogue;       /* MD_EPI_* */
  int32_t store_pad_cols; /* 1: also store columns [n, n_pad) (zeros) */
  int32_t gelu_from_col;  /* MD_EPI_GELU: GELU applies to columns >= this */
} md_gemm_f8_args;
md_status md_gemm_f8(const md_gemm_f8_args* args, void* stream);

/* bf16 [rows][ldx] -> e4m3fn [rows][ldy bytes]: y = fp8(sat(x * inv_scale)) for columns < cols, 0x00 for columns
 * cols..cols_pad-1 (the consumer's K padding).  cols % 8 == 0, cols_pad % 8 == 0. */
md_status md_quantize_f8(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t cols, int32_t cols_pad,
                         float inv_scale, void* stream);
/* md_layernorm_bf16 with the result rounded to bf16 (the reference's rounding point) and then quantised like
 * md_quantize_f8; columns dim..dim_pad-1 of y are written as zero. */
md_status md_layernorm_f8(const void* x, int64_t ldx, void* y, int64_t ldy, const md_layernorm* p, int32_t rows,
                          int32_t dim, int32_t dim_pad, float eps, float inv_scale, void* stream);
/* *amax = max(*amax, max |x[r][c]|) over rows x cols (calibration of the activation scales; *amax is device memory the
 * caller zeroes; non-finite values are ignored). */
md_status md_amax_bf16(const void* x, int64_t ldx, int32_t rows, int32_t cols, float* amax, void* stream);

/* Measurement / test hook, not needed by the product path: overrides one of the GEMM dispatch
 * knobs at run time (the same knobs are read once from MD_GEMM_* / MD_DECODE_* environment
 * variables at first use).  PROCESS-WIDE and not thread-safe: for sweeps and A/B tests only; nothing that decides the
 * bits of a product call lives here (that is md_gemm_args.tile_policy, per call).  The complete key list:
 *   "tile"          -1 = automatic; otherwise the id of a tile config, forced for every launch (the table of
 *                   csrc/gemm_bf16.hip, one row per id; an id it does not have runs 2):
 *                      1  256x128, eight waves, two-stage ring
 *                      2  128x128, four waves, two-stage ring (what an unknown id runs, too)
 *                      3  decode regime: 64x128 tiles, two waves, 4-deep ring
 *                     10  decode regime: 64x64 tiles, two waves, no helper waves
 *                     11  eight-wave 256x256 baseline of 20: alternating wave groups, 2 slices ahead
 *                     15  11 with a persistent tile loop
 *                     16  decode regime (default): 64x64 tiles, two compute waves + two DMA-only helper waves
 *                     17  decode regime: 64x64 tiles, FOUR compute waves + helpers, 128-wide K slices where the layer allows
 *                     18  17's four compute waves on 64-wide K slices
 *                     19  16's two compute waves on 128-wide K slices where the layer allows
 *                     20  four-wave 256x256 (16x16x32 MFMAs), persistent: the default for large launches
 *                     21  decode regime at 65 .. 128 rows (MD_TILE_DECODE_TALL): 128x64 tiles, four compute waves x 32 rows + helpers
 *                   Every id but 20 multiplies with 32x32x16 MFMAs.
 *   "small_m_rule"  tile rule of MD_TILE_BY_SHAPE launches: 1 (default) = round 5's (the 128x128 config for up to 512 tiles
 *                   of 128x128), 0 = round 2's (the cost model above 128 such tiles), n > 1 = n tiles instead of 512; same
 *                   bits either way
 *   "w4"            0: the eight-wave 256x256 kernels wherever the four-wave one would be picked (also under
 *                   MD_TILE_PINNED)
 *   "persist"       0: eight-wave kernels without their persistent tile loop
 *   "group_m"       row panels per tile-order group (0 = by shape)
 *   "decode_nt"     1: decode-regime weights streamed non-temporally
 *   "decode_cfg"    16 (default) / 17 / 18 / 19 / 10 / 3: the decode-regime tile config of launches of <= 64 rows
 *   "decode_slices" K slices per decode-regime tile (0 = by shape)
 *   "rope_fuse"     0: prefill RoPE + KV write as their own kernel instead of the qkv GEMM's epilogue
 *   "attn_skip_dead"  (not a GEMM key; the library's one tuning entry point) exact work skipping of md_attention_prefill:
 *                   bit 0 = the second 32-key half of a last key tile with no live key in it, bit 1 = waves with no live
 *                   query row; default 3, 0 = round 4's kernel; same bits whatever the value
 *   "w4_grid"       workgroups of the four-wave kernel's persistent grid (0 = one per CU)
 * Every tile config of one MFMA family accumulates K in the same order, so within a family outputs do not depend on
 * these.  Unknown key: MD_ERR_INVALID_ARG. */
md_status md_gemm_set_tuning(const char* key, int32_t value);

/* Live timing of the GEMM launches for the roofline report: while enabled,
 * md_gemm_bf16 brackets every launch with HIP events on the caller's stream.
 * md_profile_gemm(0|1) also resets the log.  md_profile_gemm_read waits for the
 * recorded events of one kernel family and returns its summed ALGORITHMIC work,
 * kernel time in ms and launch count: kind 0 = the MFMA tile kernel (m > 64),
 * work = flops 2 m n k; kind 1 = the decode-regime weight-streaming kernel
 * (m <= 64), work = weight bytes 2 n k (logical n, k).  Not for use inside
 * hipGraph capture. */
void md_profile_gemm(int32_t enable);
md_status md_profile_gemm_read(int32_t kind, double* work, double* ms, int64_t* launches);
/* Algorithmic HBM bytes of the logged launches of one family: operands read once (A rows x k_pad,
 * W n_pad x k_pad, residual rows) and results written once -- the yard-stick for the PMC traffic
 * counters (FETCH_SIZE / WRITE_SIZE) of the same step. */
md_status md_profile_gemm_bytes(int32_t kind, double* read_bytes, double* written_bytes);

/* y[r, :dim] = LN(x[r, :dim]) * w + b, fp32 statistics, eps as given
 * (reference: layers.py:118-119, default eps 1e-5).  dim % 8 == 0, dim <= 4096. */
md_status md_layernorm_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, const md_layernorm* p,
                            int32_t rows, int32_t dim, float eps, void* stream);

/* ------------------------------------------------------------------ *
 * Vision front end                                                    *
 * ------------------------------------------------------------------ */

/* uint8 HWC crops [n][crop][crop][3] -> bf16 patch rows [n*grid*grid][ld_out]
 * with feature order (c, py, px), columns >= 3*patch*patch zero-filled.  lut is
 * the 256-entry bf16 table of the reference's pixel normalisation
 * (vision.py:33-40 followed by create_patches, vision.py:44-61). */
md_status md_patchify_u8(const void* crops_u8, const void* lut_bf16, void* out, int64_t ld_out,
                         int32_t n_crops, int32_t crop, int32_t patch, void* stream);

/* same from the already-normalised bf16 CHW tensor the reference's _vis_enc
 * receives (moondream.py:168-169; create_patches vision.py:44-61). */
md_status md_patchify_bf16(const void* crops_bf16_chw, void* out, int64_t ld_out, int32_t n_crops,
                           int32_t crop, int32_t patch, void* stream);

/* ------------------------------------------------------------------ *
 * Attention                                                           *
 * ------------------------------------------------------------------ */

/* Tiled (flash-style) softmax attention on MFMA for a block of queries:
 *   ViT encoder, no mask (layers.py:163) and the decoder prefill with the
 *   prefix-LM rule (text.py:48-50 with the mask of moondream.py:138-146):
 *   key j is visible to the query at position p iff j <= p or (p < prefix and
 *   j < prefix); only keys [0, kv_len) exist.
 * Element (b, t, h, d) of q/o lives at base + b*bs + t*ts + h*hs + d; k/v alike
 * (strides in elements).  head_dim is 64 or 72.  q_pos0[b] (device int32, or
 * NULL for 0) is the position of query row 0; kv_len[b] (device int32, or NULL
 * for kv_len_all) the number of valid keys. */
typedef struct {
  const void* q;
  int64_t q_bs, q_ts, q_hs;
  const void* k;
  int64_t k_bs, k_ts, k_hs;
  const void* v;
  int64_t v_bs, v_ts, v_hs;
  void* o;
  int64_t o_bs, o_ts, o_hs;
  int32_t batch, n_heads, n_kv_heads, head_dim;
  int32_t q_len;      /* query rows per batch element */
  int32_t kv_len_all; /* used when kv_len == NULL */
  const int32_t* q_pos0;
  const int32_t* kv_len;
  int32_t prefix_len; /* bidirectional prefix; >= kv_len disables the causal rule */
  float scale;        /* 1/sqrt(head_dim) */
  /* opt-in FP8 mode (md_gemm_f8's A operand), trailing since ABI 3: when o8 != NULL the output row is ALSO written as OCP
   * e4m3 bytes -- element (b, t, h, d) at o8 + b * o8_bs + t * o8_ts + h * head_dim + d, the value being the bf16-rounded
   * output times o8_inv_scale, exactly what md_quantize_f8 makes of the bf16 output -- and o may then be NULL */
  void* o8;
  int64_t o8_bs, o8_ts; /* bytes */
  float o8_inv_scale;
} md_attn_args;

md_status md_attention_prefill(const md_attn_args* args, void* stream);

/* One query per (batch, head) against the KV slab: the decode step
 * (text.py:48-50 with the [1,1,2048] mask of moondream.py:472-474 == keys
 * [0, pos]).  q, o: [batch][n_heads*64]; slabs [batch][n_kv_heads][ctx][64];
 * kv_len[b] valid keys (device int32). */
md_status md_attention_decode(const void* q, int64_t ldq, void* o, int64_t ldo, const void* k_slab,
                              const void* v_slab, int64_t slab_batch_stride, int32_t ctx, const int32_t* kv_len,
                              int32_t batch, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                              float scale, void* stream);

/* The decode step's RoPE + KV-slab write + attention in ONE launch (MHA, head_dim 64):
 * qkv rows are the UN-rotated fused activation [q heads | k heads | v heads]; each
 * (sequence, head) workgroup rotates its q and k (rope.py:20-48), stores rotated k and v
 * at slot kv_len[b]-1 (moondream.py:74-78) and attends over keys [0, kv_len[b])
 * (text.py:48-50).  Bit-identical to md_rope_kv_write followed by md_attention_decode. */
md_status md_attention_decode_rope(const void* qkv, int64_t ld, void* o, int64_t ldo, const float* freqs,
                                   void* k_slab, void* v_slab, int64_t slab_batch_stride, int32_t ctx,
                                   const int32_t* kv_len, int32_t batch, int32_t n_heads, int32_t head_dim,
                                   int32_t rot_dim, float scale, void* stream);

/* md_attention_decode / md_attention_decode_rope with the slot table of md_text_forward_slots and the shared-prefix table of
 * md_text_forward_shared (slots, n_slots, prefix_slots, prefix_len: see there), so that tests reach the grouped kernel
 * directly.  prefix_slots == NULL: the slot-table launch.  The _rope form is MHA only. */
md_status md_attention_decode_shared(const void* q, int64_t ldq, void* o, int64_t ldo, const void* k_slab, const void* v_slab,
                                     int64_t slab_batch_stride, int32_t ctx, const int32_t* kv_len, int32_t batch, int32_t n_heads,
                                     int32_t n_kv_heads, int32_t head_dim, float scale, const int32_t* slots, int32_t n_slots,
                                     const int32_t* prefix_slots, const int32_t* prefix_len, void* stream);
md_status md_attention_decode_rope_shared(const void* qkv, int64_t ld, void* o, int64_t ldo, const float* freqs, void* k_slab,
                                          void* v_slab, int64_t slab_batch_stride, int32_t ctx, const int32_t* kv_len, int32_t batch,
                                          int32_t n_heads, int32_t head_dim, int32_t rot_dim, float scale, const int32_t* slots,
                                          int32_t n_slots, const int32_t* prefix_slots, const int32_t* prefix_len, void* stream);

/* Partial RoPE + KV-cache write (reference: rope.py:20-48, text.py:42-46,
 * moondream.py:74-78).  qkv: bf16 [batch*q_len][ld] rows laid out q|k|v.  The
 * first rot_dim features of every q and k head are read half-split, rotated in
 * fp32 with the fp32 table freqs[pos][rot_dim/2][2] (cos, sin) and written
 * INTERLEAVED; q is rewritten in place, rotated k and v go to
 * slab[b][h][pos][:].  pos = pos0[b] + t (pos0 device int32 [batch]). */
md_status md_rope_kv_write(void* qkv, int64_t ld, const float* freqs, const int32_t* pos0,
                           void* k_slab, void* v_slab, int64_t slab_batch_stride, int32_t ctx,
                           int32_t batch, int32_t q_len, int32_t n_heads, int32_t n_kv_heads,
                           int32_t head_dim, int32_t rot_dim, void* stream);

/* ------------------------------------------------------------------ *
 * Small ops                                                           *
 * ------------------------------------------------------------------ */

/* out[i, :dim] = table[ids[i], :dim]  (reference: text.py:12-13). */
md_status md_embed_tokens(const int32_t* ids, const void* table, int64_t ld_table, void* out,
                          int64_t ld_out, int32_t n, int32_t dim, void* stream);

/* next[b] = argmax_v logits[b, v] with logits[b, suppress_id] treated as -inf
 * when suppress_id >= 0 (reference: moondream.py:517,521-524); ties -> lowest
 * index (torch.argmax on CPU). */
md_status md_argmax_bf16(const void* logits, int64_t ld, int32_t batch, int32_t vocab,
                         int32_t suppress_id, int32_t* next, void* stream);

/* Temperature / top-p sampling of one token per sequence, device resident (reference:
 * moondream.py:521-528 with _apply_top_p, moondream.py:270-278):
 *   p = bf16(softmax(bf16(logits / temperature)));  in descending-p order keep the tokens whose
 *   preceding mass is <= top_p;  q = bf16(p / bf16(sum kept));  next[b] ~ q by inverse CDF over
 *   token ids with the caller's uniforms[b] in [0, 1)  (torch.multinomial draws from the same q;
 *   the random stream differs, the distribution does not).
 * logits[b, suppress_id] is treated as -inf when suppress_id >= 0 (moondream.py:517).
 * probs_out (optional, bf16 [batch][ld_probs]) receives q -- what _apply_top_p returns. */
md_status md_sample_top_p(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id,
                          float temperature, float top_p, const float* uniforms, int32_t* next,
                          void* probs_out, int64_t ld_probs, void* stream);

/* md_sample_top_p with per-row settings: temperature, top_p and uniforms are device fp32 [batch].  One workgroup per
 * row reads temperature[b] once and takes one of three paths:
 *   temperature[b] > 0:  the row is sampled exactly as md_sample_top_p samples it with the scalars
 *     (temperature[b], top_p[b]) and uniforms[b] -- the same next[b] and the same probs_out row, bit for bit (both
 *     kernels run one device function);
 *   temperature[b] == 0: greedy, next[b] = what md_argmax_bf16 gives the row (suppress_id as -inf, ties -> lowest id);
 *     top_p[b] and uniforms[b] are not read, the probs_out row is not written;
 *   temperature[b] < 0:  idle, next[b] and the probs_out row keep their contents and the row's logits are not read.
 * The greedy path uses plain loads: unlike md_argmax_bf16 there is no vocab % 8 / ld % 8 requirement.  The values in the
 * arrays are the caller's contract (finite, 0 < top_p <= 1); no host sync, no allocation: capturable. */
md_status md_sample_rows(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id,
                         const float* temperature, const float* top_p, const float* uniforms,
                         int32_t* next, void* probs_out, int64_t ld_probs, void* stream);

/* md_sample_rows with two more truncation rules per row: top_k (device int32 [batch]) and min_p (device fp32 [batch]).
 * A sampled row (temperature[b] > 0) forms z = bf16(logit / T) and p = bf16(softmax(z)) as md_sample_top_p does and takes
 * the tokens in descending p, ties by ascending id.  Each rule keeps a prefix of that order, all three judged on the same
 * unrenormalised p:
 *   top_p[b]:  md_sample_top_p's rule, bit for bit;
 *   top_k[b]:  the first top_k[b] tokens; inside the boundary value the lowest ids survive.  <= 0 or >= vocab: off;
 *   min_p[b]:  the tokens with p >= bf16(min_p[b] * p_max), p_max the row's largest bf16 probability (what
 *              `probs >= min_p * probs.max()` gives on a bf16 tensor); the best token always survives.  <= 0: off;
 *              values above 1 act as 1.
 * The survivors are the SHORTEST of the three prefixes; they are renormalised and drawn exactly as md_sample_top_p's:
 * q = bf16(p / bf16(sum kept)), inverse CDF over token ids with uniforms[b].  (HF / vLLM renormalise after top-k before
 * top-p; here the cuts do not depend on an order of application.)  A row with top_k[b] <= 0 and min_p[b] <= 0 carries the
 * bits of md_sample_rows, next[b] and probs_out row alike.  temperature[b] == 0 (greedy: md_argmax_bf16's id) and < 0 (idle:
 * nothing read or written) are md_sample_rows' paths and read neither setting.  The order is realised as there, by the
 * histogram over bf16 patterns; the walk over it carries a token count next to the mass, the top-k boundary is the
 * pattern at which the count reaches k, the min-p boundary the smallest occupied pattern >= the threshold's, and the row's
 * boundary the largest of the three patterns with the smallest survivor count inside it.  One workgroup of 1024 per row,
 * md_sample_rows' LDS.  The values in the arrays are the caller's contract; no host sync, no allocation: capturable. */
md_status md_sample_rows_filtered(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id,
                                  const float* temperature, const float* top_p, const int32_t* top_k, const float* min_p,
                                  const float* uniforms, int32_t* next, void* probs_out, int64_t ld_probs, void* stream);

/* Log-probability and rank of ONE GIVEN token per row: targets[r] in row r of logits (bf16 [rows][ld]).  One workgroup per row.
 *   Live tokens: v is live unless v == suppress_id, suppress_id >= 0 and row r is suppressed; row r is suppressed when
 *     suppress_rows == NULL or suppress_rows[r] != 0 (int32 [rows]).  The rule of md_argmax_bf16 / md_sample_* (moondream.py:517),
 *     per row here because a scoring launch mixes a sequence's first decision (not suppressed) with its later ones.
 *   t = targets[r];  m = max over live v of float(logit[v]);  s = sum over live v of exp(float(logit[v]) - m) in fp32
 *     (a -inf logit adds 0);  logprob[r] = (float(logit[t]) - m) - log(s).
 *   This is the model's OWN distribution at temperature 1, untruncated, with the suppression generation applies -- NOT the
 *     tempered / top-p-renormalised distribution a sampled token was drawn from.
 *   rank (optional, NULL to skip): rank[r] = #{live v: logit[v] > logit[t]} + #{live v < t: logit[v] == logit[t]} -- exact, and
 *     0 exactly when t is what md_argmax_bf16 returns for the row (ties go to the lowest id).
 *   t outside [0, vocab) (idle / padding rows): logprob[r] = NaN, rank[r] = -1, the logits row is not read.
 *   t the suppressed token of a suppressed row: logprob[r] = -inf, rank[r] = -1.
 * Two passes (max, then sum) in a summation order that depends on vocab alone (csrc/logprobs.hip).  Plain loads: no
 * vocab % 8 / ld % 8 requirement.  No host sync, no allocation: capturable.  rows == 0: MD_OK, nothing launched.
 * MD_ERR_INVALID_ARG: NULL logits / targets / logprob, rows < 0, vocab <= 0, ld < vocab. */
md_status md_token_logprobs(const void* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t suppress_id,
                            const int32_t* suppress_rows, const int32_t* targets, float* logprob, int32_t* rank,
                            void* stream);

/* The k most probable live tokens of every row with their log-probabilities: entry j of row r is the live token whose
 * md_token_logprobs rank is j (greater logit first, equal logits by lower id; +0.0 and -0.0 tie; a -inf logit is live, sorts
 * last by id and has log-probability -inf).  top_ids int32 [rows][k], top_logprobs fp32 [rows][k]; one workgroup per row, a
 * row's result independent of the rows beside it.
 *   Live tokens, m, s and their summation order: md_token_logprobs'.  top_logprobs[r][j] = (float(logit[id]) - m) - log(s),
 *     bit for bit what md_token_logprobs returns for targets[r] = top_ids[r][j] on the same row.
 *   gate (int32 [rows], or NULL: every row): row r is computed iff 0 <= gate[r] < vocab -- the step's token, as targets gate
 *     md_token_logprobs.  A gated-off row is not read; its k entries are -1 / NaN.
 *   A row with fewer than k live tokens: the remaining entries are -1 / NaN.  A NaN logit is out of contract.
 * Selection by a two-level radix select over the 16-bit keys of the bf16 logits (csrc/logprobs.hip), not k arg-max
 * passes.  Plain loads: no vocab % 8 / ld % 8 requirement.  No host sync, no allocation: capturable.  rows == 0: MD_OK, nothing
 * launched.  MD_ERR_INVALID_ARG: NULL logits / top_ids / top_logprobs, k < 1, k > MD_TOPK_MAX, rows < 0, vocab < 1, ld < vocab. */
#define MD_TOPK_MAX 32
md_status md_topk_logprobs(const void* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t suppress_id,
                           const int32_t* suppress_rows, const int32_t* gate, int32_t k, int32_t* top_ids,
                           float* top_logprobs, void* stream);

/* Repetition, presence and frequency penalties on the logits a token is about to be picked from, from each row's OWN history
 * of generated tokens, which the call also extends.  logits bf16 [batch][ld], updated in place; one workgroup per row, a row's
 * result independent of the rows beside it.  hist int32 [n_slots][hist_cap] and hist_len int32 [n_slots] are the caller's
 * device arrays; row r's history is that of slot s = slots ? slots[r] : slot0 + r (two live rows of one launch never share one).
 *   s < 0 (idle row): nothing is read or written -- not the logits row, not a history, not a length.
 *   Append: t = tokens_in[r], the token the row produced last.  If 0 <= t < vocab and hist_len[s] < hist_cap, hist[s][hist_len[s]] = t
 *     and hist_len[s] grows by one.  A full history drops t; a t that is no id is not appended; the row is penalised either way.
 *   Neutral row (repetition[r] == 1, presence[r] == 0, frequency[r] == 0): the append happens, the logits row is neither read
 *     nor written.
 *   Penalise: for every DISTINCT token v of the history (the one just appended included), c its count, x = float(logit[v]):
 *       if repetition[r] != 1:  x = x > 0 ? x / repetition[r] : x * repetition[r]      (the HF / vLLM rule; zero stays zero)
 *       x = x - (presence[r] + frequency[r] * float(c))
 *     in fp32, every operation rounded on its own (no fused multiply-add), then logit[v] = bf16(x), round to nearest even.
 *     Each distinct token is updated exactly once however often it occurs; a -inf logit stays -inf.
 * Cost: the history's tokens are read once and one logit per distinct token is loaded and stored -- the row is never scanned
 * (an LDS hash table finds each distinct token with its count: csrc/logits_edit.hip).  Plain loads: no vocab % 8 / ld % 8
 * requirement.  The values in the three arrays are the caller's contract (finite, repetition > 0).  No host sync, no
 * allocation: capturable.  batch == 0: MD_OK, nothing launched.
 * MD_ERR_INVALID_ARG: NULL logits / tokens_in / hist / hist_len / repetition / presence / frequency, batch < 0, vocab < 1,
 * ld < vocab, hist_cap < 1, hist_cap > MD_PENALTY_HIST_MAX (the table of 2 * hist_cap entries lives in 64 KiB of LDS). */
#define MD_PENALTY_HIST_MAX 4096
md_status md_penalize_rows(void* logits, int64_t ld, int32_t batch, int32_t vocab, const int32_t* tokens_in,
                           const int32_t* slots, int32_t slot0, int32_t* hist, int32_t hist_cap, int32_t* hist_len,
                           const float* repetition, const float* presence, const float* frequency, void* stream);

/* Constrained decoding: every row follows its own deterministic automaton over token ids; the call advances the row's state
 * by the token it consumed and sets the logits of the tokens the new state forbids to bf16 -inf (0xFF80), so that the pick
 * that follows cannot produce them.  logits bf16 [batch][ld], updated in place; one workgroup per row, a row's result
 * independent of the rows beside it.  The table (the caller's device arrays, any number of automata concatenated):
 *   row_ptr int32 [state_cap + 1], default_next int32 [state_cap], edge_tok / edge_next int32 [row_ptr[state_cap]]:
 *   state q lists the edges row_ptr[q] .. row_ptr[q + 1], their tokens strictly ascending; a token that is not listed
 *   goes to default_next[q].  A next value is a state id in [0, state_cap), MD_CONSTRAINT_FREE (the row is unconstrained
 *   from here on) or MD_CONSTRAINT_FORBID (the token may not be produced in this state).
 * state int32 [n_slots]: row r uses state[s], s = slots ? slots[r] : slot0 + r (two live rows of one launch never share one).
 *   s < 0 (idle row), or q = state[s] < 0 (MD_CONSTRAINT_FREE, MD_CONSTRAINT_DEAD): nothing of the row is read or written
 *     -- not its logits, not its state.
 *   q >= state_cap: state[s] = MD_CONSTRAINT_DEAD, the logits untouched; nothing is indexed by q.
 *   Advance (tokens_in != NULL): t = tokens_in[r], the token the row produced last.  q' = edge_next[e] when t is edge e of
 *     state q (binary search), otherwise default_next[q].  t outside [0, vocab), q' == MD_CONSTRAINT_FORBID, or a q' that
 *     is no next value (>= state_cap, < MD_CONSTRAINT_FORBID): q' = MD_CONSTRAINT_DEAD.  state[s] = q'; q' < 0: the logits
 *     are untouched.  tokens_in == NULL: q' = q (the first token, picked from the prompt pass: nothing consumed yet).
 *   Mask: logit[v] = 0xFF80 for every v in [0, vocab) whose next value in state q' -- its edge's, otherwise the default -- is
 *     MD_CONSTRAINT_FORBID.  Every other bit of the row is unchanged; columns [vocab, ld) are never written.
 * Cost: the logits are never loaded.  A default-allow state stores 2 bytes per listed forbidden token.  A default-forbid
 * state builds a vocab-bit map of its allowed tokens in LDS and sweeps the row with stores alone, 16 bytes at a time
 * wherever a whole 16-byte-aligned group is forbidden (csrc/logits_edit.hip).  No vocab % 8 / ld % 8 requirement.  No
 * host sync, no allocation: capturable.  batch == 0: MD_OK, nothing launched.
 * MD_ERR_INVALID_ARG: NULL logits / state / row_ptr / default_next / edge_tok / edge_next, batch < 0, vocab < 1, ld < vocab,
 * state_cap < 1, vocab > MD_CONSTRAIN_VOCAB_MAX (the bit map lives in 32 KiB of LDS). */
#define MD_CONSTRAIN_VOCAB_MAX 262144
#define MD_CONSTRAINT_FREE (-1)
#define MD_CONSTRAINT_DEAD (-2)
#define MD_CONSTRAINT_FORBID (-3)
md_status md_constrain_rows(void* logits, int64_t ld, int32_t batch, int32_t vocab, const int32_t* tokens_in,
                            const int32_t* slots, int32_t slot0, int32_t* state, const int32_t* row_ptr,
                            const int32_t* default_next, const int32_t* edge_tok, const int32_t* edge_next,
                            int32_t state_cap, void* stream);

/* Compiling a byte-level DFA to the table above, on the device (csrc/automaton.hip).  The DFA: trans int32 [n_states][256],
 * an entry a next state or -1 (dead; any entry outside [0, n_states) reads as dead), accept uint8 [n_states], start state 0.
 * The vocabulary: token v spells tok_bytes[tok_off[v] .. tok_off[v + 1]) (tok_off int32 [vocab + 1], non-decreasing: the
 * caller's contract; tok_bytes uint8 [n_bytes]); forbidden uint8 [vocab]: nonzero, the token is never allowed.  All device
 * arrays.  The LIFT of state q and token v, next(q, v):
 *   v == eos_id: MD_CONSTRAINT_FREE where accept[q], otherwise MD_CONSTRAINT_FORBID (whatever eos spells or forbidden says);
 *   forbidden[v], a zero-length token, or a byte range outside [0, n_bytes): MD_CONSTRAINT_FORBID;
 *   otherwise the state reached by walking v's bytes through trans from q, MD_CONSTRAINT_FORBID once a step is dead.
 * md_automaton_lift: next int32 [nq][vocab] = next(q0 + i, v) for one slab of states, 1 <= nq <= MD_AUTOMATON_SLAB,
 *   q0 + nq <= n_states.
 * md_automaton_count: for every state q, default_next[q] = the most frequent of next(q, 0 .. vocab - 1), ties to the smallest
 *   value as a signed integer (FORBID < FREE < state 0 < ..); row_ptr int32 [n_states + 1] = the exclusive scan of the
 *   numbers of tokens whose next value differs from the default, row_ptr[n_states] the total.
 * md_automaton_fill: with default_next / row_ptr as md_automaton_count left them and edge_tok / edge_next int32 [edge_cap],
 *   edge_cap >= row_ptr[n_states] (the caller reads that one number in between): state q's edges at row_ptr[q] ..
 *   row_ptr[q + 1] are exactly the tokens whose next value differs from default_next[q], strictly ascending, with that
 *   value.  Nothing is written at or beyond edge_cap.  edge_cap == 0: MD_OK, nothing launched (the arrays may be NULL).
 * The four arrays are then a table md_constrain_rows reads with state_cap = n_states.  Exact: integers only, the same
 * result on every run.  count and fill lift the states in slabs of MD_AUTOMATON_SLAB into ws (fill lifts again rather than
 * keep n_states * vocab values), ws_bytes >= md_automaton_workspace_bytes(n_states, vocab) = min(n_states,
 * MD_AUTOMATON_SLAB) * vocab * 4 (0 for sizes out of range).  No host sync, no allocation.
 * MD_ERR_INVALID_ARG, before any launch: a NULL pointer, n_states outside [1, MD_AUTOMATON_STATES_MAX], vocab < 1,
 * vocab > MD_CONSTRAIN_VOCAB_MAX, eos_id outside [0, vocab), n_bytes < 0, a slab outside the states, edge_cap < 0, ws_bytes
 * too small. */
#define MD_AUTOMATON_STATES_MAX 4096
#define MD_AUTOMATON_SLAB 256
size_t md_automaton_workspace_bytes(int32_t n_states, int32_t vocab);
md_status md_automaton_lift(const int32_t* trans, const uint8_t* accept, int32_t n_states, const int32_t* tok_off,
                            const uint8_t* tok_bytes, int64_t n_bytes, int32_t vocab, int32_t eos_id, const uint8_t* forbidden,
                            int32_t q0, int32_t nq, int32_t* next, void* stream);
md_status md_automaton_count(const int32_t* trans, const uint8_t* accept, int32_t n_states, const int32_t* tok_off,
                             const uint8_t* tok_bytes, int64_t n_bytes, int32_t vocab, int32_t eos_id, const uint8_t* forbidden,
                             int32_t* default_next, int32_t* row_ptr, void* ws, size_t ws_bytes, void* stream);
md_status md_automaton_fill(const int32_t* trans, const uint8_t* accept, int32_t n_states, const int32_t* tok_off,
                            const uint8_t* tok_bytes, int64_t n_bytes, int32_t vocab, int32_t eos_id, const uint8_t* forbidden,
                            const int32_t* default_next, const int32_t* row_ptr, int32_t* edge_tok, int32_t* edge_next,
                            int64_t edge_cap, void* ws, size_t ws_bytes, void* stream);

/* Stop strings and stop token ids: every row feeds the token it just produced to its own matcher, and the first match is
 * recorded in the row's result triple (csrc/stop.hip).  One thread per row; a row's result is independent of the rows beside it.
 * tokens int32 [batch]: the tokens just picked.  Row r uses the words of slot s = slots ? slots[r] : slot0 + r (two live
 * rows of one launch never share one).  All arrays are the caller's device arrays.
 * The table, any number of stop sets' automata concatenated (moondream_amd/stop.py: pack): trans uint16 [state_cap][256] --
 *   a complete byte-level Aho-Corasick DFA, goto and failure links folded in, so every (state, byte) has a next state;
 *   match_len uint16 [state_cap]: the length of the longest stop string that is a suffix of the state's path, 0: none;
 *   match_id int32 [state_cap]: that string's index in its stop set.  An entry of trans >= state_cap reads as state 0.
 * The rows' stop ids: row s lists ids[id_ptr[s] .. id_ptr[s + 1]) (id_ptr int32 [n_slots + 1]; at most MD_STOP_IDS_MAX of
 *   them are read; an entry of -1 matches nothing) and id_base int32 [n_slots] is the `which` of its first id (the number of
 *   strings of its stop set).
 * The vocabulary: token v spells tok_bytes[tok_off[v] .. tok_off[v + 1]) (tok_off int32 [vocab + 1], tok_bytes uint8 [n_bytes]:
 *   the layout md_automaton_lift reads).  A token outside [0, vocab), or a byte range outside [0, n_bytes], spells nothing.
 *   Both NULL: every token spells nothing (stop sets of ids alone).
 * Per slot, int32 [n_slots] each: state (the row's DFA state; negative: the row has no stop set), n_tok and n_seen (the
 *   tokens and bytes it has seen), and the result triple at / keep / which -- at is -1 until a match.
 *   s < 0 (idle row) or state[s] < 0: nothing of the row is read or written.
 *   Otherwise, with v = tokens[r], nt = n_tok[s], nb = n_seen[s]:  n_tok[s] = nt + 1 and n_seen[s] = nb + len(v) ALWAYS; and
 *   while at[s] == -1:
 *     1. v is the j-th of the row's stop ids:  at = nt, keep = nb, which = id_base[s] + j; no byte is walked.
 *     2. otherwise v's bytes are walked through trans from state[s], and state[s] becomes the state reached.  At the FIRST
 *        byte i (0-based) after which match_len[q] > 0:  at = nt, keep = nb + i + 1 - match_len[q], which = match_id[q] --
 *        the earliest end, and among the strings ending at that byte the longest.  The walk stops there: state[s] is
 *        the state q of the match, and it is not read again.
 *   A row whose at[s] >= 0 only counts.  A token of zero bytes leaves the state alone.
 * Cost: a chain of dependent trans loads, one per byte of the row's token; the bytes are fetched 16 at a time in front of
 * it and match_len is read beside it.  Integers only.  No host sync, no allocation: capturable.  batch == 0: MD_OK, nothing launched.
 * MD_ERR_INVALID_ARG: NULL tokens / trans / match_len / match_id / id_ptr / ids / id_base or a NULL state word array,
 * batch < 0, state_cap outside [1, MD_STOP_STATES_MAX], one of tok_off / tok_bytes NULL alone, and with them vocab < 1 or n_bytes < 0. */
#define MD_STOP_STATES_MAX 4096
#define MD_STOP_IDS_MAX 16
md_status md_stop_rows(const int32_t* tokens, int32_t batch, const int32_t* slots, int32_t slot0, const uint16_t* trans,
                       const uint16_t* match_len, const int32_t* match_id, int32_t state_cap, const int32_t* id_ptr,
                       const int32_t* ids, const int32_t* id_base, const int32_t* tok_off, const uint8_t* tok_bytes,
                       int32_t vocab, int64_t n_bytes, int32_t* state, int32_t* n_tok, int32_t* n_seen, int32_t* at,
                       int32_t* keep, int32_t* which, void* stream);

/* Region head, device resident (reference: region.py:12-71 inside the loop of moondream.py:653-733).
 * md_fourier_features: out[r] = [cos(f) | sin(f)], f = bf16(bf16(2 pi x[r, :in_dim]) . w[in_dim][half])
 *   (region.py:12-29; in_dim 1 for coordinates, 2 for sizes) -- the input of coord_encoder /
 *   size_encoder.
 * md_region_pick_encode: one step of the points loop for `batch` sequences with no host round trip:
 *   bins[b][g] = argmax of logits[b][g*n_bins .. (g+1)*n_bins) (ties -> lowest index), value =
 *   value_table[bin] (bf16 [n_bins]: bin/1024 for coordinates, 2^(bin/1023*10-10) for sizes --
 *   moondream.py:673-674,696-701), then the Fourier features of the value(s) as above. */
md_status md_fourier_features(const void* x, int64_t ldx, int32_t rows, int32_t in_dim, const void* w,
                              int32_t half, void* out, int64_t ld_out, void* stream);
md_status md_region_pick_encode(const void* logits, int64_t ld, int32_t batch, int32_t n_groups,
                                int32_t n_bins, const void* value_table, const void* feat_w, int32_t half,
                                int32_t* bins, int64_t ld_bins, void* feats, int64_t ld_feats, void* stream);

/* The spatial references of a batch of prompts (reference: region.py:96-136, placed by moondream.py:293-301): ONE launch
 * encodes every reference TOKEN of a call and stores it into its row of the prompt embeddings.
 * desc int32 [n][4], 16-byte aligned, one descriptor per token: {dst, kind, v0, v1} -- kind 0: a coordinate (value v0,
 * the coord_* operands), kind 1: a size (values v0, v1, the size_* operands); a value is a bf16 bit pattern in the low 16
 * bits.  For every descriptor, with row = dst - dst0 in [0, rows):
 *     feat = md_fourier_features' row of the value(s) (bit for bit),
 *     emb[row][j] = bf16(b[j] + sum_k feat[k] * w[j][k])    for j < dim, accumulated in fp32.
 * *_fw: the Fourier matrix bf16 [in_dim][*_feat / 2]; *_w: the encoder bf16 [dim][*_ldw], row-major, k < *_feat read;
 * *_b: bf16 [dim].  emb bf16 [rows][ld].  A descriptor of another kind, or whose row lies outside [0, rows), stores
 * nothing; nothing else of emb is written (plain vector stores, 8 bytes each); the caller keeps the dst values distinct.
 * A token's result depends on its values and the operands alone -- not on n, its index in the table, dst or the other
 * descriptors: a workgroup owns 16 descriptors and 64 columns (an encoder row is fetched once per 16 tokens) and sums in an
 * order fixed by *_feat (csrc/region.hip).  No host sync, no allocation: capturable.
 * MD_ERR_INVALID_ARG: a NULL pointer, n <= 0, rows <= 0, dim <= 0 or dim % 4, ld < dim or ld % 4, a *_feat <= 0, % 8 or
 * > 2048, a *_ldw < *_feat or % 4, desc not 16-byte or an encoder / bias / emb pointer not 8-byte aligned. */
md_status md_spatial_ref_embed(const int32_t* desc, int32_t n, const void* coord_fw, int32_t coord_feat,
                               const void* coord_w, int64_t coord_ldw, const void* coord_b, const void* size_fw,
                               int32_t size_feat, const void* size_w, int64_t size_ldw, const void* size_b, int32_t dim,
                               void* emb, int64_t ld, int64_t dst0, int32_t rows, void* stream);

/* md_region_pick_encode with a confidence per pick.  bins and feats: md_region_pick_encode's on the same inputs, bit for bit
 * (ties -> lowest bin, an all-NaN group -> bin 0).  logprobs fp32 [batch][ld_logprobs]: for group g of row b, with x the
 * group's bf16 logits as fp32, p = bins[b][g] and m = x[p],
 *     S = sum over every bin i of exp(x[i] - m),   W = the same sum over the bins with |i - p| <= window, inside [0, n_bins),
 *     logprobs[b][g] = log(W) - log(S):
 *   the log of the probability mass the head put within `window` bins of its pick.  window = 0: W is exactly 1 and the value is
 *   the log-softmax of the picked bin.  window >= n_bins - 1: W and S are one sum and the value is exactly 0.0f.  A -inf logit
 *   adds 0.  A NaN anywhere in the group, or a group whose maximum is not finite, gives NaN for that group.
 * One workgroup per row, a row's result independent of the rows beside it; the summation order depends on n_bins alone
 * (csrc/region.hip).  Plain loads: no alignment demand on n_bins, ld, ld_bins or ld_logprobs.  No host sync, no
 * allocation: capturable.
 * MD_ERR_INVALID_ARG: what md_region_pick_encode refuses, NULL logprobs, window < 0, ld_logprobs < n_groups. */
md_status md_region_pick_encode_scored(const void* logits, int64_t ld, int32_t batch, int32_t n_groups,
                                       int32_t n_bins, const void* value_table, const void* feat_w, int32_t half,
                                       int32_t* bins, int64_t ld_bins, void* feats, int64_t ld_feats, int32_t window,
                                       float* logprobs, int64_t ld_logprobs, void* stream);

/* Overlap-crop stitch + adaptive average pool + concat with the global crop's
 * features (reference: moondream.py:213-226, image_crops.py:170-231 with
 * patch_size=1, vision.py:83-88).  feats: bf16 [1 + th*tw][g*g][dim] for ONE
 * image (crop 0 = global).  out: bf16 [g*g][ld_out] = [global | pooled]. */
md_status md_stitch_pool_concat(const void* feats, void* out, int64_t ld_out, int32_t dim,
                                int32_t grid, int32_t margin, int32_t tiles_h, int32_t tiles_w,
                                void* stream);

/* ------------------------------------------------------------------ *
 * The seam: whole-stage entry points                                  *
 * ------------------------------------------------------------------ */

typedef struct {
  md_layernorm ln1;
  md_linear qkv, proj;
  md_layernorm ln2;
  md_linear fc1, fc2;
} md_vit_block;

/* Optional FP8 mode of the vision path (md_gemm_f8 above): e4m3 copies of every block's four linears and of the
 * projector MLP, and ONE static scale per quantised activation tensor (s_*: activation ~= s * fp8), found by a
 * calibration pass.  calib != NULL: md_vit_encode / md_vision_project run the bf16 path and record the running
 * max |x| of every quantisation site into calib (device fp32, zeroed by the caller: [4 l + {0 ln1, 1 attention,
 * 2 ln2, 3 gelu}] for block l, then [4 n_layers] the projector's concatenated input, [4 n_layers + 1] its GELU
 * output).  calib == NULL and blocks != NULL: the fp8 path runs (patch embedding, attention, layer norms'
 * statistics and the residual stream stay bf16 / fp32). */
typedef struct {
  md_linear_f8 qkv, proj, fc1, fc2;
  float s_ln1, s_att, s_ln2, s_ff;
} md_vit_block_f8;
typedef struct {
  const md_vit_block_f8* blocks; /* host array of n_layers, or NULL */
  md_linear_f8 proj_fc1, proj_fc2;
  float s_cat, s_pff;
  float* calib;
} md_vit_f8;

typedef struct {
  int32_t dim, n_heads, n_layers, ff_dim;
  int32_t patch, crop;     /* 14, 378 */
  md_linear patch_emb;
  const void* pos_emb;     /* bf16 [grid*grid][dim] */
  const md_vit_block* blocks; /* host array of n_layers */
  md_layernorm post_ln;
  md_linear proj_fc1, proj_fc2; /* vision projector MLP (vision.py:77-89) */
  const void* pixel_lut;   /* bf16 [256] */
  const md_vit_f8* f8;     /* NULL: bf16 everywhere (the reference's precision) */
  int32_t tile_policy;     /* MD_TILE_BY_SHAPE / MD_TILE_PINNED for every GEMM of this call (ABI 5) */
} md_vit_model;

enum { MD_CROPS_U8_HWC = 0, MD_CROPS_BF16_CHW = 1 };

size_t md_vit_workspace_bytes(const md_vit_model* m, int32_t n_crops);

/* vision_encoder (reference: vision.py:64-74 behind moondream.py:168-169):
 * crops -> out bf16 [n_crops][grid*grid][dim]. */
md_status md_vit_encode(const md_vit_model* m, const void* crops, int32_t crops_kind,
                        int32_t n_crops, void* out, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Image preprocessing on the device: the crops the encoder takes (MD_CROPS_U8_HWC), cut from raw RGB images with Pillow's
 * 8-bit LANCZOS resize restated as the integer arithmetic it is -- per output pixel a window [xmin, xmin + n) of taps with
 * int32 coefficients at 22 fractional bits, ((1 << 21) + sum k * pixel) >> 22 in int32 (wrapping, as C's int) clamped to
 * 0 .. 255, horizontally into a uint8 intermediate and then vertically.  With the tables of moondream_amd/resample.py the
 * crops are byte for byte those of image_crops.overlap_crop_image on its PIL branch.
 *   packed (device, 16-byte aligned, packed_bytes long): [descriptors | coefficient tables | raw RGB pixels], one upload.
 *   The descriptors are n_images x MD_RESAMPLE_DESC_WORDS int64 at byte 0; offsets are bytes from `packed`:
 *     0 src_h  1 src_w  2 tiles_h  3 tiles_w  4 crop0 (the image's first crop slot)  5 mode  6 pixels (uint8 [src_h][src_w][3],
 *     a multiple of 16)  7 the image's intermediates (bytes from `workspace`)
 *     8 + 12 * t .. : target t -- out_h, out_w, taps per row of the horizontal and of the vertical table, then the offsets
 *     (multiples of 4) of the horizontal bounds int32 [out_w][2] = (xmin, n), the horizontal coefficients int32 [out_w][taps],
 *     the vertical bounds [out_h][2] and the vertical coefficients [out_h][taps], then the target's first workgroup in the
 *     horizontal and in the vertical launch.
 *   mode MD_RESAMPLE_TWO_TARGETS: target 0 (crop x crop, the global crop) goes to slot crop0; target 1, of size
 *     (tiles_h * window + 2 * margin_px) x (tiles_w * window + 2 * margin_px), is never stored as an image: each of its pixels
 *     goes into every slot crop0 + 1 + ty * tiles_w + tx whose window [ty * window, ty * window + crop) x [tx * window, ..)
 *     holds it.  MD_RESAMPLE_BOTH_SLOTS (tiling (1, 1): the global and the local crop are one computation): target 0 goes to
 *     slots crop0 and crop0 + 1.  MD_RESAMPLE_ONE_SLOT: to crop0 alone (the caller encodes it once).
 *   Canonical order is part of the contract and checked: crop0 and the intermediates' offsets are running sums over the
 *     images (an image's intermediates: target 0's uint8 [src_h][pitch], then target 1's; pitch = out_w * 3 rounded up to
 *     16), the workgroup prefixes are running sums of ceil(out_w * 3 / MD_RESAMPLE_H_SEG_BYTES) * ceil(src_h /
 *     MD_RESAMPLE_H_ROWS) and of ceil(pitch / MD_RESAMPLE_V_SEG_BYTES) * ceil(out_h / MD_RESAMPLE_V_ROWS) over (image,
 *     target), an absent target carrying its successor's; total_crops is the sum of the images' slots.
 *   host_desc: the SAME descriptors in host memory: they are what is validated, before any launch -- every size, offset and
 *     extent against packed_bytes, total_crops and workspace_bytes.  The tables' CONTENTS are device data: a window that
 *     leaves the image or the staged span contributes nothing (no address outside the image, the workspace or crops_out is
 *     formed), and the result is then not PIL's.
 *   crops_out: uint8 [total_crops][crop][crop][3]; every byte of it is written, nothing outside it.
 * Two launches over the whole chunk, each a flat list of workgroups over (image, target).  No host sync, no allocation.
 * MD_ERR_INVALID_ARG: NULL or misaligned pointers, n_images outside 1 .. MD_RESAMPLE_MAX_IMAGES, crop != window + 2 *
 * margin_px, a side outside 1 .. MD_RESAMPLE_MAX_SIDE, an unknown mode, target sizes that are not the geometry's, anything
 * that is not in canonical order or reaches outside packed_bytes.  MD_ERR_WORKSPACE: workspace_bytes below
 * md_image_resample_workspace_bytes.  MD_ERR_UNSUPPORTED: a horizontal scale whose staged span does not fit the LDS. */
#define MD_RESAMPLE_DESC_WORDS 32
#define MD_RESAMPLE_MAX_SIDE 16384
#define MD_RESAMPLE_MAX_IMAGES 4096
#define MD_RESAMPLE_H_SEG_BYTES 256
#define MD_RESAMPLE_H_ROWS 4
#define MD_RESAMPLE_V_SEG_BYTES 1024
#define MD_RESAMPLE_V_ROWS 8
enum { MD_RESAMPLE_TWO_TARGETS = 0, MD_RESAMPLE_BOTH_SLOTS = 1, MD_RESAMPLE_ONE_SLOT = 2 };
size_t md_image_resample_workspace_bytes(const int64_t* host_desc, int32_t n_images);
md_status md_image_resample_crops(const void* packed, size_t packed_bytes, const int64_t* host_desc, int32_t n_images,
                                  int32_t crop, int32_t window, int32_t margin_px, void* crops_out, int32_t total_crops,
                                  void* workspace, size_t workspace_bytes, void* stream);

size_t md_vision_project_workspace_bytes(const md_vit_model* m, int32_t n_images);

/* vision_projection for n_images images that all share one tiling
 * (reference: vision.py:77-89 behind moondream.py:171-172, plus the stitch of
 * moondream.py:213-226).  feats: [n_images][1 + th*tw][g*g][dim];
 * out: bf16 [n_images][g*g][ld_out] (proj_out_dim columns). */
md_status md_vision_project(const md_vit_model* m, const void* feats, int32_t n_images,
                            int32_t tiles_h, int32_t tiles_w, int32_t margin, void* out,
                            int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream);

/* The seam form of the same stage: _vis_proj(g, r) with r the ALREADY stitched
 * [H][W][dim] grid, exactly what the reference passes (moondream.py:171-172,
 * vision.py:77-89).  global_feats: [g*g][dim]; out: [g*g][ld_out].  Workspace:
 * md_vision_project_workspace_bytes(m, 1). */
md_status md_vision_project_grid(const md_vit_model* m, const void* global_feats,
                                 const void* grid_feats, int32_t H, int32_t W, void* out,
                                 int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream);

typedef struct {
  md_layernorm ln;
  md_linear qkv, proj, fc1, fc2;
  /* Optional fusion: qkv and fc1 read the same LayerNorm output (text.py:145-157), so
   * their weights may be packed as ONE matrix [qkv rows | fc1 rows] and run as one
   * GEMM (GELU on the fc1 columns only); every output element is computed exactly
   * as by the two separate layers.  w == NULL: not packed, the two layers run
   * separately. */
  md_linear qkv_fc1;
} md_text_block;

/* Optional FP8 copies of the decoder's weight stream: used by md_text_forward / md_lm_head / md_decode_step for
 * launches of <= 64 rows (the decode regime) when md_text_model.fp8 is set; prefill always runs the bf16 weights.
 * A member with w == NULL falls back to bf16 for that layer. */
typedef struct {
  md_linear_fp8 qkv_fc1, proj, fc2;
} md_text_block_fp8;
typedef struct {
  const md_text_block_fp8* blocks; /* host array of n_layers */
  md_linear_fp8 lm_head;
} md_text_fp8;

/* Optional FP8 mode of the decoder's PREFILL (launches of more than 64 rows; md_gemm_f8): e4m3 copies of the fused
 * qkv|fc1, proj and fc2 matrices of every block and one static scale per quantised activation tensor.  calib as in
 * md_vit_f8: [3 l + {0 ln, 1 attention, 2 gelu}].  Needs the fused qkv|fc1 packing.  RoPE, attention, the KV cache
 * and the residual stream stay bf16. */
typedef struct {
  md_linear_f8 qkv_fc1, proj, fc2;
  float s_ln, s_att, s_ff;
} md_text_block_f8;
typedef struct {
  const md_text_block_f8* blocks; /* host array of n_layers, or NULL */
  float* calib;
} md_text_f8;

typedef struct {
  int32_t dim, n_heads, n_kv_heads, n_layers, ff_dim, vocab, max_context, prefix_len, rot_dim;
  const md_text_block* blocks; /* host array of n_layers */
  md_layernorm post_ln;
  md_linear lm_head;
  const void* wte;       /* bf16 [vocab][dim] */
  const float* freqs;    /* fp32 [max_context][rot_dim/2][2] */
  const md_text_fp8* fp8; /* NULL: bf16 weights everywhere (the reference's precision) */
  const md_text_f8* f8;  /* NULL: bf16 prefill */
  int32_t tile_policy;   /* MD_TILE_BY_SHAPE / MD_TILE_PINNED for every GEMM of this call (ABI 5) */
} md_text_model;

/* KV slabs: layer l's keys at k + l*layer_stride, element (b,h,p,d) at
 * b*batch_stride + (h*ctx + p)*64 + d (the reference's [1,H,2048,64] slab per
 * sequence, moondream.py:62-72, batched on a leading axis). */
typedef struct {
  void* k;
  void* v;
  int64_t layer_stride, batch_stride; /* elements */
  int32_t ctx;
  /* Optional e4m3fn copy of the cache for the decode steps of the fp8 mode (NULL: bf16 only): slabs of the same shape with
   * one byte per element and ONE static scale per layer (HOST arrays of n_layers floats: value ~= scale * fp8).  When
   * set, md_text_forward keeps both copies current (prefill rows are quantised after the bf16 rows are written, a
   * decode step writes the new row into both) and the decode attention reads the e4m3 copy -- half the bytes of the
   * step's dominant stream.  MHA with head_dim 64 only; md_text_forward_lora and md_decode_step_b1 ignore it. */
  void* k8;
  void* v8;
  const float* k_scale;
  const float* v_scale;
} md_kv_cache;

/* md_attention_decode_rope over the e4m3 copy of ONE layer's slabs (k8 / v8: that layer's e4m3 K / V slab, k_scale /
 * v_scale its scales): RoPE of the new token's q / k, the new K / V row written into BOTH copies, attention of every
 * (sequence, head) over keys [0, kv_len[b]) of the e4m3 copy with the new row taken as the cache will hold it
 * (quantised, dequantised).  head_dim 64, MHA.  Tolerance-judged against md_attention_decode_rope. */
md_status md_attention_decode_rope_f8(const void* qkv, int64_t ld, void* o, int64_t ldo, const float* freqs, void* k_slab,
                                      void* v_slab, void* k8_slab, void* v8_slab, int64_t slab_batch_stride, int32_t ctx,
                                      const int32_t* kv_len, int32_t batch, int32_t n_heads, int32_t rot_dim, float scale,
                                      float k_scale, float v_scale, void* stream);

/* md_attention_decode_rope_f8 with the slot table of md_text_forward_slots and the shared-prefix table of
 * md_text_forward_shared (slots, n_slots, prefix_slots, prefix_len: see there), so that tests reach the grouped e4m3
 * kernel directly: row b reads keys [0, prefix_len[b]) from slot prefix_slots[b] of the e4m3 slabs, the rest from its own
 * slot, and writes the new row (both copies) to its own slot only.  Every output bit and slab byte of a live row equals
 * what the call without a prefix table gives over a slot that holds a copy of the prefix.  prefix_slots == NULL: the
 * slot-table launch of md_attention_decode_rope_f8's kernel.  A prefix slot's e4m3 bytes are its WRITER's job: an image
 * prefill into the slot through md_text_forward* quantises them, anything else calls md_kv_quantize_f8. */
md_status md_attention_decode_rope_f8_shared(const void* qkv, int64_t ld, void* o, int64_t ldo, const float* freqs, void* k_slab,
                                             void* v_slab, void* k8_slab, void* v8_slab, int64_t slab_batch_stride, int32_t ctx,
                                             const int32_t* kv_len, int32_t batch, int32_t n_heads, int32_t rot_dim, float scale,
                                             float k_scale, float v_scale, const int32_t* slots, int32_t n_slots,
                                             const int32_t* prefix_slots, const int32_t* prefix_len, void* stream);

/* (Re)build the e4m3 copy from the bf16 slabs for positions pos .. pos + n_pos - 1 of `batch` slots, every layer and
 * head (pos = pos0[b], device int32, or pos_fixed when pos0 is NULL): after bf16 rows were written by something other
 * than md_text_forward (load_encoded_image's copy). */
md_status md_kv_quantize_f8(const md_kv_cache* kv, int32_t n_layers, int32_t batch, int32_t n_heads, const int32_t* pos0,
                            int32_t pos_fixed, int32_t n_pos, void* stream);

/* Beam search, the reorder: for every row r, key and value positions [from[r], to[r]) of EVERY layer and head are copied from
 * slot src[r] to slot dst[r] of the bf16 slabs -- a surviving beam's KV tail goes where its child will read it.  src, dst,
 * from, to: device int32 [rows].  One (row, layer, head, K|V) piece is one contiguous run of (to - from) * 128 bytes (head_dim
 * 64); a workgroup of 256 moves the K and the V runs of every head of one (row, layer) with 16-byte loads and stores, up to
 * four loads in flight per lane before their stores.  Run lengths are device data: the grid is n_layers x rows (1536
 * workgroups at 2B with 64 rows; one per head would be 49152, most of them skipped copies), and a workgroup with nothing to
 * do exits.
 *   A row is skipped entirely when dst[r] < 0, src[r] < 0, src[r] == dst[r] or to[r] <= from[r] -- and, so that no address
 *     outside the slabs is ever formed, when a slot is >= n_slots, from[r] < 0 or to[r] > kv->ctx.
 *   Caller contract: no dst of a live row equals any live row's src, and live dst values are distinct; the launch then has no
 *     read / write hazard.  md_beam_select's hand-off satisfies it by construction.
 *   No byte outside the named runs is written.  No host sync, no allocation: capturable.  rows == 0: MD_OK, nothing launched.
 * MD_ERR_INVALID_ARG: NULL kv / slabs / arrays, rows < 0, n_layers < 1, n_heads < 1, n_slots <= 0, slabs or strides that are
 * not 16-byte multiples, batch_stride < n_heads * ctx * 64, n_slots * batch_stride > layer_stride, or a cache with the e4m3
 * copy attached (kv->k8 / kv->v8: beam search is not served in the fp8 KV mode). */
md_status md_kv_copy_tail(const md_kv_cache* kv, int32_t n_layers, int32_t n_heads, int32_t n_slots, int32_t rows,
                          const int32_t* src, const int32_t* dst, const int32_t* from, const int32_t* to, void* stream);

/* Beam search, the choice: the next num_beams beams of every request from num_beams x vocab candidates, the finished
 * hypotheses' pool, the done rule and the KV slot hand-off, on the device.  Rows are groups x W, W = num_beams in 1 ..
 * MD_BEAM_MAX (2W <= MD_TOPK_MAX); row r is beam r % W of group r / W.  Everything in md_beam_state is the CALLER's device
 * memory, read and rewritten by the call:
 *   cum fp32 [rows]        each beam's summed log-probability; -inf: a dead beam
 *   cur int32 [rows]       the slot each beam decodes in (the slot table of the decode step); -1: an idle row
 *   own int32 [rows][2]    the two slots a row owns (read only); cur[r] starts as own[r][0]
 *   len int32 [groups]     the tokens the group's hypotheses hold (0 before the first decision)
 *   done int32 [groups]    != 0: the group is finished
 *   prefix_len int32 [groups]   (read only) the positions of the group's shared prefix
 *   pool_n int32 [groups], pool_score fp32 / pool_sum fp32 / pool_parent int32 / pool_step int32 [groups][W]: the finished
 *     hypotheses: normalised score h, raw sum s, the beam j whose continuation by eos it is, and len at that decision -- its
 *     tokens are the pool_step tokens read back from beam pool_parent through parent planes pool_step - 1 .. 0
 *   inv_norm fp32 [n_norm] (read only): inv_norm[n] = float32(1 / n ** length_penalty), the host's, computed in float64;
 *     an index beyond the table reads its last entry
 *   cand_ids int32 / cand_lp fp32 [rows][2W]: scratch, left holding the call's per-row candidates
 * Row phase.  beams_in is W, or 1 for the first decision: group g then reads logits row g and beam 0 alone is live.  Entry i
 *   of a live row j is what md_topk_logprobs(k = 2W) returns for the row's logits, ids and fp32 log-probabilities bit for bit
 *   (the same device function; suppress_id / suppress_rows as there, suppress_rows indexed by the logits row).  A beam with
 *   cum == -inf is not read.
 * Group order.  Candidate (j, i) has score s = cum[j] + lp[j][i], one fp32 add; candidates of a dead beam and entries of id -1
 *   do not exist.  Order: s descending, then j ascending, then i ascending.
 * Walk over the first 2W candidates in that order, walk index w = 0, 1, ..; L = len[g] before the call:
 *   token == eos_id (eos_id >= 0) and w < W: a finished hypothesis of score h = s * inv_norm[L + 1] (one fp32 multiply; no
 *     powf, no divide) enters the pool -- appended while pool_n < W, otherwise it replaces the entry of lowest score (among
 *     equal scores the one of highest index) and only if h is strictly greater;
 *   token == eos_id and w >= W: dropped (the HF rule);
 *   any other candidate is the next live beam n = 0, 1, .. until W are chosen: tokens_out[g*W+n] = token, parent[g*W+n] = j,
 *     cum[g*W+n] = s.  Beams that are not filled are dead: cum = -inf, parent -1, cur -1 (an idle decode row) and
 *     tokens_out 0 -- an id the next step's embedding lookup can read, which -1 is not; parent -1 is what marks the row.
 * Done.  len[g] = L + 1.  The group is done when no live beam is left, or when the pool is full and either early_stopping or
 *   cum[g*W] * inv_norm[L + 1] <= the pool's lowest score (HF's early_stopping=False test: the best live beam cannot beat
 *   the worst finished one).  A group that becomes done has cur = -1 and src = dst = -1 in all its rows; later calls neither
 *   read nor write anything of a done group.
 * Slot hand-off, inside the group; every cur is read before any is written.  Child n with parent n keeps its slot and emits
 *   src = dst = cur[n] (a skipped copy).  Child n with parent p != n emits src = cur[p] (before the call), dst = the one of
 *   own[n] that is not cur[n], and cur[n] becomes it: a dst is never any row's current slot, which is md_kv_copy_tail's
 *   contract.  from = prefix_len[g], to = prefix_len[g] + L (the position after the token the step consumed) are written for EVERY row of
 *   a group that was not done at entry, dead rows included; a dead row has src = dst = cur = -1, which is what skips its copy.
 * One launch of 1024 per row (the row phase), one wave per group (merge, walk, pool and hand-off from LDS).  NaN logits are
 * out of contract.  No host sync, no allocation: capturable.  groups == 0: MD_OK, nothing launched.
 * MD_ERR_INVALID_ARG: NULL logits / st / any array of st / tokens_out / parent / src / dst / from / to, groups < 0,
 * num_beams outside 1 .. MD_BEAM_MAX, beams_in neither 1 nor num_beams, vocab < 1, ld < vocab, n_norm < 1, early_stopping
 * neither 0 nor 1. */
#define MD_BEAM_MAX 16
typedef struct {
  float* cum;
  int32_t* cur;
  const int32_t* own;
  int32_t* len;
  int32_t* done;
  const int32_t* prefix_len;
  int32_t* pool_n;
  float* pool_score;
  float* pool_sum;
  int32_t* pool_parent;
  int32_t* pool_step;
  const float* inv_norm;
  int32_t n_norm;
  int32_t* cand_ids;
  float* cand_lp;
} md_beam_state;
md_status md_beam_select(const void* logits, int64_t ld, int32_t groups, int32_t num_beams, int32_t beams_in, int32_t vocab,
                         int32_t suppress_id, const int32_t* suppress_rows, int32_t eos_id, int32_t early_stopping,
                         const md_beam_state* st, int32_t* tokens_out, int32_t* parent, int32_t* src, int32_t* dst,
                         int32_t* from, int32_t* to, void* stream);

size_t md_text_workspace_bytes(const md_text_model* m, int32_t batch, int32_t q_len);

/* text_decoder over a block of q_len new tokens per sequence (reference:
 * text.py:128-160 behind moondream.py:174-192): x bf16 [batch*q_len][dim]
 * (embeddings) -> hidden bf16 [batch*q_len][dim]; writes K,V at positions
 * pos0[b] .. pos0[b]+q_len-1 of every layer's slab.  x may alias hidden. */
md_status md_text_forward(const md_text_model* m, const void* x, void* hidden, int32_t batch,
                          int32_t q_len, const int32_t* pos0, const md_kv_cache* kv,
                          void* workspace, size_t workspace_bytes, void* stream);

/* md_text_forward where sequence b's K / V live in slot slots[b] of kv (slot 0 at kv->k / kv->v, slot j at j * batch_stride),
 * not in slot b -- the library side of continuous batching: rows of one launch address any slots of a slab, so finished
 * sequences leave a decode step and new ones take their slots without moving a cache row.
 * slots: device int32 [batch], or NULL (== md_text_forward).  n_slots: slots addressable from kv (n_slots * batch_stride <=
 * layer_stride).
 * q_len == 1 only: a row whose slot is < 0 or >= n_slots is IDLE -- its hidden / logits rows are computed but unspecified, and it
 * reads and writes no slab memory (no K / V write, no attention over a slab; its attention output is zero).
 * q_len > 1 (prefill): every slot must be valid and distinct (caller contract, as pos0 is today).
 * The slot table changes addresses only: a row gets the same bits from its slot as md_text_forward gives it in slot b.
 * Workspace: md_text_workspace_bytes(m, batch, q_len). */
md_status md_text_forward_slots(const md_text_model* m, const void* x, void* hidden, int32_t batch, int32_t q_len,
                                const int32_t* pos0, const int32_t* slots, int32_t n_slots, const md_kv_cache* kv,
                                void* workspace, size_t workspace_bytes, void* stream);

/* md_text_forward_slots with a SHARED KV PREFIX: row b reads key positions j < prefix_len[b] from slot prefix_slots[b] and
 * keys j >= prefix_len[b] from its own slot slots[b] -- one image prefix, prefilled once, serves many prompts without a copy.
 * prefix_slots, prefix_len: device int32 [batch]; prefix_slots[b] < 0 (or >= n_slots): no shared prefix for the row.
 * prefix_slots == NULL: md_text_forward_slots (the same launches).  Otherwise slots must not be NULL.  Every write goes to
 * slots[b]; the prefix slots are only read.  Caller contract (checked by the Python layer): pos0[b] >= prefix_len[b], and no
 * row's own slot is another row's prefix slot in the same call.  Idle rows as in md_text_forward_slots.
 * Bits: every output of a row (hidden, the K / V rows written) equals md_text_forward_slots' over a slot into which keys
 * [0, prefix_len[b]) of the prefix slot have been copied.  The decode attention groups rows: one K / V load of a prefix row
 * serves every row of a group sharing its prefix slot.
 * The e4m3 copy of the fp8 mode (kv->k8 / v8 with k_scale / v_scale; MHA, head_dim 64): the prompt prefill attends over the
 * bf16 slabs and quantises its rows into the rows' own slots; a decode step attends over the e4m3 copy with the same
 * addressing rule and grouping (csrc/attention_f8kv.hip), and the bit statement above holds for all four slabs.  The e4m3
 * bytes of a prefix slot are its writer's job: an image prefill into the slot quantises them, md_kv_quantize_f8 after any
 * other write (load_encoded_image's copy).
 * kv->k8 / kv->v8 without both scale arrays, NULL kv, slots with n_slots <= 0: MD_ERR_INVALID_ARG.
 * Workspace: md_text_workspace_bytes(m, batch, q_len). */
md_status md_text_forward_shared(const md_text_model* m, const void* x, void* hidden, int32_t batch, int32_t q_len,
                                 const int32_t* pos0, const int32_t* slots, int32_t n_slots, const int32_t* prefix_slots,
                                 const int32_t* prefix_len, const md_kv_cache* kv, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* The decoder for a caller that does not keep every hidden row.  hidden_mode:
 *   MD_HIDDEN_ALL   every row in hidden [batch*q_len][dim]: md_text_forward_shared (hidden_last is not read);
 *   MD_HIDDEN_LAST  the last row of every sequence in hidden_last bf16 [batch][dim] (16-byte aligned) -- what lm_head and
 *                   the first decode step read after a prefill;
 *   MD_HIDDEN_NONE  no hidden row (hidden_last may be NULL): the K / V rows of the slab are the result (an image prefill).
 * In the last two modes hidden [batch*q_len][dim] is working memory whose contents are unspecified afterwards (x may still
 * alias it).  slots / prefix_slots / prefix_len as in md_text_forward_shared, each may be NULL (slots == NULL: sequence b in
 * slot b, md_text_forward).
 * What it saves: in the LAST block the decode steps read only K and V of every row, so ln(x) and the [q | k | v] columns of
 * the packed qkv|fc1 layer run over all rows (K / V leave from the RoPE epilogue as ever) and everything else -- the fc1
 * columns, attention, proj, fc2, the residual adds -- runs for the kept rows only: the query block of 128 rows that holds
 * the sequences' last rows, then the `batch` last rows gathered into compact buffers, through the same 256x256 kernel
 * (MD_TILE_PINNED_ANY_ROWS).
 * Bits: hidden_last and every K / V row written equal md_text_forward*'s.  The trim applies where that can be promised:
 * q_len > 1, batch * q_len > 64, the packed qkv|fc1 layer, tile_policy MD_TILE_PINNED, no fp8 prefill / calibration
 * (m->f8), no e4m3 copy of the cache; everywhere else the call runs the full computation and copies the last rows out, so
 * a caller never branches.  hidden_mode outside the three values, MD_HIDDEN_LAST with hidden_last NULL or misaligned:
 * MD_ERR_INVALID_ARG.  Workspace: md_text_workspace_bytes(m, batch, q_len). */
enum { MD_HIDDEN_ALL = 0, MD_HIDDEN_LAST = 1, MD_HIDDEN_NONE = 2 };
md_status md_text_forward_trim(const md_text_model* m, const void* x, void* hidden, void* hidden_last, int32_t hidden_mode,
                               int32_t batch, int32_t q_len, const int32_t* pos0, const int32_t* slots, int32_t n_slots,
                               const int32_t* prefix_slots, const int32_t* prefix_len, const md_kv_cache* kv, void* workspace,
                               size_t workspace_bytes, void* stream);

/* LoRA "variant" side path (reference: lora.py:54-79 -> text.py:31-32,55-56 and layers.py:129-146 with lora != None).
 * delta(x) = (x A^T) B^T with A [r][k] and B [n][r] packed as bias-free md_linear (r zero-padded to 64); a pair with
 * a.w == NULL is absent.  Per block, in the reference's order and with its bf16 roundings:
 *   qkv  = bf16(qkv(l_in) + delta_qkv(l_in))
 *   attn = bf16(proj(att) + delta_proj(l_in))        -- sic: the reference feeds the BLOCK INPUT to this pair (text.py:55)
 *   h    = gelu(bf16(fc1(l_in) + delta_fc1(l_in)));  mlp = bf16(fc2(h) + delta_fc2(h))
 *   x    = bf16(bf16(x + attn) + mlp) */
typedef struct {
  md_linear a, b;
} md_lora_pair;
typedef struct {
  md_lora_pair qkv, proj, fc1, fc2;
} md_text_block_lora;

/* md_text_forward with the side path: lora = host array of n_layers entries (NULL: plain md_text_forward).
 * Runs the unfused kernels (separate qkv / fc1, stand-alone GELU and adds). */
size_t md_text_lora_workspace_bytes(const md_text_model* m, int32_t batch, int32_t q_len);
md_status md_text_forward_lora(const md_text_model* m, const md_text_block_lora* lora, const void* x, void* hidden,
                               int32_t batch, int32_t q_len, const int32_t* pos0, const md_kv_cache* kv,
                               void* workspace, size_t workspace_bytes, void* stream);

/* out[r, :cols] = bf16(a[r, :cols] + b[r, :cols]);  out = gelu_tanh(a)  (bf16 rows, cols % 8 == 0). */
md_status md_add_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int32_t rows,
                      int32_t cols, void* stream);
md_status md_gelu_bf16(const void* a, int64_t lda, void* out, int64_t ldo, int32_t rows, int32_t cols, void* stream);

size_t md_lm_head_workspace_bytes(const md_text_model* m, int32_t batch);

/* lm_head on the LAST token of each sequence (reference: text.py:163-167):
 * hidden [batch*q_len][dim] -> logits bf16 [batch][ld_logits]. */
md_status md_lm_head(const md_text_model* m, const void* hidden, int32_t batch, int32_t q_len,
                     void* logits, int64_t ld_logits, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Single-sequence decode as ONE persistent kernel (csrc/decode_b1.hip): all decoder blocks of one token inside one
 * launch of one workgroup per CU, grid barriers instead of kernel boundaries (the body of _decode_one_tok,
 * moondream.py:183-192 -> text.py:128-160, at batch 1).  x_in / hidden: bf16 [dim]; kv: the sequence's slot
 * (k / v pointing at its batch entry); sync_state: >= 16 KiB of device memory owned by the caller, ZERO before first
 * use and written by nothing else (barrier counters carry over from launch to launch; word 704 is raised if a
 * barrier ever timed out).  fp32 matrix-vector products and per-slice softmax maxima: the same tolerance against the
 * reference as the batched kernels, not bit-identical to them.  Needs the fused qkv|fc1 packing and n_kv_heads ==
 * n_heads, head_dim 64. */
size_t md_decode_b1_workspace_bytes(const md_text_model* m);
/* 1 when md_decode_step_b1 / md_decode_b1_layers can run this model with this cache on the current device: every static
 * limit of the kernel (dims, head layout, ctx <= 2048, fused packing, biases present, no fp8 weights attached) AND one
 * workgroup per CU of its grid resident at once (occupancy query; its software grid barriers need the whole grid on
 * the chip).  0: use md_decode_step.  Callers should also keep it off streams that run next to other persistent
 * kernels: co-residency with ANOTHER kernel's workgroups cannot be queried (a barrier then times out, raises word 704
 * of sync_state and the step's outputs are invalid -- repeat the step with md_decode_step). */
int32_t md_decode_step_b1_supported(const md_text_model* m, const md_kv_cache* kv);
md_status md_decode_b1_layers(const md_text_model* m, const void* x_in, void* hidden, const int32_t* pos,
                              const md_kv_cache* kv, void* workspace, size_t workspace_bytes, void* sync_state,
                              void* stream);
/* md_decode_step for ONE sequence on that kernel: embed -> md_decode_b1_layers -> lm_head -> suppress -> argmax;
 * pos[0] += 1.  Workspace: md_decode_step_b1_workspace_bytes(m). */
size_t md_decode_step_b1_workspace_bytes(const md_text_model* m);
md_status md_decode_step_b1(const md_text_model* m, const int32_t* token, int32_t* next, int32_t* pos,
                            const md_kv_cache* kv, int32_t suppress_id, void* logits, int64_t ld_logits,
                            void* workspace, size_t workspace_bytes, void* sync_state, void* stream);

/* One greedy decode step for the whole batch, device-resident (the body of the
 * reference's generator loop, moondream.py:512-530, without its per-token host
 * sync): embed tokens[b] -> decoder at pos[b] -> lm_head -> suppress
 * suppress_id -> argmax -> next[b]; pos[b] += 1.  done[b] != 0 sequences are
 * still computed (lockstep) but keep their token. */
md_status md_decode_step(const md_text_model* m, const int32_t* tokens, int32_t* next, int32_t* pos,
                         int32_t batch, const md_kv_cache* kv, int32_t suppress_id, void* logits,
                         int64_t ld_logits, void* workspace, size_t workspace_bytes, void* stream);

size_t md_decode_workspace_bytes(const md_text_model* m, int32_t batch);

/* md_decode_step with the slot table of md_text_forward_slots (embed -> md_text_forward_slots -> lm_head -> suppress -> argmax;
 * pos[b] += 1 for every row, idle ones included).  slots == NULL: md_decode_step.  An idle row's next[b] is unspecified.
 * Workspace: md_decode_workspace_bytes(m, batch). */
md_status md_decode_step_slots(const md_text_model* m, const int32_t* tokens, int32_t* next, int32_t* pos,
                               int32_t batch, const int32_t* slots, int32_t n_slots, const md_kv_cache* kv,
                               int32_t suppress_id, void* logits, int64_t ld_logits, void* workspace,
                               size_t workspace_bytes, void* stream);

/* md_decode_step_slots with the shared-prefix table of md_text_forward_shared (prefix_slots == NULL: md_decode_step_slots).
 * Workspace: md_decode_workspace_bytes(m, batch). */
md_status md_decode_step_shared(const md_text_model* m, const int32_t* tokens, int32_t* next, int32_t* pos, int32_t batch,
                                const int32_t* slots, int32_t n_slots, const int32_t* prefix_slots, const int32_t* prefix_len,
                                const md_kv_cache* kv, int32_t suppress_id, void* logits, int64_t ld_logits, void* workspace,
                                size_t workspace_bytes, void* stream);

/* Mixed LoRA variants in one batch (csrc/lora_multi.hip).  A BANK holds up to MD_LORA_MAX_VARIANTS resident variants; a
 * device int32 table variant[b] names sequence b's variant, and every value outside [0, n_variants) (-1 by convention) is
 * the base model.  Every token row of sequence b (q_len > 1: one segment) takes variant[b].  Per block, each row follows
 * the rounding order of md_text_forward_lora's comment (the reference's): qkv = bf16(bf16(qkv(l_in)) + bf16(delta)), and so
 * on.  A row's result does not depend on the other rows of the call or on their variants.
 *
 * The bank: rank[v][pair] is the packed rank of pair (0 qkv, 1 proj, 2 fc1, 3 fc2) of variant v, the true rank rounded up
 * to 16 (0: no such pair in any layer), at most MD_LORA_MAX_RANK.  table: device memory of md_lora_bank_table_bytes(n_layers)
 * bytes, [layer][MD_LORA_MAX_VARIANTS][pair] of (A, B) device pointers, written by md_lora_bank_set_variant; a NULL entry (a
 * pair missing in that layer) adds nothing.  A variant's pairs are md_lora_pair of md_linear with a [rank][in] (n_pad = the
 * packed rank, k = k_pad = in) and b [out][rank] (k_pad = the packed rank); the padding rows / columns are zero. */
#define MD_LORA_MAX_VARIANTS 16
#define MD_LORA_MAX_RANK 256
#define MD_LORA_QKV 1   /* pair bits of md_lora_shrink_grouped */
#define MD_LORA_PROJ 2
#define MD_LORA_FC1 4
#define MD_LORA_FC2 8
#define MD_LORA_ADD 0   /* md_lora_expand_grouped: out = bf16(bf16(out) + bf16(delta)), then gelu on columns >= gelu_from */
#define MD_LORA_DELTA 1 /*                         out = bf16(delta) (0 for rows without the pair) */
typedef struct {
  int32_t n_variants;
  int32_t n_layers;
  int32_t rank[MD_LORA_MAX_VARIANTS][4];
  void* table;
} md_lora_bank;

size_t md_lora_bank_table_bytes(int32_t n_layers);
/* An empty bank over `table` (zeroed here; host call, synchronous). */
md_status md_lora_bank_init(md_lora_bank* bank, int32_t n_layers, void* table, size_t table_bytes);
/* Variant `index` (<= n_variants: replace one or append) from a host array of m->n_layers md_text_block_lora.  Checks the
 * shapes against m; a rank above MD_LORA_MAX_RANK: MD_ERR_UNSUPPORTED.  Host call, synchronous (copies into the table). */
md_status md_lora_bank_set_variant(md_lora_bank* bank, const md_text_model* m, int32_t index, const md_text_block_lora* lora);

/* Kernel-level entry points.  Shrink: t[row] = the concatenation, in pair order, of bf16(x[row] A_p^T) over the pairs p set in
 * `pairs`, for the row's variant (a variant lacking a pair has no columns for it); x [batch * q_len][ldx] with k columns
 * (k % 32 == 0).  Expand: for the pair `pair` of a t shrunk with `t_pairs`, out[row, :n] as MD_LORA_ADD / MD_LORA_DELTA says
 * (n % 16 == 0; gelu_from < 0 or >= n: no GELU).  Rows of the base model: ADD leaves out (GELU still applies), DELTA writes 0. */
md_status md_lora_shrink_grouped(const md_lora_bank* bank, int32_t layer, int32_t pairs, const int32_t* variant, int32_t batch,
                                 int32_t q_len, const void* x, int64_t ldx, int32_t k, void* t, int64_t ldt, void* stream);
md_status md_lora_expand_grouped(const md_lora_bank* bank, int32_t layer, int32_t pair, int32_t t_pairs, const int32_t* variant,
                                 int32_t batch, int32_t q_len, const void* t, int64_t ldt, void* out, int64_t ldo, int32_t n,
                                 int32_t flags, int32_t gelu_from, void* stream);

/* md_text_forward_slots with per-sequence variants.  bank == NULL: exactly md_text_forward_slots.  Per layer, four launches
 * beyond the base path: one shrink from l_in for qkv, proj and fc1 together, one expand adding the qkv and fc1 deltas (and
 * GELU, which the fused qkv|fc1 GEMM then leaves out), the fc2 shrink, and one expand of the proj and fc2 deltas, which
 * the fused block tail adds.  fp8 weight copies (m->fp8, m->f8) and the e4m3 KV copy: MD_ERR_UNSUPPORTED.  No host sync;
 * capturable.  Workspace: md_text_multi_lora_workspace_bytes. */
size_t md_text_multi_lora_workspace_bytes(const md_text_model* m, const md_lora_bank* bank, int32_t batch, int32_t q_len);
md_status md_text_forward_multi_lora(const md_text_model* m, const md_lora_bank* bank, const int32_t* variant, const void* x,
                                     void* hidden, int32_t batch, int32_t q_len, const int32_t* pos0, const int32_t* slots,
                                     int32_t n_slots, const md_kv_cache* kv, void* workspace, size_t workspace_bytes, void* stream);
/* md_decode_step_slots over md_text_forward_multi_lora (bank == NULL: exactly md_decode_step_slots).
 * Workspace: md_decode_multi_lora_workspace_bytes. */
size_t md_decode_multi_lora_workspace_bytes(const md_text_model* m, const md_lora_bank* bank, int32_t batch);
md_status md_decode_step_multi_lora(const md_text_model* m, const md_lora_bank* bank, const int32_t* variant, const int32_t* tokens,
                                    int32_t* next, int32_t* pos, int32_t batch, const int32_t* slots, int32_t n_slots,
                                    const md_kv_cache* kv, int32_t suppress_id, void* logits, int64_t ld_logits, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * Reasoning queries in lockstep                                       *
 * ------------------------------------------------------------------ */

/* query(image, question, reasoning=True) (reference: moondream.py:541-618 over :323-432 and :434-539) for B rows as ONE
 * lockstep decode loop with a phase per row.  With a one-token query suffix the reference's suffix pass (:604) is an
 * ordinary decode step that feeds the suffix token, so a row is, step by step:
 *   REASON  feeds the picked token -- or, after a coordinate token, the coordinate encoder's output for the bin the
 *           coordinate decoder picks on the hidden state that predicted the token (moondream.py:377-389); the step's
 *           logits lose eos_id and size_id (:397-398);
 *   then ONE step that feeds suffix_id, nothing suppressed (the pick of a prompt pass, :313-318);
 *   ANSWER  feeds the picked token; the step's logits lose answer_id (:517);
 *   DONE    still travels in the lockstep, as finished rows of md_decode_step do.
 * The very first token of a row is picked by the caller from its prompt pass, nothing suppressed. */
enum { MD_REASON_PHASE_IDLE = -1, MD_REASON_PHASE_REASON = 0, MD_REASON_PHASE_ANSWER = 1, MD_REASON_PHASE_DONE = 2 };
enum { MD_REASON_KIND_NONE = 0, MD_REASON_KIND_REASON = 1, MD_REASON_KIND_SUFFIX = 2, MD_REASON_KIND_ANSWER = 3 };

/* The coordinate half of the region head (reference: region.py:32-57): decoder MLP, Fourier matrix, encoder, and the
 * bin -> value table md_region_pick_encode reads (bf16 [n_bins]: bin / n_bins). */
typedef struct {
  md_linear dec_fc1, dec_fc2; /* coordinate decoder MLP: dim -> inner -> n_bins */
  md_linear encoder;          /* coordinate encoder: 2 * half -> dim */
  const void* fourier_w;      /* bf16 [1][half] */
  const void* value_table;    /* bf16 [n_bins] */
  int32_t half;
  int32_t n_bins;
} md_region_coord;

/* A step's view of the rows' reasoning state: device arrays of `batch` entries (suppress: [batch][2]) and the ids. */
typedef struct {
  int32_t *phase, *n_reason, *n_answer; /* in / out: MD_REASON_PHASE_*, reasoning / answer tokens kept so far */
  int32_t *kind, *ground, *suppress;    /* out: MD_REASON_KIND_* of the consumed token, its coordinate bin or -1, the ids to mask */
  int32_t* coord_bin;                   /* the bin md_region_pick_encode wrote for the row (written by md_decode_step_reason) */
  void* hidden_prev;                    /* bf16 [batch][dim], in / out: the hidden state that predicted the consumed token */
  const int32_t* forced;                /* [batch] or NULL: a value >= 0 replaces the consumed token (teacher forcing) */
  int32_t max_reason, max_answer;
  int32_t answer_id, eos_id, size_id, coord_id, suffix_id;
} md_reason_state;

/* The input stage of a step, one workgroup per row.  t = forced[b] if forced != NULL and forced[b] >= 0, else tokens[b].
 *   phase REASON, t == answer_id or n_reason[b] >= max_reason:  phase = ANSWER, kind = SUFFIX, x = wte[suffix_id],
 *       suppress = {-1, -1}, ground = -1  (t is fed nowhere and kept nowhere);
 *   phase REASON otherwise:  kind = REASON, n_reason[b] += 1, suppress = {eos_id, size_id};  t == coord_id: x = coord_emb[b],
 *       ground = coord_bin[b];  else x = wte[t], ground = -1;
 *   phase ANSWER, t == eos_id or n_answer[b] >= max_answer:  phase = DONE, kind = NONE, x = wte[t], suppress = {-1, -1};
 *   phase ANSWER otherwise:  kind = ANSWER, n_answer[b] += 1, x = wte[t], suppress = {answer_id, -1};
 *   phase DONE:  kind = NONE, x = wte[t], suppress = {-1, -1};
 *   phase < 0 (idle):  nothing of the row is read or written -- kind, ground, suppress and x keep the caller's contents.
 * x rows are bit copies of the table row or of coord_emb[b]; a t outside [0, vocab) copies row 0 (never an index out of
 * range).  hidden_prev is not used here.  dim % 8 == 0; wte, coord_emb, x 16-byte aligned with leading dimensions
 * (elements) that are multiples of 8.  No host sync, no allocation: capturable.  MD_ERR_INVALID_ARG: a NULL pointer
 * (forced excepted), batch / vocab / dim <= 0, a negative budget, suffix_id outside [0, vocab), a bad stride. */
md_status md_reason_route(const md_reason_state* st, const int32_t* tokens, const void* wte, int64_t ld_wte, int32_t vocab,
                          const void* coord_emb, int64_t ld_coord, void* x, int64_t ldx, int32_t batch, int32_t dim,
                          void* stream);

/* logits[b][ids[b][k]] = bf16 -inf for k = 0, 1 and every ids[b][k] in [0, vocab) (ids: device int32 [batch][2]).  No other
 * bit of the row changes; a negative id masks nothing, a row with both ids negative is untouched, equal ids are one
 * write.  The pick then runs with suppress_id = -1 (md_sample_rows: a greedy row takes its argmax).  Capturable.
 * MD_ERR_INVALID_ARG: NULL logits / ids, batch <= 0, vocab <= 0, ld < vocab. */
md_status md_mask_logits_rows(void* logits, int64_t ld, int32_t batch, int32_t vocab, const int32_t* ids, void* stream);

/* One reasoning step for the whole batch, device resident; the rows are routed as md_decode_step_shared routes them
 * (slots == NULL: row b in slot b; prefix_slots == NULL: no shared prefix).  In launch order:
 *   1. coordinate decoder MLP on st->hidden_prev for ALL rows (there is no skipping it without a host decision), as
 *      decode-regime GEMMs over blocks of <= 64 rows: a row's bits do not depend on the batch;
 *   2. md_region_pick_encode -> st->coord_bin;  3. coordinate encoder -> coord_emb;
 *   4. md_reason_route(st, tokens) -> x;  5. the decoder at pos[b] (q_len 1);  6. the step's hidden -> st->hidden_prev;
 *   7. md_lm_head -> logits [batch][ld_logits];  8. md_mask_logits_rows(st->suppress);  pos[b] += 1 for every row.
 * The pick from the masked logits is the caller's launch (md_sample_rows with suppress_id -1).  An idle row
 * (phase < 0) should carry an idle slot and suppress = {-1, -1}.  bank != NULL (mixed LoRA variants): MD_ERR_UNSUPPORTED.
 * Argument errors are reported before any launch: NULL pointers / batch <= 0 / negative budgets / ld_logits < vocab
 * MD_ERR_INVALID_ARG; a region head whose shapes do not chain onto the model's (dec_fc1.k_pad == dim, dec_fc2.k_pad ==
 * dec_fc1.n_pad, dec_fc2.n == n_bins, encoder.k_pad == 2 * half, encoder.n == encoder.n_pad == dim) MD_ERR_UNSUPPORTED;
 * workspace below md_decode_reason_workspace_bytes MD_ERR_WORKSPACE. */
size_t md_decode_reason_workspace_bytes(const md_text_model* m, const md_region_coord* rc, int32_t batch);
md_status md_decode_step_reason(const md_text_model* m, const md_region_coord* rc, const md_reason_state* st,
                                const md_lora_bank* bank, const int32_t* tokens, int32_t* pos, int32_t batch,
                                const int32_t* slots, int32_t n_slots, const int32_t* prefix_slots, const int32_t* prefix_len,
                                const md_kv_cache* kv, void* logits, int64_t ld_logits, void* workspace, size_t workspace_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOONDREAM_HIP_H */
