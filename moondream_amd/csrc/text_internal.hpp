// Internal interface between api.hip and the translation units whose kernels it sequences (not part of the C ABI): the
// row map of a decoder call, the decode-attention descriptor, and the ONE declaration of every internal function that
// crosses a translation unit.  Every unit that defines one of them includes this header, so a signature that changes on
// one side only fails to compile.
#pragma once
#include "md_common.hpp"

// Where the rows of a decoder call live and which adapters they carry (moondream.py's _Rows, one level down).  Null is
// absent: no slot table = row b in slot b, no prefix tables = no shared prefix, no bank = the base weights.
struct RowMap {
  const int32_t* slots = nullptr;      // [batch]: row b's K / V are slot slots[b]; outside [0, n_slots) = idle decode row
  int32_t n_slots = 0;                 // slots the call may address
  const int32_t* pfx_slots = nullptr;  // [batch]: keys [0, pfx_len[b]) of row b are read from slot pfx_slots[b]
  const int32_t* pfx_len = nullptr;
  const md_lora_bank* bank = nullptr;  // mixed LoRA variants: variant[b] indexes the bank, -1 = base
  const int32_t* variant = nullptr;
  // the map of rows [b0, ...): every table that is present advances, n_slots stays.  Without a slot table the CALLER
  // moves the slab base by b0 slots instead (the contiguous case).
  RowMap block(int b0) const {
    RowMap r = *this;
    if (slots) r.slots += b0;
    if (pfx_slots) r.pfx_slots += b0;
    if (pfx_len) r.pfx_len += b0;
    if (variant) r.variant += b0;
    return r;
  }
};

// One decode attention (q_len 1) over a layer's slab.  fused: q is the un-rotated [q | k | v] activation row, and the
// kernel applies RoPE and writes the new K / V row itself (MHA only).  k8_slab / v8_slab: the optional e4m3 copy.
struct DecodeAttn {
  const void* q;
  int64_t ldq;
  void* o;
  int64_t ldo;
  const float* freqs;
  void *k_slab, *v_slab;
  void *k8_slab, *v8_slab;
  float k_scale, v_scale;
  int64_t slab_batch_stride;
  int32_t ctx;
  const int32_t* kv_len;
  int32_t batch, n_heads, n_kv_heads, head_dim, rot_dim;
  float scale;
  bool fused;
};

// attention.hip
md_status md_attention_decode_rows(const DecodeAttn& d, const RowMap& rows, hipStream_t stream);
// q_blk0, n_q_blks: the 128-row query blocks [q_blk0, q_blk0 + n_q_blks) only (n_q_blks < 0: all of them); a row of a block that
// runs sits in the workgroup and wave it has in the full launch
md_status md_attention_prefill_rows(const md_attn_args* a, const RowMap& rows, hipStream_t stream, int q_blk0 = 0, int n_q_blks = -1);
// attention_f8kv.hip
md_status md_attention_decode_f8_rows(const DecodeAttn& d, const RowMap& rows, hipStream_t stream);
md_status md_attention_decode_f8_shared_rows(const DecodeAttn& d, const RowMap& rows, hipStream_t stream);  // rows with a prefix table
md_status md_kv_quantize_f8_layer(const md_kv_cache* kv, int layer, const int32_t* pos0, int pos_fixed, int batch, int n_heads,
                                  int n_pos, const RowMap& rows, hipStream_t stream);
// elementwise.hip
md_status md_rope_kv_write_slots(void* qkv, int64_t ld, const float* freqs, const int32_t* pos0, void* k_slab, void* v_slab,
                                 int64_t slab_batch_stride, int32_t ctx, int32_t batch, int32_t q_len, int32_t n_heads,
                                 int32_t n_kv_heads, int32_t head_dim, int32_t rot_dim, const RowMap& rows, hipStream_t stream);
md_status md_reduce_residual_layernorm_add(void* x, int64_t ldx, const float* partial_a, int32_t slices_a, const void* bias_a,
                                           const float* partial_b, int32_t slices_b, const void* bias_b, int64_t ld_partial,
                                           int64_t slice_stride, void* y, int64_t ldy, const md_layernorm* ln, int32_t rows,
                                           int32_t dim, float eps, const void* da, const void* db, int64_t ldd, void* stream);
md_status md_argmax_advance(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id, int32_t* next,
                            int32_t* pos, hipStream_t stream);
md_status md_stitch_pool_batched(const void* feats, void* out, int64_t ld_out, int64_t out_img_stride, int32_t n_images,
                                 int32_t dim, int32_t grid, int32_t margin, int32_t tiles_h, int32_t tiles_w, hipStream_t stream);
md_status md_pool_grid_concat(const void* global_feats, const void* grid_feats, int32_t H, int32_t W, void* out, int64_t ld_out,
                              int32_t dim, int32_t grid, hipStream_t stream);
// logits_edit.hip: md_mask_logits_rows that also advances pos (pos == nullptr: the public form)
md_status md_mask_logits_advance(void* logits, int64_t ld, int32_t batch, int32_t vocab, const int32_t* ids, int32_t* pos,
                                 hipStream_t stream);
// logprobs.hip: the row phase of md_beam_select (csrc/beam.hip) -- md_topk_logprobs' entries, k = 2 * num_beams, for
// every live beam (the kernel that shares md_topk_logprobs' device function)
md_status md_beam_rows(const void* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t suppress_id,
                       const int32_t* suppress_rows, int32_t num_beams, int32_t beams_in, const float* cum, const int32_t* done,
                       int32_t* cand_ids, float* cand_lp, hipStream_t stream);
// lora_multi.hip
md_status lora_bank_ok(const md_lora_bank* bank);
int32_t md_lora_shrink_cols(const md_lora_bank* bank, int32_t pairs);
// decode_b1.hip: embedding lookup, every decoder block, final layer norm, lm_head, suppression, argmax and pos += 1 in ONE launch
md_status md_decode_b1_step(const md_text_model* m, const int32_t* token, int32_t* next, int32_t* pos, const md_kv_cache* kv,
                            int32_t suppress_id, void* logits, void* workspace, size_t workspace_bytes, void* sync_state,
                            hipStream_t s);
