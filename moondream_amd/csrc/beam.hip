// Beam search on the device (include/moondream_hip.h: md_beam_select, md_kv_copy_tail): the group phase of the choice --
// merge of the beams' ranked candidates, the walk that feeds the pool of finished hypotheses and picks the next beams, the
// done rule and the KV slot hand-off -- and the copy that moves a surviving beam's KV tail to its child's slot.  The row
// phase (every beam's 2W best continuations) is md_topk_logprobs' device function, launched from logprobs.hip.
#include "text_internal.hpp"

namespace {

constexpr int BEAM_CAND = 2 * MD_BEAM_MAX;  // candidates per beam: MD_TOPK_MAX
static_assert(BEAM_CAND <= MD_TOPK_MAX, "a beam's 2W candidates are one md_topk_logprobs row");

struct BeamGroup {
  md_beam_state st;
  int W, beams_in, eos_id, early;
  int32_t *tokens_out, *parent, *src, *dst, *from, *to;
};

// One wave per group.  Every array the walk reads is staged in LDS first (<= 16 x 32 candidates, 16 pool entries); lane 0
// walks -- at most 2W steps of a W-way merge over lists that are already in rank order, the order of the header: s
// descending, beam ascending, entry ascending -- and lanes 0 .. W-1 write the rows' results.  The group's cum and cur are
// in LDS before any of them is rewritten.
__global__ __launch_bounds__(64) void beam_group_kernel(BeamGroup a) {
  __shared__ float c_s[MD_BEAM_MAX * BEAM_CAND];
  __shared__ int c_id[MD_BEAM_MAX * BEAM_CAND];
  __shared__ float cum_s[MD_BEAM_MAX], p_h[MD_BEAM_MAX], p_s[MD_BEAM_MAX], ch_s[MD_BEAM_MAX];
  __shared__ int cur_s[MD_BEAM_MAX], p_par[MD_BEAM_MAX], p_step[MD_BEAM_MAX], ch_tok[MD_BEAM_MAX], ch_par[MD_BEAM_MAX];
  __shared__ int head[MD_BEAM_MAX];
  __shared__ int n_live_s, pool_n_s, done_s;
  const int g = blockIdx.x, lane = threadIdx.x;
  const md_beam_state& st = a.st;
  if (st.done[g] != 0) return;  // the whole wave: nothing of a done group is read or written
  const int W = a.W, K = 2 * W, row0 = g * W;
  const int L = st.len[g], P = st.prefix_len[g];
  if (lane < W) {
    cum_s[lane] = lane < a.beams_in ? st.cum[row0 + lane] : -INFINITY;
    cur_s[lane] = st.cur[row0 + lane];
    p_h[lane] = st.pool_score[row0 + lane];
    p_s[lane] = st.pool_sum[row0 + lane];
    p_par[lane] = st.pool_parent[row0 + lane];
    p_step[lane] = st.pool_step[row0 + lane];
    head[lane] = 0;
  }
  __syncthreads();
  for (int e = lane; e < W * K; e += 64) {
    const int j = e / K, i = e - j * K;
    const float cum = cum_s[j];
    int id = -1;
    float s = -INFINITY;
    if (cum != -INFINITY) {  // a dead beam's entries are not read
      id = st.cand_ids[(int64_t)row0 * K + e];
      s = cum + st.cand_lp[(int64_t)row0 * K + e];  // the one fp32 add
    }
    c_id[j * BEAM_CAND + i] = id;
    c_s[j * BEAM_CAND + i] = s;
  }
  __syncthreads();
  if (lane == 0) {
    int n_live = 0, pn = min(max(st.pool_n[g], 0), W);
    const float norm1 = st.inv_norm[min(L + 1, st.n_norm - 1)];
    for (int w = 0; w < K && n_live < W; ++w) {  // (once W beams are chosen every later candidate has w >= W: dropped or unused)
      int best = -1;
      float bs = 0.f;
      for (int j = 0; j < W; ++j) {
        const int i = head[j];
        if (i >= K || c_id[j * BEAM_CAND + i] < 0) continue;  // the list's end: ids are -1 from there on
        const float s = c_s[j * BEAM_CAND + i];
        if (best < 0 || s > bs) {  // strictly greater: equal scores go to the lower beam
          best = j;
          bs = s;
        }
      }
      if (best < 0) break;  // fewer than 2W candidates exist
      const int tok = c_id[best * BEAM_CAND + head[best]];
      head[best] += 1;
      if (a.eos_id >= 0 && tok == a.eos_id) {
        if (w >= W) continue;  // the HF rule
        const float h = bs * norm1;
        int at = pn;
        if (pn == W) {  // full: the lowest score, among equal ones the highest index, and only a strictly better h
          at = 0;
          for (int q = 1; q < W; ++q)
            if (p_h[q] <= p_h[at]) at = q;
          if (!(h > p_h[at])) continue;
        } else {
          pn += 1;
        }
        p_h[at] = h;
        p_s[at] = bs;
        p_par[at] = best;
        p_step[at] = L;
        continue;
      }
      ch_tok[n_live] = tok;
      ch_par[n_live] = best;
      ch_s[n_live] = bs;
      n_live += 1;
    }
    int done = n_live == 0;
    if (!done && pn == W) {
      float lowest = p_h[0];
      for (int q = 1; q < W; ++q) lowest = fminf(lowest, p_h[q]);
      done = a.early || ch_s[0] * st.inv_norm[min(L + 1, st.n_norm - 1)] <= lowest;
    }
    n_live_s = n_live;
    pool_n_s = pn;
    done_s = done;
    st.len[g] = L + 1;
    st.pool_n[g] = pn;
    st.done[g] = done;
  }
  __syncthreads();
  if (lane < W) {
    const int n = lane, r = row0 + n;
    st.pool_score[r] = p_h[n];
    st.pool_sum[r] = p_s[n];
    st.pool_parent[r] = p_par[n];
    st.pool_step[r] = p_step[n];
    const bool live = n < n_live_s;
    a.tokens_out[r] = live ? ch_tok[n] : 0;
    a.parent[r] = live ? ch_par[n] : -1;
    st.cum[r] = live ? ch_s[n] : -INFINITY;
    int cur = -1, src = -1, dst = -1;
    if (live && !done_s) {
      const int p = ch_par[n], mine = cur_s[n];
      if (p == n && mine >= 0) {
        cur = src = dst = mine;  // the beam goes on in its own slot: a skipped copy
      } else {
        const int o0 = st.own[2 * r], o1 = st.own[2 * r + 1];
        cur = dst = (mine == o0) ? o1 : o0;  // never any row's current slot
        src = cur_s[p];
      }
    }
    st.cur[r] = cur;
    a.src[r] = src;
    a.dst[r] = dst;
    a.from[r] = P;
    a.to[r] = P + L;
  }
}

// One workgroup per (row, layer): the K and the V runs of all its heads, 2 * n_heads runs of (to - from) * 8 pieces of 16
// bytes, as one index space over the workgroup -- piece c is piece c % n of run c / n, run 2h the keys and run 2h + 1 the
// values of head h.  A lane issues up to four loads before their stores.  The grid is n_layers x rows (1536 workgroups at
// 2B with 64 rows, under the ~2048 a memory-bound grid should stay below), not one workgroup per head: most rows of a
// step are skipped copies, and a skipped workgroup costs its launch slot and four loads for nothing.
__global__ __launch_bounds__(256) void kv_copy_tail_kernel(bf16_t* __restrict__ k, bf16_t* __restrict__ v, int64_t layer_stride,
                                                           int64_t batch_stride, int ctx, int n_slots, int n_heads,
                                                           const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                           const int32_t* __restrict__ from, const int32_t* __restrict__ to) {
  const int l = blockIdx.x, r = blockIdx.y;
  const int s = src[r], d = dst[r], p0 = from[r], p1 = to[r];
  if (d < 0 || s < 0 || s == d || p1 <= p0) return;                  // the row is skipped
  if (s >= n_slots || d >= n_slots || p0 < 0 || p1 > ctx) return;     // never an address outside the slabs
  const int n = (p1 - p0) * 8;  // 16-byte pieces per run
  const int total = 2 * n_heads * n;
  const int64_t at = (int64_t)l * layer_stride + (int64_t)p0 * 64;
  const int64_t from_slot = at + (int64_t)s * batch_stride, to_slot = at + (int64_t)d * batch_stride;
  // piece c -> the slab and the element offset inside a slot (the same for source and destination)
  auto place = [&](int c, bool& is_v) -> int64_t {
    const int run = c / n, piece = c - run * n;
    is_v = run & 1;
    return (int64_t)(run >> 1) * ctx * 64 + (int64_t)piece * 8;
  };
  for (int c0 = threadIdx.x; c0 < total; c0 += 4 * 256) {
    u32x4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u * 256;
      if (c < total) {
        bool is_v;
        const int64_t off = place(c, is_v);
        x[u] = *(const u32x4*)((is_v ? v : k) + from_slot + off);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u * 256;
      if (c < total) {
        bool is_v;
        const int64_t off = place(c, is_v);
        *(u32x4*)((is_v ? v : k) + to_slot + off) = x[u];
      }
    }
  }
}
}  // namespace

extern "C" md_status md_kv_copy_tail(const md_kv_cache* kv, int32_t n_layers, int32_t n_heads, int32_t n_slots, int32_t rows,
                                     const int32_t* src, const int32_t* dst, const int32_t* from, const int32_t* to, void* stream) {
  MD_CHECK_ARG(kv && kv->k && kv->v && src && dst && from && to && rows >= 0 && n_layers >= 1 && n_heads >= 1 && n_slots > 0);
  MD_CHECK_ARG(kv->k8 == nullptr && kv->v8 == nullptr);  // the e4m3 copy would go stale: not served
  MD_CHECK_ARG(kv->ctx > 0 && ((uintptr_t)kv->k % 16) == 0 && ((uintptr_t)kv->v % 16) == 0 && kv->layer_stride % 8 == 0 &&
               kv->batch_stride % 8 == 0);
  MD_CHECK_ARG(kv->batch_stride >= (int64_t)n_heads * kv->ctx * 64 && (int64_t)n_slots * kv->batch_stride <= kv->layer_stride);
  MD_CHECK_ARG(rows <= 65535 && (int64_t)n_heads * kv->ctx * 16 <= 0x7fffffff);  // grid y; the piece index is an int
  if (rows == 0) return MD_OK;
  hipLaunchKernelGGL(kv_copy_tail_kernel, dim3(n_layers, rows), dim3(256), 0, (hipStream_t)stream, (bf16_t*)kv->k,
                     (bf16_t*)kv->v, kv->layer_stride, kv->batch_stride, kv->ctx, n_slots, n_heads, src, dst, from, to);
  return md_launch_status();
}

extern "C" md_status md_beam_select(const void* logits, int64_t ld, int32_t groups, int32_t num_beams, int32_t beams_in,
                                    int32_t vocab, int32_t suppress_id, const int32_t* suppress_rows, int32_t eos_id,
                                    int32_t early_stopping, const md_beam_state* st, int32_t* tokens_out, int32_t* parent,
                                    int32_t* src, int32_t* dst, int32_t* from, int32_t* to, void* stream) {
  MD_CHECK_ARG(logits && st && tokens_out && parent && src && dst && from && to);
  MD_CHECK_ARG(st->cum && st->cur && st->own && st->len && st->done && st->prefix_len && st->pool_n && st->pool_score &&
               st->pool_sum && st->pool_parent && st->pool_step && st->inv_norm && st->cand_ids && st->cand_lp);
  MD_CHECK_ARG(groups >= 0 && num_beams >= 1 && num_beams <= MD_BEAM_MAX && (beams_in == 1 || beams_in == num_beams));
  MD_CHECK_ARG(vocab >= 1 && ld >= vocab && st->n_norm >= 1 && (early_stopping == 0 || early_stopping == 1));
  MD_CHECK_ARG((int64_t)groups * num_beams <= 0x7fffffff / (2 * MD_BEAM_MAX));
  if (groups == 0) return MD_OK;
  hipStream_t s = (hipStream_t)stream;
  MD_TRY(md_beam_rows(logits, ld, groups * num_beams, vocab, suppress_id, suppress_rows, num_beams, beams_in, st->cum, st->done,
                      st->cand_ids, st->cand_lp, s));
  BeamGroup a{*st, num_beams, beams_in, eos_id, early_stopping, tokens_out, parent, src, dst, from, to};
  hipLaunchKernelGGL(beam_group_kernel, dim3(groups), dim3(64), 0, s, a);
  return md_launch_status();
}
