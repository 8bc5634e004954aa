// What a decode step does to its rows between the logits and the pick, one launch each, one workgroup per row:
//   * the reasoning query's per-row control flow and next embedding (md_reason_route);
//   * the ids a row's logits lose to -inf (md_mask_logits_rows; md_mask_logits_advance also bumps pos);
//   * repetition / presence / frequency penalties from the row's history (md_penalize_rows);
//   * the token automaton of constrained decoding, advanced and applied as a mask (md_constrain_rows).
// These kernels write logits and per-sequence state in place; none of them picks a token.
#include "row_reduce.hpp"
#include "text_internal.hpp"

namespace {

// ---------------------------------------------------------------------------
// The reasoning query's control flow, per row, on the device (reference: moondream.py:323-432 then :434-539 after the
// suffix pass of :604): which embedding the row feeds to this decode step, which ids the step's logits lose before the
// pick, and when the row moves from reasoning to answering to done.  One workgroup per row; the row's state is a few
// words that every wave reads BEFORE thread 0 rewrites them (the barrier), the embedding is a 16-byte-chunk copy.
struct ReasonRoute {
  const int32_t *tokens, *forced, *coord_bin;
  int32_t *phase, *n_reason, *n_answer, *kind, *ground, *suppress;
  int max_reason, max_answer, answer_id, eos_id, size_id, coord_id, suffix_id, vocab;
  const bf16_t *wte, *coord_emb;
  int64_t ld_wte, ld_coord, ldx;
  bf16_t* x;
  int dim;
};

__global__ __launch_bounds__(256) void reason_route_kernel(ReasonRoute a) {
  const int b = blockIdx.x;
  const int ph = a.phase[b];
  if (ph < 0) return;  // idle: taken by the whole workgroup, before the barrier; nothing of the row is read or written
  int t = a.tokens[b];
  if (a.forced) {
    const int f = a.forced[b];
    if (f >= 0) t = f;
  }
  const int nr = a.n_reason[b], na = a.n_answer[b];
  __syncthreads();
  int nph = ph, kind = MD_REASON_KIND_NONE, ground = -1, s0 = -1, s1 = -1, src = t, nr2 = nr, na2 = na;
  bool from_coord = false;
  if (ph == MD_REASON_PHASE_REASON) {
    if (t == a.answer_id || nr >= a.max_reason) {  // the loop of moondream.py:357 ends; the suffix pass (:604) is this step
      nph = MD_REASON_PHASE_ANSWER;
      kind = MD_REASON_KIND_SUFFIX;
      src = a.suffix_id;
    } else {
      kind = MD_REASON_KIND_REASON;
      nr2 = nr + 1;
      s0 = a.eos_id;  // moondream.py:397-398
      s1 = a.size_id;
      if (t == a.coord_id) {
        from_coord = true;
        ground = a.coord_bin[b];
      }
    }
  } else if (ph == MD_REASON_PHASE_ANSWER) {
    if (t == a.eos_id || na >= a.max_answer) {
      nph = MD_REASON_PHASE_DONE;
    } else {
      kind = MD_REASON_KIND_ANSWER;
      na2 = na + 1;
      s0 = a.answer_id;  // moondream.py:517
    }
  }
  if (src < 0 || src >= a.vocab) src = 0;  // never a table index out of range (a finished row's token is whatever was picked)
  const u32x4* from = (const u32x4*)(from_coord ? a.coord_emb + (int64_t)b * a.ld_coord : a.wte + (int64_t)src * a.ld_wte);
  u32x4* to = (u32x4*)(a.x + (int64_t)b * a.ldx);
  for (int ch = threadIdx.x; ch < (a.dim >> 3); ch += 256) to[ch] = from[ch];
  if (threadIdx.x == 0) {
    a.phase[b] = nph;
    a.n_reason[b] = nr2;
    a.n_answer[b] = na2;
    a.kind[b] = kind;
    a.ground[b] = ground;
    a.suppress[2 * b] = s0;
    a.suppress[2 * b + 1] = s1;
  }
}

// logits[b][ids[b][k]] = -inf (bf16 0xff80) for the ids inside [0, vocab); optionally pos[b] += 1 (the step's advance)
__global__ __launch_bounds__(64) void mask_logits_rows_kernel(bf16_t* __restrict__ logits, int64_t ld, int vocab,
                                                              const int32_t* __restrict__ ids, int32_t* __restrict__ pos_inc) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k < 2) {
    const int id = ids[2 * b + k];
    if (id >= 0 && id < vocab) logits[(int64_t)b * ld + id] = (bf16_t)0xff80;
  }
  if (k == 2 && pos_inc) pos_inc[b] += 1;
}

// ---------------------------------------------------------------------------
// Repetition / presence / frequency penalties from each row's own history of generated tokens (md_penalize_rows).
// One workgroup per row.  The row's token is appended to its history, then every DISTINCT token of the history is found
// once, with its count, through an open-addressing hash table in LDS: each thread inserts its strided share of the
// history (atomicCAS claims a key, atomicAdd counts it), and after a barrier each occupied entry is one token's update.
// The table has at least twice as many entries as the history has tokens (a power of two chosen from the row's length, so
// the clear and the scan cost what the history holds, not what it could hold): a probe sequence always ends.
// Global traffic: the history's tokens (4 B each) and one 2-byte load and store per distinct token -- never the row.
constexpr int PENALTY_THREADS = 256;

__device__ __forceinline__ unsigned penalty_hash(int t, int bits) { return ((unsigned)t * 2654435761u) >> (32 - bits); }

__global__ __launch_bounds__(PENALTY_THREADS) void penalize_rows_kernel(
    bf16_t* __restrict__ logits, int64_t ld, int vocab, const int32_t* __restrict__ tokens_in, const int32_t* __restrict__ slots,
    int slot0, int32_t* hist, int hist_cap, int32_t* __restrict__ hist_len, const float* __restrict__ repetition,
    const float* __restrict__ presence, const float* __restrict__ frequency, int table_cap) {
  extern __shared__ int penalty_smem[];
  __shared__ int s_len;
  int* keys = penalty_smem;            // [table_cap] token id, -1: empty
  int* counts = penalty_smem + table_cap;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int slot = state_slot(slots, slot0, r);
  if (slot < 0) return;  // idle: nothing read, nothing written (the whole workgroup leaves, before any barrier)
  int32_t* h = hist + (int64_t)slot * hist_cap;
  // ---- append: one thread owns the history's length
  if (tid == 0) {
    int len = min(max(hist_len[slot], 0), hist_cap);
    const int t = tokens_in[r];
    if (t >= 0 && t < vocab && len < hist_cap) {
      h[len] = t;
      hist_len[slot] = ++len;
    }
    s_len = len;
  }
  const float rep = repetition[r], pres = presence[r], freq = frequency[r];
  if (rep == 1.f && pres == 0.f && freq == 0.f) return;  // neutral: the logits row is neither read nor written
  __syncthreads();  // s_len; thread 0's store to h[len - 1] is visible to the workgroup after it too
  const int len = s_len;
  if (len == 0) return;
  int bits = 6;
  while ((1 << bits) < 2 * len) ++bits;  // 2 * len <= 2 * hist_cap <= table_cap
  const int size = 1 << bits;
  for (int e = tid; e < size; e += PENALTY_THREADS) {
    keys[e] = -1;
    counts[e] = 0;
  }
  __syncthreads();
  for (int i = tid; i < len; i += PENALTY_THREADS) {
    const int t = h[i];
    if (t < 0 || t >= vocab) continue;  // not an id: the caller's memory was not a history; never an address
    unsigned e = penalty_hash(t, bits);
    for (int probe = 0; probe < size; ++probe) {  // load factor <= 1/2: ends long before `size` probes
      const int prev = atomicCAS(&keys[e], -1, t);
      if (prev == -1 || prev == t) {
        atomicAdd(&counts[e], 1);
        break;
      }
      e = (e + 1) & (size - 1);
    }
  }
  __syncthreads();
  bf16_t* lr = logits + (int64_t)r * ld;
  for (int e = tid; e < size; e += PENALTY_THREADS) {
    const int v = keys[e];
    if (v < 0) continue;
    float x = bf2f(lr[v]);
    if (rep != 1.f) x = x > 0.f ? __fdiv_rn(x, rep) : __fmul_rn(x, rep);
    x = __fsub_rn(x, __fadd_rn(pres, __fmul_rn(freq, (float)counts[e])));
    lr[v] = f2bf(x);
  }
}

// ---------------------------------------------------------------------------
// Constrained decoding: a deterministic automaton over token ids per row, advanced by the token the row consumed and
// applied to the logits it picks from next (md_constrain_rows).  One workgroup per row.  Every thread reads the row's
// state and walks the same (wave-uniform) binary search over the state's sorted edges, so nothing is broadcast; after a
// barrier thread 0 stores the new state.  The mask only STORES bf16 -inf: the row is never loaded.
//   default-allow state: one 2-byte store per listed forbidden token.
//   default-forbid state: the edges that allow a token set its bit in a vocab-bit map in LDS; the sweep then walks the
//     row in 16-byte groups aligned in MEMORY (the row may start anywhere: no ld % 8 requirement), one 16-byte store
//     for a whole group without an allowed token, 2-byte stores in a group that has one and in the clipped groups at the
//     row's two ends.
constexpr int CONSTRAIN_THREADS = 256;
constexpr bf16_t BF16_NEG_INF = 0xFF80;

__global__ __launch_bounds__(CONSTRAIN_THREADS) void constrain_rows_kernel(
    bf16_t* __restrict__ logits, int64_t ld, int vocab, const int32_t* __restrict__ tokens_in, const int32_t* __restrict__ slots,
    int slot0, int32_t* state, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ default_next,
    const int32_t* __restrict__ edge_tok, const int32_t* __restrict__ edge_next, int state_cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned constrain_allowed[];  // [ceil(vocab / 32)] bit v: token v allowed
  const int r = blockIdx.x, tid = threadIdx.x;
  const int slot = state_slot(slots, slot0, r);
  if (slot < 0) return;  // idle: nothing read, nothing written (the whole workgroup leaves, before any barrier)
  int q = state[slot];
  if (q < 0) return;  // FREE or DEAD: the row is left alone
  __syncthreads();    // every thread has read the state before thread 0 replaces it
  if (q >= state_cap) {  // no state of this table: never an index
    if (tid == 0) state[slot] = MD_CONSTRAINT_DEAD;
    return;
  }
  if (tokens_in) {  // ---- advance by the token the row consumed
    const int t = tokens_in[r];
    int nxt = default_next[q];
    int lo = row_ptr[q], hi = row_ptr[q + 1];
    while (lo < hi) {  // the first edge whose token is >= t
      const int mid = (lo + hi) >> 1;
      if (edge_tok[mid] < t) lo = mid + 1; else hi = mid;
    }
    if (lo < row_ptr[q + 1] && edge_tok[lo] == t) nxt = edge_next[lo];
    // a token that is no id, a forbidden one, or a next value that is no state of this table: the row is dead
    if (t < 0 || t >= vocab || nxt == MD_CONSTRAINT_FORBID || nxt >= state_cap || nxt < MD_CONSTRAINT_FORBID) nxt = MD_CONSTRAINT_DEAD;
    q = nxt;
    if (tid == 0) state[slot] = q;
    if (q < 0) return;
  }
  // ---- mask the row for state q
  bf16_t* lr = logits + (int64_t)r * ld;
  const int e0 = row_ptr[q], e1 = row_ptr[q + 1];
  if (default_next[q] != MD_CONSTRAINT_FORBID) {
    for (int e = e0 + tid; e < e1; e += CONSTRAIN_THREADS) {
      const int v = edge_tok[e];
      if (edge_next[e] == MD_CONSTRAINT_FORBID && v >= 0 && v < vocab) lr[v] = BF16_NEG_INF;
    }
    return;
  }
  const int words = (vocab + 31) >> 5;
  for (int w = tid; w < words; w += CONSTRAIN_THREADS) constrain_allowed[w] = 0u;
  __syncthreads();
  for (int e = e0 + tid; e < e1; e += CONSTRAIN_THREADS) {
    const int v = edge_tok[e];
    if (edge_next[e] != MD_CONSTRAINT_FORBID && v >= 0 && v < vocab) atomicOr(&constrain_allowed[v >> 5], 1u << (v & 31));
  }
  __syncthreads();
  // group g covers the elements [8 g - a, 8 g - a + 8) of the row, a = the row's offset (in elements) into its 16-byte line
  const int a = (int)(((uintptr_t)lr >> 1) & 7);
  const int groups = (vocab + a + 7) >> 3;
  const uint4 wide = make_uint4(0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u);
  for (int g = tid; g < groups; g += CONSTRAIN_THREADS) {
    const int v0 = 8 * g - a;
    if (v0 >= 0 && v0 + 8 <= vocab) {
      const int w = v0 >> 5, sh = v0 & 31;
      unsigned bits = constrain_allowed[w] >> sh;
      if (sh > 24) bits |= constrain_allowed[w + 1] << (32 - sh);  // (v0 + 7 < vocab: word w + 1 exists)
      bits &= 0xFFu;
      if (bits == 0u) {
        *reinterpret_cast<uint4*>(lr + v0) = wide;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!((bits >> j) & 1u)) lr[v0 + j] = BF16_NEG_INF;
      }
    } else {  // clipped at one of the row's ends
      for (int v = max(v0, 0); v < min(v0 + 8, vocab); ++v)
        if (!((constrain_allowed[v >> 5] >> (v & 31)) & 1u)) lr[v] = BF16_NEG_INF;
    }
  }
}

}  // namespace

extern "C" md_status md_reason_route(const md_reason_state* st, const int32_t* tokens, const void* wte, int64_t ld_wte,
                                     int32_t vocab, const void* coord_emb, int64_t ld_coord, void* x, int64_t ldx,
                                     int32_t batch, int32_t dim, void* stream) {
  MD_CHECK_ARG(st && tokens && wte && coord_emb && x && batch > 0 && vocab > 0 && dim > 0 && dim % 8 == 0);
  MD_CHECK_ARG(st->phase && st->n_reason && st->n_answer && st->kind && st->ground && st->suppress && st->coord_bin);
  MD_CHECK_ARG(st->max_reason >= 0 && st->max_answer >= 0 && st->suffix_id >= 0 && st->suffix_id < vocab);
  MD_CHECK_ARG(ld_wte >= dim && ld_coord >= dim && ldx >= dim && ld_wte % 8 == 0 && ld_coord % 8 == 0 && ldx % 8 == 0);
  MD_CHECK_ARG((((uintptr_t)wte | (uintptr_t)coord_emb | (uintptr_t)x) & 15) == 0);
  ReasonRoute a;
  a.tokens = tokens; a.forced = st->forced; a.coord_bin = st->coord_bin;
  a.phase = st->phase; a.n_reason = st->n_reason; a.n_answer = st->n_answer; a.kind = st->kind; a.ground = st->ground;
  a.suppress = st->suppress;
  a.max_reason = st->max_reason; a.max_answer = st->max_answer; a.answer_id = st->answer_id; a.eos_id = st->eos_id;
  a.size_id = st->size_id; a.coord_id = st->coord_id; a.suffix_id = st->suffix_id; a.vocab = vocab;
  a.wte = (const bf16_t*)wte; a.coord_emb = (const bf16_t*)coord_emb; a.ld_wte = ld_wte; a.ld_coord = ld_coord; a.ldx = ldx;
  a.x = (bf16_t*)x; a.dim = dim;
  hipLaunchKernelGGL(reason_route_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, a);
  return md_launch_status();
}

// internal (api.hip): the mask that also advances pos
md_status md_mask_logits_advance(void* logits, int64_t ld, int32_t batch, int32_t vocab, const int32_t* ids, int32_t* pos,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(mask_logits_rows_kernel, dim3(batch), dim3(64), 0, stream, (bf16_t*)logits, ld, vocab, ids, pos);
  return md_launch_status();
}

extern "C" md_status md_mask_logits_rows(void* logits, int64_t ld, int32_t batch, int32_t vocab, const int32_t* ids,
                                         void* stream) {
  MD_CHECK_ARG(logits && ids && batch > 0 && vocab > 0 && ld >= vocab);
  return md_mask_logits_advance(logits, ld, batch, vocab, ids, nullptr, (hipStream_t)stream);
}

extern "C" md_status md_penalize_rows(void* logits, int64_t ld, int32_t batch, int32_t vocab, const int32_t* tokens_in,
                                      const int32_t* slots, int32_t slot0, int32_t* hist, int32_t hist_cap, int32_t* hist_len,
                                      const float* repetition, const float* presence, const float* frequency, void* stream) {
  MD_CHECK_ARG(logits && tokens_in && hist && hist_len && repetition && presence && frequency);
  MD_CHECK_ARG(batch >= 0 && vocab >= 1 && ld >= vocab && hist_cap >= 1 && hist_cap <= MD_PENALTY_HIST_MAX);
  if (batch == 0) return MD_OK;
  int table_cap = 64;
  while (table_cap < 2 * hist_cap) table_cap *= 2;  // <= 2 * MD_PENALTY_HIST_MAX entries of 8 bytes: 64 KiB, the static limit
  hipLaunchKernelGGL(penalize_rows_kernel, dim3(batch), dim3(PENALTY_THREADS), (size_t)table_cap * 8, (hipStream_t)stream,
                     (bf16_t*)logits, ld, vocab, tokens_in, slots, slot0, hist, hist_cap, hist_len, repetition, presence,
                     frequency, table_cap);
  return md_launch_status();
}

extern "C" md_status md_constrain_rows(void* logits, int64_t ld, int32_t batch, int32_t vocab, const int32_t* tokens_in,
                                       const int32_t* slots, int32_t slot0, int32_t* state, const int32_t* row_ptr,
                                       const int32_t* default_next, const int32_t* edge_tok, const int32_t* edge_next,
                                       int32_t state_cap, void* stream) {
  MD_CHECK_ARG(logits && state && row_ptr && default_next && edge_tok && edge_next);
  MD_CHECK_ARG(batch >= 0 && vocab >= 1 && ld >= vocab && state_cap >= 1 && vocab <= MD_CONSTRAIN_VOCAB_MAX);
  if (batch == 0) return MD_OK;
  const size_t lds = (size_t)((vocab + 127) / 128) * 16;  // one bit per token, in whole 16-byte pieces: <= 32 KiB
  hipLaunchKernelGGL(constrain_rows_kernel, dim3(batch), dim3(CONSTRAIN_THREADS), lds, (hipStream_t)stream, (bf16_t*)logits, ld,
                     vocab, tokens_in, slots, slot0, state, row_ptr, default_next, edge_tok, edge_next, state_cap);
  return md_launch_status();
}
