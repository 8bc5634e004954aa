// Stop strings and stop token ids, matched on the device (md_stop_rows): one launch per decode step feeds every row's
// newly picked token to the row's matcher -- a membership test in its stop-id list, then a walk of the token's bytes
// through a complete byte-level Aho-Corasick DFA (moondream_amd/stop.py: goto and failure links folded into trans, so a
// byte costs one lookup whatever it is).  The first match is recorded once in the row's result triple and never again.
//
// Mapping: one THREAD per row, 64 rows (one wave) per workgroup.  A row's work is a chain of dependent trans loads, one
// per byte of its token (an L2 / vector-L1 hit each: the table is at most MD_STOP_STATES_MAX * 512 B = 2 MiB and the
// states a text visits are few), so a launch lasts as long as its longest token's chain whatever the number of rows; the
// lanes' chains overlap inside one wave, and a second wave only starts at the 65th row.  Everything that is not the
// chain is issued in front of it: the token's bytes arrive in 16-byte pieces (one wide load per piece, the next piece
// requested before the current one is walked), and match_len is read beside the chain, not in it -- no lookup waits for it.
// Integers only; plain C++ and vector stores.
#include "row_reduce.hpp"

namespace {
constexpr int STOP_THREADS = 64;  // rows per workgroup: one wave

struct StopRows {
  const int32_t *tokens, *slots;
  int slot0, batch;
  const uint16_t *trans, *match_len;
  const int32_t* match_id;
  int state_cap;
  const int32_t *id_ptr, *ids, *id_base;
  const int32_t* tok_off;
  const uint8_t* tok_bytes;
  int vocab;
  int64_t n_bytes;
  int32_t *state, *n_tok, *n_seen, *at, *keep, *which;
};

// 16 bytes of the vocabulary from byte `i` on, as four dwords in memory order.  The bytes of a token start anywhere:
// a piece that lies inside the array is ONE load of 16 bytes at that address (global loads need no alignment), the
// last piece of the array is gathered byte by byte and never reads past n_bytes.
__device__ __forceinline__ uint4 load_piece(const uint8_t* __restrict__ p, int64_t i, int64_t n_bytes) {
  uint4 w = make_uint4(0u, 0u, 0u, 0u);
  if (i + 16 <= n_bytes) {
    __builtin_memcpy(&w, p + i, 16);
  } else {
    unsigned v[4] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < 16 && i + j < n_bytes; ++j) v[j >> 2] |= (unsigned)p[i + j] << (8 * (j & 3));
    w = make_uint4(v[0], v[1], v[2], v[3]);
  }
  return w;
}

__global__ __launch_bounds__(STOP_THREADS) void stop_rows_kernel(StopRows a) {
  const int r = blockIdx.x * STOP_THREADS + threadIdx.x;
  if (r >= a.batch) return;
  const int s = state_slot(a.slots, a.slot0, r);
  if (s < 0) return;  // idle: nothing of the row is read or written
  int q = a.state[s];
  if (q < 0) return;  // no stop set: skipped, its words stay what they are
  const int v = a.tokens[r];
  const int nt = a.n_tok[s], nb = a.n_seen[s];
  // the token's byte range; a token that is no id, or a range outside the array, spells nothing
  int64_t off = 0, end = 0;
  if (a.tok_off && v >= 0 && v < a.vocab) {
    off = a.tok_off[v];
    end = a.tok_off[v + 1];
    if (off < 0 || end < off || end > a.n_bytes) end = off;
  }
  const int len = (int)(end - off);
  a.n_tok[s] = nt + 1;
  a.n_seen[s] = nb + len;
  if (a.at[s] >= 0) return;  // matched before: the counters only
  uint4 piece = make_uint4(0u, 0u, 0u, 0u);
  if (len > 0) piece = load_piece(a.tok_bytes, off, a.n_bytes);  // in flight while the ids are compared
  if (q >= a.state_cap) q = 0;  // (never an index outside the table)
  // ---- 1. a stop id: the row ends in front of the token
  const int i0 = a.id_ptr[s];
  const int n_ids = min(max(a.id_ptr[s + 1] - i0, 0), MD_STOP_IDS_MAX);
  for (int j = 0; j < n_ids; ++j) {
    if (a.ids[i0 + j] == v) {
      a.at[s] = nt;
      a.keep[s] = nb;
      a.which[s] = a.id_base[s] + j;
      return;
    }
  }
  // ---- 2. the token's bytes through the automaton: the first byte after which a string is a suffix of the text
  int hit = -1, hit_q = 0;
  for (int p0 = 0; p0 < len; p0 += 16) {
    const uint4 cur = piece;
    if (p0 + 16 < len) piece = load_piece(a.tok_bytes, off + p0 + 16, a.n_bytes);  // the next piece, before this one's chain
    const unsigned w[4] = {cur.x, cur.y, cur.z, cur.w};
    const int m = min(16, len - p0);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < m) {
        const unsigned c = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        int nq = a.trans[q * 256 + (int)c];
        if (nq >= a.state_cap) nq = 0;
        q = nq;
        const int ml = a.match_len[q];  // beside the chain: the next lookup does not wait for it
        if (hit < 0 && ml > 0) {
          hit = p0 + j;
          hit_q = q;
        }
      }
    }
    if (hit >= 0) break;  // (the rest of a piece was walked beside the chain; the match's state is what is stored)
  }
  a.state[s] = hit >= 0 ? hit_q : q;  // a matched row keeps the state of its match (moondream_amd/stop.py: walk)
  if (hit >= 0) {
    a.at[s] = nt;
    a.keep[s] = nb + hit + 1 - (int)a.match_len[hit_q];
    a.which[s] = a.match_id[hit_q];
  }
}

}  // namespace

extern "C" md_status md_stop_rows(const int32_t* tokens, int32_t batch, const int32_t* slots, int32_t slot0,
                                  const uint16_t* trans, const uint16_t* match_len, const int32_t* match_id, int32_t state_cap,
                                  const int32_t* id_ptr, const int32_t* ids, const int32_t* id_base, const int32_t* tok_off,
                                  const uint8_t* tok_bytes, int32_t vocab, int64_t n_bytes, int32_t* state, int32_t* n_tok,
                                  int32_t* n_seen, int32_t* at, int32_t* keep, int32_t* which, void* stream) {
  MD_CHECK_ARG(tokens && trans && match_len && match_id && id_ptr && ids && id_base && state && n_tok && n_seen && at && keep && which);
  MD_CHECK_ARG(batch >= 0 && state_cap >= 1 && state_cap <= MD_STOP_STATES_MAX);
  MD_CHECK_ARG((tok_off == nullptr) == (tok_bytes == nullptr) && (tok_off ? vocab >= 1 && n_bytes >= 0 : true));
  if (batch == 0) return MD_OK;
  StopRows a;
  a.tokens = tokens; a.slots = slots; a.slot0 = slot0; a.batch = batch;
  a.trans = trans; a.match_len = match_len; a.match_id = match_id; a.state_cap = state_cap;
  a.id_ptr = id_ptr; a.ids = ids; a.id_base = id_base;
  a.tok_off = tok_off; a.tok_bytes = tok_bytes; a.vocab = tok_off ? vocab : 0; a.n_bytes = tok_off ? n_bytes : 0;
  a.state = state; a.n_tok = n_tok; a.n_seen = n_seen; a.at = at; a.keep = keep; a.which = which;
  hipLaunchKernelGGL(stop_rows_kernel, dim3((batch + STOP_THREADS - 1) / STOP_THREADS), dim3(STOP_THREADS), 0,
                     (hipStream_t)stream, a);
  return md_launch_status();
}
