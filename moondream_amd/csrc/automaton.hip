// Compiling a byte-level DFA to a token automaton (md_automaton_lift / _count / _fill): the table md_constrain_rows reads,
// made on the device.  Three kernels, all integer, all deterministic:
//   lift:  next[q][v] = the DFA state after token v's bytes from state q.  A thread owns one token and walks LIFT_QT
//          states at a time through it, so each byte is loaded once per LIFT_QT walks and the LIFT_QT dependent chains
//          overlap (the walk is latency bound: one table read per byte, each depending on the last).  Neighbouring
//          threads own neighbouring tokens, whose bytes are neighbours in tok_bytes.  A DFA of <= LIFT_LDS_STATES states
//          is staged whole in LDS as int16 (512 B per state); a larger one is read from global memory (4 MiB at the cap:
//          one XCD's L2 holds it).
//   count: one workgroup per state: a histogram of the row's next values in LDS (S + 3 bins; FORBID, by far the most
//          frequent value, is counted in a register and never touches an LDS atomic), the most frequent value (ties: the
//          smallest) as the default, the number of other tokens as the edge count.  A one-workgroup exclusive scan turns
//          the counts into row_ptr.
//   fill:  one workgroup per state: a ballot / popcount stream compaction over the row in token order writes the
//          (token, next) pairs that differ from the default, ascending.
// States go through the lift in slabs of MD_AUTOMATON_SLAB, so that the next matrix never exceeds slab * V entries; the
// fill pass lifts every slab again rather than keep S * V entries.
#include "md_common.hpp"

namespace {
constexpr int LIFT_THREADS = 256;
constexpr int LIFT_QT = 4;             // states walked together by one thread
constexpr int LIFT_LDS_STATES = 128;   // a DFA up to this size lives in LDS: 128 * 256 * 2 B = 64 KiB
constexpr int LIFT_QPB_GLOBAL = 16;    // states per workgroup on the global-memory path
constexpr int ROW_THREADS = 512;       // count / fill: one workgroup per state
constexpr int ROW_WAVES = ROW_THREADS / MD_WAVE;
constexpr int SCAN_THREADS = 1024;     // 4 states per thread: MD_AUTOMATON_STATES_MAX in one workgroup
constexpr int HIST_BINS_MAX = MD_AUTOMATON_STATES_MAX + 3;

template <bool IN_LDS>
__global__ __launch_bounds__(LIFT_THREADS) void automaton_lift_kernel(
    const int32_t* __restrict__ trans, const uint8_t* __restrict__ accept, int n_states, const int32_t* __restrict__ tok_off,
    const uint8_t* __restrict__ tok_bytes, int64_t n_bytes, int vocab, int eos_id, const uint8_t* __restrict__ forbidden, int q0,
    int nq, int qpb, int32_t* __restrict__ next) {
  extern __shared__ __attribute__((aligned(16))) int16_t lift_trans[];  // IN_LDS: [n_states][256], -1: dead
  const int tid = threadIdx.x;
  if (IN_LDS) {
    for (int i = tid; i < n_states * 256; i += LIFT_THREADS) {
      const int t = trans[i];
      lift_trans[i] = (unsigned)t < (unsigned)n_states ? (int16_t)t : (int16_t)-1;
    }
    __syncthreads();
  }
  const int v = blockIdx.x * LIFT_THREADS + tid;
  if (v >= vocab) return;  // after the only barrier
  int64_t off = tok_off[v], end = tok_off[v + 1];
  const bool spelled = !forbidden[v] && off >= 0 && end > off && end <= n_bytes;  // else: FORBID in every state
  if (!spelled) end = off;
  const int qb0 = blockIdx.y * qpb, qb1 = min(qb0 + qpb, nq);
  for (int qb = qb0; qb < qb1; qb += LIFT_QT) {
    int s[LIFT_QT];
#pragma unroll
    for (int j = 0; j < LIFT_QT; ++j) s[j] = (spelled && qb + j < qb1) ? q0 + qb + j : -1;
    for (int64_t i = off; i < end; ++i) {
      const int b = tok_bytes[i];
#pragma unroll
      for (int j = 0; j < LIFT_QT; ++j) {
        if (s[j] >= 0) {
          if (IN_LDS) {
            s[j] = lift_trans[s[j] * 256 + b];
          } else {
            const int t = trans[(int64_t)s[j] * 256 + b];
            s[j] = (unsigned)t < (unsigned)n_states ? t : -1;
          }
        }
      }
      static_assert(LIFT_QT == 4, "the test below names four walks");
      if ((s[0] & s[1] & s[2] & s[3]) < 0) break;  // every sign bit set: every walk is dead
    }
#pragma unroll
    for (int j = 0; j < LIFT_QT; ++j) {
      if (qb + j >= qb1) break;
      int r = s[j] >= 0 ? s[j] : MD_CONSTRAINT_FORBID;
      if (v == eos_id) r = accept[q0 + qb + j] ? MD_CONSTRAINT_FREE : MD_CONSTRAINT_FORBID;
      next[(int64_t)(qb + j) * vocab + v] = r;
    }
  }
}

// default_next[q] and the edge count of state q (into row_ptr[q]) from its row of the slab's next matrix.
__global__ __launch_bounds__(ROW_THREADS) void automaton_count_kernel(const int32_t* __restrict__ next, int vocab, int n_states, int q0,
                                                                      int32_t* __restrict__ default_next, int32_t* __restrict__ row_ptr) {
  __shared__ unsigned hist[HIST_BINS_MAX];  // bin = value + 3: FORBID, DEAD (never stored), FREE, state 0 ..
  __shared__ unsigned best;
  const int tid = threadIdx.x, bins = n_states + 3;
  const int32_t* row = next + (int64_t)blockIdx.x * vocab;
  for (int i = tid; i < bins; i += ROW_THREADS) hist[i] = 0;
  if (tid == 0) best = 0;
  __syncthreads();
  unsigned n_forbid = 0;
  for (int v = tid; v < vocab; v += ROW_THREADS) {
    const int x = row[v];
    if (x == MD_CONSTRAINT_FORBID)
      ++n_forbid;
    else if ((unsigned)(x + 3) < (unsigned)bins)
      atomicAdd(&hist[x + 3], 1u);
  }
  if (n_forbid) atomicAdd(&hist[0], n_forbid);
  __syncthreads();
  // the largest count, ties to the smallest value: one max over (count << 13 | 8191 - bin); count <= 2^18, bin < 2^13
  unsigned key = 0;
  for (int i = tid; i < bins; i += ROW_THREADS) key = max(key, (hist[i] << 13) | (unsigned)(8191 - i));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, o, 64));
  if ((tid & 63) == 0) atomicMax(&best, key);
  __syncthreads();
  if (tid == 0) {
    const unsigned k = best;
    default_next[q0 + blockIdx.x] = (int)(8191 - (k & 8191u)) - 3;
    row_ptr[q0 + blockIdx.x] = vocab - (int)(k >> 13);
  }
}

// row_ptr[0 .. n] holds n counts (entry n unread): in place, their exclusive scan, the total in entry n.
__global__ __launch_bounds__(SCAN_THREADS) void automaton_scan_kernel(int32_t* __restrict__ row_ptr, int n) {
  __shared__ int wave_sum_lds[SCAN_THREADS / MD_WAVE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int c[4], mine = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = 4 * tid + j < n ? row_ptr[4 * tid + j] : 0;
    mine += c[j];
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wave_sum_lds[wave] = incl;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < SCAN_THREADS / MD_WAVE; ++w) {
    const int t = wave_sum_lds[w];
    if (w < wave) before += t;
    total += t;
  }
  int run = before + incl - mine;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (4 * tid + j < n) row_ptr[4 * tid + j] = run;
    run += c[j];
  }
  if (tid == 0) row_ptr[n] = total;
}

// The edges of state q: the tokens whose next value is not the default, ascending, at row_ptr[q] ..
__global__ __launch_bounds__(ROW_THREADS) void automaton_fill_kernel(const int32_t* __restrict__ next, int vocab, int q0,
                                                                     const int32_t* __restrict__ default_next,
                                                                     const int32_t* __restrict__ row_ptr, int32_t* __restrict__ edge_tok,
                                                                     int32_t* __restrict__ edge_next, int64_t edge_cap) {
  __shared__ int wave_n[2][ROW_WAVES];  // double buffered: one barrier per chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = q0 + blockIdx.x;
  const int32_t* row = next + (int64_t)blockIdx.x * vocab;
  const int d = default_next[q];
  const int64_t lo = row_ptr[q], hi = min((int64_t)row_ptr[q + 1], edge_cap);
  int64_t run = lo;
  int buf = 0;
  for (int v0 = 0; v0 < vocab; v0 += ROW_THREADS, buf ^= 1) {
    const int v = v0 + tid;
    const int x = v < vocab ? row[v] : d;
    const bool edge = x != d;
    const unsigned long long m = __ballot(edge);
    if (lane == 0) wave_n[buf][wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < ROW_WAVES; ++w) {
      const int t = wave_n[buf][w];
      if (w < wave) before += t;
      total += t;
    }
    const int64_t at = run + before + __popcll(m & ((1ull << lane) - 1ull));
    if (edge && at < hi) {  // never past the state's own range nor the caller's arrays
      edge_tok[at] = v;
      edge_next[at] = x;
    }
    run += total;
  }
}

bool dfa_args_ok(const int32_t* trans, const uint8_t* accept, int32_t n_states, const int32_t* tok_off, const uint8_t* tok_bytes,
                 int64_t n_bytes, int32_t vocab, int32_t eos_id, const uint8_t* forbidden) {
  return trans && accept && tok_off && tok_bytes && forbidden && n_states >= 1 && n_states <= MD_AUTOMATON_STATES_MAX && vocab >= 1 &&
         vocab <= MD_CONSTRAIN_VOCAB_MAX && eos_id >= 0 && eos_id < vocab && n_bytes >= 0;
}

md_status launch_lift(const int32_t* trans, const uint8_t* accept, int n_states, const int32_t* tok_off, const uint8_t* tok_bytes,
                      int64_t n_bytes, int vocab, int eos_id, const uint8_t* forbidden, int q0, int nq, int32_t* next, hipStream_t st) {
  const int gx = (vocab + LIFT_THREADS - 1) / LIFT_THREADS;
  if (n_states <= LIFT_LDS_STATES) {
    const size_t lds = (size_t)n_states * 256 * sizeof(int16_t);
    MD_TRY(md_ensure_dynamic_lds((const void*)automaton_lift_kernel<true>, LIFT_LDS_STATES * 256 * (int)sizeof(int16_t)));
    hipLaunchKernelGGL(automaton_lift_kernel<true>, dim3(gx, 1), dim3(LIFT_THREADS), lds, st, trans, accept, n_states, tok_off, tok_bytes,
                       n_bytes, vocab, eos_id, forbidden, q0, nq, nq, next);
  } else {
    const int gy = (nq + LIFT_QPB_GLOBAL - 1) / LIFT_QPB_GLOBAL;
    hipLaunchKernelGGL(automaton_lift_kernel<false>, dim3(gx, gy), dim3(LIFT_THREADS), 0, st, trans, accept, n_states, tok_off,
                       tok_bytes, n_bytes, vocab, eos_id, forbidden, q0, nq, LIFT_QPB_GLOBAL, next);
  }
  return md_launch_status();
}
}  // namespace

extern "C" size_t md_automaton_workspace_bytes(int32_t n_states, int32_t vocab) {
  if (n_states < 1 || n_states > MD_AUTOMATON_STATES_MAX || vocab < 1 || vocab > MD_CONSTRAIN_VOCAB_MAX) return 0;
  return (size_t)(n_states < MD_AUTOMATON_SLAB ? n_states : MD_AUTOMATON_SLAB) * (size_t)vocab * sizeof(int32_t);
}

extern "C" md_status md_automaton_lift(const int32_t* trans, const uint8_t* accept, int32_t n_states, const int32_t* tok_off,
                                       const uint8_t* tok_bytes, int64_t n_bytes, int32_t vocab, int32_t eos_id,
                                       const uint8_t* forbidden, int32_t q0, int32_t nq, int32_t* next, void* stream) {
  MD_CHECK_ARG(dfa_args_ok(trans, accept, n_states, tok_off, tok_bytes, n_bytes, vocab, eos_id, forbidden) && next);
  MD_CHECK_ARG(q0 >= 0 && nq >= 1 && nq <= MD_AUTOMATON_SLAB && q0 <= n_states - nq);
  return launch_lift(trans, accept, n_states, tok_off, tok_bytes, n_bytes, vocab, eos_id, forbidden, q0, nq, next, (hipStream_t)stream);
}

extern "C" md_status md_automaton_count(const int32_t* trans, const uint8_t* accept, int32_t n_states, const int32_t* tok_off,
                                        const uint8_t* tok_bytes, int64_t n_bytes, int32_t vocab, int32_t eos_id,
                                        const uint8_t* forbidden, int32_t* default_next, int32_t* row_ptr, void* ws, size_t ws_bytes,
                                        void* stream) {
  MD_CHECK_ARG(dfa_args_ok(trans, accept, n_states, tok_off, tok_bytes, n_bytes, vocab, eos_id, forbidden));
  MD_CHECK_ARG(default_next && row_ptr && ws && ws_bytes >= md_automaton_workspace_bytes(n_states, vocab));
  hipStream_t st = (hipStream_t)stream;
  for (int q0 = 0; q0 < n_states; q0 += MD_AUTOMATON_SLAB) {
    const int nq = n_states - q0 < MD_AUTOMATON_SLAB ? n_states - q0 : MD_AUTOMATON_SLAB;
    MD_TRY(launch_lift(trans, accept, n_states, tok_off, tok_bytes, n_bytes, vocab, eos_id, forbidden, q0, nq, (int32_t*)ws, st));
    hipLaunchKernelGGL(automaton_count_kernel, dim3(nq), dim3(ROW_THREADS), 0, st, (const int32_t*)ws, vocab, n_states, q0, default_next,
                       row_ptr);
    MD_TRY(md_launch_status());
  }
  hipLaunchKernelGGL(automaton_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, row_ptr, n_states);
  return md_launch_status();
}

extern "C" md_status md_automaton_fill(const int32_t* trans, const uint8_t* accept, int32_t n_states, const int32_t* tok_off,
                                       const uint8_t* tok_bytes, int64_t n_bytes, int32_t vocab, int32_t eos_id,
                                       const uint8_t* forbidden, const int32_t* default_next, const int32_t* row_ptr, int32_t* edge_tok,
                                       int32_t* edge_next, int64_t edge_cap, void* ws, size_t ws_bytes, void* stream) {
  MD_CHECK_ARG(dfa_args_ok(trans, accept, n_states, tok_off, tok_bytes, n_bytes, vocab, eos_id, forbidden));
  MD_CHECK_ARG(default_next && row_ptr && edge_cap >= 0 && (edge_cap == 0 || (edge_tok && edge_next)));
  MD_CHECK_ARG(ws && ws_bytes >= md_automaton_workspace_bytes(n_states, vocab));
  if (edge_cap == 0) return MD_OK;
  hipStream_t st = (hipStream_t)stream;
  for (int q0 = 0; q0 < n_states; q0 += MD_AUTOMATON_SLAB) {
    const int nq = n_states - q0 < MD_AUTOMATON_SLAB ? n_states - q0 : MD_AUTOMATON_SLAB;
    MD_TRY(launch_lift(trans, accept, n_states, tok_off, tok_bytes, n_bytes, vocab, eos_id, forbidden, q0, nq, (int32_t*)ws, st));
    hipLaunchKernelGGL(automaton_fill_kernel, dim3(nq), dim3(ROW_THREADS), 0, st, (const int32_t*)ws, vocab, q0, default_next, row_ptr,
                       edge_tok, edge_next, edge_cap);
    MD_TRY(md_launch_status());
  }
  return MD_OK;
}
