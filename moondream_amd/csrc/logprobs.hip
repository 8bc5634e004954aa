// Log-probabilities of the model's own distribution over a row of logits (temperature 1, untruncated):
//   * of one given token per row, with its rank (md_token_logprobs);
//   * of the k most probable tokens per row, by a radix select over the bf16 keys (md_topk_logprobs);
//   * the same k entries for every live beam: the row phase of md_beam_select (md_beam_rows, called from beam.hip).
// The three share one maximum and one sum per row, in one summation order.  One workgroup of 1024 threads per row.
#include "row_reduce.hpp"
#include "text_internal.hpp"

namespace {

// ---------------------------------------------------------------------------
// log-probability and rank of one given token per row (md_token_logprobs): the model's own distribution at temperature 1,
// untruncated, over the LIVE tokens of the row (all but the suppressed id of a suppressed row).
// TWO-PASS form: pass 1 takes the maximum m of the live logits (and the integer rank counts), pass 2 sums exp(x - m).
// Summation order, a function of vocab alone (never of the row count or the row):
//   1. thread tid adds its strided share exp(x[tid + k * 1024] - m), k = 0, 1, .. ascending, sequentially in fp32
//      (n_t = ceil(vocab / 1024) terms: 50 at vocab 51200);
//   2. a 6-level xor butterfly over the wave's 64 lanes (offsets 32, 16, .., 1);
//   3. a 4-level xor butterfly over the 16 wave partials (offsets 8, 4, 2, 1).
// So every term passes through at most (n_t - 1) + log2(1024) additions.  A -inf logit adds exp(-inf) = 0.  The rank is
// a sum of integers: exact, whatever the order.  Plain 2-byte loads: no alignment demand on vocab or the row stride.
constexpr int LOGPROB_THREADS = 1024;

__global__ __launch_bounds__(LOGPROB_THREADS) void token_logprobs_kernel(const bf16_t* __restrict__ logits, int64_t ld, int vocab,
                                                                         int suppress_id, const int32_t* __restrict__ suppress_rows,
                                                                         const int32_t* __restrict__ targets,
                                                                         float* __restrict__ logprob, int32_t* __restrict__ rank) {
  __shared__ float red_max[LOGPROB_THREADS / 64];
  __shared__ float red_sum[LOGPROB_THREADS / 64];
  __shared__ int red_cnt[LOGPROB_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  // every exit below is taken by the whole workgroup (t and sup are per row), before any barrier
  const int t = targets[r];
  if (t < 0 || t >= vocab) {  // an idle / padding row: the logits row is not read
    if (tid == 0) {
      logprob[r] = __builtin_nanf("");
      if (rank) rank[r] = -1;
    }
    return;
  }
  const int sup = row_suppress(suppress_id, suppress_rows, r);
  if (t == sup) {
    if (tid == 0) {
      logprob[r] = -INFINITY;
      if (rank) rank[r] = -1;
    }
    return;
  }
  const bf16_t* lr = logits + (int64_t)r * ld;
  const float xt = bf2f(lr[t]);

  // ---- pass 1: maximum of the live logits; tokens that come before t in md_argmax_bf16's order (greater, or equal with a lower id)
  float mx = -INFINITY;
  int cnt = 0;
  for (int i = tid; i < vocab; i += LOGPROB_THREADS) {
    if (i == sup) continue;
    const float x = bf2f(lr[i]);
    mx = fmaxf(mx, x);
    cnt += (x > xt || (x == xt && i < t)) ? 1 : 0;
  }
  mx = wave_max(mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  wave_partial_store(mx, red_max);
  wave_partial_store(cnt, red_cnt);
  __syncthreads();
  mx = fold16_max(red_max);
  cnt = fold16_sum(red_cnt);

  // ---- pass 2: s = sum over live v of exp(x[v] - m), in the order documented above
  float s = 0.f;
  for (int i = tid; i < vocab; i += LOGPROB_THREADS) {
    if (i == sup) continue;
    s += expf(bf2f(lr[i]) - mx);
  }
  wave_partial_store(wave_sum(s), red_sum);
  __syncthreads();
  s = fold16_sum(red_sum);

  if (tid == 0) {
    logprob[r] = (xt - mx) - logf(s);
    if (rank) rank[r] = cnt;
  }
}

// ---------------------------------------------------------------------------
// The k live tokens of lowest md_token_logprobs rank per row, with their log-probabilities (md_topk_logprobs): entry j is
// the live token of rank j (greater logit first, equal logits by lower id).  m and s are token_logprobs_kernel's, in its
// summation order (the same strided loops, then the same wave_sum / fold16_* of row_reduce.hpp), so a value here is that
// kernel's value for the same token, bit for bit.
// A bf16 logit is a 16-bit key, so the k-th largest is found by a two-level radix select instead of k arg-max passes:
//   pass 1  m, and a histogram of the key's high byte           -> the high byte H of the k-th token, n(high byte > H)
//   pass 2  s, and a histogram of the low byte among high == H  -> the threshold key T, n_gt = n(key > T) < k
//   (only if more tokens equal T than the k - n_gt that fit: a bitmap over the ids of the tokens equal to T, one bit per
//    id, gives the id I of the last one that fits; ids are distinct, so "id <= I" keeps exactly the lowest ids)
//   pass 3  the tokens with key > T, or key == T and id <= I, go to at most 32 slots in arrival order
//   wave 0  orders the slots by counting (key descending, id ascending) and writes the row's outputs.
// The key is monotone in the float order and the two zeros share one key, so key order is the `>` / `==` of
// token_logprobs_kernel's rank; -inf has the lowest key of all non-NaN values.  A NaN logit is out of contract; its key
// is a 16-bit number like any other, so it can misplace entries but not an address.
// Histograms: 256 bins x 32 copies, a lane adds to copy (lane & 31): whatever the bins, the 32 lanes of an LDS lane group
// hit 32 different banks, where one copy would serialise a wave on the two or three exponents that hold most of a row.
// The row (100 KiB at vocab 51200) is read three or four times, after the first from L2.
constexpr int TOPK_THREADS = LOGPROB_THREADS;
constexpr int TOPK_COPIES = 32;
constexpr int TOPK_HIST_WORDS = 256 * TOPK_COPIES;      // 32 KiB; afterwards the id bitmap
constexpr int TOPK_WINDOW = TOPK_HIST_WORDS * 32;       // ids one bitmap covers

__device__ __forceinline__ unsigned topk_key(bf16_t bits) {
  unsigned u = (unsigned)bits & 0xffffu;
  if (u == 0x8000u) u = 0u;  // -0.0 == +0.0
  return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}

__device__ __forceinline__ void topk_zero(unsigned* hist) {
  for (int i = threadIdx.x; i < TOPK_HIST_WORDS; i += TOPK_THREADS) hist[i] = 0u;
}

// hist [256][32] -> cnt[256] (all threads; thread t sums 8 copies of bin t >> 2, rotated by the bin: bank-conflict free),
// then wave 0 walks the bins from 255 down: the bin that holds the need-th token in descending order, need =
// min(want, total).  found = {bin (-1: no live token), tokens in higher bins, tokens in the bin, total}.  Ends in a barrier.
__device__ __forceinline__ void topk_find_digit(const unsigned* hist, unsigned* cnt, int want, int* found) {
  const int tid = threadIdx.x;
  __syncthreads();
  {
    const int bin = tid >> 2, q = tid & 3;
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) c += hist[bin * TOPK_COPIES + q * 8 + ((j + bin) & 7)];
    c += __shfl_xor(c, 1, 64);
    c += __shfl_xor(c, 2, 64);
    if (q == 0) cnt[bin] = c;
  }
  __syncthreads();
  if (tid < 64) {
    unsigned c[4], sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c[i] = cnt[255 - 4 * tid - i];
      sum += c[i];
    }
    const unsigned incl = wave_inclusive_scan(sum);
    const unsigned total = __shfl(incl, 63, 64);
    const unsigned need = min((unsigned)want, total);
    if (tid == 0) {
      found[0] = -1;
      found[3] = (int)total;
    }
    unsigned above = incl - sum;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (above < need && above + c[i] >= need) {  // one bin at most: the counts above it only grow downwards
        found[0] = 255 - 4 * tid - i;
        found[1] = (int)above;
        found[2] = (int)c[i];
      }
      above += c[i];
    }
  }
  __syncthreads();
}

// a row that is not computed: its k entries are -1 / NaN (whole workgroup)
__device__ __forceinline__ void topk_row_off(int k, int32_t* __restrict__ out_id, float* __restrict__ out_lp) {
  if ((int)threadIdx.x < k) {
    out_id[threadIdx.x] = -1;
    out_lp[threadIdx.x] = __builtin_nanf("");
  }
}

// One row's k entries, by the whole workgroup of TOPK_THREADS: the body of md_topk_logprobs' kernel, and of the row phase of
// md_beam_select (beam_rows_kernel), which is why the two agree bit for bit.  lr: the row; sup: the suppressed id or -1.
__device__ __forceinline__ void topk_row(const bf16_t* __restrict__ lr, int vocab, int sup, int k, int32_t* __restrict__ out_id,
                                         float* __restrict__ out_lp) {
  __shared__ unsigned hist[TOPK_HIST_WORDS];
  __shared__ unsigned cnt[256];
  __shared__ float red_max[TOPK_THREADS / 64];
  __shared__ float red_sum[TOPK_THREADS / 64];
  __shared__ int wave_bits[TOPK_THREADS / 64];
  __shared__ int found[4];
  __shared__ int last_id;   // I: the highest id equal to T that is kept
  __shared__ int n_slots;
  __shared__ unsigned slot_key[MD_TOPK_MAX];
  __shared__ int slot_id[MD_TOPK_MAX];
  const int tid = threadIdx.x;
  // every exit below is taken by the whole workgroup (per-row values), before or between barriers
  const int copy = tid & (TOPK_COPIES - 1);

  // ---- pass 1: maximum of the live logits (token_logprobs_kernel's reduction), histogram of the high byte
  topk_zero(hist);
  if (tid == 0) {
    n_slots = 0;
    last_id = 0x7fffffff;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int i = tid; i < vocab; i += TOPK_THREADS) {
    if (i == sup) continue;
    const bf16_t b = lr[i];
    mx = fmaxf(mx, bf2f(b));
    atomicAdd(&hist[(topk_key(b) >> 8) * TOPK_COPIES + copy], 1u);
  }
  wave_partial_store(wave_max(mx), red_max);
  topk_find_digit(hist, cnt, k, found);  // (its first barrier orders red_max too)
  mx = fold16_max(red_max);
  const int hi = found[0], above_hi = found[1];
  const int n_take = min(k, found[3]);  // entries the row fills
  if (hi < 0) {                         // no live token at all (vocab 1, suppressed)
    topk_row_off(k, out_id, out_lp);
    return;
  }

  // ---- pass 2: s in token_logprobs_kernel's order, histogram of the low byte inside the high byte's bin
  topk_zero(hist);
  __syncthreads();
  float s = 0.f;
  for (int i = tid; i < vocab; i += TOPK_THREADS) {
    if (i == sup) continue;
    s += expf(bf2f(lr[i]) - mx);
    const unsigned key = topk_key(lr[i]);
    if ((int)(key >> 8) == hi) atomicAdd(&hist[(key & 0xffu) * TOPK_COPIES + copy], 1u);
  }
  wave_partial_store(wave_sum(s), red_sum);
  topk_find_digit(hist, cnt, n_take - above_hi, found);
  s = fold16_sum(red_sum);
  const unsigned thr = ((unsigned)hi << 8) | (unsigned)found[0];  // T
  const int n_gt = above_hi + found[1];                          // tokens above T: < n_take
  const int n_eq = found[2];                                     // tokens equal to T
  const int eq_take = n_take - n_gt;                             // of which the lowest ids are kept: >= 1

  // ---- more equal tokens than fit: the id of the eq_take-th of them, from a bitmap over the ids, a window at a time
  if (n_eq > eq_take) {
    int before = 0;  // equal tokens in the windows already seen (the same in every thread)
    for (int w0 = 0;;) {
      __syncthreads();
      topk_zero(hist);
      __syncthreads();
      const int w1 = (vocab - w0 > TOPK_WINDOW) ? w0 + TOPK_WINDOW : vocab;
      for (int i = w0 + tid; i < w1; i += TOPK_THREADS) {
        if (i == sup) continue;
        if (topk_key(lr[i]) == thr) atomicOr(&hist[(i - w0) >> 5], 1u << ((i - w0) & 31));
      }
      __syncthreads();
      // thread t owns words 8t .. 8t+7, in id order: a block-wide exclusive scan of the bit counts
      int mine = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) mine += __popc(hist[tid * 8 + j]);
      const int incl = wave_inclusive_scan(mine);
      if ((tid & 63) == 63) wave_bits[tid >> 6] = incl;
      __syncthreads();
      int excl = before + incl - mine, in_window = 0;
      for (int w = 0; w < TOPK_THREADS / 64; ++w) {
        if (w < (tid >> 6)) excl += wave_bits[w];
        in_window += wave_bits[w];
      }
      if (excl < eq_take && excl + mine >= eq_take) {  // one thread: the eq_take-th bit is in its words
        int left = eq_take - excl;
        for (int j = 0; j < 8; ++j) {
          unsigned word = hist[tid * 8 + j];
          const int c = __popc(word);
          if (left > c) {
            left -= c;
            continue;
          }
          for (; left > 1; --left) word &= word - 1u;  // drop the lowest set bits before it
          last_id = w0 + (tid * 8 + j) * 32 + (__ffs(word) - 1);
          break;
        }
      }
      before += in_window;
      if (before >= eq_take || w1 == vocab) break;  // uniform
      w0 = w1;
    }
    __syncthreads();
  }
  const int keep_to = last_id;

  // ---- pass 3: the n_take kept tokens, in arrival order
  for (int i = tid; i < vocab; i += TOPK_THREADS) {
    if (i == sup) continue;
    const unsigned key = topk_key(lr[i]);
    if (key > thr || (key == thr && i <= keep_to)) {
      const int at = atomicAdd(&n_slots, 1);
      if (at < MD_TOPK_MAX) {
        slot_key[at] = key;
        slot_id[at] = i;
      }
    }
  }
  __syncthreads();

  // ---- order by counting and write: entry = the number of kept tokens that come before this one
  if (tid < k) {
    int id = -1;
    float lp = __builtin_nanf("");
    int at = tid;
    const int n_have = min(n_take, n_slots);  // == n_take: the passes read the same row; never a slot that was not written
    if (tid < n_have) {
      const unsigned key = slot_key[tid];
      id = slot_id[tid];
      at = 0;
      for (int j = 0; j < n_have; ++j) at += (slot_key[j] > key || (slot_key[j] == key && slot_id[j] < id)) ? 1 : 0;
      lp = (bf2f(lr[id]) - mx) - logf(s);
    }
    out_id[at] = id;  // a permutation of 0 .. n_take-1 (keys with ids are distinct), then the unfilled entries in place
    out_lp[at] = lp;
  }
}

__global__ __launch_bounds__(TOPK_THREADS) void topk_logprobs_kernel(const bf16_t* __restrict__ logits, int64_t ld, int vocab,
                                                                     int suppress_id, const int32_t* __restrict__ suppress_rows,
                                                                     const int32_t* __restrict__ gate, int k,
                                                                     int32_t* __restrict__ top_ids, float* __restrict__ top_logprobs) {
  const int r = blockIdx.x;
  int32_t* out_id = top_ids + (int64_t)r * k;
  float* out_lp = top_logprobs + (int64_t)r * k;
  if (gate) {
    const int g = gate[r];
    if (g < 0 || g >= vocab) {  // an idle / padding row: the logits row is not read
      topk_row_off(k, out_id, out_lp);
      return;
    }
  }
  const int sup = row_suppress(suppress_id, suppress_rows, r);
  topk_row(logits + (int64_t)r * ld, vocab, sup, k, out_id, out_lp);
}

// The row phase of md_beam_select (csrc/beam.hip): the 2W best continuations of every live beam, md_topk_logprobs' entries.
// Row r is beam r % W of group r / W and reads logits row r (beams_in == W) or row r / W (beams_in == 1: the first decision,
// beam 0 alone).  A done group's rows are neither read nor written; a dead beam's (cum == -inf) entries are -1 / NaN.
__global__ __launch_bounds__(TOPK_THREADS) void beam_rows_kernel(const bf16_t* __restrict__ logits, int64_t ld, int vocab,
                                                                 int suppress_id, const int32_t* __restrict__ suppress_rows, int W,
                                                                 int beams_in, const float* __restrict__ cum,
                                                                 const int32_t* __restrict__ done, int32_t* __restrict__ cand_ids,
                                                                 float* __restrict__ cand_lp) {
  const int r = blockIdx.x, g = r / W, j = r - g * W, k = 2 * W;
  if (done[g] != 0) return;
  int32_t* out_id = cand_ids + (int64_t)r * k;
  float* out_lp = cand_lp + (int64_t)r * k;
  if (j >= beams_in || cum[r] == -INFINITY) {
    topk_row_off(k, out_id, out_lp);
    return;
  }
  const int lrow = beams_in == 1 ? g : r;
  const int sup = row_suppress(suppress_id, suppress_rows, lrow);
  topk_row(logits + (int64_t)lrow * ld, vocab, sup, k, out_id, out_lp);
}

}  // namespace

// internal (beam.hip): the row phase of md_beam_select
md_status md_beam_rows(const void* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t suppress_id,
                       const int32_t* suppress_rows, int32_t num_beams, int32_t beams_in, const float* cum, const int32_t* done,
                       int32_t* cand_ids, float* cand_lp, hipStream_t stream) {
  hipLaunchKernelGGL(beam_rows_kernel, dim3(rows), dim3(TOPK_THREADS), 0, stream, (const bf16_t*)logits, ld, vocab, suppress_id,
                     suppress_rows, num_beams, beams_in, cum, done, cand_ids, cand_lp);
  return md_launch_status();
}

extern "C" md_status md_token_logprobs(const void* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t suppress_id,
                                       const int32_t* suppress_rows, const int32_t* targets, float* logprob, int32_t* rank,
                                       void* stream) {
  MD_CHECK_ARG(logits && targets && logprob && rows >= 0 && vocab > 0 && ld >= vocab);
  if (rows == 0) return MD_OK;
  hipLaunchKernelGGL(token_logprobs_kernel, dim3(rows), dim3(LOGPROB_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, ld,
                     vocab, suppress_id, suppress_rows, targets, logprob, rank);
  return md_launch_status();
}

extern "C" md_status md_topk_logprobs(const void* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t suppress_id,
                                      const int32_t* suppress_rows, const int32_t* gate, int32_t k, int32_t* top_ids,
                                      float* top_logprobs, void* stream) {
  MD_CHECK_ARG(logits && top_ids && top_logprobs && rows >= 0 && vocab > 0 && ld >= vocab && k >= 1 && k <= MD_TOPK_MAX);
  if (rows == 0) return MD_OK;
  hipLaunchKernelGGL(topk_logprobs_kernel, dim3(rows), dim3(TOPK_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, ld,
                     vocab, suppress_id, suppress_rows, gate, k, top_ids, top_logprobs);
  return md_launch_status();
}
