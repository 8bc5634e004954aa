// The pick of one token per row from its logits: temperature / top-p sampling (reference: moondream.py:270-278,
// 313-318, 521-528), the top-k and min-p cuts of the same order, and the greedy row.  One kernel template, three entries:
// md_sample_top_p (one setting for all rows), md_sample_rows (per row), md_sample_rows_filtered (per row, with the cuts).
// HBM-bound row kernels: one workgroup of 1024 threads per sequence, plain 2-byte loads, wave shuffles.
#include "row_reduce.hpp"

#include <type_traits>

namespace {

// ---------------------------------------------------------------------------
// temperature + top-p sampling of one token per sequence.
//   z = bf16(logit / T);  p = bf16(softmax(z))                          moondream.py:526 (bf16 tensors, fp32 inside)
//   in descending-p order keep the tokens whose preceding mass is <= top_p (evaluated with the
//   reference's bf16 roundings, see below); renormalise                    moondream.py:270-278
//   draw from the kept distribution with the caller's uniform u          moondream.py:528 (torch.multinomial)
// The descending order is realised without a sort: bf16 probabilities take < 2^15 distinct
// positive values, so a histogram over the bit pattern (LDS, 128 KiB) gives every value's count
// and the mass above it; within the boundary value the lowest token ids are kept.
constexpr int SAMPLE_THREADS = 1024;
constexpr int HIST_BINS = 32768;

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < SAMPLE_THREADS / 64; ++i) t += red[i];
  return t;
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = -INFINITY;
  for (int i = 0; i < SAMPLE_THREADS / 64; ++i) t = fmaxf(t, red[i]);
  return t;
}

constexpr int SAMPLE_LDS = HIST_BINS * 4 + 16 * 4 + SAMPLE_THREADS * 4 + 16 * 4;  // histogram, wave partials, block scan, results

// One row, one workgroup of SAMPLE_THREADS: lr the row's logits, u its uniform, next its token, pr its row of probs_out (or
// nullptr).  The body of the sampling kernels; smem is the workgroup's SAMPLE_LDS bytes.
// FILTER (md_sample_rows_filtered): two more cuts of the same descending order, each a pair (boundary pattern, survivors
// inside it) like the top-p cut, all three taken on the same unrenormalised p:
//   top_k > 0 and < vocab: the first top_k tokens -- the walk carries a token COUNT next to the mass; the boundary is the
//     pattern at which the running count reaches top_k, of which top_k - (count above it) tokens survive;
//   min_p > 0: the tokens with p >= bf16(min_p * p_max) -- the boundary is the smallest occupied pattern >= that
//     threshold's, kept whole (p_max: the largest occupied pattern, so the best token always survives).
// The row's boundary is the LARGEST of the three patterns (the shortest prefix); where cuts share it, the smallest
// survivor count.  With FILTER false nothing of this is compiled: the unfiltered kernels do not pay for it.
template <bool FILTER>
__device__ __forceinline__ void sample_top_p_row(char* smem, const bf16_t* __restrict__ lr, int vocab, int suppress,
                                                 float temperature, float top_p, const float* __restrict__ u,
                                                 int32_t* __restrict__ next, bf16_t* __restrict__ pr, int top_k = 0,
                                                 float min_p = 0.f) {
  unsigned* hist = (unsigned*)smem;                    // [HIST_BINS] counts per bf16 bit pattern
  float* red = (float*)(smem + HIST_BINS * 4);         // [16]
  float* scan = red + 16;                              // [SAMPLE_THREADS] block scans
  int* shared_i = (int*)(scan + SAMPLE_THREADS);       // [16] boundary pattern, survivors in it, drawn token, ...
  const int tid = threadIdx.x;
  const float inv_t = temperature;  // division, not a reciprocal multiply: the reference divides
  if (FILTER && tid == 0) shared_i[5] = 0;  // the largest occupied pattern (the reductions below order it before its use)

  // ---- z = bf16(logit / T), softmax statistics
  float mx = -INFINITY;
  for (int i = tid; i < vocab; i += SAMPLE_THREADS) {
    float z = (i == suppress) ? -INFINITY : bf2f(f2bf(bf2f(lr[i]) / inv_t));
    mx = fmaxf(mx, z);
  }
  mx = block_max(mx, red);
  float s = 0.f;
  for (int i = tid; i < vocab; i += SAMPLE_THREADS) {
    float z = (i == suppress) ? -INFINITY : bf2f(f2bf(bf2f(lr[i]) / inv_t));
    s += expf(z - mx);
  }
  s = block_sum(s, red);
  auto prob_bits = [&](int i) -> unsigned {
    float z = (i == suppress) ? -INFINITY : bf2f(f2bf(bf2f(lr[i]) / inv_t));
    return (unsigned)f2bf(expf(z - mx) / s);  // non-negative: the sign bit is clear
  };

  // ---- histogram over the 15-bit pattern
  for (int i = tid; i < HIST_BINS; i += SAMPLE_THREADS) hist[i] = 0u;
  __syncthreads();
  for (int i = tid; i < vocab; i += SAMPLE_THREADS) atomicAdd(&hist[prob_bits(i) & 0x7fffu], 1u);
  __syncthreads();

  // ---- walk the values from the largest down: thread t owns HIST_BINS / 1024 = 32 consecutive patterns
  constexpr int PER = HIST_BINS / SAMPLE_THREADS;
  const int top_pat = HIST_BINS - 1 - tid * PER;  // this thread's largest pattern
  float mass = 0.f;
  int cnt = 0, my_top = 0;  // FILTER: this thread's tokens of positive probability, its largest occupied pattern
  for (int k = 0; k < PER; ++k) {
    const int pat = top_pat - k;
    if (hist[pat]) mass += (float)hist[pat] * bf2f((bf16_t)pat);  // empty patterns include inf / NaN encodings
    if (FILTER && hist[pat] && bf2f((bf16_t)pat) > 0.f) {  // the patterns the second walk visits
      cnt += (int)hist[pat];
      if (my_top == 0) my_top = pat;
    }
  }
  if (FILTER && my_top > 0) atomicMax(&shared_i[5], my_top);
  // exclusive prefix over threads (descending value order == ascending tid)
  float before = block_inclusive_scan<SAMPLE_THREADS>(mass, scan) - mass;  // mass of all strictly larger values owned by earlier threads
  int cnt_before = 0;               // FILTER: tokens of all strictly larger values owned by earlier threads
  if (FILTER) {
    // the count's exclusive prefix: a shuffle scan per wave, then the 16 wave totals through `red` (free since block_sum)
    const int incl = wave_inclusive_scan(cnt);
    int* wave_cnt = (int*)red;
    if ((tid & 63) == 63) wave_cnt[tid >> 6] = incl;
    __syncthreads();
    cnt_before = incl - cnt;
    for (int w = 0; w < (tid >> 6); ++w) cnt_before += wave_cnt[w];
  }
  if (tid == 0) {
    shared_i[0] = HIST_BINS;  // boundary pattern: the SMALLEST value that still has a surviving token
    shared_i[1] = 0;          // how many tokens of that value survive
    shared_i[3] = -1;         // the drawn token
    shared_i[4] = -1;         // last survivor (fallback when rounding puts the target past the end)
    if (FILTER) {
      shared_i[6] = 0;          // top-k boundary pattern (0: no cut) ...
      shared_i[7] = 0;          // ... and its survivors
      shared_i[8] = HIST_BINS;  // min-p boundary pattern
    }
  }
  __syncthreads();
  // FILTER: the clamps -- k <= 0 or >= vocab is off, m <= 0 (or NaN) is off, m > 1 is 1
  const int k_cut = (FILTER && top_k > 0 && top_k < vocab) ? top_k : 0;
  const bool m_on = FILTER && min_p > 0.f;
  int m_thr = 0;  // pattern of bf16(float(min_p) * p_max): positive bf16 patterns order as their values do
  if (m_on) m_thr = (int)(f2bf(fminf(min_p, 1.f) * bf2f((bf16_t)shared_i[5])) & 0x7fffu);
  // `before` only grows as the values descend, so the values with survivors form a prefix of the
  // descending order and every value above the boundary survives whole
  int my_b = HIST_BINS, my_n = 0, my_m = HIST_BINS;
  const float tp16 = bf2f(f2bf(top_p));
  for (int k = 0; k < PER; ++k) {
    const int pat = top_pat - k;
    const unsigned c = hist[pat];
    const float v = bf2f((bf16_t)pat);
    if (c > 0u && v > 0.f) {
      // token j of this value (j = 0..c-1): the reference's cumsum is an fp32 running sum rounded to
      // bf16 per element, the subtraction and the comparison are bf16 too (the python scalar top_p is
      // cast to bf16):  keep iff  bf16(bf16(before + (j+1) v) - v) <= bf16(top_p).  Monotone in j.
      auto kept = [&](int j) { return bf2f(f2bf(bf2f(f2bf(before + (float)(j + 1) * v)) - v)) <= tp16; };
      if (kept(0)) {
        int lo = 0, hi = (int)c - 1;  // largest j that is kept
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (kept(mid)) lo = mid; else hi = mid - 1;
        }
        my_b = pat;
        my_n = lo + 1;
      }
      if (FILTER) {
        if (k_cut && cnt_before < k_cut && cnt_before + (int)c >= k_cut) {  // one pattern at most: the count only grows
          shared_i[6] = pat;
          shared_i[7] = k_cut - cnt_before;
        }
        cnt_before += (int)c;
        if (m_on && pat >= m_thr) my_m = pat;  // descending walk: ends at this thread's smallest such pattern
      }
    }
    if (c) before += (float)c * v;
  }
  if (my_b < HIST_BINS) atomicMin(&shared_i[0], my_b);
  if (FILTER && my_m < HIST_BINS) atomicMin(&shared_i[8], my_m);
  __syncthreads();
  const int tp_pat = shared_i[0];
  if (my_b == tp_pat && tp_pat < HIST_BINS) shared_i[1] = my_n;  // every pattern has exactly one owner
  __syncthreads();
  int bpat = tp_pat, n_boundary = shared_i[1];
  if (FILTER) {  // the same values in every thread: the largest boundary, the smallest count inside it
    const int k_pat = shared_i[6], k_n = shared_i[7];
    if (k_pat > bpat || (k_pat == bpat && k_n < n_boundary)) {
      bpat = k_pat;
      n_boundary = k_n;
    }
    if (m_on) {
      const int m_pat = shared_i[8];  // (an occupied pattern, or HIST_BINS: nothing reaches the threshold, nothing survives)
      const int m_n = m_pat < HIST_BINS ? (int)hist[m_pat] : 0;
      if (m_pat > bpat || (m_pat == bpat && m_n < n_boundary)) {
        bpat = m_pat;
        n_boundary = m_n;
      }
    }
  }

  // ---- survivors: pattern > bpat, or pattern == bpat and among its n_boundary lowest ids (e: the equal tokens before).
  // Contiguous chunks per thread keep id order; two block scans (equal-count, kept mass).
  auto survives = [&](int pat, int& e) {
    bool keep = pat > bpat;
    if (pat == bpat) keep = (e++ < n_boundary);
    return keep;
  };
  const int chunk = (vocab + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
  const int i0 = tid * chunk, i1 = min(vocab, i0 + chunk);
  int eq = 0;
  for (int i = i0; i < i1; ++i) eq += ((int)(prob_bits(i) & 0x7fffu) == bpat);
  __syncthreads();
  const int eq_before = block_inclusive_scan<SAMPLE_THREADS>(eq, (int*)scan) - eq;
  __syncthreads();
  // kept mass (sum of the surviving bf16 probabilities, fp32)
  float kept = 0.f;
  {
    int e = eq_before;
    for (int i = i0; i < i1; ++i) {
      const int pat = (int)(prob_bits(i) & 0x7fffu);
      if (survives(pat, e)) kept += bf2f((bf16_t)pat);
    }
  }
  const float total = block_sum(kept, red);
  const float denom = bf2f(f2bf(total));  // probs_sort.sum(): a bf16 tensor
  // renormalised probabilities bf16(p / denom); chunk masses for the draw
  float cm = 0.f;
  {
    int e = eq_before;
    for (int i = i0; i < i1; ++i) {
      const int pat = (int)(prob_bits(i) & 0x7fffu);
      const bf16_t q = survives(pat, e) ? f2bf(bf2f((bf16_t)pat) / denom) : (bf16_t)0;
      if (pr) pr[i] = q;
      cm += bf2f(q);
    }
  }
  __syncthreads();
  const float hi = block_inclusive_scan<SAMPLE_THREADS>(cm, scan);
  const float all = scan[SAMPLE_THREADS - 1];
  const float target = *u * all;
  const float lo = hi - cm;
  int last = -1;
  {
    float acc = lo;
    int e = eq_before, pick = -1;
    const bool mine = cm > 0.f && target >= lo && target < hi;
    for (int i = i0; i < i1; ++i) {
      const int pat = (int)(prob_bits(i) & 0x7fffu);
      if (!survives(pat, e)) continue;
      last = i;
      if (mine && pick < 0) {
        acc += bf2f(f2bf(bf2f((bf16_t)pat) / denom));
        if (target < acc) pick = i;
      }
    }
    if (mine) shared_i[3] = pick >= 0 ? pick : last;  // the intervals [lo, hi) partition [0, all): one owner
  }
  if (last >= 0) atomicMax(&shared_i[4], last);
  __syncthreads();
  if (tid == 0) *next = shared_i[3] >= 0 ? shared_i[3] : (shared_i[4] > 0 ? shared_i[4] : 0);
}

// greedy row: argmax with lr[suppress] as -inf, ties -> lowest id, an all-NaN row -> 0: block_argmax (row_reduce.hpp), which
// argmax_kernel (elementwise.hip) ends in too.  Plain 2-byte loads: no alignment demand on vocab or the row stride.
__device__ __forceinline__ void argmax_row(char* smem, const bf16_t* __restrict__ lr, int vocab, int suppress,
                                           int32_t* __restrict__ next) {
  float* sv = (float*)smem;  // [16] wave partials
  int* si = (int*)(sv + 16);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < vocab; i += SAMPLE_THREADS)  // ascending ids per thread: a later equal value never replaces
    argmax_take(best, bi, (i == suppress) ? -INFINITY : bf2f(lr[i]), i);
  bi = block_argmax<SAMPLE_THREADS / 64>(best, bi, vocab, sv, si);
  if (threadIdx.x == 0) *next = bi;
}

// One kernel for the three entries.  SETTING is how temperature and top_p arrive: float (md_sample_top_p), one value with
// which every row is sampled, or const float*, one per row: temperature[b] > 0 samples the row with (temperature[b],
// top_p[b], uniforms[b]), == 0 takes its argmax, < 0 leaves the row alone.  One load decides for the whole workgroup,
// before any barrier.
// FILTER (md_sample_rows_filtered) adds two per-row settings, top_k[b] (int32) and min_p[b] (fp32): a sampled row is also
// cut to its first top_k[b] tokens and to the tokens of probability >= bf16(min_p[b] * p_max) (sample_top_p_row<true>).  A
// row of top_k[b] <= 0 (or >= vocab) and min_p[b] <= 0 carries the bits of the unfiltered kernel; greedy and idle rows read
// neither, and without FILTER the two pointers are never read.
template <bool FILTER, class SETTING>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(const bf16_t* __restrict__ logits, int64_t ld, int vocab,
                                                                int suppress, SETTING temperature, SETTING top_p,
                                                                const float* __restrict__ uniforms, int32_t* __restrict__ next,
                                                                bf16_t* __restrict__ probs_out, int64_t ldp,
                                                                const int32_t* __restrict__ top_k, const float* __restrict__ min_p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  const bf16_t* lr = logits + (int64_t)b * ld;
  float t, p;
  if constexpr (std::is_pointer<SETTING>::value) {
    t = temperature[b];
    if (t < 0.f) return;  // idle: next[b], the probs_out row and the row's logits stay untouched
    if (t == 0.f) {
      argmax_row(smem, lr, vocab, suppress, next + b);
      return;
    }
    p = top_p[b];
  } else {
    t = temperature;
    p = top_p;
  }
  sample_top_p_row<FILTER>(smem, lr, vocab, suppress, t, p, uniforms + b, next + b,
                           probs_out ? probs_out + (int64_t)b * ldp : nullptr, FILTER ? top_k[b] : 0, FILTER ? min_p[b] : 0.f);
}

// the entries' launch: the instantiation's dynamic-LDS limit, then one workgroup per row
template <bool FILTER, class SETTING>
md_status launch_sample(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id, SETTING temperature,
                        SETTING top_p, const float* uniforms, int32_t* next, void* probs_out, int64_t ld_probs,
                        const int32_t* top_k, const float* min_p, void* stream) {
  MD_CHECK_ARG(probs_out == nullptr || ld_probs >= vocab);
  MD_TRY(md_ensure_dynamic_lds((const void*)sample_kernel<FILTER, SETTING>, SAMPLE_LDS));
  hipLaunchKernelGGL((sample_kernel<FILTER, SETTING>), dim3(batch), dim3(SAMPLE_THREADS), SAMPLE_LDS, (hipStream_t)stream,
                     (const bf16_t*)logits, ld, vocab, suppress_id, temperature, top_p, uniforms, next, (bf16_t*)probs_out,
                     ld_probs, top_k, min_p);
  return md_launch_status();
}

}  // namespace

extern "C" md_status md_sample_top_p(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id,
                                     float temperature, float top_p, const float* uniforms, int32_t* next,
                                     void* probs_out, int64_t ld_probs, void* stream) {
  MD_CHECK_ARG(logits && uniforms && next && batch > 0 && vocab > 0 && ld >= vocab && temperature > 0.f);
  return launch_sample<false>(logits, ld, batch, vocab, suppress_id, temperature, top_p, uniforms, next, probs_out, ld_probs, nullptr,
                              nullptr, stream);
}

extern "C" md_status md_sample_rows(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id,
                                    const float* temperature, const float* top_p, const float* uniforms, int32_t* next,
                                    void* probs_out, int64_t ld_probs, void* stream) {
  MD_CHECK_ARG(logits && temperature && top_p && uniforms && next && batch > 0 && vocab > 0 && ld >= vocab);
  return launch_sample<false>(logits, ld, batch, vocab, suppress_id, temperature, top_p, uniforms, next, probs_out, ld_probs, nullptr,
                              nullptr, stream);
}

extern "C" md_status md_sample_rows_filtered(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id,
                                             const float* temperature, const float* top_p, const int32_t* top_k,
                                             const float* min_p, const float* uniforms, int32_t* next, void* probs_out,
                                             int64_t ld_probs, void* stream) {
  MD_CHECK_ARG(logits && temperature && top_p && top_k && min_p && uniforms && next && batch > 0 && vocab > 0 && ld >= vocab);
  return launch_sample<true>(logits, ld, batch, vocab, suppress_id, temperature, top_p, uniforms, next, probs_out, ld_probs, top_k,
                             min_p, stream);
}
