// Device-resident pieces of the generation loops above the seam:
//   * the region head's "pick a bin and re-encode it" step of detect / point
//     (reference: moondream.py:672-713 around region.py:12-71), so a points loop over B
//     images needs no host round trip per coordinate;
//   * temperature / top-p sampling (reference: moondream.py:270-278, 313-318, 521-528).
// HBM-bound row kernels: one workgroup per sequence, 16-byte loads, wave shuffles.
#include "text_internal.hpp"

namespace {

// ---------------------------------------------------------------------------
// [cos(f) | sin(f)],  f = bf16( sum_g bf16(2 pi v_g) * W[g][j] )          (region.py:12-29)
// v_g bf16; the K = 1 / K = 2 contraction is an fp32 sum of exact products, rounded once.
__device__ __forceinline__ void fourier_row(const float* v, int n_groups, const bf16_t* __restrict__ w, int half,
                                            bf16_t* __restrict__ out) {
  float t[2];
  for (int g = 0; g < n_groups; ++g) t[g] = bf2f(f2bf(v[g] * 6.283185307179586f));  // 2 * math.pi * x, in bf16
  for (int j = threadIdx.x; j < half; j += blockDim.x) {
    float f = t[0] * bf2f(w[j]);
    if (n_groups == 2) f += t[1] * bf2f(w[half + j]);
    f = bf2f(f2bf(f));
    out[j] = f2bf(cosf(f));
    out[half + j] = f2bf(sinf(f));
  }
}

__global__ __launch_bounds__(256) void fourier_kernel(const bf16_t* __restrict__ x, int64_t ldx, int in_dim,
                                                      const bf16_t* __restrict__ w, int half,
                                                      bf16_t* __restrict__ out, int64_t ldo) {
  const int r = blockIdx.x;
  float v[2] = {bf2f(x[r * ldx]), in_dim == 2 ? bf2f(x[r * ldx + 1]) : 0.f};
  fourier_row(v, in_dim, w, half, out + (int64_t)r * ldo);
}

// one workgroup per sequence: argmax of each 1024-bin group (ties -> lowest index, like
// torch.argmax on the reference's CPU path), value = table[bin], then the Fourier features
__global__ __launch_bounds__(256) void region_pick_kernel(const bf16_t* __restrict__ logits, int64_t ld, int n_groups,
                                                          int n_bins, const bf16_t* __restrict__ table,
                                                          const bf16_t* __restrict__ w, int half,
                                                          int32_t* __restrict__ bins, int64_t ld_bins,
                                                          bf16_t* __restrict__ feats, int64_t ldf) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ float val[2];
  const int b = blockIdx.x;
  for (int g = 0; g < n_groups; ++g) {
    const bf16_t* lr = logits + (int64_t)b * ld + (int64_t)g * n_bins;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n_bins; i += 256) {
      const float x = bf2f(lr[i]);
      if (x > best || (x == best && i < bi)) {
        best = x;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) {
        best = ov;
        bi = oi;
      }
    }
    if ((threadIdx.x & 63) == 0) {
      sv[threadIdx.x >> 6] = best;
      si[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int wv = 1; wv < 4; ++wv)
        if (sv[wv] > best || (sv[wv] == best && si[wv] < bi)) {
          best = sv[wv];
          bi = si[wv];
        }
      if (bi >= n_bins) bi = 0;  // all-NaN row
      bins[(int64_t)b * ld_bins + g] = bi;
      val[g] = bf2f(table[bi]);
    }
    __syncthreads();
  }
  float v[2] = {val[0], n_groups == 2 ? val[1] : 0.f};
  fourier_row(v, n_groups, w, half, feats + (int64_t)b * ldf);
}

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
// nullptr).  The body of both sampling kernels; smem is the workgroup's SAMPLE_LDS bytes.
__device__ __forceinline__ void sample_top_p_row(char* smem, const bf16_t* __restrict__ lr, int vocab, int suppress,
                                                 float temperature, float top_p, const float* __restrict__ u,
                                                 int32_t* __restrict__ next, bf16_t* __restrict__ pr) {
  unsigned* hist = (unsigned*)smem;                    // [HIST_BINS] counts per bf16 bit pattern
  float* red = (float*)(smem + HIST_BINS * 4);         // [16]
  float* scan = red + 16;                              // [SAMPLE_THREADS] block scans
  int* shared_i = (int*)(scan + SAMPLE_THREADS);       // [8] boundary pattern, survivors in it, drawn token, ...
  const int tid = threadIdx.x;
  const float inv_t = temperature;  // division, not a reciprocal multiply: the reference divides

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
  for (int k = 0; k < PER; ++k) {
    const int pat = top_pat - k;
    if (hist[pat]) mass += (float)hist[pat] * bf2f((bf16_t)pat);  // empty patterns include inf / NaN encodings
  }
  // exclusive prefix over threads (descending value order == ascending tid)
  scan[tid] = mass;
  __syncthreads();
  for (int off = 1; off < SAMPLE_THREADS; off <<= 1) {
    const float add = (tid >= off) ? scan[tid - off] : 0.f;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  float before = scan[tid] - mass;  // mass of all strictly larger values owned by earlier threads
  if (tid == 0) {
    shared_i[0] = HIST_BINS;  // boundary pattern: the SMALLEST value that still has a surviving token
    shared_i[1] = 0;          // how many tokens of that value survive
    shared_i[3] = -1;         // the drawn token
    shared_i[4] = -1;         // last survivor (fallback when rounding puts the target past the end)
  }
  __syncthreads();
  // `before` only grows as the values descend, so the values with survivors form a prefix of the
  // descending order and every value above the boundary survives whole
  int my_b = HIST_BINS, my_n = 0;
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
    }
    if (c) before += (float)c * v;
  }
  if (my_b < HIST_BINS) atomicMin(&shared_i[0], my_b);
  __syncthreads();
  const int bpat = shared_i[0];
  if (my_b == bpat && bpat < HIST_BINS) shared_i[1] = my_n;  // every pattern has exactly one owner
  __syncthreads();
  const int n_boundary = shared_i[1];

  // ---- survivors: pattern > bpat, or pattern == bpat and among its n_boundary lowest ids.
  // Contiguous chunks per thread keep id order; two block scans (equal-count, kept mass).
  const int chunk = (vocab + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
  const int i0 = tid * chunk, i1 = min(vocab, i0 + chunk);
  int eq = 0;
  for (int i = i0; i < i1; ++i) eq += ((int)(prob_bits(i) & 0x7fffu) == bpat);
  int* iscan = (int*)scan;
  __syncthreads();
  iscan[tid] = eq;
  __syncthreads();
  for (int off = 1; off < SAMPLE_THREADS; off <<= 1) {
    const int add = (tid >= off) ? iscan[tid - off] : 0;
    __syncthreads();
    iscan[tid] += add;
    __syncthreads();
  }
  int eq_before = iscan[tid] - eq;
  __syncthreads();
  // kept mass (sum of the surviving bf16 probabilities, fp32)
  float kept = 0.f;
  {
    int e = eq_before;
    for (int i = i0; i < i1; ++i) {
      const int pat = (int)(prob_bits(i) & 0x7fffu);
      bool keep = pat > bpat;
      if (pat == bpat) keep = (e++ < n_boundary);
      if (keep) kept += bf2f((bf16_t)pat);
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
      bool keep = pat > bpat;
      if (pat == bpat) keep = (e++ < n_boundary);
      const bf16_t q = keep ? f2bf(bf2f((bf16_t)pat) / denom) : (bf16_t)0;
      if (pr) pr[i] = q;
      cm += bf2f(q);
    }
  }
  __syncthreads();
  scan[tid] = cm;
  __syncthreads();
  for (int off = 1; off < SAMPLE_THREADS; off <<= 1) {
    const float add = (tid >= off) ? scan[tid - off] : 0.f;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const float all = scan[SAMPLE_THREADS - 1];
  const float target = *u * all;
  const float lo = scan[tid] - cm;
  int last = -1;
  {
    float acc = lo;
    int e = eq_before, pick = -1;
    const bool mine = cm > 0.f && target >= lo && target < scan[tid];
    for (int i = i0; i < i1; ++i) {
      const int pat = (int)(prob_bits(i) & 0x7fffu);
      bool keep = pat > bpat;
      if (pat == bpat) keep = (e++ < n_boundary);
      if (!keep) continue;
      last = i;
      if (mine && pick < 0) {
        acc += bf2f(f2bf(bf2f((bf16_t)pat) / denom));
        if (target < acc) pick = i;
      }
    }
    if (mine) shared_i[3] = pick >= 0 ? pick : last;  // the intervals [lo, scan) partition [0, all): one owner
  }
  if (last >= 0) atomicMax(&shared_i[4], last);
  __syncthreads();
  if (tid == 0) *next = shared_i[3] >= 0 ? shared_i[3] : (shared_i[4] > 0 ? shared_i[4] : 0);
}

// greedy row: argmax with lr[suppress] as -inf, ties -> lowest id, an all-NaN row -> 0 (argmax_kernel's rule, elementwise.hip).
// Plain 2-byte loads: no alignment demand on vocab or the row stride.
__device__ __forceinline__ void argmax_row(char* smem, const bf16_t* __restrict__ lr, int vocab, int suppress,
                                           int32_t* __restrict__ next) {
  float* sv = (float*)smem;  // [16] wave partials
  int* si = (int*)(sv + 16);
  const int tid = threadIdx.x;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < vocab; i += SAMPLE_THREADS) {  // ascending ids per thread: a later equal value never replaces
    const float v = (i == suppress) ? -INFINITY : bf2f(lr[i]);
    if (v > best || (v == best && i < bi)) {
      best = v;
      bi = i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    sv[tid >> 6] = best;
    si[tid >> 6] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SAMPLE_THREADS / 64; ++w)
      if (sv[w] > best || (sv[w] == best && si[w] < bi)) {
        best = sv[w];
        bi = si[w];
      }
    *next = (bi >= vocab) ? 0 : bi;
  }
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_top_p_kernel(const bf16_t* __restrict__ logits, int64_t ld, int vocab,
                                                                      int suppress, float temperature, float top_p,
                                                                      const float* __restrict__ uniforms,
                                                                      int32_t* __restrict__ next,
                                                                      bf16_t* __restrict__ probs_out, int64_t ldp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  sample_top_p_row(smem, logits + (int64_t)b * ld, vocab, suppress, temperature, top_p, uniforms + b, next + b,
                   probs_out ? probs_out + (int64_t)b * ldp : nullptr);
}

// per-row settings: temperature[b] > 0 samples the row with (temperature[b], top_p[b], uniforms[b]), == 0 takes its argmax,
// < 0 leaves the row alone.  One load decides for the whole workgroup, before any barrier.
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_rows_kernel(const bf16_t* __restrict__ logits, int64_t ld, int vocab,
                                                                     int suppress, const float* __restrict__ temperature,
                                                                     const float* __restrict__ top_p,
                                                                     const float* __restrict__ uniforms,
                                                                     int32_t* __restrict__ next,
                                                                     bf16_t* __restrict__ probs_out, int64_t ldp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  const float t = temperature[b];
  if (t < 0.f) return;  // idle: next[b], the probs_out row and the row's logits stay untouched
  const bf16_t* lr = logits + (int64_t)b * ld;
  if (t == 0.f) {
    argmax_row(smem, lr, vocab, suppress, next + b);
    return;
  }
  sample_top_p_row(smem, lr, vocab, suppress, t, top_p[b], uniforms + b, next + b,
                   probs_out ? probs_out + (int64_t)b * ldp : nullptr);
}

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
  const int sup = (suppress_id >= 0 && (suppress_rows == nullptr || suppress_rows[r] != 0)) ? suppress_id : -1;
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
  if ((tid & 63) == 0) {
    red_max[tid >> 6] = mx;
    red_cnt[tid >> 6] = cnt;
  }
  __syncthreads();
  mx = red_max[tid & 15];  // every 16 consecutive lanes hold the 16 wave partials
  cnt = red_cnt[tid & 15];
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }

  // ---- pass 2: s = sum over live v of exp(x[v] - m), in the order documented above
  float s = 0.f;
  for (int i = tid; i < vocab; i += LOGPROB_THREADS) {
    if (i == sup) continue;
    s += expf(bf2f(lr[i]) - mx);
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) red_sum[tid >> 6] = s;
  __syncthreads();
  s = red_sum[tid & 15];
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);

  if (tid == 0) {
    logprob[r] = (xt - mx) - logf(s);
    if (rank) rank[r] = cnt;
  }
}

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

extern "C" md_status md_fourier_features(const void* x, int64_t ldx, int32_t rows, int32_t in_dim, const void* w,
                                         int32_t half, void* out, int64_t ld_out, void* stream) {
  MD_CHECK_ARG(x && w && out && rows > 0 && (in_dim == 1 || in_dim == 2) && half > 0 && ld_out >= 2 * half && ldx >= in_dim);
  hipLaunchKernelGGL(fourier_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, in_dim,
                     (const bf16_t*)w, half, (bf16_t*)out, ld_out);
  return md_launch_status();
}

extern "C" md_status md_region_pick_encode(const void* logits, int64_t ld, int32_t batch, int32_t n_groups,
                                           int32_t n_bins, const void* value_table, const void* feat_w, int32_t half,
                                           int32_t* bins, int64_t ld_bins, void* feats, int64_t ld_feats, void* stream) {
  MD_CHECK_ARG(logits && value_table && feat_w && bins && feats && batch > 0 && n_bins > 0);
  MD_CHECK_ARG((n_groups == 1 || n_groups == 2) && ld >= (int64_t)n_groups * n_bins && ld_bins >= n_groups && ld_feats >= 2 * half);
  hipLaunchKernelGGL(region_pick_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits, ld, n_groups,
                     n_bins, (const bf16_t*)value_table, (const bf16_t*)feat_w, half, bins, ld_bins, (bf16_t*)feats, ld_feats);
  return md_launch_status();
}

extern "C" md_status md_sample_top_p(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id,
                                     float temperature, float top_p, const float* uniforms, int32_t* next,
                                     void* probs_out, int64_t ld_probs, void* stream) {
  MD_CHECK_ARG(logits && uniforms && next && batch > 0 && vocab > 0 && ld >= vocab && temperature > 0.f);
  MD_CHECK_ARG(probs_out == nullptr || ld_probs >= vocab);
  MD_TRY(md_ensure_dynamic_lds((const void*)sample_top_p_kernel, SAMPLE_LDS));
  hipLaunchKernelGGL(sample_top_p_kernel, dim3(batch), dim3(SAMPLE_THREADS), SAMPLE_LDS, (hipStream_t)stream, (const bf16_t*)logits,
                     ld, vocab, suppress_id, temperature, top_p, uniforms, next, (bf16_t*)probs_out, ld_probs);
  return md_launch_status();
}

extern "C" md_status md_sample_rows(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id,
                                    const float* temperature, const float* top_p, const float* uniforms, int32_t* next,
                                    void* probs_out, int64_t ld_probs, void* stream) {
  MD_CHECK_ARG(logits && temperature && top_p && uniforms && next && batch > 0 && vocab > 0 && ld >= vocab);
  MD_CHECK_ARG(probs_out == nullptr || ld_probs >= vocab);
  MD_TRY(md_ensure_dynamic_lds((const void*)sample_rows_kernel, SAMPLE_LDS));
  hipLaunchKernelGGL(sample_rows_kernel, dim3(batch), dim3(SAMPLE_THREADS), SAMPLE_LDS, (hipStream_t)stream, (const bf16_t*)logits,
                     ld, vocab, suppress_id, temperature, top_p, uniforms, next, (bf16_t*)probs_out, ld_probs);
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
