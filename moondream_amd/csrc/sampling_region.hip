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

// region_pick_kernel with a confidence per group (md_region_pick_encode_scored).  The pick is region_pick_kernel's own,
// statement for statement (a kernel of its own: the reasoning step bakes region_pick_kernel into captured graphs), so bins
// and features are bit-identical: ties -> lowest bin, an all-NaN group -> bin 0.  Then, per group, with m = x[pick] (the
// group's maximum) in fp32 from the bf16 logits x:
//   S = sum over all bins i of exp(x_i - m),   W = the same sum over the bins with |i - pick| <= window (clamped to the group),
//   logprobs[b][g] = log(W) - log(S).
// The group (2 KB at 1024 bins) is read twice, once for the pick and once for the sums, the second time from L2.
// Summation order, a function of n_bins alone (never of the row or the row count), the same for S and for W:
//   1. thread tid adds its strided share exp(x[tid + k * 256] - m), k = 0, 1, .. ascending, sequentially in fp32
//      (n_t = ceil(n_bins / 256) terms: 4 at 1024 bins); W adds the term itself inside the window and +0.0f outside it;
//   2. a 6-level xor butterfly over the wave's 64 lanes (offsets 32, 16, .., 1);
//   3. thread 0 adds the 4 wave partials in wave order, ((p0 + p1) + p2) + p3.
// So every term passes through at most (n_t - 1) + 6 + 3 additions.  Adding +0.0f changes nothing, so W is the fp32 sum of
// the window's terms in S's order: with window = 0 it is exp(0) = 1 and the value is the log-softmax of the pick; with a
// window that covers the group W and S are the same sequence of operations on the same numbers and the value is exactly
// 0.0f.  A -inf logit adds exp(-inf) = 0.  A NaN in the group makes S, and the value, NaN (the pick skips it); so does a
// group whose maximum is not finite.  Plain 2-byte loads: no alignment demand on n_bins or the strides.
__global__ __launch_bounds__(256) void region_pick_scored_kernel(const bf16_t* __restrict__ logits, int64_t ld, int n_groups,
                                                                 int n_bins, const bf16_t* __restrict__ table,
                                                                 const bf16_t* __restrict__ w, int half,
                                                                 int32_t* __restrict__ bins, int64_t ld_bins,
                                                                 bf16_t* __restrict__ feats, int64_t ldf, int window,
                                                                 float* __restrict__ logprobs, int64_t ld_lp) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ float val[2];
  __shared__ int picked;
  __shared__ float part_s[4];
  __shared__ float part_w[4];
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
      picked = bi;
    }
    __syncthreads();
    // ---- the sums, in the order documented above
    const int pick = picked;
    const float m = bf2f(lr[pick]);
    const int lo = pick - min(window, pick), hi = pick + min(window, n_bins - 1 - pick);  // no overflow for any window >= 0
    float s = 0.f, ws = 0.f;
    for (int i = threadIdx.x; i < n_bins; i += 256) {
      const float e = expf(bf2f(lr[i]) - m);
      s = __fadd_rn(s, e);  // never fused with expf's last multiply: S and W add the same rounded term
      ws = __fadd_rn(ws, (i >= lo && i <= hi) ? e : 0.f);
    }
    s = wave_sum(s);
    ws = wave_sum(ws);
    if ((threadIdx.x & 63) == 0) {
      part_s[threadIdx.x >> 6] = s;
      part_w[threadIdx.x >> 6] = ws;
    }
    __syncthreads();  // (also: every thread has read `picked` before thread 0 rewrites it for the next group)
    if (threadIdx.x == 0) {
      const float st = ((part_s[0] + part_s[1]) + part_s[2]) + part_s[3];
      const float wt = ((part_w[0] + part_w[1]) + part_w[2]) + part_w[3];
      logprobs[(int64_t)b * ld_lp + g] = logf(wt) - logf(st);
    }
  }
  float v[2] = {val[0], n_groups == 2 ? val[1] : 0.f};
  fourier_row(v, n_groups, w, half, feats + (int64_t)b * ldf);
}

// ---------------------------------------------------------------------------
// Spatial references of a batch of prompts (reference: region.py:96-136 + moondream.py:293-301): every reference
// TOKEN of a call -- a coordinate (one value, coord_encoder) or a size (two values, size_encoder) -- is encoded and
// stored into its row of the prompt embeddings in ONE launch.
//   feat = fourier_row(values)                       (bf16, in LDS: md_fourier_features' bits)
//   emb[dst][n] = bf16(bias[n] + sum_k feat[k] * W[n][k])                 (fp32)
// A workgroup owns SREF_TOKENS descriptors and SREF_COLS output columns, so an encoder row is fetched once per 16
// tokens.  A wave takes 16 of the columns, one at a time: its 64 lanes split K (4 consecutive k per lane and trip of
// 256), each lane keeps one partial sum per token, and a halving butterfly (lane ^ 32, 16, 8, 4: half of the tokens
// stay on either side; then ^ 2, ^ 1) leaves token (lane >> 2)'s total on its four lanes.  The order of every
// addition is a function of K alone: fp32 addition commutes, so which side of an exchange a token stays on -- its
// place in the group -- does not change a bit, and neither do the table's length, the token's index or dst.
constexpr int SREF_TOKENS = 16;
constexpr int SREF_COLS = 64;
constexpr int SREF_THREADS = 256;

struct SpatialRefArgs {
  const int32_t* desc;  // [n][4]: dst, kind (0 coordinate, 1 size), value bits, value bits
  int n;
  const bf16_t *fw0, *w0, *b0, *fw1, *w1, *b1;  // Fourier matrix, encoder, bias of either kind
  int feat0, feat1, feat_max;
  int64_t ldw0, ldw1;
  int dim;
  bf16_t* emb;
  int64_t ld, dst0;
  int rows;
};

template <int H>
__device__ __forceinline__ void sref_fold(const float* in, float* out, int lane) {
  const bool hi = (lane & (4 * H)) != 0;  // H = 8, 4, 2, 1 tokens kept: lanes ^ 32, 16, 8, 4
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const float keep = hi ? in[j + H] : in[j];
    const float send = hi ? in[j] : in[j + H];
    out[j] = keep + __shfl_xor(send, 4 * H, 64);
  }
}

__global__ __launch_bounds__(SREF_THREADS) void spatial_ref_embed_kernel(SpatialRefArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16_t sref_feat[];  // [SREF_TOKENS][feat_max]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = blockIdx.x * SREF_TOKENS;
  const int nt = min(SREF_TOKENS, a.n - t0);
  const int4* desc = reinterpret_cast<const int4*>(a.desc) + t0;

  // zero fill: every LDS word a pass reads is defined.  In the pass of the OTHER kind a token's row holds what it has
  // (a coordinate's features then zeros; the head of a size's features): that lane sum is meaningless and is never
  // stored -- only tokens of the pass's kind (`live`) store.
  for (int i = tid; i < SREF_TOKENS * a.feat_max / 8; i += SREF_THREADS) reinterpret_cast<uint4*>(sref_feat)[i] = uint4{0, 0, 0, 0};
  __syncthreads();
  unsigned live0 = 0u, live1 = 0u;  // the group's tokens of either kind whose destination lies inside the tensor
  for (int t = 0; t < nt; ++t) {
    const int4 d = desc[t];  // the same for every thread
    const int64_t row = (int64_t)d.x - a.dst0;
    if ((d.y != 0 && d.y != 1) || row < 0 || row >= a.rows) continue;
    if (d.y) live1 |= 1u << t; else live0 |= 1u << t;
    const float v[2] = {bf2f((bf16_t)d.z), bf2f((bf16_t)d.w)};
    fourier_row(v, d.y + 1, d.y ? a.fw1 : a.fw0, (d.y ? a.feat1 : a.feat0) / 2, sref_feat + t * a.feat_max);
  }
  __syncthreads();

  const int slot = lane >> 2, part = lane & 3;                       // after the butterfly: the lane's token, and
  const int col4 = blockIdx.y * SREF_COLS + wave * 16 + part * 4;    // the four columns it stores
  for (int p = 0; p < 2; ++p) {
    const unsigned live = p ? live1 : live0;
    if (!live) continue;
    const bf16_t* w = p ? a.w1 : a.w0;
    const int64_t ldw = p ? a.ldw1 : a.ldw0;
    const int K = p ? a.feat1 : a.feat0;
    float res[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      res[i] = 0.f;
      for (int c = 0; c < 4; ++c) {
        const int col = blockIdx.y * SREF_COLS + wave * 16 + c * 4 + i;  // the same for the whole wave
        float acc[SREF_TOKENS];
#pragma unroll
        for (int t = 0; t < SREF_TOKENS; ++t) acc[t] = 0.f;
        if (col < a.dim) {
          for (int k0 = lane * 4; k0 < K; k0 += 256) {
            const uint2 wv = *reinterpret_cast<const uint2*>(w + (int64_t)col * ldw + k0);
            const float wk[4] = {bf2f((bf16_t)(wv.x & 0xffffu)), bf2f((bf16_t)(wv.x >> 16)), bf2f((bf16_t)(wv.y & 0xffffu)),
                                 bf2f((bf16_t)(wv.y >> 16))};
#pragma unroll
            for (int t = 0; t < SREF_TOKENS; ++t) {
              const uint2 fv = *reinterpret_cast<const uint2*>(sref_feat + t * a.feat_max + k0);
              acc[t] += bf2f((bf16_t)(fv.x & 0xffffu)) * wk[0];
              acc[t] += bf2f((bf16_t)(fv.x >> 16)) * wk[1];
              acc[t] += bf2f((bf16_t)(fv.y & 0xffffu)) * wk[2];
              acc[t] += bf2f((bf16_t)(fv.y >> 16)) * wk[3];
            }
          }
        }
        float a8[8], a4[4], a2[2], a1[1];
        sref_fold<8>(acc, a8, lane);
        sref_fold<4>(a8, a4, lane);
        sref_fold<2>(a4, a2, lane);
        sref_fold<1>(a2, a1, lane);
        float s = a1[0];
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 1, 64);
        if (part == c) res[i] = s;
      }
    }
    if (((live >> slot) & 1u) && col4 < a.dim) {  // dim % 4 == 0: four columns are inside together
      const bf16_t* b = (p ? a.b1 : a.b0) + col4;
      const uint2 bv = *reinterpret_cast<const uint2*>(b);
      const float o0 = bf2f((bf16_t)(bv.x & 0xffffu)) + res[0], o1 = bf2f((bf16_t)(bv.x >> 16)) + res[1];
      const float o2 = bf2f((bf16_t)(bv.y & 0xffffu)) + res[2], o3 = bf2f((bf16_t)(bv.y >> 16)) + res[3];
      uint2 o;
      o.x = (uint32_t)f2bf(o0) | ((uint32_t)f2bf(o1) << 16);
      o.y = (uint32_t)f2bf(o2) | ((uint32_t)f2bf(o3) << 16);
      const int64_t row = (int64_t)desc[slot].x - a.dst0;
      *reinterpret_cast<uint2*>(a.emb + row * a.ld + col4) = o;
    }
  }
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
// nullptr).  The body of the sampling kernels; smem is the workgroup's SAMPLE_LDS bytes.
// FILTER (md_sample_rows_filtered): two more cuts of the same descending order, each a pair (boundary pattern, survivors
// inside it) like the top-p cut, all three taken on the same unrenormalised p:
//   top_k > 0 and < vocab: the first top_k tokens -- the walk carries a token COUNT next to the mass; the boundary is the
//     pattern at which the running count reaches top_k, of which top_k - (count above it) tokens survive;
//   min_p > 0: the tokens with p >= bf16(min_p * p_max) -- the boundary is the smallest occupied pattern >= that
//     threshold's, kept whole (p_max: the largest occupied pattern, so the best token always survives).
// The row's boundary is the LARGEST of the three patterns (the shortest prefix); where cuts share it, the smallest
// survivor count.  With FILTER false nothing of this is compiled: the two older kernels are what they were.
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
  scan[tid] = mass;
  __syncthreads();
  for (int off = 1; off < SAMPLE_THREADS; off <<= 1) {
    const float add = (tid >= off) ? scan[tid - off] : 0.f;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  float before = scan[tid] - mass;  // mass of all strictly larger values owned by earlier threads
  int cnt_before = 0;               // FILTER: tokens of all strictly larger values owned by earlier threads
  if (FILTER) {
    // the count's exclusive prefix: a shuffle scan per wave, then the 16 wave totals through `red` (free since block_sum)
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if ((tid & 63) >= o) incl += v;
    }
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
  sample_top_p_row<false>(smem, logits + (int64_t)b * ld, vocab, suppress, temperature, top_p, uniforms + b, next + b,
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
  sample_top_p_row<false>(smem, lr, vocab, suppress, t, top_p[b], uniforms + b, next + b,
                          probs_out ? probs_out + (int64_t)b * ldp : nullptr);
}

// sample_rows_kernel with two more per-row settings, top_k[b] (int32) and min_p[b] (fp32): a sampled row is also cut to
// its first top_k[b] tokens and to the tokens of probability >= bf16(min_p[b] * p_max) (sample_top_p_row<true>).  A row of
// top_k[b] <= 0 (or >= vocab) and min_p[b] <= 0 carries the bits of sample_rows_kernel; greedy and idle rows read neither.
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_rows_filtered_kernel(
    const bf16_t* __restrict__ logits, int64_t ld, int vocab, int suppress, const float* __restrict__ temperature,
    const float* __restrict__ top_p, const int32_t* __restrict__ top_k, const float* __restrict__ min_p,
    const float* __restrict__ uniforms, int32_t* __restrict__ next, bf16_t* __restrict__ probs_out, int64_t ldp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  const float t = temperature[b];
  if (t < 0.f) return;  // idle: next[b], the probs_out row and the row's logits stay untouched
  const bf16_t* lr = logits + (int64_t)b * ld;
  if (t == 0.f) {
    argmax_row(smem, lr, vocab, suppress, next + b);
    return;
  }
  sample_top_p_row<true>(smem, lr, vocab, suppress, t, top_p[b], uniforms + b, next + b,
                         probs_out ? probs_out + (int64_t)b * ldp : nullptr, top_k[b], min_p[b]);
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
// The k live tokens of lowest md_token_logprobs rank per row, with their log-probabilities (md_topk_logprobs): entry j is
// the live token of rank j (greater logit first, equal logits by lower id).  m and s are token_logprobs_kernel's, in its
// summation order, so a value here is that kernel's value for the same token, bit for bit.
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
    unsigned incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(incl, o, 64);
      if (tid >= o) incl += v;
    }
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
  mx = wave_max(mx);
  if ((tid & 63) == 0) red_max[tid >> 6] = mx;
  topk_find_digit(hist, cnt, k, found);  // (its first barrier orders red_max too)
  mx = red_max[tid & 15];
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
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
  s = wave_sum(s);
  if ((tid & 63) == 0) red_sum[tid >> 6] = s;
  topk_find_digit(hist, cnt, n_take - above_hi, found);
  s = red_sum[tid & 15];
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
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
      int incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if ((tid & 63) >= o) incl += v;
      }
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
  const int sup = (suppress_id >= 0 && (suppress_rows == nullptr || suppress_rows[r] != 0)) ? suppress_id : -1;
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
  const int sup = (suppress_id >= 0 && (suppress_rows == nullptr || suppress_rows[lrow] != 0)) ? suppress_id : -1;
  topk_row(logits + (int64_t)lrow * ld, vocab, sup, k, out_id, out_lp);
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

// ---------------------------------------------------------------------------
// Repetition / presence / frequency penalties from each row's own history of generated tokens (md_penalize_rows).
// One workgroup per row.  The row's token is appended to its history, then every DISTINCT token of the history is found
// once, with its count, through an open-addressing hash table in LDS: each thread inserts its strided share of the
// history (atomicCAS claims a key, atomicAdd counts it), and after a barrier each occupied entry is one token's update.
// The table has at least twice as many entries as the history has tokens (a power of two chosen from the row's length, so
// the clear and the scan cost what the history holds, not what it could hold): a probe sequence always ends.
// Global traffic: the history's tokens (4 B each) and one 2-byte load and store per distinct token -- never the row.
namespace {
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
  const int slot = slots ? slots[r] : slot0 + r;
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
}  // namespace

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
namespace {
constexpr int CONSTRAIN_THREADS = 256;
constexpr bf16_t BF16_NEG_INF = 0xFF80;

__global__ __launch_bounds__(CONSTRAIN_THREADS) void constrain_rows_kernel(
    bf16_t* __restrict__ logits, int64_t ld, int vocab, const int32_t* __restrict__ tokens_in, const int32_t* __restrict__ slots,
    int slot0, int32_t* state, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ default_next,
    const int32_t* __restrict__ edge_tok, const int32_t* __restrict__ edge_next, int state_cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned constrain_allowed[];  // [ceil(vocab / 32)] bit v: token v allowed
  const int r = blockIdx.x, tid = threadIdx.x;
  const int slot = slots ? slots[r] : slot0 + r;
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

// internal (beam.hip): the row phase of md_beam_select
md_status md_beam_rows(const void* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t suppress_id,
                       const int32_t* suppress_rows, int32_t num_beams, int32_t beams_in, const float* cum, const int32_t* done,
                       int32_t* cand_ids, float* cand_lp, hipStream_t stream) {
  hipLaunchKernelGGL(beam_rows_kernel, dim3(rows), dim3(TOPK_THREADS), 0, stream, (const bf16_t*)logits, ld, vocab, suppress_id,
                     suppress_rows, num_beams, beams_in, cum, done, cand_ids, cand_lp);
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

extern "C" md_status md_region_pick_encode_scored(const void* logits, int64_t ld, int32_t batch, int32_t n_groups,
                                                  int32_t n_bins, const void* value_table, const void* feat_w, int32_t half,
                                                  int32_t* bins, int64_t ld_bins, void* feats, int64_t ld_feats, int32_t window,
                                                  float* logprobs, int64_t ld_logprobs, void* stream) {
  MD_CHECK_ARG(logits && value_table && feat_w && bins && feats && batch > 0 && n_bins > 0);
  MD_CHECK_ARG((n_groups == 1 || n_groups == 2) && ld >= (int64_t)n_groups * n_bins && ld_bins >= n_groups && ld_feats >= 2 * half);
  MD_CHECK_ARG(logprobs && window >= 0 && ld_logprobs >= n_groups);
  hipLaunchKernelGGL(region_pick_scored_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits, ld,
                     n_groups, n_bins, (const bf16_t*)value_table, (const bf16_t*)feat_w, half, bins, ld_bins, (bf16_t*)feats,
                     ld_feats, window, logprobs, ld_logprobs);
  return md_launch_status();
}

extern "C" md_status md_spatial_ref_embed(const int32_t* desc, int32_t n, const void* coord_fw, int32_t coord_feat,
                                          const void* coord_w, int64_t coord_ldw, const void* coord_b, const void* size_fw,
                                          int32_t size_feat, const void* size_w, int64_t size_ldw, const void* size_b,
                                          int32_t dim, void* emb, int64_t ld, int64_t dst0, int32_t rows, void* stream) {
  MD_CHECK_ARG(desc && coord_fw && coord_w && coord_b && size_fw && size_w && size_b && emb);
  MD_CHECK_ARG(n > 0 && rows > 0 && dim > 0 && dim % 4 == 0 && ld >= dim && ld % 4 == 0);
  MD_CHECK_ARG(coord_feat > 0 && coord_feat % 8 == 0 && size_feat > 0 && size_feat % 8 == 0);
  MD_CHECK_ARG(coord_ldw >= coord_feat && coord_ldw % 4 == 0 && size_ldw >= size_feat && size_ldw % 4 == 0);
  const int feat_max = coord_feat > size_feat ? coord_feat : size_feat;
  MD_CHECK_ARG(feat_max <= 2048);  // the group's features live in LDS: 16 rows of feat_max bf16, <= 64 KiB
  MD_CHECK_ARG((uintptr_t)desc % 16 == 0);  // 16-byte descriptors, 8-byte pieces of the weights and of the rows
  MD_CHECK_ARG(((uintptr_t)coord_w | (uintptr_t)coord_b | (uintptr_t)size_w | (uintptr_t)size_b | (uintptr_t)emb) % 8 == 0);
  SpatialRefArgs a{desc, n, (const bf16_t*)coord_fw, (const bf16_t*)coord_w, (const bf16_t*)coord_b, (const bf16_t*)size_fw,
                   (const bf16_t*)size_w, (const bf16_t*)size_b, coord_feat, size_feat, feat_max, coord_ldw, size_ldw, dim,
                   (bf16_t*)emb, ld, dst0, rows};
  const size_t lds = (size_t)SREF_TOKENS * feat_max * sizeof(bf16_t);
  hipLaunchKernelGGL(spatial_ref_embed_kernel, dim3((n + SREF_TOKENS - 1) / SREF_TOKENS, (dim + SREF_COLS - 1) / SREF_COLS),
                     dim3(SREF_THREADS), lds, (hipStream_t)stream, a);
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

extern "C" md_status md_sample_rows_filtered(const void* logits, int64_t ld, int32_t batch, int32_t vocab, int32_t suppress_id,
                                             const float* temperature, const float* top_p, const int32_t* top_k,
                                             const float* min_p, const float* uniforms, int32_t* next, void* probs_out,
                                             int64_t ld_probs, void* stream) {
  MD_CHECK_ARG(logits && temperature && top_p && top_k && min_p && uniforms && next && batch > 0 && vocab > 0 && ld >= vocab);
  MD_CHECK_ARG(probs_out == nullptr || ld_probs >= vocab);
  MD_TRY(md_ensure_dynamic_lds((const void*)sample_rows_filtered_kernel, SAMPLE_LDS));
  hipLaunchKernelGGL(sample_rows_filtered_kernel, dim3(batch), dim3(SAMPLE_THREADS), SAMPLE_LDS, (hipStream_t)stream,
                     (const bf16_t*)logits, ld, vocab, suppress_id, temperature, top_p, top_k, min_p, uniforms, next,
                     (bf16_t*)probs_out, ld_probs);
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
