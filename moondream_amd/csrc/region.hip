// The region head's device-resident pieces:
//   * Fourier features of coordinates and sizes (md_fourier_features; reference: region.py:12-29);
//   * the "pick a bin and re-encode it" step of detect / point (md_region_pick_encode, and _scored with a confidence
//     per pick; reference: moondream.py:672-713 around region.py:12-71), so a points loop over B images needs no host
//     round trip per coordinate;
//   * the spatial references of a batch of prompts, encoded into their embedding rows (md_spatial_ref_embed).
// Row kernels: one workgroup per sequence (or per 16 reference tokens), wave shuffles.
#include "row_reduce.hpp"

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
// torch.argmax on the reference's CPU path; an all-NaN group -> bin 0: block_argmax, row_reduce.hpp), value = table[bin],
// then the Fourier features.
// SCORED adds a confidence per group (md_region_pick_encode_scored) after the same pick, so bins and features are
// bit-identical: the reasoning step bakes the plain instantiation into captured graphs, and with SCORED false nothing of
// the sums is compiled.  Per group, with m = x[pick] (the group's maximum) in fp32 from the bf16 logits x:
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
template <bool SCORED>
__global__ __launch_bounds__(256) void region_pick_kernel(const bf16_t* __restrict__ logits, int64_t ld, int n_groups,
                                                          int n_bins, const bf16_t* __restrict__ table,
                                                          const bf16_t* __restrict__ w, int half,
                                                          int32_t* __restrict__ bins, int64_t ld_bins,
                                                          bf16_t* __restrict__ feats, int64_t ldf, int window,
                                                          float* __restrict__ logprobs, int64_t ld_lp) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ float val[2];
  __shared__ int picked;  // (SCORED)
  __shared__ float part_s[4];
  __shared__ float part_w[4];
  const int b = blockIdx.x;
  for (int g = 0; g < n_groups; ++g) {
    const bf16_t* lr = logits + (int64_t)b * ld + (int64_t)g * n_bins;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n_bins; i += 256) argmax_take(best, bi, bf2f(lr[i]), i);
    bi = block_argmax<4>(best, bi, n_bins, sv, si);
    if (threadIdx.x == 0) {
      bins[(int64_t)b * ld_bins + g] = bi;
      val[g] = bf2f(table[bi]);
      if (SCORED) picked = bi;
    }
    __syncthreads();
    if constexpr (SCORED) {
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

}  // namespace

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
  hipLaunchKernelGGL(region_pick_kernel<false>, dim3(batch), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits, ld,
                     n_groups, n_bins, (const bf16_t*)value_table, (const bf16_t*)feat_w, half, bins, ld_bins, (bf16_t*)feats,
                     ld_feats, 0, (float*)nullptr, (int64_t)0);
  return md_launch_status();
}

extern "C" md_status md_region_pick_encode_scored(const void* logits, int64_t ld, int32_t batch, int32_t n_groups,
                                                  int32_t n_bins, const void* value_table, const void* feat_w, int32_t half,
                                                  int32_t* bins, int64_t ld_bins, void* feats, int64_t ld_feats, int32_t window,
                                                  float* logprobs, int64_t ld_logprobs, void* stream) {
  MD_CHECK_ARG(logits && value_table && feat_w && bins && feats && batch > 0 && n_bins > 0);
  MD_CHECK_ARG((n_groups == 1 || n_groups == 2) && ld >= (int64_t)n_groups * n_bins && ld_bins >= n_groups && ld_feats >= 2 * half);
  MD_CHECK_ARG(logprobs && window >= 0 && ld_logprobs >= n_groups);
  hipLaunchKernelGGL(region_pick_kernel<true>, dim3(batch), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits, ld,
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
