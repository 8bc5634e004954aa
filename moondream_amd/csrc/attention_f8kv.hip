// Decode attention over an FP8 (OCP e4m3fn) copy of the KV cache -- part of the opt-in fp8 mode (BASELINE configs[4]).
//
// At B = 64 the decode step is bound by the K / V bytes it reads (the bf16 kernel runs at 5.6 TB/s and is 58 % of the
// step): only fewer bytes help.  The cache keeps its bf16 slabs (prefill attention, EncodedImage snapshots and the
// reference-compatible views read those); this mode adds e4m3 slabs of the same [layer][slot][head][position][64]
// shape with ONE static scale per layer for K and one for V (value ~= scale * fp8), written by
//   * kv_quantize_kernel after a prefill (positions pos0[b] .. pos0[b] + q_len - 1 of every layer), and
//   * the decode attention itself for the new token's row (RoPE + cache update fused in, like attn_decode_kernel<true>),
// and read by attn_decode_f8_kernel: one workgroup per (sequence, head), four waves, a 64-byte row = 4 lanes x 16 B
// (16-byte loads: 8-byte ones run at 0.54-0.70x the rate), two streaming passes (scores -> LDS, then P.V), the K scale
// folded into q and the V scale into the output.  The newest key / value enter as what the cache will hold for them
// (quantised, dequantised), so a step sees the same numbers as every later step.
// Tolerance-judged like the rest of the fp8 mode; no bit-compatibility with the bf16 kernel is claimed.
// Rows with a shared-prefix table (md_decode_step_shared) take attn_decode_f8_shared_kernel: the same per-row arithmetic,
// bit for bit, with several rows per workgroup and the keys of a common prefix slot loaded once per group.  The e4m3 bytes of
// a prefix slot are its writer's job (an image prefill into the slot quantises them; md_kv_quantize_f8 after any other write).
#include "text_internal.hpp"

#include <algorithm>

namespace {

constexpr int F8_MAX_CTX = 2048;

typedef float f32x2v __attribute__((ext_vector_type(2)));
// 16 e4m3 bytes -> 16 floats
__device__ __forceinline__ void unpack16(const u32x4& w, float (&f)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i + 0] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}
__device__ __forceinline__ float deq1(uint32_t byte) {  // one e4m3 byte (low 8 bits) -> float
  return __builtin_amdgcn_cvt_pk_f32_fp8((int)byte, false)[0];
}

// bf16 slab rows -> e4m3 slab rows of ONE layer: positions pos0[b] .. pos0[b] + n_pos - 1 of every (slot, head); one
// 16-byte bf16 chunk (8 features) per thread
__global__ __launch_bounds__(256) void kv_quantize_kernel(const bf16_t* __restrict__ ks, const bf16_t* __restrict__ vs, uint8_t* __restrict__ k8,
                                                          uint8_t* __restrict__ v8, float ik, float iv, const int32_t* __restrict__ pos0,
                                                          int pos_fixed, int64_t batch_stride, int ctx, int batch, int n_heads, int n_pos,
                                                          const int32_t* __restrict__ slots, int n_slots) {
  const int64_t total = (int64_t)batch * n_heads * n_pos * 8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ch = (int)(r & 7);
    r >>= 3;
    const int t = (int)(r % n_pos);
    r /= n_pos;
    const int h = (int)(r % n_heads), b = (int)(r / n_heads);
    const int sb = slots ? slots[b] : b;  // slot table (md_text_forward_slots); an idle row has no rows to quantise
    if (sb < 0 || (slots && sb >= n_slots)) continue;
    const int pos = (pos0 ? pos0[b] : pos_fixed) + t;
    if (pos >= ctx) continue;
    const int64_t off = (int64_t)sb * batch_stride + ((int64_t)h * ctx + pos) * 64 + ch * 8;
    const u32x4 kq = *(const u32x4*)(ks + off), vq = *(const u32x4*)(vs + off);
    u32x2 ko, vo;
    ko[0] = pack_fp8x4(lo_bf(kq[0]) * ik, hi_bf(kq[0]) * ik, lo_bf(kq[1]) * ik, hi_bf(kq[1]) * ik);
    ko[1] = pack_fp8x4(lo_bf(kq[2]) * ik, hi_bf(kq[2]) * ik, lo_bf(kq[3]) * ik, hi_bf(kq[3]) * ik);
    vo[0] = pack_fp8x4(lo_bf(vq[0]) * iv, hi_bf(vq[0]) * iv, lo_bf(vq[1]) * iv, hi_bf(vq[1]) * iv);
    vo[1] = pack_fp8x4(lo_bf(vq[2]) * iv, hi_bf(vq[2]) * iv, lo_bf(vq[3]) * iv, hi_bf(vq[3]) * iv);
    *(u32x2*)(k8 + off) = ko;
    *(u32x2*)(v8 + off) = vo;
  }
}

// One workgroup (4 waves) per (sequence, head).  Lane l: row group g = l >> 2 (16 per wave, 64 per workgroup), 16-byte
// chunk c = l & 3 of the 64-byte row.  Key j of round i, slot u (of UNR): j = 64 (i + u) + 16 wave + g.
constexpr int UNR = 8;  // rows requested together per lane: 8 x 16 B in flight
__global__ __launch_bounds__(256) void attn_decode_f8_kernel(const bf16_t* __restrict__ qkv, int64_t ld, bf16_t* __restrict__ o, int64_t ldo,
                                                             const float* __restrict__ freqs, bf16_t* __restrict__ kslab, bf16_t* __restrict__ vslab,
                                                             uint8_t* __restrict__ k8slab, uint8_t* __restrict__ v8slab, int64_t slab_bs, int ctx,
                                                             const int32_t* __restrict__ kv_len_p, int n_heads, float scale_log2, int rot,
                                                             float k_scale, float v_scale, const int32_t* __restrict__ slots, int n_slots) {
  __shared__ float sc[F8_MAX_CTX];
  __shared__ float red[64][64 + 1];  // [row group][feature | sum of p]
  __shared__ float red_m[4];
  __shared__ float newq[64];                                      // rotated q (fp32 of its bf16 value)
  __shared__ __attribute__((aligned(16))) uint8_t new8[2][64];    // the new token's K and V rows as stored in the fp8 cache
  __shared__ __attribute__((aligned(16))) bf16_t newbf[2][64];    // and as stored in the bf16 cache

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 2, c = lane & 3;
  const int b = blockIdx.y, h = blockIdx.x;
  // slot table (md_text_forward_slots): row b's K / V live in slot slots[b]; an idle row (slot outside [0, n_slots)) writes a
  // zero output and touches neither copy of the cache (uniform per workgroup, before any barrier)
  int sb = b;
  if (slots != nullptr) {
    sb = slots[b];
    if (sb < 0 || sb >= n_slots) {
      if (tid < 64) o[(int64_t)b * ldo + h * 64 + tid] = f2bf(0.f);
      return;
    }
  }
  const int kv_len = kv_len_p[b], pos = kv_len - 1;
  const int64_t head_off = (int64_t)sb * slab_bs + (int64_t)h * ctx * 64;
  const uint8_t* kb = k8slab + head_off;
  const uint8_t* vb = v8slab + head_off;

  {  // RoPE of q and k, pass-through features, v: the new token's rows (text.py:35-46, rope.py:20-48)
    const bf16_t* row = qkv + (int64_t)b * ld;
    const int half = rot >> 1;
    if (tid < 2 * half) {
      const int which = tid / half, j = tid % half;
      const bf16_t* hp = row + (which ? (n_heads + h) : h) * 64;
      const float re = bf2f(hp[j]), im = bf2f(hp[half + j]);
      const float cs = freqs[((int64_t)pos * half + j) * 2], sn = freqs[((int64_t)pos * half + j) * 2 + 1];
      float o_re, o_im;
      md_rope_pair(re, im, cs, sn, o_re, o_im);
      if (which == 0) {
        newq[2 * j] = bf2f(f2bf(o_re));
        newq[2 * j + 1] = bf2f(f2bf(o_im));
      } else {
        newbf[0][2 * j] = f2bf(o_re);
        newbf[0][2 * j + 1] = f2bf(o_im);
      }
    } else if (tid >= 64 && tid < 64 + 2 * (64 - rot)) {
      const int t2 = tid - 64, which = t2 / (64 - rot), i = rot + t2 % (64 - rot);
      const bf16_t x = row[(which ? (n_heads + h) : h) * 64 + i];
      if (which == 0) newq[i] = bf2f(x); else newbf[0][i] = x;
    } else if (tid >= 192 && tid < 256) {
      newbf[1][tid - 192] = row[(2 * n_heads + h) * 64 + tid - 192];
    }
    __syncthreads();
    if (tid < 32) {  // 2 rows x 16 words of 4 features: quantise, keep in LDS, write both caches
      const int which = tid >> 4, w4 = tid & 15;
      const float inv = 1.0f / (which ? v_scale : k_scale);
      const bf16_t* src = &newbf[which][4 * w4];
      const uint32_t q = pack_fp8x4(bf2f(src[0]) * inv, bf2f(src[1]) * inv, bf2f(src[2]) * inv, bf2f(src[3]) * inv);
      *(uint32_t*)(&new8[which][4 * w4]) = q;
      *(uint32_t*)((which ? v8slab : k8slab) + head_off + (int64_t)pos * 64 + 4 * w4) = q;
    } else if (tid >= 64 && tid < 128) {
      kslab[head_off + (int64_t)pos * 64 + tid - 64] = newbf[0][tid - 64];
    } else if (tid >= 128 && tid < 192) {
      vslab[head_off + (int64_t)pos * 64 + tid - 128] = newbf[1][tid - 128];
    }
    __syncthreads();
  }

  float qv[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) qv[e] = newq[16 * c + e] * (scale_log2 * k_scale);

  // ---- pass 1: scores --------------------------------------------------------------------------------------------
  float mx = -INFINITY;
  for (int i0 = 0; i0 * 64 < kv_len; i0 += UNR) {
    u32x4 kq[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = 64 * (i0 + u) + 16 * wave + g;
      kq[u] = __builtin_nontemporal_load((const u32x4*)(kb + (int64_t)min(j, pos) * 64 + c * 16));  // read once per step (attention.hip: NT)
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = 64 * (i0 + u) + 16 * wave + g;
      // (the newest key is not yet visible in global memory to this CU: take it from LDS)
      const u32x4 kk = (j == pos) ? *(const u32x4*)(&new8[0][c * 16]) : kq[u];
      float kf[16];
      unpack16(kk, kf);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) s += qv[e] * kf[e];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      if (j < kv_len) {
        if (c == 0) sc[j] = s;
        mx = fmaxf(mx, s);
      }
    }
  }
  mx = wave_max(mx);
  if (lane == 0) red_m[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));

  // ---- pass 2: probabilities and P.V -----------------------------------------------------------------------------
  float acc[16], l = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int i0 = 0; i0 * 64 < kv_len; i0 += UNR) {
    u32x4 vq[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = 64 * (i0 + u) + 16 * wave + g;
      vq[u] = __builtin_nontemporal_load((const u32x4*)(vb + (int64_t)min(j, pos) * 64 + c * 16));
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = 64 * (i0 + u) + 16 * wave + g;
      const u32x4 vv = (j == pos) ? *(const u32x4*)(&new8[1][c * 16]) : vq[u];
      const float pj = (j < kv_len) ? __builtin_amdgcn_exp2f(sc[min(j, pos)] - mx) : 0.f;
      l += pj;
      const float pr = bf2f(f2bf(pj));  // probabilities enter the second contraction as bf16, as in the bf16 kernel
      float vf[16];
      unpack16(vv, vf);
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] += pr * vf[e];
    }
  }
  const int rg = 16 * wave + g;
#pragma unroll
  for (int e = 0; e < 16; ++e) red[rg][16 * c + e] = acc[e];
  if (c == 0) red[rg][64] = l;
  __syncthreads();
  if (tid < 64) {
    float s = 0.f, lt = 0.f;
    for (int r = 0; r < 64; ++r) {
      s += red[r][tid];
      lt += red[r][64];
    }
    o[(int64_t)b * ldo + h * 64 + tid] = f2bf(lt > 0.f ? s * v_scale / lt : 0.f);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// decode over the e4m3 copy with a shared KV prefix (md_text_forward_shared / md_decode_step_shared): G rows per workgroup
// ---------------------------------------------------------------------------------------------------------------------
// Row b reads keys [0, plen_b) from slot pslots[b] of the e4m3 slabs and keys [plen_b, kv_len_b) from its own slot slots[b];
// all four writes of the new row (bf16 K / V, e4m3 K / V, at kv_len_b - 1) go to slots[b].  One workgroup serves one head and
// F8G consecutive rows.  When every live row of the group names the same prefix slot, the keys of whole 64-key rounds below
// the group's smallest plen are loaded ONCE (default cache policy: the head's other groups read them again) and applied to
// the F8G queries held in registers, in both passes; every other key is loaded per row (non-temporal, except a round that
// lies wholly inside the row's prefix).  A group with mixed prefix slots takes the per-row path throughout.
//
// A second launch shape of attn_decode_f8_kernel's definition, not a second definition: thread (wave, g, c) owns key class
// j mod 64 == 16 wave + g and chunk c, a score is the same 16-term sum and butterfly with k_scale * scale * log2(e) folded
// into q, the maximum runs over live keys, p = exp2(s - max) is rounded to bf16 before P.V while its fp32 value enters the
// row sum, a class accumulates in ascending key order, the 64 classes are summed in ascending order, o = s * v_scale / l,
// and the newest key / value enter from LDS as the e4m3 bytes the cache will hold.  Every output bit and every slab byte of
// a live row is what the one-row kernel gives over a slot into which keys [0, plen_b) were copied.  The one-row kernel
// runs rounds past a row's kv_len with p = 0 over row kv_len - 1 (exact zeros); here a row skips a round that lies wholly
// past its kv_len and clamps the loads of its last round to kv_len - 1 in its own slot, so no product is ever formed with a
// byte from at or beyond the row's kv_len.
// LDS at F8G = 4: scores [4][2048] fp32 (32 768 B) + one row's reduction (16 640 B, reused row by row) + the wave maxima
// (64 B) + the new rows (q 1 024 B, e4m3 K / V 512 B, bf16 K / V 1 024 B) = 52 032 B.
constexpr int F8G = 4;    // divides 64: a step of more than 64 rows arrives in 64-row blocks (rows.block)
constexpr int F8UNRS = 8; // shared rounds whose loads are issued together, as UNR

template <int G>
__global__ __launch_bounds__(256) void attn_decode_f8_shared_kernel(const bf16_t* __restrict__ qkv, int64_t ld, bf16_t* __restrict__ o, int64_t ldo,
                                                                    const float* __restrict__ freqs, bf16_t* __restrict__ kslab,
                                                                    bf16_t* __restrict__ vslab, uint8_t* __restrict__ k8slab,
                                                                    uint8_t* __restrict__ v8slab, int64_t slab_bs, int ctx,
                                                                    const int32_t* __restrict__ kv_len_p, int batch, int n_heads,
                                                                    float scale_log2, int rot, float k_scale, float v_scale,
                                                                    const int32_t* __restrict__ slots, int n_slots,
                                                                    const int32_t* __restrict__ pslots, const int32_t* __restrict__ plen_p) {
  __shared__ float sc[G][F8_MAX_CTX];
  __shared__ float red[64][64 + 1];  // one row at a time: [row group][feature | sum of p]
  __shared__ float red_m[G][4];
  __shared__ float newq[G][64];
  __shared__ __attribute__((aligned(16))) uint8_t new8[G][2][64];
  __shared__ __attribute__((aligned(16))) bf16_t newbf[G][2][64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g4 = lane >> 2, c = lane & 3;
  const int h = blockIdx.x, b0 = blockIdx.y * G;
  const int cls = 16 * wave + g4;  // the key class this thread owns
  const int64_t head_off = (int64_t)h * ctx * 64;

  // per-row state, uniform per workgroup.  A row past batch is absent; a slot outside [0, n_slots) (or a kv_len the slab
  // cannot hold) is an IDLE row: zero output, no slab read or write; a prefix slot outside [0, n_slots) means no shared prefix.
  bool live[G];
  int kvl[G], plen[G];
  int64_t own[G], pre[G];  // element (= byte, in the e4m3 slabs) offsets of the row's own slot / of its prefix slot
  int shared_slot = -1, min_plen = F8_MAX_CTX, kv_max = 0;
  bool same = true, any_live = false;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int b = b0 + g;
    live[g] = false;
    kvl[g] = 0;
    plen[g] = 0;
    own[g] = pre[g] = 0;
    if (b >= batch) continue;
    const int sb = slots[b];
    const int kl = kv_len_p[b];
    if (sb < 0 || sb >= n_slots || kl < 1 || kl > ctx) {
      if (tid < 64) o[(int64_t)b * ldo + h * 64 + tid] = f2bf(0.f);
      continue;
    }
    live[g] = any_live = true;
    kvl[g] = kl;
    own[g] = (int64_t)sb * slab_bs + head_off;
    const int ps = pslots[b];
    const int pl = (ps >= 0 && ps < n_slots) ? min(max(plen_p[b], 0), kl - 1) : 0;
    plen[g] = pl;
    pre[g] = (pl > 0 ? (int64_t)ps * slab_bs + head_off : own[g]);
    if (pl == 0) same = false;
    else if (shared_slot < 0) shared_slot = ps;
    else if (shared_slot != ps) same = false;
    min_plen = min(min_plen, pl);
    kv_max = max(kv_max, kl);
  }
  if (!any_live) return;  // uniform, before any barrier
  // whole 64-key rounds below every live row's prefix end: one load per key for the whole group
  const int n_shared = (same && shared_slot >= 0) ? min_plen / 64 : 0;
  const int64_t shared_off = (n_shared > 0) ? (int64_t)shared_slot * slab_bs + head_off : 0;

  // per row, as attn_decode_f8_kernel: RoPE of q and k, pass-through features, v; then both copies of the new row
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (!live[g]) continue;
    const int pos = kvl[g] - 1;
    const bf16_t* row = qkv + (int64_t)(b0 + g) * ld;
    const int half = rot >> 1;
    if (tid < 2 * half) {
      const int which = tid / half, j = tid % half;
      const bf16_t* hp = row + (which ? (n_heads + h) : h) * 64;
      const float re = bf2f(hp[j]), im = bf2f(hp[half + j]);
      const float cs = freqs[((int64_t)pos * half + j) * 2], sn = freqs[((int64_t)pos * half + j) * 2 + 1];
      float o_re, o_im;
      md_rope_pair(re, im, cs, sn, o_re, o_im);
      if (which == 0) {
        newq[g][2 * j] = bf2f(f2bf(o_re));
        newq[g][2 * j + 1] = bf2f(f2bf(o_im));
      } else {
        newbf[g][0][2 * j] = f2bf(o_re);
        newbf[g][0][2 * j + 1] = f2bf(o_im);
      }
    } else if (tid >= 64 && tid < 64 + 2 * (64 - rot)) {
      const int t2 = tid - 64, which = t2 / (64 - rot), i = rot + t2 % (64 - rot);
      const bf16_t x = row[(which ? (n_heads + h) : h) * 64 + i];
      if (which == 0) newq[g][i] = bf2f(x); else newbf[g][0][i] = x;
    } else if (tid >= 192 && tid < 256) {
      newbf[g][1][tid - 192] = row[(2 * n_heads + h) * 64 + tid - 192];
    }
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (!live[g]) continue;
    const int pos = kvl[g] - 1;
    if (tid < 32) {  // 2 rows x 16 words of 4 features: quantise, keep in LDS, write both caches
      const int which = tid >> 4, w4 = tid & 15;
      const float inv = 1.0f / (which ? v_scale : k_scale);
      const bf16_t* src = &newbf[g][which][4 * w4];
      const uint32_t q = pack_fp8x4(bf2f(src[0]) * inv, bf2f(src[1]) * inv, bf2f(src[2]) * inv, bf2f(src[3]) * inv);
      *(uint32_t*)(&new8[g][which][4 * w4]) = q;
      *(uint32_t*)((which ? v8slab : k8slab) + own[g] + (int64_t)pos * 64 + 4 * w4) = q;
    } else if (tid >= 64 && tid < 128) {
      kslab[own[g] + (int64_t)pos * 64 + tid - 64] = newbf[g][0][tid - 64];
    } else if (tid >= 128 && tid < 192) {
      vslab[own[g] + (int64_t)pos * 64 + tid - 128] = newbf[g][1][tid - 128];
    }
  }
  __syncthreads();

  // ---- pass 1: scores --------------------------------------------------------------------------------------------
  float mx[G];
  {
    float qv[G][16];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      mx[g] = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) qv[g][e] = live[g] ? newq[g][16 * c + e] * (scale_log2 * k_scale) : 0.f;
    }
    // the per-lane partial and butterfly of attn_decode_f8_kernel
    auto score = [&](int g, const float (&kf)[16]) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) s += qv[g][e] * kf[e];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      return s;
    };
    for (int i0 = 0; i0 < n_shared; i0 += F8UNRS) {
      u32x4 kq[F8UNRS];
#pragma unroll
      for (int u = 0; u < F8UNRS; ++u) {
        const int j = 64 * min(i0 + u, n_shared - 1) + cls;
        kq[u] = *(const u32x4*)(k8slab + shared_off + (int64_t)j * 64 + c * 16);
      }
#pragma unroll
      for (int u = 0; u < F8UNRS; ++u) {
        if (i0 + u >= n_shared) break;  // uniform
        const int j = 64 * (i0 + u) + cls;
        float kf[16];
        unpack16(kq[u], kf);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (!live[g]) continue;
          const float s = score(g, kf);  // j < plen <= kv_len - 1 for every live row
          if (c == 0) sc[g][j] = s;
          mx[g] = fmaxf(mx[g], s);
        }
      }
    }
    for (int i = n_shared; i * 64 < kv_max; ++i) {
      const int j = 64 * i + cls;
      u32x4 kq[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        kq[g] = u32x4{0, 0, 0, 0};
        if (!live[g] || 64 * i >= kvl[g]) continue;  // uniform
        const int jj = min(j, kvl[g] - 1);           // (kv_len - 1 >= plen: the clamp stays in the own slot)
        if (64 * (i + 1) <= plen[g]) kq[g] = *(const u32x4*)(k8slab + pre[g] + (int64_t)jj * 64 + c * 16);
        else kq[g] = __builtin_nontemporal_load((const u32x4*)(k8slab + (jj < plen[g] ? pre[g] : own[g]) + (int64_t)jj * 64 + c * 16));
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (!live[g] || 64 * i >= kvl[g]) continue;
        // (the newest key is not yet visible in global memory to this CU: take it from LDS)
        const u32x4 kk = (j == kvl[g] - 1) ? *(const u32x4*)(&new8[g][0][c * 16]) : kq[g];
        float kf[16];
        unpack16(kk, kf);
        const float s = score(g, kf);
        if (j < kvl[g]) {
          if (c == 0) sc[g][j] = s;
          mx[g] = fmaxf(mx[g], s);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    mx[g] = wave_max(mx[g]);
    if (lane == 0) red_m[g][wave] = mx[g];
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < G; ++g) mx[g] = fmaxf(fmaxf(red_m[g][0], red_m[g][1]), fmaxf(red_m[g][2], red_m[g][3]));

  // ---- pass 2: probabilities and P.V -----------------------------------------------------------------------------
  float acc[G][16], l[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[g][e] = 0.f;
  }
  auto accumulate = [&](int g, float pj, const float (&vf)[16]) {
    l[g] += pj;
    const float pr = bf2f(f2bf(pj));  // probabilities enter the second contraction as bf16, as in the bf16 kernel
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[g][e] += pr * vf[e];
  };
  for (int i0 = 0; i0 < n_shared; i0 += F8UNRS) {
    u32x4 vq[F8UNRS];
#pragma unroll
    for (int u = 0; u < F8UNRS; ++u) {
      const int j = 64 * min(i0 + u, n_shared - 1) + cls;
      vq[u] = *(const u32x4*)(v8slab + shared_off + (int64_t)j * 64 + c * 16);
    }
#pragma unroll
    for (int u = 0; u < F8UNRS; ++u) {
      if (i0 + u >= n_shared) break;  // uniform
      const int j = 64 * (i0 + u) + cls;
      float vf[16];
      unpack16(vq[u], vf);
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (live[g]) accumulate(g, __builtin_amdgcn_exp2f(sc[g][j] - mx[g]), vf);
    }
  }
  for (int i = n_shared; i * 64 < kv_max; ++i) {
    const int j = 64 * i + cls;
    u32x4 vq[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      vq[g] = u32x4{0, 0, 0, 0};
      if (!live[g] || 64 * i >= kvl[g]) continue;  // uniform
      const int jj = min(j, kvl[g] - 1);
      if (64 * (i + 1) <= plen[g]) vq[g] = *(const u32x4*)(v8slab + pre[g] + (int64_t)jj * 64 + c * 16);
      else vq[g] = __builtin_nontemporal_load((const u32x4*)(v8slab + (jj < plen[g] ? pre[g] : own[g]) + (int64_t)jj * 64 + c * 16));
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (!live[g] || 64 * i >= kvl[g]) continue;
      const int pos = kvl[g] - 1;
      const u32x4 vv = (j == pos) ? *(const u32x4*)(&new8[g][1][c * 16]) : vq[g];
      const float pj = (j < kvl[g]) ? __builtin_amdgcn_exp2f(sc[g][min(j, pos)] - mx[g]) : 0.f;
      float vf[16];
      unpack16(vv, vf);
      accumulate(g, pj, vf);
    }
  }
  // one row at a time through the reduction array, classes in ascending order
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (!live[g]) continue;  // uniform
#pragma unroll
    for (int e = 0; e < 16; ++e) red[cls][16 * c + e] = acc[g][e];
    if (c == 0) red[cls][64] = l[g];
    __syncthreads();
    if (tid < 64) {
      float s = 0.f, lt = 0.f;
      for (int r = 0; r < 64; ++r) {
        s += red[r][tid];
        lt += red[r][64];
      }
      o[(int64_t)(b0 + g) * ldo + h * 64 + tid] = f2bf(lt > 0.f ? s * v_scale / lt : 0.f);
    }
    __syncthreads();
  }
}

}  // namespace

// internal (api.hip)
md_status md_kv_quantize_f8_layer(const md_kv_cache* kv, int layer, const int32_t* pos0, int pos_fixed, int batch, int n_heads,
                                  int n_pos, const RowMap& rows, hipStream_t s) {
  MD_CHECK_ARG(kv && kv->k && kv->v && kv->k8 && kv->v8 && kv->k_scale && kv->v_scale && kv->k_scale[layer] > 0.f && kv->v_scale[layer] > 0.f);
  const int64_t total = (int64_t)batch * n_heads * n_pos * 8;
  if (total <= 0) return MD_OK;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 32);
  const int64_t lo = (int64_t)layer * kv->layer_stride;
  hipLaunchKernelGGL(kv_quantize_kernel, dim3(blocks), dim3(256), 0, s, (const bf16_t*)kv->k + lo, (const bf16_t*)kv->v + lo,
                     (uint8_t*)kv->k8 + lo, (uint8_t*)kv->v8 + lo, 1.0f / kv->k_scale[layer], 1.0f / kv->v_scale[layer], pos0, pos_fixed,
                     kv->batch_stride, kv->ctx, batch, n_heads, n_pos, rows.slots, rows.n_slots);
  return md_launch_status();
}

extern "C" md_status md_kv_quantize_f8(const md_kv_cache* kv, int32_t n_layers, int32_t batch, int32_t n_heads, const int32_t* pos0,
                                       int32_t pos_fixed, int32_t n_pos, void* stream) {
  MD_CHECK_ARG(kv && n_layers > 0 && batch > 0 && n_heads > 0 && n_pos > 0 && pos_fixed >= 0);
  for (int l = 0; l < n_layers; ++l)
    MD_TRY(md_kv_quantize_f8_layer(kv, l, pos0, pos_fixed, batch, n_heads, n_pos, RowMap{}, (hipStream_t)stream));
  return MD_OK;
}

// internal (md_attention_decode_rows picks it): the fused MHA step over the e4m3 copy; the checks that are this kernel's own
md_status md_attention_decode_f8_rows(const DecodeAttn& d, const RowMap& rows, hipStream_t s) {
  MD_CHECK_ARG(d.k8_slab && d.v8_slab && d.ctx <= F8_MAX_CTX && d.k_scale > 0.f && d.v_scale > 0.f);
  hipLaunchKernelGGL(attn_decode_f8_kernel, dim3(d.n_heads, d.batch), dim3(256), 0, s, (const bf16_t*)d.q, d.ldq, (bf16_t*)d.o, d.ldo,
                     d.freqs, (bf16_t*)d.k_slab, (bf16_t*)d.v_slab, (uint8_t*)d.k8_slab, (uint8_t*)d.v8_slab, d.slab_batch_stride,
                     d.ctx, d.kv_len, d.n_heads, d.scale * 1.4426950408889634f, d.rot_dim, d.k_scale, d.v_scale, rows.slots,
                     rows.n_slots);
  return md_launch_status();
}

// internal (md_attention_decode_rows picks it when the rows carry a prefix table): the grouped kernel and its own checks
md_status md_attention_decode_f8_shared_rows(const DecodeAttn& d, const RowMap& rows, hipStream_t s) {
  MD_CHECK_ARG(d.k8_slab && d.v8_slab && d.ctx <= F8_MAX_CTX && d.k_scale > 0.f && d.v_scale > 0.f);
  MD_CHECK_ARG(rows.slots && rows.n_slots > 0 && rows.pfx_slots && rows.pfx_len);
  static_assert(64 % F8G == 0, "a 64-row block of a decode step must be a whole number of groups");
  hipLaunchKernelGGL(attn_decode_f8_shared_kernel<F8G>, dim3(d.n_heads, (d.batch + F8G - 1) / F8G), dim3(256), 0, s, (const bf16_t*)d.q,
                     d.ldq, (bf16_t*)d.o, d.ldo, d.freqs, (bf16_t*)d.k_slab, (bf16_t*)d.v_slab, (uint8_t*)d.k8_slab, (uint8_t*)d.v8_slab,
                     d.slab_batch_stride, d.ctx, d.kv_len, d.batch, d.n_heads, d.scale * 1.4426950408889634f, d.rot_dim, d.k_scale,
                     d.v_scale, rows.slots, rows.n_slots, rows.pfx_slots, rows.pfx_len);
  return md_launch_status();
}

extern "C" md_status md_attention_decode_rope_f8(const void* qkv, int64_t ld, void* o, int64_t ldo, const float* freqs, void* k_slab,
                                                 void* v_slab, void* k8_slab, void* v8_slab, int64_t slab_batch_stride, int32_t ctx,
                                                 const int32_t* kv_len, int32_t batch, int32_t n_heads, int32_t rot_dim, float scale,
                                                 float k_scale, float v_scale, void* stream) {
  return md_attention_decode_rope_f8_shared(qkv, ld, o, ldo, freqs, k_slab, v_slab, k8_slab, v8_slab, slab_batch_stride, ctx, kv_len,
                                            batch, n_heads, rot_dim, scale, k_scale, v_scale, nullptr, 0, nullptr, nullptr, stream);
}

extern "C" md_status md_attention_decode_rope_f8_shared(const void* qkv, int64_t ld, void* o, int64_t ldo, const float* freqs, void* k_slab,
                                                        void* v_slab, void* k8_slab, void* v8_slab, int64_t slab_batch_stride,
                                                        int32_t ctx, const int32_t* kv_len, int32_t batch, int32_t n_heads,
                                                        int32_t rot_dim, float scale, float k_scale, float v_scale, const int32_t* slots,
                                                        int32_t n_slots, const int32_t* prefix_slots, const int32_t* prefix_len,
                                                        void* stream) {
  MD_CHECK_ARG(k8_slab && v8_slab);  // without the copy the dispatcher would take the bf16 kernels
  const DecodeAttn d = {qkv, ld, o, ldo, freqs, k_slab, v_slab, k8_slab, v8_slab, k_scale, v_scale, slab_batch_stride, ctx, kv_len,
                        batch, n_heads, n_heads, 64, rot_dim, scale, true};
  return md_attention_decode_rows(d, RowMap{slots, n_slots, prefix_slots, prefix_len}, (hipStream_t)stream);
}
