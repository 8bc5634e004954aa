// Mixed LoRA variants in one launch (Punica / S-LoRA style): every sequence row b carries its own adapter variant[b] from a
// resident bank (md_lora_bank), -1 (or any value outside [0, n_variants)) meaning the base model only.  Two grouped
// kernels serve the low-rank pairs of a whole batch, whatever its mix of variants:
//
//   shrink  t[row, c]  = bf16(x[row] . A_v[r]^T)           fp32 accumulation, v = the row's variant
//   expand  out[row, n] = bf16(bf16(out[row, n]) + bf16(t[row] . B_v[n]^T))     (MD_LORA_ADD)
//           out[row, n] = bf16(t[row] . B_v[n]^T)                                 (MD_LORA_DELTA)
//
// The ADD form rounds twice, in the reference's order: the base linear's output is a bf16 tensor, the low-rank product is
// another, and their sum is rounded again (text.py:31-32,55-56; layers.py:129-142).  The older lora_add of
// md_text_forward_lora instead accumulates the product onto the base output in fp32 and rounds ONCE.
//
// Grouping: a workgroup serves ONE variant.  It finds its rows by scanning the per-sequence table on the device (a ballot
// compaction into LDS; the rows of a sequence across q_len form one contiguous segment) and exits at once when the variant
// has no rows in its chunk.  The shrink loads each 16-row tile of A once per K step for all (<= 64) rows of its chunk; the
// expand holds its 16 columns of B in registers for all rows of its chunk.  Both multiply with v_mfma_f32_16x16x32_bf16.
//
// Row independence: the K order of every output element is fixed by the layer shape (the shrink splits K over its four
// waves by 32-element steps, interleaved, and sums the four partial tiles in wave order), so a row's result does not
// depend on how many rows share its adapter, on where in a tile it lands, or on the other rows' variants.
//
// Operand maps of v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j]
// [col l & 15]; the accumulator has col = l & 15, row = 4 (l >> 4) + j.
#include "gemm_internal.hpp"
#include "text_internal.hpp"

#include <climits>
#include <cstdlib>

#include <algorithm>

namespace {

constexpr int kMaxSeqs = 1024;  // sequences per launch (the LDS row list)

struct LoraEntry {  // one (layer, variant, pair) of the device table
  const bf16_t* a;  // [rank][k]   rank = the bank's packed rank of (variant, pair), a multiple of 16
  const bf16_t* b;  // [n][rank]
};

struct BankView {
  int n_variants;
  int rank[MD_LORA_MAX_VARIANTS][4];
  const LoraEntry* table;  // [n_layers][MD_LORA_MAX_VARIANTS][4]
  int layer;
  __device__ const LoraEntry& at(int v, int pair) const { return table[((int64_t)layer * MD_LORA_MAX_VARIANTS + v) * 4 + pair]; }
};

// column of `pair` in a t row shrunk over the pairs of `mask` (their ranks concatenated in pair order)
__host__ __device__ inline int t_offset(const int (&rank)[4], int mask, int pair) {
  int off = 0;
  for (int q = 0; q < pair; ++q)
    if (mask >> q & 1) off += rank[q];
  return off;
}

// the sequences of group g (g < 0: every entry outside [0, nv)) in ascending order -> list; returns their count
__device__ int collect_sequences(const int32_t* __restrict__ variant, int batch, int g, int nv, int* list, int* count) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int base = 0;
    for (int b0 = 0; b0 < batch; b0 += 64) {
      const int b = b0 + lane;
      const int v = b < batch ? variant[b] : 0;
      const bool in = b < batch && (g >= 0 ? v == g : (v < 0 || v >= nv));
      const uint64_t m = __ballot(in);
      if (in) list[base + __popcll(m & ((1ull << lane) - 1ull))] = b;
      base += __popcll(m);
    }
    if (lane == 0) *count = base;
  }
  __syncthreads();
  return *count;
}

__device__ __forceinline__ int64_t row_of(const int* list, int i, int q_len) {
  const int s = i / q_len;
  return (int64_t)list[s] * q_len + (i - s * q_len);
}

// grid (rank tiles of 16, n_variants, chunks of 64 rows), 256 threads.  A's tile rows r0 .. r0 + 15 of one pair.
__global__ __launch_bounds__(256) void lora_shrink_kernel(BankView bk, int pairs, const int32_t* __restrict__ variant, int batch,
                                                          int q_len, const bf16_t* __restrict__ x, int64_t ldx, int K,
                                                          bf16_t* __restrict__ t, int64_t ldt) {
  __shared__ int seqs[kMaxSeqs];
  __shared__ int n_seqs;
  __shared__ f32x4 red[4][4][64];
  const int v = blockIdx.y;
  const int tcol = blockIdx.x * 16;
  int pair = -1, r0 = 0, col0 = 0;
  for (int q = 0; q < 4; ++q) {
    if (!(pairs >> q & 1) || pair >= 0) continue;
    const int r = bk.rank[v][q];
    if (tcol - col0 < r) {
      pair = q;
      r0 = tcol - col0;
    } else {
      col0 += r;
    }
  }
  if (pair < 0) return;  // beyond this variant's ranks (uniform)
  const bf16_t* A = bk.at(v, pair).a;
  if (A == nullptr) return;  // the pair is absent in this layer: nothing reads these columns
  const int n_rows = collect_sequences(variant, batch, v, bk.n_variants, seqs, &n_seqs) * q_len;
  const int start = blockIdx.z * 64;
  if (start >= n_rows) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = 8 * (lane >> 4);
  const bf16_t* xr[4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    const int i = start + rt * 16 + lr;
    xr[rt] = i < n_rows ? x + row_of(seqs, i, q_len) * ldx + lk : nullptr;
  }
  const bf16_t* ar = A + (int64_t)(r0 + lr) * K + lk;
  f32x4 acc[4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k0 = wave * 32; k0 < K; k0 += 128) {
    const bf16x8 bf = *(const bf16x8*)(ar + k0);
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const bf16x8 af = xr[rt] ? *(const bf16x8*)(xr[rt] + k0) : zero;
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[rt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) red[wave][rt][lane] = acc[rt];
  __syncthreads();
  // wave w finishes row tile w: the four K-interleaved partials summed in wave order
  const int rt = wave;
  f32x4 s = red[0][rt][lane];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const f32x4 p = red[w][rt][lane];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += p[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = start + rt * 16 + 4 * (lane >> 4) + j;
    if (i < n_rows) t[row_of(seqs, i, q_len) * ldt + tcol + lr] = f2bf(s[j]);
  }
}

struct ExpandArgs {
  ExpandSeg seg[2];
  int n_seg;
};

constexpr int kExpandRowTiles = 16;  // rows per workgroup: 16 tiles of 16

// grid (column tiles of 64 over all segments, 1 + n_variants groups (group 0: the base rows), chunks of 256 rows), 256 threads
__global__ __launch_bounds__(256) void lora_expand_kernel(BankView bk, ExpandArgs ea, const int32_t* __restrict__ variant,
                                                          int batch, int q_len) {
  __shared__ int seqs[kMaxSeqs];
  __shared__ int n_seqs;
  const int si = (ea.n_seg > 1 && (int)blockIdx.x >= ea.seg[1].tile0) ? 1 : 0;
  const ExpandSeg& sg = ea.seg[si];
  const int g = (int)blockIdx.y - 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = ((int)blockIdx.x - sg.tile0) * 64 + wave * 16;
  int rank = 0, tcol = 0;
  const bf16_t* B = nullptr;
  if (g >= 0) {
    rank = bk.rank[g][sg.pair];
    B = rank > 0 ? bk.at(g, sg.pair).b : nullptr;
    tcol = t_offset(bk.rank[g], sg.t_pairs, sg.pair);
  }
  const bool has = B != nullptr;
  if (!has && !sg.delta && sg.gelu_from >= sg.n) return;  // out stays as it is (uniform)
  const int n_rows = collect_sequences(variant, batch, g, bk.n_variants, seqs, &n_seqs) * q_len;
  const int start = blockIdx.z * (16 * kExpandRowTiles);
  if (start >= n_rows || n0 >= sg.n) return;
  const int lr = lane & 15, lk = 8 * (lane >> 4);
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 bfr[MD_LORA_MAX_RANK / 32];
  const int ksteps = (rank + 31) / 32;
  if (has) {
#pragma unroll
    for (int ks = 0; ks < MD_LORA_MAX_RANK / 32; ++ks)
      bfr[ks] = (ks < ksteps && ks * 32 + lk < rank) ? *(const bf16x8*)(B + (int64_t)(n0 + lr) * rank + ks * 32 + lk) : zero;
  }
  const int col = n0 + lr;
  for (int rt = 0; rt < kExpandRowTiles; ++rt) {
    const int i0 = start + rt * 16;
    if (i0 >= n_rows) break;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (has) {
      const int ia = i0 + lr;
      const bf16_t* tr = ia < n_rows ? sg.t + row_of(seqs, ia, q_len) * sg.ldt + tcol + lk : nullptr;
#pragma unroll
      for (int ks = 0; ks < MD_LORA_MAX_RANK / 32; ++ks) {
        if (ks < ksteps) {
          const bf16x8 af = (tr && ks * 32 + lk < rank) ? *(const bf16x8*)(tr + ks * 32) : zero;
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[ks], acc, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + 4 * (lane >> 4) + j;
      if (i >= n_rows) continue;
      bf16_t* o = sg.out + row_of(seqs, i, q_len) * sg.ldo + col;
      const float d = bf2f(f2bf(acc[j]));
      if (sg.delta) {
        *o = f2bf(d);
      } else {
        float y = bf2f(*o);
        if (has) y = bf2f(f2bf(y + d));
        if (col >= sg.gelu_from) y = gelu_tanh_f32(y);
        *o = f2bf(y);
      }
    }
  }
}

BankView bank_view(const md_lora_bank* bank, int layer) {
  BankView v;
  v.n_variants = bank->n_variants;
  for (int i = 0; i < MD_LORA_MAX_VARIANTS; ++i)
    for (int q = 0; q < 4; ++q) v.rank[i][q] = bank->rank[i][q];
  v.table = (const LoraEntry*)bank->table;
  v.layer = layer;
  return v;
}

int shrink_width(const md_lora_bank* bank, int pairs) {  // the widest t row of any variant
  int w = 0;
  for (int v = 0; v < bank->n_variants; ++v) w = std::max(w, t_offset(bank->rank[v], pairs, 4));
  return w;
}

}  // namespace

md_status lora_bank_ok(const md_lora_bank* bank) {
  MD_CHECK_ARG(bank && bank->table && bank->n_layers > 0);
  MD_CHECK_ARG(bank->n_variants >= 1 && bank->n_variants <= MD_LORA_MAX_VARIANTS);
  for (int v = 0; v < MD_LORA_MAX_VARIANTS; ++v)
    for (int q = 0; q < 4; ++q) MD_CHECK_ARG(bank->rank[v][q] >= 0 && bank->rank[v][q] <= MD_LORA_MAX_RANK && bank->rank[v][q] % 16 == 0);
  return MD_OK;
}

// t columns a shrink over `pairs` needs (the widest variant), rounded to 16 so that every row stays 32-byte aligned
int32_t md_lora_shrink_cols(const md_lora_bank* bank, int32_t pairs) { return std::max(16, shrink_width(bank, pairs)); }

extern "C" md_status md_lora_shrink_grouped(const md_lora_bank* bank, int32_t layer, int32_t pairs, const int32_t* variant,
                                            int32_t batch, int32_t q_len, const void* x, int64_t ldx, int32_t k, void* t,
                                            int64_t ldt, void* stream) {
  MD_TRY(lora_bank_ok(bank));
  MD_CHECK_ARG(variant && x && t && layer >= 0 && layer < bank->n_layers && pairs > 0 && pairs < 16);
  MD_CHECK_ARG(batch > 0 && batch <= kMaxSeqs && q_len > 0 && k > 0 && k % 32 == 0 && ldx >= k && ldx % 8 == 0);
  MD_CHECK_ARG(ldt % 8 == 0 && ldt >= shrink_width(bank, pairs));
  MD_CHECK_ARG((((uintptr_t)x | (uintptr_t)t) & 15) == 0);
  const int width = shrink_width(bank, pairs);
  if (width == 0) return MD_OK;
  const int64_t rows = (int64_t)batch * q_len;
  dim3 grid(width / 16, bank->n_variants, (unsigned)((rows + 63) / 64));
  hipLaunchKernelGGL(lora_shrink_kernel, grid, dim3(256), 0, (hipStream_t)stream, bank_view(bank, layer), pairs, variant, batch,
                     q_len, (const bf16_t*)x, ldx, k, (bf16_t*)t, ldt);
  return md_launch_status();
}

// one launch over one or two segments (the decode path's qkv + fc1, or proj + fc2)
md_status lora_expand_segments(const md_lora_bank* bank, int layer, const int32_t* variant, int batch, int q_len,
                               const ExpandSeg* segs, int n_seg, hipStream_t s) {
  ExpandArgs ea = {};
  int tiles = 0;
  for (int i = 0; i < n_seg; ++i) {
    const ExpandSeg& g = segs[i];
    MD_CHECK_ARG(g.t && g.out && g.n > 0 && g.n % 16 == 0 && g.ldo >= g.n && g.pair >= 0 && g.pair < 4 && (g.t_pairs >> g.pair & 1));
    MD_CHECK_ARG(g.ldt % 8 == 0 && g.ldt >= shrink_width(bank, g.t_pairs) && ((uintptr_t)g.t & 15) == 0);
    ea.seg[i] = g;
    ea.seg[i].tile0 = tiles;
    tiles += (g.n + 63) / 64;
  }
  ea.n_seg = n_seg;
  const int64_t rows = (int64_t)batch * q_len;
  const int per = 16 * kExpandRowTiles;
  dim3 grid(tiles, 1 + bank->n_variants, (unsigned)((rows + per - 1) / per));
  hipLaunchKernelGGL(lora_expand_kernel, grid, dim3(256), 0, s, bank_view(bank, layer), ea, variant, batch, q_len);
  return md_launch_status();
}

extern "C" md_status md_lora_expand_grouped(const md_lora_bank* bank, int32_t layer, int32_t pair, int32_t t_pairs,
                                            const int32_t* variant, int32_t batch, int32_t q_len, const void* t, int64_t ldt,
                                            void* out, int64_t ldo, int32_t n, int32_t flags, int32_t gelu_from, void* stream) {
  MD_TRY(lora_bank_ok(bank));
  MD_CHECK_ARG(variant && t && out && layer >= 0 && layer < bank->n_layers && t_pairs > 0 && t_pairs < 16);
  MD_CHECK_ARG(batch > 0 && batch <= kMaxSeqs && q_len > 0 && (flags == MD_LORA_ADD || flags == MD_LORA_DELTA));
  ExpandSeg g = {};
  g.t = (const bf16_t*)t;
  g.ldt = ldt;
  g.t_pairs = t_pairs;
  g.pair = pair;
  g.out = (bf16_t*)out;
  g.ldo = ldo;
  g.n = n;
  g.gelu_from = (flags == MD_LORA_ADD && gelu_from >= 0 && gelu_from < n) ? gelu_from : INT_MAX;
  g.delta = flags == MD_LORA_DELTA;
  return lora_expand_segments(bank, layer, variant, batch, q_len, &g, 1, (hipStream_t)stream);
}

// ------------------------------------------------------------------ the bank
extern "C" size_t md_lora_bank_table_bytes(int32_t n_layers) {
  if (n_layers <= 0) return 0;
  return (size_t)n_layers * MD_LORA_MAX_VARIANTS * 4 * sizeof(LoraEntry);
}

extern "C" md_status md_lora_bank_init(md_lora_bank* bank, int32_t n_layers, void* table, size_t table_bytes) {
  MD_CHECK_ARG(bank && table && n_layers > 0 && table_bytes >= md_lora_bank_table_bytes(n_layers));
  if (hipMemset(table, 0, md_lora_bank_table_bytes(n_layers)) != hipSuccess) return MD_ERR_LAUNCH;
  bank->n_variants = 0;
  bank->n_layers = n_layers;
  for (int v = 0; v < MD_LORA_MAX_VARIANTS; ++v)
    for (int q = 0; q < 4; ++q) bank->rank[v][q] = 0;
  bank->table = table;
  return MD_OK;
}

extern "C" md_status md_lora_bank_set_variant(md_lora_bank* bank, const md_text_model* m, int32_t index,
                                              const md_text_block_lora* lora) {
  MD_CHECK_ARG(bank && bank->table && m && lora && bank->n_layers == m->n_layers && m->n_heads > 0);
  MD_CHECK_ARG(index >= 0 && index < MD_LORA_MAX_VARIANTS && index <= bank->n_variants);
  const int hd = m->dim / m->n_heads;
  const int qkv_w = (m->n_heads + 2 * m->n_kv_heads) * hd;
  const int in_dim[4] = {m->dim, m->dim, m->dim, m->ff_dim}, out_dim[4] = {qkv_w, m->dim, m->ff_dim, m->dim};
  int rank[4] = {0, 0, 0, 0};
  const int L = m->n_layers;
  LoraEntry* host = (LoraEntry*)calloc((size_t)L * 4, sizeof(LoraEntry));
  if (!host) return MD_ERR_INVALID_ARG;
  md_status st = MD_OK;
  for (int l = 0; l < L && st == MD_OK; ++l) {
    const md_lora_pair* p[4] = {&lora[l].qkv, &lora[l].proj, &lora[l].fc1, &lora[l].fc2};
    for (int q = 0; q < 4; ++q) {
      const md_lora_pair& lp = *p[q];
      if (lp.a.w == nullptr && lp.b.w == nullptr) continue;
      const int r = lp.a.n_pad;
      // A [r][in] and B [out][r], unpadded in K / N, the rank a multiple of 16 (zero rows / columns past the true rank)
      const bool ok = lp.a.w && lp.b.w && r > 0 && r % 16 == 0 && r <= MD_LORA_MAX_RANK && lp.a.k == in_dim[q] &&
                      lp.a.k_pad == in_dim[q] && lp.b.k_pad == r && lp.b.n == out_dim[q] && (rank[q] == 0 || rank[q] == r) &&
                      in_dim[q] % 32 == 0 && out_dim[q] % 16 == 0 && (((uintptr_t)lp.a.w | (uintptr_t)lp.b.w) & 15) == 0;
      if (!ok) {
        st = r > MD_LORA_MAX_RANK ? MD_ERR_UNSUPPORTED : MD_ERR_INVALID_ARG;
        break;
      }
      rank[q] = r;
      host[l * 4 + q] = LoraEntry{(const bf16_t*)lp.a.w, (const bf16_t*)lp.b.w};
    }
  }
  if (st == MD_OK) {
    // the variant's slice of every layer: [layer][index][4]
    for (int l = 0; l < L && st == MD_OK; ++l) {
      LoraEntry* dst = (LoraEntry*)bank->table + ((int64_t)l * MD_LORA_MAX_VARIANTS + index) * 4;
      if (hipMemcpy(dst, host + l * 4, 4 * sizeof(LoraEntry), hipMemcpyHostToDevice) != hipSuccess) st = MD_ERR_LAUNCH;
    }
  }
  free(host);
  if (st != MD_OK) return st;
  for (int q = 0; q < 4; ++q) bank->rank[index][q] = rank[q];
  if (index == bank->n_variants) bank->n_variants = index + 1;
  return MD_OK;
}
