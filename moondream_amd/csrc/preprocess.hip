// Image preprocessing on the device (include/moondream_hip.h: md_image_resample_crops): Pillow's 8-bit LANCZOS resize as
// the integer arithmetic it is -- per output pixel a window of taps with int32 coefficients at 22 fractional bits,
// ((1 << 21) + sum k * pixel) >> 22 clamped to 0 .. 255, horizontally into a uint8 intermediate, then vertically -- and the
// cutting of the overlapping crops, which is only WHERE the vertical pass stores.  Two launches over a whole ViT chunk; the
// work list is flat: an entry is (image, target), its blocks follow the previous entry's, and a block finds its entry by
// binary search over the block prefixes the descriptors carry.
#include "md_common.hpp"

namespace {

constexpr int H_SEG = MD_RESAMPLE_H_SEG_BYTES, H_ROWS = MD_RESAMPLE_H_ROWS;  // horizontal: 256 output bytes x 4 source rows
constexpr int V_SEG = MD_RESAMPLE_V_SEG_BYTES, V_ROWS = MD_RESAMPLE_V_ROWS;  // vertical: 1024 output bytes x 8 output rows
constexpr int DW = MD_RESAMPLE_DESC_WORDS, T0 = 8, TW = 12;
constexpr int PREC = 22;
constexpr int LDS_MAX = 64 * 1024;
static_assert(H_SEG == 256 && V_SEG == 4 * 256, "one output byte / one output dword per thread of a 256-thread block");

// words of a target inside a descriptor
enum { T_OUT_H, T_OUT_W, T_KX_N, T_KY_N, T_BX, T_KX, T_BY, T_KY, T_HBLK0, T_VBLK0 };

struct Geometry {
  int crop, window, total_crops;
};

__host__ __device__ inline int64_t pitch_of(int64_t out_w) { return (out_w * 3 + 15) / 16 * 16; }

// the entry (image * 2 + target) whose blocks hold `bid`: the LAST one whose first block is <= bid (an entry without work
// has its successor's first block and is never the last such)
__device__ __forceinline__ int find_entry(const int64_t* __restrict__ desc, int n_entries, int bid, int word) {
  int lo = 0, hi = n_entries - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[(int64_t)(mid >> 1) * DW + T0 + (mid & 1) * TW + word] <= bid) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ uint8_t clip8(uint32_t acc) {
  const int v = (int)acc >> PREC;
  return (uint8_t)min(max(v, 0), 255);
}

// Horizontal pass.  A block: 256 consecutive output bytes (x, channel interleaved) of H_ROWS source rows.  The source span
// those outputs read -- [x_lo, x_hi) pixels, the windows of the segment's first and last output pixel: windows move
// monotonically -- is staged in LDS for each row with aligned dword loads (the image base is 16-byte aligned, so a byte
// offset inside the image that is a multiple of 4 is an aligned address; a dword that would reach past the image's last
// byte is read byte by byte), and a thread then walks its taps once for all rows: one coefficient load per tap.
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ packed, int n_entries, uint8_t* __restrict__ ws,
                                                         int span_cap) {
  extern __shared__ uint8_t lds[];  // [H_ROWS][span_cap]
  const int64_t* desc = (const int64_t*)packed;
  const int tid = threadIdx.x, bid = blockIdx.x;
  const int e = find_entry(desc, n_entries, bid, T_HBLK0);
  const int64_t* d = desc + (int64_t)(e >> 1) * DW;
  const int64_t* t = d + T0 + (e & 1) * TW;
  const int src_h = (int)d[0], src_w = (int)d[1], out_w = (int)t[T_OUT_W], ksize = (int)t[T_KX_N];
  const int row_bytes = out_w * 3, nseg = (row_bytes + H_SEG - 1) / H_SEG;
  const int local = bid - (int)t[T_HBLK0], seg = local % nseg, y0 = (local / nseg) * H_ROWS;
  if (y0 >= src_h) return;  // (not one of this entry's blocks: the descriptors disagree with the grid)
  const int32_t* bounds = (const int32_t*)(packed + t[T_BX]);
  const int32_t* coef = (const int32_t*)(packed + t[T_KX]);
  const uint8_t* img = packed + d[6];
  const int64_t img_bytes = (int64_t)src_h * src_w * 3;
  int64_t inter_off = d[7];
  if (e & 1) inter_off += (int64_t)src_h * pitch_of(d[T0 + T_OUT_W]);  // the second target's intermediate follows the first's
  uint8_t* inter = ws + inter_off;
  const int64_t pitch = pitch_of(out_w);

  const int b0 = seg * H_SEG, b_last = min(b0 + H_SEG, row_bytes) - 1;
  const int xo_first = b0 / 3, xo_last = b_last / 3;
  const int x_lo = bounds[2 * xo_first], x_hi = bounds[2 * xo_last] + bounds[2 * xo_last + 1];
  const int span = (x_hi - x_lo) * 3;
  if (x_lo < 0 || x_hi > src_w || span <= 0 || span + 3 > span_cap) return;  // never an address outside the image or the LDS
  const int rows = min(H_ROWS, src_h - y0);

  int shift[H_ROWS];
#pragma unroll
  for (int r = 0; r < H_ROWS; ++r) {
    const int64_t g0 = ((int64_t)(y0 + r) * src_w + x_lo) * 3;  // first byte of the span inside the image
    shift[r] = (int)(g0 & 3);
    if (r < rows) {
      const int64_t a0 = g0 - shift[r];
      const int nd = (shift[r] + span + 3) >> 2;
      uint8_t* row = lds + r * span_cap;
      for (int i = tid; i < nd; i += 256) {
        const int64_t at = a0 + 4 * (int64_t)i;
        uint32_t w = 0;
        if (at + 4 <= img_bytes) {
          w = *(const uint32_t*)(img + at);
        } else {
          for (int q = 0; q < 4; ++q)
            if (at + q < img_bytes) w |= (uint32_t)img[at + q] << (8 * q);
        }
        *(uint32_t*)(row + 4 * i) = w;
      }
    }
  }
  __syncthreads();

  const int b = b0 + tid;
  if (b >= row_bytes) return;
  const int xo = b / 3, c = b - 3 * xo;
  int xmin = bounds[2 * xo], n = bounds[2 * xo + 1];
  if (xmin < x_lo || xmin + n > x_hi || n > ksize) n = 0;  // (a table that is not monotone: no read outside the staged span)
  const int32_t* k = coef + (int64_t)xo * ksize;
  uint32_t acc[H_ROWS];
#pragma unroll
  for (int r = 0; r < H_ROWS; ++r) acc[r] = 1u << (PREC - 1);
  const int at0 = (xmin - x_lo) * 3 + c;
  for (int j = 0; j < n; ++j) {
    const uint32_t kv = (uint32_t)k[j];
#pragma unroll
    for (int r = 0; r < H_ROWS; ++r) acc[r] += kv * lds[r * span_cap + shift[r] + at0 + 3 * j];  // (rows past the image: never stored)
  }
#pragma unroll
  for (int r = 0; r < H_ROWS; ++r)
    if (r < rows) inter[(int64_t)(y0 + r) * pitch + b] = clip8(acc[r]);
}

// Vertical pass.  A block: 256 dwords (1024 bytes) of V_ROWS output rows; threads run along x, so a tap is one aligned
// dword load per lane from the intermediate (its pitch is a multiple of 16) and the row's window and coefficients are the
// same for the whole block.  A result byte is stored into every crop slot that holds it: the global target into crop0 (and
// crop0 + 1 for an image of tiling (1, 1) whose two crops are one computation), a pixel (y, x) of the tiled target into crop
// (ty, tx) for every window [ty * window, ty * window + crop) x [tx * window, tx * window + crop) that contains it.  Crop rows
// are crop * 3 bytes, which aligns nothing: byte stores.
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ packed, int n_entries, const uint8_t* __restrict__ ws,
                                                         uint8_t* __restrict__ out, Geometry g) {
  const int64_t* desc = (const int64_t*)packed;
  const int tid = threadIdx.x, bid = blockIdx.x;
  const int e = find_entry(desc, n_entries, bid, T_VBLK0);
  const int64_t* d = desc + (int64_t)(e >> 1) * DW;
  const int64_t* t = d + T0 + (e & 1) * TW;
  const int src_h = (int)d[0], th = (int)d[2], tw = (int)d[3], crop0 = (int)d[4], mode = (int)d[5];
  const int out_h = (int)t[T_OUT_H], out_w = (int)t[T_OUT_W], ksize = (int)t[T_KY_N];
  const int row_bytes = out_w * 3;
  const int64_t pitch = pitch_of(out_w);
  const int nseg = (int)((pitch + V_SEG - 1) / V_SEG);
  const int local = bid - (int)t[T_VBLK0], seg = local % nseg, yo0 = (local / nseg) * V_ROWS;
  if (yo0 >= out_h) return;
  const int b = seg * V_SEG + 4 * tid;
  if (b >= pitch) return;
  const int32_t* bounds = (const int32_t*)(packed + t[T_BY]);
  const int32_t* coef = (const int32_t*)(packed + t[T_KY]);
  int64_t inter_off = d[7];
  if (e & 1) inter_off += (int64_t)src_h * pitch_of(d[T0 + T_OUT_W]);
  const uint8_t* col = ws + inter_off + b;
  const int64_t crop_row = (int64_t)g.crop * 3, crop_bytes = crop_row * g.crop;
  const bool tiled = (e & 1) != 0;
  const int n_slots = tiled ? th * tw : (mode == MD_RESAMPLE_BOTH_SLOTS ? 2 : 1);
  if (crop0 < 0 || crop0 + (tiled ? 1 : 0) + n_slots > g.total_crops) return;  // never a store outside the crops buffer

  for (int yo = yo0; yo < min(yo0 + V_ROWS, out_h); ++yo) {
    const int ymin = bounds[2 * yo];
    int n = bounds[2 * yo + 1];
    if (ymin < 0 || ymin + n > src_h || n > ksize) n = 0;
    const int32_t* k = coef + (int64_t)yo * ksize;
    uint32_t a0 = 1u << (PREC - 1), a1 = a0, a2 = a0, a3 = a0;
    const uint8_t* p = col + (int64_t)ymin * pitch;
    for (int j = 0; j < n; ++j, p += pitch) {
      const uint32_t kv = (uint32_t)k[j], w = *(const uint32_t*)p;
      a0 += kv * (w & 255u);
      a1 += kv * ((w >> 8) & 255u);
      a2 += kv * ((w >> 16) & 255u);
      a3 += kv * (w >> 24);
    }
    const uint8_t v[4] = {clip8(a0), clip8(a1), clip8(a2), clip8(a3)};
    if (!tiled) {
      uint8_t* o = out + (int64_t)crop0 * crop_bytes + (int64_t)yo * crop_row;  // (out_h == out_w == crop: checked by the host)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (b + i < row_bytes) {
          o[b + i] = v[i];
          if (n_slots == 2) o[crop_bytes + b + i] = v[i];
        }
    } else {
      const int ty_hi = min(yo / g.window, th - 1), ty_lo = yo < g.crop ? 0 : (yo - g.crop) / g.window + 1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int bb = b + i;
        if (bb >= row_bytes) break;
        const int x = bb / 3, c = bb - 3 * x;
        const int tx_hi = min(x / g.window, tw - 1), tx_lo = x < g.crop ? 0 : (x - g.crop) / g.window + 1;
        for (int ty = ty_lo; ty <= ty_hi; ++ty)
          for (int tx = tx_lo; tx <= tx_hi; ++tx)
            out[(int64_t)(crop0 + 1 + ty * tw + tx) * crop_bytes + (int64_t)(yo - ty * g.window) * crop_row + (x - tx * g.window) * 3 + c] =
                v[i];
      }
    }
  }
}

struct Checked {
  int64_t h_blocks, v_blocks, ws_bytes;
  int span_cap;
};

// Everything the two kernels rely on, from the host copy of the descriptors.
md_status check_descriptors(const int64_t* desc, int32_t n_images, size_t packed_bytes, int32_t crop, int32_t window, int32_t margin_px,
                            int64_t total_crops, Checked* out) {
  MD_CHECK_ARG(desc && n_images >= 1 && n_images <= MD_RESAMPLE_MAX_IMAGES);
  MD_CHECK_ARG(crop >= 1 && window >= 1 && margin_px >= 0 && crop == window + 2 * margin_px && crop <= 4096);
  const int64_t head = (int64_t)n_images * DW * 8, total = (int64_t)packed_bytes;
  MD_CHECK_ARG(total >= head);
  int64_t slot = 0, ws = 0, hblk = 0, vblk = 0;
  int span_cap = 16;
  for (int i = 0; i < n_images; ++i) {
    const int64_t* d = desc + (int64_t)i * DW;
    const int64_t src_h = d[0], src_w = d[1], th = d[2], tw = d[3], mode = d[5];
    MD_CHECK_ARG(src_h >= 1 && src_h <= MD_RESAMPLE_MAX_SIDE && src_w >= 1 && src_w <= MD_RESAMPLE_MAX_SIDE);
    MD_CHECK_ARG(mode == MD_RESAMPLE_TWO_TARGETS || mode == MD_RESAMPLE_BOTH_SLOTS || mode == MD_RESAMPLE_ONE_SLOT);
    MD_CHECK_ARG(th >= 1 && tw >= 1 && th * tw <= 4096 && (mode == MD_RESAMPLE_TWO_TARGETS || (th == 1 && tw == 1)));
    MD_CHECK_ARG(d[4] == slot && d[7] == ws);  // crop slots and intermediates in image order, nothing shared
    MD_CHECK_ARG(d[6] >= head && d[6] % 16 == 0 && d[6] + src_h * src_w * 3 <= total);
    const int n_targets = mode == MD_RESAMPLE_TWO_TARGETS ? 2 : 1;
    for (int k = 0; k < 2; ++k) {
      const int64_t* t = d + T0 + k * TW;
      MD_CHECK_ARG(t[T_HBLK0] == hblk && t[T_VBLK0] == vblk);
      if (k >= n_targets) continue;
      const int64_t out_h = t[T_OUT_H], out_w = t[T_OUT_W], kxn = t[T_KX_N], kyn = t[T_KY_N];
      if (k == 0) MD_CHECK_ARG(out_h == crop && out_w == crop);
      else MD_CHECK_ARG(out_h == th * window + 2 * margin_px && out_w == tw * window + 2 * margin_px);
      MD_CHECK_ARG(out_h <= MD_RESAMPLE_MAX_SIDE && out_w <= MD_RESAMPLE_MAX_SIDE);
      MD_CHECK_ARG(kxn >= 1 && kxn <= 6 * MD_RESAMPLE_MAX_SIDE + 8 && kyn >= 1 && kyn <= 6 * MD_RESAMPLE_MAX_SIDE + 8);
      const int64_t offs[4] = {t[T_BX], t[T_KX], t[T_BY], t[T_KY]}, sizes[4] = {out_w * 8, out_w * kxn * 4, out_h * 8, out_h * kyn * 4};
      for (int q = 0; q < 4; ++q) MD_CHECK_ARG(offs[q] >= head && offs[q] % 4 == 0 && offs[q] + sizes[q] <= total);
      // the widest staged span of a horizontal segment: its output pixels' centres are at most (86 - 1) * scale apart, a window
      // reaches ceil(support) + 1 to either side; + 3 bytes of alignment slack, rounded to 16
      const double scale = (double)src_w / (double)out_w, support = 3.0 * (scale < 1.0 ? 1.0 : scale);
      int64_t px = (int64_t)((H_SEG / 3 + 1) * scale + 2.0 * support + 4.0);
      if (px > src_w) px = src_w;
      const int64_t cap = (px * 3 + 3 + 15) / 16 * 16;
      if (cap * H_ROWS > LDS_MAX) return MD_ERR_UNSUPPORTED;
      if (cap > span_cap) span_cap = (int)cap;
      hblk += ((out_w * 3 + H_SEG - 1) / H_SEG) * ((src_h + H_ROWS - 1) / H_ROWS);
      vblk += ((pitch_of(out_w) + V_SEG - 1) / V_SEG) * ((out_h + V_ROWS - 1) / V_ROWS);
      ws += src_h * pitch_of(out_w);
    }
    slot += mode == MD_RESAMPLE_ONE_SLOT ? 1 : th * tw + 1;
    MD_CHECK_ARG(hblk <= 0x7fffffff && vblk <= 0x7fffffff);
  }
  MD_CHECK_ARG(slot == total_crops);
  *out = Checked{hblk, vblk, ws, span_cap};
  return MD_OK;
}
}  // namespace

extern "C" size_t md_image_resample_workspace_bytes(const int64_t* host_desc, int32_t n_images) {
  if (!host_desc || n_images < 1 || n_images > MD_RESAMPLE_MAX_IMAGES) return 0;
  int64_t ws = 0;
  for (int i = 0; i < n_images; ++i) {
    const int64_t* d = host_desc + (int64_t)i * DW;
    if (d[0] < 1 || d[0] > MD_RESAMPLE_MAX_SIDE) return 0;
    for (int k = 0; k < (d[5] == MD_RESAMPLE_TWO_TARGETS ? 2 : 1); ++k) {
      const int64_t out_w = d[T0 + k * TW + T_OUT_W];
      if (out_w < 1 || out_w > MD_RESAMPLE_MAX_SIDE) return 0;
      ws += d[0] * pitch_of(out_w);
    }
  }
  return (size_t)ws;
}

extern "C" md_status md_image_resample_crops(const void* packed, size_t packed_bytes, const int64_t* host_desc, int32_t n_images,
                                             int32_t crop, int32_t window, int32_t margin_px, void* crops_out, int32_t total_crops,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  MD_CHECK_ARG(packed && host_desc && crops_out && workspace && total_crops >= 1);
  MD_CHECK_ARG(((uintptr_t)packed % 16) == 0 && ((uintptr_t)workspace % 16) == 0);
  Checked c;
  MD_TRY(check_descriptors(host_desc, n_images, packed_bytes, crop, window, margin_px, total_crops, &c));
  if ((int64_t)workspace_bytes < c.ws_bytes) return MD_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)c.h_blocks), dim3(256), (size_t)c.span_cap * H_ROWS, s, (const uint8_t*)packed,
                     2 * n_images, (uint8_t*)workspace, c.span_cap);
  hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)c.v_blocks), dim3(256), 0, s, (const uint8_t*)packed, 2 * n_images,
                     (const uint8_t*)workspace, (uint8_t*)crops_out, Geometry{crop, window, total_crops});
  return md_launch_status();
}
