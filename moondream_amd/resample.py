"""Host plan of the device-side image preprocessing (csrc/preprocess.hip: md_image_resample_crops).

PIL's 8-bit LANCZOS resize is integer arithmetic once its coefficient tables exist: per output pixel a window
``[xmin, xmin + n)`` of taps with int32 coefficients at 22 fractional bits, ``((1 << 21) + sum k * pixel) >> 22`` clamped
to 0 .. 255, horizontally into a uint8 intermediate and then vertically.  ``coeffs`` builds those tables (Pillow's
``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the Lanczos-3 filter, in double precision with ``math.sin``);
``plan`` says, per image, which resizes the crops of ``image_crops.overlap_crop_image`` need; ``layout`` lays one ViT
chunk out as ONE upload: ``[descriptors | coefficient tables | raw RGB pixels, each image 16-byte aligned]``.

Pure Python / numpy: no GPU, no PIL.  The kernels implement the PIL branch of ``image_crops`` only.

Limits of the device path: every image side in 1 .. ``MAX_SIDE`` (16384).  ``plan`` returns None for a call with an image
outside them (a side of 0, or above 16384), and the caller tiles the whole call on the host as before.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .image_crops import crop_count

PRECISION_BITS = 32 - 8 - 2  # Pillow's Resample.c: coefficients at 22 fractional bits
MAX_SIDE = 16384
LANCZOS_SUPPORT = 3.0

# md_image_resample_crops' descriptor: DESC_WORDS int64 per image (include/moondream_hip.h)
DESC_WORDS = 32
D_SRC_H, D_SRC_W, D_TH, D_TW, D_CROP0, D_MODE, D_PIXELS, D_INTER = range(8)
D_TARGET0, D_TARGET_WORDS = 8, 12
T_OUT_H, T_OUT_W, T_KX_N, T_KY_N, T_BX, T_KX, T_BY, T_KY, T_HBLK0, T_VBLK0 = range(10)
MODE_TWO_TARGETS, MODE_BOTH_SLOTS, MODE_ONE_SLOT = 0, 1, 2
# the two launches' work units (the kernels' constants: the entry point checks the block prefixes against its own)
H_SEG_BYTES, H_ROWS, V_SEG_BYTES, V_ROWS = 256, 4, 1024, 8

_tables: Dict[Tuple[int, int], Tuple[np.ndarray, np.ndarray]] = {}


def coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out, 2] = (xmin, taps), k int32 [out, ksize]) of one axis, cached by (in, out).  Pillow's order of
    operations: the weights are summed in tap order and divided by that sum, then rounded away from zero
    at 22 bits.  ``in == out``: the one-tap identity table, which is Pillow's early return (a pass it skips)."""
    key = (int(in_size), int(out_size))
    hit = _tables.get(key)
    if hit is not None:
        return hit
    n_in, n_out = key
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resample.coeffs: sizes must be positive, got {key}")
    if n_in == n_out:
        bounds = np.stack([np.arange(n_out, dtype=np.int32), np.ones(n_out, dtype=np.int32)], axis=1)
        k = np.full((n_out, 1), 1 << PRECISION_BITS, dtype=np.int32)
    else:
        scale = n_in / n_out
        filterscale = max(scale, 1.0)
        support = LANCZOS_SUPPORT * filterscale
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / filterscale
        one = float(1 << PRECISION_BITS)
        # Pillow's loop, a row of taps at a time in numpy where the operations are the same IEEE double ones; the two that
        # are not are kept scalar: the sine (np.sin is not promised to round as math.sin does) and the sum of a row's
        # weights in tap order (cumsum adds sequentially, sum pairwise)
        center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # (astype truncates toward zero, as C's cast)
        xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
        taps = np.arange(ksize, dtype=np.int64)[None, :]
        live = taps < xmax[:, None]
        x = ((taps + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
        inside = live & (x >= -3.0) & (x < 3.0) & (x != 0.0)
        a, b = x[inside] * math.pi, (x[inside] / 3) * math.pi
        sin_a = np.array([math.sin(v) for v in a.tolist()], dtype=np.float64)
        sin_b = np.array([math.sin(v) for v in b.tolist()], dtype=np.float64)
        w = np.zeros((n_out, ksize), dtype=np.float64)
        w[inside] = (sin_a / a) * (sin_b / b)
        w[live & (x == 0.0)] = 1.0
        ww = np.cumsum(w, axis=1)[:, -1:]
        w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
        bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
        k = np.where(w < 0, -0.5 + w * one, 0.5 + w * one).astype(np.int32)
        k[~live] = 0
    bounds.setflags(write=False)
    k.setflags(write=False)
    _tables[key] = (bounds, k)
    return bounds, k


@dataclass(frozen=True)
class ImagePlan:
    """What one image's crops need.  ``targets``: the (height, width) of each resize -- the global ``crop x crop`` one, then
    (tiling above (1, 1) only) the tiled one, whose ``crop``-sized windows at stride ``window`` are the local crops.  An image
    of tiling (1, 1) has ONE resize: its global and its local crop are the same computation (window + 2 * margin_px == crop),
    and the result is written to both crop slots."""

    height: int
    width: int
    tiling: Tuple[int, int]
    n_crops: int
    targets: Tuple[Tuple[int, int], ...]

    @property
    def both_slots(self) -> bool:
        return len(self.targets) == 1


def geometry(v) -> Tuple[int, int, int]:
    """(crop, window, margin_px) of a vision config."""
    margin_px = v.enc_patch_size * v.overlap_margin
    window = (v.crop_size // v.enc_patch_size - 2 * v.overlap_margin) * v.enc_patch_size
    if window <= 0 or window + 2 * margin_px != v.crop_size:
        raise ValueError("resample.plan: crop_size must be patches x patch_size with room for the overlap margins")
    return v.crop_size, window, margin_px


def plan(sizes: Sequence[Tuple[int, int]], v) -> Optional[List[ImagePlan]]:
    """Per-image records for images of ``sizes`` [(height, width)], or None when one of them is outside the device path's
    limits (a side of 0 or above MAX_SIDE = 16384): the whole call then takes the host path."""
    crop, window, margin_px = geometry(v)
    out = []
    for h, w in sizes:
        h, w = int(h), int(w)
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            return None
        n, (th, tw) = crop_count(h, w, v.overlap_margin, v.max_crops, (crop, crop), v.enc_patch_size)
        targets = ((crop, crop),) if (th, tw) == (1, 1) else ((crop, crop), (th * window + 2 * margin_px, tw * window + 2 * margin_px))
        out.append(ImagePlan(h, w, (th, tw), n, targets))
    return out


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


def inter_pitch(out_w: int) -> int:
    """Bytes of one row of the horizontal pass's intermediate [H_in][pitch]: out_w * 3 rounded up to 16."""
    return _align(out_w * 3, 16)


@dataclass
class ChunkLayout:
    """The packed upload of one ViT chunk: ``head`` (descriptors + tables, uint8) goes to byte 0, image i's RGB bytes to
    ``pixel_off[i]``; ``desc`` int64 [n, DESC_WORDS] is the host copy of the descriptors the entry point validates."""

    desc: np.ndarray
    head: np.ndarray
    pixel_off: List[int]
    nbytes: int
    out_crops: int           # crop slots the launch writes
    ws_bytes: int            # the intermediates
    expand: Optional[List[int]]  # feats[expand] are the chunk's crops when slots were shared (dedup); else None

    def write(self, buf: np.ndarray, arrays: Sequence[np.ndarray]) -> None:
        """Fill ``buf`` (uint8 [nbytes]) from the images' [H, W, 3] uint8 arrays."""
        buf[: self.head.size] = self.head
        for d, off, a in zip(self.desc, self.pixel_off, arrays):
            h, w = int(d[D_SRC_H]), int(d[D_SRC_W])
            if a.shape != (h, w, 3) or a.dtype != np.uint8:
                raise ValueError(f"resample.ChunkLayout.write: image of shape {a.shape} {a.dtype}, planned ({h}, {w}, 3) uint8")
            np.copyto(buf[off : off + h * w * 3].reshape(h, w, 3), a)


def layout(records: Sequence[ImagePlan], v, dedup: bool = False) -> ChunkLayout:
    """Byte layout of one chunk.  ``dedup``: an image of tiling (1, 1) gets one crop slot (encoded once; ``expand`` maps the
    slots back to the chunk's crops)."""
    crop, window, margin_px = geometry(v)
    n = len(records)
    desc = np.zeros((n, DESC_WORDS), dtype=np.int64)
    off = n * DESC_WORDS * 8
    placed: Dict[Tuple[int, int], Tuple[int, int]] = {}  # a table is stored once per chunk
    parts: List[Tuple[int, np.ndarray]] = []

    def place(n_in: int, n_out: int) -> Tuple[int, int, int]:
        nonlocal off
        if (n_in, n_out) not in placed:
            bounds, k = coeffs(n_in, n_out)
            placed[(n_in, n_out)] = (off, off + bounds.nbytes)
            parts.extend([(off, bounds), (off + bounds.nbytes, k)])
            off += bounds.nbytes + k.nbytes
        b_off, k_off = placed[(n_in, n_out)]
        return b_off, k_off, coeffs(n_in, n_out)[1].shape[1]

    slot = ws = hblk = vblk = 0
    expand: List[int] = []
    for d, r in zip(desc, records):
        d[D_SRC_H], d[D_SRC_W], d[D_TH], d[D_TW], d[D_CROP0], d[D_INTER] = r.height, r.width, r.tiling[0], r.tiling[1], slot, ws
        d[D_MODE] = MODE_TWO_TARGETS if not r.both_slots else (MODE_ONE_SLOT if dedup else MODE_BOTH_SLOTS)
        for t in range(2):
            tw_ = d[D_TARGET0 + t * D_TARGET_WORDS :]
            if t < len(r.targets):
                oh, ow = r.targets[t]
                bx, kx, kxn = place(r.width, ow)
                by, ky, kyn = place(r.height, oh)
                tw_[: T_KY + 1] = (oh, ow, kxn, kyn, bx, kx, by, ky)
                tw_[T_HBLK0], tw_[T_VBLK0] = hblk, vblk
                hblk += -(-ow * 3 // H_SEG_BYTES) * -(-r.height // H_ROWS)
                vblk += -(-inter_pitch(ow) // V_SEG_BYTES) * -(-oh // V_ROWS)
                ws += r.height * inter_pitch(ow)
            else:
                tw_[T_HBLK0], tw_[T_VBLK0] = hblk, vblk  # no work: the next entry's first block
        slots = 1 if d[D_MODE] == MODE_ONE_SLOT else r.n_crops
        expand += [slot, slot] if d[D_MODE] == MODE_ONE_SLOT else list(range(slot, slot + slots))
        slot += slots
    pixel_off = []
    for d, r in zip(desc, records):
        off = _align(off, 16)
        d[D_PIXELS] = off
        pixel_off.append(off)
        off += r.height * r.width * 3
    head = np.zeros(pixel_off[0] if pixel_off else off, dtype=np.uint8)
    head[: desc.nbytes] = desc.view(np.uint8).reshape(-1)
    for at, a in parts:
        head[at : at + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return ChunkLayout(desc, head, pixel_off, off, slot, ws, expand if len(expand) != slot else None)


def unpack(buf: np.ndarray, n_images: int):
    """The inverse of ``ChunkLayout.write``: [(descriptor int64 [DESC_WORDS], pixels uint8 [H, W, 3], [(bounds_x, k_x, bounds_y,
    k_y) per target])] read back from the packed bytes alone."""
    desc = np.frombuffer(buf[: n_images * DESC_WORDS * 8].tobytes(), dtype=np.int64).reshape(n_images, DESC_WORDS)
    out = []

    def table(at: int, rows: int, cols: int) -> np.ndarray:
        return np.frombuffer(buf[at : at + rows * cols * 4].tobytes(), dtype=np.int32).reshape(rows, cols)

    for d in desc:
        h, w = int(d[D_SRC_H]), int(d[D_SRC_W])
        pixels = buf[int(d[D_PIXELS]) : int(d[D_PIXELS]) + h * w * 3].reshape(h, w, 3)
        tables = []
        for t in range(1 if d[D_MODE] != MODE_TWO_TARGETS else 2):
            oh, ow, kxn, kyn, bx, kx, by, ky = (int(x) for x in d[D_TARGET0 + t * D_TARGET_WORDS :][: T_KY + 1])
            tables.append((table(bx, ow, 2), table(kx, ow, kxn), table(by, oh, 2), table(ky, oh, kyn)))
        out.append((d, pixels, tables))
    return out
