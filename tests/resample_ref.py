"""Restatement of Pillow's 8-bit LANCZOS resize from ``moondream_amd.resample.coeffs`` tables, in numpy: the horizontal pass
into a uint8 intermediate, then the vertical pass, each ``((1 << 21) + sum k * pixel) >> 22`` in int32 (wrapping, as C's
int) clamped to 0 .. 255.  What the device kernels (csrc/preprocess.hip) are held to, and itself held to PIL byte for
byte by tests/test_resample_cpu.py."""
import numpy as np

from moondream_amd import resample


def _pass(src: np.ndarray, bounds: np.ndarray, k: np.ndarray) -> np.ndarray:
    """Resample axis 0 of ``src`` [n_in, ...] uint8 -> [n_out, ...] uint8."""
    n_out = bounds.shape[0]
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    wide = src.astype(np.int32)
    shape = (-1,) + (1,) * (src.ndim - 1)
    with np.errstate(over="ignore"):
        for i in range(n_out):
            lo, n = int(bounds[i, 0]), int(bounds[i, 1])
            acc = (wide[lo : lo + n] * k[i, :n].reshape(shape)).sum(axis=0, dtype=np.int32) + np.int32(1 << (resample.PRECISION_BITS - 1))
            out[i] = np.clip(acc >> resample.PRECISION_BITS, 0, 255)
    return out


def resize(img: np.ndarray, height: int, width: int) -> np.ndarray:
    """img uint8 [H, W, C] -> uint8 [height, width, C], the bytes of ``PIL.Image.resize((width, height), LANCZOS)``."""
    bx, kx = resample.coeffs(img.shape[1], width)
    by, ky = resample.coeffs(img.shape[0], height)
    inter = _pass(np.ascontiguousarray(img.transpose(1, 0, 2)), bx, kx).transpose(1, 0, 2)  # [H, width, C]
    return _pass(np.ascontiguousarray(inter), by, ky)


def crops_from_plan(img: np.ndarray, record: "resample.ImagePlan", v) -> np.ndarray:
    """The crops of ``image_crops.overlap_crop_image`` from a plan record: [n_crops, crop, crop, 3]."""
    crop, window, _ = resample.geometry(v)
    th, tw = record.tiling
    out = np.empty((record.n_crops, crop, crop, 3), dtype=np.uint8)
    out[0] = resize(img, *record.targets[0])
    tiled = out[0] if record.both_slots else resize(img, *record.targets[1])
    for ty in range(th):
        for tx in range(tw):
            out[1 + ty * tw + tx] = tiled[ty * window : ty * window + crop, tx * window : tx * window + crop]
    return out
