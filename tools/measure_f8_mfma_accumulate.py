"""The accumulate error of v_mfma_f32_32x32x64_f8f6f4 as md_gemm_f8 uses it, measured at the smallest problem the kernel
accepts: one 256 x 256 tile, K = 64 (ONE instruction per output block), random e4m3 operands, a power-of-two a_scale, unit
weight scales and no bias, so the fp32 value before the bf16 rounding is the instruction's result itself.  Per element
|got - exact| - half a bf16 spacing is a lower bound of that error; it is printed in units of K u mag (u = 2^-23), the
accumulate term of util.compare_f8_elementwise.  The largest ratio over the draws is util.F8_MFMA_MEASURED_U; its output is
kept in profiles/gemm_f8_exact_tests_gpu.txt.

    python tools/measure_f8_mfma_accumulate.py [draws]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gemm_f8_exact_gpu as T  # noqa: E402  (its guarded launch of md_gemm_f8)
from moondream_amd import _lib  # noqa: E402
from util import bf16_spacing, gemm_f8_exact  # noqa: E402

M = N = 256
K = 64
U = 2.0 ** -23


def draw(seed):
    """e4m3 codes drawn like the tests' (max -> 448); the scales handed to the kernel are exact powers of two."""
    g = torch.Generator(device="cuda").manual_seed(1000 + seed)
    x = torch.randn(M, K, generator=g, device="cuda")
    w = torch.randn(N, K, generator=g, device="cuda")
    a8 = (x / (x.abs().max() / 448)).clamp(-448, 448).to(T.F8).view(torch.uint8)
    w8 = (w / (w.abs().amax(dim=1, keepdim=True) / 448)).clamp(-448, 448).to(T.F8).view(torch.uint8)
    return a8, 2.0 ** -12, w8, torch.ones(N, device="cuda")


def main(draws=48):
    lib = _lib.load()
    worst = 0.0
    for seed in range(draws):
        a8, a_scale, w8, wscale = draw(seed)
        exact, mag = gemm_f8_exact(a8, a_scale, w8, wscale, None)
        case = T.Case(f"measure{seed}", M, N, K, bias=False)
        got, _ = T.launch(lib, case, M, a8, a_scale, w8, wscale, None, None, 1.0)
        g = got.double()
        err = ((g - exact).abs() - 0.5 * bf16_spacing(torch.maximum(g.abs(), exact.abs()))).clamp_min(0)
        ratio = err / (K * U * mag)
        r = float(ratio.max())
        row, col = divmod(int(ratio.argmax()), N)
        worst = max(worst, r)
        print(f"draw {seed}: largest (|got - exact| - half spacing) / (K u mag) = {r:.4f} at ({row}, {col}): exact "
              f"{float(exact[row, col]):.6e} mag {float(mag[row, col]):.6e} got {float(g[row, col]):.6e}; share above 1: "
              f"{float((ratio > 1).double().mean()):.2e}")
    print(f"LARGEST RATIO over {draws} draws of one {M} x {N} x {K} tile: {worst:.4f} (in units of u = 2^-23 per accumulate step)")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 48)
