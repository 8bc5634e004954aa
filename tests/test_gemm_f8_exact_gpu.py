"""md_gemm_f8 (csrc/gemm_f8.hip) held to an exact probe and to the per-element intervals of util.compare_f8_elementwise, at the
shapes the rel-rms tests of test_kernels_gpu.py never launch: a workgroup's second and third tile (more tiles than CUs), K of
one to three slices (shorter than the operand ring runs ahead), the grouped tile order with a ragged last group, GELU / fp8
column switches on 64-column boundaries, an all-fp8 output, no bias, an in-place residual, and leading dimensions wider than
the data.  Every launch is surrounded by guard rows and guard columns that must keep their bit pattern.

The exact probe needs no tolerance: A8 and W8 hold integers in [-4, 4] (exact e4m3 codes), a_scale and wscale[n] are powers
of two (wscale varies with n % 5), bias[n] = n % 7 - 3.  Every product, every partial sum in any order (|sum| <= 16 K < 2^24)
and the scaled FMA are exact in fp32 -- probe_headroom() checks it for every shape, here and without a GPU in
test_util_cpu.py -- so the bf16 output must equal the round-to-nearest-even of the float64 value bit for bit; the residual's
second rounding and a power-of-two fp8 quantisation are modelled, and the GELU is held to the error term of gelu_tanh_f32x2
alone since its input is known to the bit.

The same shape list then runs with random operands drawn like test_kernels_gpu.f8_case, against the derived intervals."""
import ctypes as C
import math
from dataclasses import dataclass

import pytest
import torch

from moondream_amd import _lib
from util import compare_f8_elementwise, f8_code_interval, f8_output_interval, gemm_f8_exact, round_to_bf16

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
F8 = torch.float8_e4m3fn
GUARD_BITS = 0x7FC1   # a bf16 NaN with a payload no kernel produces
GUARD_CODE = 0x7F     # e4m3fn NaN: the epilogue saturates at +-448 and never stores it
BIAS, GELU, RESIDUAL = 0, 1, 2
TILE = 256
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pad64(v):
    return (v + 63) // 64 * 64


@dataclass(frozen=True)
class Case:
    """One launch.  m / n / k are literal, or for m a name resolved against the CU count (persistent_rows)."""
    name: str
    m: object
    n: int
    k: int
    epi: int = BIAS
    gelu_from: int = 0
    f8_from: object = None     # None: no fp8 output; 0: all-fp8, c == NULL
    store_pad: int = 0
    bias: bool = True
    res_row_mod: int = 0
    res_rows: int = 0          # rows of the residual operand (0: m)
    in_place: bool = False

    def __str__(self):
        return self.name


def grid_size():
    """(CU count, workgroups of a launch with more tiles than that).  The second number restates launch() in csrc/gemm_f8.hip
    (``n_cu = n_cu >= 8 ? (n_cu / 8) * 8 : 8`` and ``min(nwg, n_cu)`` just below it): the tile-count assertions of run_case
    are made against it, so if that rule changes, change it here too -- or the persistent cases stop proving that a
    workgroup takes a second and a third tile.  On an MI355X both numbers are 256."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    return cu, max(8, cu // 8 * 8)


def persistent_rows(kind):
    """Row counts whose last row tile holds 37 rows, for n = 1000 (four column tiles) resp. n = 2368 (ten, group_m = 4)."""
    cu, grid = grid_size()
    if kind == "two":      # grid < tiles < 2 grid: some workgroups take two tiles, some one
        tiles_m = (3 * grid // 2) // 4
    elif kind == "three":  # tiles > 2 grid: a workgroup takes three
        tiles_m = 2 * grid // 4 + 1
    else:                  # "grouped": tiles_m % 4 == 3 (ragged last group), more tiles than workgroups, nwg % 8 != 0 (uneven XCD chunks)
        tiles_m = next(t for t in range(3, 1 << 20, 4) if t * 10 > grid and (t * 10) % 8 != 0)
    return (tiles_m - 1) * TILE + 37


def tile_counts(m, n_store):
    return (m + TILE - 1) // TILE, (n_store + TILE - 1) // TILE


def short_k_cases():
    out = []
    for k in (64, 128, 192, 256, 320, 588):
        out += [Case(f"k{k}-bias", 300, 320, k), Case(f"k{k}-residual", 300, 320, k, epi=RESIDUAL), Case(f"k{k}-gelu", 300, 320, k, epi=GELU)]
    return out


def persistent_cases(kinds_k):
    out = []
    for kind, k in kinds_k:
        out += [Case(f"{kind}-tiles-k{k}-bias", kind, 1000, k), Case(f"{kind}-tiles-k{k}-residual", kind, 1000, k, epi=RESIDUAL),
                Case(f"{kind}-tiles-k{k}-gelu", kind, 1000, k, epi=GELU),
                Case(f"{kind}-tiles-k{k}-gelu-f8tail", kind, 1000, k, epi=GELU, gelu_from=512, f8_from=512)]
    return out


OTHER_CASES = [
    Case("grouped-order-bias", "grouped", 2368, 64),
    Case("grouped-order-gelu-f8tail", "grouped", 2368, 64, epi=GELU, gelu_from=1152, f8_from=1152),
    Case("gelu192-f8-192", 300, 448, 128, epi=GELU, gelu_from=192, f8_from=192),
    Case("gelu128-f8-320", 300, 448, 128, epi=GELU, gelu_from=128, f8_from=320),
    Case("gelu64-no-f8", 300, 448, 128, epi=GELU, gelu_from=64),
    Case("all-f8-gelu", 300, 448, 128, epi=GELU, f8_from=0),
    Case("all-f8-bias", 300, 448, 128, f8_from=0),
    Case("pad-cols-bf16", 300, 4304, 64, store_pad=1),
    Case("pad-cols-gelu-f8", 300, 4304, 64, epi=GELU, gelu_from=1152, f8_from=1152, store_pad=1),
    Case("residual-mod129", 700, 320, 128, epi=RESIDUAL, res_row_mod=129, res_rows=129),
    Case("residual-in-place", 300, 320, 128, epi=RESIDUAL, in_place=True),
    Case("bias-null", 300, 320, 128, bias=False),
    Case("residual-bias-null", 300, 320, 128, epi=RESIDUAL, bias=False),
    Case("long-k", 300, 1152, 4304),
]
ALL_KINDS = [("two", 64), ("two", 256), ("three", 64), ("three", 256)]
EXACT_CASES = short_k_cases() + persistent_cases(ALL_KINDS) + OTHER_CASES
RANDOM_CASES = short_k_cases() + persistent_cases([("two", 64), ("three", 256)]) + OTHER_CASES


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def probe_a_scale(k_pad):
    """A power of two that puts the widest columns (wscale = 1) at a standard deviation of about 4: a sum of K products of two
    uniform integers in [-4, 4] has the standard deviation (20 / 3) sqrt(K)."""
    return 2.0 ** round(math.log2(0.6 / math.sqrt(k_pad)))


def probe_headroom(k_pad, a_scale):
    """The exact probe's fp32 arithmetic is exact: partial sums are integers below 2^24, and acc * sc + bias is a multiple of
    the smallest scale product whose magnitude stays below 2^24 of them (one FMA, so only the final value needs to fit)."""
    assert 16 * k_pad < 2 ** 24
    quantum = a_scale * 2.0 ** -4                      # wscale in {1, 1/2, .., 1/16}; the bias is an integer, a multiple of it
    assert quantum <= 1.0 and math.log2(quantum) == round(math.log2(quantum))
    assert (16 * k_pad * a_scale + 3) / quantum < 2 ** 24, (k_pad, a_scale)


def probe_operands(m, n, k, with_bias):
    k_pad, n_pad = pad64(k), pad64(n)
    g = torch.Generator(device=DEV).manual_seed(7 * m + 3 * n + k)
    a = torch.zeros(m, k_pad, device=DEV)
    w = torch.zeros(n_pad, k_pad, device=DEV)
    a[:, :k] = torch.randint(-4, 5, (m, k), generator=g, device=DEV).float()
    w[:n, :k] = torch.randint(-4, 5, (n, k), generator=g, device=DEV).float()
    cols = torch.arange(n_pad, device=DEV)
    wscale = torch.exp2(-(cols % 5).float())
    bias = ((cols % 7) - 3).to(BF16)
    bias[n:] = 0                                       # padded columns: zero weights, zero bias
    a_scale = probe_a_scale(k_pad)
    probe_headroom(k_pad, a_scale)
    return a.to(F8).view(torch.uint8), a_scale, w.to(F8).view(torch.uint8), wscale, (bias if with_bias else None)


def random_operands(m, n, k, with_bias):
    """As test_kernels_gpu.f8_case draws them: one activation scale (max |x| -> 448), one weight scale per output channel."""
    k_pad, n_pad = pad64(k), pad64(n)
    g = torch.Generator(device=DEV).manual_seed(11 * m + 5 * n + k)
    x = torch.randn(m, k, generator=g, device=DEV).to(BF16).float()
    w = (torch.randn(n, k, generator=g, device=DEV) / math.sqrt(k)).to(BF16).float()
    bias = torch.zeros(n_pad, dtype=BF16, device=DEV)
    bias[:n] = (torch.randn(n, generator=g, device=DEV) * 0.1).to(BF16)
    a_scale = float(x.abs().max()) / 448.0
    wscale = torch.ones(n_pad, device=DEV)
    wscale[:n] = w.abs().amax(dim=1) / 448.0
    a8 = torch.zeros(m, k_pad, dtype=torch.uint8, device=DEV)
    w8 = torch.zeros(n_pad, k_pad, dtype=torch.uint8, device=DEV)
    a8[:, :k] = (x / a_scale).clamp(-448, 448).to(F8).view(torch.uint8)
    w8[:n, :k] = (w / wscale[:n, None]).clamp(-448, 448).to(F8).view(torch.uint8)
    return a8, a_scale, w8, wscale, (bias if with_bias else None)


_PROBLEMS = {}


def problem(kind, m, n, k, with_bias):
    """Operands and their float64 reference, computed once per shape and shared by the epilogue cases that follow each other
    in the list (only the latest shape is kept: the largest reference is a quarter of a gigabyte)."""
    key = (kind, m, n, k, with_bias)
    if key not in _PROBLEMS:
        _PROBLEMS.clear()
        ops = (probe_operands if kind == "exact" else random_operands)(m, n, k, with_bias)
        _PROBLEMS[key] = ops + gemm_f8_exact(*ops)
    return _PROBLEMS[key]


# ---------------------------------------------------------------------------------------------------------------------
# one guarded launch
# ---------------------------------------------------------------------------------------------------------------------
def launch(lib, case, m, a8, a_scale, w8, wscale, bias, r, c8_inv_scale):
    """md_gemm_f8 with lda > k_pad, ldc / ldc8 / ldr wider than the stored width, 64 guard rows below both outputs.  Returns the
    bf16 columns and the e4m3 columns (either may be None) after checking that every guard element kept its bits."""
    n_pad, k_pad = w8.shape
    width = n_pad if case.store_pad else case.n
    n_bf = width if case.f8_from is None else case.f8_from
    n_f8 = 0 if case.f8_from is None else width - case.f8_from
    a_buf = torch.full((m, k_pad + 64), 0x38, dtype=torch.uint8, device=DEV)   # 1.0 beyond k_pad: a slice too many is seen
    a_buf[:, :k_pad] = a8
    cbuf = c8buf = None
    if n_bf > 0:
        cbuf = torch.full((m + 64, n_bf + 64), GUARD_BITS, dtype=torch.int16, device=DEV)
    if n_f8 > 0:
        c8buf = torch.full((m + 64, n_f8 + 64), GUARD_CODE, dtype=torch.uint8, device=DEV)
    r_ptr, ldr = None, 0
    if case.epi == RESIDUAL:
        if case.in_place:
            cbuf.view(BF16)[:m, :n_bf] = r
            r_ptr, ldr = cbuf.data_ptr(), cbuf.stride(0)
        else:
            r_buf = torch.full((r.shape[0], width + 64), GUARD_BITS, dtype=torch.int16, device=DEV).view(BF16)
            r_buf[:, :width] = r
            r_ptr, ldr = r_buf.data_ptr(), r_buf.stride(0)
    lin = _lib.MdLinearF8(w8.data_ptr(), wscale.data_ptr(), bias.data_ptr() if bias is not None else None, case.n, case.k, n_pad, k_pad)
    args = _lib.MdGemmF8Args(a_buf.data_ptr(), a_buf.stride(0), float(a_scale), lin,
                             cbuf.data_ptr() if cbuf is not None else None, cbuf.stride(0) if cbuf is not None else 0,
                             c8buf.data_ptr() if c8buf is not None else None, c8buf.stride(0) if c8buf is not None else 0,
                             float(c8_inv_scale), int(case.f8_from or 0), r_ptr, ldr, case.res_row_mod, m, case.epi, case.store_pad,
                             case.gelu_from)
    _lib.check(lib.md_gemm_f8(C.byref(args), stream()), "md_gemm_f8")
    torch.cuda.synchronize()
    got = got8 = None
    if cbuf is not None:
        assert bool((cbuf[m:] == GUARD_BITS).all()), f"{case}: bf16 rows below the result were written"
        assert bool((cbuf[:m, n_bf:] == GUARD_BITS).all()), f"{case}: bf16 columns right of the result were written"
        got = cbuf.view(BF16)[:m, :n_bf]
        assert not bool((cbuf[:m, :n_bf] == GUARD_BITS).any()), f"{case}: bf16 elements left unwritten"
    if c8buf is not None:
        assert bool((c8buf[m:] == GUARD_CODE).all()), f"{case}: e4m3 rows below the result were written"
        assert bool((c8buf[:m, n_f8:] == GUARD_CODE).all()), f"{case}: e4m3 columns right of the result were written"
        got8 = c8buf[:m, :n_f8]
        assert not bool((got8 == GUARD_CODE).any()), f"{case}: e4m3 elements left unwritten (or NaN)"
    return got, got8


def run_case(lib, case, kind):
    m = persistent_rows(case.m) if isinstance(case.m, str) else case.m
    a8, a_scale, w8, wscale, bias, exact, mag = problem(kind, m, case.n, case.k, case.bias)
    n_pad, k_pad = w8.shape
    width = n_pad if case.store_pad else case.n
    tiles_m, tiles_n = tile_counts(m, width)
    cu, grid = grid_size()
    print(f"{kind} {case}: m {m} n {case.n} k {case.k}: {tiles_m} x {tiles_n} = {tiles_m * tiles_n} tiles, {cu} CUs, {min(grid, tiles_m * tiles_n)} workgroups")
    # the paths the case is there for exist on this device
    if case.m == "two":
        assert grid < tiles_m * tiles_n < 2 * grid and tiles_n == 4 and m % TILE == 37
    elif case.m == "three":
        assert tiles_m * tiles_n > 2 * grid and tiles_n == 4 and m % TILE == 37
    elif case.m == "grouped":
        assert tiles_n == 10 and tiles_m % 4 == 3 and tiles_m * tiles_n > grid and (tiles_m * tiles_n) % 8 != 0
    exact, mag = exact[:, :width], mag[:, :width]
    r = r_rows = None
    if case.epi == RESIDUAL:
        g = torch.Generator(device=DEV).manual_seed(99)
        rows = case.res_rows or m
        if kind == "exact":   # integers and halves up to +-8: bf16 values whose fp32 sum with the output rounds like any other
            r = (torch.randint(-16, 17, (rows, width), generator=g, device=DEV).float() / 2).to(BF16)
        else:
            r = torch.randn(rows, width, generator=g, device=DEV).to(BF16)
        r_rows = r[torch.arange(m, device=DEV) % case.res_row_mod] if case.res_row_mod else r
    gelu_from = case.gelu_from if case.epi == GELU else None
    kw = dict(exact_acc=(kind == "exact"), residual=r_rows, gelu_from=gelu_from)
    c8_inv_scale = 1.0
    if case.f8_from is not None:
        lo, hi = f8_output_interval(exact, mag, k_pad, **kw)
        ref = hi[:, case.f8_from : case.n]             # the fp8 columns of the reference, padding left out
        if kind == "exact":
            c8_inv_scale = 32.0
        else:
            c8_inv_scale = 448.0 / float(ref.abs().max())
        codes = f8_code_interval(ref, ref, c8_inv_scale)[0]
        saturated = float((codes.abs() >= 448.0).double().mean())
        distinct = int(torch.unique(codes).numel())
        print(f"  reference fp8 part: {saturated:.4f} saturated, {distinct} distinct codes")
        assert saturated < 0.01 and distinct >= 30
    if gelu_from is not None and kind == "exact":
        pre = exact[:, gelu_from : case.n]
        share = float((pre.abs() < 4).double().mean())
        print(f"  reference GELU inputs: {share:.3f} with |x| < 4")
        assert share >= 0.5
    got, got8 = launch(lib, case, m, a8, a_scale, w8, wscale, bias, r, c8_inv_scale)
    if kind == "exact" and case.epi == BIAS and got is not None:
        want = exact.to(BF16)                          # float64 -> bf16 of a value with < 24 significant bits: one rounding
        assert torch.equal(got, want), f"{case}: {int((got != want).sum())} elements differ from the rounded exact value"
    compare_f8_elementwise(f"{kind} {case}", got, exact, mag, k_pad, got8=got8, f8_from=case.f8_from, c8_inv_scale=c8_inv_scale, **kw)
    if case.store_pad and width > case.n:
        n_bf = width if case.f8_from is None else case.f8_from
        if n_bf > case.n:
            assert bool((got[:, case.n :].view(torch.int16) == 0).all()), f"{case}: bf16 pad columns are not +0"
        if got8 is not None:
            assert bool((got8[:, max(case.n - case.f8_from, 0) :] == 0).all()), f"{case}: e4m3 pad columns are not 0x00"


@pytest.mark.parametrize("case", EXACT_CASES, ids=str)
def test_gemm_f8_exact_probe(lib, case):
    run_case(lib, case, "exact")


@pytest.mark.parametrize("case", RANDOM_CASES, ids=str)
def test_gemm_f8_random_operands_per_element(lib, case):
    run_case(lib, case, "random")


def test_reference_rounding_on_the_device_is_round_to_nearest_even():
    """util.round_to_bf16 as the references use it, on the device: ties included, it is the float32 -> bf16 conversion."""
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(1 << 16, generator=g, device=DEV) * torch.exp2(torch.randint(-20, 20, (1 << 16,), generator=g, device=DEV).float())
    ties = (torch.arange(256, 512, device=DEV).float() + 0.5) / 32          # every tie of the binade [8, 16)
    for v in (x, ties, -ties):
        assert torch.equal(round_to_bf16(v.double()), v.to(BF16).double())
