"""md_gemm_fp8w and md_gemm_fp8w_partial_f32_pair (csrc/gemm_fp8w.hip), both weight formats (MD_WSTREAM_E4M3,
MD_WSTREAM_INT4_G128), held to exact probes and to derived per-element bounds instead of a relative RMS over the whole output.
Every launch reads A as a column slice of a wider buffer filled with NaN (zeros only in [k, round_up(k, 64))) and writes into
an output surrounded by guard rows and guard columns (GUARD_BITS for bf16, a NaN for fp32 partials) that must keep their bits.

Which claim of gemm_fp8w.hip each part pins:

1. One-hot probe (test_one_hot_rows_return_every_stored_weight).  Row i of A is 1.0 at column k_i: C[i, :] must BE column k_i
   of the weight matrix.  Over all K columns, at m = 64 (ring, MF = 2), 32 (ring, MF = 1) and 8 (resident), this pins
     * "the bf16 operand the MFMA sees is bit for bit the weight the bf16 path multiplies with" (int4: bf16(bf16(q - zero) *
       scale), against weights.dequantize_int4, the loader's copy; fractional zero points so that the first rounding is live
       -- asserted: a single rounding changes more than 10 % of the weights),
     * every byte and nibble position of both fragment layouts ("lane l holds channel 32 nb + (l & 31), bytes 0..7 = ..."),
     * the (scale, zero) index of every 128-step and each lane's channel ("qparams: fp32 (scale, zero) at [step][n_pad]"),
       the per-channel scale[n] of the e4m3 epilogue,
     * rows past m replaying the last row (min(r, M - 1), min(l31, M - 1)) without a store, and padding channels being zero.
2. Integer probe (test_integer_probe_is_exact).  Operands for which every product, every partial sum in any order, the scale
   multiply and the bias add are exact in fp32 (probe_headroom): the stored bf16 must equal round_to_bf16(exact float64).
   It pins "both paths add the same products in the same order ... row-subset invariant" (row 0 alone reproduces row 0),
   the branch-free block loops ("step indices past the slice are clamped to its last step and their weights replaced by
   zeros") one step past a block of PFW = 8 and PFR = 4, resident_fits on both sides at K = 8192 and at m = 8 / 9, the MF
   switch at m = 32 / 33, "the loader supplies zeros beyond Ka itself" (NaN right behind Ka, K = 588 and 704), the
   ``n >= n_store`` skip with store_pad_cols = 0 at n % 64 = 8, and the GELU column switch on an 8-column boundary.
3. Random operands (test_random_operands_per_element): the same launches with randn operands against
   util.compare_f8_elementwise(accum_u = 2^-23): "the products are exact ... and accumulate in fp32", one rounding of
   acc * sc, one of the bias add, one to bf16, a second after the GELU.
4. Pair launches (test_pair_partials_per_slice): two UNEQUAL problems, so the early return
   ``n0 >= p.n_pad || slice >= p.slices`` runs for real workgroups; every slice's fp32 partial is held on its own to its K
   range [s per 128, min((s + 1) per, steps) 128) -- a step counted twice or by no slice is seen -- bit for bit with the
   integer operands; the slice counts restate md_gemm_fp8w_partial_slices.

The instruments are tested without a GPU in tests/test_util_cpu.py."""
import ctypes as C
import functools
import math
from dataclasses import dataclass

import pytest
import torch

from moondream_amd import _lib
from moondream_amd.weights import PackedLinearFp8, PackedLinearInt4, dequantize_int4
from util import (compare_elementwise, compare_f8_elementwise, dequantize_int4_single_rounding, pack_int4, quantize_int4, round_to_bf16,
                  wstream_exact)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
GUARD_BITS = 0x7FC1   # a bf16 NaN with a payload no kernel produces
BIAS, GELU = 0, 1
E4M3, INT4 = _lib.MD_WSTREAM_E4M3, _lib.MD_WSTREAM_INT4_G128
FORMATS = [E4M3, INT4]
FMT_NAME = {E4M3: "e4m3", INT4: "int4"}
STEP = 128
A_OFF = 8             # bf16 elements = 16 bytes: where the data start inside the NaN-filled activation buffer
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pad64(v):
    return (v + 63) // 64 * 64


def pad128(v):
    return (v + 127) // 128 * 128


@dataclass(frozen=True)
class Case:
    """One shape of md_gemm_fp8w; ``formats``: the weight formats it runs in (int4 needs k % 128 == 0)."""
    m: int
    k: int
    n: int
    store_pad: int = 1
    formats: tuple = (E4M3, INT4)
    why: str = ""

    def __str__(self):
        return f"m{self.m}-k{self.k}-n{self.n}" + ("" if self.store_pad else "-nopad")

    def gelu_from(self):
        """An 8-column boundary that is no 32- or 64-column boundary, in the upper half of the channels."""
        return 8 * (self.n // 16) + 8


CASES = [
    Case(3, 8192, 128, why="resident_fits at long K: 3 rows x 64 steps fit the LDS"),
    Case(4, 8192, 128, why="... 4 rows do not: the ring with 4 rows"),
    Case(8, 2048, 192, why="m <= 8: resident, two full blocks of 8 steps"),
    Case(9, 2048, 192, why="m = 9: ring"),
    Case(32, 1152, 192, why="MF = 1, one step past two ring blocks"),
    Case(33, 1152, 192, why="MF = 2, row 32 alone in the second row block"),
    Case(64, 640, 64, why="one step past a ring block"),
    Case(1, 128, 64, why="one row, one step"),
    Case(64, 1152, 200, store_pad=0, why="n % 64 = 8 without pad columns: the n >= n_store skip; guard columns from 200 on"),
    Case(7, 588, 1152, formats=(E4M3,), why="ragged K: zeros only in [588, 640), 5 steps resident, 18 workgroups"),
    Case(40, 704, 256, formats=(E4M3,), why="Ka = 704 < k_pad = 768: the loader's own zeros"),
    # added from reading the kernel
    Case(5, 1152, 64, why="resident, one step past a block of PFW = 8"),
    Case(8, 1024, 64, why="resident, exactly one block"),
    Case(33, 512, 64, why="ring, exactly one block of PFR = 4"),
    Case(64, 128, 64, why="ring with a single step: three of the four prefetched steps are dead"),
]
CASE_FORMATS = [(c, f) for c in CASES for f in c.formats]


def case_id(v):
    return FMT_NAME[v] if isinstance(v, int) else str(v)


# ---------------------------------------------------------------------------------------------------------------------
# layers: the packed stream and, for the references, the operands the kernel sees
# ---------------------------------------------------------------------------------------------------------------------
class Layer:
    """A packed weight stream.  ``q`` [n_pad, k_pad] and ``scale`` ([n_pad] fp32, or None for int4) are the arguments of
    util.wstream_exact; ``weight`` [n_pad, k_pad] bf16 is what a one-hot row must return."""

    def __init__(self, fmt, n, k, packed, q, scale, weight):
        self.fmt, self.n, self.k, self.packed = fmt, n, k, packed
        self.n_pad, self.k_pad = packed.n_pad, packed.k_pad
        self.q, self.scale, self.weight = q, scale, weight
        assert tuple(q.shape) == tuple(weight.shape) == (self.n_pad, self.k_pad)

    def struct(self, bias):
        p = self.packed
        params = p.scale if self.fmt == E4M3 else p.qparams
        return _lib.MdLinearFp8(p.w.data_ptr(), params.data_ptr(), bias.data_ptr() if bias is not None else None, self.n, self.k,
                                self.n_pad, self.k_pad, self.fmt)


def e4m3_layer(w, dev):
    """``w`` float [n, k] -> PackedLinearFp8 over the zero-padded [n_pad][round_up(k, 64)] packing PackedModel.enable_fp8_decode hands
    it, but in fp32: the largest of a channel's bf16 weights has 8 significant bits, and a few dozen distinct scales among
    hundreds of channels would hide a channel that reads its neighbour's."""
    n, k = w.shape
    wp = torch.zeros(pad64(n), pad64(k), dtype=torch.float32, device=dev)
    wp[:n, :k] = w.to(dev)
    p = PackedLinearFp8(wp, None, n, k)
    assert p.k_pad == pad128(k)
    weight = (p.q.float() * p.scale[:, None]).to(BF16)      # one fp32 product rounded to bf16: the kernel's acc * sc for a one-hot row
    return Layer(E4M3, n, k, p, p.q.float(), p.scale, weight)


def int4_layer(packed, scale, zero, n, dev):
    """The checkpoint triple -> PackedLinearInt4; the reference weight is dequantize_int4's, the loader's bf16 copy."""
    p = PackedLinearInt4([(packed, scale, zero, n)], None, dev)
    weight = torch.zeros(p.n_pad, p.k, dtype=BF16, device=dev)
    weight[:n] = dequantize_int4(packed, scale, zero, n).to(dev)
    return Layer(INT4, n, p.k, p, weight, None, weight)


def gen(dev, *seed):
    return torch.Generator(device=dev).manual_seed(sum(s * f for s, f in zip(seed, (1, 7, 131, 1009, 9176))))


@functools.lru_cache(maxsize=6)
def random_layer(fmt, k, n, dev=DEV):
    """Gaussian weights scaled 1 / sqrt(K), like test_kernels_gpu.py: per-channel scales that are no powers of two and all
    distinct (e4m3); fractional zero points, every group with its own scale and zero (int4, zero_shift = 0.3)."""
    w = torch.randn(n, k, generator=gen("cpu", 1, fmt, k, n)) / math.sqrt(k)
    if fmt == E4M3:
        layer = e4m3_layer(w, dev)
        sc = layer.scale[:n]
        assert int(torch.unique(sc).numel()) == n, "every channel has its own scale"
        assert not bool((torch.frexp(sc)[0] == 0.5).any()), "no scale is a power of two"
        return layer
    assert k % STEP == 0
    packed, scale, zero = quantize_int4(w, zero_shift=0.3)
    groups = n * k // STEP
    assert int(torch.unique(torch.cat([scale, zero], 1), dim=0).shape[0]) == groups, "every group has its own (scale, zero)"
    assert int(torch.unique(scale).numel()) > 0.99 * groups and int(torch.unique(zero).numel()) > 0.99 * groups
    double, single = dequantize_int4(packed, scale, zero, n), dequantize_int4_single_rounding(packed, scale, zero, n)
    share = float((double != single).double().mean())
    assert share >= 0.10, f"the first rounding is live in only {share:.3f} of the weights: the probe could pass without it"
    return int4_layer(packed, scale, zero, n, dev)


def probe_weights(fmt, k, n, g):
    """The integer probe's stored numbers (CPU).  e4m3: ``w`` [n, k], multiples of 32 in [-448, 448] with one +-448 in every
    channel.  int4: (nibbles [n, k], scale [n, k / 128] = 2^-(g % 3), zero [n, k / 128] integers in 0..15), g the group index."""
    if fmt == E4M3:
        w = 32.0 * torch.randint(-14, 15, (n, k), generator=g).float()
        peak = torch.randint(0, k, (n,), generator=g)
        sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
        w[torch.arange(n), peak] = 448.0 * sign
        return w
    steps = k // STEP
    q = torch.randint(0, 16, (n, k), generator=g).to(torch.uint8)
    group = torch.arange(n * steps).reshape(n, steps)
    scale = torch.exp2(-(group % 3).float())
    zero = torch.randint(0, 16, (n, steps), generator=g).float()
    return q, scale, zero


@functools.lru_cache(maxsize=6)
def probe_layer(fmt, k, n, dev=DEV):
    g = gen("cpu", 2, fmt, k, n)
    if fmt == E4M3:
        w = probe_weights(fmt, k, n, g)
        layer = e4m3_layer(w, dev)
        assert bool((layer.scale == 1).all()), "one +-448 per channel: every scale is exactly 1"
        assert torch.equal(layer.q[:n, :k], w.to(dev)) and not bool(layer.q[n:].any()) and not bool(layer.q[:, k:].any())
        return layer
    q, scale, zero = probe_weights(fmt, k, n, g)
    layer = int4_layer(*pack_int4(q, scale, zero), n, dev)
    want = (q.float() - zero.repeat_interleave(STEP, 1)) * scale.repeat_interleave(STEP, 1)   # exact in fp32 and in bf16
    assert torch.equal(layer.weight[:n].float(), want.to(dev))
    return layer


PROBE_A_MAX = {E4M3: 4, INT4: 8}
PROBE_W_UNIT = {E4M3: (32.0, 14), INT4: (0.25, 60)}   # (the common power of two of the weights, max |w| in units of it)
PROBE_W_STD = {E4M3: 268.0, INT4: 4.3}                # standard deviation of a probe weight (sizes the shift below)


def probe_a_shift(fmt, k):
    """The power of two s for which integer activations times 2^-s give sums of a standard deviation near 3: with integer
    activations the sums are thousands, the bias is below the bf16 spacing and the GELU an identity or zero."""
    std_a = math.sqrt(((2 * PROBE_A_MAX[fmt] + 1) ** 2 - 1) / 12.0)
    return max(0, round(math.log2(math.sqrt(k) * std_a * PROBE_W_STD[fmt] / 3.0)))


def probe_headroom(fmt, k_pad, shift):
    """The integer probe's fp32 arithmetic is exact.  In units of the operands' common powers of two (2^-shift for A, 32 or
    1/4 for the weights) every product and every partial sum in any order is an integer of magnitude at most
    K max|a| max|w| < 2^24; the scale is 1 (e4m3) or inside the operand (int4); and acc + bias is a multiple of
    ``quantum`` = min(unit of the sum, 1) -- the bias is an integer -- with fewer than 2^24 of them."""
    a_max, (w_unit, w_max) = PROBE_A_MAX[fmt], PROBE_W_UNIT[fmt]
    assert k_pad * a_max * w_max < 2 ** 24, (fmt, k_pad)
    sum_unit = w_unit * 2.0 ** -shift
    quantum = min(sum_unit, 1.0)
    assert math.log2(quantum) == round(math.log2(quantum)) and 1.0 / quantum == round(1.0 / quantum)
    assert (k_pad * a_max * w_max * sum_unit + 3) / quantum < 2 ** 24, (fmt, k_pad, shift)


def probe_activations(fmt, m, k, shift, dev, g):
    probe_headroom(fmt, pad128(k), shift)
    hi = PROBE_A_MAX[fmt]
    return (torch.randint(-hi, hi + 1, (m, k), generator=g, device=dev).float() * 2.0 ** -shift).to(BF16)


def probe_bias(n_pad, n, dev):
    cols = torch.arange(n_pad, device=dev)
    bias = ((cols % 7) - 3).to(BF16)
    bias[n:] = 0                                           # padded channels: zero weights, zero bias
    return bias


def random_activations(m, k, dev, g):
    return torch.randn(m, k, generator=g, device=dev).to(BF16)


def random_bias(n_pad, n, dev, g):
    bias = torch.zeros(n_pad, dtype=BF16, device=dev)
    bias[:n] = (torch.randn(n, generator=g, device=dev) * 0.1).to(BF16)
    return bias


# ---------------------------------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
def wide_activations(a, k, k_pad):
    """``a`` [..., m, k] inside a NaN-filled buffer: the data at a 16-byte-aligned column offset, zeros only in
    [k, round_up(k, 64)), lda at least 64 above that.  Returns (buffer, lda, byte offset of the first element, the [..., m, k_pad]
    operand the references multiply with)."""
    k64 = pad64(k)
    lda = A_OFF + k64 + 72
    buf = torch.full((*a.shape[:-1], lda), float("nan"), dtype=BF16, device=a.device)
    buf[..., A_OFF : A_OFF + k] = a
    buf[..., A_OFF + k : A_OFF + k64] = 0
    seen = torch.zeros(*a.shape[:-1], k_pad, dtype=BF16, device=a.device)
    seen[..., :k] = a
    assert lda % 8 == 0 and lda >= k64 + 64
    return buf, lda, 2 * A_OFF, seen


C_TOP, C_LEFT, C_EXTRA = 2, 8, 24


def guarded_c(batch, m, width, dev):
    """``batch`` bf16 outputs of m x width, each with two guard rows above and below, 8 guard columns left and 16 right."""
    ldc = width + C_EXTRA
    buf = torch.full((batch, m + 2 * C_TOP, ldc), GUARD_BITS, dtype=torch.int16, device=dev)
    assert ldc % 4 == 0
    return buf, ldc


def c_pointer(buf, i):
    return buf.data_ptr() + 2 * ((i * buf.shape[1] + C_TOP) * buf.shape[2] + C_LEFT)


def c_result(name, buf, m, width):
    """The written region [batch, m, width] after checking that every guard element kept its bits and every result was stored."""
    inside = torch.zeros(buf.shape[1:], dtype=torch.bool, device=buf.device)
    inside[C_TOP : C_TOP + m, C_LEFT : C_LEFT + width] = True
    guard = buf == GUARD_BITS
    assert bool(guard[:, ~inside].all()), f"{name}: {int((~guard[:, ~inside]).sum())} guard elements around the result were written"
    assert not bool(guard[:, inside].any()), f"{name}: {int(guard[:, inside].sum())} elements left unwritten"
    return buf[:, C_TOP : C_TOP + m, C_LEFT : C_LEFT + width].contiguous().view(BF16)


def run_fp8w(lib, layer, a, m, bias, epi=BIAS, store_pad=1, gelu_from=0):
    """One md_gemm_fp8w launch per leading index of ``a`` [batch, m, k] (one synchronisation for all of them), guarded on every
    side.  Returns ([batch, m, n_store] bf16, the [batch, m, k_pad] operand the kernel was given)."""
    batch = a.shape[0]
    abuf, lda, a_off, seen = wide_activations(a, layer.k, layer.k_pad)
    width = layer.n_pad if store_pad else layer.n
    cbuf, ldc = guarded_c(batch, m, width, a.device)
    st = layer.struct(bias)
    for i in range(batch):
        a_ptr = abuf.data_ptr() + 2 * i * m * lda + a_off
        _lib.check(lib.md_gemm_fp8w(a_ptr, lda, C.byref(st), c_pointer(cbuf, i), ldc, m, epi, store_pad, gelu_from, stream()), "md_gemm_fp8w")
    torch.cuda.synchronize()
    return c_result(f"{FMT_NAME[layer.fmt]} m{m} k{layer.k} n{layer.n}", cbuf, m, width), seen


# ---------------------------------------------------------------------------------------------------------------------
# 1. one-hot probe
# ---------------------------------------------------------------------------------------------------------------------
ONE_HOT = [(k, n, store_pad) for n, store_pad in ((192, 0), (96, 1)) for k in (128, 256, 1152)]


@pytest.mark.parametrize("m", [64, 32, 8])
@pytest.mark.parametrize("k,n,store_pad", ONE_HOT)
@pytest.mark.parametrize("fmt", FORMATS, ids=case_id)
def test_one_hot_rows_return_every_stored_weight(lib, fmt, k, n, store_pad, m):
    layer = random_layer(fmt, k, n)
    launches = k // m
    a = torch.zeros(launches * m, k, dtype=BF16, device=DEV)
    a[torch.arange(k), torch.arange(k)] = 1.0              # row i of launch j is 1.0 at column j m + i: all K columns
    got, _ = run_fp8w(lib, layer, a.view(launches, m, k), m, None, store_pad=store_pad)
    got = got.reshape(k, -1)
    width = layer.n_pad if store_pad else n
    want = layer.weight[:width, :k].t().contiguous()
    differ = got.view(torch.int16) != want.view(torch.int16)
    print(f"one-hot {FMT_NAME[fmt]} k{k} n{n} m{m}: {launches} launches, {got.numel()} weights read back, {int(differ.sum())} differ")
    assert torch.equal(got, want), f"{int(differ.sum())} of {got.numel()} weights differ, first at (k, n) = {tuple(differ.nonzero()[0].tolist())}"
    if width > n:
        assert bool((got[:, n:].view(torch.int16) == 0).all()), "padding channels are not +0"
        assert not bool(layer.weight[n:].any())


# ---------------------------------------------------------------------------------------------------------------------
# 2. and 3.  the case list with integer and with random operands
# ---------------------------------------------------------------------------------------------------------------------
def check_row0(lib, name, layer, a, bias, got, **kw):
    sub, _ = run_fp8w(lib, layer, a[:, :1].contiguous(), 1, bias, **kw)
    assert torch.equal(sub.view(torch.int16), got[:, :1].view(torch.int16)), f"{name}: row 0 alone differs from row 0 of {a.shape[1]} rows"


@pytest.mark.parametrize("case,fmt", CASE_FORMATS, ids=case_id)
def test_integer_probe_is_exact(lib, case, fmt):
    m, k, n = case.m, case.k, case.n
    layer = probe_layer(fmt, k, n)
    bias = probe_bias(layer.n_pad, n, DEV)
    width = layer.n_pad if case.store_pad else n
    gf = case.gelu_from()
    for shift in (0, probe_a_shift(fmt, k)):
        a = probe_activations(fmt, m, k, shift, DEV, gen(DEV, 3, fmt, m, k, n)).unsqueeze(0)
        for epi in (BIAS, GELU):
            name = f"integer {FMT_NAME[fmt]} {case} shift {shift} epi {epi}"
            kw = dict(epi=epi, store_pad=case.store_pad, gelu_from=gf if epi == GELU else 0)
            got, seen = run_fp8w(lib, layer, a, m, bias, **kw)
            exact, mag = wstream_exact(seen[0], layer.q, layer.scale, bias)
            exact, mag, got0 = exact[:, :width], mag[:, :width], got[0]
            n_exact = width if epi == BIAS else gf
            want = exact.to(BF16)                          # float64 -> bf16 of a value with < 24 significant bits: one rounding
            assert torch.equal(want.double(), round_to_bf16(exact))
            differ = got0[:, :n_exact].view(torch.int16) != want[:, :n_exact].view(torch.int16)
            note = ""
            if epi == GELU:
                live = float((exact[:, gf:n].abs() < 4).double().mean())
                note = f"; GELU from column {gf}, {live:.3f} of its inputs with |x| < 4"
                assert shift == 0 or live >= 0.5
            print(f"{name}: {int(differ.sum())} of {differ.numel()} plain elements differ from bf16(exact), max |exact| {float(exact.abs().max()):.4g}{note}")
            assert not bool(differ.any()), f"{name}: {int(differ.sum())} elements differ from the rounded exact value"
            compare_f8_elementwise(name, got0, exact, mag, layer.k_pad, exact_acc=True, gelu_from=gf if epi == GELU else None)
            check_row0(lib, name, layer, a, bias, got, **kw)


@pytest.mark.parametrize("case,fmt", CASE_FORMATS, ids=case_id)
def test_random_operands_per_element(lib, case, fmt):
    m, k, n = case.m, case.k, case.n
    layer = random_layer(fmt, k, n)
    g = gen(DEV, 4, fmt, m, k, n)
    a = random_activations(m, k, DEV, g).unsqueeze(0)
    bias = random_bias(layer.n_pad, n, DEV, g)
    width = layer.n_pad if case.store_pad else n
    gf = case.gelu_from()
    for epi in (BIAS, GELU):
        name = f"random {FMT_NAME[fmt]} {case} epi {epi}"
        kw = dict(epi=epi, store_pad=case.store_pad, gelu_from=gf if epi == GELU else 0)
        got, seen = run_fp8w(lib, layer, a, m, bias, **kw)
        exact, mag = wstream_exact(seen[0], layer.q, layer.scale, bias)
        compare_f8_elementwise(name, got[0], exact[:, :width], mag[:, :width], layer.k_pad, accum_u=2.0 ** -23,
                               gelu_from=gf if epi == GELU else None)
        check_row0(lib, name, layer, a, bias, got, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 4. pair launches, per slice
# ---------------------------------------------------------------------------------------------------------------------
def partial_slices(n, k_pad):
    """The host rule of md_gemm_fp8w_partial_slices and of the pair launch: (slices, 128-steps per slice)."""
    tiles, steps = (n + 63) // 64, k_pad // STEP
    s = max(1, min(256 // max(1, tiles), 8, steps // 8))   # at least 8 steps (one prefetch window) per slice
    per = (steps + s - 1) // s
    slices = (steps + per - 1) // per
    return slices, (steps + slices - 1) // slices


def slice_ranges(k_pad, slices, per):
    steps = k_pad // STEP
    return [(s * per * STEP, min((s + 1) * per, steps) * STEP) for s in range(slices)]


@dataclass(frozen=True)
class Problem:
    k: int
    n: int
    slices: int    # what md_gemm_fp8w_partial_slices must answer
    per: int       # 128-steps per slice


# (K, n) pairs with the slice split stated: 256 = 2 steps -> 1 slice; 8192 = 64 steps -> 8 x 8; 1152 = 9 steps -> 1 slice of 9 (a
# slice holds at least 8 steps, so nine steps do not split); 2048 = 16 steps -> 2 x 8; 3200 = 25 steps -> 9 + 9 + 7;
# 2176 = 17 steps -> 9 + 8.  The last pair is there for slices of unequal length, which 1152 does not give.
PAIRS = [(Problem(256, 192, 1, 2), Problem(8192, 256, 8, 8)),
         (Problem(1152, 256, 1, 9), Problem(2048, 256, 2, 8)),
         (Problem(3200, 256, 3, 9), Problem(2176, 192, 2, 9))]


def pair_id(v):
    return f"k{v[0].k}n{v[0].n}+k{v[1].k}n{v[1].n}" if isinstance(v, tuple) else case_id(v)


def run_pair(lib, layers, acts, m):
    """One md_gemm_fp8w_partial_f32_pair launch.  Each problem's partials lie in a NaN-filled buffer of one slice more than the
    LARGER problem has, with a guard slice in front, one guard row above and two below every slice, 8 guard columns.  Returns
    per problem ([slices, m, n4] fp32 after the guard checks, the operand the kernel was given)."""
    n4 = [min(l.n_pad, (l.n + 3) // 4 * 4) for l in layers]
    counts = [partial_slices(l.n, l.k_pad)[0] for l in layers]
    ld = max(n4) + 8
    rows = m + 3
    bufs, ptrs, wides, seens = [], [], [], []
    for layer, a in zip(layers, acts):
        buf = torch.full((max(counts) + 2, rows, ld), float("nan"), dtype=torch.float32, device=a.device)
        bufs.append(buf)
        ptrs.append(buf.data_ptr() + 4 * (rows * ld + ld))   # slice 0 = buf[1], its row 0 = buf[1, 1]
        wide = wide_activations(a, layer.k, layer.k_pad)
        wides.append(wide)
        seens.append(wide[3])
    sts = [l.struct(None) for l in layers]
    _lib.check(lib.md_gemm_fp8w_partial_f32_pair(wides[0][0].data_ptr() + wides[0][2], wides[0][1], C.byref(sts[0]), ptrs[0],
                                                 wides[1][0].data_ptr() + wides[1][2], wides[1][1], C.byref(sts[1]), ptrs[1],
                                                 m, ld, rows * ld, stream()), "md_gemm_fp8w_partial_f32_pair")
    torch.cuda.synchronize()
    out = []
    for i, buf in enumerate(bufs):
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
        inside[1 : 1 + counts[i], 1 : 1 + m, : n4[i]] = True
        untouched = torch.isnan(buf)
        assert bool(untouched[~inside].all()), (f"problem {i}: {int((~untouched[~inside]).sum())} guard elements written (rows >= m, "
                                                f"columns >= {n4[i]} or slices >= {counts[i]})")
        out.append(buf[1 : 1 + counts[i], 1 : 1 + m, : n4[i]].contiguous())
    return out, seens


@pytest.mark.parametrize("m", [5, 33, 64])
@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
@pytest.mark.parametrize("kind", ["integer", "random"])
@pytest.mark.parametrize("fmt", FORMATS, ids=case_id)
def test_pair_partials_per_slice(lib, fmt, kind, pair, m):
    layers = [(probe_layer if kind == "integer" else random_layer)(fmt, p.k, p.n) for p in pair]
    acts = []
    for i, p in enumerate(pair):
        g = gen(DEV, 5 + i, fmt, m, p.k, p.n)
        acts.append(probe_activations(fmt, m, p.k, 0, DEV, g) if kind == "integer" else random_activations(m, p.k, DEV, g))
    for p, layer in zip(pair, layers):
        st = layer.struct(None)
        assert (p.slices, p.per) == partial_slices(p.n, layer.k_pad), "the stated split restates the host rule"
        assert int(lib.md_gemm_fp8w_partial_slices(C.byref(st))) == p.slices
    parts, seens = run_pair(lib, layers, acts, m)
    for i, (p, layer, part, seen) in enumerate(zip(pair, layers, parts, seens)):
        n4 = part.shape[2]
        scale = torch.ones(layer.n_pad, dtype=torch.float64, device=DEV) if layer.scale is None else layer.scale.double()
        w64 = (layer.q.double() * scale[:, None])[:n4]     # e4m3: the dequantised weight in float64; int4: the bf16 weight
        ranges = slice_ranges(layer.k_pad, p.slices, p.per)
        assert ranges[0][0] == 0 and ranges[-1][1] == layer.k_pad and all(lo < hi for lo, hi in ranges)
        for s, (lo, hi) in enumerate(ranges):
            name = f"pair {kind} {FMT_NAME[fmt]} m{m} problem {i} (k{p.k} n{p.n}) slice {s} of {p.slices}: K [{lo}, {hi})"
            if kind == "integer":
                exact = seen[:, lo:hi].double() @ w64[:, lo:hi].t()
                differ = part[s] != exact.float()
                print(f"{name}: {int(differ.sum())} of {differ.numel()} elements differ from the exact sum")
                assert torch.equal(part[s].double(), exact), f"{name}: {int(differ.sum())} elements differ from the exact sum"
            else:
                compare_elementwise(name, part[s], seen[:, lo:hi], w64[:, lo:hi], None, rounded=False)
    # row 0 alone: every slice of both problems reproduces its row 0
    parts1, _ = run_pair(lib, layers, [a[:1].contiguous() for a in acts], 1)
    for part, part1 in zip(parts, parts1):
        assert torch.equal(part1.view(torch.int32), part[:, :1].contiguous().view(torch.int32)), "row 0 alone differs"
