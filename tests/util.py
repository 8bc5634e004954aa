"""Shared helpers for the parity tests."""
import math

import numpy as np
import torch


def bits_to_bf16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).copy()).view(torch.bfloat16)


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """spacing of bf16 at |x| (8 significand bits)."""
    ax = x.float().abs().clamp_min(2.0 ** -120)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


def compare(name, got: torch.Tensor, ref: torch.Tensor, rel_rms: float, max_frac: float = None):
    """Tolerance check for bf16 activations of two implementations that share
    rounding points but not accumulation order: the RMS error relative to the
    RMS of the reference must stay below ``rel_rms``; ``max_frac`` optionally
    bounds the largest absolute error as a fraction of the largest |ref|."""
    g, r = got.detach().float().cpu(), ref.detach().float().cpu()
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    err = (g - r)
    rms = float(err.pow(2).mean().sqrt() / r.pow(2).mean().sqrt().clamp_min(1e-30))
    mx = float(err.abs().max() / r.abs().max().clamp_min(1e-30))
    msg = f"{name}: rel-rms {rms:.3e} (tol {rel_rms:.1e}), max-err/max-ref {mx:.3e}"
    print(msg)
    assert rms <= rel_rms, msg
    if max_frac is not None:
        assert mx <= max_frac, msg
    return rms, mx


def elementwise_excess(got: torch.Tensor, a: torch.Tensor, w: torch.Tensor, bias, *, rounded: bool) -> torch.Tensor:
    """``|got - exact| - bound`` per element (float64, on ``got``'s device) for ``got ~ a @ w^T + bias``; positive = violation.
    See compare_elementwise for the bound.  ``a`` [m, K] and ``w`` [n, K] are the bf16 operands, ``bias`` [n] or None."""
    dev = got.device
    a64, w64 = a.detach().to(dev).double(), w.detach().to(dev).double()
    b64 = torch.zeros(w.shape[0], dtype=torch.float64, device=dev) if bias is None else bias.detach().to(dev).double()
    assert a64.dim() == 2 and w64.dim() == 2 and a64.shape[1] == w64.shape[1]
    assert tuple(got.shape) == (a64.shape[0], w64.shape[0]), f"shape {tuple(got.shape)} vs {(a64.shape[0], w64.shape[0])}"
    k = a64.shape[1]
    exact = a64 @ w64.t() + b64
    mag = a64.abs() @ w64.abs().t() + b64.abs()
    g = got.detach().double()
    bound = (k + 1) * 2.0 ** -23 * mag
    if rounded:
        big = torch.maximum(g.abs(), exact.abs())
        _, e = torch.frexp(big)                       # big = f * 2^e, f in [0.5, 1): the bf16 spacing at big is 2^(e - 8)
        ulp = torch.ldexp(torch.ones_like(big), e.clamp_min(-125) - 8)
        bound = bound + 0.5 * torch.where(big > 0, ulp, torch.zeros_like(ulp))
    excess = (g - exact).abs() - bound
    return torch.where(torch.isfinite(g), excess, torch.full_like(excess, float("inf")))


def compare_elementwise(name, got: torch.Tensor, a: torch.Tensor, w: torch.Tensor, bias, *, rounded: bool):
    """Per-element bound for a GEMM with fp32 accumulation, derived and not measured.  With ``exact = a @ w^T + bias`` and
    ``mag = |a| @ |w|^T + |bias|`` evaluated in float64 from the bf16 operands, EVERY element must satisfy

        |got - exact| <= (0.5 * ulp_bf16(max(|got|, |exact|)) if rounded else 0) + (K + 1) * 2^-23 * mag

    Each of the K fp32 accumulate steps and the bias add is charged a relative error of 2^-23 of the running magnitude (which
    covers a truncating as well as a round-to-nearest accumulator) -- in any summation order and any split-K association; the
    single rounding to bf16 adds half a bf16 spacing at the larger of the two values, so a result that rounds across a binade
    is no false alarm.  ``rounded=False``: fp32 results (K-slice partial sums).  No element is excluded and there is no slack
    factor.  Returns ``|got - exact| - bound`` per element."""
    excess = elementwise_excess(got, a, w, bias, rounded=rounded)
    bad = excess > 0
    n_bad = int(bad.sum())
    flat = int(torch.argmax(excess))
    row, col = divmod(flat, excess.shape[1])
    msg = f"{name}: {n_bad} of {excess.numel()} elements exceed the per-element bound; worst ({row}, {col}) by {float(excess[row, col]):.3e}"
    print(msg if n_bad else f"{name}: all {excess.numel()} elements within the per-element bound (closest ({row}, {col}): {float(-excess[row, col]):.3e} to spare)")
    assert n_bad == 0, msg
    return excess


def _e4m3_values(t: torch.Tensor) -> torch.Tensor:
    """e4m3fn codes (uint8, or a float8 tensor) as float64 values."""
    if t.dtype == torch.uint8:
        t = t.view(torch.float8_e4m3fn)
    return t.float().double()


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as float64 for integer e in the normal range, assembled from its bits: a device's ldexp may go through pow and be
    an ulp off, which would move a tie."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def bf16_spacing(x: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 at |x| (float64 in, float64 out, an exact power of two; the subnormal spacing below 2^-126)."""
    _, e = torch.frexp(x)                                    # x = f * 2^e, f in [0.5, 1): the bf16 spacing at x is 2^(e - 8)
    return _pow2(e.clamp_min(-125) - 8)


def round_to_bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value, ties to even, as float64 (no detour through float32: no double rounding)."""
    s = bf16_spacing(x)
    return torch.round(x / s) * s                            # x / s is exact; torch.round rounds halves to even


def gemm_f8_exact(a8: torch.Tensor, a_scale: float, w8: torch.Tensor, wscale: torch.Tensor, bias, row_chunk: int = 8192):
    """md_gemm_f8 before its epilogue, in float64 from the e4m3 codes with NO intermediate rounding:
    ``exact = a_scale * wscale[n] * (A8 . W8^T) + bias`` and ``mag``, the same expression over absolute values.
    a8 [m, K] and w8 [n, K] are e4m3fn codes (uint8 or float8; a8 may be a strided view), wscale [n] fp32, bias [n] bf16 or
    None; a_scale is taken as the float the C ABI hands the kernel.  Evaluated on a8's device in chunks of rows."""
    dev = a8.device
    w64 = _e4m3_values(w8.to(dev))
    s64 = wscale.detach().to(dev).double() * float(np.float32(a_scale))
    b64 = torch.zeros(w64.shape[0], dtype=torch.float64, device=dev) if bias is None else bias.detach().to(dev).double()
    assert a8.dim() == 2 and w64.dim() == 2 and a8.shape[1] == w64.shape[1] and s64.shape == b64.shape == (w64.shape[0],)
    m, n = a8.shape[0], w64.shape[0]
    exact = torch.empty(m, n, dtype=torch.float64, device=dev)
    mag = torch.empty_like(exact)
    wt, wt_abs = w64.t().contiguous(), w64.abs().t().contiguous()
    for r0 in range(0, m, row_chunk):
        a64 = _e4m3_values(a8[r0 : r0 + row_chunk])
        exact[r0 : r0 + row_chunk] = (a64 @ wt) * s64 + b64
        mag[r0 : r0 + row_chunk] = (a64.abs() @ wt_abs) * s64.abs() + b64.abs()
    return exact, mag


# The charge per K accumulate step of compare_f8_elementwise: twice the largest error MEASURED for the fp8 matrix instruction
# (2.8696 * 2^-23 of mag per step; see the docstring and profiles/gemm_f8_exact_tests_gpu.txt), not the 2^-23 of an fp32 accumulator.
F8_MFMA_MEASURED_U = 2.8696 * 2.0 ** -23
F8_ACCUM_U = 2.0 * F8_MFMA_MEASURED_U
_GELU_A = -2.0 * math.log2(math.e) * math.sqrt(2.0 / math.pi)
_GELU_B = _GELU_A * 0.044715
_GELU_DIP = (-0.80, -0.70)   # brackets the minimiser of the tanh-GELU (x = -0.7525...)


def _gelu64(p: torch.Tensor):
    """tanh-GELU in float64 in the algebraically equal form x / (1 + 2^z), z = x (A + B x^2), that does not cancel for x << 0,
    and the error bound of gelu_tanh_f32x2 at p (see compare_f8_elementwise)."""
    z = p * (_GELU_A + _GELU_B * p * p)
    s = 1.0 / (1.0 + torch.exp2(z))
    y = p * s
    rel = ((1.0 - s) * (4.0 * math.log(2.0) * z.abs() + 1.0) + 2.0) * 2.0 ** -23
    return y, rel * y.abs() + p.abs() * 2.0 ** -120


def _gelu_floor() -> float:
    xs = torch.linspace(_GELU_DIP[0], _GELU_DIP[1], 100001, dtype=torch.float64)
    ys = _gelu64(xs)[0]
    i = int(torch.argmin(ys))
    assert 0 < i < xs.numel() - 1, "the bracket does not hold the minimiser"
    return float(ys[i]) - 1e-12   # a grid of step 1e-6 misses the minimum by <= 0.5 * max|gelu''| * (0.5e-6)^2 < 1e-12


_GELU_FLOOR = _gelu_floor()


def f8_output_interval(exact, mag, k, *, exact_acc=False, accum_u=F8_ACCUM_U, residual=None, gelu_from=None):
    """The closed interval [lo, hi] of bf16 values (as float64) md_gemm_f8 may store for every element; see
    compare_f8_elementwise.  ``residual`` [m, n]: the rows the kernel adds (already gathered); ``gelu_from``: first GELU column."""
    e32 = torch.zeros_like(mag) if exact_acc else (k * accum_u + 2 * 2.0 ** -23) * mag
    lo, hi = round_to_bf16(exact - e32), round_to_bf16(exact + e32)
    if residual is not None:
        r32 = residual.detach().to(exact.device).float()
        assert r32.shape == exact.shape
        lo, hi = ((r32 + p.float()).to(torch.bfloat16).double() for p in (lo, hi))
    if gelu_from is not None and gelu_from < exact.shape[1]:
        p_lo, p_hi = lo[:, gelu_from:], hi[:, gelu_from:]
        (y_lo, g_lo), (y_hi, g_hi) = _gelu64(p_lo), _gelu64(p_hi)
        ymin, ymax = torch.minimum(y_lo - g_lo, y_hi - g_hi), torch.maximum(y_lo + g_lo, y_hi + g_hi)
        dip = (p_lo < _GELU_DIP[1]) & (p_hi > _GELU_DIP[0])
        ymin = torch.where(dip, torch.clamp_max(ymin, _GELU_FLOOR - torch.maximum(g_lo, g_hi)), ymin)
        w = 2.0 ** -50                                       # this reference's own float64 evaluation (exp2, a division, products)
        lo, hi = lo.clone(), hi.clone()
        lo[:, gelu_from:] = round_to_bf16(ymin - w * ymin.abs())
        hi[:, gelu_from:] = round_to_bf16(ymax + w * ymax.abs())
    return lo, hi


def f8_code_interval(lo, hi, c8_inv_scale: float):
    """The e4m3 values (float64) of the two ends of a bf16 interval as the epilogue quantises them:
    e4m3(clamp(fp32(v * c8_inv_scale), +-448)), round to nearest even -- monotone in v."""
    s = torch.tensor(float(np.float32(c8_inv_scale)), dtype=torch.float32, device=lo.device)
    q = lambda v: (v.float() * s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float().double()
    return q(lo), q(hi)


def f8_excess(got, exact, mag, k, *, got8=None, f8_from=None, c8_inv_scale=1.0, **kw):
    """Distance of every element from its allowed interval (float64, > 0 = violation, non-finite = +inf): one tensor for the
    bf16 columns [0, f8_from) of ``got`` (None when there are none) and one for the e4m3 columns of ``got8`` (uint8 codes of
    columns f8_from .. n - 1; None without an fp8 output).  ``kw``: the arguments of f8_output_interval."""
    lo, hi = f8_output_interval(exact, mag, k, **kw)
    n = exact.shape[1]
    n_bf = n if got8 is None else int(f8_from)
    out = [None, None]
    if n_bf > 0:
        assert got is not None and tuple(got.shape) == (exact.shape[0], n_bf), f"bf16 part {tuple(got.shape)} vs {(exact.shape[0], n_bf)}"
        g = got.detach().double()
        ex = torch.maximum(lo[:, :n_bf] - g, g - hi[:, :n_bf])
        out[0] = torch.where(torch.isfinite(g), ex, torch.full_like(ex, float("inf")))
    if got8 is not None:
        assert tuple(got8.shape) == (exact.shape[0], n - n_bf), f"fp8 part {tuple(got8.shape)} vs {(exact.shape[0], n - n_bf)}"
        q_lo, q_hi = f8_code_interval(lo[:, n_bf:], hi[:, n_bf:], c8_inv_scale)
        g8 = _e4m3_values(got8.detach())
        ex8 = torch.maximum(q_lo - g8, g8 - q_hi)
        out[1] = torch.where(torch.isfinite(g8), ex8, torch.full_like(ex8, float("inf")))
    return out


def compare_f8_elementwise(name, got, exact, mag, k, *, got8=None, f8_from=None, c8_inv_scale=1.0, exact_acc=False,
                           accum_u=F8_ACCUM_U, residual=None, gelu_from=None):
    """Per-element bound for md_gemm_f8 (csrc/gemm_f8.hip), derived and not measured, with ``exact`` and ``mag`` of
    gemm_f8_exact and K = ``k`` (k_pad).  EVERY stored element must lie in an interval that follows the kernel's own
    operations; no element is excluded and there is no slack factor.  u = 2^-23.

    Pre-activation.  The kernel stores pre = bf16(fma(acc, sc, bias)), sc = fp32(wscale[n] * a_scale).  Its fp32 value x
    satisfies |x - exact| <= e32 = (K + 2) u mag in the fp32 model:
      * K u mag: the K accumulate steps of acc, each charged u of the running magnitude (<= mag), which covers a truncating as
        well as a round-to-nearest accumulator in any order.  The products need no term: e4m3 x e4m3 is 4 x 4 significand
        bits, exact in fp32.
        MEASURED, and this term alone widened: v_mfma_f32_32x32x64_f8f6f4 does not meet that model.  The exact probe of
        tests/test_gemm_f8_exact_gpu.py (integer operands, every fp32 step exact) passes bit for bit at every shape, yet with
        random operands K u mag was exceeded at K = 64 (13 of 96000 elements at 300 x 320 x 64, by up to one bf16 step),
        and only at K = 64, where no other term can hide it.  The instruction was therefore measured on its own at the
        smallest problem the kernel accepts -- one 256 x 256 tile, K = 64 (one instruction per output block), unit scales,
        no bias, 48 random operand draws -- against the float64 value: the largest (|got - exact| - half a bf16 spacing) /
        (K u mag) is 2.8696 (between 1.31 and 2.87 per draw; 2e-4 of the elements are above 1).  Sixty-four exact products summed
        with an error near 2^-15.5 of their magnitudes says the instruction aligns the products of a K block to a common
        exponent and drops the bits below a fixed width before it adds them.  The term is charged TWICE the measured value,
        so that another operand draw does not trip it: ``accum_u`` = F8_ACCUM_U = 2 * 2.8696 u = 5.74 u per step, i.e.
        e32 = (5.74 K + 2) u mag.  No figure comes from the kernel's output at a shape under test.
        What that costs: the K term grows with K while half a bf16 spacing does not.  At K = 4352 it is 5.74 K u mag = 3e-3
        mag, and mag is some 60 times a typical |value| of random operands: a fifth of the value.  With random operands the
        per-element check is therefore sharp at short K (at K = 64 it sees one bf16 step) and WEAK at long K, where it still
        finds a wrong scale or a lost slice only in the elements they move most (tests/test_util_cpu.py: "at least one
        element" at K = 4352).  Long K is guarded by the exact probe (``exact_acc``), which has no such term: do not rely
        on the random bound there.
      * u mag: the rounding of wscale[n] * a_scale to fp32, 2^-24.
      * u mag: the one rounding of the FMA with the bias, 2^-24 of a result of at most mag.
        The two roundings are charged u rather than 2^-24 each: the spare u pays for their products with the K-step term
        (K u * u apiece).  The count is K + 2, as compare_elementwise's is K + 1 for a GEMM without the scale.
    Rounding to nearest is monotone, so pre lies in [bf16(exact - e32), bf16(exact + e32)].  That is the bound
        |pre - exact| <= 0.5 ulp_bf16(max(|pre|, |exact|)) + (K accum_u + 2 u) mag
    in its sharpest form (every value of the interval satisfies it; the closest element is printed in this form).
    ``exact_acc``: e32 = 0 -- for operands whose products, partial sums and scaled FMA are exact in fp32 (small integers,
    power-of-two scales): pre must equal bf16(exact) bit for bit.

    Residual epilogue.  The kernel adds bf16(r) to the ROUNDED pre in fp32 and rounds once more: out = bf16(fp32(r + pre)),
    monotone in pre, evaluated with those rounding points at both ends of the interval.

    GELU epilogue (columns >= gelu_from), gelu_tanh_f32x2 on the rounded pre p (exact in fp32):
        y = p / (1 + 2^z),  z = p (A + B p^2),  A = -2 log2(e) sqrt(2 / pi),  B = 0.044715 A      (= 0.5 p (1 + tanh(..)))
      * z: the literals behind the fp32 constants are rounded (log2 e, sqrt(2 / pi), 0.044715: 3) and multiplied (-2 is a
        power of two: 2 products) -> B is off by at most 5 * 2^-24; the three polynomial operations p p (exact for a bf16 p,
        charged anyway: it pays for the second-order terms), the FMA and the product with p add 2^-24 each.  A and B p^2 have
        one sign, so nothing cancels: |dz| <= 8 * 2^-24 |z| = 4 u |z|.
      * v_exp_f32 is accurate to 1 ulp: 2^z (1 + e), |e| <= u, the same as an error of log2(1 + e) <= u / ln 2 in z.
      * s(z) = 1 / (1 + 2^z) has ds / dz = -ln 2 s (1 - s): a relative error of s of ln 2 (1 - s) |dz|
        <= (1 - s)(4 ln 2 |z| + 1) u.  It is bounded: (1 - s) |z| s has the maximum 0.224 / ln 2, so the ABSOLUTE error of
        y = p s from z never exceeds 1.2 u |p| however large |z| grows; the bound charges the sharper relative form.
      * 1 + 2^z (2^-24), v_rcp_f32 (1 ulp = u) and the product with p (2^-24): 2 u.
        |y_kernel - y| <= G(p) = ((1 - s)(4 ln 2 |z| + 1) + 2) u |y| + 2^-120 |p|,
      the last term for 2^z overflowing or flushing beyond 2^+-126, where y is below 2^-126 |p| or equals p.
    p may be any bf16 value of its interval [p_lo, p_hi]; y -+ G is monotone wherever y is (G is 1e-6 of |y|), so the image
    is spanned by the two ends, and by the global minimum of the tanh-GELU (-0.17 at x = -0.7525) where the interval reaches
    the bracket [-0.80, -0.70] around it.  The image, widened by 2^-50 for this reference's own float64 arithmetic, is
    rounded to bf16 at both ends: out lies in [bf16(ymin), bf16(ymax)].

    fp8 output (``got8``: the e4m3 codes of columns f8_from .. n - 1).  code = e4m3(clamp(fp32(v * c8_inv_scale), +-448))
    is monotone in the bf16 value v: every code must lie between the codes of the two ends of v's interval (compared as
    values, so +0 and -0 agree).  There is no cap on a share of differing codes: none may differ beyond that.

    Returns the excess tensors of f8_excess."""
    kw = dict(exact_acc=exact_acc, accum_u=accum_u, residual=residual, gelu_from=gelu_from)
    ex, ex8 = f8_excess(got, exact, mag, k, got8=got8, f8_from=f8_from, c8_inv_scale=c8_inv_scale, **kw)
    total = n_bad = 0
    notes = []
    for part, e in (("bf16", ex), ("e4m3", ex8)):
        if e is None:
            continue
        total += e.numel()
        bad = int((e > 0).sum())
        n_bad += bad
        if bad:
            row, col = divmod(int(torch.argmax(e)), e.shape[1])
            notes.append(f"{bad} {part} elements outside, worst ({row}, {col}) by {float(e[row, col]):.3e}")
        else:
            notes.append(f"{part}: {float((e == 0).double().mean()):.3f} of {e.numel()} on an end of their interval")
    if ex is not None and residual is None and not exact_acc:
        # the plain columns in the |pre - exact| form, for the record: how much the closest element has to spare
        n_plain = ex.shape[1] if gelu_from is None else min(ex.shape[1], gelu_from)
        if n_plain > 0:
            g, x, mg = got[:, :n_plain].detach().double(), exact[:, :n_plain], mag[:, :n_plain]
            half = 0.5 * bf16_spacing(torch.maximum(g.abs(), x.abs()))
            spare = half + (k * accum_u + 2 * 2.0 ** -23) * mg - (g - x).abs()
            row, col = divmod(int(torch.argmin(spare)), n_plain)
            notes.append(f"closest ({row}, {col}): {float(spare[row, col]):.3e} to spare")
    msg = f"{name}: {n_bad} of {total} elements exceed the per-element bound; " + "; ".join(notes)
    print(msg if n_bad else f"{name}: all {total} elements within the per-element bound; " + "; ".join(notes))
    assert n_bad == 0, msg
    return ex, ex8


def attention_exact(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, allowed, scale: float):
    """Softmax attention in float64 from the operands as the kernel sees them (bf16, or dequantised e4m3), with NO intermediate
    rounding.  q [..., rows, d], k / v [..., keys, d], ``allowed`` bool [..., rows, keys] (None: every key); every row must see
    at least one key.  Returns ``exact = P V`` and ``mag = P |V|`` ([..., rows, d], float64, on q's device)."""
    return _attention_terms(q, k, v, allowed, scale)[:2]


def _attention_terms(q, k, v, allowed, scale):
    """attention_exact plus what the bound needs per row: the number of visible keys and A = scale * max_j sum_i |q_i| |k_ji|."""
    dev = q.device
    q64, k64, v64 = q.detach().double(), k.detach().to(dev).double(), v.detach().to(dev).double()
    scale = float(np.float32(scale))                         # the C ABI hands the kernels a float
    s = (q64 @ k64.transpose(-1, -2)) * scale
    a = (q64.abs() @ k64.abs().transpose(-1, -2)) * abs(scale)
    if allowed is None:
        allowed = torch.ones(s.shape, dtype=torch.bool, device=dev)
    allowed = allowed.to(dev).expand(s.shape)
    n_vis = allowed.sum(-1, keepdim=True)
    assert int(n_vis.min()) > 0, "a row without a visible key has no softmax"
    s = s.masked_fill(~allowed, float("-inf"))
    p = torch.softmax(s, dim=-1)
    a_row = a.masked_fill(~allowed, 0.0).amax(-1, keepdim=True)
    return p @ v64, p @ v64.abs(), n_vis.double(), a_row


ATTN_TAIL_OPS = 8  # the constant c of compare_attention_elementwise


def attention_excess(got: torch.Tensor, q, k, v, allowed, scale) -> torch.Tensor:
    """``|got - exact| - bound`` per element (float64, on ``got``'s device); positive = violation, a non-finite ``got`` is +inf.
    See compare_attention_elementwise for the bound."""
    exact, mag, n_vis, a_row = _attention_terms(q.to(got.device), k, v, allowed, scale)
    assert tuple(got.shape) == tuple(exact.shape), f"shape {tuple(got.shape)} vs {tuple(exact.shape)}"
    hd = q.shape[-1]
    assert int(n_vis.max()) <= 64 * hd, "the rescale count of the bound is derived for at most 64 * head_dim visible keys"
    u = 2.0 ** -23
    spread = a_row > 0                                       # rows whose scores are not all exactly equal
    ds = torch.where(spread, (hd + 2) * u * a_row + u, torch.zeros_like(a_row))
    p_round = torch.where(spread, torch.full_like(a_row, 2.0 ** -8), torch.zeros_like(a_row))
    rel = p_round + 2 * ds + (n_vis + hd + ATTN_TAIL_OPS) * u
    g = got.detach().double()
    big = torch.maximum(g.abs(), exact.abs())
    _, e = torch.frexp(big)                                  # big = f * 2^e, f in [0.5, 1): the bf16 spacing at big is 2^(e - 8)
    ulp = torch.ldexp(torch.ones_like(big), e.clamp_min(-125) - 8)
    vmax = v.detach().to(got.device).double().abs().amax(dim=(-1, -2), keepdim=True)
    bound = 0.5 * torch.where(big > 0, ulp, torch.zeros_like(ulp)) + rel * mag + n_vis * 2.0 ** -126 * vmax
    excess = (g - exact).abs() - bound
    return torch.where(torch.isfinite(g), excess, torch.full_like(excess, float("inf")))


def compare_attention_elementwise(name, got: torch.Tensor, q, k, v, allowed, scale):
    """Per-element bound for softmax attention, derived and not measured.  With ``exact = P V`` and ``mag = P |V|`` of
    attention_exact (float64, from the operands the kernel reads), n the number of keys the row may see, d = head_dim,
    u = 2^-23 and A = scale * max_j sum_i |q_i| |k_ji| over the row's visible keys (so |s_j| <= A for its scores
    s_j = scale * q . k_j), EVERY element must satisfy

        |got - exact| <= 0.5 * ulp_bf16(max(|got|, |exact|)) + (2^-8 + 2 ds + (n + d + c) u) * mag + n * 2^-126 * max|V|
        ds = (d + 2) u A + u,      c = 8

    Where each term comes from (attn_prefill_dma_kernel, attn_decode_kernel, attn_decode_f8_kernel); every kernel computes
    o = bf16((sum_j P~_j v_j) / (sum_j p^_j)) with p^_j = exp2((s^_j - m) c2), c2 = fp32(scale * log2 e), m a reference
    common to the row, P~_j = bf16(p^_j):
      * 0.5 ulp_bf16: the single rounding of the output, at the larger of the two values so that a result which rounds across
        a binade is no false alarm.
      * 2^-8: P~_j = p^_j (1 + r_j), |r_j| <= 2^-8 for truncation (2^-9 for round-to-nearest): the probabilities enter the P V
        product as bf16 while the row sum l adds their fp32 values, so the factor does not cancel.  The products P~_j v_j
        (8 x 8 significand bits, or 8 x 4 for e4m3) are exact in fp32.
      * 2 ds: a score error |s^_j - s_j| <= ds turns p_j into p_j e^(+-ds); numerator and denominator of o each move by that
        factor, e^(2 ds) - 1 -> 2 ds of mag.  ds in units of u A:  d for the head_dim accumulates of q . k_j, charged u of the
        running magnitude each as compare_elementwise does (any order; covers a truncating MFMA accumulator; the decode
        kernels' rounding of q_i * c2 and their FMA chain of 8 + 3 or 16 + 2 steps are 2^-24 each and stay far below it);
        1 for the one rounding of (s^_j - m) c2 -- the FMA of the prefill kernel, the subtraction of the decode kernels -- 2^-24
        of |s_j - m| c2 <= 2 A c2;  1 for c2 itself: the reference uses float32(scale), as the kernel receives it, which
        leaves the rounding of the literal log2(e) (2^-26.2) and of the product (2^-24), 1.22 * 2^-24 of |s_j - m| <= 2 A --
        the 0.22 u A beyond the unit is covered by the matrix cores rounding to nearest (their d accumulates cost d / 2).
        The fp8 kernel folds k_scale into the same constant: one more 2^-24, inside the same margin (its chain is 18 deep).
        The final + u: v_exp_f32 is accurate to 1 ulp (CDNA ISA), a relative error of p^_j of at most 2^-23 = an exponent
        error of u.  Errors of the reference m itself are common to all keys of the row and cancel in o.
      * n u: each visible key enters two fp32 sums, P V and the row sum l, by one round-to-nearest accumulate each: 2^-24 of
        the running magnitude (<= the final one: the terms of l are positive, mag sums |.|) apiece, in any order and any
        partition into classes, tiles or lanes.  Masked keys add exact zeros.
      * d u: the online-softmax rescales of the prefill kernel: O and l are both multiplied by alpha (alpha itself is common
        and cancels), 2 * 2^-24 = u per rescale, at most one per 64-key tile over the row's own keys: n / 64 <= d (asserted:
        n <= 64 d; the longest context of this project is 2048).
      * c = 8: three more rescales in the tiles past the row's own keys that its 128-row block still walks (3); the last
        cross-lane add of l (1, prefill); the normalisation, v_rcp_f32 (1 ulp) and a multiply in the prefill kernel, a
        division of <= 2.5 ulp in the decode kernels (3); the v_scale multiply of the fp8 kernel (1).
      * n * 2^-126 * max|V|: a probability below the smallest normal fp32 / bf16 number is flushed to zero, an absolute
        error of at most 2^-126 per key against l >= 1 (the largest p^_j of a row is >= 1).
    A row whose scores are all exactly equal (A = 0: q = 0) has s^_j = m = 0 in any arithmetic and p^_j = exp2(0) = 1, exact
    in fp32 and bf16: its 2^-8 and ds terms are dropped, and the bound is one output rounding plus the fp32 sums.  That is
    what lets the uniform probe see ONE key dropped or added among 2048.
    No element is excluded and there is no slack factor.  Returns ``|got - exact| - bound`` per element."""
    excess = attention_excess(got, q, k, v, allowed, scale)
    bad = excess > 0
    n_bad = int(bad.sum())
    flat = int(torch.argmax(excess))
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(excess.shape)))
    worst = float(excess.flatten()[flat])
    msg = f"{name}: {n_bad} of {excess.numel()} elements exceed the per-element bound; worst {idx} by {worst:.3e}"
    print(msg if n_bad else f"{name}: all {excess.numel()} elements within the per-element bound (closest {idx}: {-worst:.3e} to spare)")
    assert n_bad == 0, msg
    return excess


def margin_aware_mismatches(got, ref, margins, thr=0.5):
    """Greedy ids of two correct bf16 implementations can only part ways at a decision whose
    reference top-1/top-2 logit margin is within bf16 noise.  For every sequence: the first
    position where ``got`` and ``ref`` differ must have reference margin <= thr (margins[i][j] is the
    margin of the decision that produced token j); after that the sequences are unrelated.
    Returns (number of exactly equal sequences, list of violations)."""
    exact, bad = 0, []
    for i, (g, r) in enumerate(zip(got, ref)):
        g, r = list(g), list(r)
        n = min(len(g), len(r))
        j = next((t for t in range(n) if g[t] != r[t]), None)
        if j is None:
            exact += 1
        elif float(margins[i][j]) > thr:
            bad.append((i, j, g[j], r[j], float(margins[i][j])))
    return exact, bad


def leading_wide_objects(margins: np.ndarray, thr: float) -> int:
    """detect/point goldens: number of leading objects all of whose decisions (and every decision
    before them) have a reference margin >= thr bf16 ulps."""
    n = 0
    for row in margins:
        if float(row.min()) < thr:
            break
        n += 1
    return n


def vit_fp64(x_bchw: torch.Tensor, sd, cfg) -> torch.Tensor:
    """The ViT encoder as a function of its bf16 weights and bf16 input, evaluated in float64 with
    NO intermediate rounding (reference structure: vision.py:44-74, layers.py:118-166) -- the
    "truth" both bf16 implementations approximate."""
    v = cfg.vision
    f = lambda k: sd[k].detach().cpu().double()
    x = x_bchw.detach().cpu().double()
    B, C, H, W = x.shape
    P = v.enc_patch_size
    x = x.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // P) * (W // P), C * P * P)
    x = x @ f("vision.patch_emb.weight").t() + f("vision.patch_emb.bias") + f("vision.pos_emb")
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (t.shape[-1],), f(p + ".weight"), f(p + ".bias"), 1e-5)
    hd = v.enc_dim // v.enc_n_heads
    for i in range(v.enc_n_layers):
        p = f"vision.blocks.{i}"
        h = ln(x, p + ".ln1")
        qkv = h @ f(p + ".attn.qkv.weight").t() + f(p + ".attn.qkv.bias")
        q, k, vv = [t.reshape(B, -1, v.enc_n_heads, hd).transpose(1, 2) for t in qkv.chunk(3, dim=-1)]
        a = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1) @ vv
        a = a.transpose(1, 2).reshape(B, -1, v.enc_dim)
        x = x + a @ f(p + ".attn.proj.weight").t() + f(p + ".attn.proj.bias")
        h = ln(x, p + ".ln2")
        h = torch.nn.functional.gelu(h @ f(p + ".mlp.fc1.weight").t() + f(p + ".mlp.fc1.bias"), approximate="tanh")
        x = x + h @ f(p + ".mlp.fc2.weight").t() + f(p + ".mlp.fc2.bias")
    return ln(x, "vision.post_ln")


def quantize_int4(w, group=128, zero_shift=0.0):
    """The checkpoint format dequantize_int4 / the int4 weight stream read (reference layers.py:38-74), from a float weight."""
    rows = w.float().cpu().reshape(-1, group)
    lo, hi = rows.min(1, keepdim=True).values, rows.max(1, keepdim=True).values
    scale = ((hi - lo) / 15).clamp_min(1e-8)
    zero = -lo / scale + zero_shift
    q = torch.clamp(torch.round(rows / scale + zero), 0, 15).to(torch.uint8)
    step = q.shape[0] // 2
    return (q[:step] << 4) | q[step:], scale, zero


def int4_codes(packed: torch.Tensor) -> torch.Tensor:
    """The nibbles of the checkpoint format as uint8 group rows [2 * packed.shape[0], 128]: high nibbles first (dequantize_int4)."""
    return torch.cat([(packed & 0xF0) >> 4, packed & 0x0F], 0)


def pack_int4(q: torch.Tensor, scale: torch.Tensor, zero: torch.Tensor, group=128):
    """The inverse of int4_codes with given quantisation parameters: ``q`` uint8 [n, k] nibbles, ``scale`` / ``zero`` [n, k / group]
    -> (packed, scale, zero) as quantize_int4 returns them, so that a test can choose every stored number itself."""
    rows = q.to(torch.uint8).cpu().reshape(-1, group)
    assert rows.shape[0] % 2 == 0 and tuple(scale.shape) == tuple(zero.shape) == (q.shape[0], q.shape[1] // group)
    step = rows.shape[0] // 2
    return (rows[:step] << 4) | rows[step:], scale.float().cpu().reshape(-1, 1), zero.float().cpu().reshape(-1, 1)


def dequantize_int4_single_rounding(packed, scale, zero, out_features: int) -> torch.Tensor:
    """NOT the checkpoint's weights: bf16((q - zero) * scale) with ONE rounding, the mistake a kernel makes that keeps q - zero
    in fp32.  The tests use it as a mutation, and to show that their operands tell it from dequantize_int4's two roundings."""
    w = ((int4_codes(packed).float() - zero.float()) * scale.float()).to(torch.bfloat16)
    return w.reshape(out_features, -1)


def wstream_exact(a: torch.Tensor, q: torch.Tensor, scale, bias, row_chunk: int = 8192):
    """md_gemm_fp8w before its epilogue, in float64 from the operands the kernel sees with NO intermediate rounding:
    ``exact = (A . q^T) * scale[n] + bias`` and ``mag``, the same expression over absolute values.  a [m, K] bf16 (may be a
    strided view); q [n, K]: for the e4m3 stream the code VALUES (PackedLinearFp8.q) with ``scale`` [n] the fp32 per-channel
    scale, for the int4 stream dequantize_int4's bf16 weight with ``scale`` None (= 1: the group scales are inside the
    operand); bias [n] bf16 or None.  Evaluated on a's device in chunks of rows."""
    dev = a.device
    q64 = q.detach().to(dev).float().double()
    n = q64.shape[0]
    s64 = torch.ones(n, dtype=torch.float64, device=dev) if scale is None else scale.detach().to(dev).double()
    b64 = torch.zeros(n, dtype=torch.float64, device=dev) if bias is None else bias.detach().to(dev).double()
    assert a.dim() == 2 and q64.dim() == 2 and a.shape[1] == q64.shape[1] and s64.shape == b64.shape == (n,)
    m = a.shape[0]
    exact = torch.empty(m, n, dtype=torch.float64, device=dev)
    mag = torch.empty_like(exact)
    qt, qt_abs = q64.t().contiguous(), q64.abs().t().contiguous()
    for r0 in range(0, m, row_chunk):
        a64 = a[r0 : r0 + row_chunk].detach().double()
        exact[r0 : r0 + row_chunk] = (a64 @ qt) * s64 + b64
        mag[r0 : r0 + row_chunk] = (a64.abs() @ qt_abs) * s64.abs() + b64.abs()
    return exact, mag


# ---- the single-sequence decode kernel (csrc/decode_b1.hip): layout, branch map and a float64 decoder block --------------------
B1_SLICES, B1_PART, B1_NWV, B1_MAX_KEYS = 8, 68, 8, 256   # key slices per head, floats per partial, waves per workgroup, keys per slice
B1_ERR_WORD = 64 * 11                                     # word of the sync state a timed-out barrier raises


def b1_layout(dim: int, ff_pad: int, n_heads: int) -> dict:
    """Byte offsets of the workspace as b1_fill lays it out: the two residual rows x[0], x[1], the fused [q | k | v | gelu(fc1)]
    row ``act`` and the attention partials ``part`` [n_heads][8][68] fp32, each rounded up to 256 bytes; ``total`` must equal
    md_decode_b1_workspace_bytes."""
    a256 = lambda v: (v + 255) // 256 * 256
    xb, ab, pb = a256(dim * 2), a256((3 * dim + ff_pad) * 2), a256(n_heads * B1_SLICES * B1_PART * 4)
    return {"x0": 0, "x1": xb, "act": 2 * xb, "part": 2 * xb + ab, "total": 2 * xb + ab + pb}


B1_BRANCHES = (
    "second (head, slice) item per workgroup", "phase C second pass", "combine second pass", "phase A second row pair per wave",
    "phase A idle waves", "phase D second row pair per wave", "phase D fewer row pairs than workgroups", "empty proj half",
    "two live proj halves, unequal", "two live fc2 halves, unequal", "fc2 half boundary not a multiple of 512 from the end",
    "empty key slice", "L = 8k", "L = 8k + 1", "slice fills sc[] (chunk == B1_MAX_KEYS)", "pos == ctx - 1",
    "key index clamp to ctx - 1 binds", "dim limit (4096)", "ff limit (8192)",
)


def b1_branches(n_cu: int, *, dim: int, n_heads: int, ff: int, L: int, ctx: int, vocab: int = 0) -> set:
    """Which of B1_BRANCHES one launch of decode_b1_kernel<8> takes on a device with ``n_cu`` workgroups, restating the kernel's
    own expressions (np_a, npw_a, np_c, npw_c, PPP, nchd, nch2, chunk, j0 / j1, load_kv's clamp, np_d, npw_d)."""
    nwv, nt, ppp = B1_NWV, 64 * B1_NWV, B1_NWV // 2
    npw = lambda n_pairs, b: (n_pairs - 1 - b) // n_cu + 1 if b < n_pairs else 0
    s = set()
    if n_heads * B1_SLICES > n_cu:
        s.add("second (head, slice) item per workgroup")
    np_c = dim // 2
    if npw(np_c, 0) > ppp:
        s.add("phase C second pass")
    if dim // 4 > nt:
        s.add("combine second pass")
    np_a = (3 * dim + ff) // 2
    if npw(np_a, 0) > nwv:
        s.add("phase A second row pair per wave")
    if npw(np_a, n_cu - 1) < nwv:
        s.add("phase A idle waves")
    if vocab:
        np_d = vocab // 2
        if npw(np_d, 0) > nwv:
            s.add("phase D second row pair per wave")
        if np_d < n_cu:
            s.add("phase D fewer row pairs than workgroups")
    halves = lambda k: (max(min(k, 512 * (((k + 511) // 512) // 2)), 0), k - max(min(k, 512 * (((k + 511) // 512) // 2)), 0))
    kp, kf = halves(dim), halves(ff)
    if kp[0] == 0:
        s.add("empty proj half")
    if kp[0] > 0 and kp[1] > 0 and kp[0] != kp[1]:
        s.add("two live proj halves, unequal")
    if kf[0] > 0 and kf[1] > 0 and kf[0] != kf[1]:
        s.add("two live fc2 halves, unequal")
    if kf[0] > 0 and kf[1] % 512 != 0:
        s.add("fc2 half boundary not a multiple of 512 from the end")
    chunk = (L + B1_SLICES - 1) // B1_SLICES
    if any(sl * chunk >= L for sl in range(B1_SLICES)):
        s.add("empty key slice")
    if L % 8 == 0:
        s.add("L = 8k")
    if L % 8 == 1 and L > 1:
        s.add("L = 8k + 1")
    if chunk == B1_MAX_KEYS:
        s.add("slice fills sc[] (chunk == B1_MAX_KEYS)")
    if L == ctx:
        s.add("pos == ctx - 1")
    # load_kv: j = min(min(j0 + g + NG i, j1 - 1), ctx - 1) with j1 = max(min(L, j0 + chunk), j0 + 1)
    if any(max(min(L, sl * chunk + chunk), sl * chunk + 1) - 1 > ctx - 1 for sl in range(B1_SLICES)):
        s.add("key index clamp to ctx - 1 binds")
    if dim == 4096:
        s.add("dim limit (4096)")
    if ff == 8192:
        s.add("ff limit (8192)")
    return s


def b1_barriers(n_layers: int, step: bool) -> int:
    """Grid barriers of one launch: two per block, one more behind every block that another block or phase D follows, and the
    one in front of phase D's final choice."""
    return 3 * n_layers + 1 if step else 3 * n_layers - 1


def rope64(v: torch.Tensor, cs: torch.Tensor, sn: torch.Tensor, rot: int) -> torch.Tensor:
    """The kernel's RoPE of head rows v [..., 64] at one position (float64): with re = v[j], im = v[rot / 2 + j], j < rot / 2,
    out[2 j] = re cs[j] - im sn[j] and out[2 j + 1] = re sn[j] + im cs[j] (the reference interleaves its output); columns
    >= rot pass.  At position 0 (cs = 1, sn = 0) this is the permutation alone."""
    hr = rot // 2
    re, im = v[..., :hr], v[..., hr:rot]
    out = v.clone()
    out[..., 0:rot:2] = re * cs - im * sn
    out[..., 1:rot:2] = re * sn + im * cs
    return out


B1_MUTATIONS = ("drop_key", "stale_key", "one_residual_rounding", "gelu_before_rounding", "neighbour_pair")


def b1_block_ref(x, w, kc, vc, pos: int, cs, sn, rot: int, *, rounded: bool, mutation=None, n_cu: int = 256, drop=(0, 0)):
    """One decoder block at one row in float64 (layers.py / text.py of the reference at batch 1, q_len 1).
    x [D]; w: dict of float64 tensors ln_w, ln_b [D], w1 [3 D + ff, D], b1, wp [D, D], bp, w2 [D, ff], b2 holding bf16 values;
    kc / vc [H, ctx, 64]: the slabs, rows < pos are the cache (row pos is read only by the "stale_key" mutation); cs / sn
    [rot / 2]: the fp32 table's row of position pos.
    ``rounded = False``: the truth, no intermediate rounding.  ``rounded = True``: round_to_bf16 at the rounding points both
    kernel families share -- the layer-norm output, each linear plus bias, GELU on the bf16 value and rounded again, the rotated
    q and k, the probabilities that enter P.V (the row sum adds them unrounded), the attention row, and the two sequential
    residual adds bf16(bf16(x + proj) + fc2).
    ``mutation``: one of B1_MUTATIONS, the mistakes the probes must see -- key ``drop`` = (head, index) left out; the key at
    pos read from the slab instead of the new rotated row; one rounding for both residual adds; GELU of the unrounded fc1;
    the weight rows of every output pair >= n_cu (the second pass of a workgroup) taken from the neighbouring pair.
    Returns hidden [D], k / v [H, 64] (the new slab rows), act [3 D + ff] (q | k | v | gelu(fc1) before RoPE), att [D], and the
    terms of the residual chain: x, proj = Wp att + bp, fc2 = W2 gelu + b2."""
    assert mutation is None or mutation in B1_MUTATIONS
    r = round_to_bf16 if rounded else (lambda t: t)
    d = x.numel()
    h = d // 64
    mean = x.mean()
    var = ((x - mean) ** 2).mean()
    ln = r((x - mean) / torch.sqrt(var + float(np.float32(1e-5))) * w["ln_w"] + w["ln_b"])
    pre = w["w1"] @ ln + w["b1"]
    g = r(_gelu64(pre[3 * d:] if mutation == "gelu_before_rounding" else r(pre[3 * d:]))[0])
    qkv = r(pre[: 3 * d])
    q, k, v = qkv.view(3, h, 64)
    qr, kr = r(rope64(q, cs, sn, rot)), r(rope64(k, cs, sn, rot))
    keys, vals = kc[:, : pos + 1].clone(), vc[:, : pos + 1].clone()
    if mutation != "stale_key":
        keys[:, pos] = kr
    vals[:, pos] = v
    s = torch.einsum("hd,hjd->hj", qr, keys) * 0.125
    if mutation == "drop_key":
        s[drop[0], drop[1]] = float("-inf")
    p = torch.exp(s - s.amax(-1, keepdim=True))
    att = r(torch.einsum("hj,hjd->hd", r(p), vals) / p.sum(-1, keepdim=True)).reshape(d)
    wp, w2 = w["wp"], w["w2"]
    if mutation == "neighbour_pair" and d // 2 > n_cu:
        pair = torch.arange(d // 2, device=x.device)
        src = torch.where(pair >= n_cu, torch.where(pair + 1 < d // 2, pair + 1, pair - 1), pair)
        rows = (2 * src[:, None] + torch.arange(2, device=x.device)).reshape(-1)
        wp, w2 = wp[rows], w2[rows]
    t1, t2 = r(wp @ att + w["bp"]), r(w2 @ g + w["b2"])
    hidden = r(x + t1 + t2) if mutation == "one_residual_rounding" else r(r(x + t1) + t2)
    return {"hidden": hidden, "k": kr, "v": v, "act": torch.cat([qkv, g]), "att": att, "x": x, "proj": t1, "fc2": t2}


def b1_logits_ref(hidden, post_w, post_b, lm_w, lm_b, *, rounded: bool, parts: bool = False):
    """The final layer norm and lm_head of the step entry in float64, with or without the two bf16 roundings.  ``parts``: also
    the dot products lm_w . ln without the bias."""
    r = round_to_bf16 if rounded else (lambda t: t)
    mean = hidden.mean()
    var = ((hidden - mean) ** 2).mean()
    ln = r((hidden - mean) / torch.sqrt(var + float(np.float32(1e-5))) * post_w + post_b)
    return (r(lm_w @ ln + lm_b), lm_w @ ln) if parts else r(lm_w @ ln + lm_b)


def gelu_interval(p: torch.Tensor):
    """[lo, hi] of bf16 values gelu_tanh_f32x2 may store for the bf16 pre-activation p (float64): the float64 GELU widened by the
    bound _gelu64 states, rounded at both ends.  (The probes keep p outside the dip bracket or accept its two ends.)"""
    y, g = _gelu64(p)
    return round_to_bf16(y - g - 2.0 ** -50 * y.abs()), round_to_bf16(y + g + 2.0 ** -50 * y.abs())


def err_in_spacings(got: torch.Tensor, truth: torch.Tensor, *terms):
    """(RMS, maximum) of |got - truth| per element, in units of the bf16 spacing at the largest of |truth| and |terms| (float64
    tensors of truth's shape: the addends the kernel rounds on the way to the result).  A result is as accurate as the roundings
    of its addends allow: where x + proj + fc2 cancels, one rounding of a term falling the other way under another summation
    order is many spacings of the small sum but one spacing of the term -- the unit that makes that count as one, and still
    counts an error of the terms in THEIR spacing instead of the spacing of a large x."""
    big = truth.abs()
    for t in terms:
        big = torch.maximum(big, t.reshape(truth.shape).abs())
    e = (got.double().reshape(truth.shape) - truth).abs() / bf16_spacing(big)
    assert torch.isfinite(e).all(), "non-finite error"
    return float(e.pow(2).mean().sqrt()), float(e.max())


def hidden_terms(ref: dict):
    """The addends of b1_block_ref's hidden, for err_in_spacings."""
    return ref["x"], ref["proj"], ref["fc2"]


# ---- inputs of tests/test_decode_b1_exact_gpu.py (built here so that the CPU tests of the instruments use the same numbers) ---
def b1_shapes(n_cu: int) -> dict:
    """The smallest shapes that reach each branch, from the CU count: S3 has more (head, slice) items than workgroups, more
    than 4 output pairs per workgroup in phase C and more than 512 four-feature groups; S4 sits on every static limit."""
    h3 = max(n_cu // 8 + 8, 4 * n_cu // 32 + 8, 2048 // 64 + 8)  # 40 at 256 CUs
    return {"S1": dict(dim=256, ff=704), "S2": dict(dim=640, ff=1096), "S3": dict(dim=64 * h3, ff=520), "S4": dict(dim=4096, ff=8192)}


KEY_COUNTS = (1, 2, 7, 8, 9, 16, 17, 2041, 2048)


def b1_case_list():
    """(shape, n_layers, L, ctx, vocab): every launch geometry tests/test_decode_b1_exact_gpu.py plans (vocab 0: the layers
    entry).  The GPU module records what it launches and asserts that it is exactly this list."""
    cases = [("S1", n, 1, 64, 0) for n in (1, 2, 3)] + [("S2", 1, 1, 64, 0), ("S2", 2, 1, 64, 0), ("S3", 1, 1, 64, 0), ("S3", 2, 1, 64, 0),
                                                        ("S4", 1, 1, 64, 0)]
    cases += [("S1", 1, L, 2048, 0) for L in KEY_COUNTS] + [("S1", 1, 40, 40, 0), ("S1", 1, 34, 34, 0), ("S1", 1, 41, 2048, 0)]
    cases += [("S2", 1, 17, 2048, 0), ("S3", 1, 7, 2048, 0), ("S3", 1, 9, 2048, 0), ("S3", 1, 2048, 2048, 0), ("S4", 1, 2048, 2048, 0)]
    cases += [("S1", 1, L, 64, v) for L in (1, 6) for v in (256, 4610)] + [("S1", 1, 778, 2048, 4616)]
    cases += [(s, 1, L, 2048, 0) for s in ("S1", "S2", "S3") for L in (1, 9, 778, 2048)] + [("S4", 1, 778, 2048, 0)]
    return sorted(set(cases))


def zero_weights(dim, ff, dev="cpu"):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    return {"ln_w": z(dim), "ln_b": z(dim), "w1": z(3 * dim + ff, dim), "b1": z(3 * dim + ff), "wp": z(dim, dim), "bp": z(dim),
            "w2": z(dim, ff), "b2": z(dim)}


def gen(seed, dev="cpu"):
    return torch.Generator(device=dev).manual_seed(seed)


def rint(g, lo, hi, *shape):
    """Integers of [lo, hi] as float64, drawn on the generator's device."""
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device).double()


def assert_fp32_exact(name, mat, vec, bias, unit):
    """Every term of mat @ vec + bias is a multiple of ``unit`` and the sum of their magnitudes stays below 2^24 units: every
    partial sum in any order is exact in fp32."""
    for t in (mat[:, :1] * vec[:1], bias):
        assert bool((torch.round(t / unit) * unit == t).all()), name
    mag = float((mat.abs() @ vec.abs() + bias.abs()).max())
    assert mag < 2.0 ** 24 * unit, f"{name}: magnitude {mag} needs more than 24 bits at unit {unit}"


SAFE_GELU = (0., 4., 5., 6., 7., 8.)  # pre-activations whose GELU rounds to themselves in bf16 under util.gelu_interval


def int_weights(dim, ff, seed, *, fc1_live=True, dev="cpu"):
    """One block whose every sum is exact in fp32 with ln.w = 0 (assert_exact_block): ln.b integers in [-4, 4]; q rows zero
    (uniform scores); k and fc1 rows integers in [-8, 8] / 64 with biases k / 128; v rows integers in [-2, 2] with integer
    biases, so that the attention row of one key is an integer vector; Wp integers in [-8, 8] / 64, W2 integers in [-32, 32] / 64
    against gelu values <= 8, their biases k / 128.  fc1_live = False: fc1 weights zero and fc1 biases in SAFE_GELU."""
    g = gen(seed, dev)
    w = zero_weights(dim, ff, dev)
    w["ln_b"] = rint(g, -4, 4, dim)
    w["w1"] = rint(g, -8, 8, 3 * dim + ff, dim) / 64
    w["b1"] = rint(g, -255, 255, 3 * dim + ff) / 128
    w["w1"][:dim] = 0  # q = 0: uniform scores
    w["b1"][:dim] = 0
    w["w1"][2 * dim: 3 * dim] = rint(g, -2, 2, dim, dim)
    w["b1"][2 * dim: 3 * dim] = rint(g, -64, 64, dim)
    if not fc1_live:
        w["w1"][3 * dim:] = 0
        w["b1"][3 * dim:] = torch.tensor(SAFE_GELU, dtype=torch.float64, device=dev)[rint(g, 0, 5, ff).long()]
    w["wp"] = rint(g, -8, 8, dim, dim) / 64
    w["bp"] = rint(g, -255, 255, dim) / 128
    w["w2"] = rint(g, -32, 32, dim, ff) / 64
    w["b2"] = rint(g, -255, 255, dim) / 128
    return w


def int_x(dim, seed, dev="cpu"):
    return rint(gen(seed, dev), -255, 255, dim) / 128


def assert_exact_block(name, w, att, gel):
    d = w["ln_w"].numel()
    assert_fp32_exact(f"{name}: fused rows", w["w1"], w["ln_b"], w["b1"], 2.0 ** -7)
    assert_fp32_exact(f"{name}: proj", w["wp"], att, w["bp"], 2.0 ** -7)
    assert_fp32_exact(f"{name}: fc2", w["w2"], gel, w["b2"], 2.0 ** -7)


def residual_chain(x, att, gel, w):
    """x' = bf16(bf16(x + bf16(Wp att + bp)) + bf16(W2 gelu + b2)) in float64 with its four roundings, and the two evaluations a
    wrong kernel could make: one rounding for both adds, and fc2 added first."""
    r = round_to_bf16
    t1, t2 = r(w["wp"] @ att + w["bp"]), r(w["w2"] @ gel + w["b2"])
    return r(r(x + t1) + t2), r(x + t1 + t2), r(r(x + t2) + t1)


def planted_v(H, n_keys):
    """V[h, j]: 2^((j // 64) % 16) in column (j + 7 h) % 64, else 0: within a slice (<= 256 consecutive keys) every key owns its
    (column, bit); a key missing, doubled or taken from another head changes the slice's sum, which stays below 2^17."""
    v = torch.zeros(H, n_keys, 64, dtype=torch.float64)
    j = torch.arange(n_keys)
    for h in range(H):
        v[h, j, (j + 7 * h) % 64] = torch.exp2(((j // 64) % 16).double())
    return v


def slice_probe_inputs(dim, ff, L, seed=31, dev="cpu"):
    """(weights, planted V [H, L, 64], cache K [H, L, 64]) of the uniform-score probe with L keys, the last one the new token's."""
    H, pos = dim // 64, L - 1
    g = gen(seed + L, dev)
    w = zero_weights(dim, ff, dev)
    vplant = planted_v(H, L).to(dev)
    w["b1"][dim: 2 * dim] = rint(g, -255, 255, dim) / 64
    w["b1"][2 * dim: 3 * dim] = vplant[:, pos].reshape(-1)
    w["wp"] = torch.eye(dim, dtype=torch.float64, device=dev)
    return w, vplant, rint(g, -255, 255, H, L, 64) / 64


B1_RMS_RATIO, B1_MAX_EXTRA = 1.5, 2.0    # the persistent kernel against the batched kernels: RMS ratio, spacings more at the maximum
TIER2_CASES = [("S1", (0, 8, 777, 2047)), ("S2", (0, 8, 777, 2047)), ("S3", (0, 8, 777, 2047)), ("S4", (777,))]
TIER2_CTX = 2048
TIER2_STEP = dict(vocab=4616, pos=777, token=1234)  # a second row pair in some waves; a multiple of 8 for the batched GEMM's stores


def random_weights(dim, ff, seed, dev="cpu"):
    """randn operands of one block (weights scaled by 1 / sqrt(K), biases by 0.1) as bf16 values in float64, drawn on the CPU:
    the same numbers with and without a GPU.  Returns (weights, the generator)."""
    g = gen(seed, "cpu")
    rn = lambda *s: torch.randn(*s, generator=g)
    q = lambda t: t.to(torch.bfloat16).to(dev).double()
    return {"ln_w": q(1 + 0.1 * rn(dim)), "ln_b": q(0.1 * rn(dim)), "w1": q(rn(3 * dim + ff, dim) / dim ** 0.5), "b1": q(0.1 * rn(3 * dim + ff)),
            "wp": q(rn(dim, dim) / dim ** 0.5), "bp": q(0.1 * rn(dim)), "w2": q(rn(dim, ff) / ff ** 0.5), "b2": q(0.1 * rn(dim))}, g


def tier2_inputs(dim, ff, dev="cpu"):
    """(weights, cache K, cache V [H, ctx, 64] bf16, x [D] bf16) of the random-operand cases: all randn."""
    w, g = random_weights(dim, ff, 81, dev)
    kc, vc = (torch.randn(dim // 64, TIER2_CTX, 64, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    return w, kc, vc, torch.randn(dim, generator=g).to(torch.bfloat16).to(dev)


def tier2_step_inputs(dim, ff, dev="cpu"):
    """(weights, head, cache K, cache V) of the random step: head = post_w, post_b, lm_w [V, D], lm_b, wte [V, D], all randn."""
    w, g = random_weights(dim, ff, 91, dev)
    rn = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev).double()
    v = TIER2_STEP["vocab"]
    head = dict(post_w=1 + 0.1 * rn(dim), post_b=0.1 * rn(dim), lm_w=rn(v, dim) / dim ** 0.5, lm_b=0.1 * rn(v), wte=rn(v, dim))
    head = {k: t.to(torch.bfloat16).double() for k, t in head.items()}
    return w, head, rn(dim // 64, TIER2_CTX, 64).to(torch.bfloat16), rn(dim // 64, TIER2_CTX, 64).to(torch.bfloat16)
