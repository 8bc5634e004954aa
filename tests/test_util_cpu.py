"""The per-element GEMM bound of util.compare_elementwise has teeth and raises no false alarm: on the CPU, an fp32 accumulator
walked in 64-wide K chunks (the kernels' slice width) in several orders and split-K associations passes with zero violations,
and every localised error of the kind a ragged tile makes -- a K slice lost in one row, the bias lost in one column, two
8-column store groups swapped, the rows of the second 64-row half shifted by one -- is rejected, with every violation inside the
mutated region.

The same for the per-element attention bound of util.compare_attention_elementwise, on the probe inputs of
tests/test_attention_exact_gpu.py: a float32 model of the kernels (64-key tiles, online softmax, bf16 probabilities) is inside
it, and the model with ONE key wrongly admitted or wrongly dropped is outside it in every row the probe aims at that key.

And for the fp8 tile GEMM's references, util.gemm_f8_exact and util.compare_f8_elementwise: a float32 model of gemm_f8_kernel's
arithmetic (64-wide K slices, the fp32 scale, the FMA with the bias, bf16 rounding, the GELU in its sigmoid form, the residual's
second rounding, e4m3 rounding) is inside the intervals, and one dropped K element, one column that reads its neighbour's
wscale and one bias taken from the next column are outside them, in the affected elements only.

And for the weight stream's instruments (tests/test_gemm_wstream_exact_gpu.py, util.wstream_exact): a float32 model of
gemm_fp8w_kernel (two K halves of every 128-step summed apart and added in a fixed order, the fp32 scale, the bias add) and a
chunked one with another association are inside the intervals; a product dropped in the last row, a channel that reads its
neighbour's scale, a 128-step that reads the next step's (scale, zero), a single-rounding dequantisation in one nibble position
and a step counted by two slices are each refused by the part that is meant to see them; the integer probe's headroom holds
for every case of the GPU list."""
import math

import numpy as np
import pytest
import torch

import test_gemm_wstream_exact_gpu as WS
from test_attention_exact_gpu import DEC_CTX, PROBES, prefill_geometry, visibility
from util import (attention_excess, compare_attention_elementwise, compare_elementwise, compare_f8_elementwise, dequantize_int4_single_rounding,
                  elementwise_excess, f8_excess, gemm_f8_exact, int4_codes, pack_int4, quantize_int4, round_to_bf16, wstream_exact)

BF16 = torch.bfloat16
SHAPES = [(128, 2048, 3584), (100, 8192, 2048), (65, 704, 256), (97, 1024, 1000)]
CHUNK = 64


def operands(m, k, n):
    g = torch.Generator(device="cpu").manual_seed(1000 + m + k + n)
    rnd = lambda *s: torch.randn(*s, generator=g)
    a = rnd(m, k).to(BF16)
    w = (rnd(n, k) / math.sqrt(k)).to(BF16)
    # the bound grows with sqrt(K) (about 0.06 per element at K = 8192): a bias of scale 0.1 can land below it there
    scale = 0.5 if k >= 8192 else 0.1
    b = rnd(n) * scale
    if abs(float(b[-1])) < scale:       # the column whose bias the mutation drops carries at least one sigma
        b[-1] = math.copysign(scale, float(b[-1]))
    return a, w, b.to(BF16)


def chunk_sum(a, w, chunks, skip_last_row_chunk=None):
    """fp32 accumulator over the given 64-wide K chunks, in the given order."""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    af, wf = a.float(), w.float()
    for c in chunks:
        p = af[:, c * CHUNK : (c + 1) * CHUNK] @ wf[:, c * CHUNK : (c + 1) * CHUNK].t()
        if c == skip_last_row_chunk:
            p[-1] = 0
        acc = acc + p
    return acc


def n_chunks(k):
    return (k + CHUNK - 1) // CHUNK


def slice_sums(a, w, slices):
    """split-K as the kernels do it: contiguous chunk ranges of ceil(nk / slices) chunks, partial sums added in slice order."""
    nk = n_chunks(a.shape[1])
    per = (nk + slices - 1) // slices
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for s in range(slices):
        acc = acc + chunk_sum(a, w, range(min(s * per, nk), min((s + 1) * per, nk)))
    return acc


def finish(acc, b):
    return (acc + b.float()).to(BF16)


@pytest.mark.parametrize("m,k,n", SHAPES)
def test_clean_fp32_accumulation_passes_in_every_order_and_association(m, k, n):
    a, w, b = operands(m, k, n)
    nk = n_chunks(k)
    runs = {"forward": chunk_sum(a, w, range(nk)), "reversed": chunk_sum(a, w, reversed(range(nk)))}
    for s in (2, 4, 8):
        runs[f"{s} slices"] = slice_sums(a, w, s)
    for name, acc in runs.items():
        ex = compare_elementwise(f"clean {m}x{k}x{n} {name}", finish(acc, b), a, w, b, rounded=True)
        assert int((ex > 0).sum()) == 0
        # the fp32 sums themselves, against the bound without the bf16 term (what the K-slice partials are held to)
        ex32 = compare_elementwise(f"clean fp32 {m}x{k}x{n} {name}", acc, a, w, None, rounded=False)
        assert int((ex32 > 0).sum()) == 0


def rejected(name, got, a, w, b, region):
    """compare_elementwise must refuse ``got``; returns the number of violations, all of which lie inside ``region`` (bool mask)."""
    with pytest.raises(AssertionError, match="exceed the per-element bound"):
        compare_elementwise(name, got, a, w, b, rounded=True)
    bad = elementwise_excess(got, a, w, b, rounded=True) > 0
    assert int(bad.sum()) > 0
    assert not bool((bad & ~region).any()), f"{name}: violations outside the mutated region"
    print(f"{name}: {int(bad.sum())} of {int(region.sum())} mutated elements violate")
    return int(bad.sum())


@pytest.mark.parametrize("m,k,n", SHAPES)
def test_last_k_slice_dropped_in_the_last_row_is_rejected(m, k, n):
    a, w, b = operands(m, k, n)
    nk = n_chunks(k)
    got = finish(chunk_sum(a, w, range(nk), skip_last_row_chunk=nk - 1), b)
    region = torch.zeros(m, n, dtype=torch.bool)
    region[-1] = True
    rejected(f"dropped K slice {m}x{k}x{n}", got, a, w, b, region)


@pytest.mark.parametrize("m,k,n", SHAPES)
def test_bias_dropped_in_the_last_column_is_rejected_in_every_row(m, k, n):
    a, w, b = operands(m, k, n)
    acc = chunk_sum(a, w, range(n_chunks(k)))
    b_mut = b.clone()
    b_mut[-1] = 0
    got = finish(acc, b_mut)
    region = torch.zeros(m, n, dtype=torch.bool)
    region[:, -1] = True
    assert rejected(f"dropped bias {m}x{k}x{n}", got, a, w, b, region) == m


@pytest.mark.parametrize("m,k,n", SHAPES)
def test_two_adjacent_8_column_groups_swapped_is_rejected(m, k, n):
    a, w, b = operands(m, k, n)
    clean = finish(chunk_sum(a, w, range(n_chunks(k))), b)
    got = clean.clone()
    got[:, n - 16 : n - 8], got[:, n - 8 :] = clean[:, n - 8 :], clean[:, n - 16 : n - 8]
    region = torch.zeros(m, n, dtype=torch.bool)
    region[:, n - 16 :] = True
    assert rejected(f"swapped column groups {m}x{k}x{n}", got, a, w, b, region) > region.sum() // 2


@pytest.mark.parametrize("m,k,n", [s for s in SHAPES if s[0] > 65])
def test_rows_of_the_second_half_rotated_by_one_is_rejected(m, k, n):
    a, w, b = operands(m, k, n)
    clean = finish(chunk_sum(a, w, range(n_chunks(k))), b)
    got = clean.clone()
    got[64:] = torch.roll(clean[64:], 1, dims=0)
    region = torch.zeros(m, n, dtype=torch.bool)
    region[64:] = True
    assert rejected(f"rotated rows {m}x{k}x{n}", got, a, w, b, region) > region.sum() // 2


def test_non_finite_and_fp32_partials():
    """A NaN is a violation (never 'not greater than the bound'), and rounded=False holds an fp32 sum to the accumulation term
    alone: the bf16 rounding of a clean result does not fit in it."""
    m, k, n = 65, 704, 256
    a, w, b = operands(m, k, n)
    acc = chunk_sum(a, w, range(n_chunks(k)))
    got = finish(acc, b).float()
    got[3, 5] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 16640 elements .* worst \(3, 5\)"):
        compare_elementwise("nan", got, a, w, b, rounded=True)
    with pytest.raises(AssertionError):
        compare_elementwise("bf16 result held to the fp32 bound", finish(acc, b), a, w, b, rounded=False)


# ---------------------------------------------------------------------------------------------------------------------
# attention: util.compare_attention_elementwise on the probes of test_attention_exact_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
def attention_model_f32(q, k, v, allowed, scale, tile=64):
    """The kernels' arithmetic in float32 for one sequence: q [H, rows, d], k / v [H, keys, d], allowed [rows, keys].  Keys in tiles
    of 64, raw scores, online softmax in the exp2 domain with the scale folded into one constant, probabilities rounded to bf16
    for P V while the row sum adds their fp32 values, one division and one bf16 rounding at the end."""
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    qf, kf, vf = q.float(), k.float(), v.float()
    h, rows, _ = qf.shape
    m = torch.full((h, rows), float("-inf"))
    l = torch.zeros(h, rows)
    o = torch.zeros(h, rows, vf.shape[-1])
    for k0 in range(0, kf.shape[1], tile):
        live = allowed[:, k0 : k0 + tile]
        if not bool(live.any()):
            continue
        s = (qf @ kf[:, k0 : k0 + tile].transpose(-1, -2)).masked_fill(~live, float("-inf"))
        m_new = torch.maximum(m, s.amax(-1))
        ref = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2((m - ref) * c))
        p = torch.exp2(s * c - (ref * c).unsqueeze(-1))
        l = l * alpha + p.sum(-1)
        o = o * alpha.unsqueeze(-1) + p.to(BF16).float() @ vf[:, k0 : k0 + tile]
        m = m_new
    return (o / l.unsqueeze(-1)).to(BF16)


# (prefix, q_len, ctx, pos0 per sequence, no mask, head_dim): causal over two query blocks, a prefix inside a wave, a continuation
# across the prefix end, no mask with head_dim 72, and decode rows at both ends of the length list
ATTN_GEOMETRY = [(0, 129, 256, (0, 3), False, 64), (70, 200, 256, (0, 3), False, 64), (730, 33, 768, (731, 728), False, 64),
                 (732, 729, 729, (0, 3), True, 72)]


def attention_cases():
    for prefix, q_len, ctx, pos0, no_mask, hd in ATTN_GEOMETRY:
        kv_lens, vis = prefill_geometry(prefix, q_len, ctx, pos0, no_mask)
        yield f"prefix{prefix} q{q_len} ctx{ctx} hd{hd}", vis, kv_lens, ctx, hd
    lens = [1, 2, 33, 256, 729, 2047, 2048]
    yield "decode rows", [visibility(n - 1, 1, n, 0, DEC_CTX) for n in lens], lens, DEC_CTX, 64


ATTN_CASES = list(attention_cases())


@pytest.mark.parametrize("probe", list(PROBES))
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: c[0])
def test_attention_bound_accepts_the_float32_kernel_model(case, probe):
    name, vis, kv_lens, ctx, hd = case
    scale = 1.0 / math.sqrt(hd)
    q, k, v, _ = PROBES[probe](vis, 4, 4, hd, ctx, kv_lens, scale, seed=7)
    for bi, (allowed, _) in enumerate(vis):
        got = attention_model_f32(q[bi], k[bi], v[bi], allowed, scale)
        ex = compare_attention_elementwise(f"model {name} {probe} seq {bi}", got, q[bi], k[bi], v[bi], allowed.unsqueeze(0), scale)
        assert int((ex > 0).sum()) == 0


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: c[0])
def test_one_key_mask_errors_are_rejected_in_every_row_the_spikes_aim_at(case):
    """Head 0's rows aim at their last visible key: the model that DROPS it is outside the bound in each of them.  Head 1's rows
    aim at their first hidden key: the model that ADMITS it is outside the bound in each of them."""
    name, vis, kv_lens, ctx, hd = case
    scale = 1.0 / math.sqrt(hd)
    q, k, v, targets = PROBES["spikes"](vis, 4, 4, hd, ctx, kv_lens, scale, seed=7)
    checked = {"dropped": 0, "admitted": 0}
    for bi, (allowed, _) in enumerate(vis):
        rows = torch.arange(allowed.shape[0])
        n_vis = allowed.sum(1)
        for what, head in (("dropped", 0), ("admitted", 1)):
            t = targets[bi, head]
            # the row owns a spike at exactly the key the mutation flips (a row with one visible key cannot lose it: no softmax left)
            owns = (t == n_vis - 1) & (n_vis > 1) if what == "dropped" else (t == n_vis) & (t >= 0)
            if not bool(owns.any()):
                continue
            mutated = allowed.clone()
            mutated[rows[owns], t[owns]] = what == "admitted"
            got = attention_model_f32(q[bi], k[bi], v[bi], mutated, scale)
            with pytest.raises(AssertionError, match="exceed the per-element bound"):
                compare_attention_elementwise(f"{what} {name} seq {bi}", got, q[bi], k[bi], v[bi], allowed.unsqueeze(0), scale)
            bad = (attention_excess(got, q[bi], k[bi], v[bi], allowed.unsqueeze(0), scale) > 0).any(-1)  # [H, rows]
            assert bool(bad[head][owns].all()), f"{what} {name} seq {bi}: rows {rows[owns][~bad[head][owns]].tolist()} of head {head} pass"
            assert not bool(bad[:, ~owns].any()), f"{what} {name} seq {bi}: violations outside the mutated rows"
            checked[what] += int(owns.sum())
    print(f"{name}: {checked}")
    assert checked["dropped"] > 0 and (checked["admitted"] > 0 or all(int(a.sum(1).min()) == ctx for a, _ in vis))


@pytest.mark.parametrize("n", [33, 729, 2048])
def test_uniform_probe_flags_one_dropped_key(n):
    """q = 0, integer V: one key lost anywhere among n moves most features by more than one bf16 rounding plus the fp32 sums."""
    vis = [visibility(n - 1, 1, n, 0, DEC_CTX)]
    q, k, v, _ = PROBES["uniform"](vis, 4, 4, 64, DEC_CTX, [n], 0.125, seed=11)
    allowed = vis[0][0]
    for lost in (0, n // 2, n - 1):
        mutated = allowed.clone()
        mutated[0, lost] = False
        got = attention_model_f32(q[0], k[0], v[0], mutated, 0.125)
        bad = attention_excess(got, q[0], k[0], v[0], allowed.unsqueeze(0), 0.125) > 0  # [H, 1, 64]
        print(f"n {n}, key {lost} lost: {bad.sum(-1).flatten().tolist()} of 64 features flagged per head")
        assert bool(bad.any(-1).all())
        assert int(bad.sum()) > bad.numel() // 2


# ---------------------------------------------------------------------------------------------------------------------
# md_gemm_f8: gemm_f8_exact / compare_f8_elementwise
# ---------------------------------------------------------------------------------------------------------------------
F8 = torch.float8_e4m3fn
F8_SHAPES = [(64, 64, 192), (130, 588, 320), (40, 4304, 192)]


def f8_operands(m, k, n, seed=0):
    """e4m3 operands drawn as the kernel tests draw them: per-tensor activation scale, per-channel weight scales, K zero padded."""
    g = torch.Generator(device="cpu").manual_seed(2000 + m + k + n + seed)
    k_pad = (k + 63) // 64 * 64
    x = torch.randn(m, k, generator=g).to(BF16).float()
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).to(BF16).float()
    bias = (torch.randn(n, generator=g) * 0.1).to(BF16)
    a_scale = float(x.abs().max()) / 448.0
    wscale = (w.abs().amax(dim=1) / 448.0).float()
    a8 = torch.zeros(m, k_pad, dtype=torch.uint8)
    w8 = torch.zeros(n, k_pad, dtype=torch.uint8)
    a8[:, :k] = (x / a_scale).clamp(-448, 448).to(F8).view(torch.uint8)
    w8[:, :k] = (w / wscale[:, None]).clamp(-448, 448).to(F8).view(torch.uint8)
    return a8, a_scale, w8, wscale, bias


def f8_model(a8, a_scale, w8, wscale, bias, *, drop=None, scale_from=None, bias_from=None):
    """bf16(fma(acc, sc, bias)) in float32 the way gemm_f8_kernel does it, one 64-wide K slice after the other.  Mutations:
    ``drop`` = (row, kk): that A element reads as zero; ``scale_from`` / ``bias_from`` = (col, src): column col takes
    wscale / bias of column src."""
    af, wf = a8.view(F8).float(), w8.view(F8).float()
    if drop is not None:
        af[drop[0], drop[1]] = 0.0
    acc = torch.zeros(af.shape[0], wf.shape[0], dtype=torch.float32)
    for c in range(af.shape[1] // CHUNK):
        acc = acc + af[:, c * CHUNK : (c + 1) * CHUNK] @ wf[:, c * CHUNK : (c + 1) * CHUNK].t()
    sc = wscale * torch.tensor(np.float32(a_scale))
    b = bias.float().clone()
    if scale_from is not None:
        sc[scale_from[0]] = sc[scale_from[1]]
    if bias_from is not None:
        b[bias_from[0]] = b[bias_from[1]]
    return (acc * sc + b).to(BF16)


def gelu_model(pre):
    """gelu_tanh_f32x2 in float32: constants folded in float32, x / (1 + 2^z)."""
    ka = np.float32(-2.0) * np.float32(1.4426950408889634) * np.float32(0.7978845608028654)
    kb = ka * np.float32(0.044715)
    x = pre.float()
    z = x * (float(kb) * (x * x) + float(ka))
    return (x * (1.0 / (1.0 + torch.exp2(z)))).to(BF16)


def quant_model(v, inv):
    return (v.float() * torch.tensor(np.float32(inv))).clamp(-448.0, 448.0).to(F8).view(torch.uint8)


def test_round_to_bf16_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(20000, generator=g) * torch.exp2(torch.randint(-20, 20, (20000,), generator=g).float())
    assert torch.equal(round_to_bf16(x.double()), x.to(BF16).double())
    ties = torch.tensor([1.00390625, 1.01171875, -2.0078125, 255.5, 0.0], dtype=torch.float64)
    assert round_to_bf16(ties).tolist() == [1.0, 1.015625, -2.0, 256.0, 0.0]


@pytest.mark.parametrize("m,k,n", F8_SHAPES)
def test_f8_bound_accepts_the_float32_kernel_model_in_every_epilogue(m, k, n):
    a8, a_scale, w8, wscale, bias = f8_operands(m, k, n)
    k_pad = a8.shape[1]
    exact, mag = gemm_f8_exact(a8, a_scale, w8, wscale, bias)
    assert exact.dtype == torch.float64 and bool((mag >= exact.abs()).all())
    pre = f8_model(a8, a_scale, w8, wscale, bias)
    compare_f8_elementwise(f"model bias {m}x{k}x{n}", pre, exact, mag, k_pad)
    # residual: the second rounding
    r = torch.randn(m, n, generator=torch.Generator().manual_seed(7)).to(BF16)
    compare_f8_elementwise(f"model residual {m}x{k}x{n}", (r.float() + pre.float()).to(BF16), exact, mag, k_pad, residual=r)
    # GELU from a 64-column boundary on, with an fp8 tail from the next one
    gf, ff = 64, 128
    out = pre.clone()
    out[:, gf:] = gelu_model(pre[:, gf:])
    inv = 448.0 / float(out[:, ff:].float().abs().max())
    compare_f8_elementwise(f"model gelu + e4m3 {m}x{k}x{n}", out[:, :ff], exact, mag, k_pad, gelu_from=gf,
                           got8=quant_model(out[:, ff:], inv), f8_from=ff, c8_inv_scale=inv)
    # all-fp8 output, no bias
    exact0, mag0 = gemm_f8_exact(a8, a_scale, w8, wscale, None)
    pre0 = f8_model(a8, a_scale, w8, wscale, torch.zeros_like(bias))
    inv0 = 448.0 / float(pre0.float().abs().max())
    compare_f8_elementwise(f"model all-e4m3 {m}x{k}x{n}", None, exact0, mag0, k_pad, got8=quant_model(pre0, inv0), f8_from=0, c8_inv_scale=inv0)


def f8_rejected(name, got, exact, mag, k_pad, region, least, **kw):
    """compare_f8_elementwise must refuse ``got``, with every violation inside ``region`` and at least ``least`` of them."""
    with pytest.raises(AssertionError, match="exceed the per-element bound"):
        compare_f8_elementwise(name, got, exact, mag, k_pad, **kw)
    bad = f8_excess(got, exact, mag, k_pad, **kw)[0] > 0
    assert not bool((bad & ~region).any()), f"{name}: violations outside the mutated region"
    print(f"{name}: {int(bad.sum())} of {int(region.sum())} mutated elements violate")
    assert int(bad.sum()) >= least, f"{name}: {int(bad.sum())} < {least}"


@pytest.mark.parametrize("m,k,n", F8_SHAPES)
def test_f8_bound_rejects_a_dropped_k_element_a_neighbours_scale_and_a_shifted_bias(m, k, n):
    """Each mutation changes one row or one column.  How many of its elements must leave the bound, at K <= 640: the
    neighbour's wscale moves the column's products by the ratio of two channel maxima (the columns are chosen at least 3 %
    apart, eight bf16 half-spacings) and the next column's bias moves it by at least 0.05 against values of order one, so at
    least 90 % of the column in both; a dropped element -- the row's largest activation code -- moves an output by |a w|,
    which is below the output's half-spacing where the weight code is small: at least a quarter of the row.  At K = 4352 the
    accumulate term alone, 5.74 K u mag = 3e-3 mag with mag some 60 times a typical |value|, is a fifth of the value: there
    each mutation must still be refused, by at least one element, and never outside its region."""
    a8, a_scale, w8, wscale, bias = f8_operands(m, k, n)
    k_pad = a8.shape[1]
    exact, mag = gemm_f8_exact(a8, a_scale, w8, wscale, bias)
    row = m - 1
    kk = int(a8.view(F8).float()[row].abs().argmax())
    region = torch.zeros(m, n, dtype=torch.bool)
    region[row] = True
    f8_rejected(f"dropped K element {m}x{k}x{n}", f8_model(a8, a_scale, w8, wscale, bias, drop=(row, kk)), exact, mag, k_pad, region,
                n // 4 if k <= 640 else 1)
    ratio = (wscale[1:] / wscale[:-1] - 1).abs()
    col = int(ratio.argmax())
    assert float(ratio[col]) >= 0.03
    region = torch.zeros(m, n, dtype=torch.bool)
    region[:, col] = True
    f8_rejected(f"neighbour's wscale {m}x{k}x{n}", f8_model(a8, a_scale, w8, wscale, bias, scale_from=(col, col + 1)), exact, mag, k_pad,
                region, int(0.9 * m) if k <= 640 else 1)
    step = (bias.float()[1:] - bias.float()[:-1]).abs()
    col = int(step.argmax())
    assert float(step[col]) >= 0.05
    region = torch.zeros(m, n, dtype=torch.bool)
    region[:, col] = True
    f8_rejected(f"bias of the next column {m}x{k}x{n}", f8_model(a8, a_scale, w8, wscale, bias, bias_from=(col, col + 1)), exact, mag,
                k_pad, region, int(0.9 * m) if k <= 640 else 1)


def test_f8_exact_probe_form_and_code_interval_have_no_tolerance():
    """exact_acc: one bf16 step off is refused; the e4m3 interval refuses a code one step outside and a NaN code."""
    a8, a_scale, w8, wscale, bias = f8_operands(64, 64, 128)
    exact, mag = gemm_f8_exact(a8, a_scale, w8, wscale, bias)
    pre = round_to_bf16(exact).to(BF16)
    compare_f8_elementwise("rounded exact", pre, exact, mag, 64, exact_acc=True)
    off = pre.clone()
    off.view(torch.int16)[3, 5] += 1
    with pytest.raises(AssertionError, match="1 of"):
        compare_f8_elementwise("one bf16 step", off, exact, mag, 64, exact_acc=True)
    codes = quant_model(pre, 8.0)
    compare_f8_elementwise("codes", None, exact, mag, 64, exact_acc=True, got8=codes, f8_from=0, c8_inv_scale=8.0)
    for value in (int(codes[2, 9]) ^ 1, 0x7F):
        wrong = codes.clone()
        wrong[2, 9] = value
        with pytest.raises(AssertionError, match="1 of"):
            compare_f8_elementwise("one code", None, exact, mag, 64, exact_acc=True, got8=wrong, f8_from=0, c8_inv_scale=8.0)


def test_exact_probe_arithmetic_is_exact_in_fp32_for_every_shape_of_the_gpu_list():
    """The headroom argument of tests/test_gemm_f8_exact_gpu.py, and on its smallest K the claim itself: the float32 model
    equals the rounded float64 value bit for bit in any slice order."""
    import test_gemm_f8_exact_gpu as T

    for case in T.EXACT_CASES:
        k_pad = T.pad64(case.k)
        T.probe_headroom(k_pad, T.probe_a_scale(k_pad))
    assert {T.pad64(c.k) for c in T.EXACT_CASES} >= {64, 128, 192, 256, 320, 640, 4352}
    old, T.DEV = T.DEV, "cpu"
    try:
        for k in (64, 588, 4304):
            a8, a_scale, w8, wscale, bias = T.probe_operands(70, 130, k, True)
            exact, mag = gemm_f8_exact(a8, a_scale, w8, wscale, bias)
            got = f8_model(a8, a_scale, w8, wscale, bias)
            assert torch.equal(got, exact.to(BF16)) and torch.equal(got.double(), round_to_bf16(exact))
            compare_f8_elementwise(f"probe model k={k}", got, exact, mag, T.pad64(k), exact_acc=True)
    finally:
        T.DEV = old


# ---------------------------------------------------------------------------------------------------------------------
# md_gemm_fp8w: wstream_exact and the probes of tests/test_gemm_wstream_exact_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
WS_SHAPE = (64, 2048, 256)   # the shape at which the rel-rms tolerances let these mutations pass
U23 = 2.0 ** -23


def ws_operands(fmt, m=WS_SHAPE[0], k=WS_SHAPE[1], n=WS_SHAPE[2]):
    layer = WS.random_layer(fmt, k, n, "cpu")
    g = WS.gen("cpu", 4, fmt, m, k, n)
    a = WS.random_activations(m, k, "cpu", g)
    a[-1, -1] = math.copysign(max(1.0, abs(float(a[-1, -1]))), float(a[-1, -1]))   # the product the mutation drops carries a sigma
    bias = WS.random_bias(layer.n_pad, n, "cpu", g)
    seen = torch.zeros(m, layer.k_pad, dtype=BF16)
    seen[:, :k] = a
    return layer, seen, bias


def ws_acc(a, q, order="kernel"):
    """The fp32 accumulator of fp8w_body.  "kernel": the two 64-wide halves of every 128-step summed apart, step after step, then
    first half + second half.  "chunked": 64-wide chunks from the last to the first into ONE accumulator."""
    af, qf = a.float(), q.float()
    k = af.shape[1]
    part = lambda c: af[:, c * 64 : (c + 1) * 64] @ qf[:, c * 64 : (c + 1) * 64].t()
    if order == "chunked":
        acc = torch.zeros(af.shape[0], qf.shape[0])
        for c in reversed(range(k // 64)):
            acc = acc + part(c)
        return acc
    halves = [torch.zeros(af.shape[0], qf.shape[0]) for _ in range(2)]
    for s in range(k // 128):
        for h in range(2):
            halves[h] = halves[h] + part(2 * s + h)
    return halves[0] + halves[1]


def ws_model(a, q, scale, bias, order="kernel"):
    sc = torch.ones(q.shape[0]) if scale is None else scale.float()
    return (ws_acc(a, q, order) * sc + bias.float()).to(BF16)


def ws_rejected(name, got, exact, mag, k_pad, region, least, **kw):
    f8_rejected(name, got, exact, mag, k_pad, region, least, accum_u=U23, **kw)


@pytest.mark.parametrize("fmt", WS.FORMATS, ids=WS.case_id)
def test_wstream_bound_accepts_the_float32_kernel_model(fmt):
    for m, k, n in [WS_SHAPE, (40, 704, 256) if fmt == WS.E4M3 else (40, 640, 256), (3, 8192, 128)]:
        layer, a, bias = ws_operands(fmt, m, k, n)
        exact, mag = wstream_exact(a, layer.q, layer.scale, bias)
        assert exact.dtype == torch.float64 and bool((mag >= exact.abs()).all())
        for order in ("kernel", "chunked"):
            pre = ws_model(a, layer.q, layer.scale, bias, order)
            compare_f8_elementwise(f"wstream model {WS.FMT_NAME[fmt]} {m}x{k}x{n} {order}", pre, exact, mag, layer.k_pad, accum_u=U23)
            gf = 8 * (n // 16) + 8
            out = pre.clone()
            out[:, gf:] = gelu_model(pre[:, gf:])
            compare_f8_elementwise(f"wstream model gelu {WS.FMT_NAME[fmt]} {m}x{k}x{n} {order}", out, exact, mag, layer.k_pad, accum_u=U23, gelu_from=gf)


@pytest.mark.parametrize("fmt", WS.FORMATS, ids=WS.case_id)
def test_wstream_bound_rejects_the_last_product_dropped_in_the_last_row(fmt):
    """|a w| of one product against half a bf16 spacing plus K u mag: at K = 2048 about half of the row's elements leave the
    interval (the relative RMS over the whole output moves by 1.75e-3, inside the old 3e-3); at least a quarter is asserted."""
    layer, a, bias = ws_operands(fmt)
    m, n = a.shape[0], layer.n_pad
    exact, mag = wstream_exact(a, layer.q, layer.scale, bias)
    mut = a.clone()
    mut[-1, WS_SHAPE[1] - 1] = 0
    region = torch.zeros(m, n, dtype=torch.bool)
    region[-1] = True
    ws_rejected(f"dropped last product {WS.FMT_NAME[fmt]}", ws_model(mut, layer.q, layer.scale, bias), exact, mag, layer.k_pad, region, n // 4)


def test_wstream_bound_and_one_hot_reject_a_neighbouring_channels_scale():
    layer, a, bias = ws_operands(WS.E4M3)
    m, n = a.shape[0], layer.n_pad
    exact, mag = wstream_exact(a, layer.q, layer.scale, bias)
    ratio = (layer.scale[1:] / layer.scale[:-1] - 1).abs()
    col = int(ratio.argmax())
    assert float(ratio[col]) >= 0.03
    sc = layer.scale.clone()
    sc[col] = layer.scale[col + 1]
    region = torch.zeros(m, n, dtype=torch.bool)
    region[:, col] = True
    ws_rejected("neighbour's scale", ws_model(a, layer.q, sc, bias), exact, mag, layer.k_pad, region, m // 2)
    # the one-hot probe compares bf16(q * scale): most of the channel's weights differ
    wrong = (layer.q[col] * sc[col]).to(BF16)
    assert float((wrong != layer.weight[col]).double().mean()) > 0.5


def int4_triple(k, n):
    w = torch.randn(n, k, generator=WS.gen("cpu", 1, WS.INT4, k, n)) / math.sqrt(k)
    return quantize_int4(w, zero_shift=0.3)


def test_wstream_bound_and_one_hot_reject_the_next_steps_qparams():
    """One channel, one 128-step dequantised with the (scale, zero) of the step after it."""
    m, k, n = WS_SHAPE
    layer, a, bias = ws_operands(WS.INT4)
    packed, scale, zero = int4_triple(k, n)
    assert torch.equal(WS.dequantize_int4(packed, scale, zero, n), layer.weight[:n])
    steps = k // 128
    dz = (zero.reshape(n, steps)[:, 1:] - zero.reshape(n, steps)[:, :-1]).abs()
    col, step = divmod(int(dz.argmax()), steps - 1)
    s_mut, z_mut = scale.clone(), zero.clone()
    s_mut[col * steps + step], z_mut[col * steps + step] = scale[col * steps + step + 1], zero[col * steps + step + 1]
    w_mut = WS.dequantize_int4(packed, s_mut, z_mut, n)
    differ = w_mut != layer.weight[:n]
    assert bool(differ.any()) and not bool(differ[:, : step * 128].any()) and not bool(differ[:, (step + 1) * 128 :].any())
    assert int(differ.any(1).sum()) == 1 and bool(differ[col].any()), "the one-hot probe sees it, in that channel and step only"
    exact, mag = wstream_exact(a, layer.q, None, bias)
    region = torch.zeros(m, layer.n_pad, dtype=torch.bool)
    region[:, col] = True
    q_mut = layer.q.clone()
    q_mut[:n] = w_mut
    ws_rejected("next step's qparams", ws_model(a, q_mut, None, bias), exact, mag, layer.k_pad, region, m // 2)


def test_one_hot_probe_sees_a_single_rounding_in_one_nibble_position():
    m, k, n = WS_SHAPE
    packed, scale, zero = int4_triple(k, n)
    double, single = WS.dequantize_int4(packed, scale, zero, n), dequantize_int4_single_rounding(packed, scale, zero, n)
    assert float((double != single).double().mean()) >= 0.10
    for j in range(8):
        mut = double.clone()
        mut[:, j::8] = single[:, j::8]
        differ = mut != double
        print(f"single rounding in nibble {j}: {int(differ.sum())} of {differ.numel()} weights differ")
        assert int(differ.sum()) >= 1 and not torch.equal(mut, double)
        assert float(differ[:, j::8].double().mean()) >= 0.10 and int(differ.sum()) == int(differ[:, j::8].sum())


def test_int4_helpers_round_trip():
    q = torch.randint(0, 16, (6, 256), generator=torch.Generator().manual_seed(3)).to(torch.uint8)
    scale, zero = torch.rand(6, 2) + 0.5, torch.rand(6, 2) * 15
    packed, s, z = pack_int4(q, scale, zero)
    assert torch.equal(int4_codes(packed).reshape(6, 256), q) and tuple(s.shape) == tuple(z.shape) == (12, 1)
    want = ((q.float() - zero.repeat_interleave(128, 1)).to(BF16).float() * scale.repeat_interleave(128, 1)).to(BF16)
    assert torch.equal(WS.dequantize_int4(packed, s, z, 6), want)


@pytest.mark.parametrize("fmt", WS.FORMATS, ids=WS.case_id)
def test_per_slice_check_rejects_a_step_counted_in_two_slices(fmt):
    """The fp32 partials of the pair launch, slice by slice: the clean model passes; slice 0 running one 128-step into slice 1
    is refused with random operands and differs from the exact sum with the integer ones."""
    m, (k, n) = 33, (2048, 256)
    slices, per = WS.partial_slices(n, k)
    assert (slices, per) == (2, 8)
    (lo, hi), _ = WS.slice_ranges(k, slices, per)
    for kind in ("random", "integer"):
        layer = (WS.random_layer if kind == "random" else WS.probe_layer)(fmt, k, n, "cpu")
        g = WS.gen("cpu", 6, fmt, m, k, n)
        a = WS.random_activations(m, k, "cpu", g) if kind == "random" else WS.probe_activations(fmt, m, k, 0, "cpu", g)
        sc = torch.ones(n) if layer.scale is None else layer.scale
        w64 = layer.q.double() * sc.double()[:, None]
        clean = ws_acc(a[:, lo:hi], layer.q[:, lo:hi]) * sc
        twice = ws_acc(a[:, lo : hi + 128], layer.q[:, lo : hi + 128]) * sc
        if kind == "random":
            compare_elementwise(f"slice model {WS.FMT_NAME[fmt]}", clean, a[:, lo:hi], w64[:, lo:hi], None, rounded=False)
            with pytest.raises(AssertionError, match="exceed the per-element bound"):
                compare_elementwise(f"step in two slices {WS.FMT_NAME[fmt]}", twice, a[:, lo:hi], w64[:, lo:hi], None, rounded=False)
            bad = elementwise_excess(twice, a[:, lo:hi], w64[:, lo:hi], None, rounded=False) > 0
            assert float(bad.double().mean()) > 0.9
        else:
            exact = a[:, lo:hi].double() @ w64[:, lo:hi].t()
            assert torch.equal(clean.double(), exact) and not torch.equal(twice.double(), exact)


def test_wstream_integer_probe_is_exact_in_fp32_for_every_case_of_the_gpu_list():
    """probe_headroom for every launch of the GPU file, the stated slice splits against the host rule and the library, and on
    small shapes the claim itself: the float32 model equals the rounded float64 value bit for bit in both associations."""
    import ctypes as C

    from moondream_amd import _lib

    for case, fmt in WS.CASE_FORMATS:
        for shift in (0, WS.probe_a_shift(fmt, case.k)):
            WS.probe_headroom(fmt, WS.pad128(case.k), shift)
        assert case.gelu_from() % 8 == 0 and 0 < case.gelu_from() < case.n and case.gelu_from() % 32 != 0
    lib = _lib.load()
    for pair in WS.PAIRS:
        for p in pair:
            for fmt in WS.FORMATS:
                WS.probe_headroom(fmt, p.k, 0)
            assert WS.partial_slices(p.n, p.k) == (p.slices, p.per)
            st = _lib.MdLinearFp8(None, None, None, p.n, p.k, WS.pad64(p.n), p.k, WS.E4M3)
            assert int(lib.md_gemm_fp8w_partial_slices(C.byref(st))) == p.slices
            ranges = WS.slice_ranges(p.k, p.slices, p.per)
            assert [hi - lo for lo, hi in ranges][:-1] == [p.per * 128] * (p.slices - 1) and ranges[-1][1] == p.k
    assert any(len({hi - lo for lo, hi in WS.slice_ranges(p.k, p.slices, p.per)}) > 1 for pair in WS.PAIRS for p in pair)
    with pytest.raises(AssertionError):
        WS.probe_headroom(WS.E4M3, 16384, 0)          # 16384 * 4 * 448 + 3 needs more than 24 bits
    for fmt in WS.FORMATS:
        for m, k, n in [(9, 640, 72), (5, 1152, 64)]:
            layer = WS.probe_layer(fmt, k, n, "cpu")
            bias = WS.probe_bias(layer.n_pad, n, "cpu")
            for shift in (0, WS.probe_a_shift(fmt, k)):
                a = WS.probe_activations(fmt, m, k, shift, "cpu", WS.gen("cpu", 3, fmt, m, k, n))
                exact, mag = wstream_exact(a, layer.q, layer.scale, bias)
                for order in ("kernel", "chunked"):
                    got = ws_model(a, layer.q, layer.scale, bias, order)
                    assert torch.equal(got, exact.to(BF16)) and torch.equal(got.double(), round_to_bf16(exact))
                    compare_f8_elementwise(f"wstream probe model {WS.FMT_NAME[fmt]} k={k}", got, exact, mag, layer.k_pad, exact_acc=True)
                    off = got.clone()
                    off.view(torch.int16)[m - 1, n - 1] += 1
                    with pytest.raises(AssertionError, match="1 of"):
                        compare_f8_elementwise("one bf16 step", off, exact, mag, layer.k_pad, exact_acc=True)


# ---- the instruments of tests/test_decode_b1_exact_gpu.py ---------------------------------------------------------------------
import util as B1
from moondream_amd.weights import rope_table
from util import (B1_BRANCHES, b1_barriers, b1_block_ref, b1_branches, b1_layout, bf16_spacing, err_in_spacings, gelu_interval)

B1_CU = 256  # the branch map at the CU count the shapes were chosen for; the GPU module repeats it with the device's own


def test_b1_case_list_takes_every_branch_at_256_cus():
    sh = B1.b1_shapes(B1_CU)
    assert sh["S3"]["dim"] == 2560
    per_shape = {}
    for name, n_layers, L, ctx, vocab in B1.b1_case_list():
        s = sh[name]
        per_shape.setdefault(name, set()).update(b1_branches(B1_CU, dim=s["dim"], n_heads=s["dim"] // 64, ff=s["ff"], L=L, ctx=ctx, vocab=vocab))
    assert set().union(*per_shape.values()) == set(B1_BRANCHES)
    assert {"empty proj half", "phase A idle waves", "empty key slice", "L = 8k + 1", "slice fills sc[] (chunk == B1_MAX_KEYS)",
            "pos == ctx - 1", "key index clamp to ctx - 1 binds", "phase D fewer row pairs than workgroups",
            "phase D second row pair per wave"} <= per_shape["S1"]
    assert {"two live proj halves, unequal", "two live fc2 halves, unequal", "fc2 half boundary not a multiple of 512 from the end"} <= per_shape["S2"]
    assert {"second (head, slice) item per workgroup", "phase C second pass", "combine second pass", "phase A second row pair per wave"} <= per_shape["S3"]
    assert {"dim limit (4096)", "ff limit (8192)"} <= per_shape["S4"]
    # the tiny and the 2b model on 256 CUs take none of the second passes: what the suite missed before
    for dim, ff in ((256, 704), (2048, 8192)):
        got = b1_branches(B1_CU, dim=dim, n_heads=dim // 64, ff=ff, L=740, ctx=2048, vocab=0)
        assert not got & {"second (head, slice) item per workgroup", "phase C second pass", "combine second pass"}, got
    assert b1_layout(256, 704, 4) == {"x0": 0, "x1": 512, "act": 1024, "part": 1024 + 3072, "total": 4096 + 8704}
    assert [b1_barriers(1, False), b1_barriers(2, False), b1_barriers(3, False), b1_barriers(1, True)] == [2, 5, 8, 4]


def _torch_bf16_block(x, w, kc, vc, pos, cs, sn, rot):
    """The block in float32 torch with a bf16 rounding at every documented point (reference layers.py / text.py / rope.py)."""
    F = torch.nn.functional
    f = lambda t: t.float()
    d = x.numel()
    h = d // 64
    ln = F.layer_norm(f(x), (d,), f(w["ln_w"]), f(w["ln_b"]), 1e-5).to(BF16)
    pre = F.linear(f(ln), f(w["w1"]), f(w["b1"])).to(BF16)
    g = F.gelu(f(pre[3 * d:]), approximate="tanh").to(BF16)
    q, k, v = pre[: 3 * d].view(3, h, 64)

    def rope(t):
        t = f(t)
        re, im = t[..., : rot // 2], t[..., rot // 2: rot]
        out = torch.stack((re * cs - im * sn, re * sn + im * cs), dim=-1).flatten(-2)
        return torch.cat([out, t[..., rot:]], dim=-1).to(BF16)

    qr, kr = rope(q), rope(k)
    keys, vals = torch.cat([f(kc[:, :pos]), f(kr)[:, None]], 1), torch.cat([f(vc[:, :pos]), f(v)[:, None]], 1)
    s = torch.einsum("hd,hjd->hj", f(qr), keys) * 0.125
    p = torch.exp(s - s.amax(-1, keepdim=True))
    att = (torch.einsum("hj,hjd->hd", f(p.to(BF16)), vals) / p.sum(-1, keepdim=True)).to(BF16).reshape(d)
    t1, t2 = F.linear(f(att), f(w["wp"]), f(w["bp"])).to(BF16), F.linear(f(g), f(w["w2"]), f(w["b2"])).to(BF16)
    x1 = (f(x) + f(t1)).to(BF16)
    return {"hidden": (f(x1) + f(t2)).to(BF16), "k": kr, "v": v, "act": torch.cat([pre[: 3 * d], g]), "att": att}


@pytest.mark.parametrize("name,pos,rot", [("S1", 9, 32), ("S2", 130, 32), ("S1", 40, 16), ("S1", 40, 64)])
def test_b1_rounded_reference_is_the_torch_bf16_block(name, pos, rot):
    s = B1.b1_shapes(B1_CU)[name]
    w, kc, vc, x = B1.tier2_inputs(s["dim"], s["ff"], "cpu")
    fr = rope_table(rot, B1.TIER2_CTX)[pos]
    ref = b1_block_ref(x.double(), w, kc.double(), vc.double(), pos, fr[:, 0].double(), fr[:, 1].double(), rot, rounded=True)
    alt = _torch_bf16_block(x, w, kc, vc, pos, fr[:, 0], fr[:, 1], rot)
    for key in ("act", "k", "v", "att", "hidden"):
        a, b = ref[key].reshape(-1), alt[key].double().reshape(-1)
        same = float((a == b).double().mean())
        worst = float(((a - b).abs() / bf16_spacing(a)).max())
        print(f"{name} pos {pos} rot {rot} {key}: {same:.4f} equal, worst {worst:.2f} spacings")
        # float32 against float64 between the roundings: a value next to a rounding boundary may fall on the other side
        assert same >= 0.97 and worst <= 1.0, (key, same, worst)


@pytest.mark.parametrize("L", [2, 9, 17, 2041])
def test_b1_slice_probe_sees_a_dropped_and_a_stale_key(L):
    s = B1.b1_shapes(B1_CU)["S1"]
    d, H, pos = s["dim"], s["dim"] // 64, L - 1
    w, vplant, kcache = B1.slice_probe_inputs(d, s["ff"], L, dev="cpu")
    kc, vc = kcache.clone(), vplant.clone()
    kc[:, pos], vc[:, pos] = float("nan"), float("nan")  # what the GPU probe leaves in row pos before the launch
    fr = rope_table(32, 2048)[pos].double()
    run = lambda **kw: b1_block_ref(torch.zeros(d, dtype=torch.float64), w, kc, vc, pos, fr[:, 0], fr[:, 1], 32, rounded=True, **kw)
    good = run()
    assert torch.equal(good["hidden"], round_to_bf16(vplant.sum(1).reshape(-1) / L))  # the probe's own expectation
    assert torch.equal(good["v"], vplant[:, pos])
    chunk = (L + 7) // 8
    for h, j in {(0, 0), (H - 1, pos), (1, min(chunk, pos)), (2, max(0, min(chunk, pos) - 1))}:
        bad = run(mutation="drop_key", drop=(h, j))["hidden"]
        # (the combined row is rounded to bf16: among 2041 keys one small power of two is below its spacing, which is why the
        # probe holds every partial, not only the row, to the exact sum)
        assert L > 17 or not torch.equal(bad, good["hidden"]), (h, j)
        # the partial the GPU probe compares exactly: the slice's sum without the key, or with another head's key in its place
        sl = j // chunk
        full = vplant[h, sl * chunk: min(L, sl * chunk + chunk)].sum(0)
        assert not torch.equal(full - vplant[h, j], full)
        assert not torch.equal(full - vplant[h, j] + vplant[(h + 1) % H, j], full)
        assert not torch.equal(full + vplant[h, j], full)
    assert bool(torch.isnan(run(mutation="stale_key")["hidden"]).any())  # the NaN row reaches hidden: the probe's NaN check fires


@pytest.mark.parametrize("name", ["S1", "S2"])
def test_b1_integer_block_sees_a_lost_rounding(name):
    s = B1.b1_shapes(B1_CU)[name]
    d, ff = s["dim"], s["ff"]
    one, zero = torch.ones(16, dtype=torch.float64), torch.zeros(16, dtype=torch.float64)
    H = d // 64
    nan = torch.full((H, 1, 64), float("nan"), dtype=torch.float64)
    x = B1.int_x(d, 22, "cpu")
    # residual chain: fc1 biases whose GELU is exact
    w = B1.int_weights(d, ff, 21, fc1_live=False, dev="cpu")
    good = b1_block_ref(x, w, nan, nan, 0, one, zero, 32, rounded=True)
    B1.assert_exact_block(name, w, good["att"], good["act"][3 * d:])
    want, single, swapped = B1.residual_chain(x, good["att"], good["act"][3 * d:], w)
    assert torch.equal(good["hidden"], want)
    bad = b1_block_ref(x, w, nan, nan, 0, one, zero, 32, rounded=True, mutation="one_residual_rounding")["hidden"]
    assert torch.equal(bad, single)
    for other in (single, swapped):
        assert float((other != want).double().mean()) >= 0.05
    # GELU before the rounding: outside the interval the phase-A check allows
    w = B1.int_weights(d, ff, 21, dev="cpu")
    good = b1_block_ref(x, w, nan, nan, 0, one, zero, 32, rounded=True)
    pre = w["w1"] @ w["ln_b"] + w["b1"]
    assert torch.equal(good["act"][: 3 * d], round_to_bf16(pre[: 3 * d]))
    lo, hi = gelu_interval(round_to_bf16(pre[3 * d:]))
    inside = lambda t: (t >= lo) & (t <= hi)
    assert bool(inside(good["act"][3 * d:]).all())
    bad = b1_block_ref(x, w, nan, nan, 0, one, zero, 32, rounded=True, mutation="gelu_before_rounding")["act"][3 * d:]
    share = float((~inside(bad)).double().mean())
    print(f"{name}: GELU before the rounding leaves the interval on {share:.3f} of the fc1 columns")
    assert share >= 0.05, share


def test_b1_second_pass_probe_sees_a_neighbouring_row_pair():
    s = B1.b1_shapes(B1_CU)["S3"]
    d, ff = s["dim"], s["ff"]
    one, zero = torch.ones(16, dtype=torch.float64), torch.zeros(16, dtype=torch.float64)
    nan = torch.full((d // 64, 1, 64), float("nan"), dtype=torch.float64)
    x = B1.int_x(d, 22, "cpu")
    w = B1.int_weights(d, ff, 21, fc1_live=False, dev="cpu")
    good = b1_block_ref(x, w, nan, nan, 0, one, zero, 32, rounded=True)["hidden"]
    bad = b1_block_ref(x, w, nan, nan, 0, one, zero, 32, rounded=True, mutation="neighbour_pair", n_cu=B1_CU)["hidden"]
    diff = bad != good
    assert not bool(diff[: 2 * B1_CU].any()) and float(diff[2 * B1_CU:].double().mean()) > 0.9
    # and the one-column probe: neighbouring rows differ in most of the columns it plants
    for mat in (w["wp"], w["w2"]):
        assert float((mat[2 * B1_CU: -2] != mat[2 * B1_CU + 2:]).double().mean()) > 0.8


# The Tier 2 margins compare two implementations of the SAME rounding points.  Their stand-ins here: the float64 block with those
# roundings (an ideal kernel) in the place of the persistent kernel, the float32 torch block in the place of the batched kernels.
# The ideal kernel must pass the Tier 2 check on the Tier 2 inputs in the Tier 2 unit (util.err_in_spacings with the addends).  Its
# own distance from the truth is printed: about one spacing RMS, while single elements reach 4 to 15 spacings where a dot product
# (proj, fc2, a logit) is itself a cancelled sum that carries the rounding of the layer norm and of the gelu row in every term --
# shared by every implementation of these rounding points, which is why the margins are relative to the batched kernels.
@pytest.mark.parametrize("name,positions", B1.TIER2_CASES)
def test_b1_tier2_inputs_keep_the_rounded_reference_within_the_margins(name, positions):
    s = B1.b1_shapes(B1_CU)[name]
    w, kc, vc, x = B1.tier2_inputs(s["dim"], s["ff"], "cpu")
    table = rope_table(32, B1.TIER2_CTX)
    for pos in positions:
        cs, sn = table[pos, :, 0], table[pos, :, 1]
        a = (x.double(), w, kc.double(), vc.double(), pos, cs.double(), sn.double(), 32)
        truth, rnd = b1_block_ref(*a, rounded=False), b1_block_ref(*a, rounded=True)
        yard = _torch_bf16_block(x, w, kc, vc, pos, cs, sn, 32)
        for key in ("hidden", "k", "v"):
            terms = B1.hidden_terms(truth) if key == "hidden" else ()
            (rms, mx), (yr, ym) = (err_in_spacings(t[key].reshape(-1), truth[key].reshape(-1), *terms) for t in (rnd, yard))
            print(f"{name} pos {pos} {key}: rounded reference rms {rms:.3f} max {mx:.2f} | float32 torch block rms {yr:.3f} max {ym:.2f} spacings")
            assert rms <= B1.B1_RMS_RATIO * yr and mx <= ym + B1.B1_MAX_EXTRA, (name, pos, key, rms, mx, yr, ym)


def test_b1_tier2_step_inputs_keep_the_rounded_logits_within_the_margins():
    F = torch.nn.functional
    s = B1.b1_shapes(B1_CU)["S1"]
    d = s["dim"]
    w, head, kc, vc = B1.tier2_step_inputs(d, s["ff"], "cpu")
    pos, token = B1.TIER2_STEP["pos"], B1.TIER2_STEP["token"]
    fr = rope_table(32, B1.TIER2_CTX)[pos]
    x = head["wte"][token]
    a = (x, w, kc.double(), vc.double(), pos, fr[:, 0].double(), fr[:, 1].double(), 32)
    h = [head[k] for k in ("post_w", "post_b", "lm_w", "lm_b")]
    lt, dot = B1.b1_logits_ref(b1_block_ref(*a, rounded=False)["hidden"], *h, rounded=False, parts=True)
    lr = B1.b1_logits_ref(b1_block_ref(*a, rounded=True)["hidden"], *h, rounded=True)
    hid = _torch_bf16_block(x.to(BF16), w, kc, vc, pos, fr[:, 0], fr[:, 1], 32)["hidden"]
    ln = F.layer_norm(hid.float(), (d,), h[0].float(), h[1].float(), 1e-5).to(BF16)
    ly = F.linear(ln.float(), h[2].float(), h[3].float()).to(BF16)
    (rms, mx), (yr, ym) = err_in_spacings(lr, lt, dot), err_in_spacings(ly, lt, dot)
    print(f"step logits: rounded reference rms {rms:.3f} max {mx:.2f} | float32 torch rms {yr:.3f} max {ym:.2f} spacings from the truth")
    assert rms <= B1.B1_RMS_RATIO * yr and mx <= ym + B1.B1_MAX_EXTRA, (rms, mx, yr, ym)


def test_err_in_spacings_counts_in_the_spacing_of_the_addends():
    truth = torch.tensor([1.0, 2.0 ** -10, 3.0], dtype=torch.float64)
    term = torch.tensor([0.25, 1.0, 0.5], dtype=torch.float64)
    got = truth + torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6], dtype=torch.float64)
    assert err_in_spacings(got, truth)[1] == 2.0 ** -7 / 2.0 ** -17          # the cancelled element alone: 1024 spacings
    assert err_in_spacings(got, truth, term) == (1.0, 1.0)                    # one spacing of its largest addend
    assert err_in_spacings(truth * (1 + 2.0 ** -4), truth, term)[1] >= 8.0    # a 6 % error of a result is still many spacings
