"""The per-element GEMM bound of util.compare_elementwise has teeth and raises no false alarm: on the CPU, an fp32 accumulator
walked in 64-wide K chunks (the kernels' slice width) in several orders and split-K associations passes with zero violations,
and every localised error of the kind a ragged tile makes -- a K slice lost in one row, the bias lost in one column, two
8-column store groups swapped, the rows of the second 64-row half shifted by one -- is rejected, with every violation inside the
mutated region.

The same for the per-element attention bound of util.compare_attention_elementwise, on the probe inputs of
tests/test_attention_exact_gpu.py: a float32 model of the kernels (64-key tiles, online softmax, bf16 probabilities) is inside
it, and the model with ONE key wrongly admitted or wrongly dropped is outside it in every row the probe aims at that key."""
import math

import pytest
import torch

from test_attention_exact_gpu import DEC_CTX, PROBES, prefill_geometry, visibility
from util import attention_excess, compare_attention_elementwise, compare_elementwise, elementwise_excess

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
