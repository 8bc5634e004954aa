"""The per-element GEMM bound of util.compare_elementwise has teeth and raises no false alarm: on the CPU, an fp32 accumulator
walked in 64-wide K chunks (the kernels' slice width) in several orders and split-K associations passes with zero violations,
and every localised error of the kind a ragged tile makes -- a K slice lost in one row, the bias lost in one column, two
8-column store groups swapped, the rows of the second 64-row half shifted by one -- is rejected, with every violation inside the
mutated region."""
import math

import pytest
import torch

from util import compare_elementwise, elementwise_excess

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
