"""md_region_pick_encode_scored on the MI355X through the C ABI: bins and Fourier features bit for bit those of
md_region_pick_encode on the same inputs, the window log-probabilities against the float64 restatement of
tests/detect_score_ref.py within a bound derived from the kernel's documented summation order, a full window exactly 0.0,
a row's bits independent of the launch it sits in, nothing written outside [b, g], and the argument checks."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from detect_score_ref import bf16_bits_to_f64, group_logprob, region_scores
from moondream_amd import _lib

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
THREADS = 256        # the workgroup of region_pick_scored_kernel (csrc/sampling_region.hip)
WAVES = THREADS // 64
B = 5
HALF = 40            # Fourier features per half: not a multiple of the wave
SENT_LP = -12345.0   # what the outputs hold before a launch
SENT_BIN = -77
SENT_FEAT = 0x7B7B
NAN_BITS = 0x7FC0    # a bf16 NaN: the padding columns of the logits, which must not be read
U = 2.0 ** -24       # unit roundoff of fp32

# The log-probability bound.  got = log(W) - log(S) in fp32; S the sum of e_i = exp(x_i - m) over the group, W over the window,
# both in the order the kernel documents: n_t = ceil(n_bins / 256) terms per thread sequentially, 6 butterfly levels, then the
# 4 wave partials one after the other.  L = ln(n_bins).  All in units of U, absolute, per sum (the errors of W and of S need
# not cancel, so each is charged twice -- except at a full window, which the tests hold to exactly 0.0 instead):
#   additions: every term passes through at most (n_t - 1) + 6 + 3 additions of relative error <= U each, all terms >= 0:
#              a relative error <= (n_t + 8) U of the sum, that much absolute error of its logarithm                  n_t + 8
#   exp:       expf is good to 2 ulp = 4 U relative per term, hence <= 4 U relative in the sum                           4
#   subtract:  x_i - m is a rounded fp32 difference, absolute error <= U d_i with d_i = m - x_i, which changes e_i by the
#              factor exp(+-U d_i): relative error of the sum <= U sum_i p_i d_i, p_i = e_i / sum; the pick's own term is
#              exp(0) = 1 and lies in both sums, so sum >= 1 and sum_i p_i d_i = entropy(p) - ln(sum) <= L                L
#   log:       logf is good to 2 ulp = 4 U relative, of a logarithm that lies in [0, L] (1 <= W <= S <= n_bins)           4 L
# and once: the final subtraction, U |ref|; one unit of slack for the products of the (1 + U)-factors (second order); and a
# term below the smallest normal fp32 number may be flushed to zero: n_bins * 2^-126 against a sum >= 1.
def bound(n_bins, ref):
    n_t = -(-n_bins // THREADS)
    per_sum = (n_t + math.log2(64) + (WAVES - 1) - 1) + 4 + math.log(n_bins) + 4 * math.log(n_bins)
    return (2 * per_sum + 1) * U + U * abs(ref) + n_bins * 2.0 ** -126


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_rows(groups, n_bins):
    """(names, logits bf16 [B, groups * n_bins]): random rows at the logit scale of the region head with the planted groups."""
    gen = torch.Generator().manual_seed(1000 * groups + n_bins)
    lg = (torch.randn(B, groups, n_bins, generator=gen) * 4.0).to(BF16)
    top = lambda r, g: float(lg[r, g].float().max())
    names = {}
    v = top(0, 0) + 1.0
    lg[0, 0, 0] = lg[0, 0, 500] = v                                       # a tie that the lowest bin wins: a pick at bin 0
    names[(0, 0)] = "tie of bins 0 and 500"
    lg[1, 0, n_bins - 1] = top(1, 0) + 2.0
    names[(1, 0)] = "pick at the last bin"
    lg[2, 0, :] = 1.5
    names[(2, 0)] = "all equal"
    lg[3, 0, 100:300] = float("-inf")
    lg[3, 0, n_bins - 5 :] = float("-inf")
    names[(3, 0)] = "-inf entries"
    lg[4, 0, 777] = top(4, 0) + 30.0
    names[(4, 0)] = "spike of +30"
    if groups == 2:
        v = top(0, 1) + 0.5
        lg[0, 1, 300] = lg[0, 1, 700] = lg[0, 1, n_bins - 1] = v
        names[(0, 1)] = "tie of bins 300, 700 and the last"
        lg[1, 1, 0] = top(1, 1) + 2.0
        names[(1, 1)] = "pick at bin 0"
        lg[2, 1, :] = -3.0
        names[(2, 1)] = "all equal"
        lg[3, 1, 3] = top(3, 1) + 30.0
        names[(3, 1)] = "spike of +30 near the start"
        lg[4, 1, 0:64] = float("-inf")
        names[(4, 1)] = "-inf entries"
    return names, lg.reshape(B, groups * n_bins)


class Case:
    pass


_CASES = {}


def case(groups, n_bins):
    """Per shape, built once: inputs on the device in buffers whose row strides exceed the rows (NaN in the logits' padding)."""
    key = (groups, n_bins)
    if key in _CASES:
        return _CASES[key]
    c = Case()
    c.groups, c.n_bins = groups, n_bins
    c.names, lg = make_rows(groups, n_bins)
    c.ld = groups * n_bins + 24
    padded = torch.full((B, c.ld), NAN_BITS, dtype=torch.int16).view(BF16)
    padded[:, : groups * n_bins] = lg
    c.bits = lg.view(torch.int16).numpy().copy()
    c.logits = padded.cuda()
    gen = torch.Generator().manual_seed(5)
    c.table = (torch.arange(n_bins) / n_bins).to(BF16).cuda()
    c.fw = torch.randn(groups, HALF, generator=gen).to(BF16).cuda()
    c.refs = {}
    _CASES[key] = c
    return c


def ref_for(c, window):
    if window not in c.refs:
        c.refs[window] = region_scores(c.bits, c.groups, c.n_bins, window)
    return c.refs[window]


def launch(lib, c, logits, rows, window, scored=True):
    """One launch over ``rows`` rows of ``logits`` (stride c.ld).  Outputs sit in buffers two rows longer than the launch and
    wider than the groups, prefilled with sentinels; asserts that nothing outside [b, g] / the feature columns was written.
    Returns (bins [rows, groups], feature bits [rows, 2 * HALF], logprobs fp32 [rows, groups] or None)."""
    g, ldb, ldf, ldl = c.groups, 3, 2 * HALF + 8, 3
    bins = torch.full((rows + 2, ldb), SENT_BIN, dtype=torch.int32, device="cuda")
    feats = torch.full((rows + 2, ldf), SENT_FEAT, dtype=torch.int16, device="cuda")
    lps = torch.full((rows + 2, ldl), SENT_LP, dtype=torch.float32, device="cuda")
    head = (logits.data_ptr(), c.ld, rows, g, c.n_bins, c.table.data_ptr(), c.fw.data_ptr(), HALF, bins.data_ptr(), ldb,
            feats.data_ptr(), ldf)
    if scored:
        st = lib.md_region_pick_encode_scored(*head, window, lps.data_ptr(), ldl, stream())
    else:
        st = lib.md_region_pick_encode(*head, stream())
    assert st == 0, st
    torch.cuda.synchronize()
    bins, feats, lps = bins.cpu().numpy(), feats.cpu().numpy(), lps.cpu().numpy()
    assert (bins[rows:] == SENT_BIN).all() and (bins[:, g:] == SENT_BIN).all(), "bins written outside [b, g]"
    assert (feats[rows:] == SENT_FEAT).all() and (feats[:, 2 * HALF :] == SENT_FEAT).all(), "features written outside the row"
    if scored:
        assert (lps[rows:] == np.float32(SENT_LP)).all() and (lps[:, g:] == np.float32(SENT_LP)).all(), "logprobs written outside [b, g]"
    else:
        assert (lps == np.float32(SENT_LP)).all()
    return bins[:rows, :g], feats[:rows, : 2 * HALF], lps[:rows, :g] if scored else None


def words(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32).tolist()


@pytest.mark.parametrize("n_bins", [1024, 1000])
@pytest.mark.parametrize("groups", [1, 2])
def test_kernel_against_the_plain_pick_and_float64(lib, groups, n_bins):
    c = case(groups, n_bins)
    x64 = bf16_bits_to_f64(c.bits).reshape(B, groups, n_bins)

    # the test's own sensitivity, on the CPU: ONE bin of share >= 1e-3 left out of S lands outside the bound
    n_seen = 0
    for r in range(B):
        for g in range(groups):
            x = x64[r, g]
            pick = int(ref_for(c, 0)[0][r, g])
            e = np.exp(x - x[pick])
            share = e / e.sum()
            for i in np.flatnonzero((share >= 1e-3) & (np.arange(n_bins) != pick))[:4]:
                ref = group_logprob(x, pick, 0)
                omitted = -math.log(e.sum() - e[i])
                assert abs(omitted - ref) > bound(n_bins, ref), (c.names.get((r, g)), int(i), omitted, ref)
                n_seen += 1
    assert n_seen >= 4

    plain_bins, plain_feats, _ = launch(lib, c, c.logits, B, 0, scored=False)
    assert plain_bins[0, 0] == 0 and plain_bins[1, 0] == n_bins - 1 and plain_bins[2, 0] == 0  # the planted picks
    if groups == 2:
        assert plain_bins[0, 1] == 300 and plain_bins[1, 1] == 0 and plain_bins[3, 1] == 3
    worst = 0.0
    for window in (0, 1, 8, n_bins - 1):
        bins, feats, lps = launch(lib, c, c.logits, B, window)
        assert (bins == plain_bins).all() and (feats == plain_feats).all(), f"window {window}: bins / features differ from md_region_pick_encode"
        ref_bins, ref = ref_for(c, window)
        assert (bins == ref_bins).all()
        for r in range(B):
            for g in range(groups):
                got, want = float(lps[r, g]), float(ref[r, g])
                name = (c.names.get((r, g), "random"), window)
                if window == n_bins - 1:
                    assert want == 0.0 and got == 0.0 and not math.copysign(1.0, got) < 0, (name, got, want)
                    continue
                err, lim = abs(got - want), bound(n_bins, want)
                worst = max(worst, err / lim)
                assert err <= lim, (name, got, want, err, lim)
        if window == 0:
            for g in range(groups):  # the all-equal row
                assert abs(float(lps[2, g]) + math.log(n_bins)) <= bound(n_bins, math.log(n_bins))
    print(f"groups {groups} n_bins {n_bins}: worst |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("n_bins", [1024, 1000])
@pytest.mark.parametrize("groups", [1, 2])
def test_a_rows_bits_do_not_depend_on_the_launch(lib, groups, n_bins):
    """Alone, at B = 5 and at B = 70 in other row positions: the same fp32 bits, bins and features."""
    c = case(groups, n_bins)
    for window in (0, 8):
        bins5, feats5, lps5 = launch(lib, c, c.logits, B, window)
        for r in range(B):
            b1, f1, l1 = launch(lib, c, c.logits[r : r + 1], 1, window)
            assert (b1[0] == bins5[r]).all() and (f1[0] == feats5[r]).all() and words(l1[0]) == words(lps5[r]), (r, window)
        idx = [(3 * i + 1) % B for i in range(70)]
        big = c.logits[idx].contiguous()
        assert big.stride(0) == c.ld
        b70, f70, l70 = launch(lib, c, big, 70, window)
        for i, r in enumerate(idx):
            assert (b70[i] == bins5[r]).all() and (f70[i] == feats5[r]).all() and words(l70[i]) == words(lps5[r]), (i, r, window)


def test_nan_rules(lib):
    """A NaN in a group: never picked, the group's value is NaN; an all-NaN group: bin 0, NaN.  The other group is untouched."""
    c = case(2, 1000)
    lg = c.logits[:2].clone()
    lg[0, 17] = float("nan")
    lg[1, 1000:2000] = float("nan")
    torch.cuda.synchronize()
    plain_bins, plain_feats, _ = launch(lib, c, lg, 2, 0, scored=False)
    bins, feats, lps = launch(lib, c, lg, 2, 3)
    assert (bins == plain_bins).all() and (feats == plain_feats).all()
    assert bins[0, 0] == 0 and bins[1, 1] == 0
    assert math.isnan(lps[0, 0]) and math.isnan(lps[1, 1])
    ref = ref_for(c, 3)[1]
    for r, g in ((0, 1), (1, 0)):
        assert abs(float(lps[r, g]) - ref[r, g]) <= bound(1000, ref[r, g])


def test_kernel_argument_checks(lib):
    c = case(1, 1000)
    g, ldb, ldf, ldl = 1, 3, 2 * HALF + 8, 3
    bins = torch.full((B, ldb), SENT_BIN, dtype=torch.int32, device="cuda")
    feats = torch.full((B, ldf), SENT_FEAT, dtype=torch.int16, device="cuda")
    lps = torch.full((B, ldl), SENT_LP, dtype=torch.float32, device="cuda")
    good = dict(logits=c.logits.data_ptr(), ld=c.ld, batch=B, n_groups=g, n_bins=c.n_bins, table=c.table.data_ptr(), fw=c.fw.data_ptr(),
                half=HALF, bins=bins.data_ptr(), ld_bins=ldb, feats=feats.data_ptr(), ld_feats=ldf, window=0, logprobs=lps.data_ptr(),
                ld_logprobs=ldl)
    call = lambda **kw: lib.md_region_pick_encode_scored(*{**good, **kw}.values(), stream())
    for bad in (dict(window=-1), dict(logprobs=None), dict(ld_logprobs=0), dict(logits=None), dict(bins=None), dict(feats=None),
                dict(table=None), dict(fw=None), dict(batch=0), dict(batch=-1), dict(n_bins=0), dict(n_groups=0), dict(n_groups=3),
                dict(ld=c.n_bins - 1), dict(ld_bins=0), dict(ld_feats=2 * HALF - 1)):
        assert call(**bad) == 1, bad  # MD_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (bins == SENT_BIN).all() and (feats == SENT_FEAT).all() and (lps == SENT_LP).all()  # nothing was launched
    assert call(window=2 ** 31 - 1) == 0  # any window >= 0: clamped to the group
    torch.cuda.synchronize()
    assert lps[:, 0].tolist() == [0.0] * B
