"""md_sample_rows_filtered through the C ABI against the CPU restatement (tests/sampling_filter_ref.py): every sampled row's
renormalised probabilities word for word, its id for three uniforms, neutral rows against md_sample_rows, the greedy row
against md_argmax_bf16, the idle row untouched.

The restatement works on bf16 probabilities, and the kernel forms its own from fp32 exp / sum / divide, whose last bits
are not torch's.  So the rows are built from 64 logit levels and the test first checks ITS FIXTURE: every distinct
probability, computed in float64, lies at least 16 fp32 ulps from a bf16 rounding boundary (the device's fp32 error --
exp, a 51200-term sum, one division -- stays under 8), so the bf16 words are the same whoever computes them."""
import ctypes as C

import numpy as np
import pytest
import torch

from moondream_amd import _lib
from sampling_filter_ref import draw, filter_probs

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FILL_ID = -7
FILL_BITS = 0x7FC0  # a bf16 NaN: the pattern probs_out holds before the launch
U_MIXED = [0.37, 0.91, 0.5, 0.123, 0.77, 0.05, 0.66, 0.42, 0.98, 0.31, 0.59, 0.5, 0.5, 0.84, 0.29, 0.71]
U_LAST = float(np.nextafter(np.float32(1.0), np.float32(0.0)))  # the largest uniform below 1


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def words(t):
    return t.view(torch.int16).cpu()


def settings(vocab):
    """(temperature, top_p, top_k, min_p) per row.  Rows 11 / 12: greedy / idle.  Row 13: the best token is suppressed.
    Row 14: 8 tokens share the largest logit.  Row 15: a flat plateau of 20 tokens crosses k."""
    return [
        (0.5, 0.3, 0, 0.0),           # 0 neutral
        (0.5, 1.0, 1, 0.0),           # 1
        (0.5, 1.0, 2, 0.0),           # 2
        (0.7, 1.0, 40, 0.0),          # 3
        (0.5, 0.3, vocab, 0.0),       # 4 off: k == vocab
        (1.0, 0.9, vocab + 5, 0.0),   # 5 off: k > vocab
        (1.0, 1.0, 0, 1e-3),          # 6
        (0.5, 1.0, 0, 0.1),           # 7
        (0.7, 1.0, 0, 1.0),           # 8 only the tokens tied for best
        (1.0, 0.3, 40, 0.1),          # 9 all three
        (1.0, 1.0, 5, 1e-3),          # 10 both, top-p open
        (0.0, 0.3, 3, 0.5),           # 11 greedy: reads neither
        (-1.0, 0.3, 3, 0.5),          # 12 idle
        (0.5, 1.0, 3, 0.0),           # 13 suppressed best
        (0.5, 1.0, 3, 0.0),           # 14 ties at the top
        (1.0, 1.0, 11, 0.0),          # 15 plateau across k
    ]


GREEDY, IDLE, SUPPRESSED_BEST, TIES, PLATEAU = 11, 12, 13, 14, 15
NEUTRAL = [0, 4, 5]


def make_logits(vocab, ld):
    """[16, ld] bf16 from 64 levels (multiples of 0.25 in [-8, 8)), few tokens at the high ones; the planted rows."""
    g = torch.Generator().manual_seed(1000 + vocab)
    idx = (torch.randn(16, ld, generator=g).abs() * 14).long().clamp_(0, 63)
    logits = (-8.0 + 0.25 * idx.float()).to(BF16)
    suppress = 5 % vocab
    logits[SUPPRESSED_BEST, suppress] = 9.0
    tie_ids = [3, 11, 12, 20, 25, 30, 33, 36] if vocab < 64 else [7, 100, 101, 512, vocab // 2, vocab - 300, vocab - 2, vocab - 1]
    logits[TIES, tie_ids] = 9.0
    logits[PLATEAU, 2 % vocab] = 9.5
    plateau = list(range(8, 28)) if vocab < 64 else list(range(vocab // 3, vocab // 3 + 40, 2))
    logits[PLATEAU, plateau] = 9.0
    return logits, suppress, tie_ids, plateau


def host_probs(row, temperature, suppress):
    """p = bf16(softmax(bf16(logit / T))) of one row, from float64 -- and the fixture check of the module docstring."""
    z = (row.float() / temperature).to(BF16).double()
    if suppress >= 0:
        z[suppress] = float("-inf")
    e = torch.exp(z - z.max())
    p64 = e / e.sum()
    low = p64.float().view(torch.int32) & 0xFFFF
    live = p64 > 0
    assert int((low[live] - 0x8000).abs().min()) >= 16, "fixture: a probability sits on a bf16 rounding boundary"
    return p64.float().to(BF16)


def launch(lib, logits, ld, vocab, suppress, st, u, fn="md_sample_rows_filtered", probs_ld=None):
    b = logits.shape[0]
    dev = lambda vals, dt: torch.tensor(vals, dtype=dt, device="cuda")
    t, p = dev([s[0] for s in st], torch.float32), dev([s[1] for s in st], torch.float32)
    k, m = dev([s[2] for s in st], torch.int32), dev([s[3] for s in st], torch.float32)
    ud = dev(u, torch.float32)
    nxt = torch.full((b,), FILL_ID, dtype=torch.int32, device="cuda")
    pld = probs_ld or ld
    probs = torch.full((b, pld), FILL_BITS, dtype=torch.int16, device="cuda").view(BF16)
    if fn == "md_sample_rows":
        rc = lib.md_sample_rows(logits.data_ptr(), ld, b, vocab, suppress, t.data_ptr(), p.data_ptr(), ud.data_ptr(), nxt.data_ptr(),
                                probs.data_ptr(), pld, stream())
    else:
        rc = lib.md_sample_rows_filtered(logits.data_ptr(), ld, b, vocab, suppress, t.data_ptr(), p.data_ptr(), k.data_ptr(),
                                         m.data_ptr(), ud.data_ptr(), nxt.data_ptr(), probs.data_ptr(), pld, stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    return nxt.tolist(), words(probs)


@pytest.mark.parametrize("vocab", [37, 1025, 51200])
def test_every_row_against_the_restatement(lib, vocab):
    """37: fewer tokens than threads and than k = 40; 1025: one token past a whole chunk per thread; 51200: the model's.
    The row stride is vocab + 19: odd, so no row but the first is aligned to anything."""
    ld = vocab + 19
    host, suppress, tie_ids, plateau = make_logits(vocab, ld)
    logits = host.cuda()
    before = words(logits).clone()
    st = settings(vocab)
    sampled = [r for r in range(16) if st[r][0] > 0]

    want = {}
    for r in sampled:
        p = host_probs(host[r, :vocab], st[r][0], suppress)
        want[r] = filter_probs(p, st[r][1], st[r][2], st[r][3])

    runs = {name: launch(lib, logits, ld, vocab, suppress, st, u)
            for name, u in (("mixed", U_MIXED), ("zero", [0.0] * 16), ("last", [U_LAST] * 16))}
    plain_ids, plain_words = launch(lib, logits, ld, vocab, suppress, st, U_MIXED, fn="md_sample_rows")
    ids, got = runs["mixed"]
    fill = torch.tensor(FILL_BITS, dtype=torch.int16)

    for r in sampled:
        w = words(want[r])
        print(f"vocab {vocab} row {r}: {int((want[r].float() > 0).sum())} survivors, ids "
              f"{[runs[n][0][r] for n in ('mixed', 'zero', 'last')]}")
        assert torch.equal(got[r, :vocab], w), f"row {r}: probabilities differ from the restatement's"
        k = st[r][2]
        if 0 < k < vocab:
            assert int((got[r, :vocab] != 0).sum()) <= k, r
        for name, u in (("mixed", U_MIXED[r]), ("zero", 0.0), ("last", U_LAST)):
            assert torch.equal(runs[name][1][r], got[r]), (r, name)  # the uniform changes no probability
            assert runs[name][0][r] == draw(want[r], u), (r, name)
        assert ids[r] != suppress and want[r][suppress] == 0
    for r in NEUTRAL:  # the bits of md_sample_rows, id and probabilities
        assert ids[r] == plain_ids[r] and torch.equal(got[r], plain_words[r]), r

    # the planted rows
    kept = lambda r: (got[r, :vocab] != 0).nonzero().flatten().tolist()
    assert kept(1) == [int(torch.argmax(host[1, :vocab].float()))]  # k = 1: the argmax (lowest id of the best value)
    assert kept(TIES) == tie_ids[:3]
    assert kept(SUPPRESSED_BEST) and suppress not in kept(SUPPRESSED_BEST)
    assert kept(PLATEAU) == [2 % vocab] + plateau[:10]
    best8 = host[8, :vocab].float()
    assert kept(8) == (best8 == best8.max()).nonzero().flatten().tolist()  # min_p = 1: exactly the tokens tied for best

    # greedy: md_argmax_bf16's id (where its alignment contract holds; the plain argmax anywhere), nothing else written
    ref = host[GREEDY, :vocab].float().clone()
    ref[suppress] = float("-inf")
    assert ids[GREEDY] == int(torch.argmax(ref))
    if vocab % 8 == 0:
        one = torch.full((1,), FILL_ID, dtype=torch.int32, device="cuda")
        aligned = logits[GREEDY, :vocab].clone()
        _lib.check(lib.md_argmax_bf16(aligned.data_ptr(), vocab, 1, vocab, suppress, one.data_ptr(), stream()))
        torch.cuda.synchronize()
        assert ids[GREEDY] == int(one[0])
    assert ids[IDLE] == FILL_ID
    for r in (GREEDY, IDLE):
        assert bool((got[r] == fill).all()), f"row {r}: probs_out was written"
    assert bool((got[:, vocab:] == fill).all()), "probs_out was written past the vocabulary"
    assert torch.equal(words(logits), before), "the logits were written"


def test_null_settings_are_refused_on_the_host(lib):
    vocab = 64
    logits = torch.zeros(2, vocab, dtype=BF16, device="cuda")
    f = torch.tensor([1.0, 1.0], dtype=torch.float32, device="cuda")
    k = torch.zeros(2, dtype=torch.int32, device="cuda")
    nxt = torch.full((2,), FILL_ID, dtype=torch.int32, device="cuda")

    def call(top_k=k, min_p=f, t=f, ld=vocab):
        ptr = lambda x: x.data_ptr() if x is not None else None
        return lib.md_sample_rows_filtered(logits.data_ptr(), ld, 2, vocab, -1, ptr(t), f.data_ptr(), ptr(top_k), ptr(min_p),
                                           f.data_ptr(), nxt.data_ptr(), None, 0, stream())

    assert call(top_k=None) == 1 and call(min_p=None) == 1 and call(t=None) == 1 and call(ld=vocab - 1) == 1  # MD_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert nxt.tolist() == [FILL_ID, FILL_ID]  # rejected on the host: nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert all(0 <= i < vocab for i in nxt.tolist())


def test_a_captured_launch_replays_the_eager_one(lib):
    vocab, ld = 1025, 1044
    host, suppress, _, _ = make_logits(vocab, ld)
    logits = host.cuda()
    st = settings(vocab)
    eager_ids, eager_words = launch(lib, logits, ld, vocab, suppress, st, U_MIXED)
    dev = lambda vals, dt: torch.tensor(vals, dtype=dt, device="cuda")
    t, p = dev([s[0] for s in st], torch.float32), dev([s[1] for s in st], torch.float32)
    k, m = dev([s[2] for s in st], torch.int32), dev([s[3] for s in st], torch.float32)
    u = dev(U_MIXED, torch.float32)
    nxt = torch.full((16,), FILL_ID, dtype=torch.int32, device="cuda")
    probs = torch.full((16, ld), FILL_BITS, dtype=torch.int16, device="cuda").view(BF16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body = lambda: _lib.check(lib.md_sample_rows_filtered(
            logits.data_ptr(), ld, 16, vocab, suppress, t.data_ptr(), p.data_ptr(), k.data_ptr(), m.data_ptr(), u.data_ptr(),
            nxt.data_ptr(), probs.data_ptr(), ld, C.c_void_p(s.cuda_stream)))
        body()  # warm-up: the launch's one-time attribute call is not capturable
        s.synchronize()
        nxt.fill_(FILL_ID)
        probs.view(torch.int16).fill_(FILL_BITS)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            body()
        graph.replay()
        s.synchronize()
    assert nxt.tolist() == eager_ids
    assert torch.equal(words(probs), eager_words)
