"""md_sample_rows, the per-row form of md_sample_top_p, through the C ABI: a row of temperature > 0 carries the bits of
md_sample_top_p on that row alone with its scalars, a row of temperature 0 the id of md_argmax_bf16, a row of temperature
< 0 is left alone.  Every comparison is exact (ids, and raw bf16 words of the probabilities); the yardsticks are the two
older entry points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from moondream_amd import _lib

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FILL_ID = -7
FILL_BITS = 0x7FC0  # a bf16 NaN: the pattern probs_out holds before the launch

# (temperature, top_p, uniform) per row; None: not read by the kernel (the buffers hold NaN there)
SETTINGS = [
    (0.5, 0.3, 0.37),
    (4.0, 0.999, 0.91),
    (1.0, 1.0, 0.0),
    (1.0, 0.8, 0.999999),
    (0.05, 0.3, 0.5),
    (0.0, None, None),   # greedy; its maximum is the suppressed id
    (0.0, None, None),   # greedy, a two-way tie at the maximum
    (-1.0, None, None),  # idle
    (0.5, 0.3, 0.37),    # row 0 again, on a copy of its logits
]
SAMPLED, GREEDY, IDLE = [0, 1, 2, 3, 4, 8], [5, 6], 7


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def words(t):
    return t.view(torch.int16).cpu()


def filled(rows, ld):
    nxt = torch.full((rows,), FILL_ID, dtype=torch.int32, device="cuda")
    probs = torch.full((rows, ld), FILL_BITS, dtype=torch.int16, device="cuda").view(BF16)
    return nxt, probs


def f32(values):
    return torch.tensor([float("nan") if v is None else v for v in values], dtype=torch.float32, device="cuda")


def scalar_row(lib, logits, r, vocab, suppress, temperature, top_p, u):
    """md_sample_top_p on row r alone: (id, raw words of its probabilities)."""
    nxt, probs = filled(1, vocab)
    ud = torch.tensor([u], dtype=torch.float32, device="cuda")
    _lib.check(lib.md_sample_top_p(logits[r].data_ptr(), logits.stride(0), 1, vocab, suppress, temperature, top_p, ud.data_ptr(),
                                   nxt.data_ptr(), probs.data_ptr(), vocab, stream()))
    torch.cuda.synchronize()
    return int(nxt[0]), words(probs[0])


def argmax_row(lib, logits, r, vocab, suppress):
    nxt = torch.full((1,), FILL_ID, dtype=torch.int32, device="cuda")
    _lib.check(lib.md_argmax_bf16(logits[r].data_ptr(), logits.stride(0), 1, vocab, suppress, nxt.data_ptr(), stream()))
    torch.cuda.synchronize()
    return int(nxt[0])


@pytest.mark.parametrize("vocab", [520, 1504, 51200])
def test_a_row_equals_the_scalar_kernel_on_that_row(lib, vocab):
    """520: fewer tokens than the 1024 threads; 1504: the last threads' id chunks are ragged or empty; 51200: the model's.
    The row stride is vocab + 64, so a kernel that strides by the vocabulary reads the wrong rows."""
    ld = vocab + 64
    g = torch.Generator().manual_seed(vocab)
    logits = (torch.randn(9, ld, generator=g) * 3).to(BF16)
    suppress = int(torch.argmax(logits[0, :vocab].float()))
    logits[5, suppress] = 30.0  # row 5's maximum is the suppressed token
    tie_lo, tie_hi = 37, vocab - 11
    assert suppress not in (tie_lo, tie_hi)
    logits[6, tie_lo] = logits[6, tie_hi] = 40.0
    logits[8] = logits[0]
    logits = logits.cuda()
    assert float(logits[:, :vocab].float().max()) == 40.0 and float(logits[5, :vocab].float().max()) == 30.0

    nxt, probs = filled(9, ld)
    t, p, u = (f32([s[k] for s in SETTINGS]) for k in range(3))
    _lib.check(lib.md_sample_rows(logits.data_ptr(), ld, 9, vocab, suppress, t.data_ptr(), p.data_ptr(), u.data_ptr(),
                                  nxt.data_ptr(), probs.data_ptr(), ld, stream()))
    torch.cuda.synchronize()
    got_ids, got_words = nxt.tolist(), words(probs)

    for r in SAMPLED:
        want_id, want_words = scalar_row(lib, logits, r, vocab, suppress, *SETTINGS[r])
        assert got_ids[r] == want_id, (r, got_ids[r], want_id)
        assert torch.equal(got_words[r, :vocab], want_words), f"row {r}: probabilities differ from md_sample_top_p's"
        assert 0 <= got_ids[r] < vocab and got_ids[r] != suppress
    assert got_ids[8] == got_ids[0] and torch.equal(got_words[8], got_words[0])
    for r in GREEDY:
        assert got_ids[r] == argmax_row(lib, logits, r, vocab, suppress), r
    ref5 = logits[5, :vocab].float().cpu()
    ref5[suppress] = float("-inf")
    assert got_ids[5] == int(torch.argmax(ref5)) != suppress
    assert got_ids[6] == tie_lo
    assert got_ids[IDLE] == FILL_ID
    fill = torch.tensor(FILL_BITS, dtype=torch.int16)
    for r in GREEDY + [IDLE]:
        assert bool((got_words[r] == fill).all()), f"row {r}: probs_out was written"
    assert bool((got_words[:, vocab:] == fill).all()), "probs_out was written past the vocabulary"


def test_reference_fixture_through_the_per_row_entry_point(lib, golden_dir):
    """Every case of tests/golden/sampling_top_p.npz (the reference's softmax + _apply_top_p on fixed logits) with its own
    (temperature, top_p) per row: ids and probabilities equal the per-case md_sample_top_p call.  A launch has one
    vocabulary size, so the cases of each size are stacked into one launch."""
    from util import bits_to_bf16

    g = np.load(os.path.join(golden_dir, "sampling_top_p.npz"))
    by_vocab = {}
    for i in range(int(g["n_cases"])):
        by_vocab.setdefault(g[f"case{i}.logits"].shape[1], []).append(i)
    assert sum(len(c) for c in by_vocab.values()) == int(g["n_cases"])
    for vocab, cases in by_vocab.items():
        logits = torch.cat([bits_to_bf16(g[f"case{i}.logits"]) for i in cases]).cuda()
        rows_of = [g[f"case{i}.logits"].shape[0] for i in cases]
        t = f32([float(g[f"case{i}.temperature"]) for i, n in zip(cases, rows_of) for _ in range(n)])
        p = f32([float(g[f"case{i}.top_p"]) for i, n in zip(cases, rows_of) for _ in range(n)])
        b = logits.shape[0]
        u = torch.linspace(0.05, 0.95, b, device="cuda")
        nxt, probs = filled(b, vocab)
        _lib.check(lib.md_sample_rows(logits.data_ptr(), vocab, b, vocab, -1, t.data_ptr(), p.data_ptr(), u.data_ptr(),
                                      nxt.data_ptr(), probs.data_ptr(), vocab, stream()))
        torch.cuda.synchronize()
        r0 = 0
        for i, n in zip(cases, rows_of):
            part = logits[r0 : r0 + n]
            want_n, want_p = filled(n, vocab)
            _lib.check(lib.md_sample_top_p(part.data_ptr(), vocab, n, vocab, -1, float(g[f"case{i}.temperature"]),
                                           float(g[f"case{i}.top_p"]), u[r0 : r0 + n].data_ptr(), want_n.data_ptr(),
                                           want_p.data_ptr(), vocab, stream()))
            torch.cuda.synchronize()
            assert nxt[r0 : r0 + n].tolist() == want_n.tolist(), i
            assert torch.equal(words(probs[r0 : r0 + n]), words(want_p)), i
            assert bool((probs[r0 : r0 + n].float() > 0).any())  # (the fill pattern is gone: the rows were sampled)
            r0 += n


def test_argument_checks(lib):
    vocab = 520
    logits = torch.zeros(2, vocab, dtype=BF16, device="cuda")
    t = f32([1.0, 0.0])
    p = f32([0.5, 0.5])
    u = f32([0.5, 0.5])
    nxt, probs = filled(2, vocab)

    def call(t_=t, p_=p, u_=u, ld=vocab):
        return lib.md_sample_rows(logits.data_ptr(), ld, 2, vocab, -1, t_.data_ptr() if t_ is not None else None,
                                  p_.data_ptr() if p_ is not None else None, u_.data_ptr() if u_ is not None else None,
                                  nxt.data_ptr(), probs.data_ptr(), vocab, stream())

    assert call(t_=None) == 1 and call(p_=None) == 1 and call(u_=None) == 1  # MD_ERR_INVALID_ARG
    assert call(ld=vocab - 8) == 1
    torch.cuda.synchronize()
    assert nxt.tolist() == [FILL_ID, FILL_ID]  # rejected on the host: nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    got = nxt.tolist()
    assert 0 <= got[0] < vocab and got[1] == 0  # (all-equal logits: the greedy row takes the lowest id)
