"""md_penalize_rows on the MI355X through the C ABI against tests/penalty_ref.py: EXACT equality of the bf16 bits of the
whole logits array (padding columns included), of the whole history table and of the lengths, after every launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from moondream_amd import _lib
from penalty_ref import bf16_bits_to_f32, penalize_rows

pytestmark = pytest.mark.gpu
SHAPES = [(51200, 51200), (1000, 1003)]  # (vocab, ld)
NAN_BITS = 0x7FC0      # padding columns
POISON = 0x4B4B        # a finite bf16 (about 1.3e7): rows that must not be written; NaN-free, so a read-modify-write shows
HIST_SENT = -12345     # history entries nobody has written
NEG_INF = np.int16(-128)  # 0xFF80
MD_ERR_INVALID_ARG = 1  # include/moondream_hip.h


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_logits(rows, vocab, ld, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.full((rows, ld), NAN_BITS, dtype=torch.int16)
    x[:, :vocab] = (torch.randn(rows, vocab, generator=gen) * 8.0).to(torch.bfloat16).view(torch.int16)
    return x.numpy().copy()


def bits_of(value):
    return torch.tensor([value], dtype=torch.float32).to(torch.bfloat16).view(torch.int16).item()


def new_hist(n_slots, cap, rows=()):
    """History table with ``rows[s]`` (a token list) in slot s and sentinels everywhere else."""
    hist = np.full((n_slots, cap), HIST_SENT, dtype=np.int32)
    lens = np.zeros(n_slots, dtype=np.int32)
    for s, toks in enumerate(rows):
        hist[s, : len(toks)] = toks
        lens[s] = len(toks)
    return hist, lens


def launch(lib, logits, vocab, tokens_in, slots, slot0, hist, lens, rep, pres, freq, check=True):
    """One launch on copies of the arguments; returns (logits bits, hist, lens) as numpy, compared with the reference."""
    b = logits.shape[0]
    d_lg = torch.from_numpy(logits).cuda()
    d_tok = torch.tensor(tokens_in, dtype=torch.int32, device="cuda")
    d_slots = torch.tensor(slots, dtype=torch.int32, device="cuda") if slots is not None else None
    d_hist, d_len = torch.from_numpy(hist).cuda(), torch.from_numpy(lens).cuda()
    d_set = [torch.tensor(x, dtype=torch.float32, device="cuda") for x in (rep, pres, freq)]
    st = lib.md_penalize_rows(d_lg.data_ptr(), d_lg.stride(0), b, vocab, d_tok.data_ptr(),
                              d_slots.data_ptr() if d_slots is not None else None, slot0, d_hist.data_ptr(), hist.shape[1],
                              d_len.data_ptr(), d_set[0].data_ptr(), d_set[1].data_ptr(), d_set[2].data_ptr(), stream())
    assert st == 0, st
    torch.cuda.synchronize()
    got = d_lg.cpu().numpy(), d_hist.cpu().numpy(), d_len.cpu().numpy()
    if check:
        want = penalize_rows(logits, vocab, tokens_in, slots, slot0, hist, lens, rep, pres, freq)
        for name, g, w in zip(("logits", "hist", "hist_len"), got, want):
            bad = np.argwhere(g != w)
            assert bad.size == 0, (name, bad[:8].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    return got


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_histories_and_logit_values(lib, vocab, ld):
    """Empty, length 1, one token five times, 600 entries over 7 distinct tokens (each updated ONCE: a second update of a
    token would show in its bits), tokens 0 and vocab - 1; positive, negative, zero and -inf logits at penalised ids;
    repetition below and above 1, negative presence."""
    seven = [5, vocab // 2, 17, vocab - 2, 300, 301, 64]
    many = [seven[(i + i // 7) % 7] for i in range(599)]  # 599 + the appended token: 600 entries
    assert set(many) == set(seven)
    hist, lens = new_hist(4, 640, [[], [], [42] * 4, many])
    lg = make_logits(4, vocab, ld, seed=vocab)
    for v, val in zip(seven, (3.5, -2.25, 0.0, float("-inf"), 1e-3, -100.0, 7.0)):
        lg[3, v] = bits_of(val)
    lg[2, 42] = bits_of(6.0)
    lg[1, 9] = bits_of(-0.0)
    rep, pres, freq = [1.5, 1.3, 0.7, 1.25], [0.5, -0.5, 0.0, 0.75], [0.0, 0.25, 0.5, 0.125]
    got, _, got_len = launch(lib, lg, vocab, [-1, 9, 42, seven[3]], None, 0, hist, lens, rep, pres, freq)
    assert got_len.tolist() == [0, 1, 5, 600]
    assert (got[0] == lg[0]).all(), "an empty history penalises nothing"
    changed = np.flatnonzero(got[3, :vocab] != lg[3, :vocab]).tolist()
    assert sorted(changed) == sorted(v for v in seven if v != seven[3]), "every distinct token once; -inf stays -inf"
    assert got[3, seven[3]] == NEG_INF and got[3, seven[2]] != lg[3, seven[2]]  # 0 - (presence + frequency * c) < 0
    # the edges of the vocabulary
    hist, lens = new_hist(3, 16, [[0, vocab - 1], [vocab - 1], [0, 0]])
    lg = make_logits(3, vocab, ld, seed=vocab + 1)
    launch(lib, lg, vocab, [vocab - 1, 0, 0], None, 0, hist, lens, [2.0, 0.5, 1.0], [0.0, 1.0, -2.0], [1.0, 0.0, 0.5])


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_slot_table_with_an_idle_row(lib, vocab, ld):
    """slots [2, -1, 0]: the idle row's poisoned logits, its token and every history it could alias (slot 1 = its row
    index, slot 3 = one past the others) stay untouched; rows 0 and 2 land in slots 2 and 0."""
    hist, lens = new_hist(4, 12, [[7, 8], [1, 2, 3], [9], [4] * 12])
    lg = make_logits(3, vocab, ld, seed=3)
    lg[1, :] = np.int16(POISON)
    got, got_hist, got_len = launch(lib, lg, vocab, [100, 200, 300], [2, -1, 0], 0, hist, lens, [1.2] * 3, [0.5] * 3, [0.25] * 3)
    assert (got[1] == np.int16(POISON)).all()
    assert (got_hist[[1, 3]] == hist[[1, 3]]).all() and got_len.tolist() == [3, 3, 2, 12]
    assert got_hist[2, :2].tolist() == [9, 100] and got_hist[0, :3].tolist() == [7, 8, 300]
    assert got[0, 9] != lg[0, 9] and got[0, 100] != lg[0, 100] and got[2, 7] != lg[2, 7] and got[2, 300] != lg[2, 300]


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_contiguous_slots_from_slot0(lib, vocab, ld):
    hist, lens = new_hist(4, 12, [[11] * 3, [5], [6, 6], [13]])
    lg = make_logits(3, vocab, ld, seed=4)
    _, got_hist, got_len = launch(lib, lg, vocab, [21, 22, 23], None, 1, hist, lens, [0.8] * 3, [-1.0] * 3, [0.5] * 3)
    assert got_len.tolist() == [3, 2, 3, 2] and (got_hist[0] == hist[0]).all()
    assert [got_hist[s, got_len[s] - 1] for s in (1, 2, 3)] == [21, 22, 23]


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_full_history_and_tokens_that_are_no_ids(lib, vocab, ld):
    """hist_cap = 8, full: the token is dropped and the row is penalised over what the history holds.  A token outside
    [0, vocab) is not appended and the row is still penalised."""
    full = [3, 3, 4, 5, 3, 6, 4, 3]
    hist, lens = new_hist(4, 8, [full, full[:5], full[:2], full[:7]])
    lg = make_logits(4, vocab, ld, seed=5)
    got, got_hist, got_len = launch(lib, lg, vocab, [77, vocab, -5, 2**31 - 1], None, 0, hist, lens, [1.5, 1.5, 0.5, 1.0],
                                    [0.0, 1.0, 0.0, -3.0], [0.5, 0.0, 0.0, 0.0])
    assert got_len.tolist() == [8, 5, 2, 7] and (got_hist == hist).all()
    assert got[0, 77] == lg[0, 77] and all(got[0, v] != lg[0, v] for v in (3, 4, 5, 6))
    for r in (1, 2, 3):
        assert got[r, 3] != lg[r, 3]


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_neutral_row_beside_a_penalised_one(lib, vocab, ld):
    """The neutral row's logits keep their bits (a NaN-free poison pattern, so equality of bits means what it says and
    any write of another value shows) and its history still grows."""
    hist, lens = new_hist(3, 12, [[1, 2], [1, 2], [1, 2]])
    lg = make_logits(3, vocab, ld, seed=6)
    lg[1, :] = np.int16(POISON)
    got, got_hist, got_len = launch(lib, lg, vocab, [2, 2, 50], None, 0, hist, lens, [1.1, 1.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0])
    assert (got[1] == np.int16(POISON)).all() and got_len.tolist() == [3, 3, 3] and got_hist[1, :3].tolist() == [1, 2, 2]
    assert got[0, 2] != lg[0, 2] and got[2, 50] != lg[2, 50]


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_consecutive_launches_accumulate(lib, vocab, ld):
    hist, lens = new_hist(3, 12)
    rep, pres, freq = [1.3, 1.0, 0.9], [0.25, 0.0, -0.5], [0.5, 2.0, 0.0]
    for step, toks in enumerate(([8, 8, 8], [8, 9, vocab - 1], [8, 8, 0])):
        lg = make_logits(3, vocab, ld, seed=10 + step)  # fresh logits each step, as a decode step leaves them
        _, hist, lens = launch(lib, lg, vocab, toks, None, 0, hist, lens, rep, pres, freq)
    assert lens.tolist() == [3, 3, 3] and hist[:, :3].tolist() == [[8, 8, 8], [8, 9, 8], [8, vocab - 1, 0]]


def test_values_are_the_documented_rule(lib):
    """Hand-worked, independent of the restatement: 6.0 seen 5 times, repetition 0.7 -> 6 / 0.7 = 8.5714..., minus
    0.5 * 5 -> 6.0714..., bf16 6.0625; -2.25 at repetition 1.25 -> -2.8125, minus (0.75 + 0.125 * c)."""
    hist, lens = new_hist(2, 16, [[42] * 4, [7, 7]])
    lg = make_logits(2, 1000, 1003, seed=1)
    lg[0, 42], lg[1, 7] = bits_of(6.0), bits_of(-2.25)
    got, _, _ = launch(lib, lg, 1000, [42, 7], None, 0, hist, lens, [0.7, 1.25], [0.0, 0.75], [0.5, 0.125])
    assert bf16_bits_to_f32(got[0, 42:43])[0] == np.float32(6.0625)
    assert bf16_bits_to_f32(got[1, 7:8])[0] == np.float32(-3.9375)  # -2.8125 - (0.75 + 0.375) = -3.9375, exact in bf16


def test_error_codes(lib):
    lg = torch.zeros(2, 64, dtype=torch.bfloat16, device="cuda")
    tok = torch.zeros(2, dtype=torch.int32, device="cuda")
    hist = torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    ln = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = torch.ones(3, 2, dtype=torch.float32, device="cuda")
    good = dict(logits=lg.data_ptr(), ld=64, batch=2, vocab=64, tokens_in=tok.data_ptr(), slots=None, slot0=0, hist=hist.data_ptr(),
                hist_cap=8, hist_len=ln.data_ptr(), repetition=st[0].data_ptr(), presence=st[1].data_ptr(),
                frequency=st[2].data_ptr())
    call = lambda **kw: lib.md_penalize_rows(*{**good, **kw}.values(), stream())
    assert call() == 0 and call(batch=0) == 0
    for name in ("logits", "tokens_in", "hist", "hist_len", "repetition", "presence", "frequency"):
        assert call(**{name: None}) == MD_ERR_INVALID_ARG, name
    for bad in (dict(batch=-1), dict(vocab=0), dict(ld=63), dict(hist_cap=0), dict(hist_cap=_lib.MD_PENALTY_HIST_MAX + 1)):
        assert call(**bad) == MD_ERR_INVALID_ARG, bad
    torch.cuda.synchronize()
