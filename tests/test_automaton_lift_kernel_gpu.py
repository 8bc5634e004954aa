"""md_automaton_lift / md_automaton_count / md_automaton_fill on the MI355X through the C ABI against tests/grammar_ref.py:
EXACT equality of the whole next matrix and of the four compacted arrays (integers: there is no tolerance)."""
import ctypes as C

import numpy as np
import pytest
import torch

import grammar_ref as ref
from moondream_amd import _lib
from moondream_amd.grammar import vocab_arrays

pytestmark = pytest.mark.gpu
MD_ERR_INVALID_ARG = 1  # include/moondream_hip.h
SLAB = _lib.MD_AUTOMATON_SLAB
GUARD = 64  # poisoned int32 entries behind every output
POISON = 0x5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_dfa(s, seed, live=0.35):
    """A seeded DFA: every entry dead or a random state; in every state the bytes of '0'..'9' mostly lead somewhere, so that
    multi-byte tokens survive.  State 0 accepts iff the seed is even (eos is met at both kinds)."""
    rng = np.random.default_rng(seed)
    trans = np.where(rng.random((s, 256)) < live, rng.integers(0, s, size=(s, 256)), -1).astype(np.int32)
    trans[:, 0x30:0x3A] = rng.integers(0, s, size=(s, 10))
    accept = rng.random(s) < 0.5
    accept[0] = seed % 2 == 0
    return trans, accept


class Problem:
    """One DFA and vocabulary on the device, with the reference's next matrix (computed once)."""

    def __init__(self, trans, accept, vocab_bytes, eos_id, forbidden_ids=()):
        self.trans, self.accept = np.ascontiguousarray(trans, dtype=np.int32), np.asarray(accept, dtype=bool)
        self.s, self.v, self.eos = self.trans.shape[0], len(vocab_bytes), eos_id
        self.tok_off, self.tok_bytes = vocab_arrays(vocab_bytes)
        self.forbidden = np.zeros(self.v, dtype=np.uint8)
        self.forbidden[list(forbidden_ids)] = 1
        self.want_next = ref.lift(self.trans, self.accept, vocab_bytes, eos_id, self.forbidden)
        self.d = [dev(self.trans), dev(self.accept.astype(np.uint8)), dev(self.tok_off), dev(self.tok_bytes), dev(self.forbidden)]

    def common(self):
        t, a, off, data, forb = self.d
        return (t.data_ptr(), a.data_ptr(), self.s, off.data_ptr(), data.data_ptr(), int(self.tok_bytes.shape[0]), self.v, self.eos,
                forb.data_ptr())


def guarded(n):
    return torch.full((n + GUARD,), POISON, dtype=torch.int32, device="cuda")


def check_guard(t, n, what):
    assert bool((t[n:] == POISON).all()), f"{what}: written past its {n} entries"


def device_next(lib, p):
    out = np.empty((p.s, p.v), dtype=np.int32)
    for q0 in range(0, p.s, SLAB):
        nq = min(SLAB, p.s - q0)
        d = guarded(nq * p.v)
        assert lib.md_automaton_lift(*p.common(), q0, nq, d.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        check_guard(d, nq * p.v, "next")
        out[q0 : q0 + nq] = d[: nq * p.v].cpu().numpy().reshape(nq, p.v)
    return out


def device_compact(lib, p):
    ws_bytes = lib.md_automaton_workspace_bytes(p.s, p.v)
    assert ws_bytes == min(p.s, SLAB) * p.v * 4
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    default, row_ptr = guarded(p.s), guarded(p.s + 1)
    assert lib.md_automaton_count(*p.common(), default.data_ptr(), row_ptr.data_ptr(), ws.data_ptr(), ws_bytes, stream()) == 0
    torch.cuda.synchronize()
    n = int(row_ptr[p.s].item())
    assert 0 <= n <= p.s * p.v
    tok, nxt = guarded(n), guarded(n)
    assert lib.md_automaton_fill(*p.common(), default.data_ptr(), row_ptr.data_ptr(), tok.data_ptr(), nxt.data_ptr(), n, ws.data_ptr(),
                                 ws_bytes, stream()) == 0
    torch.cuda.synchronize()
    for t, k, what in ((default, p.s, "default_next"), (row_ptr, p.s + 1, "row_ptr"), (tok, n, "edge_tok"), (nxt, n, "edge_next")):
        check_guard(t, k, what)
    return tuple(t[:k].cpu().numpy() for t, k in ((row_ptr, p.s + 1), (default, p.s), (tok, n), (nxt, n)))


def check(lib, p):
    got = device_next(lib, p)
    bad = np.argwhere(got != p.want_next)
    assert bad.size == 0, ("next", len(bad), bad[:8].tolist(), got[tuple(bad[0])], p.want_next[tuple(bad[0])])
    want = ref.compact(p.want_next)
    for name, g, w in zip(("row_ptr", "default_next", "edge_tok", "edge_next"), device_compact(lib, p), want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, g.shape, w.shape, g[:16], w[:16])
    return want


# V around the 256-token workgroup, S around the state group of 4 and the LDS / global switch (128) and one above the slab
@pytest.mark.parametrize("v", [1, 255, 257, 1000])
@pytest.mark.parametrize("s", [1, 3])
def test_small_shapes(lib, v, s):
    vocab = ref.synthetic_vocab(v, seed=v + s)
    trans, accept = random_dfa(s, seed=v + s)
    for eos in sorted({0, v - 1}):
        check(lib, Problem(trans, accept, vocab, eos, forbidden_ids=[i for i in (2, v // 2) if i < v]))


@pytest.mark.parametrize("s", [128, 129, SLAB + 1])
def test_state_counts_across_the_lds_switch_and_the_slab(lib, s):
    vocab = ref.synthetic_vocab(1000, seed=s)
    trans, accept = random_dfa(s, seed=s)
    check(lib, Problem(trans, accept, vocab, eos_id=999, forbidden_ids=[0, 3, 500]))


def test_full_vocabulary(lib):
    vocab = ref.synthetic_vocab(51200, seed=11)
    trans, accept = random_dfa(64, seed=11)
    check(lib, Problem(trans, accept, vocab, eos_id=0, forbidden_ids=range(1, 10)))


def test_defaults_ties_and_dead_states(lib):
    """State 0: every byte leads to state 1 -> the default is a state id.  State 1: everything dead, not accepting -> every
    token forbidden, no edge.  State 2: exactly as many tokens to state 0 as to state 1, the rest fewer -> the tie goes to
    the smaller value.  State 3: accepting and dead -> only eos (FREE) is an edge."""
    v = 64
    vocab = [bytes([b]) for b in range(v)]
    trans = np.full((4, 256), -1, dtype=np.int32)
    trans[0, :] = 1
    trans[2, 0:20], trans[2, 20:40], trans[2, 40:50] = 1, 0, 3
    accept = np.array([False, False, False, True])
    p = Problem(trans, accept, vocab, eos_id=63, forbidden_ids=[55])
    row_ptr, default, tok, nxt = check(lib, p)
    assert default.tolist() == [1, ref.FORBID, 0, ref.FORBID]
    assert row_ptr.tolist()[:3] == [0, 2, 2] and tok[:2].tolist() == [55, 63]  # state 0: the forbidden id and eos; state 1: none
    counts = np.bincount(p.want_next[2] + 3)
    assert counts[0 + 3] == counts[1 + 3] == 20 and counts.max() == 20, "state 2 is a tie between states 0 and 1"
    assert tok[row_ptr[3] : row_ptr[4]].tolist() == [63] and nxt[row_ptr[3] : row_ptr[4]].tolist() == [ref.FREE]


def test_invalid_arguments_launch_nothing(lib):
    p = Problem(*random_dfa(3, seed=1), ref.synthetic_vocab(300, seed=1), eos_id=0)
    nxt = guarded(3 * p.v)
    default, row_ptr, tok, edge = guarded(3), guarded(4), guarded(8), guarded(8)
    ws_bytes = lib.md_automaton_workspace_bytes(3, p.v)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    good = list(p.common())
    lift = lambda c, q0=0, nq=3, out=nxt.data_ptr(): lib.md_automaton_lift(*c, q0, nq, out, stream())
    count = lambda c, d=default.data_ptr(), r=row_ptr.data_ptr(), w=ws.data_ptr(), wb=ws_bytes: lib.md_automaton_count(*c, d, r, w, wb, stream())
    fill = lambda c, cap=8, w=ws.data_ptr(), wb=ws_bytes: lib.md_automaton_fill(*c, default.data_ptr(), row_ptr.data_ptr(), tok.data_ptr(),
                                                                                edge.data_ptr(), cap, w, wb, stream())
    bad_commons = []
    for i in (0, 1, 3, 4, 8):  # trans, accept, tok_off, tok_bytes, forbidden: NULL
        bad_commons.append(good[:i] + [None] + good[i + 1 :])
    for i, x in ((2, 0), (2, _lib.MD_AUTOMATON_STATES_MAX + 1), (6, 0), (6, _lib.MD_CONSTRAIN_VOCAB_MAX + 1), (7, -1), (7, p.v)):
        bad_commons.append(good[:i] + [x] + good[i + 1 :])
    for c in bad_commons:
        assert lift(c) == MD_ERR_INVALID_ARG and count(c) == MD_ERR_INVALID_ARG and fill(c) == MD_ERR_INVALID_ARG, c
    assert lift(good, out=None) == MD_ERR_INVALID_ARG
    assert lift(good, q0=1, nq=3) == MD_ERR_INVALID_ARG and lift(good, nq=0) == MD_ERR_INVALID_ARG and lift(good, q0=-1) == MD_ERR_INVALID_ARG
    assert count(good, d=None) == MD_ERR_INVALID_ARG and count(good, r=None) == MD_ERR_INVALID_ARG
    assert count(good, w=None) == MD_ERR_INVALID_ARG and count(good, wb=ws_bytes - 1) == MD_ERR_INVALID_ARG
    assert fill(good, cap=-1) == MD_ERR_INVALID_ARG and fill(good, wb=ws_bytes - 1) == MD_ERR_INVALID_ARG
    assert lib.md_automaton_workspace_bytes(0, 10) == 0 and lib.md_automaton_workspace_bytes(3, 0) == 0
    torch.cuda.synchronize()
    for t in (nxt, default, row_ptr, tok, edge):
        assert bool((t == POISON).all()), "a refused call wrote"
