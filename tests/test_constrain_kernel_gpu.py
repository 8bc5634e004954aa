"""md_constrain_rows on the MI355X through the C ABI against tests/constraint_ref.py: EXACT equality of the bf16 bits of
the whole logits array (padding columns included) and of the whole state array, after every launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from constraint_ref import DEAD, FORBID, FREE, constrain_rows
from moondream_amd import _lib
from moondream_amd.constraint import TokenAutomaton, pack

pytestmark = pytest.mark.gpu
SHAPES = [(51200, 51200), (1000, 1003)]  # (vocab, ld): rows 16-byte aligned, and rows at every 2-byte offset
NAN_BITS = 0x7FC0      # padding columns
POISON = 0x4B4B        # a finite bf16: rows that must not be written
NEG_INF = np.int16(-128)  # 0xFF80
MD_ERR_INVALID_ARG = 1  # include/moondream_hip.h


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_logits(rows, vocab, ld, seed, poison=()):
    gen = torch.Generator().manual_seed(seed)
    x = torch.full((rows, ld), NAN_BITS, dtype=torch.int16)
    x[:, :vocab] = (torch.randn(rows, vocab, generator=gen) * 8.0).to(torch.bfloat16).view(torch.int16)
    x = x.numpy().copy()
    for r in poison:
        x[r, :] = np.int16(POISON)
    return x


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def call(lib, d_lg, vocab, d_tok, d_slots, slot0, d_state, d_table, state_cap, batch=None):
    ptr = lambda t: t.data_ptr() if t is not None else None
    return lib.md_constrain_rows(d_lg.data_ptr(), d_lg.stride(0), d_lg.shape[0] if batch is None else batch, vocab, ptr(d_tok),
                                 ptr(d_slots), slot0, d_state.data_ptr(), *(t.data_ptr() for t in d_table), state_cap, stream())


def launch(lib, logits, vocab, tokens_in, slots, slot0, state, table, state_cap=None):
    """One launch on copies of the arguments; returns (logits bits, state) as numpy, compared with the reference."""
    arrays = (table.row_ptr, table.default_next, np.append(table.edge_tok, 0).astype(np.int32),
              np.append(table.edge_next, 0).astype(np.int32))  # (one spare edge: an empty table is still an allocation)
    state_cap = table.n_states if state_cap is None else state_cap
    state = np.asarray(state, dtype=np.int32)
    d_lg, d_state = dev(logits), dev(state)
    d_tok = dev(np.asarray(tokens_in, dtype=np.int32)) if tokens_in is not None else None
    d_slots = dev(np.asarray(slots, dtype=np.int32)) if slots is not None else None
    st = call(lib, d_lg, vocab, d_tok, d_slots, slot0, d_state, [dev(a) for a in arrays], state_cap)
    assert st == 0, st
    torch.cuda.synchronize()
    got = d_lg.cpu().numpy(), d_state.cpu().numpy()
    want = constrain_rows(logits, vocab, tokens_in, slots, slot0, state, *arrays, state_cap)
    for name, g, w in zip(("logits", "state"), got, want):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (name, len(bad), bad[:8].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    return got


def long_edges(vocab, n=3000):
    """``n`` distinct tokens spread over the vocabulary (all of it where it has fewer), the first and the last included."""
    n = min(n, vocab)
    toks = sorted(set(np.linspace(0, vocab - 1, n).astype(int).tolist()))
    assert len(toks) == n and n > 256
    return toks


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_default_forbid_states(lib, vocab, ld):
    """The bitmap sweep, nothing consumed (tokens_in NULL): a state allowing exactly one token, one allowing only token 0
    and vocab - 1, one allowing 8 neighbours that straddle a word of the bit map, and one with an edge list longer than a
    workgroup (3000 entries at the large vocabulary, every token of the small one) whose every third edge is FORBID."""
    mid = vocab // 2 + 3
    toks = long_edges(vocab)
    a = TokenAutomaton.from_states([
        ({mid: 0}, FORBID),
        ({0: 1, vocab - 1: FREE}, FORBID),
        ({v: 2 for v in range(27, 35)}, FORBID),
        ({v: (FORBID if i % 3 == 0 else 3) for i, v in enumerate(toks)}, FORBID),
    ])
    lg = make_logits(4, vocab, ld, seed=vocab)
    got, state = launch(lib, lg, vocab, None, None, 0, [0, 1, 2, 3], pack([a]))
    assert state.tolist() == [0, 1, 2, 3]
    assert np.flatnonzero(got[0, :vocab] != NEG_INF).tolist() == [mid] and got[0, mid] == lg[0, mid]
    assert np.flatnonzero(got[1, :vocab] != NEG_INF).tolist() == [0, vocab - 1]
    assert np.flatnonzero(got[2, :vocab] != NEG_INF).tolist() == list(range(27, 35))
    assert np.flatnonzero(got[3, :vocab] != NEG_INF).tolist() == [v for i, v in enumerate(toks) if i % 3]
    assert (got[:, vocab:] == np.int16(NAN_BITS)).all()


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_default_allow_states(lib, vocab, ld):
    """One forbidden token; no edges at all (the row is not written: it holds the poison); the long edge list."""
    toks = long_edges(vocab)
    a = TokenAutomaton.from_states([
        ({vocab - 1: FORBID}, 0),
        ({}, 1),
        ({v: (FORBID if i % 3 == 0 else 2) for i, v in enumerate(toks)}, FREE),
    ])
    lg = make_logits(3, vocab, ld, seed=vocab + 1, poison=[1])
    got, _ = launch(lib, lg, vocab, None, None, 0, [0, 1, 2], pack([a]))
    assert np.flatnonzero(got[0] != lg[0]).tolist() == [vocab - 1] and got[0, vocab - 1] == NEG_INF
    assert (got[1] == np.int16(POISON)).all()
    assert np.flatnonzero(got[2] != lg[2]).tolist() == [v for i, v in enumerate(toks) if i % 3 == 0 and lg[2, v] != NEG_INF]


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_advance(lib, vocab, ld):
    """Eight rows leave state 0 by: its first listed edge, its last, the default, a FORBID edge (DEAD), t = -1 (DEAD),
    t = vocab (DEAD), an edge to FREE, and -- tokens_in given -- an edge among 3000 (the binary search's depth).  The
    dead and the free rows hold the poison: their logits are not written."""
    toks = long_edges(vocab)
    first, last, forbid, free, deep = toks[0], toks[-1], toks[1], toks[2], toks[len(toks) * 2 // 3]
    edges = {v: 4 for v in toks}
    edges.update({first: 1, last: 2, forbid: FORBID, free: FREE, deep: 3})
    default_tok = next(v for v in range(vocab) if v not in edges) if len(toks) < vocab else None
    a = TokenAutomaton.from_states([
        (edges, 5),
        ({7: 1}, FORBID),           # 1: default-forbid
        ({9: FORBID}, 2),           # 2: default-allow
        ({0: 3, vocab - 1: 3}, FORBID),
        ({}, 4),
        ({11: FORBID, 12: FORBID}, 5),
    ])
    tokens = [first, last, default_tok if default_tok is not None else first, forbid, -1, vocab, free, deep]
    lg = make_logits(8, vocab, ld, seed=vocab + 2, poison=[3, 4, 5, 6])
    got, state = launch(lib, lg, vocab, tokens, None, 0, [0] * 8, pack([a]))
    assert state.tolist() == [1, 2, 5 if default_tok is not None else 1, DEAD, DEAD, DEAD, FREE, 3]
    assert (got[3:7] == np.int16(POISON)).all()
    assert np.flatnonzero(got[0, :vocab] != NEG_INF).tolist() == [7] and got[1, 9] == NEG_INF


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_rows_left_alone_and_slot_routing(lib, vocab, ld):
    """slots as a permutation with an idle row; a FREE and a DEAD row (unwritten, state kept); a state >= state_cap
    (DEAD, unwritten); then the same table with contiguous slots from slot0 = 2."""
    a = TokenAutomaton.from_states([({5: 1}, FORBID), ({6: FORBID}, 0)])
    table = pack([a])
    lg = make_logits(6, vocab, ld, seed=7, poison=[1, 2, 3, 4])
    #        row:   0   1(idle) 2(FREE) 3(DEAD) 4(>= cap) 5
    slots = [4, -1, 0, 5, 2, 1]
    state = [FREE, 1, 2, 777, 0, DEAD]  # by slot: 0 FREE, 1 -> row 5, 2 -> row 4, 3 unused, 4 -> row 0, 5 DEAD
    got, st = launch(lib, lg, vocab, [5, 5, 5, 5, 5, 100], slots, 0, state, table)
    assert st.tolist() == [FREE, 0, DEAD, 777, 1, DEAD]
    assert (got[1:5] == np.int16(POISON)).all()
    assert got[0, 6] == NEG_INF and np.flatnonzero(got[5, :vocab] != NEG_INF).tolist() == [5]
    lg = make_logits(2, vocab, ld, seed=8)
    got, st = launch(lib, lg, vocab, None, None, 2, [9, 9, 0, 1, 9], table)
    assert st.tolist() == [9, 9, 0, 1, 9] and np.flatnonzero(got[0, :vocab] != NEG_INF).tolist() == [5] and got[1, 6] == NEG_INF


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_two_automata_in_one_table(lib, vocab, ld):
    """Rebased state ids: two rows in different automata of one packed table, over two consecutive launches."""
    a = TokenAutomaton.sequence([3, vocab - 1, 4])
    b = TokenAutomaton.min_tokens(2, 9)
    table = pack([a, b])
    assert table.starts == (0, 3)
    state = np.asarray(table.starts, dtype=np.int32)
    lg = make_logits(2, vocab, ld, seed=9)
    _, state = launch(lib, lg, vocab, None, None, 0, state, table)
    got, state = launch(lib, make_logits(2, vocab, ld, seed=10), vocab, [3, 100], None, 0, state, table)
    assert state.tolist() == [1, 4]
    assert np.flatnonzero(got[0, :vocab] != NEG_INF).tolist() == [vocab - 1] and got[1, 9] == NEG_INF
    _, state = launch(lib, make_logits(2, vocab, ld, seed=11), vocab, [vocab - 1, 100], None, 0, state, table)
    assert state.tolist() == [2, FREE]
    _, state = launch(lib, make_logits(2, vocab, ld, seed=12), vocab, [5, 100], None, 0, state, table)
    assert state.tolist() == [DEAD, FREE]


def test_captured_chunk_replays_over_rewritten_state_and_table(lib):
    """Two steps (advance and mask each) captured with torch.cuda.graph; the replay follows the state AND the table
    contents written at the same addresses afterwards: nothing of them is baked in but their addresses."""
    vocab, ld = 1000, 1003
    t1 = pack([TokenAutomaton.sequence([10, 20, 30]), TokenAutomaton.banned_tokens([1, 2])])
    t2 = pack([TokenAutomaton.banned_tokens([7]), TokenAutomaton.sequence([40, 50, 60])])
    assert t1.n_states == t2.n_states == 4 and t1.n_edges == 5 and t2.n_edges == 4
    arrays = lambda t: (t.row_ptr, t.default_next, np.resize(t.edge_tok, 5), np.resize(t.edge_next, 5))
    d_table = [dev(a) for a in arrays(t1)]
    lg0 = [make_logits(2, vocab, ld, seed=20 + i) for i in range(2)]
    d_lg = [dev(x) for x in lg0]
    d_tok = [dev(np.asarray(x, dtype=np.int32)) for x in ([10, 5], [20, 6])]
    d_state = dev(np.asarray([0, 3], dtype=np.int32))

    def body():
        for i in range(2):
            assert call(lib, d_lg[i], vocab, d_tok[i], None, 0, d_state, d_table, 4) == 0

    def expect(table, state, toks):
        out = []
        for i in range(2):
            lg, state = constrain_rows(lg0[i], vocab, toks[i], None, 0, state, *arrays(table), 4)
            out.append(lg)
        return out, state

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        body()  # warm-up
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        for t, x in zip(d_lg, lg0):
            t.copy_(torch.from_numpy(x))
        d_state.copy_(torch.tensor([0, 3], dtype=torch.int32))
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            body()
        graph.replay()
        s.synchronize()
        want, want_state = expect(t1, [0, 3], [[10, 5], [20, 6]])
        assert d_state.cpu().tolist() == want_state.tolist() == [2, 3]
        assert all((g.cpu().numpy() == w).all() for g, w in zip(d_lg, want))
        # the other table and other start states and tokens, at the same addresses
        for t, x in zip(d_table, arrays(t2)):
            t.copy_(torch.from_numpy(x))
        for t, x in zip(d_lg, lg0):
            t.copy_(torch.from_numpy(x))
        d_state.copy_(torch.tensor([1, 0], dtype=torch.int32))
        d_tok[0].copy_(torch.tensor([40, 3], dtype=torch.int32))
        d_tok[1].copy_(torch.tensor([50, 7], dtype=torch.int32))
        graph.replay()
        s.synchronize()
        want, want_state = expect(t2, [1, 0], [[40, 3], [50, 7]])
        assert d_state.cpu().tolist() == want_state.tolist() == [3, DEAD]
        assert all((g.cpu().numpy() == w).all() for g, w in zip(d_lg, want))


def test_batch_zero_and_error_codes(lib):
    lg = torch.zeros(2, 64, dtype=torch.bfloat16, device="cuda")
    tok = torch.zeros(2, dtype=torch.int32, device="cuda")
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    tab = torch.zeros(4, 4, dtype=torch.int32, device="cuda")
    good = dict(logits=lg.data_ptr(), ld=64, batch=2, vocab=64, tokens_in=tok.data_ptr(), slots=None, slot0=0,
                state=state.data_ptr(), row_ptr=tab[0].data_ptr(), default_next=tab[1].data_ptr(), edge_tok=tab[2].data_ptr(),
                edge_next=tab[3].data_ptr(), state_cap=1)
    run = lambda **kw: lib.md_constrain_rows(*{**good, **kw}.values(), stream())
    assert run() == 0 and run(batch=0) == 0 and run(tokens_in=None) == 0
    assert run(batch=0, logits=lg.data_ptr(), state_cap=1) == 0
    torch.cuda.synchronize()
    assert (lg == 0).all() and (state == 0).all()  # (the all-zero table: one default-allow state without edges)
    for name in ("logits", "state", "row_ptr", "default_next", "edge_tok", "edge_next"):
        assert run(**{name: None}) == MD_ERR_INVALID_ARG, name
    for bad in (dict(batch=-1), dict(vocab=0), dict(ld=63), dict(state_cap=0),
                dict(vocab=_lib.MD_CONSTRAIN_VOCAB_MAX + 1, ld=_lib.MD_CONSTRAIN_VOCAB_MAX + 1)):
        assert run(**bad) == MD_ERR_INVALID_ARG, bad
    torch.cuda.synchronize()
