"""md_stop_rows on the MI355X through the C ABI against tests/stop_ref.py: EXACT equality (integers) of every row's result
triple and counters, launch after launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from moondream_amd import _lib, grammar
from moondream_amd.stop import StopSet, pack, padded, walk
from stop_ref import named_cases, stop_ref

pytestmark = pytest.mark.gpu
POISON = -77  # the words of a row that must not be touched


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Rows:
    """The device state of ``n`` slots over one packed table and one vocabulary; ``sets[s]``: slot s's StopSet or None."""

    def __init__(self, lib, vocab, sets, table_sets=None):
        self.lib, self.vocab, self.sets = lib, vocab, sets
        distinct = list(dict.fromkeys(table_sets if table_sets is not None else [s for s in sets if s is not None]))
        table = pack(distinct)
        start = dict(zip(distinct, table.starts))
        trans, match_len, match_id, self.cap = padded(table)
        n = len(sets)
        off, data = grammar.vocab_arrays(vocab)
        self.n_bytes = int(off[-1])
        self.d_trans, self.d_len, self.d_mid = dev(trans.view(np.int16)), dev(match_len.view(np.int16)), dev(match_id)
        self.d_off, self.d_bytes = dev(off), dev(data.copy())
        ptr = np.zeros(n + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([len(s.token_ids) if s is not None else 0 for s in sets])
        ids = np.array([t for s in sets if s is not None for t in s.token_ids] + [-1], dtype=np.int32)
        self.d_ptr, self.d_ids = dev(ptr), dev(ids)
        self.d_base = dev(np.array([len(s.strings) if s is not None else 0 for s in sets], dtype=np.int32))
        words = np.zeros((6, n), dtype=np.int32)
        words[0] = [start[s] if s is not None else -1 for s in sets]
        words[3], words[5] = -1, -1
        for s, st in enumerate(sets):
            if st is None:
                words[1:, s] = POISON
        self.d_words = dev(words)

    def launch(self, tokens, slots=None, slot0=0):
        d_tok = dev(np.asarray(tokens, dtype=np.int32))
        d_slots = dev(np.asarray(slots, dtype=np.int32)) if slots is not None else None
        st = self.lib.md_stop_rows(d_tok.data_ptr(), len(tokens), d_slots.data_ptr() if d_slots is not None else None, slot0,
                                   self.d_trans.data_ptr(), self.d_len.data_ptr(), self.d_mid.data_ptr(), self.cap,
                                   self.d_ptr.data_ptr(), self.d_ids.data_ptr(), self.d_base.data_ptr(), self.d_off.data_ptr(),
                                   self.d_bytes.data_ptr(), len(self.vocab), self.n_bytes,
                                   *(self.d_words[i].data_ptr() for i in range(6)),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st
        torch.cuda.synchronize()
        return self.d_words.cpu().numpy()

    def expect(self, s, fed):
        """What slot s's words (n_tok, n_bytes, at, keep, which) must be after the tokens ``fed``."""
        st = self.sets[s]
        if st is None:
            return [POISON] * 5
        data = [self.vocab[t] if 0 <= t < len(self.vocab) else b"" for t in fed]
        at, keep, which = stop_ref(data, [x.encode() for x in st.strings], fed, st.token_ids)
        return [len(fed), sum(len(d) for d in data), at, keep, which]


@pytest.mark.parametrize("b", [1, 3, 65])
def test_named_cases_in_5_plus_7_launches(lib, b):
    """Every named case as one row (repeated to ``b`` rows), fed twelve tokens in launches of 5 + 7 steps -- the state is
    carried across the boundary -- and checked after EVERY launch: before the match, at it, and after it, where only the
    counters move."""
    for name, vocab, tokens, strings, ids in named_cases():
        toks = (tokens + [1, 0, 2, 6, 9, 1, 2, 14, 0, 5, 18, 1])[:12]  # twelve steps; the tail runs past every match
        rows = Rows(lib, vocab, [StopSet(strings, ids)] * b)
        for step in range(12):
            words = rows.launch([toks[step]] * b)
            want = rows.expect(0, toks[: step + 1])
            for r in {0, b // 2, b - 1}:
                assert words[1:, r].tolist() == want, (name, step, r)
        assert (words[3] >= 0).all() == (want[2] >= 0)
        # the state word too is ``walk``'s: the state of the match for a matched row, the state reached otherwise
        carried = {}
        table = pack([StopSet(strings, ids)])
        walk(table, 0, [vocab[t] for t in toks], toks, ids, len(strings), state=carried)
        assert words[0].tolist() == [carried["state"]] * b, name


def test_mixed_rows_by_slot(lib):
    """Three stop sets in one table plus rows with none, 65 rows, a slot table that permutes them with an idle row of
    slot -1; tokens of 0, 1 and 48 bytes; seeded random streams; 5 + 7 steps."""
    rng = np.random.default_rng(5)
    vocab = [b"", b"a", b"x" * 48] + [bytes(rng.integers(97, 100, size=int(rng.integers(1, 9))).tolist()) for _ in range(60)]
    kinds = [StopSet(("ab", "cab", "bcc")), StopSet(("xxxa", "ca"), (7, 9)), StopSet((), (11, 2)), None]
    n = 66  # slots; slot n - 1 is used by no row
    sets = [kinds[int(k)] for k in rng.integers(0, 4, size=n)]
    sets[0], sets[1], sets[2], sets[3] = kinds[0], kinds[1], kinds[2], None
    rows = Rows(lib, vocab, sets)
    b = 65
    fed = [[] for _ in range(n)]
    for step in range(12):
        slots = rng.permutation(n - 1)[:b].astype(np.int32)  # a request changes row from launch to launch, not slot
        slots[int(rng.integers(0, b))] = -1                   # one idle row
        tokens = rng.integers(0, len(vocab), size=b)
        tokens[: b // 4] = rng.integers(0, 3, size=b // 4)    # the 0-, 1- and 48-byte tokens
        before = rows.d_words.cpu().numpy()
        words = rows.launch(tokens.tolist(), slots.tolist())
        for r, s in enumerate(slots.tolist()):
            if s >= 0:
                fed[s].append(int(tokens[r]))
        for s in range(n):
            assert words[1:, s].tolist() == rows.expect(s, fed[s]), (step, s)
        unused = sorted(set(range(n)) - set(slots.tolist()))
        assert (words[:, unused] == before[:, unused]).all()  # idle rows and unused slots: nothing written, the state included
        no_set = [s for s in range(n) if sets[s] is None]
        assert (words[:, no_set] == before[:, no_set]).all()
    matched = sum(1 for s in range(n) if sets[s] is not None and rows.expect(s, fed[s])[2] >= 0)
    assert matched > 10  # the streams do hit their stop sets


def test_slot0_and_argument_checks(lib):
    vocab = [b"", b"a", b"b"]
    rows = Rows(lib, vocab, [None, StopSet(("ab",)), StopSet(("b",))])
    words = rows.launch([1, 2], slot0=1)  # rows 0, 1 -> slots 1, 2
    assert words[1:, 1].tolist() == [1, 1, -1, 0, -1] and words[1:, 2].tolist() == [1, 1, 0, 0, 0]
    assert words[1:, 0].tolist() == [POISON] * 5
    good = dict(tokens=rows.d_ids.data_ptr(), batch=1, slots=None, slot0=0, trans=rows.d_trans.data_ptr(),
                match_len=rows.d_len.data_ptr(), match_id=rows.d_mid.data_ptr(), state_cap=rows.cap, id_ptr=rows.d_ptr.data_ptr(),
                ids=rows.d_ids.data_ptr(), id_base=rows.d_base.data_ptr(), tok_off=rows.d_off.data_ptr(),
                tok_bytes=rows.d_bytes.data_ptr(), vocab=3, n_bytes=rows.n_bytes,
                **{k: rows.d_words[i].data_ptr() for i, k in enumerate(("state", "n_tok", "n_seen", "at", "keep", "which"))})
    call = lambda **kw: lib.md_stop_rows(*{**good, **kw}.values(), None)
    assert call(batch=0) == 0
    for bad in (dict(tokens=None), dict(trans=None), dict(at=None), dict(batch=-1), dict(state_cap=0), dict(state_cap=4097),
                dict(tok_off=None), dict(vocab=0), dict(n_bytes=-1)):
        assert call(**bad) == 1, bad


def test_ids_alone_need_no_vocabulary(lib):
    rows = Rows(lib, [b"a"], [StopSet((), (5, 3))])
    rows.d_off = rows.d_bytes = torch.zeros(0)  # (data_ptr() of an empty tensor is 0: NULL)
    assert rows.d_off.data_ptr() == 0
    out = [rows.launch([t])[1:, 0].tolist() for t in (7, 3, 5)]
    assert out == [[1, 0, -1, 0, -1], [2, 0, 1, 0, 1], [3, 0, 1, 0, 1]]
