"""Stop strings and stop ids on the host (moondream_amd/stop.py): the packed Aho-Corasick table walked by ``stop.walk``
against the naive definition of tests/stop_ref.py, the argument checks and their messages, the table's sharing and
capacities, the settings record, and how a row's ids, ``Finish`` and text are cut.  No GPU."""
import re

import numpy as np
import pytest

from moondream_amd import stop
from moondream_amd.constraint import pow2_at_least
from moondream_amd.settings import CallSettings, refuse_settings
from moondream_amd.stop import Finish, StopSet, check_stops, pack, walk
from stop_ref import named_cases, stop_ref


def run_walk(strings, ids, vocab, tokens, split=None, others=()):
    """``walk`` over the table of [others..., StopSet(strings, ids)], optionally in two calls that share the row's words."""
    s = StopSet(strings, ids)
    table = pack(list(others) + [s])
    start = table.starts[-1]
    data = [vocab[t] for t in tokens]
    if split is None:
        return walk(table, start, data, tokens, ids, len(strings))
    words = {}
    walk(table, start, data[:split], tokens[:split], ids, len(strings), state=words)
    return walk(table, start, data[split:], tokens[split:], ids, len(strings), state=words)


@pytest.mark.parametrize("case", named_cases(), ids=lambda c: c[0])
def test_named_cases(case):
    _, vocab, tokens, strings, ids = case
    want = stop_ref([vocab[t] for t in tokens], [s.encode() for s in strings], tokens, ids)
    assert run_walk(strings, ids, vocab, tokens) == want
    other = StopSet(("zq", "hello w"), (1,))
    for split in range(len(tokens) + 1):  # the row's words carry the walk across any launch boundary
        assert run_walk(strings, ids, vocab, tokens, split, [other]) == want


def test_named_cases_say_what_they_claim():
    cases = {c[0]: c for c in named_cases()}
    ref = lambda c: stop_ref([c[1][t] for t in c[2]], [s.encode() for s in c[3]], c[2], c[4])
    assert ref(cases["spans three tokens"]) == (3, 5, 0)
    assert ref(cases["ends in mid-token"]) == (1, 1, 0)
    assert ref(cases["two matches in one token: the earlier end"]) == (1, 2, 1)  # "ab" ends at byte 4, "bab" at byte 5
    assert ref(cases["ab and xab end at the same byte: the longer"]) == (1, 2, 1)
    assert ref(cases["ab and xab across tokens"]) == (1, 0, 1)
    assert ref(cases["a proper prefix of another"]) == (1, 2, 0)
    assert ref(cases["a stop id whose bytes would complete a string"]) == (1, 1, 1)
    assert ref(cases["zero-byte tokens between the halves"]) == (3, 0, 0)
    assert ref(cases["multi-byte UTF-8 split across tokens"]) == (2, 2, 0)
    assert ref(cases["no match"]) == (-1, 0, -1)
    assert ref(cases["ids alone"]) == (2, 9, 1)


@pytest.mark.parametrize("seed", range(12))
def test_random_vocabularies_against_the_naive_definition(seed):
    rng = np.random.default_rng(seed)
    n_vocab = int(rng.integers(64, 301))
    alphabet = bytes(rng.integers(33, 127, size=int(rng.integers(2, 6))).tolist())  # few symbols: matches and overlaps abound
    vocab = [bytes(alphabet[i] for i in rng.integers(0, len(alphabet), size=int(rng.integers(0, 13)))) for _ in range(n_vocab)]
    vocab[0], vocab[1] = b"", alphabet[:1]
    tokens = rng.integers(0, n_vocab, size=40).tolist()
    text = b"".join(vocab[t] for t in tokens)
    strings = []
    for _ in range(int(rng.integers(1, 17))):  # drawn from the stream itself, so that they do occur
        n = int(rng.integers(1, 65))
        a = int(rng.integers(len(text) // 3, max(len(text) // 3 + 1, len(text) - n)))
        strings.append(text[a : a + n])
    strings = [s for s in strings if s]
    ids = rng.integers(0, n_vocab, size=int(rng.integers(0, 3))).tolist()
    assert pack([]).n_states == 0  # (an empty table packs)
    table = pack([StopSet([s.decode("ascii") for s in strings], ids)])
    want = stop_ref([vocab[t] for t in tokens], strings, tokens, ids)
    assert walk(table, 0, [vocab[t] for t in tokens], tokens, ids, len(strings)) == want
    assert want[0] >= 0
    # other tokenisations of the same text: the same bytes in front of the same string
    for _ in range(3):
        cuts = sorted(set(rng.integers(0, len(text) + 1, size=int(rng.integers(1, 30))).tolist()) | {0, len(text)})
        pieces = [text[a:b] for a, b in zip(cuts, cuts[1:])]
        at, keep, which = walk(table, 0, pieces, None, (), len(strings))
        w_at, w_keep, w_which = stop_ref(pieces, strings)
        assert (at, keep, which) == (w_at, w_keep, w_which)
        if not ids or want[2] < len(strings):
            assert (keep, which) == want[1:]


def test_dfa_is_complete_and_names_the_longest_suffix():
    trans, match_len, match_id = StopSet(("ab", "xab", "b")).dfa()
    assert trans.dtype == np.uint16 and trans.shape == (trans.shape[0], 256) and trans.max() < trans.shape[0]
    assert match_len.dtype == np.uint16 and match_id.dtype == np.int32
    q = 0
    for c in b"xab":
        q = trans[q, c]
    assert (match_len[q], match_id[q]) == (3, 1)
    q = trans[trans[0, ord("a")], ord("b")]
    assert (match_len[q], match_id[q]) == (2, 0)
    assert (match_len[0], match_id[0]) == (0, -1)
    assert StopSet((), (3,)).dfa()[0].shape == (1, 256)


@pytest.mark.parametrize("args, message", [
    (dict(stop=""), "stop: an empty stop string"),
    (dict(stop=["ok", ""]), "stop: an empty stop string"),
    (dict(stop="é" * 33), "66 bytes as UTF-8; at most 64"),
    (dict(stop=["a%d" % i for i in range(17)]), "stop: 17 strings; at most 16 per request"),
    (dict(stop=[b"bytes"]), "a stop string must be a str, not b'bytes'"),
    (dict(stop=5), "stop must be a str or a list of str"),
    (dict(stop=[None, "a", "b"]), "stop: 3 entries for 2 rows"),
    (dict(stop=[["a"], [3]]), "a stop string must be a str, not 3"),
    (dict(stop_token_ids=[1.5]), "a stop id must be an int, not 1.5"),
    (dict(stop_token_ids=[True]), "a stop id must be an int, not True"),
    (dict(stop_token_ids=[100]), "id 100 is outside the vocabulary [0, 100)"),
    (dict(stop_token_ids=[-1]), "id -1 is outside the vocabulary [0, 100)"),
    (dict(stop_token_ids=list(range(17))), "stop_token_ids: 17 ids; at most 16 per request"),
    (dict(stop_token_ids=[[1], [2], [3]]), "stop_token_ids: 3 entries for 2 rows"),
    (dict(stop_token_ids=7), "stop_token_ids must be a list of token ids"),
])
def test_check_stops_errors(args, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        check_stops(args.get("stop"), args.get("stop_token_ids"), 2, 100)


def test_check_stops_refuses_too_many_states():
    rows = [["%02d" % r + chr(97 + k) * 60 for k in range(16)] for r in range(6)]  # 6 x 16 x 62 bytes, hardly shared
    with pytest.raises(ValueError, match=r"need \d+ states; at most 4096"):
        check_stops(rows, None, 6, 100)
    assert check_stops(rows[:2] + [None] * 4, None, 6, 100) is not None


def test_check_stops_forms():
    assert check_stops(None, None, 3, 10) is None
    assert check_stops([None, None, None], [None, None, None], 3, 10) is None
    a = check_stops("\n\n", None, 2, 10)
    assert a == [StopSet(("\n\n",)), StopSet(("\n\n",))] and a[0] is a[1]
    assert check_stops(["a", "b"], None, 2, 10) == [StopSet(("a", "b"))] * 2  # a list of str alone is call-wide
    rows = check_stops([None, "a", ["b", "c"]], [[1], None, [2, 3]], 3, 10)
    assert rows == [StopSet((), (1,)), StopSet(("a",)), StopSet(("b", "c"), (2, 3))]
    assert check_stops(None, [4, 5], 2, 10) == [StopSet((), (4, 5))] * 2
    assert check_stops([None, "a"], None, 2, 10) == [None, StopSet(("a",))]
    assert stop.MD_STOP_STATES_MAX == 4096


def test_pack_shares_equal_stop_sets_and_rebases():
    a, b, c = StopSet(("ab", "c")), StopSet(("ab", "c"), (7,)), StopSet(("xyz",))
    t = pack([a, b, c, a])
    n_a, n_c = a.dfa()[0].shape[0], c.dfa()[0].shape[0]
    assert t.starts == (0, 0, n_a, 0) and t.n_states == n_a + n_c
    assert t.trans[n_a:].min() >= n_a  # the second automaton's transitions stay inside it
    assert walk(t, n_a, [b"abxy", b"z"]) == (1, 2, 0) and walk(t, 0, [b"xyzab"]) == (0, 3, 0)
    later = pack([c], state0=t.n_states)
    assert later.starts == (t.n_states,) and later.trans.min() >= t.n_states


def test_capacities_are_powers_of_two():
    for strings in (("a",), ("abcdefghijklmnopq",), tuple("s%02d" % i + "x" * 40 for i in range(16))):
        t = pack([StopSet(strings)])
        trans, match_len, match_id, cap = stop.padded(t)
        assert cap == pow2_at_least(t.n_states) and cap & (cap - 1) == 0 and cap >= 16
        assert trans.shape == (cap, 256) and match_len.shape == (cap,) and match_id.shape == (cap,)
        assert not match_len[t.n_states :].any() and (match_id[t.n_states :] == -1).all()
    assert stop.padded(pack([StopSet(("a",))]))[3] == stop.padded(pack([StopSet(("bcd", "ef"))]))[3]  # the same graphs


def test_call_settings_carry_and_reorder_stops():
    free = lambda c, n: None
    st = CallSettings.of(3, free, stop=[None, "a", ["b", "c"]], stop_token_ids=[[1], None, None], include_stop_str_in_output=True,
                         vocab_bytes=[b"x"] * 10, vocab_size=10)
    assert [r.stop for r in st.rows] == [StopSet((), (1,)), StopSet(("a",)), StopSet(("b", "c"))]
    assert st.include_stop_str is True and st.stop_vocab_bytes == [b"x"] * 10
    back = st.reorder([2, 0, 1])
    assert back.stops == [StopSet(("b", "c")), StopSet((), (1,)), StopSet(("a",))]
    assert back.include_stop_str is True and back.stop_vocab_bytes is st.stop_vocab_bytes
    plain = CallSettings.of(2, free)
    assert plain.stops is None and plain.include_stop_str is False and all(r.stop is None for r in plain.rows)
    assert CallSettings.of_settings({"stop": "\n", "temperature": 0}, 2, free, vocab_size=10).stops == [StopSet(("\n",))] * 2
    with pytest.raises(ValueError, match="id 10 is outside the vocabulary"):
        CallSettings.of(1, free, stop_token_ids=[10], vocab_size=10)
    with pytest.raises(ValueError, match="include_stop_str_in_output must be a bool"):
        CallSettings.of(1, free, stop="a", include_stop_str_in_output=1)
    with pytest.raises(ValueError, match="not served by beam search"):
        CallSettings.of_settings({"stop": "a", "num_beams": 2}, 1, free)


def test_refuse_stops():
    for settings in ({"stop": "a"}, {"stop": ["a"]}, {"stop_token_ids": [3]}, {"stop": [None, "a"]}):
        with pytest.raises(ValueError, match="stop / stop_token_ids are not served by the place"):
            stop.refuse_stops(settings, "the place")
        with pytest.raises(ValueError, match="not served by the place"):
            refuse_settings(settings, "the place", ("penalties", "stops"))
    for settings in (None, {}, {"stop": None}, {"stop": [None, None]}, {"stop_token_ids": []}, {"include_stop_str_in_output": True}):
        stop.refuse_stops(settings, "the place")


def test_finish_and_text_cut():
    s = StopSet(("lo w", "!"), (9,))
    eos = 0
    # a string completed in token 2: the token stays, the text ends in front of the string (or behind it)
    assert stop.finish_of(s, 2, 3, 0, 8, False, None) == (3, Finish("stop", "lo w", 3))
    assert stop.finish_of(s, 2, 3, 0, 8, True, None) == (3, Finish("stop", "lo w", 7))
    assert stop.cut_text([b"hel", b"lo", b" wor"], Finish("stop", "lo w", 3)) == b"hel"
    assert stop.cut_text([b"hel", b"lo", b" wor"], Finish("stop", "lo w", 7)) == b"hello w"
    # a stop id: excluded like eos, no text cut
    assert stop.finish_of(s, 4, 11, 2, 8, False, None) == (4, Finish("stop", 9, None))
    # the earliest of eos and the match; a match in the eos token itself or later is no match
    assert stop.finish_of(s, 5, 3, 1, 8, False, 2) == (2, Finish("eos"))
    assert stop.finish_of(s, 2, 3, 1, 8, False, 2) == (2, Finish("eos"))
    assert stop.finish_of(s, 1, 3, 1, 8, False, 2) == (2, Finish("stop", "!", 3))
    # a match beyond the token budget is none
    assert stop.finish_of(s, 8, 3, 1, 8, False, None) == (8, Finish("length"))
    assert stop.finish_of(None, -1, 0, -1, 8, False, None) == (8, Finish("length"))
    assert stop.finish_of(None, -1, 0, -1, 8, False, 8) == (8, Finish("length"))
    assert stop.cut_text([b"ab", b"c"], Finish("eos")) == b"abc"
    assert eos == 0


def test_scheduler_retires_at_a_match_and_refills_the_slot():
    """A ``SlotScheduler`` driven with numpy arrays: one slot, two requests.  The first matches a stop string in the third
    generated token (the prefill's is token 0): it retires there with the token included, its slot returns to the pool,
    the second request is admitted into it and ends on a stop id, excluded."""
    from moondream_amd.continuous import Request, SlotScheduler
    from moondream_amd.settings import RowSettings

    sched = SlotScheduler(max_live=1, max_context=64, chunk=4)
    a = Request(0, None, [1], 10, None, settings=RowSettings(stop=StopSet(("ab", "xyz"))), include_stop_str=True)
    b = Request(1, None, [1], 10, None, settings=RowSettings(stop=StopSet(("q",), (42,))))
    c = Request(2, None, [1], 3, 99, settings=RowSettings(stop=StopSet(("q",))))
    for r in (a, b, c):
        sched.submit(r)
    admitted, chunks = [], []
    stream = {0: [11, 12, 13, 14], 1: [21, 42, 23, 24], 2: [31, 99, 33, 34]}
    hits = {0: (2, 5, 1), 1: (2, 7, 1), 2: (-1, 0, -1)}

    def admit(reqs):
        admitted.append([(r.rid, r.slot) for r in reqs])
        for r in reqs:
            r.stop_hit = (-1, 0, -1)
        return [(10 * (r.rid + 1), 5) for r in reqs]

    def step(plan):
        chunks.append([r.rid for r in plan.rows])
        out = np.zeros((plan.n, plan.bucket), dtype=np.int32)
        trip = np.zeros((3, plan.bucket), dtype=np.int64)
        for i, r in enumerate(plan.rows):
            out[:, i] = stream[r.rid][: plan.n]
            trip[:, i] = hits[r.rid]
        return out, {"stop": tuple(trip)}

    done = list(sched.run(admit, step))
    assert [r.rid for r in done] == [0, 1, 2]
    assert a.ids == [10, 11, 12] and a.finish == Finish("stop", "xyz", 5 + 3) and a.slot == -1
    assert b.ids == [20, 21] and b.finish == Finish("stop", 42, None)
    assert c.ids == [30, 31] and c.finish == Finish("eos")
    assert admitted == [[(0, 0)], [(1, 0)], [(2, 0)]] and chunks == [[0], [1], [2]]  # the one slot, refilled after each match
    assert sched.stats.decode_steps == 4 + 4 + 2 and list(sched.free) == [0]
    # a match in the prefill's own token retires the request at its start; a budget that runs out is "length"
    d = Request(3, None, [1], 10, None, settings=RowSettings(stop=StopSet((), (7,))))
    d.slot, d.stop_hit = sched.free.popleft(), (0, 0, 0)
    assert sched.start(d, 7, 5) and d.ids == [] and d.finish == Finish("stop", 7, None) and list(sched.free) == [0]
    e = Request(4, None, [1], 1, None)
    e.slot = sched.free.popleft()
    assert sched.start(e, 7, 5) and e.ids == [7] and e.finish == Finish("length")


def test_engine_stop_table_is_checked_on_the_host():
    from moondream_amd.continuous import ContinuousEngine

    class Cfg:
        class text:
            max_context, vocab_size = 64, 100

    class Model:
        config = Cfg

    eng = ContinuousEngine(Model(), max_live=2, stop_states=16)
    assert eng._register_stop(StopSet(("abc",))) == 0 and eng._register_stop(StopSet(("abc",), (5,))) == 0
    assert eng._register_stop(StopSet((), (5,))) == 4 and eng._stop_used == 5
    with pytest.raises(ValueError, match=re.escape("the engine's stop table is full: 5 + 13 states of 16 (ContinuousEngine(stop_states=))")):
        eng._register_stop(StopSet(("0123456789ab",)))
    with pytest.raises(ValueError, match="stop_states must be in 1 .. 4096"):
        ContinuousEngine(Model(), stop_states=0)
