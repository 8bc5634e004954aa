"""moondream_amd/grammar.py on the host: the regex subset against Python's ``re`` on sampled strings, trimming, every
refusal, JSON schemas against ``json.loads`` and a small checker, ``TokenAutomaton.from_arrays`` against the tuple form, and
tests/grammar_ref.py (the reference the GPU tests compare with) against brute force."""
import json
import re

import numpy as np
import pytest

import grammar_ref as ref
from moondream_amd.constraint import DEAD, FORBID, FREE, TokenAutomaton, grammar_of, pack, refuse_constraints
from moondream_amd.grammar import (MAX_STATES, ByteDFA, finish_automaton, gpt2_unicode_to_byte, json_schema_to_regex, prune_unreachable,
                                   regex_to_dfa, vocab_bytes_of)

PATTERNS = [
    r"(yes|no|maybe)",
    r"-?[0-9]{1,3}(\.[0-9]{1,2})?",
    r"a*b+c?",
    r".{2,4}",
    r"[a-f0-9]+",
    r"[^a-c\d]x",
    r"\w+\s\S*",
    r"\D\W\d",
    r"(?:ab|cd){2,}",
    r"x{,2}y{3}",
    r"a{2}b{1,}",
    r"[]a]+",
    r"[a\-z.]*q",
    r"\[\{\}\]\.\*\+\?\|\(\)\\",
    r"(a|)b",
    r"(a|b)*abb",
    r"\x41\t\n",
    r"(?:é|ü)+ß",
    r"[\w-]+@[\w.]+",
    r"(0|[1-9][0-9]*)(,(0|[1-9][0-9]*)){0,3}",
    r"\s*[+-]?\d+\s*",
]


def sample(dfa: ByteDFA, rng, n=120, longest=24):
    """Accepted strings by random walks that head for an accepting state once they are long enough."""
    s = dfa.n_states
    dist = np.full(s, 10**6)  # steps to the nearest accepting state
    dist[dfa.accept] = 0
    for _ in range(s):
        nxt = np.where(dfa.trans >= 0, dist[np.maximum(dfa.trans, 0)], 10**6).min(axis=1) + 1
        dist = np.minimum(dist, nxt)
    out = set()
    for _ in range(n):
        q, data = 0, bytearray()
        while True:
            if dfa.accept[q] and (len(data) >= longest or rng.random() < 0.3):
                break
            live = np.flatnonzero(dfa.trans[q] >= 0)
            if live.size == 0:
                break
            if len(data) >= longest:  # go home by the shortest way
                live = live[dist[dfa.trans[q, live]] == dist[dfa.trans[q, live]].min()]
            b = int(rng.choice(live))
            data.append(b)
            q = int(dfa.trans[q, b])
        assert dfa.accept[q]
        out.add(bytes(data))
    return sorted(out)


def mutations(positives, rng):
    out = set()
    for p in positives:
        if p:
            i = int(rng.integers(len(p)))
            out.add(p[:i] + bytes([int(rng.integers(256))]) + p[i + 1 :])
            out.add(p[:-1])
            out.add(p[: len(p) // 2])
        out.add(p + bytes([int(rng.integers(256))]))
        out.add(p + p[-1:] if p else b"\n")
    for _ in range(60):
        out.add(bytes(rng.integers(0, 256, size=int(rng.integers(0, 6))).astype(np.uint8)))
    return sorted(out)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_dfa_agrees_with_re(pattern):
    rng = np.random.default_rng(len(pattern) * 7919 + 1)
    dfa = regex_to_dfa(pattern)
    want = re.compile(pattern.encode())
    positives = sample(dfa, rng)
    assert positives, "no accepted string: the DFA accepts nothing"
    n_neg = 0
    for s in positives + mutations(positives, rng):
        ok = bool(want.fullmatch(s))
        assert dfa.accepts(s) == ok, (pattern, s)
        n_neg += not ok
    assert all(want.fullmatch(s) for s in positives) and n_neg > 0, "both classes are met"
    # trimmed: an accepting state is reachable from every state, and every state from the start
    assert _coreachable(dfa).all() and _reachable(dfa).all()
    # deterministic numbering: the same arrays again
    again = regex_to_dfa(pattern)
    assert np.array_equal(again.trans, dfa.trans) and np.array_equal(again.accept, dfa.accept)


def _reachable(dfa):
    seen, stack = {0}, [0]
    while stack:
        for n in set(dfa.trans[stack.pop()].tolist()) - {-1}:
            if n not in seen:
                seen.add(n)
                stack.append(n)
    return np.isin(np.arange(dfa.n_states), list(seen))


def _coreachable(dfa):
    live = dfa.accept.copy()
    for _ in range(dfa.n_states):
        live |= (np.where(dfa.trans >= 0, live[np.maximum(dfa.trans, 0)], False)).any(axis=1)
    return live


def test_trimming_drops_states_that_cannot_accept():
    dfa = regex_to_dfa(r"ab|a[^\s\S]c")  # the second branch can never finish
    assert dfa.n_states == 3 and dfa.accepts(b"ab") and dfa.walk(b"a") >= 0 and dfa.walk(b"ac") == -1
    assert regex_to_dfa(r"(a|b)*abb").n_states == 4, "minimal"


@pytest.mark.parametrize("pattern, word", [
    ("^a", "anchors"), ("a$", "anchors"), (r"\bfoo", "anchors"), (r"(a)\1", "backreferences"), ("(?=a)b", "lookaround"),
    ("(?<!a)b", "lookaround"), ("(?P<n>a)", "named"), ("(?i)a", "flags"), ("a*?", "lazy"), ("a+?", "lazy"), ("a{1,2}?", "lazy"),
    ("a++", "possessive"), ("[é]", "non-ASCII"), ("[a-é]", "non-ASCII"), (r"[^\s\S]", "matches nothing"), ("a{2,1}", "m > n"),
    ("(a", "missing"), ("a)", "unbalanced"), ("*a", "nothing to repeat"), ("a**", "multiple repeat"), ("a{", "malformed"),
    ("[a", "missing"), ("[z-a]", "bad range"), (r"\q", "unknown escape"), ("a\\", "backslash"),
])
def test_refusals_name_the_position(pattern, word):
    with pytest.raises(ValueError, match=r"position \d+") as e:
        regex_to_dfa(pattern)
    assert word in str(e.value), str(e.value)


def test_too_many_states():
    with pytest.raises(ValueError, match=f"more than {MAX_STATES}"):
        regex_to_dfa(r"(a|b)*a(a|b){12}")  # 2^13 states: the classic
    with pytest.raises(ValueError, match="NFA states"):
        regex_to_dfa(r"((a{100}){100}){100}")


def test_non_ascii_literals_are_utf8():
    dfa = regex_to_dfa("naïve|日本")
    assert dfa.accepts("naïve".encode()) and dfa.accepts("日本".encode()) and not dfa.accepts("日".encode())
    assert not dfa.accepts("naïve".encode("latin-1"))


# ---------------------------------------------------------------- JSON schemas
SCHEMAS = [
    {"type": "string"},
    {"type": "string", "minLength": 2, "maxLength": 5},
    {"type": "integer"},
    {"type": "number"},
    {"type": "boolean"},
    {"type": "null"},
    {"enum": ["red", "green", 3, 2.5, True, None, 'q"uote']},
    {"const": "a.b*c"},
    {"type": "array", "items": {"type": "integer"}, "minItems": 1, "maxItems": 3},
    {"type": "array", "items": {"type": "boolean"}},
    {"type": "object", "properties": {"label": {"type": "string", "maxLength": 6}, "count": {"type": "integer"}},
     "required": ["label", "count"], "additionalProperties": False},
    {"type": "object", "title": "nested", "properties": {
        "box": {"type": "array", "items": {"type": "number"}, "minItems": 4, "maxItems": 4},
        "tags": {"type": "array", "items": {"enum": ["a", "b"]}, "maxItems": 2},
        "who": {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"type": "null"}}, "required": ["ok", "n"]},
        "none": {"type": "object", "properties": {}}}, "required": ["box", "tags", "who", "none"]},
]


def conforms(x, schema) -> bool:
    """The supported subset of JSON Schema, for a parsed document."""
    if "const" in schema:
        return type(x) is type(schema["const"]) and x == schema["const"]
    if "enum" in schema:
        return any(type(x) is type(v) and x == v for v in schema["enum"])
    t = schema["type"]
    if t == "string":
        return isinstance(x, str) and schema.get("minLength", 0) <= len(x) <= schema.get("maxLength", 10**9)
    if t == "integer":
        return type(x) is int
    if t == "number":
        return type(x) in (int, float)
    if t == "boolean":
        return type(x) is bool
    if t == "null":
        return x is None
    if t == "array":
        return (isinstance(x, list) and schema.get("minItems", 0) <= len(x) <= schema.get("maxItems", 10**9)
                and all(conforms(i, schema["items"]) for i in x))
    props = schema.get("properties", {})
    return isinstance(x, dict) and list(x) == list(props) and all(conforms(x[k], s) for k, s in props.items())


@pytest.mark.parametrize("schema", SCHEMAS, ids=lambda s: json.dumps(s)[:40])
def test_schema_samples_parse_and_conform(schema):
    rng = np.random.default_rng(len(json.dumps(schema)))
    pattern = json_schema_to_regex(schema)
    dfa = regex_to_dfa(pattern)
    docs = sample(dfa, rng, n=60, longest=40)
    assert docs
    for d in docs:
        x = json.loads(d.decode("ascii"))
        assert conforms(x, schema), (d, schema)
        assert re.fullmatch(pattern.encode(), d)


def test_schema_hand_written_documents():
    schema = SCHEMAS[-2]
    pattern = json_schema_to_regex(schema)
    dfa = regex_to_dfa(pattern)
    dumps = lambda x: json.dumps(x, separators=(",", ":")).encode()
    valid = [{"label": "cat", "count": 3}, {"label": "", "count": -10}, {"label": 'a"b\\', "count": 0}, {"label": "a\nb", "count": 7}]
    invalid = [b'{"label":"cat","count":03}', b'{"count":3,"label":"cat"}', b'{"label":"cat"}', b'{"label": "cat","count":3}',
               b'{"label":"toolong","count":3}', b'{"label":"cat","count":3.5}', b'{"label":"cat","count":3,"x":1}',
               b'{"label":"caf\xc3\xa9","count":3}', b'{"label":"cat","count":3}\n', b""]
    for doc in [dumps(v) for v in valid] + invalid:
        assert dfa.accepts(doc) == bool(re.fullmatch(pattern.encode(), doc)), doc
    assert all(dfa.accepts(dumps(v)) and conforms(v, schema) for v in valid) and not any(dfa.accepts(d) for d in invalid)
    for number in (b"0", b"-0", b"12.50", b"1e9", b"-3.25E-7"):
        assert regex_to_dfa(json_schema_to_regex({"type": "number"})).accepts(number)
    for number in (b"01", b"1.", b".5", b"+1", b"1e", b"--1"):
        assert not regex_to_dfa(json_schema_to_regex({"type": "number"})).accepts(number)


@pytest.mark.parametrize("schema, key", [
    ({"type": "object", "properties": {"a": {"type": "null"}}}, "required"),
    ({"type": "object", "properties": {"a": {"type": "null"}, "b": {"type": "null"}}, "required": ["a"]}, "'b'"),
    ({"type": "object", "properties": {}, "additionalProperties": True}, "additionalProperties"),
    ({"type": "object", "properties": {}, "additionalProperties": {"type": "integer"}}, "additionalProperties"),
    ({"$ref": "#/x"}, "$ref"), ({"anyOf": [{"type": "null"}]}, "anyOf"), ({"oneOf": []}, "oneOf"), ({"allOf": []}, "allOf"),
    ({"type": "string", "pattern": "a+"}, "pattern"), ({"type": "string", "format": "date"}, "format"),
    ({"type": "integer", "minimum": 0}, "minimum"), ({"type": "number", "exclusiveMaximum": 1}, "exclusiveMaximum"),
    ({"type": "integer", "multipleOf": 2}, "multipleOf"), ({"type": "array", "items": {"type": "null"}, "uniqueItems": True}, "uniqueItems"),
    ({"type": "array"}, "items"), ({"type": "string", "minItems": 1}, "minItems"), ({"type": ["string", "null"]}, "type"),
    ({}, "type"), ({"enum": [[1]]}, "enum"), ({"type": "object", "properties": {"a": {"type": "integer", "maximum": 3}}, "required": ["a"]}, "properties.a.'maximum'"),
])
def test_schema_refusals_name_the_key(schema, key):
    with pytest.raises(ValueError) as e:
        json_schema_to_regex(schema)
    assert key in str(e.value), str(e.value)


# ---------------------------------------------------------------- TokenAutomaton.from_arrays
def hand_built():
    return [TokenAutomaton.choices([[5, 6], [5, 7, 8], [9]], eos_id=0), TokenAutomaton.min_tokens(3, eos_id=0),
            TokenAutomaton.allowed_tokens([4, 8, 15]), TokenAutomaton.banned_tokens([1, 2]), TokenAutomaton.sequence([7, 7, 3]),
            TokenAutomaton.from_states([({2: FORBID, 9: 1}, 0), ({2: FREE}, FORBID)])]


@pytest.mark.parametrize("i", range(6))
def test_from_arrays_round_trip(i):
    a = hand_built()[i]
    p = pack([a])
    b = TokenAutomaton.from_arrays(p.row_ptr, p.default_next, p.edge_tok, p.edge_next)
    assert b.edges == a.edges and b.default == a.default and b.n_states == a.n_states and b.n_edges == a.n_edges
    for got, want in zip(pack([b, a, b], state0=3, edge0=5).__dict__.items(), pack([a, a, a], state0=3, edge0=5).__dict__.items()):
        assert got[0] == want[0] and (np.array_equal(got[1], want[1]) and np.asarray(got[1]).dtype == np.asarray(want[1]).dtype), got[0]
    a.validate(16, 1), b.validate(16, 1)
    rng = np.random.default_rng(i)
    for _ in range(200):
        q, t = int(rng.integers(a.n_states)), int(rng.integers(16))
        assert b.next(q, t) == a.next(q, t)
        ids = rng.integers(0, 16, size=5).tolist()
        assert b.walk(ids) == a.walk(ids)
    for x, y in zip(b.arrays(), a.arrays()):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("states, vocab, suppress", [
    ([({3: 0, 2: 0}, FORBID)], 8, -1),            # unsorted is impossible through from_states; see below
    ([({9: 0}, FORBID)], 8, -1),                  # a token outside the vocabulary
    ([({1: 7}, FORBID)], 8, -1),                  # a next value that is no state
    ([({1: 0}, 5)], 8, -1),                       # a default that is no state
    ([({}, FORBID)], 8, -1),                      # nothing allowed
    ([({3: 0}, FORBID)], 8, 3),                   # only the suppressed id allowed
    ([({t: FORBID for t in range(7)}, 0)], 8, 7),  # default-allow with every other id forbidden
    ([({1: 1}, FORBID), ({2: DEAD}, 0)], 8, -1),  # the second state is the bad one
])
def test_from_arrays_validate_refuses_what_the_tuple_form_refuses(states, vocab, suppress):
    a = TokenAutomaton.from_states(states)
    b = TokenAutomaton.from_arrays(*a.arrays())
    try:
        a.validate(vocab, suppress)
        want = None
    except ValueError as e:
        want = str(e)
    if want is None:
        b.validate(vocab, suppress)
    else:
        with pytest.raises(ValueError) as e:
            b.validate(vocab, suppress)
        assert str(e.value) == want


def test_from_arrays_unsorted_and_shapes():
    with pytest.raises(ValueError, match="sorted"):
        TokenAutomaton.from_arrays([0, 2, 3], [FORBID, 0], [4, 4, 1], [0, 0, 0]).validate(8)
    TokenAutomaton.from_arrays([0, 2, 3], [FORBID, 0], [4, 5, 1], [0, 0, 0]).validate(8)  # (a new state may start lower)
    for bad in (([0, 1], [0, 0], [1], [0]), ([1, 1], [0], [1], [0]), ([0, 2], [0], [1], [0]), ([0, 1], [0], [1], [0, 0]), ([0], [], [], [])):
        with pytest.raises(ValueError, match="from_arrays"):
            TokenAutomaton.from_arrays(*bad)


def test_large_table_needs_no_per_edge_python():
    """Half a million edges: validate and pack in well under the time a per-edge loop would take (loose: seconds)."""
    import time

    s, v = 64, 51200
    rng = np.random.default_rng(0)
    per = 8000
    tok = np.concatenate([np.sort(rng.choice(v, size=per, replace=False)) for _ in range(s)]).astype(np.int32)
    a = TokenAutomaton.from_arrays(np.arange(s + 1) * per, np.full(s, FORBID), tok, rng.integers(0, s, size=s * per))
    t0 = time.perf_counter()
    a.validate(v, 3)
    p = pack([a], state0=2, edge0=7)
    assert time.perf_counter() - t0 < 2.0 and a._edges is None, "the tuples were never made"
    assert p.n_edges == s * per and p.row_ptr[0] == 7 and p.default_next[0] == FORBID and p.edge_next.min() >= 2


# ---------------------------------------------------------------- the reference lift, pruning, settings
def test_reference_lift_against_brute_force():
    rng = np.random.default_rng(5)
    s, v, eos = 5, 40, 1
    vocab = [bytes(rng.integers(0, 4, size=int(rng.integers(0, 4))).astype(np.uint8)) for _ in range(v)]
    trans = np.where(rng.random((s, 256)) < 0.7, rng.integers(0, s, size=(s, 256)), -1)
    accept = rng.random(s) < 0.5
    forbidden = np.zeros(v, dtype=np.uint8)
    forbidden[[3, 7]] = 1
    nxt = ref.lift(trans, accept, vocab, eos, forbidden)
    for q in range(s):
        for t in range(v):
            state = q
            for b in vocab[t]:
                state = int(trans[state, b]) if state >= 0 else -1
            want = state if state >= 0 and vocab[t] and not forbidden[t] else FORBID
            if t == eos:
                want = FREE if accept[q] else FORBID
            assert nxt[q, t] == want
    row_ptr, default, tok, val = ref.compact(nxt)
    for q in range(s):
        counts = {x: int((nxt[q] == x).sum()) for x in set(nxt[q].tolist())}
        best = max(counts.values())
        assert default[q] == min(x for x, c in counts.items() if c == best)
        e = slice(row_ptr[q], row_ptr[q + 1])
        assert tok[e].tolist() == [t for t in range(v) if nxt[q, t] != default[q]] and val[e].tolist() == [nxt[q, t] for t in tok[e]]
    mine = prune_unreachable(row_ptr, default, tok, val)[:4]
    for g, w in zip(mine, ref.prune(row_ptr, default, tok, val)):
        assert np.array_equal(g, w) and g.dtype == np.int32


def test_finish_automaton_names_what_cannot_be_spelled():
    dfa = regex_to_dfa("ab")
    vocab = [b"", b"a", b"c"]  # no token spells b
    with pytest.raises(ValueError, match=r"cannot be spelled with this vocabulary.*b'a'"):
        finish_automaton(dfa, ref.compact(ref.lift(dfa.trans, dfa.accept, vocab, 0, np.zeros(3, np.uint8))))
    vocab = [b"", b"a", b"b", b"ab"]
    a = finish_automaton(dfa, ref.compact(ref.lift(dfa.trans, dfa.accept, vocab, 0, np.zeros(4, np.uint8))))
    assert a.walk([1, 2, 0]) == FREE and a.walk([3, 0]) == FREE and a.walk([3, 1]) == DEAD and a.walk([0]) == DEAD
    a.validate(4)


def test_settings_keys():
    assert grammar_of(None) is None and grammar_of({"constraints": object()}) is None
    assert grammar_of({"regex": "a"}) == ("regex", "a") and grammar_of({"json_schema": {"type": "null"}})[0] == "json_schema"
    with pytest.raises(ValueError, match="mutually exclusive"):
        grammar_of({"regex": "a", "json_schema": {}})
    with pytest.raises(ValueError, match="mutually exclusive"):
        grammar_of({"regex": "a", "constraints": TokenAutomaton.allowed_tokens([1])})
    for st in ({"regex": "a"}, {"json_schema": {"type": "null"}}):
        with pytest.raises(ValueError, match="constraints are not served by detect"):
            refuse_constraints(st, "detect")


def test_vocab_bytes_of_a_stub_tokenizer():
    table = gpt2_unicode_to_byte()
    assert len(table) == 256 and sorted(table.values()) == list(range(256)) and table["Ġ"] == 0x20 and table["Ċ"] == 0x0A and table["A"] == 0x41

    class Stub:
        def get_vocab(self):
            return {"Ġyes": 0, "no": 1, "Ã©": 2, "<|endoftext|>": 3, "日": 4, "far": 99}

    got = vocab_bytes_of(Stub(), 6)
    assert got == [b" yes", b"no", "é".encode(), b"<|endoftext|>", b"", b""]
    with pytest.raises(ValueError, match="vocab_bytes"):
        vocab_bytes_of(object(), 6)
