"""Structured output: a regular expression or a JSON schema compiled to a ``TokenAutomaton`` (constraint.py).

The parsing half is host only, numpy only: ``regex_to_dfa`` (parser -> NFA -> subset construction -> trimming ->
minimisation) gives a ``ByteDFA`` over the bytes of the output, and ``json_schema_to_regex`` writes a schema as such a
pattern.  The lifting half runs on the device: ``compile_regex`` / ``compile_json_schema`` walk every token of the
vocabulary through the DFA from every state (md_automaton_count / md_automaton_fill, csrc/automaton.hip) and get back the
table md_constrain_rows reads.

The regex subset (full match: the whole output must match; everything is bytes, a class is ASCII only):
  literals (a non-ASCII one contributes its UTF-8 bytes); ``.`` any byte except ``\\n``; ``[...]`` / ``[^...]`` with ranges;
  ``\\d \\w \\s \\D \\W \\S`` (ASCII), ``\\n \\t \\r \\f \\v \\xhh`` and escaped punctuation; ``(...)`` and ``(?:...)``; ``|``;
  ``* + ? {m} {m,} {m,n} {,n}``.  A literal brace is written ``\\{``.
ValueError (with the position) for anchors, backreferences, lookaround, named groups, flags, lazy or possessive
quantifiers, a non-ASCII character in a class, a pattern that matches nothing, and a DFA of more than ``MAX_STATES``
states after trimming.
"""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .constraint import FORBID, FREE, TokenAutomaton

MAX_STATES = 4096          # include/moondream_hip.h MD_AUTOMATON_STATES_MAX
_MAX_NFA_STATES = 200_000  # before the DFA: a pattern whose repetitions multiply past this is refused
_MAX_RAW_STATES = 65_536   # subset construction stops here (trimming and minimisation only shrink)

_ALL = (1 << 256) - 1


def _mask(bs) -> int:
    m = 0
    for b in bs:
        m |= 1 << b
    return m


_DIGIT = _mask(range(0x30, 0x3A))
_WORD = _DIGIT | _mask(range(0x41, 0x5B)) | _mask(range(0x61, 0x7B)) | (1 << 0x5F)
_SPACE = _mask(b" \t\n\r\f\v")
_CLASS_ESC = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": _ALL ^ _DIGIT, "W": _ALL ^ _WORD, "S": _ALL ^ _SPACE}
_CHAR_ESC = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11}
_ANCHOR_ESC = "bBAZ"


class ByteDFA:
    """``trans`` int32 [S][256]: the next state, or -1 (dead); ``accept`` bool [S]; the start state is 0."""

    __slots__ = ("trans", "accept")

    def __init__(self, trans: np.ndarray, accept: np.ndarray):
        self.trans = np.ascontiguousarray(trans, dtype=np.int32)
        self.accept = np.ascontiguousarray(accept, dtype=bool)
        if self.trans.ndim != 2 or self.trans.shape[1] != 256 or self.accept.shape != (self.trans.shape[0],) or self.trans.shape[0] < 1:
            raise ValueError("ByteDFA: trans [S][256] and accept [S], S >= 1")

    @property
    def n_states(self) -> int:
        return int(self.trans.shape[0])

    def walk(self, data: bytes, state: int = 0) -> int:
        """The state after ``data`` from ``state``, -1 once a step is dead."""
        for b in data:
            if state < 0:
                return -1
            state = int(self.trans[state, b])
        return state

    def accepts(self, data: bytes) -> bool:
        q = self.walk(data)
        return q >= 0 and bool(self.accept[q])


# ---------------------------------------------------------------- parser: pattern -> tree
# ("set", mask) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, lo, hi or None)
class _Parser:
    def __init__(self, pattern: str):
        self.p, self.i = pattern, 0

    def fail(self, what: str, at: Optional[int] = None):
        raise ValueError(f"regex: {what} at position {self.i if at is None else at} of {self.p!r}")

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.i < len(self.p) and self.p[self.i] == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            at = self.i
            atom = self.atom()
            items.append(self.quantified(atom, at))
        return ("cat", items)

    def quantified(self, atom, at: int):
        if self.i >= len(self.p) or self.p[self.i] not in "*+?{":
            return atom
        c, q_at = self.p[self.i], self.i
        if c == "{":
            lo, hi = self.braces()
        else:
            self.i += 1
            lo, hi = {"*": (0, None), "+": (1, None), "?": (0, 1)}[c]
        if self.i < len(self.p) and self.p[self.i] in "?+":
            self.fail("lazy and possessive quantifiers are not supported")
        if self.i < len(self.p) and self.p[self.i] in "*{":
            self.fail("multiple repeat")
        if hi is not None and hi < lo:
            self.fail("{m,n} with m > n", q_at)
        return ("rep", atom, lo, hi)

    def braces(self) -> Tuple[int, Optional[int]]:
        at = self.i
        end = self.p.find("}", at)
        body = self.p[at + 1 : end] if end > 0 else ""
        lo_s, comma, hi_s = body.partition(",")
        ok = end > 0 and (lo_s.isdigit() or (lo_s == "" and comma)) and (hi_s == "" or hi_s.isdigit()) and body not in ("", ",") \
            and body.isascii()
        if not ok:
            self.fail("malformed quantifier (a literal brace is written \\{)", at)
        self.i = end + 1
        lo = int(lo_s) if lo_s else 0
        return lo, (lo if not comma else (int(hi_s) if hi_s else None))

    def atom(self):
        c = self.p[self.i]
        if c == "(":
            return self.group()
        if c == "[":
            return self.cls()
        if c == ".":
            self.i += 1
            return ("set", _ALL ^ (1 << 10))
        if c in "^$":
            self.fail("anchors are not supported (the whole output must match anyway)")
        if c in "*+?{":
            self.fail("nothing to repeat")
        if c == "\\":
            kind, val = self.escape(in_class=False)
            return ("set", val if kind == "set" else 1 << val)
        self.i += 1
        if ord(c) < 128:
            return ("set", 1 << ord(c))
        return ("cat", [("set", 1 << b) for b in c.encode("utf-8")])

    def group(self):
        at = self.i
        self.i += 1
        if self.p.startswith("?", self.i):
            nxt = self.p[self.i + 1 : self.i + 2]
            if nxt == ":":
                self.i += 2
            elif nxt in ("=", "!") or self.p[self.i + 1 : self.i + 3] in ("<=", "<!"):
                self.fail("lookaround is not supported", at)
            elif nxt in ("P", "<"):
                self.fail("named groups and backreferences are not supported", at)
            else:
                self.fail("flags and group extensions are not supported", at)
        node = self.alt()
        if self.i >= len(self.p) or self.p[self.i] != ")":
            self.fail("missing ')' for the group", at)
        self.i += 1
        return node

    def escape(self, in_class: bool):
        """At a backslash -> ("set", mask) or ("byte", value)."""
        at = self.i
        if at + 1 >= len(self.p):
            self.fail("a pattern ends in a backslash")
        c = self.p[at + 1]
        self.i += 2
        if c in _CLASS_ESC:
            return "set", _CLASS_ESC[c]
        if c in _CHAR_ESC:
            return "byte", _CHAR_ESC[c]
        if c == "x":
            h = self.p[self.i : self.i + 2]
            if len(h) != 2 or any(x not in "0123456789abcdefABCDEF" for x in h):
                self.fail("\\x takes two hex digits", at)
            self.i += 2
            return "byte", int(h, 16)
        if c == "0":
            return "byte", 0
        if c == "b" and in_class:
            return "byte", 8
        if c.isdigit():
            self.fail("backreferences are not supported", at)
        if c in _ANCHOR_ESC and not (in_class and c == "b"):
            self.fail("anchors are not supported", at)
        if ord(c) >= 128:
            self.fail("an escaped non-ASCII character", at)
        if c.isalnum():
            self.fail(f"unknown escape \\{c}", at)
        return "byte", ord(c)

    def cls(self):
        at = self.i
        self.i += 1
        negate = self.p.startswith("^", self.i)
        self.i += int(negate)
        mask, first = 0, True
        while True:
            if self.i >= len(self.p):
                self.fail("missing ']' for the class", at)
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            kind, lo = self.class_item()
            if kind == "set":
                mask |= lo
                continue
            if self.p.startswith("-", self.i) and self.i + 1 < len(self.p) and self.p[self.i + 1] != "]":
                r_at = self.i
                self.i += 1
                kind2, hi = self.class_item()
                if kind2 == "set" or hi < lo:
                    self.fail("bad range in a class", r_at)
                mask |= _mask(range(lo, hi + 1))
            else:
                mask |= 1 << lo
        return ("set", (_ALL ^ mask) if negate else mask)

    def class_item(self):
        c = self.p[self.i]
        if c == "\\":
            return self.escape(in_class=True)
        if ord(c) >= 128:
            self.fail("a non-ASCII character inside a class (classes are sets of single bytes)")
        self.i += 1
        return "byte", ord(c)


# ---------------------------------------------------------------- tree -> NFA -> DFA
class _Nfa:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[int, int]]] = []  # (mask, target)

    def new(self) -> int:
        if len(self.eps) >= _MAX_NFA_STATES:
            raise ValueError(f"regex: the pattern expands to more than {_MAX_NFA_STATES} NFA states (nested counted repetitions)")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            if node[1]:
                self.edges[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.new()
            for item in node[1]:
                s, e = self.build(item)
                self.eps[b].append(s)
                b = e
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for item in node[1]:
                s, e = self.build(item)
                self.eps[a].append(s)
                self.eps[e].append(b)
            return a, b
        _, item, lo, hi = node
        a = b = self.new()
        for _ in range(lo):
            s, e = self.build(item)
            self.eps[b].append(s)
            b = e
        if hi is None:  # a loop after the mandatory copies
            s, e = self.build(item)
            end = self.new()
            self.eps[b] += [s, end]
            self.eps[e] += [s, end]
            return a, end
        end = self.new()
        for _ in range(hi - lo):  # optional copies, each may leave to the end
            s, e = self.build(item)
            self.eps[b] += [s, end]
            b = e
        self.eps[b].append(end)
        return a, end


def _subset_construction(nfa: _Nfa, start: int, final: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (trans over byte classes int32 [S][C], accept bool [S], class of byte int64 [256]); states in the order found."""
    masks = sorted({m for es in nfa.edges for m, _ in es})
    sig: Dict[Tuple[int, ...], int] = {}
    cls_of = np.zeros(256, dtype=np.int64)
    reps: List[int] = []
    for b in range(256):
        key = tuple((m >> b) & 1 for m in masks)
        if key not in sig:
            sig[key] = len(reps)
            reps.append(b)
        cls_of[b] = sig[key]
    closure_memo: Dict[int, frozenset] = {}

    def closure(states) -> frozenset:
        out = set()
        for s0 in states:
            c = closure_memo.get(s0)
            if c is None:
                seen, stack = {s0}, [s0]
                while stack:
                    for t in nfa.eps[stack.pop()]:
                        if t not in seen:
                            seen.add(t)
                            stack.append(t)
                c = closure_memo[s0] = frozenset(seen)
            out |= c
        return frozenset(out)

    first = closure([start])
    ids, order, rows = {first: 0}, [first], []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        moves = [(m, t) for s in cur for m, t in nfa.edges[s]]
        row = []
        for b in reps:
            tgt = {t for m, t in moves if (m >> b) & 1}
            if not tgt:
                row.append(-1)
                continue
            nxt = closure(tgt)
            if nxt not in ids:
                if len(order) >= _MAX_RAW_STATES:
                    raise ValueError(f"regex: more than {_MAX_RAW_STATES} DFA states before trimming (the cap after it is {MAX_STATES})")
                ids[nxt] = len(order)
                order.append(nxt)
            row.append(ids[nxt])
        rows.append(row)
    trans = np.asarray(rows, dtype=np.int32).reshape(len(order), len(reps))
    accept = np.fromiter((final in s for s in order), dtype=bool, count=len(order))
    return trans, accept, cls_of


def _live_states(trans: np.ndarray, accept: np.ndarray) -> np.ndarray:
    """bool [S]: an accepting state is reachable (backwards breadth-first search over the reversed edges)."""
    s, c = trans.shape
    src, dst = np.repeat(np.arange(s), c), trans.reshape(-1)
    keep = dst >= 0
    src, dst = src[keep], dst[keep]
    order = np.argsort(dst, kind="stable")
    src, dst = src[order], dst[order]
    ptr = np.searchsorted(dst, np.arange(s + 1))
    live = accept.copy()
    frontier = np.flatnonzero(accept)
    while frontier.size:
        preds = np.unique(np.concatenate([src[ptr[q] : ptr[q + 1]] for q in frontier.tolist()])) if frontier.size else frontier
        frontier = preds[~live[preds]]
        live[frontier] = True
    return live


def _renumber(trans: np.ndarray, accept: np.ndarray, keep: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Drop the states outside ``keep`` (their entries become -1) and number the rest breadth first from state 0, in
    class order: the numbering depends on the language's automaton alone."""
    t = np.where((trans >= 0) & keep[np.maximum(trans, 0)], trans, -1)
    new = np.full(trans.shape[0], -1, dtype=np.int64)
    new[0], order, i = 0, [0], 0
    while i < len(order):
        for n in t[order[i]].tolist():
            if n >= 0 and new[n] < 0:
                new[n] = len(order)
                order.append(n)
        i += 1
    order_a = np.asarray(order)
    t = t[order_a]
    return np.where(t >= 0, new[np.maximum(t, 0)], -1).astype(np.int32), accept[order_a]


def _minimise(trans: np.ndarray, accept: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Moore's partition refinement on a trimmed DFA (-1 is the one dead class), then one state per block."""
    label = accept.astype(np.int64)
    n_blocks = len(np.unique(label))
    while True:
        nxt = np.where(trans >= 0, label[np.maximum(trans, 0)], -1)
        _, label = np.unique(np.concatenate([label[:, None], nxt], axis=1), axis=0, return_inverse=True)
        label = label.reshape(-1)
        n = int(label.max()) + 1
        if n == n_blocks:
            break
        n_blocks = n
    rep = np.full(n_blocks, -1, dtype=np.int64)  # the first state of each block
    for q in range(trans.shape[0] - 1, -1, -1):
        rep[label[q]] = q
    t = trans[rep]
    t = np.where(t >= 0, label[np.maximum(t, 0)], -1)
    # block ids are np.unique's; put the start state's block first, then renumber breadth first
    b0 = int(label[0])
    swap = np.arange(n_blocks)
    swap[[0, b0]] = swap[[b0, 0]]
    t = np.where(t >= 0, swap[np.maximum(t, 0)], -1)[swap]
    acc = accept[rep][swap]
    return _renumber(t.astype(np.int32), acc, np.ones(n_blocks, dtype=bool))


def regex_to_dfa(pattern: str) -> ByteDFA:
    """The minimal trimmed byte DFA of ``pattern`` under full-match semantics (the subset: the module docstring).  Every
    state has a path to an accepting one; states are numbered breadth first from the start state 0 in byte order, so equal
    patterns give equal arrays.  ValueError as the module docstring lists."""
    if not isinstance(pattern, str):
        raise ValueError(f"regex: the pattern is a str, not {type(pattern).__name__}")
    tree = _Parser(pattern).parse()
    nfa = _Nfa()
    start, final = nfa.build(tree)
    trans, accept, cls_of = _subset_construction(nfa, start, final)
    live = _live_states(trans, accept)
    if not live[0]:
        raise ValueError(f"regex: the pattern matches nothing, at position 0 of {pattern!r}")
    trans, accept = _renumber(trans, accept, live)
    trans, accept = _minimise(trans, accept)
    if trans.shape[0] > MAX_STATES:
        raise ValueError(f"regex: {trans.shape[0]} DFA states after trimming, more than {MAX_STATES}: {pattern[:60]!r}")
    return ByteDFA(trans[:, cls_of], accept)


# ---------------------------------------------------------------- JSON schema -> pattern
_STRING_CHAR = r'([ !#-\[\]-~]|\\["\\/bfnrt])'
_INTEGER = r"-?(0|[1-9][0-9]*)"
_NUMBER = _INTEGER + r"(\.[0-9]+)?([eE][+-]?[0-9]+)?"
_ANNOTATIONS = ("title", "description", "default", "examples", "$schema", "$id", "$comment")
_REFUSED = ("$ref", "anyOf", "oneOf", "allOf", "not", "if", "then", "else", "pattern", "format", "minimum", "maximum", "exclusiveMinimum",
            "exclusiveMaximum", "multipleOf", "patternProperties", "propertyNames", "minProperties", "maxProperties",
            "dependentRequired", "dependentSchemas", "prefixItems", "contains", "uniqueItems", "$defs", "definitions")
_KEYS_OF = {"string": ("minLength", "maxLength"), "integer": (), "number": (), "boolean": (), "null": (),
            "array": ("items", "minItems", "maxItems"), "object": ("properties", "required", "additionalProperties")}
_SPECIAL = set("\\.[](){}*+?|^$-")


def _escape(text: str) -> str:
    return "".join("\\" + c if c in _SPECIAL else c for c in text)


def _count(schema: dict, key: str, where: str) -> Optional[int]:
    v = schema.get(key)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ValueError(f"json schema: {where}{key!r} must be a non-negative integer, not {v!r}")
    return v


def _scalar(v, where: str, key: str) -> str:
    if not (v is None or isinstance(v, (bool, int, float, str))):
        raise ValueError(f"json schema: {where}{key!r} takes scalars only (strings, numbers, booleans, null), not {v!r}")
    return _escape(json.dumps(v, separators=(",", ":")))


def _schema_regex(schema, where: str) -> str:
    if not isinstance(schema, dict):
        raise ValueError(f"json schema: {where or 'the schema'} must be an object, not {schema!r}")
    for k in schema:
        if k in _REFUSED:
            raise ValueError(f"json schema: {where}{k!r} is not supported")
    if "const" in schema or "enum" in schema:
        for k in schema:
            if k not in ("const", "enum", "type") + _ANNOTATIONS:
                raise ValueError(f"json schema: {where}{k!r} beside enum / const is not supported")
        if "const" in schema:
            return _scalar(schema["const"], where, "const")
        vals = schema["enum"]
        if not isinstance(vals, (list, tuple)) or not vals:
            raise ValueError(f"json schema: {where}'enum' must be a non-empty list")
        return "(" + "|".join(_scalar(v, where, "enum") for v in vals) + ")"
    t = schema.get("type")
    if not isinstance(t, str) or t not in _KEYS_OF:
        raise ValueError(f"json schema: {where}'type' must be one of {', '.join(_KEYS_OF)}, not {t!r}")
    for k in schema:
        if k != "type" and k not in _KEYS_OF[t] and k not in _ANNOTATIONS:
            raise ValueError(f"json schema: {where}{k!r} is not supported for type {t!r}")
    if t == "string":
        lo, hi = _count(schema, "minLength", where) or 0, _count(schema, "maxLength", where)
        if hi is not None and hi < lo:
            raise ValueError(f"json schema: {where}'maxLength' below 'minLength'")
        quant = "*" if (lo, hi) == (0, None) else "{%d,%s}" % (lo, "" if hi is None else hi)
        return '"' + _STRING_CHAR + quant + '"'
    if t in ("integer", "number"):
        return _INTEGER if t == "integer" else _NUMBER
    if t == "boolean":
        return "(true|false)"
    if t == "null":
        return "null"
    if t == "array":
        if "items" not in schema:
            raise ValueError(f"json schema: {where}'items' is required for an array")
        item = _schema_regex(schema["items"], where + "items.")
        lo, hi = _count(schema, "minItems", where) or 0, _count(schema, "maxItems", where)
        if hi is not None and hi < lo:
            raise ValueError(f"json schema: {where}'maxItems' below 'minItems'")
        if hi == 0:
            return r"\[\]"
        more = "(," + item + "){%d,%s}" % (max(lo - 1, 0), "" if hi is None else hi - 1)
        body = "(" + item + more + ")"
        return r"\[" + body + ("?" if lo == 0 else "") + r"\]"
    props = schema.get("properties", {})
    if not isinstance(props, dict):
        raise ValueError(f"json schema: {where}'properties' must be an object")
    if schema.get("additionalProperties", False) is not False:
        raise ValueError(f"json schema: {where}'additionalProperties' other than false is not supported")
    required = schema.get("required", [])
    if not isinstance(required, (list, tuple)) or set(required) - set(props):
        raise ValueError(f"json schema: {where}'required' must list declared properties")
    missing = [k for k in props if k not in required]
    if missing:
        raise ValueError(f"json schema: {where}'required' must name every property (optional properties are not supported): "
                         f"{missing[0]!r} is optional")
    fields = [_escape(json.dumps(str(k))) + ":" + _schema_regex(v, f"{where}properties.{k}.") for k, v in props.items()]
    return r"\{" + ",".join(fields) + r"\}"


def json_schema_to_regex(schema: dict) -> str:
    """A pattern (``regex_to_dfa``'s subset) for the documents of ``schema`` in COMPACT form, no whitespace, as
    ``json.dumps(x, separators=(",", ":"))`` writes them.  Supported: ``type`` ``string`` (``minLength`` / ``maxLength``; the
    body is printable ASCII 0x20..0x7e except ``"`` and ``\\``, plus the escapes ``\\" \\\\ \\/ \\b \\f \\n \\r \\t`` -- no
    ``\\uXXXX``, no non-ASCII content yet), ``integer``, ``number``, ``boolean``, ``null``; ``enum`` / ``const`` of scalars;
    ``array`` with ``items``, ``minItems``, ``maxItems``; ``object`` with ``properties`` in declared order, every one of them
    listed in ``required``; any nesting of these.  Annotations (``title``, ``description``, ``default``, ``examples``,
    ``$schema``, ``$id``, ``$comment``) are ignored.  ValueError naming the key for optional properties,
    ``additionalProperties`` other than false / absent, ``$ref``, ``anyOf`` / ``oneOf`` / ``allOf``, ``pattern``, ``format``,
    numeric bounds, and every other keyword that restricts values."""
    return _schema_regex(schema, "")


# ---------------------------------------------------------------- the lift: ByteDFA x vocabulary -> TokenAutomaton
def vocab_arrays(vocab_bytes: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """``vocab_bytes[v]``: the bytes token v spells (empty: the token spells nothing and is never allowed) ->
    ``(tok_off int32 [V + 1], tok_bytes uint8)``, the layout md_automaton_lift reads."""
    lens = np.fromiter((len(b) for b in vocab_bytes), dtype=np.int64, count=len(vocab_bytes))
    off = np.zeros(len(vocab_bytes) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] >= 2**31:
        raise ValueError("vocab_bytes: more than 2^31 bytes in all")
    data = np.frombuffer(b"".join(bytes(b) for b in vocab_bytes), dtype=np.uint8)
    return off.astype(np.int32), (data if data.size else np.zeros(1, dtype=np.uint8))


def prune_unreachable(row_ptr: np.ndarray, default_next: np.ndarray, edge_tok: np.ndarray, edge_next: np.ndarray):
    """Drop the states no token sequence reaches from state 0 and renumber the rest in ascending order of their old ids
    (state 0 stays 0) -> the four arrays of the smaller table and ``old_id`` int64 [S'] of each kept state."""
    s = default_next.shape[0]
    seen = np.zeros(s, dtype=bool)
    seen[0] = True
    frontier = np.array([0])
    while frontier.size:
        idx = np.concatenate([np.arange(row_ptr[q], row_ptr[q + 1]) for q in frontier.tolist()]) if frontier.size else frontier
        nxt = np.concatenate([edge_next[idx.astype(np.int64)], default_next[frontier]])
        nxt = np.unique(nxt[nxt >= 0])
        frontier = nxt[~seen[nxt]]
        seen[frontier] = True
    old = np.flatnonzero(seen)
    new = np.cumsum(seen) - 1
    counts = np.diff(row_ptr)[old]
    keep_edge = np.repeat(seen, np.diff(row_ptr))
    remap = lambda n: np.where(n >= 0, new[np.maximum(n, 0)], n).astype(np.int32)
    ptr = np.zeros(old.shape[0] + 1, dtype=np.int32)
    np.cumsum(counts, out=ptr[1:])
    return ptr, remap(default_next[old]), edge_tok[keep_edge].astype(np.int32), remap(edge_next[keep_edge]), old


def _bytes_reaching(dfa: ByteDFA, target: int) -> bytes:
    """A shortest byte string from the start state to ``target`` (breadth first, smallest byte first)."""
    prev = {0: None}
    queue = [0]
    for q in queue:
        if q == target:
            break
        for b, n in enumerate(dfa.trans[q].tolist()):
            if n >= 0 and n not in prev:
                prev[n] = (q, b)
                queue.append(n)
    out, q = [], target
    while prev.get(q) is not None:
        q, b = prev[q]
        out.append(b)
    return bytes(reversed(out))


def finish_automaton(dfa: ByteDFA, arrays, what: str = "the pattern") -> TokenAutomaton:
    """The host end of a compile: the lift's four arrays (one state per DFA state) -> the pruned ``TokenAutomaton``.
    ValueError if a reachable state allows no token: the pattern cannot be spelled with this vocabulary from there."""
    row_ptr, default_next, edge_tok, edge_next, old = prune_unreachable(*[np.asarray(a) for a in arrays])
    n_edges = np.diff(row_ptr)
    forbid_edges = np.bincount(np.repeat(np.arange(old.shape[0]), n_edges)[edge_next == FORBID], minlength=old.shape[0])
    stuck = np.flatnonzero((default_next == FORBID) & (n_edges == forbid_edges))
    if stuck.size:  # a state whose default is not FORBID allows most of the vocabulary
        q = int(old[stuck[0]])
        raise ValueError(f"{what} cannot be spelled with this vocabulary: after the bytes {_bytes_reaching(dfa, q)!r} no token "
                         "(nor the end of the output) may follow")
    return TokenAutomaton.from_arrays(row_ptr, default_next, edge_tok, edge_next)


def _forbidden_mask(vocab: int, eos_id: int, forbidden_ids) -> np.ndarray:
    if not 0 <= int(eos_id) < vocab:
        raise ValueError(f"eos_id {eos_id} outside [0, {vocab})")
    mask = np.zeros(vocab, dtype=np.uint8)
    ids = np.asarray(list(forbidden_ids), dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= vocab):
        raise ValueError(f"forbidden_ids: an id outside [0, {vocab})")
    mask[ids] = 1
    return mask


def lift_on_device(dfa: ByteDFA, tok_off: np.ndarray, tok_bytes: np.ndarray, eos_id: int, forbidden: np.ndarray, device="cuda"):
    """md_automaton_count, one read of the edge total, md_automaton_fill, then ONE device-to-host copy of the four arrays
    -> ``(row_ptr, default_next, edge_tok, edge_next)`` as int32 numpy arrays, one state per DFA state."""
    import torch

    from . import _lib

    lib = _lib.load()
    s, v = dfa.n_states, int(tok_off.shape[0]) - 1
    if np.any(np.diff(tok_off) < 0) or tok_off[0] != 0 or tok_off[-1] > tok_bytes.shape[0]:
        raise ValueError("tok_off must start at 0, never decrease and end inside tok_bytes")
    dev = torch.device(device)
    with torch.cuda.device(dev):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_trans, d_accept, d_off, d_bytes, d_forb = up(dfa.trans), up(dfa.accept.astype(np.uint8)), up(tok_off), up(tok_bytes), up(forbidden)
        ws_bytes = lib.md_automaton_workspace_bytes(s, v)
        if ws_bytes == 0:
            raise ValueError(f"{s} states / {v} tokens: outside what md_automaton_lift serves")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        head = torch.empty(2 * s + 1, dtype=torch.int32, device=dev)  # default_next [s] | row_ptr [s + 1]
        stream = torch.cuda.current_stream().cuda_stream
        common = (d_trans.data_ptr(), d_accept.data_ptr(), s, d_off.data_ptr(), d_bytes.data_ptr(), int(tok_bytes.shape[0]), v,
                  int(eos_id), d_forb.data_ptr())
        _lib.check(lib.md_automaton_count(*common, head.data_ptr(), head[s:].data_ptr(), ws.data_ptr(), ws_bytes, stream),
                   "md_automaton_count")
        n_edges = int(head[2 * s].item())  # the one host read between the passes
        out = torch.empty(2 * s + 1 + 2 * n_edges, dtype=torch.int32, device=dev)
        out[: 2 * s + 1].copy_(head)
        e_tok, e_next = out[2 * s + 1 : 2 * s + 1 + n_edges], out[2 * s + 1 + n_edges :]
        _lib.check(lib.md_automaton_fill(*common, head.data_ptr(), head[s:].data_ptr(), e_tok.data_ptr() if n_edges else None,
                                         e_next.data_ptr() if n_edges else None, n_edges, ws.data_ptr(), ws_bytes, stream),
                   "md_automaton_fill")
        host = out.cpu().numpy()  # the one copy back (it waits for the stream)
    return host[s : 2 * s + 1], host[:s], host[2 * s + 1 : 2 * s + 1 + n_edges], host[2 * s + 1 + n_edges :]


def compile_dfa(dfa: ByteDFA, vocab_bytes: Sequence[bytes], eos_id: int, forbidden_ids=(), device="cuda", what="the pattern") -> TokenAutomaton:
    tok_off, tok_bytes = vocab_arrays(vocab_bytes)
    forbidden = _forbidden_mask(len(vocab_bytes), eos_id, forbidden_ids)
    return finish_automaton(dfa, lift_on_device(dfa, tok_off, tok_bytes, eos_id, forbidden, device), what)


def compile_regex(pattern: str, vocab_bytes: Sequence[bytes], eos_id: int, forbidden_ids=(), device="cuda") -> TokenAutomaton:
    """``pattern`` (``regex_to_dfa``) over the vocabulary ``vocab_bytes`` (``vocab_bytes[v]``: the bytes token v spells) as a
    ``TokenAutomaton``: a generation under it spells a match of the pattern and may end (``eos_id``) only where the
    pattern is complete; after eos the row is free.  ``forbidden_ids`` (special tokens) and tokens that spell nothing
    are never allowed.  The DFA is made on the host, lifted and compacted on ``device``, copied back once; states no token
    sequence reaches are dropped.  ValueError for what ``regex_to_dfa`` refuses, ids out of range, and a reachable state in
    which no token is allowed (the pattern cannot be spelled with this vocabulary)."""
    return compile_dfa(regex_to_dfa(pattern), vocab_bytes, eos_id, forbidden_ids, device, f"the pattern {pattern[:60]!r}")


def compile_json_schema(schema: dict, vocab_bytes: Sequence[bytes], eos_id: int, forbidden_ids=(), device="cuda") -> TokenAutomaton:
    """``compile_regex`` of ``json_schema_to_regex(schema)``: compact JSON documents of the schema."""
    return compile_dfa(regex_to_dfa(json_schema_to_regex(schema)), vocab_bytes, eos_id, forbidden_ids, device, "the JSON schema")


# ---------------------------------------------------------------- a tokenizer's vocabulary as bytes
def gpt2_unicode_to_byte() -> Dict[str, int]:
    """The inverse of GPT-2's byte-to-unicode table (byte-level BPE vocabularies print every byte as one character)."""
    keep = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[chr(b)] = b
        else:
            table[chr(256 + n)] = b
            n += 1
    return table


def vocab_bytes_of(tokenizer, vocab_size: int) -> List[bytes]:
    """The bytes of every id of a byte-level BPE ``tokenizers.Tokenizer`` (``get_vocab()`` and the GPT-2 table).  An id
    without an entry, or an entry with a character outside the table (an added special token's name), spells nothing."""
    get = getattr(tokenizer, "get_vocab", None)
    if get is None:
        raise ValueError("this tokenizer has no get_vocab(): pass vocab_bytes (one bytes object per token id)")
    table = gpt2_unicode_to_byte()
    out = [b""] * int(vocab_size)
    for text, i in get().items():
        if 0 <= i < vocab_size and all(c in table for c in text):
            out[i] = bytes(table[c] for c in text)
    return out
