"""Constrained decoding, the host side: a deterministic automaton over token ids that says which tokens a request may
produce next (``TokenAutomaton``), and the table form md_constrain_rows reads on the device (``pack``).  One mechanism
covers "one of these labels", "digits only", "never these ids", "at least n tokens before eos" and any token-level
grammar: the automaton is advanced by every token the request generates and the tokens its state forbids lose their
logits before the pick.  Host only: numpy, no torch, no kernels.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np

FREE = -1    # a next value: the request is unconstrained from here on
DEAD = -2    # a runtime state only (a forbidden token was consumed); never stored in a table
FORBID = -3  # a next value: the token may not be produced in this state


class TokenAutomaton:
    """States 0 .. S-1, start state 0.  ``edges[q]`` is the sorted list of distinct ``(token, next)`` pairs of state q and
    ``default[q]`` the next value of every token it does not list.  A next value is a state id, ``FREE`` or ``FORBID``.
    Immutable once made; one object may serve many requests (the engines pack each distinct object once).

    Two forms with one meaning: built from tuples (the constructor and the named constructors), or backed by the four
    arrays of the table form (``from_arrays``: what the grammar compiler makes, hundreds of thousands of edges), whose
    ``edges`` are materialised on first use only and whose ``validate`` / ``pack`` / ``next`` work on the arrays."""

    __slots__ = ("_edges", "default", "_arr")

    def __init__(self, edges: Sequence[Sequence[Tuple[int, int]]], default: Sequence[int]):
        if len(edges) != len(default) or len(default) == 0:
            raise ValueError("TokenAutomaton: one edge list and one default per state, at least one state")
        self._edges: Optional[Tuple[Tuple[Tuple[int, int], ...], ...]] = tuple(tuple((int(t), int(n)) for t, n in e) for e in edges)
        self.default: Tuple[int, ...] = tuple(int(d) for d in default)
        self._arr: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]] = None

    @classmethod
    def from_arrays(cls, row_ptr, default_next, edge_tok, edge_next) -> "TokenAutomaton":
        """The table form of ONE automaton (``PackedTable``'s arrays with start state 0): state q lists the edges
        ``row_ptr[q] .. row_ptr[q + 1]``.  The arrays are copied to int32 and kept; ValueError for shapes that do not fit
        together or a ``row_ptr`` that does not start at 0 or decreases (the values are ``validate``'s to check)."""
        as32 = lambda x: np.ascontiguousarray(np.array(x, dtype=np.int32).reshape(-1))
        row_ptr, default_next, edge_tok, edge_next = as32(row_ptr), as32(default_next), as32(edge_tok), as32(edge_next)
        s = default_next.shape[0]
        if s == 0 or row_ptr.shape[0] != s + 1:
            raise ValueError("from_arrays: row_ptr has one entry more than default_next, at least one state")
        if row_ptr[0] != 0 or np.any(np.diff(row_ptr) < 0) or row_ptr[-1] != edge_tok.shape[0] or edge_tok.shape != edge_next.shape:
            raise ValueError("from_arrays: row_ptr runs from 0 to the number of edges without decreasing, one next value per edge")
        a = cls.__new__(cls)
        a._edges, a.default, a._arr = None, tuple(default_next.tolist()), (row_ptr, default_next, edge_tok, edge_next)
        return a

    @property
    def edges(self) -> Tuple[Tuple[Tuple[int, int], ...], ...]:
        if self._edges is None:
            row_ptr, _, tok, nxt = self._arr
            pairs = list(zip(tok.tolist(), nxt.tolist()))
            self._edges = tuple(tuple(pairs[a:b]) for a, b in zip(row_ptr[:-1].tolist(), row_ptr[1:].tolist()))
        return self._edges

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """``(row_ptr, default_next, edge_tok, edge_next)``, int32: the kept arrays of the array-backed form, made from the
        tuples otherwise.  Not to be written to."""
        if self._arr is not None:
            return self._arr
        p = pack([self])
        return p.row_ptr, p.default_next, p.edge_tok, p.edge_next

    @property
    def n_states(self) -> int:
        return len(self.default)

    @property
    def n_edges(self) -> int:
        return int(self._arr[2].shape[0]) if self._arr is not None else sum(len(e) for e in self._edges)

    # ---- constructors
    @classmethod
    def from_states(cls, states: Sequence[Tuple[Mapping[int, int], int]]) -> "TokenAutomaton":
        """``states[q] = ({token: next, ...}, default)``."""
        return cls([sorted((int(t), int(n)) for t, n in m.items()) for m, _ in states], [d for _, d in states])

    @classmethod
    def allowed_tokens(cls, ids: Iterable[int]) -> "TokenAutomaton":
        """Only these ids, for the whole generation."""
        return cls.from_states([({int(t): 0 for t in ids}, FORBID)])

    @classmethod
    def banned_tokens(cls, ids: Iterable[int]) -> "TokenAutomaton":
        """Never these ids."""
        return cls.from_states([({int(t): FORBID for t in ids}, 0)])

    @classmethod
    def sequence(cls, ids: Sequence[int]) -> "TokenAutomaton":
        """Exactly these ids, then unconstrained."""
        ids = [int(t) for t in ids]
        if not ids:
            raise ValueError("sequence: at least one id")
        return cls.from_states([({t: (q + 1 if q + 1 < len(ids) else FREE)}, FORBID) for q, t in enumerate(ids)])

    @classmethod
    def choices(cls, seqs: Sequence[Sequence[int]], eos_id: int) -> "TokenAutomaton":
        """One of these id sequences followed by ``eos_id``, then unconstrained: a trie.  A choice that is a prefix of
        another keeps both continuations (eos, or the longer choice's next id)."""
        seqs = [[int(t) for t in s] for s in seqs]
        if not seqs or any(len(s) == 0 for s in seqs):
            raise ValueError("choices: at least one choice, none of them empty")
        if any(int(eos_id) in s for s in seqs):
            raise ValueError("choices: a choice contains eos_id")
        nodes: List[Dict[int, int]] = [{}]
        for s in seqs:
            q = 0
            for t in s:
                if t not in nodes[q]:
                    nodes.append({})
                    nodes[q][t] = len(nodes) - 1
                q = nodes[q][t]
            nodes[q][int(eos_id)] = FREE
        return cls.from_states([(m, FORBID) for m in nodes])

    @classmethod
    def min_tokens(cls, n: int, eos_id: int) -> "TokenAutomaton":
        """No ``eos_id`` among the first ``n`` ids."""
        n = int(n)
        if n < 1:
            raise ValueError("min_tokens: n >= 1")
        return cls.from_states([({int(eos_id): FORBID}, q + 1 if q + 1 < n else FREE) for q in range(n)])

    # ---- semantics
    def next(self, state: int, token: int) -> int:
        """The next value of ``token`` in ``state`` (a state id, FREE or FORBID)."""
        if self._arr is not None:
            row_ptr, _, tok, nxt = self._arr
            lo, hi = int(row_ptr[state]), int(row_ptr[state + 1])
            i = lo + int(np.searchsorted(tok[lo:hi], token))
            return int(nxt[i]) if i < hi and tok[i] == token else self.default[state]
        for t, n in self._edges[state]:
            if t == token:
                return n
        return self.default[state]

    def walk(self, ids: Iterable[int], state: int = 0) -> int:
        """The state after consuming ``ids`` from ``state``: a state id, ``FREE``, or ``DEAD`` at the first forbidden id."""
        for t in ids:
            if state < 0:
                return state
            state = self.next(state, int(t))
            if state == FORBID:
                return DEAD
        return state

    def validate(self, vocab: int, suppress_id: int = -1) -> None:
        """ValueError for edges that are not sorted or not unique, a token outside [0, vocab), a next value that is no
        state, FREE or FORBID, and a state in which no token other than ``suppress_id`` (which the pick leaves out on
        its own) is allowed: its pick would see a row of -inf alone."""
        s = self.n_states
        if self._arr is not None:
            return self._validate_arrays(int(vocab), int(suppress_id))
        for q, (edges, d) in enumerate(zip(self._edges, self.default)):
            toks = [t for t, _ in edges]
            if any(b <= a for a, b in zip(toks, toks[1:])):
                raise ValueError(f"state {q}: edges must be sorted by token and distinct")
            if toks and (toks[0] < 0 or toks[-1] >= vocab):
                raise ValueError(f"state {q}: a token outside [0, {vocab})")
            for n in [n for _, n in edges] + [d]:
                if not (0 <= n < s or n in (FREE, FORBID)):
                    raise ValueError(f"state {q}: next value {n} is no state of {s}, FREE or FORBID")
            if d == FORBID:
                live = [t for t, n in edges if n != FORBID and t != suppress_id]
                ok = bool(live)
            else:
                gone = sum(1 for t, n in edges if n == FORBID or t == suppress_id)
                gone += int(0 <= suppress_id < vocab and suppress_id not in toks)
                ok = gone < vocab
            if not ok:
                raise ValueError(f"state {q} allows no token" + (f" other than {suppress_id}" if suppress_id >= 0 else ""))

    def _validate_arrays(self, vocab: int, suppress_id: int) -> None:
        """``validate`` for the array-backed form: the same checks in the same order per state, the first failing state's
        message; no per-edge Python."""
        row_ptr, dflt, tok, nxt = self._arr
        s, e = self.n_states, tok.shape[0]
        state_of = np.repeat(np.arange(s), np.diff(row_ptr))
        big = s + 1
        first = lambda bad_states: int(bad_states.min()) if bad_states.size else big
        inner = np.ones(e, dtype=bool)  # edges that have a predecessor in their own state
        inner[row_ptr[:-1][row_ptr[:-1] < e]] = False
        unsorted = first(state_of[1:][inner[1:] & (tok[1:] <= tok[:-1])]) if e > 1 else big
        # sorted states: the first and last token bound the rest
        outside = first(state_of[(tok < 0) | (tok >= vocab)])
        is_next = lambda n: ((n >= 0) & (n < s)) | (n == FREE) | (n == FORBID)
        bad_next = min(first(state_of[~is_next(nxt)]), first(np.flatnonzero(~is_next(dflt))))
        gone_edge = (nxt == FORBID) | (tok == suppress_id)
        n_gone = np.bincount(state_of[gone_edge], minlength=s)
        n_live = np.diff(row_ptr) - n_gone
        has_sup = np.bincount(state_of[tok == suppress_id], minlength=s) > 0
        gone_allow = n_gone + ((0 <= suppress_id < vocab) & ~has_sup)
        ok = np.where(dflt == FORBID, n_live > 0, gone_allow < vocab)
        none_left = first(np.flatnonzero(~ok))
        q = min(unsorted, outside, bad_next, none_left)
        if q == big:
            return
        if q == unsorted:
            raise ValueError(f"state {q}: edges must be sorted by token and distinct")
        if q == outside:
            raise ValueError(f"state {q}: a token outside [0, {vocab})")
        if q == bad_next:
            lo, hi = int(row_ptr[q]), int(row_ptr[q + 1])
            vals = np.concatenate([nxt[lo:hi], dflt[q : q + 1]])
            n = int(vals[~is_next(vals)][0])
            raise ValueError(f"state {q}: next value {n} is no state of {s}, FREE or FORBID")
        raise ValueError(f"state {q} allows no token" + (f" other than {suppress_id}" if suppress_id >= 0 else ""))


@dataclass(frozen=True)
class PackedTable:
    """Several automata as one table (md_constrain_rows): state q lists ``edge_tok`` / ``edge_next``
    ``[row_ptr[q], row_ptr[q + 1])``; ``starts[i]`` is the start state of automaton i in it."""

    row_ptr: np.ndarray       # int32 [S + 1]
    default_next: np.ndarray  # int32 [S]
    edge_tok: np.ndarray      # int32 [E]
    edge_next: np.ndarray     # int32 [E]
    starts: Tuple[int, ...]

    @property
    def n_states(self) -> int:
        return int(self.default_next.shape[0])

    @property
    def n_edges(self) -> int:
        return int(self.edge_tok.shape[0])


def pack(automata: Sequence[TokenAutomaton], state0: int = 0, edge0: int = 0) -> PackedTable:
    """Concatenate ``automata`` into one table; state ids are rebased (automaton i's state q becomes ``starts[i] + q``),
    FREE and FORBID stay.  ``state0`` / ``edge0``: the table continues one that already holds that many states and edges
    (``row_ptr`` then starts at ``edge0`` and ``starts`` at ``state0``)."""
    row_ptr, default_next, edge_tok, edge_next, starts = [edge0], [], [], [], []
    for a in automata:
        base = state0 + len(default_next)
        starts.append(base)
        rebase = lambda n: n + base if n >= 0 else n
        if a._arr is not None:  # array-backed: whole arrays at a time (lists of ints, like the tuple form's)
            a_ptr, a_default, a_tok, a_next = a._arr
            e0 = edge0 + len(edge_tok)
            edge_tok += a_tok.tolist()
            edge_next += np.where(a_next >= 0, a_next + base, a_next).tolist()
            default_next += np.where(a_default >= 0, a_default + base, a_default).tolist()
            row_ptr += (a_ptr[1:] + e0).tolist()
            continue
        for edges, d in zip(a._edges, a.default):
            edge_tok += [t for t, _ in edges]
            edge_next += [rebase(n) for _, n in edges]
            default_next.append(rebase(d))
            row_ptr.append(edge0 + len(edge_tok))
    as32 = lambda x: np.asarray(x, dtype=np.int32)
    return PackedTable(as32(row_ptr), as32(default_next), as32(edge_tok), as32(edge_next), tuple(starts))


def check_constraints(constraints, n: int, vocab: int, suppress_id: int) -> Optional[List[Optional[TokenAutomaton]]]:
    """The ``constraints`` argument of the generation calls -- None, one ``TokenAutomaton`` for every row, or a list with
    one entry per row (None: the row is free) -> one entry per row, or None when every row is free.  ValueError for a
    list that is not ``n`` long, an entry that is neither, and whatever ``validate(vocab, suppress_id)`` refuses: host
    values only, before any GPU work."""
    if constraints is None:
        return None
    if isinstance(constraints, TokenAutomaton):
        rows = [constraints] * n
    elif isinstance(constraints, (list, tuple)):
        rows = list(constraints)
        if len(rows) != n:
            raise ValueError(f"constraints: {len(rows)} entries for {n} rows (one TokenAutomaton, or one entry per row)")
    else:
        raise ValueError(f"constraints must be a TokenAutomaton or a list of them (None: a free row), not {constraints!r}")
    seen = set()
    for a in rows:
        if a is None or id(a) in seen:
            continue
        if not isinstance(a, TokenAutomaton):
            raise ValueError(f"constraints: an entry must be a TokenAutomaton or None, not {a!r}")
        a.validate(vocab, suppress_id)
        seen.add(id(a))
    return rows if seen else None


def refuse_constraints(settings: Optional[dict], where: str) -> None:
    """An entry point that does not serve constraints: ValueError naming ``where`` when ``settings`` carries one."""
    c = (settings or {}).get("constraints")
    if c is not None and not (isinstance(c, (list, tuple)) and all(x is None for x in c)):
        raise ValueError(f"constraints are not served by {where}")
    if grammar_of(settings) is not None:  # a pattern or a schema is a constraint yet to be compiled
        raise ValueError(f"constraints are not served by {where}")


GRAMMAR_KEYS = ("regex", "json_schema")  # settings that compile to ``constraints`` (moondream_amd/grammar.py)


def grammar_of(settings: Optional[Mapping], constraint_key: str = "constraints") -> Optional[Tuple[str, object]]:
    """``settings["regex"]`` / ``settings["json_schema"]`` -> ``(key, value)``, None without either.  ValueError for both at
    once and for one of them together with ``settings[constraint_key]``: one constraint per call, given one way."""
    st = settings or {}
    found = [(k, st[k]) for k in GRAMMAR_KEYS if st.get(k) is not None]
    if not found:
        return None
    if len(found) > 1:
        raise ValueError("regex and json_schema are mutually exclusive: one grammar per call")
    if st.get(constraint_key) is not None:
        raise ValueError(f"{found[0][0]} and {constraint_key} are mutually exclusive: {found[0][0]} compiles to the call's constraint")
    return found[0]


def pow2_at_least(n: int, floor: int = 16) -> int:
    """Table capacities are powers of two, so that calls with tables of similar size share captured graphs."""
    c = floor
    while c < n:
        c *= 2
    return c
