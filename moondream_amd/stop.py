"""Stop strings and stop token ids, the host side: one request's end condition (``StopSet``), its byte-level
Aho-Corasick DFA, the table form md_stop_rows reads on the device (``pack``), the argument checks of the generation calls
(``check_stops``) and the numpy restatement of the kernel's rule (``walk``).

The rule, per generated token v of a row that has not matched yet: if v is one of the row's stop ids the row ends AT that
token (the token is excluded, like eos); otherwise v's bytes are walked through the DFA and the row ends at the FIRST byte
after which some stop string is a suffix of the generated text -- the earliest end; among the strings ending at that byte,
the longest.  ``at`` is the index of that token among the generated ones, ``keep`` the number of bytes of generated text
in front of the matched string (in front of the token, for an id), ``which`` the string's index, or ``len(strings) + j``
for the j-th stop id.  Host only: numpy, no torch, no kernels.
"""
from __future__ import annotations

import operator
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .constraint import pow2_at_least

MD_STOP_STATES_MAX = 4096  # include/moondream_hip.h: the most DFA states one table holds
STOP_STRINGS_MAX = 16
STOP_IDS_MAX = 16          # MD_STOP_IDS_MAX
STOP_BYTES_MAX = 64
NO_STOP = -1               # a row's state: it has no stop set and the kernel skips it

STOP_SETTINGS = ("stop", "stop_token_ids", "include_stop_str_in_output")


@dataclass(frozen=True)
class StopSet:
    """One request's stop condition: ``strings`` (0..16 str, each 1..64 bytes as UTF-8) and ``token_ids`` (0..16 ints).
    Immutable and hashable: equal stop sets share their states in a packed table."""

    strings: Tuple[str, ...] = ()
    token_ids: Tuple[int, ...] = ()

    def __post_init__(self):
        object.__setattr__(self, "strings", tuple(self.strings))
        object.__setattr__(self, "token_ids", tuple(int(t) for t in self.token_ids))

    def __bool__(self) -> bool:
        return bool(self.strings or self.token_ids)

    @property
    def patterns(self) -> Tuple[bytes, ...]:
        return tuple(s.encode("utf-8") for s in self.strings)

    def named(self, which: int):
        """The string or id a result's ``which`` stands for."""
        return self.strings[which] if which < len(self.strings) else self.token_ids[which - len(self.strings)]

    def dfa(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(trans uint16 [S, 256], match_len uint16 [S], match_id int32 [S])``: the complete Aho-Corasick automaton
        of ``strings`` over bytes, goto and failure links folded into ``trans``, state 0 the root.  ``match_len[q]`` is
        the length of the longest string that is a suffix of q's path (0: none) and ``match_id[q]`` its index (-1).
        Of two equal strings the first is named.  A set without strings is the root alone."""
        goto: List[Dict[int, int]] = [{}]
        own_len, own_id = [0], [-1]
        for i, p in enumerate(self.patterns):
            q = 0
            for c in p:
                if c not in goto[q]:
                    goto.append({})
                    own_len.append(0)
                    own_id.append(-1)
                    goto[q][c] = len(goto) - 1
                q = goto[q][c]
            if own_id[q] < 0:
                own_len[q], own_id[q] = len(p), i
        s = len(goto)
        trans = np.zeros((s, 256), dtype=np.int64)
        fail = [0] * s
        queue = []
        for c, q in goto[0].items():
            trans[0, c] = q
            queue.append(q)
        for q in queue:  # breadth first: a state's failure state is complete before the state is
            f = fail[q]
            trans[q] = trans[f]
            if own_id[q] < 0:  # a terminal's own string is its whole path: the longest suffix there is
                own_len[q], own_id[q] = own_len[f], own_id[f]
            for c, nxt in goto[q].items():
                fail[nxt] = int(trans[f, c])
                trans[q, c] = nxt
                queue.append(nxt)
        return trans.astype(np.uint16), np.asarray(own_len, dtype=np.uint16), np.asarray(own_id, dtype=np.int32)


@dataclass(frozen=True)
class PackedStops:
    """Several stop sets' automata as one table (md_stop_rows): ``starts[i]`` is the root of stop set i in it."""

    trans: np.ndarray      # uint16 [S, 256]
    match_len: np.ndarray  # uint16 [S]
    match_id: np.ndarray   # int32 [S]
    starts: Tuple[int, ...]

    @property
    def n_states(self) -> int:
        return int(self.match_len.shape[0])


def pack(stop_sets: Sequence[StopSet], state0: int = 0) -> PackedStops:
    """Concatenate the automata of ``stop_sets`` into one table; state ids are rebased (set i's state q becomes
    ``starts[i] + q``).  Sets with equal strings share their states (the ids play no part in the automaton).
    ``state0``: the table continues one that already holds that many states."""
    trans, mlen, mid, starts, seen = [], [], [], [], {}
    n = 0
    for s in stop_sets:
        if s.strings in seen:
            starts.append(seen[s.strings])
            continue
        t, l, i = s.dfa()
        base = state0 + n
        seen[s.strings] = base
        starts.append(base)
        if base + t.shape[0] > 65535:
            raise ValueError(f"stop: {base + t.shape[0]} states do not fit the table's 16-bit entries")
        trans.append((t.astype(np.int64) + base).astype(np.uint16))
        mlen.append(l)
        mid.append(i)
        n += t.shape[0]
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty
    return PackedStops(cat(trans, np.zeros((0, 256), dtype=np.uint16)), cat(mlen, np.zeros(0, dtype=np.uint16)),
                       cat(mid, np.zeros(0, dtype=np.int32)), tuple(starts))


def padded(table: PackedStops, state_cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """The table's three arrays at a capacity of ``state_cap`` states (None: ``pow2_at_least(n_states)``), the states past
    its own sending every byte to state 0 of the table and matching nothing -> ``(trans, match_len, match_id, state_cap)``."""
    cap = pow2_at_least(table.n_states) if state_cap is None else int(state_cap)
    assert cap >= table.n_states
    trans = np.zeros((cap, 256), dtype=np.uint16)
    match_len, match_id = np.zeros(cap, dtype=np.uint16), np.full(cap, -1, dtype=np.int32)
    trans[: table.n_states], match_len[: table.n_states], match_id[: table.n_states] = table.trans, table.match_len, table.match_id
    return trans, match_len, match_id, cap


def _strings_of(entry, what: str = "stop") -> Tuple[str, ...]:
    """One row's strings: None, a str or a list of str -> the validated tuple."""
    if entry is None:
        return ()
    items = [entry] if isinstance(entry, str) else entry
    if not isinstance(items, (list, tuple)):
        raise ValueError(f"{what} must be a str or a list of str (None: no stop strings), not {entry!r}")
    if len(items) > STOP_STRINGS_MAX:
        raise ValueError(f"{what}: {len(items)} strings; at most {STOP_STRINGS_MAX} per request")
    for s in items:
        if not isinstance(s, str):
            raise ValueError(f"{what}: a stop string must be a str, not {s!r}")
        if s == "":
            raise ValueError(f"{what}: an empty stop string")
        if len(s.encode("utf-8")) > STOP_BYTES_MAX:
            raise ValueError(f"{what}: {s[:24]!r}... is {len(s.encode('utf-8'))} bytes as UTF-8; at most {STOP_BYTES_MAX}")
    return tuple(items)


def _ids_of(entry, vocab: int, what: str = "stop_token_ids") -> Tuple[int, ...]:
    """One row's stop ids: None or a list of ints -> the validated tuple."""
    if entry is None:
        return ()
    if not isinstance(entry, (list, tuple)):
        raise ValueError(f"{what} must be a list of token ids (None: no stop ids), not {entry!r}")
    if len(entry) > STOP_IDS_MAX:
        raise ValueError(f"{what}: {len(entry)} ids; at most {STOP_IDS_MAX} per request")
    out = []
    for t in entry:
        try:
            v = None if isinstance(t, bool) else operator.index(t)
        except TypeError:
            v = None
        if v is None:
            raise ValueError(f"{what}: a stop id must be an int, not {t!r}")
        if not 0 <= v < vocab:
            raise ValueError(f"{what}: id {v} is outside the vocabulary [0, {vocab})")
        out.append(v)
    return tuple(out)


def check_stops(stop, stop_token_ids, n: int, vocab: int) -> Optional[List[Optional[StopSet]]]:
    """The ``stop`` / ``stop_token_ids`` arguments of the generation calls -> one ``StopSet`` or None per row, or None
    when every row has none.  ``stop``: None, one str, a list of str alone (call-wide: every row takes them all), or a
    list with one entry per row, each None, a str or a list of str (a list that holds a None or a list is read per row).
    ``stop_token_ids``: None, a flat list of ints (call-wide) or one list (or None) per row.  ValueError for an empty
    string, a string of more than 64 bytes as UTF-8, more than 16 entries, an entry that is no str / no int, an id outside
    ``[0, vocab)``, a per-row list that is not ``n`` long, and stop sets that need more than ``MD_STOP_STATES_MAX`` states
    in all: host values only, before any GPU work."""
    per_row = lambda x: isinstance(x, (list, tuple)) and any(e is None or isinstance(e, (list, tuple)) for e in x)
    if per_row(stop):
        if len(stop) != n:
            raise ValueError(f"stop: {len(stop)} entries for {n} rows (one str, a list of str for every row, or one entry per row)")
        strings = [_strings_of(e) for e in stop]
    else:
        strings = [_strings_of(stop)] * n
    if per_row(stop_token_ids):
        if len(stop_token_ids) != n:
            raise ValueError(f"stop_token_ids: {len(stop_token_ids)} entries for {n} rows (a list of ids for every row, or one list per row)")
        ids = [_ids_of(e, vocab) for e in stop_token_ids]
    else:
        ids = [_ids_of(stop_token_ids, vocab)] * n
    made: Dict[Tuple, StopSet] = {}
    rows = [made.setdefault((s, i), StopSet(s, i)) if (s or i) else None for s, i in zip(strings, ids)]
    if not made:
        return None
    states = pack(list(made.values())).n_states
    if states > MD_STOP_STATES_MAX:
        raise ValueError(f"stop: the call's stop strings need {states} states; at most {MD_STOP_STATES_MAX}")
    return rows


def check_include(include_stop_str_in_output) -> bool:
    if not isinstance(include_stop_str_in_output, bool):
        raise ValueError(f"include_stop_str_in_output must be a bool, not {include_stop_str_in_output!r}")
    return include_stop_str_in_output


def stops_of(settings: Optional[dict]) -> dict:
    """The stop entries of a ``settings`` dict as keyword arguments of the generation calls (absent: none)."""
    st = settings or {}
    return {"stop": st.get("stop"), "stop_token_ids": st.get("stop_token_ids"),
            "include_stop_str_in_output": st.get("include_stop_str_in_output", False)}


def refuse_stops(settings: Optional[dict], where: str) -> None:
    """An entry point that does not serve stops: ValueError naming ``where`` when ``settings`` carries a stop string or a
    stop id (per-row lists of None alone carry none)."""
    st = settings or {}
    for name in STOP_SETTINGS[:2]:
        x = st.get(name)
        if isinstance(x, (list, tuple)):
            x = [e for e in x if e is not None and e != [] and e != ()]
        if x is not None and x != []:
            raise ValueError(f"stop / stop_token_ids are not served by {where}")


@dataclass(frozen=True)
class Finish:
    """How a row ended.  ``reason``: "stop" (a stop string or stop id), "eos" or "length".  ``stop``: the matched string
    or id (None unless "stop").  ``text_bytes``: when a STRING matched, the number of bytes of the row's generated text
    that are its output -- those in front of the string, plus the string with ``include_stop_str_in_output``; otherwise None."""

    reason: str
    stop: object = None
    text_bytes: Optional[int] = None


def finish_of(stop_set: Optional[StopSet], at: int, keep: int, which: int, n_generated: int, include: bool,
              eos_at: Optional[int]) -> Tuple[int, Finish]:
    """A row's result triple, the number of tokens it generated and the index of its first eos (None: none) -> ``(the
    number of ids the row returns, its Finish)``.  The ids end at the earliest of: the eos (excluded), a stop id
    (excluded), the token in which a stop string completed (included: a token cannot be split)."""
    if stop_set is not None and at >= 0 and at < n_generated and (eos_at is None or at < eos_at):
        if which < len(stop_set.strings):
            s = stop_set.strings[which]
            return at + 1, Finish("stop", s, keep + (len(s.encode("utf-8")) if include else 0))
        return at, Finish("stop", stop_set.named(which))
    if eos_at is not None and eos_at < n_generated:
        return eos_at, Finish("eos")
    return n_generated, Finish("length")


def cut_text(token_bytes: Sequence[bytes], finish: Finish) -> bytes:
    """The bytes of a row's ids cut to ``finish.text_bytes`` (a row that did not stop on a string: all of them)."""
    data = b"".join(token_bytes)
    return data if finish.text_bytes is None else data[: finish.text_bytes]


def walk(table: PackedStops, start_state: int, token_bytes: Sequence[bytes], tokens: Optional[Sequence[int]] = None,
         stop_ids: Sequence[int] = (), n_strings: int = 0, state: Optional[dict] = None) -> Tuple[int, int, int]:
    """md_stop_rows restated: feed the generated tokens, whose bytes are ``token_bytes[i]`` (and whose ids, for the stop
    ids, are ``tokens[i]``), to one row that starts in ``start_state`` -> ``(at, keep, which)``, ``at`` -1 without a match.
    ``n_strings``: the number of strings of the row's stop set, the ``which`` of its first stop id (``id_base``).
    ``state``: a dict carrying the row's six words between calls (``state, n_tok, n_bytes, at, keep, which``), as the
    device arrays carry them from launch to launch; None: a fresh row."""
    st = state if state is not None else {}
    st.setdefault("state", int(start_state))
    for k, v in (("n_tok", 0), ("n_bytes", 0), ("at", -1), ("keep", 0), ("which", -1)):
        st.setdefault(k, v)
    if st["state"] < 0:
        return st["at"], st["keep"], st["which"]
    stop_ids = list(stop_ids)[:STOP_IDS_MAX]
    for i, data in enumerate(token_bytes):
        if st["at"] < 0:
            v = None if tokens is None else int(tokens[i])
            if v is not None and v in stop_ids:
                st["at"], st["keep"], st["which"] = st["n_tok"], st["n_bytes"], int(n_strings) + stop_ids.index(v)
            else:
                q = st["state"]
                for j, c in enumerate(bytes(data)):
                    q = int(table.trans[q, c])
                    if table.match_len[q] > 0:
                        st["at"], st["keep"], st["which"] = st["n_tok"], st["n_bytes"] + j + 1 - int(table.match_len[q]), int(table.match_id[q])
                        break
                st["state"] = q
        st["n_tok"] += 1
        st["n_bytes"] += len(data)
    return st["at"], st["keep"], st["which"]
