"""A call's decoding settings as one value: parsed and validated once, at the public entry point, then carried to the
place that builds the device records (``MoondreamModel._prepare_sequences``; the continuous engine's ``Request``).
``RowSettings`` is what one request decodes with, ``CallSettings`` the rows of a call in the caller's order with what is
call-wide.  Host values only, no torch: the validators are the ones of decode_loop.py, constraint.py and beam.py, and
their messages are the contract."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Sequence, Tuple

from .beam import beams_of, refuse_beams
from .constraint import TokenAutomaton, grammar_of, refuse_constraints
from .decode_loop import (FILTER_NEUTRAL, PENALTY_NEUTRAL, check_filters, check_penalties, check_top_logprobs, filters_of,
                          penalties_of, refuse_filters, refuse_penalties)
from .stop import StopSet, check_include, check_stops, refuse_stops, stops_of

DEFAULT_MAX_TOKENS = 768   # the reference's defaults (moondream.py:50-53), what a string-API ``settings`` dict leaves out
DEFAULT_TEMPERATURE = 0.5
DEFAULT_TOP_P = 0.3


@dataclass(frozen=True)
class RowSettings:
    """What one request decodes with.  ``temperature`` 0: greedy.  ``top_k`` / ``min_p``: the cuts of a sampled row (0:
    off).  ``penalties``: (repetition, presence, frequency).  ``constraint``: its automaton, None: free.  ``stop``: its
    stop strings and stop ids (moondream_amd/stop.py), None: it ends on eos and the token budget alone."""

    temperature: float = 0.0
    top_p: float = DEFAULT_TOP_P
    top_k: int = 0
    min_p: float = 0.0
    penalties: Tuple[float, float, float] = PENALTY_NEUTRAL
    constraint: Optional[TokenAutomaton] = None
    stop: Optional[StopSet] = None

    @property
    def sampled(self) -> bool:
        return self.temperature != 0

    @property
    def filtered(self) -> bool:
        """Sampled with a non-neutral cut (a greedy row ignores the cuts)."""
        return self.sampled and (self.top_k, self.min_p) != FILTER_NEUTRAL

    @property
    def penalised(self) -> bool:
        return self.penalties != PENALTY_NEUTRAL

    @property
    def constrained(self) -> bool:
        return self.constraint is not None


def _per_row(x, n: int) -> list:
    return list(x) if isinstance(x, (list, tuple)) else [x] * n


@dataclass(frozen=True)
class CallSettings:
    """The settings of a call over ``len(rows)`` rows, in the caller's order, and what is call-wide: ``max_tokens``,
    ``generator``, the LoRA ``variant`` / ``variants``, ``top_logprobs`` (k; 0: none) and ``beams`` (``beams_of``'s triple,
    None: no beam search).  ``penalties`` / ``filters`` / ``constraints`` are what ``check_penalties`` / ``check_filters``
    / ``check_constraints`` return for the call -- one entry per row, or None when every row is neutral: the tests that
    decide whether a launch exists at all (a call with all-neutral values is the call without the arguments).  ``stops``
    likewise (``check_stops``); ``include_stop_str`` and ``stop_vocab_bytes`` (the bytes of every id, None: the model's
    tokenizer's) are call-wide and matter with stops only."""

    rows: Tuple[RowSettings, ...]
    max_tokens: int = DEFAULT_MAX_TOKENS
    generator: Any = None
    variant: Optional[str] = None
    variants: Optional[Sequence[Optional[str]]] = None
    top_logprobs: int = 0
    beams: Optional[Tuple[int, float, bool]] = None
    include_stop_str: bool = False
    stop_vocab_bytes: Any = None

    @property
    def temperature(self):
        """Of a call whose rows all sample alike (the lockstep and sequential calls)."""
        return self.rows[0].temperature

    @property
    def top_p(self):
        return self.rows[0].top_p

    @property
    def penalties(self) -> Optional[List[Tuple[float, float, float]]]:
        return [r.penalties for r in self.rows] if any(r.penalised for r in self.rows) else None

    @property
    def filters(self) -> Optional[List[Tuple[int, float]]]:
        return None if all((r.top_k, r.min_p) == FILTER_NEUTRAL for r in self.rows) else [(r.top_k, r.min_p) for r in self.rows]

    @property
    def constraints(self) -> Optional[List[Optional[TokenAutomaton]]]:
        return [r.constraint for r in self.rows] if any(r.constrained for r in self.rows) else None

    @property
    def stops(self) -> Optional[List[Optional[StopSet]]]:
        return [r.stop for r in self.rows] if any(r.stop is not None for r in self.rows) else None

    def reorder(self, order: Sequence[int]) -> "CallSettings":
        """Row r of the result is row ``order[r]`` of this record: the rows in slot order."""
        return CallSettings(tuple(self.rows[i] for i in order), self.max_tokens, self.generator, self.variant, self.variants,
                            self.top_logprobs, self.beams, self.include_stop_str, self.stop_vocab_bytes)

    @classmethod
    def of(cls, n: int, check_automata: Callable[[Any, int], Optional[list]], *, max_tokens=DEFAULT_MAX_TOKENS,
           temperature=0.0, top_p=DEFAULT_TOP_P, generator=None, variant=None, variants=None, return_logprobs: bool = False, top_logprobs=None,
           repetition_penalty=None, presence_penalty=None, frequency_penalty=None, constraints=None, top_k=None, min_p=None,
           regex=None, json_schema=None, vocab_bytes=None, beam_settings: Optional[dict] = None,
           compile_grammar: Optional[Callable[[str, Any, Any], TokenAutomaton]] = None, stop=None, stop_token_ids=None,
           include_stop_str_in_output=False, vocab_size: Optional[int] = None) -> "CallSettings":
        """From the keyword arguments of ``batch_generate_ids`` (and the ``regex`` / ``json_schema`` / beam entries a
        ``settings`` dict may carry beside them), for ``n`` rows.  ``check_automata(constraints, n)``: ``check_constraints``
        with the model's vocabulary size and suppressed id (``MoondreamModel._check_automata``), asked only when there are
        constraints.  ``temperature`` / ``top_p``: one value, or one per row; they are taken as given (the calls that
        bound them do so themselves).  Every error is the validator's own.  With several invalid settings the first of
        this order is reported: ``regex`` / ``json_schema`` / ``constraints`` given together (``grammar_of``), the
        penalties, ``top_k`` / ``min_p``, ``top_logprobs``, ``constraints``, the beam settings -- and last, after every
        host-only check, the one step that runs on the device: ``compile_grammar(kind, value, vocab_bytes)`` (the model's
        ``_grammar_constraint``) turns a ``regex`` / ``json_schema`` into the automaton of every row.  A call that asks
        for beam search compiles nothing: that route refuses constraints.  ``stop`` / ``stop_token_ids`` /
        ``include_stop_str_in_output``: ``check_stops`` over a vocabulary of ``vocab_size`` ids, judged after the beam settings
        (beam search does not serve them); ``vocab_bytes`` also spells the ids for the stop strings."""
        found = grammar_of(dict(regex=regex, json_schema=json_schema, constraints=constraints))
        pens = check_penalties(repetition_penalty, presence_penalty, frequency_penalty, n) or [PENALTY_NEUTRAL] * n
        cuts = check_filters(top_k, min_p, n) or [FILTER_NEUTRAL] * n
        k = check_top_logprobs(top_logprobs, return_logprobs)
        automata = (constraints is not None and check_automata(constraints, n)) or [None] * n
        beams = beams_of(beam_settings)
        if found is not None and beams is None:
            automata = [compile_grammar(*found, vocab_bytes)] * n
        include = check_include(include_stop_str_in_output)
        stops = check_stops(stop, stop_token_ids, n, 2 ** 31 if vocab_size is None else int(vocab_size)) or [None] * n
        if beams is not None and any(s is not None for s in stops):
            raise ValueError("stop / stop_token_ids are not served by beam search (num_beams > 1)")
        temps, tps = _per_row(temperature, n), _per_row(top_p, n)
        rows = tuple(RowSettings(temps[i], tps[i], cuts[i][0], cuts[i][1], pens[i], automata[i], stops[i]) for i in range(n))
        return cls(rows, max_tokens, generator, variant, variants, k, beams, include, vocab_bytes)

    @classmethod
    def of_settings(cls, settings: Optional[dict], n: int, check_automata: Callable[[Any, int], Optional[list]],
                    compile_grammar: Optional[Callable[[str, Any, Any], TokenAutomaton]] = None,
                    vocab_size: Optional[int] = None) -> "CallSettings":
        """From a string-API ``settings`` dict, with the REFERENCE'S defaults (moondream.py:50-53, read at :447-457):
        max_tokens 768, temperature 0.5, top_p 0.3.  ``generator`` (an extension) seeds the draws; ``{"temperature": 0}`` is
        greedy.  The penalties, ``constraints`` / ``regex`` / ``json_schema`` (with ``vocab_bytes``), ``top_k`` / ``min_p``
        and the beam settings are extensions too: one value or one per row, neutral when absent; so are ``stop`` /
        ``stop_token_ids`` / ``include_stop_str_in_output``.  Errors and their order: ``of``'s."""
        st = settings or {}
        return cls.of(n, check_automata, max_tokens=st.get("max_tokens", DEFAULT_MAX_TOKENS),
                      temperature=st.get("temperature", DEFAULT_TEMPERATURE), top_p=st.get("top_p", DEFAULT_TOP_P),
                      generator=st.get("generator"), variant=st.get("variant"), variants=st.get("variants"),
                      constraints=st.get("constraints"), regex=st.get("regex"), json_schema=st.get("json_schema"),
                      vocab_bytes=st.get("vocab_bytes"), beam_settings=settings, compile_grammar=compile_grammar,
                      vocab_size=vocab_size, **penalties_of(settings), **filters_of(settings), **stops_of(settings))


FAMILIES = ("penalties", "constraints", "filters", "beams", "spatial_refs", "stops")  # what an entry point may not serve


def refuse_settings(settings: Optional[dict], where, families: Sequence[str] = FAMILIES[:4], n: int = 1, spatial_refs=None) -> None:
    """An entry point that does not serve some families of settings: each family of ``families``, in that order, is
    refused by its own function (``refuse_penalties``, ``refuse_constraints``, ``refuse_filters``, ``refuse_beams``,
    ``refuse_spatial_refs``, ``refuse_stops``: ValueError naming the place when ``settings`` carries a non-neutral value of the family, and
    the validators' errors for a value that is none).  ``where``: the wording of the place, or a dict of wordings per
    family (key None: the others').  ``n``: the call's rows, for the penalties.  ``spatial_refs``: the call's argument,
    beside ``settings["spatial_refs"]``."""
    def refuse_refs(w):
        from .spatial import refs_of, refuse_spatial_refs  # (here: that module's records are torch's)

        refuse_spatial_refs(refs_of(settings, spatial_refs), w)

    refuse = {"penalties": lambda w: refuse_penalties(settings, w, n), "constraints": lambda w: refuse_constraints(settings, w),
              "filters": lambda w: refuse_filters(settings, w), "beams": lambda w: refuse_beams(settings, w),
              "spatial_refs": refuse_refs, "stops": lambda w: refuse_stops(settings, w)}
    for family in families:
        refuse[family](where if isinstance(where, str) else where.get(family, where.get(None)))
