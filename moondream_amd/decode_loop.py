"""What the lockstep loop (``MoondreamModel._decode_greedy_impl``) and the continuous engine (``ContinuousEngine._step``)
share: the description of a chunk of consecutive decode steps over fixed buffers, and the one runner that launches it.
``run_chunk`` holds the only step body of the package -- decode step (or, for a reasoning query, the reasoning step), then
the optional penalty launch, then the optional constraint launch, then the optional sampling pick, then the optional
stop-matcher launch, then the optional log-probability launch and the optional top-k launch; or, for beam search, decode step, beam selection, KV tail copy -- and the only decode graph key.  No torch here: the runner moves no data, it orders launches."""
from __future__ import annotations

import math
import numbers
import operator
from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Tuple


TOPK_MAX = 32  # MD_TOPK_MAX of include/moondream_hip.h


def check_top_logprobs(top_logprobs: Optional[int], with_logprobs: bool) -> int:
    """The ``top_logprobs`` argument of the generation and scoring calls -> k (0: none).  ValueError for a k outside
    1 .. TOPK_MAX, or one asked for without the log-probabilities it extends: host values only, before any GPU work."""
    if top_logprobs is None:
        return 0
    try:
        k = operator.index(top_logprobs)
    except TypeError:
        k = -1
    if k == 0:
        return 0
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f"top_logprobs must be an integer in 1 .. {TOPK_MAX} (0 / None: none), not {top_logprobs!r}")
    if not with_logprobs:
        raise ValueError("top_logprobs extends the log-probabilities: it needs return_logprobs=True / logprobs=True")
    return k


def check_score_settings(settings: Optional[dict], n_bins: int) -> Optional[int]:
    """The ``return_scores`` / ``score_window`` entries of a detect / point ``settings`` dict -> the window (None: no scores).
    ValueError for a ``return_scores`` that is not a bool, a ``score_window`` that is not an integer in 0 .. n_bins - 1, or one
    given without ``return_scores``: host values only, before any GPU work."""
    st = settings or {}
    on = st.get("return_scores", False)
    if not isinstance(on, bool):
        raise ValueError(f"return_scores must be a bool, not {on!r}")
    if "score_window" not in st:
        return 0 if on else None
    window = st["score_window"]
    try:
        w = -1 if isinstance(window, bool) else operator.index(window)
    except TypeError:
        w = -1
    if not 0 <= w < n_bins:
        raise ValueError(f"score_window must be an integer in 0 .. {n_bins - 1}, not {window!r}")
    if not on:
        raise ValueError("score_window widens the scores: it needs return_scores=True")
    return w


PENALTY_SETTINGS = ("repetition_penalty", "presence_penalty", "frequency_penalty")
PENALTY_NEUTRAL = (1.0, 0.0, 0.0)


def check_penalties(repetition_penalty, presence_penalty, frequency_penalty, n: int) -> Optional[List[Tuple[float, float, float]]]:
    """The three penalty arguments of the generation calls, each one number or one per row (None: neutral) -> one
    (repetition, presence, frequency) triple per row, or None when every row is neutral (1, 0, 0).  ValueError for a
    repetition penalty that is not finite and > 0, a presence or frequency penalty that is not finite, or a list that is
    not ``n`` long: host values only, before any GPU work."""
    cols = []
    for name, x, neutral in zip(PENALTY_SETTINGS, (repetition_penalty, presence_penalty, frequency_penalty), PENALTY_NEUTRAL):
        try:
            vals = [x] * n if x is None or isinstance(x, numbers.Real) else list(x)
        except TypeError:
            raise ValueError(f"{name} must be a number or one number per row, not {x!r}") from None
        if len(vals) != n:
            raise ValueError(f"{name}: {len(vals)} values for {n} rows (one number, or one per row)")
        col = []
        for v in vals:
            try:
                f = neutral if v is None else float(v)
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be a number, not {v!r}") from None
            if isinstance(v, bool) or not math.isfinite(f) or (name == "repetition_penalty" and f <= 0):
                raise ValueError(f"{name} must be finite" + (" and > 0" if name == "repetition_penalty" else "") + f", not {v!r}")
            col.append(f)
        cols.append(col)
    rows = list(zip(*cols))
    return None if all(r == PENALTY_NEUTRAL for r in rows) else rows


def penalties_of(settings: Optional[dict]) -> dict:
    """The penalty entries of a ``settings`` dict as keyword arguments of the generation calls (absent: neutral)."""
    st = settings or {}
    return {name: st.get(name, neutral) for name, neutral in zip(PENALTY_SETTINGS, PENALTY_NEUTRAL)}


def refuse_penalties(settings: Optional[dict], where: str, n: int = 1) -> None:
    """An entry point that does not serve the penalties: ValueError naming ``where`` when ``settings`` carries a
    non-neutral one (and the validation errors of ``check_penalties`` for a value that is none)."""
    st = penalties_of(settings)
    for name in PENALTY_SETTINGS:  # a per-row list is judged by its values, whatever its length
        if isinstance(st[name], (list, tuple)):
            n = len(st[name])
    if check_penalties(*(st[name] for name in PENALTY_SETTINGS), n) is not None:
        raise ValueError(f"repetition_penalty / presence_penalty / frequency_penalty are not served by {where}")


FILTER_SETTINGS = ("top_k", "min_p")
FILTER_NEUTRAL = (0, 0.0)


def check_filters(top_k, min_p, n: int) -> Optional[List[Tuple[int, float]]]:
    """The ``top_k`` / ``min_p`` arguments of the generation calls, each one value or one per row (None: off) -> one
    (top_k, min_p) pair per row, or None when every row is neutral (0, 0.0).  ValueError for a ``top_k`` that is not an
    integer >= 0 (a bool is none), a ``min_p`` that is not finite or lies outside [0, 1], or a list that is not ``n`` long:
    host values only, before any GPU work."""
    cols = []
    for name, x in zip(FILTER_SETTINGS, (top_k, min_p)):
        try:
            vals = [x] * n if x is None or isinstance(x, (numbers.Real, str)) else list(x)
        except TypeError:
            raise ValueError(f"{name} must be one value or one per row, not {x!r}") from None
        if len(vals) != n:
            raise ValueError(f"{name}: {len(vals)} values for {n} rows (one value, or one per row)")
        col = []
        for v in vals:
            if v is None:
                col.append(FILTER_NEUTRAL[len(cols)])
            elif name == "top_k":
                try:
                    k = -1 if isinstance(v, bool) else operator.index(v)
                except TypeError:
                    k = -1
                if not 0 <= k < 2 ** 31:
                    raise ValueError(f"top_k must be an integer >= 0 (0: off), not {v!r}")
                col.append(k)
            else:
                try:
                    f = float("nan") if isinstance(v, (bool, str)) else float(v)
                except (TypeError, ValueError):
                    f = float("nan")
                if not (math.isfinite(f) and 0.0 <= f <= 1.0):
                    raise ValueError(f"min_p must be a number in [0, 1] (0: off), not {v!r}")
                col.append(f)
        cols.append(col)
    rows = list(zip(*cols))
    return None if all(r == FILTER_NEUTRAL for r in rows) else rows


def filters_of(settings: Optional[dict]) -> dict:
    """The ``top_k`` / ``min_p`` entries of a ``settings`` dict as keyword arguments of the generation calls (absent: off)."""
    st = settings or {}
    return {name: st.get(name, neutral) for name, neutral in zip(FILTER_SETTINGS, FILTER_NEUTRAL)}


def refuse_filters(settings: Optional[dict], where: str, n: int = 1) -> None:
    """An entry point that does not serve the sampling filters: ValueError naming ``where`` when ``settings`` carries a
    non-neutral one (and the validation errors of ``check_filters`` for a value that is none)."""
    st = filters_of(settings)
    for name in FILTER_SETTINGS:  # a per-row list is judged by its values, whatever its length
        if isinstance(st[name], (list, tuple)):
            n = len(st[name])
    if check_filters(st["top_k"], st["min_p"], n) is not None:
        raise ValueError(f"top_k / min_p are not served by {where}")


@dataclass(frozen=True, eq=False)
class Penalty:
    """The penalty state of a chunk (md_penalize_rows), all device memory at fixed addresses.  ``repetition``, ``presence``
    and ``frequency`` (fp32 [b]) are the rows' settings.  ``hist`` (int32 [n, hist_cap]) and ``hist_len`` (int32 [n]) hold
    the generated tokens of each history and are extended by every step: row r's history is row r's own, or, ``by_slot``,
    that of its KV slot ``rows.slots[r]`` (the continuous engine: a request changes row from chunk to chunk and keeps its
    slot; a row of slot -1 is idle)."""

    repetition: Any
    presence: Any
    frequency: Any
    hist: Any
    hist_len: Any
    hist_cap: int
    by_slot: bool = False

    def key(self) -> tuple:
        """What a captured chunk bakes in of the penalty state: addresses, the capacity and whose history a row's is."""
        return ("penalty",) + tuple(t.data_ptr() for t in (self.repetition, self.presence, self.frequency, self.hist,
                                                          self.hist_len)) + (int(self.hist_cap), bool(self.by_slot))


@dataclass(frozen=True, eq=False)
class Constraint:
    """The constraint state of a chunk (md_constrain_rows), all device memory at fixed addresses.  ``row_ptr`` (int32
    [state_cap + 1]), ``default_next`` (int32 [state_cap]), ``edge_tok`` and ``edge_next`` (int32 [edge_cap]) are the
    packed table of the call's automata (moondream_amd/constraint.py: ``pack``).  ``state`` (int32 [n]) holds each row's
    current state (FREE: an unconstrained row) and is advanced by every step: row r's entry is row r's own, or,
    ``by_slot``, that of its KV slot ``rows.slots[r]`` (the continuous engine; a row of slot -1 is idle)."""

    row_ptr: Any
    default_next: Any
    edge_tok: Any
    edge_next: Any
    state: Any
    state_cap: int
    by_slot: bool = False

    def key(self) -> tuple:
        """What a captured chunk bakes in of the constraint state: addresses, the capacity and whose state a row's is."""
        return ("constraint",) + tuple(t.data_ptr() for t in (self.row_ptr, self.default_next, self.edge_tok, self.edge_next,
                                                             self.state)) + (int(self.state_cap), bool(self.by_slot))


@dataclass(frozen=True, eq=False)
class Stop:
    """The stop-string / stop-id state of a chunk (md_stop_rows), all device memory at fixed addresses.  ``trans`` (uint16
    [state_cap, 256]), ``match_len`` (uint16 [state_cap]) and ``match_id`` (int32 [state_cap]) are the packed table of the
    call's stop sets (moondream_amd/stop.py: ``pack``).  ``id_ptr`` (int32 [n + 1]), ``ids`` and ``id_base`` (int32 [n])
    are the rows' stop ids.  ``tok_off`` (int32 [vocab + 1]) / ``tok_bytes`` (uint8 [n_bytes]) spell the vocabulary (None:
    stop sets of ids alone need no bytes).  ``words`` (int32 [6, n]) holds, per row, its DFA state (negative: no stop set),
    the tokens and bytes it has seen and the result triple (at, keep, which) -- ``at`` -1 until the first match, all
    three written once: row r's words are row r's own, or, ``by_slot``, those of its KV slot ``rows.slots[r]`` (the
    continuous engine; a row of slot -1 is idle)."""

    trans: Any
    match_len: Any
    match_id: Any
    id_ptr: Any
    ids: Any
    id_base: Any
    tok_off: Any
    tok_bytes: Any
    vocab: int
    n_bytes: int
    words: Any
    state_cap: int
    by_slot: bool = False

    @property
    def at(self):
        return self.words[3]

    def key(self) -> tuple:
        """What a captured chunk bakes in of the stop state: addresses, the capacity and whose words a row's are."""
        return ("stop",) + tuple(t.data_ptr() if t is not None else 0 for t in (
            self.trans, self.match_len, self.match_id, self.id_ptr, self.ids, self.id_base, self.tok_off, self.tok_bytes,
            self.words)) + (int(self.vocab), int(self.n_bytes), int(self.state_cap), bool(self.by_slot))


@dataclass(frozen=True, eq=False)
class Beam:
    """The beam-search state of a chunk (md_beam_select, md_kv_copy_tail), all device memory at fixed addresses.  The
    chunk's ``b`` rows are requests x ``num_beams`` beams.  ``state``: the library's struct over the caller's arrays
    (``_lib.MdBeamState``: cum, cur, own, len, done, prefix_len, the pool, inv_norm, the candidate scratch) -- ``cur`` is
    also the slot table of the steps' routing, so a beam changes the slot it decodes in without the launch changing.
    ``parents`` (int32 [>= n, b]): step i writes plane i, the beam each row continues.  ``src`` / ``dst`` / ``frm`` /
    ``to`` (int32 [b]): the hand-off md_beam_select emits and md_kv_copy_tail consumes in the same step.  ``eos_id`` < 0:
    nothing ever finishes.  ``keep``: the tensors behind ``state`` (their addresses are the key)."""

    num_beams: int
    eos_id: int
    early_stopping: bool
    state: Any
    parents: Any
    src: Any
    dst: Any
    frm: Any
    to: Any
    n_slots: int
    keep: Tuple[Any, ...] = ()

    def key(self) -> tuple:
        """What a captured chunk bakes in of the beam state: addresses, the width and the stopping rule."""
        return ("beam", int(self.num_beams), int(self.eos_id), bool(self.early_stopping), int(self.n_slots)) + tuple(
            t.data_ptr() for t in self.keep) + tuple(t.data_ptr() for t in (self.parents, self.src, self.dst, self.frm, self.to))


@dataclass(frozen=True, eq=False)
class Sampling:
    """How tokens are sampled (``None`` where one is expected: greedy): the reference's temperature / top-p rule with one
    uniform per (token, sequence).  Two floats are a whole call's settings: the uniforms come from ``generator`` (a device
    generator; None: the device's default one) and row i draws the uniform of row ``row_perm[i]`` (device int64 [B]: the
    shared-prefix rows see the draws of the copy path's row order).  Two device fp32 [B] tensors are every row's own
    settings (md_sample_rows): temperature > 0 samples, 0 takes the argmax, < 0 leaves the row alone.  ``top_k`` (device
    int32 [B]) and ``min_p`` (device fp32 [B]), with per-row settings only and both or neither: every sampled row is also cut
    to its first ``top_k`` tokens and to the tokens of probability >= min_p * the best one's (md_sample_rows_filtered; 0:
    off).  None, the default: the picks, launches and graph keys of a record without the fields."""

    temperature: Any
    top_p: Any
    generator: Any = None
    row_perm: Any = None
    top_k: Any = None
    min_p: Any = None

    @property
    def per_row(self) -> bool:
        return hasattr(self.temperature, "data_ptr")

    @property
    def filtered(self) -> bool:
        return self.top_k is not None

    def cut(self, r0: int, r1: int) -> "Sampling":
        """Rows [r0, r1) of a per-row record: its tensors cut like the rows.  The call's generator and draw order stay
        behind: whoever cuts the rows cuts their draws."""
        cut = lambda t: t[r0:r1] if t is not None else None
        return Sampling(self.temperature[r0:r1], self.top_p[r0:r1], top_k=cut(self.top_k), min_p=cut(self.min_p))


def pick_tokens(model, pick: Optional[Sampling], logits, suppress_id: int = -1, uniforms=None, out=None, row_perm=None):
    """The one choice among the model's three pick launches, for logits [B, V] -> int32 [B] (``out``, or a new tensor).
    ``pick`` None: the argmax (``_pick`` at temperature 0).  A record of two floats, the call's settings: ``_pick`` -- it
    draws from ``uniforms``, or, without them, from the record's generator in the order ``row_perm``.  (The first token's
    pick used to hand ``_pick`` no ``uniforms``; no caller gives it any with such a record, so its draws are the same.)
    A per-row record: ``_pick_rows`` over ``uniforms`` fp32 [B], or, with ``top_k`` / ``min_p``, ``_pick_rows_filtered``."""
    if pick is None:
        pick = Sampling(0.0, 0.0)
    if pick.filtered:
        return model._pick_rows_filtered(logits, pick.temperature, pick.top_p, pick.top_k, pick.min_p, suppress_id, uniforms, out=out)
    if pick.per_row:
        return model._pick_rows(logits, pick.temperature, pick.top_p, suppress_id, uniforms, out=out)
    return model._pick(logits, pick.temperature, pick.top_p, suppress_id, pick.generator, row_perm=row_perm, uniforms=uniforms, out=out)


@dataclass(frozen=True, eq=False)
class ReasonChunk:
    """The reasoning state of a chunk (``query(reasoning=True)`` in lockstep: md_decode_step_reason), all device memory at
    fixed addresses.  Per row (int32 [b] unless said): ``phase``, ``n_reason``, ``n_answer``, ``suppress`` [b, 2],
    ``coord_bin`` and ``hidden_prev`` (bf16 [b, D]: the hidden state that predicted the token a step consumes) are read and
    rewritten by every step.  Per step, int32 planes [>= n, b]: step i writes ``kind[i]`` / ``ground[i]`` -- what the token
    it consumed was (MD_REASON_KIND_*) and its coordinate bin, or -1 -- and, when ``forced`` is given, consumes
    ``forced[i][r]`` instead of the picked token wherever that is >= 0 (teacher forcing).  ``max_reason`` / ``max_answer``
    bound the two phases; ``region`` is the coordinate head's struct (``_lib.MdRegionCoord``)."""

    phase: Any
    n_reason: Any
    n_answer: Any
    suppress: Any
    coord_bin: Any
    hidden_prev: Any
    kind: Any
    ground: Any
    max_reason: int
    max_answer: int
    region: Any
    forced: Any = None

    def key(self) -> tuple:
        """What a captured chunk bakes in of the reasoning state: addresses and the two budgets."""
        return ("reason",) + tuple(t.data_ptr() for t in (self.phase, self.n_reason, self.n_answer, self.suppress, self.coord_bin,
                                                          self.hidden_prev, self.kind, self.ground)) + (
            self.forced.data_ptr() if self.forced is not None else 0, int(self.max_reason), int(self.max_answer),
            int(self.region.dec_fc1.w or 0))


@dataclass(frozen=True, eq=False)
class DecodeChunk:
    """What ``n`` consecutive decode steps over ``b`` rows read and write, all at fixed addresses: step i consumes
    ``tokens[i]`` and writes ``tokens[i + 1]`` (int32 [>= n + 1, b]); ``pos`` (int32 [b]) is advanced by the steps;
    ``rows_of(i)`` is the routing of step i (``_Rows``; ``rows_of(0)`` stands for the chunk in the graph key: the others
    differ in data at fixed addresses only).  ``pick`` None keeps each step's argmax; otherwise step i draws every row from
    ``uniforms[i]`` (fp32 [>= n, b]) with the call's settings (``_pick``) or each row's own (``_pick_rows``; a record with
    ``top_k`` / ``min_p``: ``_pick_rows_filtered``, and the two addresses join the graph key).
    ``logprobs`` = (fp32, int32) planes [>= n, b]: row i takes the log-probability and rank of the tokens of step i.
    ``topk`` = (int32 ids, fp32 log-probabilities) planes [>= n, b, k]: row i takes the k alternatives of every row's
    decision in step i (md_topk_logprobs after the step's md_token_logprobs, gated by the step's tokens); with ``logprobs`` only.
    ``b1``: the single-sequence persistent kernel takes the steps (b = 1, greedy).  ``step(tok_in) -> logits``: the step
    made from its pieces instead of the fused one (a LoRA adapter; eager only, its pick writes ``tokens[i + 1]``).
    ``reason`` (``ReasonChunk``): the steps are md_decode_step_reason's -- each row's phase decides what it feeds and which
    ids its logits lose (``suppress_id`` is not used), and every step's pick is the per-row one; not with ``logprobs``.
    ``penalty`` (``Penalty``): after each step and before its pick, every row's consumed token joins its history and the
    row's logits take its penalties (md_penalize_rows).  The fused step's own argmax was taken from the raw logits, so
    such a chunk always picks again -- with ``pick`` None by the argmax launch -- and the log-probabilities and
    alternatives are those of the PENALISED logits, the distribution the token was picked from before temperature and
    top-p (every greedy token still has rank 0).  Not with ``b1`` or ``reason``.
    ``constraint`` (``Constraint``): after each step (and its penalties) and before its pick, every row's automaton is
    advanced by the token the step consumed and the tokens its new state forbids lose their logits (md_constrain_rows).
    Such a chunk always picks again too, and its log-probabilities and alternatives are those of the MASKED logits: a
    greedy token has rank 0 and an alternative outside the allowed set carries -inf.  Not with ``b1`` or ``reason``.
    ``beam`` (``Beam``): beam search -- after each step md_beam_select chooses every request's next beams from the
    logits the step left, writes their tokens to ``tokens[i + 1]`` (over the step's argmax) and their parents to plane i,
    and md_kv_copy_tail moves each surviving beam's KV tail to the slot its child decodes in.  The routing's slot table
    is the record's ``cur``.  Greedy, fused steps only: not with any other optional field.
    ``stop`` (``Stop``): after each step's pick and before its log-probability launches, every row's picked token
    ``tokens[i + 1]`` goes through its stop matcher (md_stop_rows): each generated token exactly once, in order (the first
    token, which the prompt pass picks, is fed by the caller before the first chunk).  The launch reads token ids only and
    changes no logit and no pick.  Not with ``b1``, ``reason`` or ``beam``."""

    b: int
    tokens: Any
    pos: Any
    rows_of: Callable[[int], Any]
    suppress_id: int
    ws_bytes: int = 0
    pick: Optional[Sampling] = None
    uniforms: Any = None
    logprobs: Optional[Tuple[Any, Any]] = None
    b1: bool = False
    step: Optional[Callable[[Any], Any]] = None
    reason: Optional[ReasonChunk] = None
    topk: Optional[Tuple[Any, Any]] = None
    penalty: Optional[Penalty] = None
    constraint: Optional[Constraint] = None
    beam: Optional[Beam] = None
    stop: Optional[Stop] = None


def run_chunk(model, chunk: DecodeChunk, n: int, tag: str = "decode", capture_stream: Optional[int] = None,
              may_capture: Optional[Callable[[], bool]] = None) -> bool:
    """Run steps 0 .. n-1 of ``chunk`` on ``model``.  ``capture_stream`` None: eagerly.  Otherwise the handle of the current
    stream: the chunk is replayed from the graph captured for it on that stream, or, first, run eagerly and captured
    (``model._replay_or_capture``: its ``GraphStore``'s, ``may_capture`` too).  The key starts (``tag``, stream) and names everything
    the launches bake in.  Returns True when it captured.  Besides that, the model gives the buffers (_decode_logits, _workspace,
    _kv_struct) and the launches (_decode_step, _decode_step_b1, _decode_step_reason, _penalize, _constrain, _pick, _pick_rows, _pick_rows_filtered, _token_logprobs, _topk_logprobs, _beam_select, _kv_copy_tail, _stop_rows)."""
    c = chunk
    pieces = c.step is not None
    assert c.reason is None or (not pieces and not c.b1 and c.logprobs is None and c.pick is not None and c.pick.per_row)
    assert not (pieces and (capture_stream is not None or c.b1))
    assert not c.b1 or (c.b == 1 and c.pick is None)
    assert c.topk is None or c.logprobs is not None
    assert c.penalty is None or (not c.b1 and c.reason is None)
    assert c.constraint is None or (not c.b1 and c.reason is None)
    assert c.beam is None or (not pieces and not c.b1 and c.reason is None and c.pick is None and c.logprobs is None
                              and c.penalty is None and c.constraint is None)
    assert c.stop is None or (not c.b1 and c.reason is None and c.beam is None)
    if not pieces:
        logits = model._decode_logits(c.b)
        ws = model._workspace(c.ws_bytes, 2)
        kv = model._kv_struct(c.rows_of(0).slot0)
        left = logits[: c.b]  # where every fused step (the single-sequence kernel too) leaves its logits
    lp, rk = c.logprobs if c.logprobs is not None else (None, None)
    tk_ids, tk_lp = c.topk if c.topk is not None else (None, None)
    by_row = c.pick is not None and c.pick.per_row
    assert c.pick is None or not c.pick.filtered or (by_row and c.pick.min_p is not None)
    # penalised or masked logits are picked from again (greedy: by the argmax launch): the fused step's argmax saw the raw ones
    again = c.pick is not None or c.penalty is not None or c.constraint is not None
    draws = lambda i: c.uniforms[i] if c.uniforms is not None else None

    def body():
        for i in range(n):
            tok_in, tok_out = c.tokens[i], c.tokens[i + 1]
            if c.reason is not None:
                # the step masks its logits per row and leaves the pick to the per-row kernel, nothing suppressed there
                model._decode_step_reason(c.rows_of(i), c.reason, i, tok_in, c.pos, c.b, logits, ws, kv)
                pick_tokens(model, c.pick, left, -1, draws(i), out=tok_out)
                continue
            if c.b1:
                model._decode_step_b1(tok_in, tok_out, c.pos, c.suppress_id, logits, ws, kv)
            elif not pieces:
                model._decode_step(c.rows_of(i), tok_in, tok_out, c.pos, c.b, c.suppress_id, logits, ws, kv)
            lg = c.step(tok_in) if pieces else left
            if c.beam is not None:  # the request's next beams over the step's argmax, then their KV tails to their slots
                model._beam_select(lg, c.suppress_id, c.beam, c.beam.num_beams, tok_out, c.beam.parents[i])
                model._kv_copy_tail(kv, c.beam)
                continue
            if c.penalty is not None:  # tok_in joins each row's history, whose tokens' logits are penalised in place
                model._penalize(lg, tok_in, c.rows_of(i), c.penalty)
            if c.constraint is not None:  # tok_in advances each row's automaton, whose new state masks the logits in place
                model._constrain(lg, tok_in, c.rows_of(i), c.constraint)
            # a fused step wrote its argmax to tok_out: a pick draws from the logits it left instead (of per-row settings,
            # a greedy row takes the same argmax again and an idle row keeps what is there)
            if again:
                pick_tokens(model, c.pick, lg, c.suppress_id, draws(i), out=tok_out)
            if c.stop is not None:  # the picked token through each row's stop matcher: ids only, no logit is touched
                model._stop_rows(tok_out, c.rows_of(i), c.stop)
            if lp is not None:  # targets = the step's tokens
                model._token_logprobs(lg, tok_out, c.suppress_id, lp[i], rk[i])
            if tk_ids is not None:  # the decision's alternatives; a row whose token is no id (idle) is not read
                model._topk_logprobs(lg, tok_out, c.suppress_id, tk_ids[i], tk_lp[i])

    if capture_stream is None:
        body()
        return False
    # a graph is replayed only on the stream it was captured for.  Of per-row settings and uniforms only their addresses
    # are baked in (the values are device data); scalar settings are launch arguments.  The e4m3 KV copy decides the
    # attention kernel a step bakes in; the routing's part carries the bank's generation (its ranks are launch shapes).
    if by_row:
        pick = ("rows", c.pick.temperature.data_ptr(), c.pick.top_p.data_ptr())
        if c.pick.filtered:  # another launch: another graph; without the fields the key is what it was
            pick += ("filtered", c.pick.top_k.data_ptr(), c.pick.min_p.data_ptr())
    else:
        pick = None if c.pick is None else (float(c.pick.temperature), float(c.pick.top_p))
    key = (tag, capture_stream, c.b, n, c.suppress_id, c.tokens.data_ptr(), c.pos.data_ptr(), ws.data_ptr(), kv.k, kv.k8 or 0,
           logits.data_ptr(), c.b1, pick, c.uniforms.data_ptr() if c.uniforms is not None else 0) + c.rows_of(0).key()
    if lp is not None:  # a chunk with the logprob launches is another graph; without them key and graph are unchanged
        key += ("logprobs", lp.data_ptr(), rk.data_ptr())
    if tk_ids is not None:  # and one more with the top-k launches
        key += ("topk", int(tk_ids.shape[-1]), tk_ids.data_ptr(), tk_lp.data_ptr())
    if c.reason is not None:  # likewise: another graph, keyed by the state's addresses
        key += c.reason.key()
    if c.penalty is not None:  # and another with the penalty launches
        key += c.penalty.key()
    if c.constraint is not None:  # and another with the constraint launches
        key += c.constraint.key()
    if c.beam is not None:  # and another with the select and copy launches
        key += c.beam.key()
    if c.stop is not None:  # and another with the stop launches; a chunk without them keeps its key
        key += c.stop.key()
    return model._replay_or_capture(key, body, may_capture=may_capture)
