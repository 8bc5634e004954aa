"""Continuous batching for token generation: per-sequence exit and KV-slot refill in the decode loop.

``MoondreamModel.batch_generate_ids`` decodes a batch in lockstep: a sequence that has emitted EOS (or reached its length)
keeps its row in every later step and its KV slot until the whole batch ends.  Here every request owns one KV slot of a slab
sized once; each decode step runs only the live requests (``md_decode_step_slots``: row r attends over and writes slot
``slots[r]``, rows of slot -1 are idle and touch no slab memory), finished requests leave at the next chunk boundary and
queued ones are prefilled straight into the freed slots.

Exactness: every batched kernel's accumulation order is a function of the layer shape, never of the number of rows in the
launch (``batch_generate_ids``; MD_TILE_PINNED, MD_TILE_DECODE_TALL), and the slot table changes addresses only.  So a
request's ids do not depend on what else is live: they equal, bit for bit, what the lockstep path gives the same
(image, prompt) in a batch of more than one sequence.  The engine never uses the single-sequence persistent kernel and
always pins the tile config; the prompt pass of the two-pass prefill (EncodedImage inputs, ``fused_prefill`` off) runs
in launches of <= 64 rows, as ``set_strict_batch_invariance`` does, for the same reason.

``SlotScheduler`` is the pure-Python part (no GPU): slot pool, FIFO admission queue, per-request state, chunk plans and
retirement.  ``ContinuousEngine`` drives it with the library.
"""
from __future__ import annotations

import math
from collections import deque
from dataclasses import dataclass, field, replace
from typing import Callable, Deque, Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from .constraint import FREE, TokenAutomaton, check_constraints, grammar_of, pack
from . import stop as stops
from .stop import Finish
from .decode_loop import PENALTY_NEUTRAL, Constraint, DecodeChunk, Penalty, Sampling, Stop, check_top_logprobs, run_chunk
from .scores import HostScores, Scores
from .settings import CallSettings, RowSettings
from .spatial import SpatialRecord, check_spatial_refs, spatial_prompt_ids

DEFAULT_MAX_TOKENS = 768  # moondream.py (the reference's default, moondream.py:50-53)
DEFAULT_TOP_P = 0.3
MAX_GRAPHS = 16  # captured decode chunks per (model, stream)
IDLE_SLOT = -1
MD_PENALTY_HIST_MAX = 4096  # include/moondream_hip.h
DEFAULT_CONSTRAINT_STATES = 4096   # the engine's constraint table: states ...
DEFAULT_STOP_STATES = 1024         # the engine's stop table: DFA states over all the distinct stop sets its requests ever use
DEFAULT_CONSTRAINT_EDGES = 65536   # ... and edges, over all the distinct automata its requests ever use


def row_buckets(max_live: int) -> List[int]:
    """Row counts a decode chunk is padded to: powers of two below 32, then multiples of a step (32, doubled while there would
    be more than MAX_GRAPHS buckets), the last one max_live.  A chunk's launch shapes -- and its captured graph -- depend on
    the bucket only, never on which requests are live."""
    if max_live < 1:
        raise ValueError("max_live must be >= 1")
    small = [b for b in (1, 2, 4, 8, 16) if b < max_live]
    step = 32
    while len(small) + (max_live + step - 1) // step > MAX_GRAPHS:
        step *= 2
    big = list(range(step, max_live, step)) + [max_live]
    return sorted(set(small + [b for b in big if b >= 32] + [max_live]))


@dataclass(eq=False)  # identity: a request is itself, whatever its fields
class Request:
    """One generation request.  ``pos`` is the position of the next token to decode (the prompt's end after the prefill);
    ``step_limit`` the decode steps it may take: min(max_tokens - 1, max_context - 1 - pos) -- with the first token from the
    prefill that is MoondreamModel._truncate's length rule, and the context rule of the lockstep loop per request."""

    rid: int
    image: object
    prompt: List[int]
    max_tokens: int
    eos_id: Optional[int]
    seed: Optional[int] = None
    slot: int = IDLE_SLOT
    pos: int = 0
    ids: List[int] = field(default_factory=list)
    last: int = 0
    steps: int = 0
    step_limit: int = 0
    done: bool = False
    generator: object = None
    variant: int = -1  # index in the model's LoRA bank (md_lora_bank); -1: the base model
    settings: RowSettings = RowSettings()  # what it decodes with (moondream_amd/settings.py); a greedy request draws nothing
    logprobs: List[float] = field(default_factory=list)  # of ``ids``, entry for entry (an engine with logprobs=True)
    ranks: List[int] = field(default_factory=list)
    alternatives: List[list] = field(default_factory=list)  # of ``ids`` too: k (token_id, logprob) pairs each (top_logprobs=k)
    constraint_start: int = FREE  # the start state of its automaton in the engine's table
    spatial: Optional[Tuple[int, list]] = None  # (position of the first placeholder in ``prompt``, the checked refs); None: no refs
    stop_start: int = stops.NO_STOP  # the root of its stop set's automaton in the engine's table (``settings.stop``)
    include_stop_str: bool = False   # ``Finish.text_bytes`` counts the matched string too
    stop_hit: Optional[Tuple[int, int, int]] = None  # the matcher's (at, keep, which) after the prefill's token
    finish: Optional[Finish] = None  # how it ended, set when it retires

    @property
    def remaining(self) -> int:
        return 0 if self.done else max(0, self.step_limit - self.steps)


@dataclass
class ChunkPlan:
    """``n`` decode steps over ``bucket`` rows: ``rows[r]`` is the request of row r (rows past len(rows) are padding);
    ``slots[i][r]`` the slot row r addresses in step i (IDLE_SLOT: padding, or a request past its step limit).
    ``fresh[r]``: the slot of a row whose request takes its first decode step in this chunk (IDLE_SLOT otherwise) -- the
    slot has just been refilled, and whatever is kept per slot beyond the KV rows (the penalty history's length) starts
    from nothing here."""

    rows: List[Request]
    bucket: int
    n: int
    slots: np.ndarray   # int32 [n, bucket]
    tokens: np.ndarray  # int32 [bucket]: the token each row consumes in step 0
    pos: np.ndarray     # int32 [bucket]: its position
    fresh: Optional[np.ndarray] = None  # int32 [bucket]

    @property
    def live_row_steps(self) -> int:
        return int((self.slots >= 0).sum())


@dataclass
class EngineStats:
    decode_steps: int = 0
    padded_row_steps: int = 0
    live_row_steps: int = 0
    admissions: int = 0
    prefill_passes: int = 0
    graph_captures: int = 0


class SlotScheduler:
    """Slot pool of ``max_live`` KV slots, FIFO admission queue, chunk plans and retirement (no GPU, no torch).

    Admission: when at least ``admit_threshold`` slots are free, or nothing is live, the head of the queue takes free slots
    (a freed slot goes to the back of the free list: slots are reused first-in first-out).  A request retires when it
    emits its ``eos_id`` (not part of its ids), when its ids reach ``max_tokens``, when its next position reaches
    ``max_context - 1``, or at the first match of its stop set (``commit``'s ``stop`` arrays, ``Request.stop_hit`` for the
    prefill's token): in front of a stop id, behind the token a stop string completed in.  ``Request.finish`` says which."""

    def __init__(self, max_live: int, max_context: int, chunk: int = 16, admit_threshold: Optional[int] = None):
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        self.max_live = int(max_live)
        self.max_context = int(max_context)
        self.chunk = int(chunk)
        self.buckets = row_buckets(self.max_live)
        self.admit_threshold = max(1, int(admit_threshold if admit_threshold is not None else self.max_live // 8))
        self.free: Deque[int] = deque(range(self.max_live))
        self.queue: Deque[Request] = deque()
        self.live: List[Request] = []  # admission order = row order of every plan (stable)
        self.stats = EngineStats()

    # ---- admission / retirement
    def submit(self, req: Request) -> None:
        self.queue.append(req)

    def pending(self) -> bool:
        return bool(self.queue or self.live)

    def take_admissions(self) -> List[Request]:
        """Requests to prefill now, each with its slot assigned (in queue order)."""
        if not self.queue or not self.free or (self.live and len(self.free) < self.admit_threshold):
            return []
        out = []
        while self.queue and self.free:
            r = self.queue.popleft()
            r.slot = self.free.popleft()
            out.append(r)
        self.stats.admissions += 1
        return out

    def start(self, req: Request, first: int, pos: int, logprob: Optional[float] = None, rank: Optional[int] = None,
              alternatives: Optional[list] = None) -> bool:
        """The prefill of ``req`` picked ``first`` with the next token at position ``pos`` (``logprob`` / ``rank``: its values,
        kept beside it; ``alternatives``: the decision's (token_id, logprob) pairs, likewise).  Returns True if the request
        is already finished (it then no longer holds its slot)."""
        req.logprobs, req.ranks, req.alternatives = [], [], []
        req.pos = int(pos)
        req.steps = 0
        req.step_limit = max(0, min(req.max_tokens - 1, self.max_context - 1 - req.pos))
        req.last = int(first)
        if req.max_tokens <= 0 or (req.eos_id is not None and first == req.eos_id):
            req.ids = []
            return self._retire(req, Finish("length" if req.max_tokens <= 0 else "eos"))
        if req.stop_hit is not None and req.stop_hit[0] == 0:  # the first token is a stop id, or completes a stop string
            req.ids = []
            fin = self._stopped(req, int(first), *req.stop_hit[1:])
            if req.ids and logprob is not None:  # a stop string's token stays, with its scores
                req.logprobs, req.ranks = [float(logprob)], [int(rank)]
            if req.ids and alternatives is not None:
                req.alternatives = [HostScores(logprob, rank, *alternatives).alternatives()]
            return self._retire(req, fin)
        req.ids = [int(first)]
        if logprob is not None:
            req.logprobs, req.ranks = [float(logprob)], [int(rank)]
        if alternatives is not None:
            req.alternatives = [HostScores(logprob, rank, *alternatives).alternatives()]
        if req.step_limit == 0:
            return self._retire(req)
        self.live.append(req)
        return False

    @staticmethod
    def _stopped(req: Request, tok: int, keep: int, which: int) -> Finish:
        """The request matched its stop set in token ``tok``: a stop string's token joins the ids (a token cannot be split),
        a stop id does not (like eos).  Returns its ``Finish``."""
        s = req.settings.stop
        if which < len(s.strings):
            req.ids.append(int(tok))
            text = s.strings[which]
            return Finish("stop", text, int(keep) + (len(text.encode("utf-8")) if req.include_stop_str else 0))
        return Finish("stop", s.named(which))

    def _retire(self, req: Request, finish: Optional[Finish] = None) -> bool:
        req.finish = finish or Finish("length")
        req.done = True
        if req in self.live:
            self.live.remove(req)
        if req.slot >= 0:
            self.free.append(req.slot)
        req.slot = IDLE_SLOT
        return True

    # ---- chunks
    def bucket_for(self, rows: int) -> int:
        for b in self.buckets:
            if b >= rows:
                return b
        raise AssertionError((rows, self.buckets))

    def plan(self) -> Optional[ChunkPlan]:
        if not self.live:
            return None
        rows = list(self.live)
        bucket = self.bucket_for(len(rows))
        n = min(self.chunk, max(r.remaining for r in rows))
        slots = np.full((n, bucket), IDLE_SLOT, dtype=np.int32)
        tokens = np.zeros(bucket, dtype=np.int32)
        pos = np.zeros(bucket, dtype=np.int32)
        fresh = np.full(bucket, IDLE_SLOT, dtype=np.int32)
        for i, r in enumerate(rows):
            slots[: min(n, r.remaining), i] = r.slot  # past its step limit a row is idle: no cache row beyond its context
            tokens[i] = r.last
            pos[i] = r.pos
            if r.steps == 0:
                fresh[i] = r.slot
        return ChunkPlan(rows, bucket, n, slots, tokens, pos, fresh)

    @staticmethod
    def state_resets(plan: ChunkPlan, spare: int) -> Tuple[np.ndarray, np.ndarray]:
        """The constraint states a chunk starts from: (slot int64 [bucket], state int32 [bucket]) -- a row whose request
        takes its first decode step here (``plan.fresh``: its slot has just been refilled, and still holds the state its
        last occupant left) gets its request's start state, FREE for a request without an automaton; every other row
        writes FREE to the ``spare`` entry nobody reads."""
        idx = np.where(plan.fresh >= 0, plan.fresh, spare).astype(np.int64)
        val = np.full(plan.bucket, FREE, dtype=np.int32)
        for i, r in enumerate(plan.rows):
            if plan.fresh[i] >= 0:
                val[i] = r.constraint_start
        return idx, val

    def commit(self, plan: ChunkPlan, out: np.ndarray, logprobs: Optional[np.ndarray] = None,
               ranks: Optional[np.ndarray] = None, top_ids: Optional[np.ndarray] = None,
               top_logprobs: Optional[np.ndarray] = None,
               stop: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]] = None) -> List[Request]:
        """``stop`` = the chunk's (at, keep, which) arrays [bucket], row r's matcher result after the chunk (``at`` -1: no
        match yet; the index counts the request's generated tokens, the prefill's being 0): a request whose ``at`` falls
        inside the chunk retires there -- an eos in the same token wins, as in the lockstep call -- and its slot returns
        to the pool.  ``out[i][r]``: the token row r produced in step i (``logprobs[i][r]`` / ``ranks[i][r]``: its values, and
        ``top_ids[i][r]`` / ``top_logprobs[i][r]`` [k]: the decision's alternatives, appended in step with the ids; idle and
        padding rows are never read).  Advances every row, retires the finished ones (their slots return to the pool) and
        returns them in row order."""
        self.stats.decode_steps += plan.n
        self.stats.padded_row_steps += plan.n * plan.bucket
        self.stats.live_row_steps += plan.live_row_steps
        finished = []
        host = HostScores(logprobs, ranks, top_ids, top_logprobs)
        for r_idx, r in enumerate(plan.rows):
            fin = None
            at = int(stop[0][r_idx]) if stop is not None and r.settings.stop is not None else -1
            g0 = len(r.ids)  # the generated index of the chunk's first token (nothing was cut so far: no eos, no match)
            for i in range(min(plan.n, r.remaining)):
                tok = int(out[i][r_idx])
                r.steps += 1
                r.pos += 1
                r.last = tok
                if r.eos_id is not None and tok == r.eos_id:
                    fin = Finish("eos")
                    break
                if at == g0 + i:
                    fin = self._stopped(r, tok, int(stop[1][r_idx]), int(stop[2][r_idx]))
                    if logprobs is not None and len(r.ids) > len(r.logprobs):  # a string's token keeps its scores
                        r.logprobs.append(float(logprobs[i][r_idx]))
                        r.ranks.append(int(ranks[i][r_idx]))
                    if top_ids is not None and len(r.ids) > len(r.alternatives):
                        r.alternatives.append(host.alternatives((i, r_idx)))
                    break
                r.ids.append(tok)
                if logprobs is not None:
                    r.logprobs.append(float(logprobs[i][r_idx]))
                    r.ranks.append(int(ranks[i][r_idx]))
                if top_ids is not None:
                    r.alternatives.append(host.alternatives((i, r_idx)))
                if r.steps >= r.step_limit:
                    fin = Finish("length")
                    break
            if fin is not None:
                self._retire(r, fin)
                finished.append(r)
        return finished

    def run(self, admit: Callable[[List[Request]], Sequence[Tuple[int, int]]],
            step: Callable[[ChunkPlan], np.ndarray]) -> Iterator[Request]:
        """Drive the schedule: ``admit(requests)`` prefills them and returns (first token, next position) per request,
        ``step(plan)`` runs a chunk and returns its tokens [n, bucket].  With log-probabilities: (first token, next position,
        logprob, rank) and (tokens, logprobs, ranks); with alternatives one more element, (top ids [k], top logprobs [k]),
        and two more planes [n, bucket, k].  A last element that is a dict holds ``commit``'s keyword arguments (``stop``).
        Yields requests in completion order."""
        while self.pending():
            adm = self.take_admissions()
            if adm:
                for r, started in zip(adm, admit(adm)):
                    if self.start(r, *started):
                        yield r
            plan = self.plan()
            if plan is None:
                continue
            res = step(plan)
            res, kw = (res[:-1], res[-1]) if isinstance(res, tuple) and isinstance(res[-1], dict) else (res, {})
            yield from (self.commit(plan, *res, **kw) if isinstance(res, tuple) else self.commit(plan, res, **kw))


class ContinuousEngine:
    """Continuous-batching generation on a ``MoondreamModel``.

        eng = ContinuousEngine(model, max_live=64)
        for img, n in work:
            eng.submit(img, prompt_ids, max_tokens=n)
        for rid, ids in eng.run():   # completion order
            ...

    ``max_live`` KV slots are allocated once, before the first admission, and never grown during a run.  With
    ``model.compile()`` decode chunks are replayed from hipGraphs keyed by the padded row count (at most MAX_GRAPHS per
    model and stream); the token, position, slot-table, uniform and row-settings buffers of a bucket keep their addresses
    and are refreshed before each replay.  ``temperature`` / ``top_p`` are the defaults of a request that names none
    (``submit(..., temperature=, top_p=)``): every row of a decode step carries its own pair (md_sample_rows: temperature > 0
    samples, 0 takes the argmax, padding rows are idle), so greedy and sampled requests of any settings share steps and
    captured chunks.  Each sampled request draws its uniforms from its own generator (``seed``): its tokens depend neither
    on which other requests share its steps nor on their settings.

    ``logprobs``, and with it ``top_logprobs`` = k in 1 .. 32 (engine-wide, part of the chunk graph key): every step of a
    chunk also fills one row of the bucket's ``Scores`` record inside the captured chunk -- each row's log-probability and
    rank of the token it picked (md_token_logprobs, targets = the step's tokens) and its k most probable live tokens
    (md_topk_logprobs, the launch after, gated by the step's tokens) -- and every ``Request`` carries ``logprobs`` / ``ranks``
    and ``alternatives`` (k (token_id, logprob) pairs per id) beside its ids: ``run(with_logprobs=True)``.  They are, bit for
    bit, the values of ``MoondreamModel.batch_generate_ids(..., return_logprobs=True, top_logprobs=k)``: the model's own
    distribution at temperature 1, untruncated, whatever the request's sampling settings.  Off: the launches and graphs
    of an engine without the flags.

    ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty`` per request (``submit``; None: neutral):
    ``batch_generate_ids``' rule over the request's generated tokens.  The histories are per KV SLOT -- a request changes
    row from chunk to chunk and keeps its slot -- in one [max_live, max_context] table the engine owns for its lifetime; a
    refilled slot's length is zeroed in the request's first chunk (``ChunkPlan.fresh``, uploaded with the rows' settings:
    one more pinned H2D copy that only chunks with a penalised row make, no synchronisation).  Such chunks run
    md_penalize_rows before each pick and are graphs of their own; chunks whose rows are all neutral take the graph of
    an engine without penalties.  A request's ids depend on its own settings and seed only; with ``logprobs`` its scores
    are those of the penalised logits.

    ``constraint`` per request (``submit``; a ``TokenAutomaton``, None: free): ``batch_generate_ids``' rule, and its greedy
    ids bit for bit.  The engine owns ONE table of ``constraint_states`` states and ``constraint_edges`` edges for its
    lifetime and a state per KV slot, all made on first use.  The first request that uses an automaton (by identity) has
    it appended to the table: room is taken at ``submit`` (ValueError when the table is full), the rows are copied behind
    the stream before the request's prefill.  A refilled slot's state is set to its request's start state (FREE for a
    free request) in the request's first chunk (``SlotScheduler.state_resets``: two small pinned copies and one
    index_copy_ on the stream, made by every chunk once the engine has seen a constraint).  Chunks with a constrained
    row run md_constrain_rows before each pick and are graphs of their own; all others take the graph of an engine
    without constraints.

    ``top_k`` / ``min_p`` per request (``submit``; None: off): ``batch_generate_ids``' rule for a sampled request, the
    first token included.  They are stored per row next to temperature and top-p, in a per-bucket pair of fixed-address
    tables (int32 / fp32, pinned staging: one more small copy each) that only chunks with a filtered row fill; such
    chunks pick with md_sample_rows_filtered and are graphs of their own, all others are the chunks of an engine without
    the settings.  A request's ids depend on its own settings and seed only.

    ``stop`` / ``stop_token_ids`` / ``include_stop_str_in_output`` per request (``submit``): ``batch_generate_ids``' rule,
    ids and ``Finish`` per request (``Request.finish``, ``finishes``).  The engine owns ONE table of ``stop_states`` DFA
    states for its lifetime, to which each distinct stop set (by its strings) is appended on first use -- room is taken at
    ``submit`` (ValueError when the table is full) -- and six words, sixteen ids and an id base per KV SLOT, all made on
    first use.  At admission, once the engine has seen a stop set, every admitted slot's words are reset (a request
    without one gets a negative state: skipped) and ONE md_stop_rows launch feeds the prefill's tokens; chunks with a
    row that has a stop set run md_stop_rows after each pick and are graphs of their own, all others take the graph of
    an engine without stops.  The rows' (at, keep, which) come back in the chunk's copy of the ids, and
    ``SlotScheduler.commit`` retires a request at its ``at``: the KV slot goes to the next queued request instead of
    decoding to ``max_tokens``.  Stop strings need the bytes of every id: ONE vocabulary object per engine."""

    def __init__(self, model, max_live: int = 64, chunk: int = 16, temperature: float = 0.0, top_p: float = DEFAULT_TOP_P,
                 admit_threshold: Optional[int] = None, logprobs: bool = False, top_logprobs: Optional[int] = None,
                 constraint_states: int = DEFAULT_CONSTRAINT_STATES, constraint_edges: int = DEFAULT_CONSTRAINT_EDGES,
                 stop_states: int = DEFAULT_STOP_STATES):
        self.model = model
        self.logprobs = bool(logprobs)
        self.top_logprobs = check_top_logprobs(top_logprobs, self.logprobs)
        self.max_live = int(max_live)
        self.chunk = int(chunk)
        self.temperature = float(temperature)
        self.top_p = float(top_p)
        self.admit_threshold = admit_threshold
        t = model.config.text
        self.sched = SlotScheduler(self.max_live, t.max_context, self.chunk, admit_threshold)
        self._next_rid = 0
        if int(constraint_states) < 1 or int(constraint_edges) < 1:
            raise ValueError("constraint_states and constraint_edges must be >= 1")
        self.constraint_states, self.constraint_edges = int(constraint_states), int(constraint_edges)
        self._con_start: Dict[int, Tuple[TokenAutomaton, int]] = {}  # id(automaton) -> (it, its start state in the table)
        self._con_used = [0, 0]    # states and edges taken
        self._con_pending: List[TokenAutomaton] = []  # registered, rows not yet on the device (in table order)
        self._con_uploaded = [0, 0]
        self._con_table = None     # (row_ptr, default_next, edge_tok, edge_next, state int32 [max_live + 1]), made on first use
        if not 1 <= int(stop_states) <= stops.MD_STOP_STATES_MAX:
            raise ValueError(f"stop_states must be in 1 .. {stops.MD_STOP_STATES_MAX}")
        self.stop_states = int(stop_states)
        self._stop_start: Dict[tuple, int] = {}  # a stop set's strings -> the root of its automaton in the table
        self._stop_used = 0
        self._stop_pending: List[Tuple[int, stops.PackedStops]] = []  # registered, states not yet on the device
        self._stop_dev = None      # (trans int16, match_len int16, [match_id | id_ptr | ids | id_base | words] int32), made on first use
        self._stop_vocab = None    # the ONE vocabulary object whose bytes the engine's stop strings are matched in
        self.finishes: Dict[int, Finish] = {}  # rid -> how it ended, filled by ``run``
        self._penalty_hist = None  # (hist int32 [max_live + 1, max_context], hist_len int32 [max_live + 1]), made on first use

    @property
    def stats(self) -> EngineStats:
        return self.sched.stats

    # ---- submission
    def submit(self, image, prompt_ids: Sequence[int], max_tokens: int = DEFAULT_MAX_TOKENS, eos_id: Optional[int] = None,
               seed: Optional[int] = None, ignore_eos: bool = False, variant: Optional[str] = None,
               temperature: Optional[float] = None, top_p: Optional[float] = None, repetition_penalty: Optional[float] = None,
               presence_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None,
               constraint: Optional[TokenAutomaton] = None, top_k: Optional[int] = None, min_p: Optional[float] = None,
               spatial: Optional[Tuple[int, list]] = None, regex: Optional[str] = None, json_schema: Optional[dict] = None,
               vocab_bytes: Optional[Sequence[bytes]] = None, stop=None, stop_token_ids=None,
               include_stop_str_in_output: bool = False) -> int:
        """``stop`` (a str or a list of str) / ``stop_token_ids`` (a list of ids) / ``include_stop_str_in_output``:
        ``batch_generate_ids``' rule and validation for one row (``vocab_bytes`` spells the ids for stop strings where the
        tokenizer spells none); ValueError when the engine's stop table has no room for the set.
        Queue one request; ``image`` is a PIL image or an EncodedImage.  ``eos_id`` None: the tokenizer's EOS
        (``ignore_eos``: none).  ``temperature`` / ``top_p`` None: the engine's.  The three penalties (None: neutral):
        one number each, ``batch_generate_ids``' rule and validation.  ``constraint``: one ``TokenAutomaton`` (None: free),
        ``batch_generate_ids``' rule and validation; ValueError when the engine's table has no room for it.  ``regex`` /
        ``json_schema`` (with ``vocab_bytes`` where the tokenizer spells no bytes): compiled by the model's
        ``regex_constraint`` / ``json_constraint`` (cached there) into the request's ``constraint``; mutually exclusive with
        each other and with ``constraint``.  A compiled automaton can be large: size the engine's table for it.  ``top_k`` /
        ``min_p`` (None: off): one value each, ``batch_generate_ids``' rule and validation.  ``spatial``: what
        ``submit_query(spatial_refs=)`` builds -- (the position of the first placeholder in ``prompt_ids``, the checked
        refs), encoded into the prompt embeddings at admission.  Returns its id."""
        found = grammar_of(dict(regex=regex, json_schema=json_schema, constraint=constraint), "constraint")  # before anything else
        temp, tp = self._draw_settings(temperature, top_p)
        for name, x in (("repetition_penalty", repetition_penalty), ("presence_penalty", presence_penalty),
                        ("frequency_penalty", frequency_penalty)):
            if isinstance(x, (list, tuple)):
                raise ValueError(f"{name}: one number per request, not {x!r}")
        for name, x in (("top_k", top_k), ("min_p", min_p)):
            if isinstance(x, (list, tuple)):
                raise ValueError(f"{name}: one value per request, not {x!r}")
        row = CallSettings.of(1, None, temperature=temp, top_p=tp, repetition_penalty=repetition_penalty,
                              presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, top_k=top_k, min_p=min_p,
                              stop=stop, stop_token_ids=stop_token_ids, include_stop_str_in_output=include_stop_str_in_output,
                              vocab_size=self.model.config.text.vocab_size).rows[0]
        return self._enqueue(image, prompt_ids, max_tokens, eos_id, seed, ignore_eos, variant, replace(row, constraint=constraint),
                             spatial, found, vocab_bytes, include_stop_str_in_output)

    def _draw_settings(self, temperature, top_p) -> Tuple[float, float]:
        """A request's temperature and top-p (None: the engine's), in range: ValueError otherwise."""
        temp = self.temperature if temperature is None else float(temperature)
        tp = self.top_p if top_p is None else float(top_p)
        if not (math.isfinite(temp) and temp >= 0):
            raise ValueError(f"temperature must be finite and >= 0 (0: greedy), not {temp}")
        if not (math.isfinite(tp) and 0 < tp <= 1):
            raise ValueError(f"top_p must be in (0, 1], not {tp}")
        return temp, tp

    def _enqueue(self, image, prompt_ids: Sequence[int], max_tokens: int, eos_id: Optional[int], seed: Optional[int],
                 ignore_eos: bool, variant: Optional[str], row: RowSettings, spatial=None, grammar=None, vocab_bytes=None,
                 include_stop_str: bool = False) -> int:
        """Queue one request whose settings are parsed (``row``: its record; ``grammar``: ``grammar_of``'s pair, compiled
        here into the record's automaton): the checks of the request itself, then, last, what takes room in the engine's
        constraint table.  Returns its id."""
        from PIL import Image

        from .moondream import EncodedImage

        if not isinstance(image, (Image.Image, EncodedImage)):
            raise ValueError("image must be a PIL Image or EncodedImage")
        prompt = [int(p) for p in prompt_ids]
        if not prompt:
            raise ValueError("empty prompt")
        t = self.model.config.text
        prefix = image.pos if isinstance(image, EncodedImage) else 1 + self.model.config.vision.n_patches
        if prefix + len(prompt) > t.max_context:
            raise ValueError(f"image prefix + prompt ({prefix + len(prompt)} positions) do not fit the {t.max_context}-slot context")
        eos = None if ignore_eos else (self.model.config.tokenizer.eos_id if eos_id is None else int(eos_id))
        vidx = -1 if variant is None else self._variant_index(variant)
        if grammar is not None:  # (after every other check: this one compiles on the device)
            row = replace(row, constraint=self.model._grammar_constraint(*grammar, vocab_bytes))
        if row.stop is not None and row.stop.strings:  # (host only) the ONE vocabulary the engine's stop strings are spelled in
            spell = self.model._vocab_bytes("stop", vocab_bytes)
            if self._stop_vocab is not None and self._stop_vocab is not spell:
                raise ValueError("stop: one vocab_bytes object per engine (its stop strings are matched in one vocabulary)")
        if row.stop is not None:
            self._check_stop_room(row.stop)
        start = FREE if row.constraint is None else self._register_constraint(row.constraint)  # (last: nothing fails after it)
        stop_start = stops.NO_STOP
        if row.stop is not None:
            stop_start = self._register_stop(row.stop)
            if row.stop.strings:
                self._stop_vocab = spell
        rid = self._next_rid
        self._next_rid += 1
        self.sched.submit(Request(rid, image, prompt, int(max_tokens), eos, seed, variant=vidx, settings=row, constraint_start=start,
                                  spatial=spatial, stop_start=stop_start, include_stop_str=bool(include_stop_str)))
        return rid

    def _register_constraint(self, a: TokenAutomaton) -> int:
        """The start state of ``a`` in the engine's table, taking room for it on first use (by identity; the engine keeps
        the object).  Host values only: ValueError for what is no valid automaton of this model, or when the table is full."""
        if not isinstance(a, TokenAutomaton):
            raise ValueError(f"constraint must be a TokenAutomaton or None, not {a!r}")
        known = self._con_start.get(id(a))
        if known is not None:
            return known[1]
        a.validate(self.model.config.text.vocab_size, self.model.config.tokenizer.answer_id)
        states, edges = self._con_used
        if states + a.n_states > self.constraint_states or edges + a.n_edges > self.constraint_edges:
            raise ValueError(f"the engine's constraint table is full: {states} + {a.n_states} states of {self.constraint_states}, "
                             f"{edges} + {a.n_edges} edges of {self.constraint_edges} (ContinuousEngine(constraint_states=, "
                             "constraint_edges=))")
        self._con_start[id(a)] = (a, states)
        self._con_used = [states + a.n_states, edges + a.n_edges]
        self._con_pending.append(a)
        return states

    def _check_stop_room(self, s: stops.StopSet) -> None:
        """ValueError when the engine's stop table cannot take ``s`` (host values only; nothing is taken)."""
        if s.strings in self._stop_start:
            return
        n = int(s.dfa()[1].shape[0])
        if self._stop_used + n > self.stop_states:
            raise ValueError(f"the engine's stop table is full: {self._stop_used} + {n} states of {self.stop_states} "
                             "(ContinuousEngine(stop_states=))")

    def _register_stop(self, s: stops.StopSet) -> int:
        """The root of ``s``'s automaton in the engine's table, taking room for it on first use (by its strings: the ids
        play no part in the automaton; a set of ids alone is the one-state automaton)."""
        known = self._stop_start.get(s.strings)
        if known is not None:
            return known
        self._check_stop_room(s)
        t = stops.pack([s], self._stop_used)
        self._stop_start[s.strings] = self._stop_used
        self._stop_pending.append((self._stop_used, t))
        self._stop_used += t.n_states
        return self._stop_start[s.strings]

    def _stop_record(self):
        """The engine's stop table and per-slot words as a ``Stop`` record (``by_slot``), made on first use; the states of
        stop sets registered since the last call are appended first, by small pinned copies behind the stream.  Slot
        ``max_live`` is a spare nobody decodes in.  Row s's ids are ``ids[16 s .. 16 s + 16)``, -1 where it has fewer."""
        import torch

        m = self.model
        n = self.max_live + 1
        if self._stop_dev is None:
            cap, k = self.stop_states, stops.STOP_IDS_MAX
            i32 = torch.zeros(cap + (n + 1) + n * k + n + 6 * n, dtype=torch.int32, device=m.device)
            mid, ptr, ids, base, words = torch.split(i32, [cap, n + 1, n * k, n, 6 * n])
            mid.fill_(-1)
            ptr.copy_(torch.arange(n + 1, dtype=torch.int32, device=m.device) * k)
            ids.fill_(-1)
            words = words.view(6, n)
            words[0].fill_(stops.NO_STOP)
            words[3].fill_(-1)
            self._stop_dev = (torch.zeros(cap * 256, dtype=torch.int16, device=m.device),
                              torch.zeros(cap, dtype=torch.int16, device=m.device), mid, ptr, ids, base, words)
        trans, mlen, mid, ptr, ids, base, words = self._stop_dev
        for s0, t in self._stop_pending:
            up = lambda dst, at, src: dst[at : at + src.size].copy_(m._h2d(torch.from_numpy(np.ascontiguousarray(src).reshape(-1))))
            up(trans, s0 * 256, t.trans.view(np.int16))
            up(mlen, s0, t.match_len.view(np.int16))
            up(mid, s0, t.match_id)
        self._stop_pending = []
        tok_off = tok_bytes = None
        vocab = n_bytes = 0
        if self._stop_vocab is not None:
            tok_off, tok_bytes, n_bytes = m._vocab_on_device(self._stop_vocab)
            vocab = m.config.text.vocab_size
        return Stop(trans, mlen, mid, ptr, ids, base, tok_off, tok_bytes, vocab, n_bytes, words, self.stop_states, by_slot=True)

    def _admit_stops(self, rows: List[Request], first, table):
        """At admission, after the first tokens are picked: every admitted slot's matcher words are reset to its request's
        (root state or NO_STOP, nothing seen, nothing matched; its ids and id base beside them) by one pinned copy and
        three index copies on the stream, then ONE md_stop_rows launch feeds ``first`` (int32 [len(rows)], ``table``: the
        rows' routing).  Returns the rows' (at, keep, which) as a device tensor [3, len(rows)] for the admission's host copy."""
        import torch

        m = self.model
        rec = self._stop_record()
        k, n = stops.STOP_IDS_MAX, len(rows)
        host = np.zeros((7 + k, n), dtype=np.int32)  # [words (6) | id base | ids (k)] per column
        host[7:] = -1
        for c, r in enumerate(rows):
            s = r.settings.stop
            host[0, c], host[3, c], host[5, c] = r.stop_start, -1, -1
            if s is not None:
                host[6, c] = len(s.strings)
                host[7 : 7 + len(s.token_ids), c] = s.token_ids
        dev = m._h2d(torch.from_numpy(host))
        idx = table.slots.to(torch.int64)
        rec.words.index_copy_(1, idx, dev[:6])
        rec.id_base.index_copy_(0, idx, dev[6])
        rec.ids.view(-1, k).index_copy_(0, idx, dev[7:].t().contiguous())
        m._stop_rows(first, table, rec)
        return rec.words[3:6].index_select(1, idx)

    def _variant_index(self, variant: str) -> int:
        """The bank index of a LoRA variant the model can resolve (registered, or in the on-disk cache); ValueError otherwise,
        before any GPU work (the lookup precedes the packing)."""
        resolve = getattr(self.model, "_bank_index", None)
        if resolve is None:
            raise ValueError(f"this model serves no LoRA variants (asked for {variant!r})")
        try:
            return int(resolve(variant))
        except (FileNotFoundError, KeyError) as e:
            raise ValueError(f"unknown LoRA variant {variant!r}") from e

    def submit_caption(self, image, length: str = "normal", **kw) -> int:
        """The prompt ``batch_caption`` builds."""
        tpl = self.model.config.tokenizer.templates["caption"]
        if tpl is None:
            raise NotImplementedError("Model does not support captioning.")
        if length not in tpl:
            raise ValueError(f"Model does not support caption length '{length}'.")
        return self.submit(image, tpl[length], **kw)

    def submit_query(self, image, question: str, spatial_refs=None, **kw) -> int:
        """The prompt ``batch_query`` builds.  ``spatial_refs``: the request's points ``(x, y)`` / boxes ``(x0, y0, x1,
        y1)`` in front of the question, ``batch_query``'s rule and validation for one row; they are a property of the
        request, encoded into its prompt embeddings when it is admitted (md_spatial_ref_embed, through the model's one
        sequence preparation)."""
        tk = self.model.config.tokenizer
        tpl = tk.templates["query"]
        if tpl is None:
            raise NotImplementedError("Model does not support querying.")
        q = list(self.model.tokenizer.encode(question).ids)
        refs = []
        if spatial_refs is not None:
            rows = check_spatial_refs([spatial_refs], 1, [image is not None], [q], tk.coord_id, tk.size_id,
                                      getattr(self.model.w, "region", None) is not None)
            refs = rows[0] if rows else []
        prompt = spatial_prompt_ids(tpl["prefix"], refs, q + list(tpl["suffix"]) + list(tpl["suffix"]), tk.coord_id, tk.size_id)
        return self.submit(image, prompt, **kw, **({"spatial": (len(tpl["prefix"]), refs)} if refs else {}))

    # ---- running
    def run(self, with_logprobs: bool = False, with_alternatives: Optional[bool] = None) -> Iterator[tuple]:
        """Generate every queued request; yields (rid, ids) in completion order -- with ``with_logprobs`` (an engine made with
        ``logprobs=True``) (rid, ids, logprobs, ranks), and on an engine with ``top_logprobs`` (rid, ids, logprobs, ranks,
        alternatives).  ``with_alternatives`` True insists on the fifth element (ValueError on an engine without
        ``top_logprobs``, or without ``with_logprobs``), False leaves it out; None: whatever the engine has.  Requests
        submitted while this runs are admitted too.  ``stats`` counts this run."""
        import torch

        if with_logprobs and not self.logprobs:
            raise ValueError("run(with_logprobs=True) needs ContinuousEngine(..., logprobs=True)")
        if with_alternatives and not (with_logprobs and self.top_logprobs):
            raise ValueError("run(with_logprobs=True, with_alternatives=True) needs ContinuousEngine(..., logprobs=True, top_logprobs=k)")
        alts = bool(self.top_logprobs) if with_alternatives is None else bool(with_alternatives)
        self.sched.stats = EngineStats()
        with torch.inference_mode():
            self._prepare_run()
            for r in self.sched.run(self._admit, self._step):
                self.finishes[r.rid] = r.finish
                if not with_logprobs:
                    yield r.rid, list(r.ids)
                else:
                    yield (r.rid, list(r.ids), list(r.logprobs), list(r.ranks)) + ((list(r.alternatives),) if alts else ())

    def _prepare_run(self) -> None:
        """Size the KV slab (once, before the first admission: never grown during a run) and the decode buffers of the
        largest bucket, so that arena growth does not invalidate captured chunks mid-run."""
        m = self.model
        m._ensure_batch(self.max_live)
        m._select_kernels(2)  # MD_TILE_PINNED: a request's bits do not depend on what else is launched
        top = self.sched.buckets[-1]
        m._decode_logits(top)
        m._workspace(self._decode_ws_bytes(top), 2)
        self._kv_ptr = m._kv_k.data_ptr()

    def _decode_ws_bytes(self, bucket: int) -> int:
        """A decode chunk's workspace: the multi-LoRA step's once the model has a bank (it covers the plain step too)."""
        import torch

        bank = getattr(self.model, "_bank", None)
        none = torch.empty(0, dtype=torch.int32)  # (sizing reads which tables there are, not the tables)
        return self.model._decode_ws_bytes(self._rows(none, none if bank is not None and len(bank) else None), bucket)

    def _rows(self, slots, variants=None):
        """The routing of a call over this engine's slab: a slot table, and with ``variants`` a row-variant table of the
        model's bank."""
        from .moondream import _Rows

        return _Rows(slots=slots, n_slots=self.max_live, variants=variants, bank=self.model._bank if variants is not None else None)

    def run_text(self) -> Iterator[Tuple[int, str]]:
        """``run`` as text: the tokenizer's decoding of the ids; a request that stopped on a stop STRING returns the bytes
        of its ids cut to ``Finish.text_bytes``, decoded as UTF-8 with ``errors="replace"``."""
        for rid, ids in self.run():
            f = self.finishes.get(rid)
            if f is not None and f.text_bytes is not None:
                yield rid, stops.cut_text([self._stop_vocab[t] for t in ids], f).decode("utf-8", errors="replace")
            else:
                yield rid, self.model.tokenizer.decode(ids)

    def generate(self, images, prompts: Sequence[Sequence[int]], max_tokens: Union[int, Sequence[int]] = DEFAULT_MAX_TOKENS,
                 eos_id: Optional[int] = None, ignore_eos: bool = False, seeds: Optional[Sequence[Optional[int]]] = None,
                 variant: Optional[str] = None, temperature: Union[None, float, Sequence[float]] = None,
                 top_p: Union[None, float, Sequence[float]] = None, return_logprobs: bool = False,
                 repetition_penalty: Union[None, float, Sequence[float]] = None,
                 presence_penalty: Union[None, float, Sequence[float]] = None,
                 frequency_penalty: Union[None, float, Sequence[float]] = None,
                 constraints: Union[None, TokenAutomaton, Sequence[Optional[TokenAutomaton]]] = None,
                 top_k: Union[None, int, Sequence[int]] = None, min_p: Union[None, float, Sequence[float]] = None,
                 stop=None, stop_token_ids=None, include_stop_str_in_output: bool = False, vocab_bytes=None,
                 return_finish: bool = False):
        """``stop`` / ``stop_token_ids``: one value for every request or one entry per request, ``batch_generate_ids``'
        forms and rule; ``return_finish`` appends the requests' ``Finish`` records, in input order, to the return value.
        Ids for (images[i], prompts[i]) in input order; ``max_tokens`` one int or one per request, ``temperature`` and
        ``top_p`` one float or one per request (None: the engine's), the three penalties likewise (None: neutral),
        ``constraints`` one ``TokenAutomaton`` or one entry per request (None: free), ``top_k`` / ``min_p`` one value or
        one per request (None: off).  ``return_logprobs`` (an engine made with
        ``logprobs=True``): (ids, logprobs, ranks), each in input order; an engine with ``top_logprobs``: alternatives too."""
        if return_logprobs and not self.logprobs:
            raise ValueError("generate(return_logprobs=True) needs ContinuousEngine(..., logprobs=True)")
        n = len(images)
        if len(prompts) != n:
            raise ValueError("images and prompts differ in length")
        mt = [int(max_tokens)] * n if isinstance(max_tokens, (int, np.integer)) else [int(x) for x in max_tokens]
        if len(mt) != n:
            raise ValueError("one max_tokens per request")
        seeds = list(seeds) if seeds is not None else [None] * n

        def per_request(x, name):
            if x is None or isinstance(x, (int, float, np.integer, np.floating)):
                return [x] * n
            x = list(x)
            if len(x) != n:
                raise ValueError(f"one {name} per request")
            return x

        draws = [self._draw_settings(*pair) for pair in zip(per_request(temperature, "temperature"), per_request(top_p, "top_p"))]
        if isinstance(constraints, (list, tuple)) and len(constraints) != n:
            raise ValueError(f"constraints: {len(constraints)} entries for {n} requests (one TokenAutomaton, or one entry per request)")
        cfg = self.model.config
        st = CallSettings.of(n, lambda c, k: check_constraints(c, k, cfg.text.vocab_size, cfg.tokenizer.answer_id),
                             temperature=[d[0] for d in draws], top_p=[d[1] for d in draws], repetition_penalty=repetition_penalty,
                             presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, constraints=constraints,
                             top_k=top_k, min_p=min_p, stop=stop, stop_token_ids=stop_token_ids,
                             include_stop_str_in_output=include_stop_str_in_output, vocab_size=cfg.text.vocab_size)
        for s in dict.fromkeys(r.stop for r in st.rows if r.stop is not None):  # every request is checked before the first is queued
            if s.strings:
                self.model._vocab_bytes("stop", vocab_bytes)
        rids = [self._enqueue(images[i], prompts[i], mt[i], eos_id, seeds[i], ignore_eos, variant, st.rows[i],
                              vocab_bytes=vocab_bytes, include_stop_str=st.include_stop_str) for i in range(n)]
        ends = lambda: ([self.finishes[r] for r in rids],) if return_finish else ()
        if return_logprobs:  # (ids, logprobs, ranks), and alternatives on an engine with top_logprobs
            got3 = {rid: rest for rid, *rest in self.run(with_logprobs=True)}
            return tuple([got3[r][k] for r in rids] for k in range(4 if self.top_logprobs else 3)) + ends()
        got = dict(self.run())
        return ([got[r] for r in rids],) + ends() if return_finish else [got[r] for r in rids]

    # ---- the GPU side of the schedule
    def _generator(self, r: Request):
        import torch

        if r.generator is None:
            g = torch.Generator()
            if r.seed is None:
                g.seed()
            else:
                g.manual_seed(int(r.seed))
            r.generator = g
        return r.generator

    def _uniforms(self, r: Request, n: int):
        import torch

        return torch.rand(n, dtype=torch.float32, generator=self._generator(r))

    def _table(self, reqs: List[Request]):
        """The routing of a call with one row per request of ``reqs``: their slots, and their variants when one of them has
        one, in one H2D copy."""
        import torch

        lora = any(r.variant >= 0 for r in reqs)
        tab = self.model._h2d(torch.tensor([[r.slot for r in reqs]] + ([[r.variant for r in reqs]] if lora else []), dtype=torch.int32))
        return self._rows(tab[0], tab[1] if lora else None)

    def _admit(self, reqs: List[Request]) -> List[Tuple[int, int]]:
        """The prefill of ``reqs`` into their slots, through the pieces of ``MoondreamModel._prepare_sequences`` and with its
        choices: [bos | image | prompt] in one pass per prompt length when every image is raw and ``fused_prefill`` is on;
        otherwise ``_place_images`` (ONE ViT batch and ONE [bos | image] pass over the raw images, every EncodedImage loaded
        into its request's slot), then the prompt passes per (prefix, prompt length).  The engine's own part is the shape
        of the groups and the rows' records; its three launch rules, which keep a request's ids independent of what else
        is admitted: a prompt pass of t <= 64 positions after a placed image has at most max(1, 64 // t) rows; lm_head and
        the first pick run in cuts of at most 64 rows; a pass takes the variant table only if one of its rows has a variant.
        Returns, per request, (first token, next position), then its (logprob, rank) with ``logprobs``, then its
        alternatives' (ids, logprobs) with ``top_logprobs``."""
        import torch
        from PIL import Image

        m = self.model
        m._select_kernels(2)  # (again: another call on the model may have run between two chunks of this generator)
        raw = [r for r in reqs if isinstance(r.image, Image.Image)]
        fused = len(raw) == len(reqs) and m.fused_prefill
        prefix = {r: 0 for r in reqs}  # a fused pass starts at the bos
        if not fused:
            placed = raw + [r for r in reqs if r not in raw]  # the raw rows first: one run, so one [bos | image] pass
            got = m._place_images([r.image for r in placed], self._table(raw) if raw else None, lambda name: None,
                                  slots=[r.slot for r in placed])
            prefix = dict(zip(placed, got))
            self.stats.prefill_passes += bool(raw)
        by_key: Dict[Tuple[int, int], List[Request]] = {}  # in order of first appearance
        for r in reqs:
            by_key.setdefault((prefix[r], len(r.prompt)), []).append(r)
        rows: List[Request] = []  # the admission's rows, every pass a range of them
        groups, starts = [], []
        for (p, t), members in by_key.items():
            per = len(members) if fused or t > 64 else max(1, 64 // t)
            for j0 in range(0, len(members), per):
                groups.append((len(rows) + j0, len(rows) + min(j0 + per, len(members))))
                starts.append(p)
            rows += members
        table = self._table(rows)
        base = replace(table, variants=None, bank=None)
        routes = [(table if any(r.variant >= 0 for r in rows[r0:r1]) else base).sub(r0, r1) for r0, r1 in groups]
        pick = st = con = None
        if any(r.settings.sampled for r in rows):
            # one H2D copy of [temperature | top_p | uniform] rows; a greedy request draws nothing
            draws = [float(self._uniforms(r, 1)[0]) if r.settings.sampled else 0.0 for r in rows]
            st = m._h2d(torch.tensor([[r.settings.temperature for r in rows], [r.settings.top_p for r in rows], draws], dtype=torch.float32))
            pick = Sampling(st[0], st[1])
            if any(r.settings.filtered for r in rows):  # two more rows of settings: the first token is cut too
                pick = replace(pick, top_k=m._h2d(torch.tensor([r.settings.top_k for r in rows], dtype=torch.int32)),
                               min_p=m._h2d(torch.tensor([r.settings.min_p for r in rows], dtype=torch.float32)))
        if any(r.settings.constrained for r in rows):  # the rows' start states, beside the engine's table
            con = self._constraint(m._h2d(torch.tensor([r.constraint_start for r in rows], dtype=torch.int32)), by_slot=False)
        scores = Scores.new((len(rows),), self.top_logprobs, m.device) if self.logprobs else None
        spatial = None
        if any(r.spatial for r in rows):  # the rows' references: one record, one upload, one launch per pass
            spatial = SpatialRecord.build([r.spatial[1] if r.spatial else [] for r in rows],
                                          [r.spatial[0] if r.spatial else 0 for r in rows], [len(r.prompt) for r in rows])
        embed = m._sequence_embeddings([r.prompt for r in rows], [r.image for r in rows] if fused else None, spatial=spatial)
        first, _, next_pos = m._prefill_groups(groups, embed, starts, routes, pick, scores=scores, constraint=con,
                                               uniforms=st[2] if st is not None else None, head_rows=64)
        self.stats.prefill_passes += len(groups)
        # once the engine has seen a stop set every admitted slot's matcher is reset, and the first tokens go through it
        trip = self._admit_stops(rows, first, table) if self._stop_start else None
        ride = (first,) if trip is None else (first, trip)
        if scores is None:
            flat = (first if trip is None else torch.cat([first, trip.reshape(-1)])).tolist()
            picked = [(f,) for f in flat[: len(rows)]]
            hits = np.asarray(flat[len(rows) :], dtype=np.int64).reshape(3, len(rows)) if trip is not None else None
        else:
            host = scores.to_host(*ride)  # the tokens, the matchers' results and the scores in one copy
            top = [zip(host.top_ids, host.top_logprobs)] if self.top_logprobs else []
            picked = list(zip(host.extra[0].tolist(), host.logprob.tolist(), host.rank.tolist(), *top))
            hits = host.extra[1] if trip is not None else None
        for c, r in enumerate(rows):
            r.stop_hit = tuple(int(x) for x in hits[:, c]) if hits is not None and r.settings.stop is not None else None
        started = {r: (int(f[0]), pos) + tuple(f[1:]) for r, f, pos in zip(rows, picked, next_pos)}
        return [started[r] for r in reqs]

    def _buffers(self, bucket: int):
        """Fixed-address buffers of a (chunk, bucket): int32 device state [slots (chunk x bucket) | pos (bucket) | tokens ((chunk + 1) x
        bucket) | row variants (bucket)] with its pinned host staging (one H2D copy of everything a chunk reads), and fp32
        [uniforms (chunk x bucket) | temperature (bucket) | top_p (bucket)] with its own, one more copy that only chunks with a
        sampling row make.  The row-variant table sits next to the slot table; only chunks with a LoRA row read it."""
        import torch

        def make():
            c = self.chunk
            n_in = c * bucket + bucket + bucket
            dev = torch.zeros(n_in + c * bucket + bucket, dtype=torch.int32, device=self.model.device)
            with torch.inference_mode(False):
                host = torch.zeros(n_in + bucket, dtype=torch.int32, pin_memory=True)
                u_host = torch.zeros(c * bucket + 2 * bucket, dtype=torch.float32, pin_memory=True)
            u_dev = torch.zeros(c * bucket + 2 * bucket, dtype=torch.float32, device=self.model.device)
            return dev, host, u_dev, u_host, n_in

        return self.model._store.fixed("continuous", (self.chunk, bucket), make)  # the model's: its engines share captured chunks

    def _penalty_buffers(self, bucket: int):
        """What a chunk with a penalised row needs beside ``_buffers``: the engine's histories (one per KV slot, and a spare
        one past them where the length resets of rows that need none land) and, per bucket, the fixed-address settings fp32
        [repetition | presence | frequency] (bucket each) and reset indices int64 [bucket], each with its pinned staging."""
        import torch

        m = self.model
        if self._penalty_hist is None:
            cap = min(m.config.text.max_context, MD_PENALTY_HIST_MAX)  # (a request generates fewer tokens than either)
            self._penalty_hist = (torch.zeros(self.max_live + 1, cap, dtype=torch.int32, device=m.device),
                                  torch.zeros(self.max_live + 1, dtype=torch.int32, device=m.device))

        def make():
            with torch.inference_mode(False):
                st_host = torch.zeros(3 * bucket, dtype=torch.float32, pin_memory=True)
                rs_host = torch.zeros(bucket, dtype=torch.int64, pin_memory=True)
            return (torch.zeros(3 * bucket, dtype=torch.float32, device=m.device), st_host,
                    torch.zeros(bucket, dtype=torch.int64, device=m.device), rs_host)

        return self._penalty_hist + m._store.fixed("continuous_penalty", bucket, make)

    def _filter_buffers(self, bucket: int):
        """Per bucket, fixed addresses: the rows' top_k (int32 [bucket]) and min_p (fp32 [bucket]), each with its pinned
        staging -- what a chunk with a filtered row reads beside ``_buffers``' temperature and top-p."""
        import torch

        def make():
            with torch.inference_mode(False):
                k_host = torch.zeros(bucket, dtype=torch.int32, pin_memory=True)
                m_host = torch.zeros(bucket, dtype=torch.float32, pin_memory=True)
            return (torch.zeros(bucket, dtype=torch.int32, device=self.model.device), k_host,
                    torch.zeros(bucket, dtype=torch.float32, device=self.model.device), m_host)

        return self.model._store.fixed("continuous_filters", bucket, make)

    def _constraint(self, state=None, by_slot: bool = True) -> Constraint:
        """The engine's table as a ``Constraint`` record over ``state`` (None: the per-slot states), made on first use;
        the rows of automata registered since the last call are appended first, by small pinned copies behind the stream."""
        import torch

        m = self.model
        if self._con_table is None:
            s, e = self.constraint_states, self.constraint_edges
            z = lambda n, fill=0: torch.full((n,), fill, dtype=torch.int32, device=m.device)
            self._con_table = (z(s + 1), z(s, FREE), z(e), z(e), z(self.max_live + 1, FREE))
        row_ptr, default_next, edge_tok, edge_next, slot_state = self._con_table
        if self._con_pending:
            s0, e0 = self._con_uploaded
            t = pack(self._con_pending, s0, e0)
            up = lambda dst, at, src: dst[at : at + len(src)].copy_(m._h2d(torch.from_numpy(src))) if len(src) else None
            up(row_ptr, s0 + 1, t.row_ptr[1:])  # (entry s0 is the end of what was there: e0, or the 0 the table starts with)
            up(default_next, s0, t.default_next)
            up(edge_tok, e0, t.edge_tok)
            up(edge_next, e0, t.edge_next)
            self._con_uploaded = [s0 + t.n_states, e0 + t.n_edges]
            self._con_pending = []
        return Constraint(row_ptr, default_next, edge_tok, edge_next, slot_state if state is None else state,
                          self.constraint_states, by_slot=by_slot)

    def _constraint_buffers(self, bucket: int):
        """Per bucket, fixed addresses: the slots (int64 [bucket]) and start states (int32 [bucket]) of a chunk's state
        resets, each with its pinned staging."""
        import torch

        def make():
            with torch.inference_mode(False):
                i_host = torch.zeros(bucket, dtype=torch.int64, pin_memory=True)
                v_host = torch.zeros(bucket, dtype=torch.int32, pin_memory=True)
            return (torch.zeros(bucket, dtype=torch.int64, device=self.model.device), i_host,
                    torch.zeros(bucket, dtype=torch.int32, device=self.model.device), v_host)

        return self.model._store.fixed("continuous_constraint", bucket, make)

    def _score_buffers(self, bucket: int):
        """The fixed-address ``Scores`` over (chunk, bucket) with the engine's k that a chunk's steps fill (``logprobs`` only)."""
        return self.model._store.fixed("continuous_scores", (self.chunk, bucket, self.top_logprobs),
                                       lambda: Scores.new((self.chunk, bucket), self.top_logprobs, self.model.device))

    def _step(self, plan: ChunkPlan) -> np.ndarray:
        import torch

        m = self.model
        if m._kv_k.data_ptr() != self._kv_ptr:
            raise RuntimeError("the KV slab was reallocated during a continuous-batching run")
        c, B, n = self.chunk, plan.bucket, plan.n
        dev, host, u_dev, u_host, n_in = self._buffers(B)
        slots_d = dev[: c * B].view(c, B)
        pos_d = dev[c * B : c * B + B]
        hist = dev[c * B + B : n_in + c * B].view(c + 1, B)
        var_d = dev[n_in + c * B :]
        hs = host.numpy()
        hs[: c * B].reshape(c, B)[:n] = plan.slots
        hs[c * B : c * B + B] = plan.pos
        hs[c * B + B : n_in] = plan.tokens
        row_var = [r.variant for r in plan.rows]
        lora = any(v >= 0 for v in row_var)
        dev[:n_in].copy_(host[:n_in], non_blocking=True)
        if lora:
            hs[n_in:] = -1
            hs[n_in : n_in + len(row_var)] = row_var
            var_d.copy_(host[n_in:], non_blocking=True)
        sample = any(r.settings.sampled for r in plan.rows)
        if sample:
            fh = u_host.numpy()
            uh, th, ph = fh[: c * B].reshape(c, B), fh[c * B : c * B + B], fh[c * B + B :]
            uh[:] = 0.5
            th[:] = -1.0  # rows past the plan's are idle: md_sample_rows leaves them alone
            ph[:] = 1.0
            for r_idx, r in enumerate(plan.rows):
                th[r_idx], ph[r_idx] = r.settings.temperature, r.settings.top_p
                if r.settings.sampled:  # a greedy request draws nothing from its generator
                    k = min(n, r.remaining)
                    uh[:k, r_idx] = self._uniforms(r, k).numpy()
            u_dev.copy_(u_host, non_blocking=True)
        filt = None
        if any(r.settings.filtered for r in plan.rows):  # (sampled rows: ``sample`` holds) the rows' cuts, padding rows off
            k_dev, k_host, m_dev, m_host = self._filter_buffers(B)
            kh, mh = k_host.numpy(), m_host.numpy()
            kh[:], mh[:] = 0, 0.0
            for r_idx, r in enumerate(plan.rows):
                kh[r_idx], mh[r_idx] = r.settings.top_k, r.settings.min_p  # (``check_filters``: top_k below 2^31)
            k_dev.copy_(k_host, non_blocking=True)
            m_dev.copy_(m_host, non_blocking=True)
            filt = (k_dev, m_dev)
        penalty = None
        if any(r.settings.penalised for r in plan.rows):
            # the rows' settings (padding rows neutral) and the slots whose history starts here, in two small copies behind
            # the chunk's others; the lengths are zeroed on the stream, before the chunk's first launch
            p_hist, p_len, st_dev, st_host, rs_dev, rs_host = self._penalty_buffers(B)
            sh = st_host.numpy().reshape(3, B)
            sh[:] = np.asarray(PENALTY_NEUTRAL, dtype=np.float32)[:, None]
            sh[:, : len(plan.rows)] = np.asarray([r.settings.penalties for r in plan.rows], dtype=np.float32).T
            rs_host.numpy()[:] = np.where(plan.fresh >= 0, plan.fresh, self.max_live)
            st_dev.copy_(st_host, non_blocking=True)
            rs_dev.copy_(rs_host, non_blocking=True)
            p_len.index_fill_(0, rs_dev, 0)
            penalty = Penalty(st_dev[:B], st_dev[B : 2 * B], st_dev[2 * B :], p_hist, p_len, p_hist.shape[1], by_slot=True)
        constraint = None
        if self._con_start:
            # once the engine has seen an automaton every refilled slot's state is rewritten, a free request's too (FREE):
            # a later chunk may run the constraint launch over this slot.  Only chunks with a constrained row launch it.
            con = self._constraint()
            i_dev, i_host, v_dev, v_host = self._constraint_buffers(B)
            i_host.numpy()[:], v_host.numpy()[:] = SlotScheduler.state_resets(plan, self.max_live)
            i_dev.copy_(i_host, non_blocking=True)
            v_dev.copy_(v_host, non_blocking=True)
            con.state.index_copy_(0, i_dev, v_dev)
            if any(r.settings.constrained for r in plan.rows):
                constraint = con
        stop = None
        if any(r.settings.stop is not None for r in plan.rows):  # (their words were reset at admission)
            stop = self._stop_record()
        scores = self._score_buffers(B) if self.logprobs else None  # (an idle or padding row's are never read: SlotScheduler.commit)
        # step i's routing: row i of the slot table; a LoRA row in the chunk: the chunk's row-variant table with it
        rows_of = lambda i: self._rows(slots_d[i], var_d if lora else None)
        # a sampling row in the chunk: every row picks with its own settings (a greedy row its argmax again, an idle row
        # nothing); the settings are device data, in the allocation of the uniforms
        pick = Sampling(u_dev[c * B : c * B + B], u_dev[c * B + B :]) if sample else None
        if filt is not None:  # ... and a filtered row: the launch that also cuts by each row's top_k / min_p
            pick = replace(pick, top_k=filt[0], min_p=filt[1])
        chunk = DecodeChunk(B, hist, pos_d, rows_of, m.config.tokenizer.answer_id, self._decode_ws_bytes(B), pick,
                            u_dev[: c * B].view(c, B), penalty=penalty, constraint=constraint, stop=stop,
                            **(scores.chunk_fields() if scores else {}))
        stream = torch.cuda.current_stream(m.device).cuda_stream if m.use_graphs else None
        if run_chunk(m, chunk, n, "continuous", stream, lambda: m._store.count("continuous", stream) < MAX_GRAPHS):
            self.stats.graph_captures += 1
        kw = ()
        if stop is None:
            out = hist[1 : n + 1].cpu().numpy()  # the chunk's D2H copy of the ids (the lockstep loop syncs here too)
        else:  # ... with the rows' (at, keep, which) behind them: step 0's slot table names every live row's slot
            trip = stop.words[3:6].index_select(1, slots_d[0].to(torch.int64).clamp_(min=0))
            flat = torch.cat([hist[1 : n + 1].reshape(-1), trip.reshape(-1)]).cpu().numpy()
            out, kw = flat[: n * B].reshape(n, B), ({"stop": tuple(flat[n * B :].reshape(3, B))},)
        if scores is None:
            return (out,) + kw if kw else out
        host = scores[:n].to_host()  # ... and one more of the chunk's scores
        return (out, host.logprob, host.rank) + ((host.top_ids, host.top_logprobs) if self.top_logprobs else ()) + kw
