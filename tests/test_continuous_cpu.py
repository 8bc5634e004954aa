"""Continuous batching without a GPU: the slot scheduler against a fake step function with a known token stream, the
engine's bookkeeping on a fake model, and host-side argument validation of the slot-table entry points."""
import ctypes

import numpy as np
import pytest
from PIL import Image

from moondream_amd import _lib
from moondream_amd.config import get_config
from moondream_amd.continuous import IDLE_SLOT, ContinuousEngine, Request, SlotScheduler, row_buckets
from moondream_amd.moondream import MoondreamModel

PREFIX = 730


def stream(rid, k):
    """Token k of request rid (k = 0: the prefill's pick): never 0, deterministic."""
    return 1 + (rid * 7 + k * 3) % 50


def lockstep_ids(rid, pos, max_tokens, eos, max_context, eos_at=None):
    """What the lockstep loop returns: max_tokens steps capped by the context, then MoondreamModel._truncate."""
    s = max(0, min(max_tokens, max_context - 1 - pos))
    toks = [eos if (eos_at is not None and k == eos_at) else stream(rid, k) for k in range(s + 1)]
    return MoondreamModel._truncate(toks, eos, max_tokens)


class Fake:
    """admit / step functions of SlotScheduler.run that check the schedule's invariants on every chunk."""

    def __init__(self, sched, eos_at=None):
        self.sched = sched
        self.eos_at = eos_at or {}
        self.slot_log = []  # (rid, slot) in admission order
        self.chunks = 0

    def tok(self, r, k):
        return r.eos_id if self.eos_at.get(r.rid) == k else stream(r.rid, k)

    def admit(self, reqs):
        live_slots = {r.slot for r in self.sched.live}
        for r in reqs:
            assert 0 <= r.slot < self.sched.max_live and r.slot not in live_slots
            live_slots.add(r.slot)
            self.slot_log.append((r.rid, r.slot))
        return [(self.tok(r, 0), PREFIX + len(r.prompt)) for r in reqs]

    def step(self, plan):
        self.chunks += 1
        assert plan.bucket in self.sched.buckets and len(plan.rows) <= plan.bucket
        assert plan.slots.shape == (plan.n, plan.bucket)
        assert (plan.slots[:, len(plan.rows):] == IDLE_SLOT).all()  # bucket padding
        for i in range(plan.n):
            used = [int(s) for s in plan.slots[i] if s >= 0]
            assert len(used) == len(set(used)), f"two live rows share a slot: {plan.slots[i]}"
        out = np.zeros((plan.n, plan.bucket), dtype=np.int32)
        for j, r in enumerate(plan.rows):
            assert plan.pos[j] == r.pos and plan.tokens[j] == r.last
            for i in range(plan.n):
                out[i, j] = self.tok(r, r.steps + i + 1) if plan.slots[i, j] >= 0 else 0
        return out


def run_schedule(reqs, max_live, chunk=4, max_context=2048, eos_at=None, admit_threshold=None):
    sched = SlotScheduler(max_live, max_context, chunk, admit_threshold)
    for r in reqs:
        sched.submit(r)
    fake = Fake(sched, eos_at)
    done = list(sched.run(fake.admit, fake.step))
    return sched, fake, done


def test_buckets_cover_every_row_count_and_stay_bounded():
    for n in (1, 3, 4, 12, 64, 100, 128, 256, 1000):
        b = row_buckets(n)
        assert b[-1] == n and b == sorted(set(b)) and len(b) <= 16, (n, b)


def test_ragged_lengths_equal_lockstep_and_slots_never_shared():
    rng = np.random.default_rng(0)
    n = 23
    mt = [int(x) for x in rng.integers(0, 20, n)]
    prompts = [[5] * (1 + i % 3) for i in range(n)]
    reqs = [Request(i, None, prompts[i], mt[i], eos_id=0) for i in range(n)]
    sched, fake, done = run_schedule(reqs, max_live=5)
    assert sorted(r.rid for r in done) == list(range(n))
    for r in done:
        assert r.ids == lockstep_ids(r.rid, PREFIX + len(r.prompt), mt[r.rid], 0, 2048), r.rid
    assert sched.stats.admissions > 1 and not sched.live and sorted(sched.free) == list(range(5))
    # a request takes max_tokens - 1 decode steps: the live row-steps are exactly that
    assert sched.stats.live_row_steps == sum(max(0, x - 1) for x in mt)
    assert sched.stats.padded_row_steps >= sched.stats.live_row_steps


def test_retirement_at_eos():
    n = 8
    eos_at = {0: 0, 1: 1, 2: 5, 3: 9, 5: 3}
    reqs = [Request(i, None, [5, 6], 12, eos_id=0) for i in range(n)]
    sched, fake, done = run_schedule(reqs, max_live=3, eos_at=eos_at)
    for r in done:
        assert r.ids == lockstep_ids(r.rid, PREFIX + 2, 12, 0, 2048, eos_at.get(r.rid)), r.rid
    assert done[0].rid == 0 and done[0].ids == []  # EOS as the first token: done at admission


def test_retirement_at_the_context_limit_matches_truncate():
    max_context = PREFIX + 2 + 7  # 6 decode steps fit after a 2-token prompt
    reqs = [Request(i, None, [5] * (1 + i % 2), 30, eos_id=None) for i in range(6)]
    sched, fake, done = run_schedule(reqs, max_live=4, max_context=max_context)
    for r in done:
        pos = PREFIX + len(r.prompt)
        want = lockstep_ids(r.rid, pos, 30, None, max_context)
        assert r.ids == want and len(want) == max_context - pos, r.rid
        assert r.pos <= max_context - 1  # no cache row at or beyond the context


def test_freed_slots_are_reused_fifo():
    # 3 slots; requests 0, 1, 2 finish in the order 1, 2, 0 (lengths 9, 2, 5); threshold 1: each freed slot is refilled
    mt = [9, 2, 5, 20, 20, 20]
    reqs = [Request(i, None, [5], mt[i], eos_id=None) for i in range(6)]
    sched, fake, done = run_schedule(reqs, max_live=3, chunk=1, admit_threshold=1)
    slots = dict(fake.slot_log)
    assert [slots[i] for i in range(3)] == [0, 1, 2]
    assert [slots[i] for i in (3, 4, 5)] == [1, 2, 0]  # the order the slots were freed in
    for r in done:
        assert r.ids == lockstep_ids(r.rid, PREFIX + 1, mt[r.rid], None, 2048)


def test_padding_rows_use_slot_minus_one_and_rows_past_their_limit_idle():
    reqs = [Request(i, None, [5], mt, eos_id=None) for i, mt in enumerate([2, 6, 11])]
    sched = SlotScheduler(8, 2048, chunk=8)
    for r in reqs:
        sched.submit(r)
    adm = sched.take_admissions()
    for r in adm:
        sched.start(r, stream(r.rid, 0), PREFIX + 1)
    plan = sched.plan()
    assert plan.bucket == 4 and plan.n == 8
    assert (plan.slots[:, 3] == IDLE_SLOT).all()  # padding row
    assert list(plan.slots[:, 0] >= 0) == [True] + [False] * 7  # 1 step left for max_tokens 2
    assert list(plan.slots[:, 1] >= 0) == [True] * 5 + [False] * 3
    assert (plan.slots[:, 2] >= 0).all()
    assert plan.live_row_steps == 1 + 5 + 8


class FakeModel:
    def __init__(self):
        self.config = get_config("tiny")


class FakeEngine(ContinuousEngine):
    """The engine's bookkeeping (submit, generate, run) over the fake stream instead of the library."""

    def _prepare_run(self):
        self._fake = Fake(self.sched)

    def _admit(self, reqs):
        return self._fake.admit(reqs)

    def _step(self, plan):
        return self._fake.step(plan)


def test_generate_returns_input_order():
    eng = FakeEngine(FakeModel(), max_live=3, chunk=4)
    img = Image.new("RGB", (32, 32))
    mt = [12, 2, 7, 1, 0, 9, 3]
    got = eng.generate([img] * len(mt), [[5, 6]] * len(mt), max_tokens=mt, ignore_eos=True)
    assert got == [lockstep_ids(i, PREFIX + 2, mt[i], None, eng.model.config.text.max_context) for i in range(len(mt))]
    # completion order differs from input order
    eng2 = FakeEngine(FakeModel(), max_live=3, chunk=4)
    for i, x in enumerate(mt):
        eng2.submit(img, [5, 6], max_tokens=x, ignore_eos=True)
    order = [rid for rid, _ in eng2.run()]
    assert sorted(order) == list(range(len(mt))) and order != list(range(len(mt)))


def test_submit_validates():
    eng = FakeEngine(FakeModel(), max_live=2)
    img = Image.new("RGB", (32, 32))
    with pytest.raises(ValueError):
        eng.submit(img, [5], variant="some-variant")
    with pytest.raises(ValueError):
        eng.submit(img, [])
    with pytest.raises(ValueError):
        eng.submit("not an image", [5])
    with pytest.raises(ValueError):
        eng.submit(img, [5] * 2048)


def test_slot_entry_points_validate_on_the_host():
    """Both new entry points reject null models / buffers with MD_ERR_INVALID_ARG before any launch."""
    _lib.build_library(verbose=False)
    lib = _lib.load()
    kv = _lib.MdKvCache()
    text = _lib.MdTextModel()
    assert lib.md_text_forward_slots(None, None, None, 1, 1, None, None, 1, None, None, 0, None) == 1
    assert lib.md_text_forward_slots(ctypes.byref(text), None, None, 1, 1, None, None, 1, ctypes.byref(kv), None, 0, None) == 1
    assert lib.md_decode_step_slots(None, None, None, None, 1, None, 1, None, -1, None, 0, None, 0, None) == 1
    assert lib.md_decode_step_slots(ctypes.byref(text), None, None, None, 1, None, 1, ctypes.byref(kv), -1, None, 0, None, 0, None) == 1
