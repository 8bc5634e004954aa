"""Per-request sampling settings without a GPU: validation at submit, per-request sequences in generate, and the
scheduler's plans with the new Request fields (the engine's bookkeeping runs on a stand-in model and a fake token stream)."""
import numpy as np
import pytest
from PIL import Image

from moondream_amd.config import get_config
from moondream_amd.continuous import DEFAULT_TOP_P, ContinuousEngine, Request, SlotScheduler
from moondream_amd.settings import RowSettings

PREFIX = 730


def stream(rid, k):
    return 1 + (rid * 7 + k * 3) % 50


class FakeModel:
    def __init__(self):
        self.config = get_config("tiny")


class FakeEngine(ContinuousEngine):
    """submit / generate / run over a fake token stream instead of the library; records what reached the GPU side."""

    def _prepare_run(self):
        self.admitted = []

    def _admit(self, reqs):
        self.admitted += reqs
        return [(stream(r.rid, 0), PREFIX + len(r.prompt)) for r in reqs]

    def _step(self, plan):
        out = np.zeros((plan.n, plan.bucket), dtype=np.int32)
        for j, r in enumerate(plan.rows):
            for i in range(plan.n):
                out[i, j] = stream(r.rid, r.steps + i + 1)
        return out


IMG = Image.new("RGB", (32, 32))


@pytest.mark.parametrize("kw", [{"temperature": -0.1}, {"temperature": float("nan")}, {"top_p": 0}, {"top_p": 1.5},
                                {"top_p": float("inf")}], ids=lambda kw: "%s=%s" % next(iter(kw.items())))
def test_submit_rejects_bad_settings(kw):
    eng = FakeEngine(FakeModel(), max_live=2)
    with pytest.raises(ValueError):
        eng.submit(IMG, [5], **kw)
    assert not eng.sched.queue and not eng.sched.pending()
    with pytest.raises(ValueError):
        eng.submit_caption(IMG, **kw)
    assert not eng.sched.queue
    assert list(eng.run()) == []


def test_submit_defaults_to_the_engines_settings_and_accepts_the_edges():
    eng = FakeEngine(FakeModel(), max_live=4, temperature=0.7, top_p=0.9)
    eng.submit(IMG, [5])
    eng.submit(IMG, [5], temperature=0)              # greedy beside the engine's sampled default
    eng.submit(IMG, [5], temperature=2.5, top_p=1)   # top_p = 1 is inside (0, 1]
    eng.submit_caption(IMG, top_p=0.25)
    got = [(r.settings.temperature, r.settings.top_p) for r in eng.sched.queue]
    assert got == [(0.7, 0.9), (0.0, 0.9), (2.5, 1.0), (0.7, 0.25)]
    assert all(isinstance(x, float) for pair in got for x in pair)
    plain = FakeEngine(FakeModel(), max_live=2)
    plain.submit(IMG, [5])
    assert (plain.sched.queue[0].settings.temperature, plain.sched.queue[0].settings.top_p) == (0.0, DEFAULT_TOP_P)


def test_generate_takes_one_setting_or_one_per_request():
    eng = FakeEngine(FakeModel(), max_live=3, chunk=4)
    n = 5
    for bad in ({"temperature": [0.5] * (n - 1)}, {"top_p": [0.5] * (n + 1)}, {"temperature": [0.5] * n, "top_p": []}):
        with pytest.raises(ValueError):
            eng.generate([IMG] * n, [[5, 6]] * n, max_tokens=4, ignore_eos=True, **bad)
        assert not eng.sched.pending()  # nothing was queued
    temps = [0.0, 0.5, 4.0, 1.0, 0.0]
    ids = eng.generate([IMG] * n, [[5, 6]] * n, max_tokens=4, ignore_eos=True, temperature=temps, top_p=0.8)
    assert sorted((r.rid, r.settings.temperature, r.settings.top_p) for r in eng.admitted) == [(i, temps[i], 0.8) for i in range(n)]
    assert ids == [[stream(i, k) for k in range(4)] for i in range(n)]
    eng.generate([IMG] * 2, [[5]] * 2, max_tokens=2, ignore_eos=True, temperature=np.float32(0.5))
    assert [(r.settings.temperature, r.settings.top_p) for r in eng.admitted] == [(0.5, DEFAULT_TOP_P)] * 2
    # a bad value inside a sequence is the submit's ValueError
    with pytest.raises(ValueError):
        eng.generate([IMG] * 2, [[5]] * 2, max_tokens=2, temperature=[0.5, -1.0])


def test_plans_do_not_depend_on_the_settings():
    def plans(settings):
        sched = SlotScheduler(4, 2048, chunk=4)
        mt = [9, 2, 5, 12, 7, 3]
        for i, m in enumerate(mt):
            sched.submit(Request(i, None, [5] * (1 + i % 2), m, None, **settings(i)))
        log = []

        def admit(reqs):
            log.append([(r.rid, r.slot) for r in reqs])
            return [(stream(r.rid, 0), PREFIX + len(r.prompt)) for r in reqs]

        def step(plan):
            log.append((plan.bucket, plan.n, plan.slots.tolist(), plan.tokens.tolist(), plan.pos.tolist()))
            out = np.zeros((plan.n, plan.bucket), dtype=np.int32)
            for j, r in enumerate(plan.rows):
                for i in range(plan.n):
                    out[i, j] = stream(r.rid, r.steps + i + 1)
            return out

        done = [(r.rid, r.ids) for r in sched.run(admit, step)]
        return log, done

    base = plans(lambda i: {})
    mixed = plans(lambda i: {"settings": RowSettings(temperature=[0.0, 0.5, 4.0][i % 3], top_p=[0.3, 1.0][i % 2])})
    assert base == mixed and len(base[0]) > 4
