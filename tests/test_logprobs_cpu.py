"""Token log-probabilities without a GPU: the scorer's argument checks (raised before any device work), the bookkeeping of
query_choices over a stand-in scorer, and the scheduler keeping logprobs / ranks aligned with the ids it truncates."""
import types

import numpy as np
import pytest
from PIL import Image

from moondream_amd.config import get_config
from moondream_amd.continuous import ContinuousEngine, Request, SlotScheduler
from moondream_amd.moondream import EncodedImage, IdTokenizer, MoondreamModel

IMG = Image.new("RGB", (32, 32))
PREFIX = 730


def host_model(fp8=None, f8=None, kv8=None):
    """A MoondreamModel with its host-side state only: any device work raises AttributeError."""
    m = object.__new__(MoondreamModel)
    m.config = get_config("tiny")
    m.tokenizer = IdTokenizer()
    m._kv8_scales = kv8
    m.w = types.SimpleNamespace(text=types.SimpleNamespace(fp8=fp8, f8=f8))
    return m


def test_score_ids_rejects_bad_arguments_before_any_device_work():
    m = host_model()
    ctx = m.config.text.max_context
    bad = [
        ([IMG], [[1, 2]], [[]]),                       # an empty continuation
        ([IMG], [[]], [[5]]),                          # an empty prompt
        ([IMG, IMG], [[1]], [[5], [6]]),               # lists of different lengths
        ([IMG, IMG], [[1], [1]], [[5]]),
        ([], [], []),
        ([IMG], [[1] * 10], [[5] * (ctx - PREFIX - 10 + 1)]),                         # one position too many
        ([EncodedImage(ctx - 4, [])], [[1, 2]], [[5, 6, 7]]),                        # ... behind an EncodedImage's prefix
        (["image.png"], [[1]], [[5]]),
    ]
    for images, prompts, conts in bad:
        with pytest.raises(ValueError):
            m.score_ids(images, prompts, conts)
        with pytest.raises(ValueError):
            m.score_ids(images, prompts, conts, share_prefix=True)
    # the longest that fits passes the checks (and then reaches for the device this stand-in does not have)
    m._check_score_args([IMG], [[1] * 10], [[5] * (ctx - PREFIX - 10)])
    m._check_score_args([EncodedImage(ctx - 4, [])], [[1, 2]], [[5, 6]])
    for kw in ({"fp8": object()}, {"f8": object()}, {"kv8": object()}):
        with pytest.raises(ValueError, match="fp8"):
            host_model(**kw).score_ids([IMG], [[1]], [[5]])


def test_query_choices_bookkeeping():
    m = host_model()
    enc = EncodedImage(PREFIX, [])
    seen = {}

    def fake_score(images, prompts, continuations, share_prefix=False, variant=None):
        seen.update(images=images, prompts=prompts, conts=continuations, share_prefix=share_prefix, variant=variant)
        table = {2: [-1.0, -1.0], 4: [-0.5, -0.25, -1.5, -0.75], 3: [-0.125, -3.0, -0.5]}
        lp = [table[len(c)] for c in continuations]
        return lp, [[0] * len(c) for c in continuations]

    m.score_ids = fake_score
    m.encode_image = lambda image, settings=None: enc
    out = m.query_choices(IMG, "7 8 9", ["11", "21 22 23", "31 32"], settings={"variant": "v1"})
    eos = m.config.tokenizer.eos_id
    assert seen["conts"] == [[11, eos], [21, 22, 23, eos], [31, 32, eos]]
    assert seen["prompts"] == [m._query_prompts(["7 8 9"])[0]] * 3 and seen["prompts"][0][3:6] == [7, 8, 9]
    assert all(im is enc for im in seen["images"]) and seen["share_prefix"] is True and seen["variant"] == "v1"
    assert out["logprobs"] == [-2.0, -3.0, -3.625]
    assert out["mean_logprobs"] == [-1.0, -0.75, -3.625 / 3]
    assert out["per_token"] == [[-1.0, -1.0], [-0.5, -0.25, -1.5, -0.75], [-0.125, -3.0, -0.5]]
    assert out["best"] == 0 and out["best_normalized"] == 1  # the two argmaxes part
    assert m.query_choices(IMG, "7", ["11", "12"])["best"] == 0 and seen["variant"] is None  # a tie: the first choice
    with pytest.raises(ValueError):
        m.query_choices(IMG, "7", [])


def lp_of(rid, k):
    return -(rid + 1) - k / 64.0


def test_commit_keeps_logprobs_and_ranks_aligned_with_the_ids():
    """Requests that stop at EOS, at max_tokens and at the context end, in chunks of 4 with idle rows: every kept id has its
    own logprob and rank, nothing of an idle / padding row or of the EOS token is kept."""
    tok = lambda rid, k: 100 + rid * 50 + k
    sched = SlotScheduler(4, 2048, chunk=4)
    spec = [(0, 9, None), (1, 2, None), (2, 20, tok(2, 6)), (3, 1, None), (4, 7, None), (5, 30, None)]
    for rid, mt, eos in spec:
        sched.submit(Request(rid, None, [5], mt, eos))
    pos0 = {5: 2048 - 1 - 4}  # request 5 has room for 4 decode steps only

    def admit(reqs):
        return [(tok(r.rid, 0), pos0.get(r.rid, PREFIX + 1), lp_of(r.rid, 0), r.rid) for r in reqs]

    def step(plan):
        out = np.full((plan.n, plan.bucket), -1, dtype=np.int32)
        lp = np.full((plan.n, plan.bucket), np.nan, dtype=np.float32)  # idle and padding rows: what the kernel leaves there
        rk = np.full((plan.n, plan.bucket), -1, dtype=np.int32)
        for j, r in enumerate(plan.rows):
            for i in range(min(plan.n, r.remaining)):
                k = r.steps + i + 1
                out[i, j], lp[i, j], rk[i, j] = tok(r.rid, k), lp_of(r.rid, k), r.rid * 1000 + k
        return out, lp, rk

    done = {r.rid: r for r in sched.run(admit, step)}
    want_len = {0: 9, 1: 2, 2: 6, 3: 1, 4: 7, 5: 5}
    for rid, n in want_len.items():
        r = done[rid]
        assert r.ids == [tok(rid, k) for k in range(n)]
        assert len(r.logprobs) == len(r.ranks) == n
        assert r.logprobs == [float(np.float32(lp_of(rid, k))) for k in range(n)]
        assert r.ranks == [rid] + [rid * 1000 + k for k in range(1, n)]
        assert not any(np.isnan(x) for x in r.logprobs)


def test_a_request_that_ends_at_its_first_token_keeps_nothing_extra():
    sched = SlotScheduler(2, 2048, chunk=4)
    a, b = Request(0, None, [5], 8, 42), Request(1, None, [5], 0, None)
    a.slot = b.slot = 0
    assert sched.start(a, 42, PREFIX + 1, -0.5, 0) and a.ids == a.logprobs == a.ranks == []   # EOS first
    assert sched.start(b, 7, PREFIX + 1, -0.5, 0) and b.ids == b.logprobs == b.ranks == []    # max_tokens 0
    c = Request(2, None, [5], 1, None)
    c.slot = 1
    assert sched.start(c, 7, PREFIX + 1, -0.5, 3) and (c.ids, c.logprobs, c.ranks) == ([7], [-0.5], [3])
    d = Request(3, None, [5], 4, None)  # without the values: the lists stay empty, as before
    d.slot = 1
    assert not sched.start(d, 7, PREFIX + 1) and d.ids == [7] and d.logprobs == d.ranks == []


class FakeEngine(ContinuousEngine):
    def _prepare_run(self):
        pass

    def _admit(self, reqs):
        extra = lambda r: (lp_of(r.rid, 0), 0) if self.logprobs else ()
        return [(10 + r.rid, PREFIX + len(r.prompt)) + extra(r) for r in reqs]

    def _step(self, plan):
        out = np.zeros((plan.n, plan.bucket), dtype=np.int32)
        for j, r in enumerate(plan.rows):
            for i in range(plan.n):
                out[i, j] = 10 + r.rid + r.steps + i + 1
        if not self.logprobs:
            return out
        return out, (-out / 8.0).astype(np.float32), out % 3


class FakeModel:
    def __init__(self):
        self.config = get_config("tiny")


def test_engine_yields_pairs_unless_asked():
    off = FakeEngine(FakeModel(), max_live=2, chunk=4)
    ids = off.generate([IMG] * 3, [[5]] * 3, max_tokens=[3, 5, 2], ignore_eos=True)
    assert ids == [[10 + i + k for k in range(n)] for i, n in enumerate([3, 5, 2])]
    for call in (lambda: off.generate([IMG], [[5]], max_tokens=2, return_logprobs=True), lambda: list(off.run(with_logprobs=True))):
        with pytest.raises(ValueError):
            call()
    on = FakeEngine(FakeModel(), max_live=2, chunk=4, logprobs=True)
    got = on.generate([IMG] * 3, [[5]] * 3, max_tokens=[3, 5, 2], ignore_eos=True, return_logprobs=True)
    assert got[0] == ids
    for i in range(3):
        assert got[1][i] == [lp_of(i, 0)] + [-t / 8.0 for t in ids[i][1:]]
        assert got[2][i] == [0] + [t % 3 for t in ids[i][1:]]
    on.submit(IMG, [5], max_tokens=2, ignore_eos=True)
    assert [len(item) for item in on.run()] == [2]
    on.submit(IMG, [5], max_tokens=2, ignore_eos=True)
    assert [len(item) for item in on.run(with_logprobs=True)] == [4]
