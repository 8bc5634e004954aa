"""Repetition / presence / frequency penalties end to end on the tiny model (B = 4, 12 tokens, greedy, ignore_eos).
The checks use BOOSTS, whose effect follows from the rule alone: a presence penalty of -1e4 is a bonus of +1e4 for every
token a row has generated, which dwarfs every logit (|logit| < 100 here), so the row repeats its first token for ever; a
frequency penalty of 4e3 on top leaves +6000 at count 1, +2000 at count 2 and -2000 at count 3, so the row emits runs of
exactly three equal tokens whose run tokens are pairwise distinct."""
import os

import numpy as np
import pytest
import torch

from moondream_amd import synth
from moondream_amd.config import get_config
from moondream_amd.continuous import ContinuousEngine
from PIL import Image

pytestmark = pytest.mark.gpu
N = 12
SAME = dict(presence_penalty=-1e4)
RUNS = dict(presence_penalty=-1e4, frequency_penalty=4e3)


class Tiny:
    pass


def golden_image(g, idx, kind="cap"):
    src = int(g["image_index"][idx])
    arr = synth.synthetic_image_array(src, int(g["seed"]), tuple(g[f"img{idx}.{kind}.size"]))
    return Image.fromarray(arr, "RGB")


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    assert torch.cuda.is_available(), "GPU tests need a device"
    t = Tiny()
    g = np.load(os.path.join(golden_dir, "tiny_seed1.npz"))
    t.cfg = get_config("tiny")
    sd = synth.synthetic_state_dict(t.cfg, seed=int(g["seed"]), device="cuda")
    t.model = MoondreamModel(t.cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=8)
    imgs = [golden_image(g, i) for i in range(3)]
    t.images = imgs + imgs[:1]
    t.prompts = [g[f"img{i}.cap.prompt"].tolist() for i in range(3)] + [[1, 708, 9, 3]]  # two lengths: two prefill groups
    t.kw = dict(max_tokens=N, ignore_eos=True)
    t.plain = t.model.batch_generate_ids(t.images, t.prompts, **t.kw)
    assert t.plain[0] == g["img0.cap.tokens"].tolist()[:N] and all(len(s) == N for s in t.plain)
    t.same = t.model.batch_generate_ids(t.images, t.prompts, **t.kw, **SAME)
    t.runs = t.model.batch_generate_ids(t.images, t.prompts, **t.kw, **RUNS)
    return t


def launches(model):
    """Count md_penalize_rows launches of ``model`` from here on: returns the list the counts go to."""
    seen = []
    inner = model._penalize
    model._penalize = lambda *a, **k: (seen.append(1), inner(*a, **k))[1]
    return seen


def test_all_same(tiny):
    for row, plain in zip(tiny.same, tiny.plain):
        assert row == [plain[0]] * N


def test_runs_of_three(tiny):
    """The first run's token is the plain call's first token (both picked from the prompt pass's logits with an empty
    history).  From the second run on the context differs from the plain call's (the run token three times instead of
    once), so the plain call's ids say nothing there; what the rule gives is checked instead: whole runs of exactly three,
    run tokens pairwise distinct.  The second run's token is checked against the model itself: it is the best live token
    other than the first run's after [t0, t0, t0], which ``score_ids`` reads from the plain (unpenalised) model."""
    m = tiny.model
    for row, plain in zip(tiny.runs, tiny.plain):
        runs = [row[i : i + 3] for i in range(0, N, 3)]
        assert all(len(set(r)) == 1 for r in runs), row
        heads = [r[0] for r in runs]
        assert len(set(heads)) == len(heads), row
        assert heads[0] == plain[0]
    conts = [row[:4] for row in tiny.runs]  # [t0, t0, t0, t1]
    _, _, alts = m.score_ids(tiny.images, tiny.prompts, conts, top_logprobs=2)
    for row, alt in zip(tiny.runs, alts):
        best = [t for t, _ in alt[3] if t != row[0]][0]  # the decision after [t0, t0, t0], without t0 (its bonus is -2000)
        assert row[3] == best, (row, alt[3])


def test_mixed_batch_rows_depend_on_their_own_settings_only(tiny):
    m = tiny.model
    mixed = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, presence_penalty=[-1e4, 0.0, -1e4, 0.0],
                                 frequency_penalty=[4e3, 0.0, 4e3, 0.0])
    assert mixed[1] == tiny.plain[1] and mixed[3] == tiny.plain[3]
    assert mixed[0] == tiny.runs[0] and mixed[2] == tiny.runs[2]


def test_neutral_settings_are_the_plain_call(tiny):
    m = tiny.model
    seen = launches(m)
    m.compile()
    try:
        assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw) == tiny.plain
        keys = set(m._graphs)
        got = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, repetition_penalty=1.0, presence_penalty=[0.0] * 4,
                                   frequency_penalty=0)
        assert got == tiny.plain and set(m._graphs) == keys and not seen
        assert not any("penalty" in k for k in keys if isinstance(k, tuple))
    finally:
        del m._penalize
        m.use_graphs = False
        m._graphs.clear()


def test_compiled_equals_eager(tiny):
    m = tiny.model
    m.compile()
    try:
        for _ in range(2):  # the capturing call, then a replay
            assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **RUNS) == tiny.runs
            assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **SAME) == tiny.same
        assert any(isinstance(k, tuple) and "penalty" in k for k in m._graphs)
        assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw) == tiny.plain
    finally:
        m.use_graphs = False
        m._graphs.clear()


def test_logprobs_are_those_of_the_penalised_logits(tiny):
    m = tiny.model
    for kw, want in ((SAME, tiny.same), (RUNS, tiny.runs)):
        ids, lp, rk = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **kw, return_logprobs=True)
        assert ids == want and all(r == 0 for row in rk for r in row)
        # a boosted token holds all of the mass: its log-probability is 0 (exp(-2000) vanishes in fp32)
        assert all(x == 0.0 for row in lp for x in row[1:3])


def test_shared_prefix_equals_the_copy_path(tiny):
    m = tiny.model
    enc = m.encode_image(tiny.images[0])
    prompts = [tiny.prompts[0], [1, 708, 9, 3], [1, 17, 708, 2, 382, 9, 3], tiny.prompts[0]]
    kw = dict(**tiny.kw, presence_penalty=[-1e4, 0.0, -1e4, -1e4], frequency_penalty=[4e3, 0.0, 0.0, 4e3])
    a = m.batch_generate_ids([enc] * 4, prompts, share_prefix=True, **kw)
    b = m.batch_generate_ids([enc] * 4, prompts, **kw)
    assert a == b
    assert a[2] == [a[2][0]] * N and a[0] == a[3] and len(set(a[0][::3])) == 4 and a[0][:3] == [a[0][0]] * 3


def test_continuous_engine_equals_lockstep_with_reused_slots(tiny):
    """Two slots, five requests of mixed settings: each equals the lockstep call's row for the same settings; a penalised
    request in a reused slot starts from an empty history (or its first run would be cut short)."""
    m = tiny.model
    idx = [0, 1, 2, 3, 0]
    pres = [-1e4, 0.0, -1e4, -1e4, 0.0]
    freq = [4e3, 0.0, 0.0, 4e3, 0.0]
    want = [tiny.runs[0], tiny.plain[1], tiny.same[2], tiny.runs[3], tiny.plain[0]]
    mt = [N, 5, 9, N, 7]
    for compiled in (False, True):
        if compiled:
            m.compile()
        try:
            eng = ContinuousEngine(m, max_live=2, chunk=4)
            got = eng.generate([tiny.images[i] for i in idx], [tiny.prompts[i] for i in idx], max_tokens=mt, ignore_eos=True,
                               presence_penalty=pres, frequency_penalty=freq)
            assert got == [w[:n] for w, n in zip(want, mt)]
            assert eng.stats.admissions > 1
        finally:
            m.use_graphs = False
            m._graphs.clear()
    got = m.batch_generate_ids_continuous([tiny.images[i] for i in idx], [tiny.prompts[i] for i in idx], max_tokens=mt, ignore_eos=True,
                                          max_live=2, chunk=4, presence_penalty=pres, frequency_penalty=freq)
    assert got == [w[:n] for w, n in zip(want, mt)]


def test_caption_and_query_take_the_settings(tiny):
    m = tiny.model
    torch.manual_seed(3)  # the sampled first tokens (the default generators)
    torch.cuda.manual_seed(3)
    for temperature in (0, 0.5):  # the chunked greedy loop and the per-token sampled one
        st = {"presence_penalty": -1e4, "max_tokens": 7, "temperature": temperature}
        cap = m.caption(tiny.images[0], settings=st)["caption"].split()
        assert len(cap) == 7 and len(set(cap)) == 1, cap
        ans = m.query(tiny.images[1], "5 6 7", settings=st)["answer"].split()
        assert len(ans) == 7 and len(set(ans)) == 1, ans
    out = m.batch_caption(tiny.images[:2], settings={"temperature": 0, "max_tokens": 6, **SAME})
    assert all(len(set(c.split())) == 1 and len(c.split()) == 6 for c in out)
    many = m.query_many(tiny.images[0], ["5 6", "7 8 9"], settings={"temperature": 0, "max_tokens": 6, **SAME})
    assert all(len(set(a["answer"].split())) == 1 for a in many)
