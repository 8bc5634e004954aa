"""Constrained decoding end to end on the tiny model (B <= 5, 12 tokens): what a row generates is what its automaton
allows -- checked by the automaton's own ``walk`` on the host -- under the argmax and under sampling, in lockstep, in the
continuous engine, alone, captured, over a shared prefix, under a LoRA variant and in the fp8 KV mode."""
import math
import os

import numpy as np
import pytest
import torch

from moondream_amd import synth
from moondream_amd.config import get_config
from moondream_amd.constraint import DEAD, FORBID, TokenAutomaton
from moondream_amd.continuous import ContinuousEngine
from PIL import Image

pytestmark = pytest.mark.gpu
N = 12
EOS = 0
X0 = [700, 5, 1023, 42, 42, 9, 512, 1]  # arbitrary ids: nothing the model would pick
X1 = [1, 2, 4]
CHOICES = [[10, 11, 12], [10, 11], [20], [30, 31, 32, 33]]  # one a prefix of another; at most 3 tokens allowed per state


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
    assert t.cfg.tokenizer.eos_id == EOS and t.cfg.tokenizer.answer_id == 3
    sd = synth.synthetic_state_dict(t.cfg, seed=int(g["seed"]), device="cuda")
    t.model = MoondreamModel(t.cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=8)
    imgs = [golden_image(g, i) for i in range(3)]
    t.images = imgs + imgs[:1]
    t.prompts = [g[f"img{i}.cap.prompt"].tolist() for i in range(3)] + [[1, 708, 9, 3]]  # two lengths: two prefill groups
    t.kw = dict(max_tokens=N, ignore_eos=True)
    t.plain = t.model.batch_generate_ids(t.images, t.prompts, **t.kw)
    assert all(len(s) == N for s in t.plain)
    t.seq0, t.seq1 = TokenAutomaton.sequence(X0), TokenAutomaton.sequence(X1)
    t.choices = TokenAutomaton.choices(CHOICES, EOS)
    t.digits = TokenAutomaton.allowed_tokens(range(100, 110))
    t.banned = TokenAutomaton.banned_tokens(sorted(set(t.plain[1])))
    # one call with a row of every kind (row 2 free); the same automaton object may serve two rows
    t.mixed = [t.seq0, t.banned, None, t.choices]
    t.mixed_ids = t.model.batch_generate_ids(t.images, t.prompts, **t.kw, constraints=t.mixed)
    return t


def check_rows(ids, automata):
    """Every row's ids pass its automaton without DEAD."""
    for row, a in zip(ids, automata):
        assert a is None or a.walk(row) != DEAD, (row, a.edges[:2])


def is_choice_then_eos(row):
    return any(row[: len(c) + 1] == c + [EOS] for c in CHOICES)


def test_sequence_rows_emit_exactly_the_sequence(tiny):
    """Fails without the feature: X0 and X1 are nothing the model picks by itself."""
    m = tiny.model
    cons = [tiny.seq0, tiny.seq1, None, tiny.seq0]
    got = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=cons)
    assert got[0][: len(X0)] == X0 and got[3][: len(X0)] == X0 and got[1][: len(X1)] == X1
    assert got[2] == tiny.plain[2] and tiny.plain[0][: len(X0)] != X0
    for seed in (1, 2):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        got = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=cons, temperature=1.0, top_p=1.0, generator=gen)
        assert got[0][: len(X0)] == X0 and got[3][: len(X0)] == X0 and got[1][: len(X1)] == X1
    one = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=tiny.seq1)  # one automaton: every row's
    assert one == m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=[tiny.seq1] * 4)
    assert all(row[: len(X1)] == X1 for row in one)


def test_mixed_call(tiny):
    """The free row's greedy ids are those of the call without constraints; the others obey their automata."""
    assert tiny.mixed_ids[2] == tiny.plain[2]
    assert tiny.mixed_ids[0][: len(X0)] == X0
    assert not set(tiny.mixed_ids[1]) & set(tiny.plain[1])
    assert is_choice_then_eos(tiny.mixed_ids[3])
    check_rows(tiny.mixed_ids, tiny.mixed)


def test_choices_rows_emit_a_choice_then_eos(tiny):
    m = tiny.model
    got = m.batch_generate_ids(tiny.images, tiny.prompts, max_tokens=N, constraints=tiny.choices)  # eos ends a row
    assert all(row in CHOICES for row in got), got
    for seed in (3, 4, 5):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        got = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=tiny.choices, temperature=1.0, top_p=1.0,
                                   generator=gen)
        assert all(is_choice_then_eos(row) for row in got), got
        check_rows(got, [tiny.choices] * 4)


def test_sampled_rows_never_leave_their_automata(tiny):
    m = tiny.model
    cons = [tiny.digits, tiny.banned, tiny.choices, TokenAutomaton.min_tokens(5, tiny.plain[3][1])]
    for seed in (6, 7, 8):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        got = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=cons, temperature=1.0, top_p=1.0, generator=gen)
        check_rows(got, cons)
        assert set(got[0]) <= set(range(100, 110)) and not set(got[1]) & set(tiny.plain[1])
    got = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=cons)
    check_rows(got, cons)
    assert set(got[0]) <= set(range(100, 110))


def test_min_tokens_keeps_eos_out_of_the_first_n(tiny):
    """With the row's own second token as eos the plain call stops after one token; under min_tokens(6, eos) that id
    is not among the first 6, and the row's first token (picked before it) is the plain one."""
    m = tiny.model
    eos = tiny.plain[0][1]
    assert m.batch_generate_ids(tiny.images[:1], tiny.prompts[:1], max_tokens=N, eos_id=eos)[0] == tiny.plain[0][:1]
    a = TokenAutomaton.min_tokens(6, eos)
    got = m.batch_generate_ids(tiny.images[:2], tiny.prompts[:2], **tiny.kw, eos_id=eos, constraints=[a, None])
    assert eos not in got[0][:6] and got[0][0] == tiny.plain[0][0] and got[1] == tiny.plain[1]
    stopped = m.batch_generate_ids(tiny.images[:2], tiny.prompts[:2], max_tokens=N, eos_id=eos, constraints=[a, None])
    assert len(stopped[0]) >= 6 and stopped[0] == got[0][: len(stopped[0])]


def test_continuous_engine_and_lone_sequence_equal_lockstep(tiny):
    """Two slots, five requests: every slot is refilled, by a constrained request after a free one and the other way
    round; each request equals the lockstep call's row.  A lone sequence gives the same ids on the batched kernels."""
    m = tiny.model
    idx = [0, 1, 2, 3, 0]
    cons = [tiny.mixed[i] for i in idx[:4]] + [tiny.digits]
    digits = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=[tiny.digits, None, None, None])[0]
    want = [tiny.mixed_ids[i] for i in idx[:4]] + [digits]
    mt = [N, 5, 9, N, 7]
    images, prompts = [tiny.images[i] for i in idx], [tiny.prompts[i] for i in idx]
    for compiled in (False, True):
        if compiled:
            m.compile()
        try:
            eng = ContinuousEngine(m, max_live=2, chunk=4)
            got = eng.generate(images, prompts, max_tokens=mt, ignore_eos=True, constraints=cons)
            assert got == [w[:n] for w, n in zip(want, mt)]
            assert eng.stats.admissions > 1
            assert eng.generate(images[:3], prompts[:3], max_tokens=N, ignore_eos=True) == tiny.plain[:3]  # stale states do not leak
        finally:
            m.use_graphs = False
            m._graphs.clear()
    got = m.batch_generate_ids_continuous(images, prompts, max_tokens=mt, ignore_eos=True, max_live=2, chunk=4, constraints=cons)
    assert got == [w[:n] for w, n in zip(want, mt)]
    m.set_strict_batch_invariance(True)
    try:
        batch = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=tiny.mixed)
        for i in (0, 1, 3):
            lone = m.batch_generate_ids(tiny.images[i : i + 1], tiny.prompts[i : i + 1], **tiny.kw, constraints=tiny.mixed[i])
            assert lone[0] == batch[i] and not m._b1_used
    finally:
        m.set_strict_batch_invariance(False)


def test_compiled_equals_eager_and_free_calls_keep_their_graphs(tiny):
    m = tiny.model
    seen = []
    inner = m._constrain
    m._constrain = lambda *a, **k: (seen.append(1), inner(*a, **k))[1]
    m.compile()
    try:
        assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw) == tiny.plain
        keys = set(m._graphs)
        assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=[None] * 4) == tiny.plain
        assert set(m._graphs) == keys and not seen and not any("constraint" in k for k in keys if isinstance(k, tuple))
        for _ in range(2):  # the capturing call, then a replay
            assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=tiny.mixed) == tiny.mixed_ids
        n_graphs = len(m._graphs)
        assert any(isinstance(k, tuple) and "constraint" in k for k in m._graphs)
        # another table of similar size: the same buffers (capacities are powers of two), so the same graphs
        other = [tiny.seq1, tiny.choices, None, tiny.seq0]
        got = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=other)
        assert len(m._graphs) == n_graphs, "20 states and 23 edges take the buffers of 18 and 21 .. 32: capacities (32, 32)"
        assert got[0][:3] == X1 and is_choice_then_eos(got[1]) and got[2] == tiny.plain[2] and got[3][: len(X0)] == X0
    finally:
        del m._constrain
        m.use_graphs = False
        m._graphs.clear()


def test_logprobs_are_those_of_the_masked_logits(tiny):
    m = tiny.model
    cons = [tiny.choices, tiny.seq1, None, tiny.choices]
    ids, lp, rk, alts = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, constraints=cons, return_logprobs=True,
                                             top_logprobs=4)
    assert all(r == 0 for row in rk for r in row), "a greedy token is the best of what its state allows"
    checked = 0
    for row, a, row_alts, row_lp in zip(ids, cons, alts, lp):
        if a is None:
            continue
        state = 0
        for j, (tok, alt) in enumerate(zip(row, row_alts)):
            if state < 0:
                break
            allowed = [t for t, n in a.edges[state] if n != FORBID]
            assert a.default[state] == FORBID and 1 <= len(allowed) <= 4
            finite = [(t, x) for t, x in alt if math.isfinite(x)]
            assert {t for t, _ in finite} == set(allowed), (j, alt, allowed)
            assert abs(sum(math.exp(x) for _, x in finite) - 1.0) <= 1e-5
            assert alt[0][0] == tok and alt[0][1] == row_lp[j]
            assert all(x == -math.inf for _, x in alt[len(allowed):])
            checked += 1
            state = a.walk([tok], state)
            assert state != DEAD
    assert checked >= 3 + 2 + 2


def test_shared_prefix_lora_variant_and_fp8_kv(tiny):
    m = tiny.model
    enc = m.encode_image(tiny.images[0])
    prompts = [tiny.prompts[0], [1, 708, 9, 3], [1, 17, 708, 2, 382, 9, 3], tiny.prompts[0]]
    cons = [tiny.seq0, tiny.digits, None, tiny.choices]

    def check(got):
        check_rows(got, cons)
        assert got[0][: len(X0)] == X0 and set(got[1]) <= set(range(100, 110)) and is_choice_then_eos(got[3])

    shared = m.batch_generate_ids([enc] * 4, prompts, share_prefix=True, **tiny.kw, constraints=cons)
    check(shared)
    assert shared == m.batch_generate_ids([enc] * 4, prompts, **tiny.kw, constraints=cons)
    m.register_variant("constraints-test", synth.synthetic_lora(tiny.cfg, seed=3, rank=8, device="cuda"))
    check(m.batch_generate_ids(tiny.images, prompts, variant="constraints-test", **tiny.kw, constraints=cons))
    m.enable_fp8(tiny.images[:3], tiny.prompts[0], kv_cache=True)
    try:
        assert m._kv8_scales is not None
        check(m.batch_generate_ids(tiny.images, prompts, **tiny.kw, constraints=cons))
    finally:
        m.enable_fp8(on=False)


def test_caption_and_query_take_the_setting(tiny):
    m = tiny.model
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    want = [str(t) for t in X0]
    for temperature in (0, 0.5):  # the chunked greedy loop and the per-token sampled one
        st = {"constraints": tiny.seq0, "max_tokens": len(X0), "temperature": temperature}
        assert m.caption(tiny.images[0], settings=st)["caption"].split() == want
        assert m.query(tiny.images[1], "5 6 7", settings=st)["answer"].split() == want
    st = {"temperature": 0, "max_tokens": len(X0), "constraints": [tiny.seq0, None]}
    out = m.batch_caption(tiny.images[:2], settings=st)
    assert out[0].split() == want and out[1].split() != want
    many = m.query_many(tiny.images[0], ["5 6", "7 8 9"], settings={**st, "constraints": tiny.seq0})
    assert all(a["answer"].split() == want for a in many)
    picked = m.query(tiny.images[0], "5 6", settings={"temperature": 0, "constraints": m.choice_constraint(["10 11", "20"])})
    assert picked["answer"].split() in (["10", "11"], ["20"])
