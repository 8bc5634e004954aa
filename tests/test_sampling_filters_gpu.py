"""Per-request top-k / min-p sampling end to end on the tiny model (B <= 5, 12 tokens): neutral arguments change nothing,
a row's ids depend on its own settings and seed only, the three generation routes agree, and ``top_k = 1`` is greedy
decoding.  The tiny checkpoint's decisions are wide (tests/test_sampling_filters_cpu.py checks the recorded margins), so
the sampled checks run at temperature 4 / top-p 0.999, where the draws really leave the argmax."""
import os

import numpy as np
import pytest
import torch

from moondream_amd import synth
from moondream_amd.config import get_config
from moondream_amd.constraint import DEAD, TokenAutomaton
from moondream_amd.continuous import ContinuousEngine
from PIL import Image

pytestmark = pytest.mark.gpu
N = 12
HOT = dict(temperature=4.0, top_p=0.999)
TOP_K = [0, 3, 1, 3]     # the mixed call: row 0 neutral, row 2 all but greedy
MIN_P = [0.0, 0.0, 0.0, 0.2]
NEAR_TIE = 2.0 ** -6     # in log-probability: below it two bf16 probabilities can tie where the logits do not


class Tiny:
    pass


def golden_image(g, idx, kind="cap"):
    src = int(g["image_index"][idx])
    arr = synth.synthetic_image_array(src, int(g["seed"]), tuple(g[f"img{idx}.{kind}.size"]))
    return Image.fromarray(arr, "RGB")


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


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
    t.greedy = t.model.batch_generate_ids(t.images, t.prompts, **t.kw)
    t.hot = t.model.batch_generate_ids(t.images, t.prompts, **t.kw, **HOT, generator=gen(11))
    assert t.greedy[0] == g["img0.cap.tokens"].tolist()[:N] and t.hot != t.greedy  # (at T = 4 the draws leave the argmax)
    t.mixed = t.model.batch_generate_ids(t.images, t.prompts, **t.kw, **HOT, generator=gen(11), top_k=TOP_K, min_p=MIN_P)
    return t


def test_neutral_arguments_are_the_call_without_them(tiny):
    """Fails without the feature (the arguments do not exist)."""
    m = tiny.model
    for compiled in (False, True):
        if compiled:
            m.compile()
        try:
            for off in (dict(top_k=0, min_p=0.0), dict(top_k=[0] * 4, min_p=[0.0] * 4)):
                assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **HOT, generator=gen(11), **off) == tiny.hot
                assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **off) == tiny.greedy
            # a greedy call accepts the settings and ignores them
            assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, top_k=2, min_p=0.5) == tiny.greedy
            # off by value, on the filtered launch: k >= the vocabulary cuts nothing, the draws are the same
            big = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **HOT, generator=gen(11), top_k=tiny.cfg.text.vocab_size)
            assert big == tiny.hot
            assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **HOT, generator=gen(11), top_k=TOP_K, min_p=MIN_P) == tiny.mixed
        finally:
            m.use_graphs = False
            m._graphs.clear()


def test_a_rows_ids_depend_on_its_own_settings_only(tiny):
    """Row i of the mixed call == row i of the call in which every row has row i's pair (same generator seed: same draws)."""
    m = tiny.model
    for pair in sorted(set(zip(TOP_K, MIN_P))):
        same = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **HOT, generator=gen(11), top_k=pair[0], min_p=pair[1])
        for i in range(4):
            if (TOP_K[i], MIN_P[i]) == pair:
                assert tiny.mixed[i] == same[i], (i, pair)
    assert tiny.mixed[0] == tiny.hot[0]        # the neutral row: the call without the arguments
    assert tiny.mixed[2] == tiny.greedy[2]     # k = 1: whatever the draw, the best token (see the margins)
    other = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **HOT, generator=gen(12), top_k=TOP_K, min_p=MIN_P)
    assert other[2] == tiny.mixed[2]           # ... under any seed


def test_the_three_routes_agree(tiny):
    """The lockstep call draws from one device generator and the engine from one host generator per request, so sampled
    ids are compared where they are a function of the settings alone (top_k = 1: one survivor, any uniform draws it) and,
    between the engine's routes, seed for seed; the yardstick of the per-request sampling tests: the request alone."""
    m = tiny.model
    one = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **HOT, generator=gen(3), top_k=1)
    assert one == tiny.greedy
    assert m.batch_generate_ids_continuous(tiny.images, tiny.prompts, **tiny.kw, **HOT, seeds=[1, 2, 3, 4], top_k=1, max_live=2,
                                           chunk=4) == one
    seeds, mt = [21, 22, 23, 24, 25], [N, 5, 9, N, 7]
    idx = [0, 1, 2, 3, 0]
    images, prompts = [tiny.images[i] for i in idx], [tiny.prompts[i] for i in idx]
    ks, ms = TOP_K + [5], MIN_P + [0.05]
    alone = []
    for i in range(5):
        eng = ContinuousEngine(m, max_live=8, chunk=4, **HOT)
        rid = eng.submit(images[i], prompts[i], max_tokens=mt[i], ignore_eos=True, seed=seeds[i], top_k=ks[i], min_p=ms[i])
        alone.append(dict(eng.run())[rid])
    assert [len(a) for a in alone] == mt and alone[2] == tiny.greedy[2][:9]
    for compiled in (False, True):
        if compiled:
            m.compile()
        try:
            got = m.batch_generate_ids_continuous(images, prompts, max_tokens=mt, ignore_eos=True, max_live=2, chunk=4, seeds=seeds,
                                                  top_k=ks, min_p=ms, **HOT)
            assert got == alone  # two slots, five requests: every slot refilled, rows filtered and not share chunks
            eng = ContinuousEngine(m, max_live=8, chunk=4)
            rids = [eng.submit(images[i], prompts[i], max_tokens=mt[i], ignore_eos=True, seed=seeds[i], top_k=ks[i], min_p=ms[i], **HOT)
                    for i in range(5)]
            res = dict(eng.run())
            assert [res[r] for r in rids] == alone
        finally:
            m.use_graphs = False
            m._graphs.clear()
    plain = ContinuousEngine(m, max_live=8, chunk=4, **HOT).generate(images, prompts, max_tokens=mt, ignore_eos=True, seeds=seeds)
    assert plain[0] == alone[0]  # the neutral request: the engine without the settings


def test_shared_prefix_equals_the_copy_path(tiny):
    m = tiny.model
    enc = m.encode_image(tiny.images[0])
    prompts = [tiny.prompts[0], tiny.prompts[3], tiny.prompts[1], tiny.prompts[0]]
    kw = dict(**tiny.kw, **HOT, top_k=[4, 0, 2, 1], min_p=[0.0, 0.1, 0.0, 0.0])
    copy = m.batch_generate_ids([enc] * 4, prompts, generator=gen(7), **kw)
    shared = m.batch_generate_ids([enc] * 4, prompts, generator=gen(7), share_prefix=True, **kw)
    assert shared == copy
    assert copy[3] == m.batch_generate_ids([enc] * 4, prompts, **tiny.kw)[3]  # its k = 1 row: greedy


def test_top_k_1_is_greedy_decoding(tiny):
    """top_k = 1 at the reference's default temperature reproduces every greedy sequence, up to but not including the first
    decision whose two best alternatives lie within 2^-6 in log-probability (there two bf16 probabilities can tie where
    the logits do not, and the lower id wins).  A condition, not a tolerance: more than a quarter of the sequences cut
    short fails.  On this fixture the oracle's recorded margins put no decision near a tie: the share is 0 of 3."""
    m = tiny.model
    images, prompts = tiny.images[:3], tiny.prompts[:3]
    ids, _, _, alts = m.batch_generate_ids(images, prompts, **tiny.kw, return_logprobs=True, top_logprobs=2)
    assert ids == tiny.greedy[:3]
    got = m.batch_generate_ids(images, prompts, **tiny.kw, temperature=0.5, top_p=0.3, generator=gen(5), top_k=1)
    cut = 0
    for i in range(3):
        gaps = [a[0][1] - a[1][1] for a in alts[i]]
        near = [j for j, gap in enumerate(gaps) if gap < NEAR_TIE]
        upto = near[0] if near else N
        cut += bool(near)
        print(f"row {i}: smallest gap {min(gaps):.4f}, compared up to decision {upto}")
        assert got[i][:upto] == ids[i][:upto], (i, upto)
    assert cut * 4 <= 3, f"{cut} of 3 sequences reach a near-tie: the fixture says nothing"


def test_penalties_and_a_choice_constraint_under_top_k(tiny):
    m = tiny.model
    choices = [[10, 11, 12], [10, 11], [20], [30, 31, 32, 33]]
    a = TokenAutomaton.choices(choices, tiny.cfg.tokenizer.eos_id)
    digits = TokenAutomaton.allowed_tokens(range(100, 110))
    for seed in (1, 2, 3):
        got = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, temperature=1.0, top_p=1.0, generator=gen(seed),
                                   constraints=[a, digits, a, digits], top_k=[2, 3, 0, 40], min_p=[0.0, 0.0, 0.05, 0.01],
                                   repetition_penalty=1.3, presence_penalty=[0.0, 0.5, 0.0, 0.5])
        for row, con in zip(got, [a, digits, a, digits]):
            assert con.walk(row) != DEAD, row
        assert set(got[1]) <= set(range(100, 110)) and set(got[3]) <= set(range(100, 110))
        eos = tiny.cfg.tokenizer.eos_id
        assert all(any(row[: len(c) + 1] == c + [eos] for c in choices) for row in (got[0], got[2])), got


def test_caption_and_query_take_the_settings(tiny):
    """The single-sequence calls: top_k = 1 at the default temperature gives the greedy text."""
    m = tiny.model
    st = {"max_tokens": 8, "temperature": 0}
    want = m.caption(tiny.images[0], settings=st)["caption"]
    assert m.caption(tiny.images[0], settings={"max_tokens": 8, "top_k": 1})["caption"] == want
    assert m.caption(tiny.images[0], settings={"max_tokens": 8, "min_p": 1.0})["caption"] == want
    assert m.batch_caption(tiny.images[:2], settings={"max_tokens": 8, "top_k": 1}) == m.batch_caption(tiny.images[:2], settings=st)


def test_lora_variant_and_fp8_kv_are_served(tiny):
    """top_k = 1 makes a sampled call a function of the logits alone: under a LoRA variant (the step made from its pieces,
    eager) and in the fp8 KV mode it must give that mode's greedy ids; min_p = 1 likewise (one best token per decision)."""
    m = tiny.model
    m.register_variant("filters-test", synth.synthetic_lora(tiny.cfg, seed=3, rank=8, device="cuda"))
    kw = dict(variant="filters-test", **tiny.kw)
    want = m.batch_generate_ids(tiny.images, tiny.prompts, **kw)
    assert m.batch_generate_ids(tiny.images, tiny.prompts, **kw, **HOT, generator=gen(2), top_k=1) == want
    assert m.batch_generate_ids(tiny.images, tiny.prompts, **kw, **HOT, generator=gen(2), top_k=[0, 1, 1, 1], min_p=[1.0, 0, 0, 0]) == want
    m.enable_fp8(tiny.images[:3], tiny.prompts[0], kv_cache=True)
    try:
        assert m._kv8_scales is not None
        want = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw)
        assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **HOT, generator=gen(2), top_k=1) == want
    finally:
        m.enable_fp8(on=False)


def test_what_is_not_served_says_so(tiny):
    m = tiny.model
    on = {"top_k": 40}
    for call in (lambda: m.batch_query(tiny.images[:1], ["q"], settings=on, reasoning=True),
                 lambda: m.query(tiny.images[0], "q", reasoning=True, settings=on),
                 lambda: m.query_many_reasoning(tiny.images[0], ["q"], settings=on),
                 lambda: m.batch_detect(tiny.images[:1], ["cat"], settings={"min_p": 0.1}),
                 lambda: m.batch_point(tiny.images[:1], ["cat"], settings=on),
                 lambda: m.detect_many(tiny.images[0], ["cat"], settings=on),
                 lambda: m.batch_generate_ids_pipelined([(tiny.images[:1], tiny.prompts[:1])], min_p=0.5)):
        with pytest.raises(ValueError, match="top_k / min_p are not served"):
            call()
