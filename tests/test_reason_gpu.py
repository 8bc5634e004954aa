"""batch_query(..., reasoning=True) / query_many_reasoning on the MI355X: the reference's recorded ids, the
single-sequence path row by row (grounding and ragged phases included), the suppression rule of every phase, the shared
prefix, and sampling."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from moondream_amd import _lib, synth
from moondream_amd.config import get_config

pytestmark = pytest.mark.gpu
K_NONE, K_REASON, K_SUFFIX, K_ANSWER = 0, 1, 2, 3
GREEDY8 = {"temperature": 0, "max_tokens": 8}


def load_golden(golden_dir, name):
    path = os.path.join(golden_dir, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not generated")
    return np.load(path)


def build(cfg_name, seed, max_batch=4):
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(cfg_name)
    sd = synth.synthetic_state_dict(cfg, seed=seed, device="cuda")
    return cfg, MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=max_batch)


def golden_images(g):
    return [Image.fromarray(synth.synthetic_image_array(int(g[f"case{i}.image_index"]), int(g["seed"]), (378, 378)), "RGB")
            for i in range(int(g["n_cases"]))]


def ids_of(text):
    return [int(t) for t in text.split()]


@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = load_golden(golden_dir, "tiny_reasoning.npz")
    cfg, model = build("tiny", int(g["seed"]))
    return g, cfg, model


def check_golden(res, g):
    assert len(res) == int(g["n_cases"])
    for i, r in enumerate(res):
        assert set(r) == {"reasoning", "answer"} and set(r["reasoning"]) == {"text", "grounding"}
        assert ids_of(r["reasoning"]["text"]) == g[f"case{i}.reasoning_tokens"].tolist(), i
        assert ids_of(r["answer"]) == g[f"case{i}.answer_tokens"].tolist(), i
        assert len(r["reasoning"]["grounding"]) == int(g[f"case{i}.n_grounding"])


# ------------------------------------------------------------------ 5. the reference's ids
def test_golden_greedy_eager_and_compiled(tiny):
    """Both recorded cases (every reference margin >= 11) in ONE batch: reasoning ids, answer ids and the grounding count
    are the reference's, eagerly and replayed from captured graphs; a second compiled call captures nothing."""
    g, cfg, model = tiny
    assert int(g["max_tokens"]) == GREEDY8["max_tokens"]
    imgs, qs = golden_images(g), ["11 12 13"] * int(g["n_cases"])
    check_golden(model.batch_query(imgs, qs, settings=GREEDY8, reasoning=True), g)
    model.compile()
    try:
        model._graphs.clear()
        check_golden(model.batch_query(imgs, qs, settings=GREEDY8, reasoning=True), g)
        n_graphs = len(model._graphs)
        assert n_graphs >= 1 and all(k[0] == "reason" for k in model._graphs)
        check_golden(model.batch_query(imgs, qs, settings=GREEDY8, reasoning=True), g)
        assert len(model._graphs) == n_graphs
    finally:
        model.use_graphs = False
        model._graphs.clear()
    # reasoning=False: strings, as ever
    plain = model.batch_query(imgs, qs, settings=GREEDY8)
    assert all(isinstance(s, str) for s in plain) and plain == model.batch_query(imgs, qs, GREEDY8, False)


def test_2b_golden_greedy(golden_dir):
    """The same check at the 2B shapes (tests/golden/md2b_reasoning.npz, recorded from the reference's public API)."""
    g = load_golden(golden_dir, "md2b_reasoning.npz")
    cfg, model = build("2b", int(g["seed"]))
    imgs, qs = golden_images(g), ["11 12 13"] * int(g["n_cases"])
    st = {"temperature": 0, "max_tokens": int(g["max_tokens"])}
    check_golden(model.batch_query(imgs, qs, settings=st, reasoning=True), g)
    check_golden(model.query_many_reasoning(imgs[0], qs[:1], settings=st) + model.query_many_reasoning(imgs[1], qs[1:], settings=st), g)


# ------------------------------------------------------------------ 6. batch against single
def single_path(model, cfg, img, question, script, settings):
    """query(reasoning=True)'s two stages, with the reasoning picks scripted through ``_pick`` (None: unscripted)."""
    tk = cfg.tokenizer
    tpl = tk.templates["query"]
    prompt = list(tpl["prefix"]) + ids_of(question) + list(tpl["suffix"]) + [tk.thinking_id]
    enc = model.encode_image(img)
    model.load_encoded_image(enc)
    orig = model._pick
    if script is not None:
        seq = iter(script)
        model._pick = lambda logits, *a, **k: torch.tensor([next(seq)], dtype=torch.int32, device=logits.device)
    try:
        pos, text, grounding = model._generate_reasoning(torch.tensor([prompt]), enc.pos, settings)
    finally:
        model._pick = orig
    answer = "".join(model._generate_answer(torch.tensor([list(tpl["suffix"])]), pos, settings))
    return pos, text, grounding, ids_of(answer)


def test_batch_equals_single_with_grounding_and_ragged_phases(tiny):
    g, cfg, model = tiny
    tk = cfg.tokenizer
    mt = 6
    st = {"temperature": 0, "max_tokens": mt}
    imgs = [synth.synthetic_image(i, 1) for i in range(4)]
    qs = ["11 12 13", "21 22", "31 32 33 34", "41"]  # ragged prompts: the rows are reordered by length inside
    grounded = [tk.start_ground_points_id, tk.coord_id, tk.coord_id, tk.end_ground_id, tk.answer_id]
    scripts = [
        grounded,                                        # grounding, then answer_id ends the reasoning
        [50, 51, 52, 53, 54, 55, 99],                    # mt kept tokens: ends on the budget (99: picked after it, dropped)
        [60, tk.coord_id, tk.coord_id, tk.coord_id, tk.answer_id],  # an odd number of coordinates, no new chunk
        None,                                            # unscripted
    ]
    forced = torch.full((2 * mt + 1, 4), -1, dtype=torch.int32)
    for r, s in enumerate(scripts):
        if s is not None:
            forced[: min(len(s), mt + 1), r] = torch.tensor(s[: mt + 1], dtype=torch.int32)
    model.set_strict_batch_invariance(True)
    try:
        rows = model._batch_query_reasoning(imgs, qs, st, share_prefix=False, forced=forced)
        singles = [single_path(model, cfg, imgs[r], qs[r], scripts[r], st) for r in range(4)]
    finally:
        model.set_strict_batch_invariance(False)
    for r, (pos, text, grounding, answer) in enumerate(singles):
        got = rows[r]
        print(f"row {r}: reasoning {got['reasoning_ids']} answer {got['answer_ids']} grounding {got['grounding']} pos {got['pos']}")
        assert got["text"] == text, r
        assert got["answer_ids"] == answer, r
        assert got["pos"] == pos, r
        assert len(got["grounding"]) == len(grounding), r
        for a, b in zip(got["grounding"], grounding):
            assert (a["start_idx"], a["end_idx"]) == (b["start_idx"], b["end_idx"]), r
            assert a["points"] == b["points"], (r, a["points"], b["points"])  # strict mode: a row's bits do not depend on its batch
    # the scripts did what they were written for
    assert rows[0]["reasoning_ids"] == grounded[:-1] and len(rows[0]["grounding"]) == 1 and len(rows[0]["grounding"][0]["points"]) == 1
    assert all(0.0 <= c < 1.0 for c in rows[0]["grounding"][0]["points"][0])
    assert rows[1]["reasoning_ids"] == scripts[1][:mt]
    assert len(rows[2]["grounding"]) == 1 and len(rows[2]["grounding"][0]["points"]) == 1  # three coordinates: one pair
    assert len({len(r["reasoning_ids"]) for r in rows}) > 1  # ragged phases in one lockstep
    assert all(1 <= len(r["answer_ids"]) <= mt for r in rows)


# ------------------------------------------------------------------ 7. what each phase suppresses
@pytest.mark.parametrize("which", ["eos_id", "size_id", "answer_id"])
def test_suppression_rule_per_phase(tiny, which):
    """One id is made the argmax of EVERY unsuppressed pick (a large lm_head bias).  A reasoning step then never yields
    eos_id / size_id, an answer step never answer_id -- while the pick of the step that feeds the suffix token, like the
    prompt pass's, suppresses nothing and yields exactly that id."""
    from moondream_amd.moondream import _Rows

    g, cfg, model = tiny
    tk = cfg.tokenizer
    hot = getattr(tk, which)
    mt = 4
    tpl = tk.templates["query"]
    prompt = list(tpl["prefix"]) + [11, 12, 13] + list(tpl["suffix"]) + [tk.thinking_id]
    imgs = [synth.synthetic_image(i, 1) for i in range(2)]
    forced = torch.full((2 * mt + 1, 2), -1, dtype=torch.int32)
    forced[0, 1] = 17  # row 1 starts on an ordinary token whatever the prompt pass picked; row 0 is unscripted
    seen = []

    def on_chunk(step0, n, state, planes):
        assert n == 1
        seen.append(dict(kind=planes["kind"][0].tolist(), suppress=state["suppress"].tolist(), picked=planes["tokens"][1].tolist(),
                         consumed=planes["tokens"][0].tolist(), logits=model._decode_logits(2)[:2].float().cpu()))

    bias = model.w.lm_head.b
    old = bias[hot].clone()
    try:
        with torch.inference_mode():
            bias[hot] = 1000.0
            prep = model._prepare_sequences(imgs, [prompt] * 2, rows=_Rows())
            assert prep.first.tolist() == [hot, hot]  # the prompt pass's pick suppresses nothing
            res = model._reason_loop(prep.hidden_last, prep.first, prep.next_pos, _Rows(), mt, None, forced.cuda(), check_every=1, on_chunk=on_chunk)
    finally:
        with torch.inference_mode():
            bias[hot] = old
    kinds = set()
    for s in seen:
        for r in range(2):
            kind, sup, lg = s["kind"][r], s["suppress"][r], s["logits"][r]
            masked = sorted(torch.nonzero(torch.isinf(lg) & (lg < 0)).reshape(-1).tolist())
            kinds.add(kind)
            if kind == K_REASON:
                assert sup == [tk.eos_id, tk.size_id] and masked == sorted({tk.eos_id, tk.size_id})
                assert s["picked"][r] not in (tk.eos_id, tk.size_id)
                assert s["picked"][r] == (hot if which == "answer_id" else int(lg.argmax()))
            elif kind == K_SUFFIX:
                assert sup == [-1, -1] and masked == []
                assert s["picked"][r] == hot  # answer_id included: unsuppressed here
            elif kind == K_ANSWER:
                assert sup == [tk.answer_id, -1] and masked == [tk.answer_id]
                assert s["picked"][r] != tk.answer_id
                assert s["picked"][r] == (int(lg.argmax()) if which == "answer_id" else hot)
            else:
                assert sup == [-1, -1] and masked == []
    assert {K_REASON, K_SUFFIX} <= kinds
    for r in res:
        assert not set(r["reasoning_ids"][1:]) & {tk.eos_id, tk.size_id}
        assert tk.answer_id not in r["answer_ids"][1:]
    if which == "answer_id":
        # row 0: the prompt pass picks answer_id -> no reasoning token at all; the suffix step picks it again, and it is KEPT
        # as the first answer token; row 1: one forced token, then answer_id ends the reasoning
        assert res[0]["reasoning_ids"] == [] and res[1]["reasoning_ids"] == [17]
        assert all(r["answer_ids"][0] == tk.answer_id for r in res)
        assert K_ANSWER in kinds
    elif which == "eos_id":
        # eos is an ordinary (kept) token when the prompt pass picks it while reasoning; the suffix step yields eos: an
        # empty answer
        assert res[0]["reasoning_ids"][0] == tk.eos_id and res[1]["reasoning_ids"][0] == 17
        assert all(r["answer_ids"] == [] for r in res)
    else:
        assert res[0]["reasoning_ids"][0] == tk.size_id and all(r["answer_ids"] == [tk.size_id] * mt for r in res)


# ------------------------------------------------------------------ 8. one image, many questions
def test_query_many_reasoning_equals_batch_over_copies(tiny):
    g, cfg, model = tiny
    img = golden_images(g)[0]
    qs = ["11 12 13", "21 22", "11 12 13", "31 32 33 34"]
    enc = model.encode_image(img)
    ref = model.batch_query([enc] * len(qs), qs, settings=GREEDY8, reasoning=True)
    got = model.query_many_reasoning(img, qs, settings=GREEDY8)
    assert got == ref
    assert ids_of(got[0]["reasoning"]["text"]) == g["case0.reasoning_tokens"].tolist() and got[0] == got[2]
    plain = model.query_many(img, qs[:2], settings=GREEDY8)
    assert [set(p) for p in plain] == [{"answer"}] * 2  # query_many itself: as before


# ------------------------------------------------------------------ 9. sampling
def test_sampling_is_seeded_and_respects_the_suppression(tiny):
    g, cfg, model = tiny
    tk = cfg.tokenizer
    imgs, qs = golden_images(g), ["11 12 13"] * int(g["n_cases"])

    def run(seed, temperature=4.0):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        st = {"temperature": temperature, "top_p": 0.95, "max_tokens": 8, "generator": gen}
        return model._batch_query_reasoning(imgs, qs, st, share_prefix=False)

    a, b, c = run(5), run(5), run(6)
    ids = lambda rows: [(r["reasoning_ids"], r["answer_ids"]) for r in rows]
    assert ids(a) == ids(b)
    print("seed 5:", ids(a), "\nseed 6:", ids(c), "(allowed to differ)")
    for rows in (a, c):
        for r in rows:
            assert not set(r["reasoning_ids"]) & {tk.eos_id, tk.size_id}
            assert tk.answer_id not in r["answer_ids"][1:]
            assert len(r["reasoning_ids"]) <= 8 and len(r["answer_ids"]) <= 8
    greedy = run(7, temperature=0)  # temperature 0 with a generator at hand: the golden's ids
    for i, r in enumerate(greedy):
        assert r["reasoning_ids"] == g[f"case{i}.reasoning_tokens"].tolist() and r["answer_ids"] == g[f"case{i}.answer_tokens"].tolist()
    assert ids(a) != ids(greedy)  # temperature 4 over margins of ~12 logits does sample
