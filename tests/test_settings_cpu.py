"""The settings record without a GPU (moondream_amd/settings.py): both constructors against the validators they are
built on -- the same per-row values, the same neutral -> None decisions, the same errors -- the pick dispatch against a
launch-recording model, and the refusal helper against the texts of the blocks it replaced."""
import numpy as np
import pytest

from moondream_amd.beam import beams_of
from moondream_amd.constraint import TokenAutomaton, check_constraints
from moondream_amd.decode_loop import (FILTER_NEUTRAL, PENALTY_NEUTRAL, Sampling, check_filters, check_penalties, check_top_logprobs,
                                       pick_tokens)
from moondream_amd.settings import CallSettings, RowSettings, refuse_settings

V, ANSWER = 64, 3
A = TokenAutomaton.allowed_tokens(range(10, 20))
B = TokenAutomaton.choices([[10, 11], [12]], 0)
ONLY_ANSWER = TokenAutomaton.allowed_tokens([ANSWER])  # validate() refuses it
CHECK = lambda constraints, n: check_constraints(constraints, n, V, ANSWER)  # what the model hands the constructors


def never(*a):
    raise AssertionError("the grammar was compiled")


def outcome(f):
    try:
        return ("ok", f())
    except Exception as e:  # noqa: BLE001 (the type is part of what is compared)
        return (type(e), str(e))


PENALTIES = [(1.0, 0.0, 0.0), (None, None, None), ([1, 1], 0, np.float32(0)), (1.2, 0.0, [0.0, -0.5]), (1, -1e4, [4e3, 0]),
             ([1.0, 1.5], [0.0, 0.0], None),
             (0.0, 0, 0), (-1.0, 0, 0), (float("nan"), 0, 0), (float("inf"), 0, 0), (1, float("inf"), 0), (1, 0, float("nan")),
             ([1.0], 0, 0), (1, [0.0] * 3, 0), ("x", 0, 0), (1, object(), 0), (True, 0, 0)]
FILTERS = [(0, 0.0), (None, None), ([0, 0], np.float32(0)), (40, 0.0), ([1, 0], [0, 0.5]), (np.int64(7), 1),
           (-1, 0), (True, 0), (1.5, 0), ("3", 0), (object(), 0), (0, 1.5), (0, -0.1), (0, float("nan")), (0, float("inf")),
           (0, "x"), (0, True), ([1], 0), (0, [0.1] * 3), ([1, -1], 0)]
CONSTRAINTS = [None, A, [A, None], [None, None], [A, B], (B, B), [A], [A, A, A], "x", [A, 5], ONLY_ANSWER, [None, ONLY_ANSWER]]
N = 2


def both(**kw):
    """The two constructors on the same settings: the keyword form and the dict form must agree."""
    a = outcome(lambda: CallSettings.of(N, CHECK, compile_grammar=never, **kw))
    b = outcome(lambda: CallSettings.of_settings(dict(kw), N, CHECK, never))
    if a[0] == "ok":  # the dict form applies the reference's sampling defaults where the keyword form has the calls'
        assert b[0] == "ok"
        for x, y in zip(a[1].rows, b[1].rows):
            assert (x.top_k, x.min_p, x.penalties, x.constraint) == (y.top_k, y.min_p, y.penalties, y.constraint)
        assert [a[1].penalties, a[1].filters, a[1].constraints] == [b[1].penalties, b[1].filters, b[1].constraints]
    else:
        assert a == b
    return a


@pytest.mark.parametrize("args", PENALTIES)
def test_penalties_are_check_penalties(args):
    want = outcome(lambda: check_penalties(*args, N))
    got = both(**dict(zip(("repetition_penalty", "presence_penalty", "frequency_penalty"), args)))
    if want[0] != "ok":
        assert got == want
        return
    assert got[1].penalties == want[1]  # None for None: the launch does not exist
    assert [r.penalties for r in got[1].rows] == (want[1] or [PENALTY_NEUTRAL] * N)
    assert [r.penalised for r in got[1].rows] == [p != PENALTY_NEUTRAL for p in want[1] or [PENALTY_NEUTRAL] * N]


@pytest.mark.parametrize("args", FILTERS)
def test_filters_are_check_filters(args):
    want = outcome(lambda: check_filters(*args, N))
    got = both(top_k=args[0], min_p=args[1], temperature=0.5)
    if want[0] != "ok":
        assert got == want
        return
    assert got[1].filters == want[1]
    assert [(r.top_k, r.min_p) for r in got[1].rows] == (want[1] or [FILTER_NEUTRAL] * N)
    assert [r.filtered for r in got[1].rows] == [f != FILTER_NEUTRAL for f in want[1] or [FILTER_NEUTRAL] * N]
    greedy = CallSettings.of(N, CHECK, top_k=args[0], min_p=args[1])
    assert greedy.filters == want[1] and not any(r.filtered for r in greedy.rows)  # a greedy row ignores the cuts


@pytest.mark.parametrize("value", CONSTRAINTS)
def test_constraints_are_check_constraints(value):
    want = outcome(lambda: check_constraints(value, N, V, ANSWER))
    got = both(constraints=value)
    if want[0] != "ok":
        assert got == want
        return
    assert got[1].constraints == want[1]
    assert [r.constraint for r in got[1].rows] == (want[1] or [None] * N)


def test_defaults_and_what_is_call_wide():
    assert RowSettings() == RowSettings(0.0, 0.3, 0, 0.0, PENALTY_NEUTRAL, None)
    plain = CallSettings.of_settings(None, 3, CHECK)
    assert (plain.max_tokens, plain.temperature, plain.top_p) == (768, 0.5, 0.3)  # the reference's defaults
    assert plain.rows[0].penalties == PENALTY_NEUTRAL and (plain.rows[0].top_k, plain.rows[0].min_p) == FILTER_NEUTRAL
    assert (plain.penalties, plain.filters, plain.constraints, plain.beams, plain.generator, plain.variant, plain.variants) == (None,) * 7
    assert all(r.sampled and not (r.filtered or r.penalised or r.constrained) for r in plain.rows)
    g = object()
    st = {"max_tokens": 9, "temperature": 0, "top_p": 0.9, "generator": g, "variant": "v", "variants": ["a", None], "num_beams": 3,
          "length_penalty": 0.5, "top_k": [4, 0], "presence_penalty": 0.25}
    rec = CallSettings.of_settings(st, 2, CHECK)
    assert (rec.max_tokens, rec.temperature, rec.top_p, rec.generator, rec.variant, rec.variants) == (9, 0, 0.9, g, "v", ["a", None])
    assert rec.beams == beams_of(st) == (3, 0.5, False)
    assert rec.filters == [(4, 0.0), (0, 0.0)] and rec.penalties == [(1.0, 0.25, 0.0)] * 2 and not rec.rows[0].sampled
    kw = CallSettings.of(2, CHECK, max_tokens=9, temperature=0, top_p=0.9, generator=g, variant="v", variants=["a", None],
                         top_k=[4, 0], presence_penalty=0.25, beam_settings=st)
    assert kw == rec  # a dict and the keyword arguments made from it
    back = rec.reorder([1, 0])
    assert back.rows == rec.rows[::-1] and back.filters == [(0, 0.0), (4, 0.0)] and back.reorder([1, 0]) == rec
    assert CallSettings.of(1, CHECK, return_logprobs=True, top_logprobs=5).top_logprobs == check_top_logprobs(5, True) == 5
    for bad in (dict(top_logprobs=5), dict(top_logprobs=33, return_logprobs=True)):
        assert outcome(lambda: CallSettings.of(1, CHECK, **bad)) == outcome(
            lambda: check_top_logprobs(bad["top_logprobs"], bad.get("return_logprobs", False)))
    assert outcome(lambda: CallSettings.of_settings({"num_beams": 0}, 1, CHECK)) == outcome(lambda: beams_of({"num_beams": 0}))


def test_the_grammar_is_compiled_last_and_only_once_everything_else_holds():
    compiled = []

    def compile_grammar(kind, value, vocab_bytes):
        compiled.append((kind, value, vocab_bytes))
        return A

    rec = CallSettings.of_settings({"regex": "a+", "vocab_bytes": "vb"}, 2, CHECK, compile_grammar)
    assert compiled == [("regex", "a+", "vb")] and rec.constraints == [A, A]
    rec = CallSettings.of(2, CHECK, json_schema={"type": "boolean"}, compile_grammar=compile_grammar)
    assert compiled[1:] == [("json_schema", {"type": "boolean"}, None)] and rec.constraints == [A, A]
    for bad in ({"top_k": -1}, {"min_p": 2}, {"repetition_penalty": 0}, {"num_beams": 99}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            CallSettings.of_settings({"regex": "a+", **bad}, 2, CHECK, never)
    # given two ways: refused before anything else is looked at
    with pytest.raises(ValueError, match="mutually exclusive"):
        CallSettings.of_settings({"regex": "a", "json_schema": {}, "top_k": -1}, 2, CHECK, never)
    with pytest.raises(ValueError, match="regex and constraints are mutually exclusive"):
        CallSettings.of_settings({"regex": "a", "constraints": A}, 2, CHECK, never)
    # the fixed order of several invalid settings: penalties, cuts, top_logprobs, constraints, beams
    order = [("repetition_penalty", 0), ("top_k", -1), ("top_logprobs", 99), ("constraints", "x"), ("num_beams", 99)]
    for i, (name, _) in enumerate(order):
        kw = dict(order[i:])
        beam = {"num_beams": kw.pop("num_beams")}
        with pytest.raises(ValueError, match=name):
            CallSettings.of(2, CHECK, return_logprobs=True, beam_settings=beam, **kw)
    # beam search refuses constraints on its own route: nothing is compiled for it
    assert CallSettings.of_settings({"regex": "a+", "num_beams": 2}, 2, CHECK, never).constraints is None


# ------------------------------------------------------------------ the pick dispatch
class Picks:
    def __init__(self):
        self.calls = []

    def _pick(self, logits, temperature, top_p, suppress_id=-1, generator=None, probs_out=None, row_perm=None, uniforms=None, out=None):
        self.calls.append(("pick", logits, temperature, top_p, suppress_id, generator, probs_out, row_perm, uniforms, out))
        return "picked"

    def _pick_rows(self, logits, temperature_dev, top_p_dev, suppress_id, uniforms, out=None):
        self.calls.append(("pick_rows", logits, temperature_dev, top_p_dev, suppress_id, uniforms, out))
        return "rows"

    def _pick_rows_filtered(self, logits, temperature_dev, top_p_dev, top_k_dev, min_p_dev, suppress_id, uniforms, out=None):
        self.calls.append(("pick_rows_filtered", logits, temperature_dev, top_p_dev, top_k_dev, min_p_dev, suppress_id, uniforms, out))
        return "filtered"


class Dev:
    """Stands for a device tensor: it has an address, and rows."""

    def __init__(self, name):
        self.name = name

    def data_ptr(self):
        return id(self)

    def __getitem__(self, rows):
        return (self.name, rows.start, rows.stop)


def test_pick_dispatch_calls_the_wrapper_each_site_called():
    t, p, k, mp = Dev("t"), Dev("p"), Dev("k"), Dev("mp")
    m = Picks()
    # no record: the argmax, as ``_first_token`` asked for it (``_pick(logits, 0.0, 0.0)``)
    assert pick_tokens(m, None, "lg") == "picked"
    assert m.calls.pop() == ("pick", "lg", 0.0, 0.0, -1, None, None, None, None, None)
    # the argmax of a penalised or masked chunk: ``_pick(lg, 0.0, 0.0, suppress_id, None, uniforms=None, out=tok_out)``
    pick_tokens(m, Sampling(0.0, 0.0), "lg", 7, out="out")
    assert m.calls.pop() == ("pick", "lg", 0.0, 0.0, 7, None, None, None, None, "out")
    # the call's settings: run_chunk's form (the chunk's uniforms) and the first token's (the generator's draws, permuted)
    pick_tokens(m, Sampling(0.5, 0.3, "gen"), "lg", 7, "u", out="out")
    assert m.calls.pop() == ("pick", "lg", 0.5, 0.3, 7, "gen", None, None, "u", "out")
    pick_tokens(m, Sampling(0.5, 0.3, "gen"), "lg", row_perm="perm")
    assert m.calls.pop() == ("pick", "lg", 0.5, 0.3, -1, "gen", None, "perm", None, None)
    # every row's own
    assert pick_tokens(m, Sampling(t, p), "lg", 7, "u", out="out") == "rows"
    assert m.calls.pop() == ("pick_rows", "lg", t, p, 7, "u", "out")
    pick_tokens(m, Sampling(t, p), "lg", -1, "u")
    assert m.calls.pop() == ("pick_rows", "lg", t, p, -1, "u", None)
    # ... with the two cuts
    assert pick_tokens(m, Sampling(t, p, top_k=k, min_p=mp), "lg", 7, "u", out="out") == "filtered"
    assert m.calls.pop() == ("pick_rows_filtered", "lg", t, p, k, mp, 7, "u", "out")
    assert not m.calls


def test_sampling_cut():
    t, p, k, mp = Dev("t"), Dev("p"), Dev("k"), Dev("mp")
    cut = Sampling(t, p, "gen", "perm", k, mp).cut(2, 5)
    # the rows' tensors cut; the call's generator and draw order stay behind (the caller cuts the draws itself)
    assert (cut.temperature, cut.top_p, cut.generator, cut.row_perm, cut.top_k, cut.min_p) == (
        ("t", 2, 5), ("p", 2, 5), None, None, ("k", 2, 5), ("mp", 2, 5))
    plain = Sampling(t, p).cut(0, 1)
    assert (plain.temperature, plain.top_p, plain.top_k, plain.min_p) == (("t", 0, 1), ("p", 0, 1), None, None)


# ------------------------------------------------------------------ the refusal helper
HF = {None: "HfMoondream (use MoondreamModel's calls)", "spatial_refs": "HfMoondream's own calls (use MoondreamModel's)"}
REASONING = {None: "reasoning queries",
             "filters": "reasoning queries (the reasoning loop picks with the call's temperature and top-p alone)"}
DETECT = {None: "detect: its loop decodes coordinates, not tokens picked from logits",
          "filters": "detect: its loop decodes coordinates, not tokens sampled from logits",
          "beams": "detect: its loop decodes coordinates, not token hypotheses"}
BEAM = "beam search (num_beams > 1)"
SCORE = {"spatial_refs": "score_ids / query_choices (the scorer's prompts carry no encoded references)",
         "constraints": "score_ids (no token is picked: scores are the model's own)",
         "penalties": "score_ids (no decode step runs: scores are the model's own)"}
PIPELINED = {"spatial_refs": "the pipelined engine (its prefill arena embeds token ids alone)",
             "filters": "the pipelined engine (it decodes greedily: there is no sampled row to cut)",
             "constraints": "the pipelined engine (its paired decode keeps no automaton states)",
             "penalties": "the pipelined engine (its paired decode keeps no histories)"}
ALL5 = ("penalties", "constraints", "filters", "beams", "spatial_refs")
# (the place's wording, its families in its order, the text of the parent commit's block per family)
SITES = {
    "hf.answer_question / batch_answer / generate": (HF, ALL5, {
        "penalties": "repetition_penalty / presence_penalty / frequency_penalty are not served by HfMoondream (use MoondreamModel's calls)",
        "constraints": "constraints are not served by HfMoondream (use MoondreamModel's calls)",
        "filters": "top_k / min_p are not served by HfMoondream (use MoondreamModel's calls)",
        "beams": "num_beams > 1 (beam search) is not served by HfMoondream (use MoondreamModel's calls)",
        "spatial_refs": "spatial_refs are not served by HfMoondream's own calls (use MoondreamModel's)"}),
    "query(reasoning=True) / _check_reasoning_served": (REASONING, ALL5[:4], {
        "penalties": "repetition_penalty / presence_penalty / frequency_penalty are not served by reasoning queries",
        "constraints": "constraints are not served by reasoning queries",
        "filters": "top_k / min_p are not served by reasoning queries (the reasoning loop picks with the call's temperature and top-p alone)",
        "beams": "num_beams > 1 (beam search) is not served by reasoning queries"}),
    "_check_detect_settings": (DETECT, ALL5[:4], {
        "penalties": "repetition_penalty / presence_penalty / frequency_penalty are not served by detect: its loop decodes coordinates, not tokens picked from logits",
        "constraints": "constraints are not served by detect: its loop decodes coordinates, not tokens picked from logits",
        "filters": "top_k / min_p are not served by detect: its loop decodes coordinates, not tokens sampled from logits",
        "beams": "num_beams > 1 (beam search) is not served by detect: its loop decodes coordinates, not token hypotheses"}),
    "_beam_best_ids": (BEAM, ALL5[:2], {
        "penalties": "repetition_penalty / presence_penalty / frequency_penalty are not served by beam search (num_beams > 1)",
        "constraints": "constraints are not served by beam search (num_beams > 1)"}),
    "score_ids": (SCORE, ("spatial_refs", "constraints", "penalties"), {
        "spatial_refs": "spatial_refs are not served by score_ids / query_choices (the scorer's prompts carry no encoded references)",
        "constraints": "constraints are not served by score_ids (no token is picked: scores are the model's own)",
        "penalties": "repetition_penalty / presence_penalty / frequency_penalty are not served by score_ids (no decode step runs: scores are the model's own)"}),
    "the pipelined engine": (PIPELINED, ("spatial_refs", "filters", "constraints", "penalties"), {
        "spatial_refs": "spatial_refs are not served by the pipelined engine (its prefill arena embeds token ids alone)",
        "filters": "top_k / min_p are not served by the pipelined engine (it decodes greedily: there is no sampled row to cut)",
        "constraints": "constraints are not served by the pipelined engine (its paired decode keeps no automaton states)",
        "penalties": "repetition_penalty / presence_penalty / frequency_penalty are not served by the pipelined engine (its paired decode keeps no histories)"}),
}
ON = {"penalties": {"presence_penalty": 0.5}, "constraints": {"constraints": A}, "filters": {"top_k": 40}, "beams": {"num_beams": 2},
      "spatial_refs": {"spatial_refs": [[(0.5, 0.5)]]}}
NEUTRAL = {"repetition_penalty": 1.0, "presence_penalty": [0.0, 0.0], "frequency_penalty": None, "constraints": [None, None], "top_k": 0,
           "min_p": 0.0, "num_beams": 1, "spatial_refs": [None, []]}


@pytest.mark.parametrize("site", SITES)
def test_refusal_texts_are_the_old_blocks(site):
    where, families, texts = SITES[site]
    assert set(texts) == set(families)
    for settings in (None, {}, NEUTRAL):
        refuse_settings(settings, where, families, 2)
    for family in families:
        with pytest.raises(ValueError) as e:
            refuse_settings({**NEUTRAL, **ON[family]}, where, families, 2)
        assert str(e.value) == texts[family]
    with pytest.raises(ValueError) as e:  # every family on: the first of the place's order speaks
        refuse_settings({k: v for f in families for k, v in ON[f].items()}, where, families, 2)
    assert str(e.value) == texts[families[0]]
    if "constraints" in families:
        with pytest.raises(ValueError) as e:  # a pattern is a constraint yet to be compiled
            refuse_settings({"regex": "a+"}, where, families)
        assert str(e.value) == texts["constraints"]
    if "spatial_refs" in families:
        with pytest.raises(ValueError) as e:  # the call's own argument, beside the settings
            refuse_settings(None, where, families, spatial_refs=[[(0.1, 0.2)]])
        assert str(e.value) == texts["spatial_refs"]
    with pytest.raises(ValueError, match="top_k must be an integer"):  # a value that is none is the validator's error
        refuse_settings({"top_k": -1}, where, ("filters",))
