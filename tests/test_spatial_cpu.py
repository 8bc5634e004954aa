"""Spatial references without a GPU: the prompt ids and the descriptor record against the oracle's ``spatial_prompt`` /
``encode_spatial_refs``, the checks (raised before any device work), the reorder by a plan's order, the table md_spatial_ref_embed
reads, and the entry point's host validation."""
import ctypes
import types

import numpy as np
import pytest
import torch

from moondream_amd import _lib, synth
from moondream_amd.config import get_config
from moondream_amd.hf_moondream import HfMoondream
from moondream_amd.moondream import IdTokenizer
from moondream_amd.shared_prefix import plan_rows
from moondream_amd.spatial import (KIND_COORD, KIND_SIZE, SpatialRecord, check_spatial_refs, placeholders, ref_values, refs_of,
                                   refuse_spatial_refs, spatial_prompt_ids)
from oracle import moondream_oracle as O
from test_logprobs_cpu import IMG, FakeEngine, FakeModel, host_model

CFG = get_config("tiny")
TK = CFG.tokenizer
TPL = TK.templates["query"]
# 0.3 + 0.4 is not representable in bf16, nor is its half; (0.1, 0.2, 0.7, 0.9)'s centre (0.4, 0.55) neither
REFS = [(0.25, 0.75), (0.1, 0.2, 0.7, 0.9), (0.3, 0.3, 0.4, 0.40625), (0.123456, 0.654321)]


@pytest.fixture(scope="module")
def oracle():
    return O.Oracle(CFG, synth.synthetic_state_dict(CFG, seed=1))


def bf16_bits(t):
    return (t.contiguous().view(torch.int16).numpy().astype(np.int32) & 0xFFFF).reshape(-1).tolist()


def engine(region=object()):
    eng = FakeEngine(FakeModel(), max_live=2)
    eng.model.tokenizer = IdTokenizer()
    eng.model.w = types.SimpleNamespace(region=region)
    return eng


def region_model(**kw):
    m = host_model(**kw)
    m.w.region = object()
    return m


def test_prompt_ids_and_positions_are_the_oracles(oracle):
    question = [11, 12, 13]
    tail = question + list(TPL["suffix"]) * 2
    ids, _ = oracle.spatial_prompt(list(TPL["prefix"]), REFS, tail)
    mine = spatial_prompt_ids(TPL["prefix"], REFS, tail, TK.coord_id, TK.size_id)
    assert mine == ids
    assert placeholders(REFS, TK.coord_id, TK.size_id) == ids[len(TPL["prefix"]) : len(ids) - len(tail)]
    rec = SpatialRecord.build([REFS], len(TPL["prefix"]), [len(ids)])
    # by position: exactly the placeholders, in order, each of its kind
    where = [i for i, t in enumerate(ids) if t in (TK.coord_id, TK.size_id)]
    assert rec.tokens[:, 1].tolist() == where and len(rec) == 2 * 4 + 2
    assert rec.tokens[:, 2].tolist() == [KIND_SIZE if ids[i] == TK.size_id else KIND_COORD for i in where]
    assert rec.tokens[:, 0].tolist() == [0] * len(where) and rec.row_ptr.tolist() == [0, len(where)]
    # the model's own builder gives the same prompt and record
    m = region_model()
    prompts, got = m._query_prompts_spatial([IMG], ["11 12 13"], [REFS], list(TPL["suffix"]) * 2)
    assert prompts == [ids] and np.array_equal(got.tokens, rec.tokens)
    plain, none = m._query_prompts_spatial([IMG], ["11 12 13"], [[]], list(TPL["suffix"]) * 2)
    assert none is None and plain == m._query_prompts(["11 12 13"])


def test_descriptor_values_are_the_bf16_tensors_the_reference_builds(oracle):
    seen = {}
    oracle.encode_coordinate = lambda c: seen.__setitem__("c", c) or torch.zeros(c.shape[0], CFG.text.dim, dtype=torch.bfloat16)
    oracle.encode_size = lambda s: seen.__setitem__("s", s) or torch.zeros(s.shape[0], CFG.text.dim, dtype=torch.bfloat16)
    try:
        oracle.encode_spatial_refs(REFS)
    finally:
        del oracle.encode_coordinate, oracle.encode_size
    c, s = ref_values(REFS)
    assert bf16_bits(c) == bf16_bits(seen["c"]) and bf16_bits(s) == bf16_bits(seen["s"])
    centre = (0.3 + 0.4) / 2
    assert float(torch.tensor(centre, dtype=torch.bfloat16)) != centre  # a centre bf16 does not hold: rounded ONCE, from the float
    rec = SpatialRecord.build([REFS], 3, [20])
    coords = rec.tokens[rec.tokens[:, 2] == KIND_COORD]
    sizes = rec.tokens[rec.tokens[:, 2] == KIND_SIZE]
    assert coords[:, 3].tolist() == bf16_bits(seen["c"]) and coords[:, 4].tolist() == [0] * 8
    assert sizes[:, 3:].reshape(-1).tolist() == bf16_bits(seen["s"])


def test_table_addresses_rows_of_each_pass_and_follows_the_plans_order():
    rows = [[], [(0.5, 0.5)], [(0.1, 0.2, 0.3, 0.4)], [], [(0.6, 0.7), (0.1, 0.1, 0.2, 0.2)]]
    lens = [6, 8, 9, 6, 11]  # head 3 + placeholders + question 3.. : rows group by TOTAL length
    rec = SpatialRecord.build(rows, 3, lens)
    imgs = [object() for _ in rows]
    plan = plan_rows(imgs, lens, False)
    slot = rec.reorder(plan.order)
    assert [slot.prompt_len[j] for j in range(5)] == [lens[i] for i in plan.order] == sorted(lens)
    for lead in (0, 730):
        tab = slot.table(lead)
        seen = 0
        for r0, r1 in plan.groups:
            t = slot.prompt_len[r0]
            i0, i1 = slot.span(r0, r1)
            local = tab[i0:i1, 0] - slot.dst0_of(r0, lead)
            want = []
            for j in range(r0, r1):
                old = plan.order[j]
                toks = rec.tokens[rec.row_ptr[old] : rec.row_ptr[old + 1]]
                want += [(j - r0) * (lead + t) + lead + int(p) for p in toks[:, 1]]
                assert np.array_equal(tab[slot.row_ptr[j] : slot.row_ptr[j + 1], 1:], toks[:, 2:])
            assert local.tolist() == want and all(0 <= d < (r1 - r0) * (lead + t) for d in want)
            seen += i1 - i0
        assert seen == len(rec) == 2 + 3 + 5 and len(set(tab[:, 0].tolist())) == len(rec)
    assert len(SpatialRecord.build([[], []], 3, [6, 6])) == 0
    with pytest.raises(ValueError):
        SpatialRecord.build([[(0.5, 0.5)]], 3, [4])  # the placeholders would end beyond the prompt


def test_checks():
    ok = dict(n_rows=2, has_image=[True, True], questions=[[11], [12]], coord_id=TK.coord_id, size_id=TK.size_id, has_region=True)
    assert check_spatial_refs(None, **ok) is None and check_spatial_refs([None, []], **ok) is None
    assert check_spatial_refs([[(1, 2)], None], **ok) == [[(1.0, 2.0)], []]
    assert check_spatial_refs([[(-3.0, 7.5, 2, 1)], []], **ok) == [[(-3.0, 7.5, 2.0, 1.0)], []]  # ranges are not checked
    bad = [[[(0.5, 0.5)]], [[(0.5, 0.5)]] * 3, "refs", [[(0.5, 0.5, 0.5)], None], [[(0.5,)], None], [[0.5, 0.5], None],
           [[(0.5, float("nan"))], None], [[(0.5, float("inf"), 0.6, 0.7)], None], [[("a", 0.5)], None], [(0.5, 0.5), None]]
    for refs in bad:
        with pytest.raises(ValueError):
            check_spatial_refs(refs, **ok)
    with pytest.raises(ValueError, match="image"):
        check_spatial_refs([[(0.5, 0.5)], None], **{**ok, "has_image": [False, True]})
    for tok in (TK.coord_id, TK.size_id):
        with pytest.raises(ValueError, match="placeholder"):
            check_spatial_refs([None, [(0.5, 0.5)]], **{**ok, "questions": [[11], [12, tok]]})
        assert check_spatial_refs([[(0.5, 0.5)], None], **{**ok, "questions": [[11], [12, tok]]}) is not None  # a ref-less row may
    with pytest.raises(NotImplementedError):
        check_spatial_refs([[(0.5, 0.5)], None], **{**ok, "has_region": False})
    assert check_spatial_refs([None, None], **{**ok, "has_region": False}) is None
    assert refs_of({"spatial_refs": [1]}) == [1] and refs_of(None, [2]) == [2] and refs_of({}) is None
    with pytest.raises(ValueError):
        refs_of({"spatial_refs": [1]}, [2])
    refuse_spatial_refs(None, "x"), refuse_spatial_refs([None, []], "x")
    with pytest.raises(ValueError, match="not served by x"):
        refuse_spatial_refs([[(0.5, 0.5)]], "x")


ON = [[(0.5, 0.5), (0.1, 0.2, 0.3, 0.4)]]


def test_errors_precede_any_device_work():
    m = region_model()  # any device work raises AttributeError
    bad = [[ON[0]] * 2, [[(0.5,)]], [[(0.5, float("nan"))]]]
    for refs in bad:
        for call in (lambda: m.batch_query([IMG], ["11"], spatial_refs=refs), lambda: m.query_many(IMG, ["11"], settings={"spatial_refs": refs}),
                     lambda: m.batch_query([IMG], ["11"], settings={"spatial_refs": refs}),
                     lambda: m.batch_query([IMG], ["11"], reasoning=True, spatial_refs=refs),
                     lambda: m.query_many_reasoning(IMG, ["11"], spatial_refs=refs)):
            with pytest.raises(ValueError):
                call()
    for q in (f"11 {TK.coord_id}", f"{TK.size_id}"):
        with pytest.raises(ValueError, match="placeholder"):
            m.batch_query([IMG], [q], spatial_refs=ON)
    with pytest.raises(ValueError):
        m.batch_query([IMG], ["11"], settings={"spatial_refs": ON}, spatial_refs=ON)
    headless = host_model()  # no region head
    headless.w.region = None
    for call in (lambda: headless.batch_query([IMG], ["11"], spatial_refs=ON), lambda: headless.query_many(IMG, ["11"], settings={"spatial_refs": ON})):
        with pytest.raises(NotImplementedError):
            call()
    eng = engine()
    for refs in ([(0.5,)], [(0.5, float("inf"))], (0.5, 0.5)):
        with pytest.raises(ValueError):
            eng.submit_query(IMG, "11", spatial_refs=refs)
    with pytest.raises(ValueError, match="placeholder"):
        eng.submit_query(IMG, f"{TK.coord_id}", spatial_refs=ON[0])
    with pytest.raises(NotImplementedError):
        engine(region=None).submit_query(IMG, "11", spatial_refs=ON[0])


def test_the_engine_keeps_the_refs_with_the_request():
    eng = engine()
    eng.submit_query(IMG, "11 12", spatial_refs=ON[0])
    eng.submit_query(IMG, "11 12")
    eng.submit_query(IMG, "11 12", spatial_refs=[])
    a, b, c = eng.sched.queue
    head = len(TPL["prefix"])
    assert a.spatial == (head, [(0.5, 0.5), (0.1, 0.2, 0.3, 0.4)]) and b.spatial is None and c.spatial is None
    assert a.prompt == spatial_prompt_ids(TPL["prefix"], a.spatial[1], [11, 12] + list(TPL["suffix"]) * 2, TK.coord_id, TK.size_id)
    assert b.prompt == c.prompt == list(TPL["prefix"]) + [11, 12] + list(TPL["suffix"]) * 2


def test_what_is_not_served_says_so():
    m = region_model()
    hf = object.__new__(HfMoondream)
    refused = [lambda: m.batch_query([IMG], ["11"], settings={"num_beams": 2}, spatial_refs=ON),
               lambda: m.query_many(IMG, ["11"], settings={"num_beams": 2, "spatial_refs": ON}),
               lambda: m.query(IMG, "11", spatial_refs=ON[0], settings={"num_beams": 2}),
               lambda: m.score_ids([IMG], [[1, 2]], [[5]], spatial_refs=ON), lambda: m.query_choices(IMG, "11", ["5"], spatial_refs=ON),
               lambda: m.query_choices(IMG, "11", ["5"], settings={"spatial_refs": ON}),
               lambda: m.batch_generate_ids_pipelined([([IMG], [[1, 2]])], spatial_refs=ON),
               lambda: hf.answer_question(IMG, "q", spatial_refs=ON[0]), lambda: hf.batch_answer([IMG], ["q"], spatial_refs=ON),
               lambda: hf.batch_answer([IMG], ["q"], settings={"spatial_refs": ON}), lambda: hf.generate(IMG, "p", spatial_refs=ON[0])]
    for call in refused:
        with pytest.raises(ValueError, match="spatial_refs|beam"):
            call()
    with pytest.raises(ValueError, match="beam"):  # whoever hands the beam route a record is refused there
        m._string_ids([IMG], [[5, 5, 1]], {"num_beams": 2}, spatial=SpatialRecord.build([[(0.5, 0.5)]], 0, [3]))
    with pytest.raises(ValueError, match="rows"):
        m.batch_generate_ids([IMG], [[1, 2]], spatial=SpatialRecord.build([[], []], 3, [6, 6]))


def test_header_binding_and_entry_point_agree():
    assert "md_spatial_ref_embed" in _lib.SIGNATURES
    lib = _lib.load()
    fn = lib.md_spatial_ref_embed
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused on the host
    ok = [p, 4, p, 256, p, 256, p, p, 512, p, 512, p, 256, p, 256, 0, 16, None]
    refused = {0: None, 1: 0, 2: None, 3: 250, 4: None, 5: 128, 6: None, 7: None, 8: 4096, 9: None, 10: 510, 11: None, 12: 0, 13: None,
               14: 255, 16: 0}
    for i, v in refused.items():
        args = list(ok)
        args[i] = v
        assert fn(*args) == 1, (i, v)
    assert fn(*[ctypes.c_void_p(4100) if i == 0 else a for i, a in enumerate(ok)]) == 1  # descriptors: 16-byte aligned
    assert fn(*[ctypes.c_void_p(4098) if i == 13 else a for i, a in enumerate(ok)]) == 1  # rows: 8-byte aligned
