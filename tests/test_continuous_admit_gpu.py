"""The launches of one ``ContinuousEngine`` admission, against values written out by hand from its rules: which decoder
passes it makes (rows, length, position, kept rows, entry point, slot table), where EncodedImages are loaded, in which cuts
lm_head runs, and what a request draws from its generator.  The rules (continuous batching):

* fused (every image raw, ``fused_prefill`` on): per prompt length, in order of first appearance, ONE [bos | image | prompt]
  pass at position 0; no image-only pass;
* two-pass (everything else): one [bos | image] pass over the raw rows, one load per EncodedImage into its request's slot,
  then per (prefix, prompt length) prompt passes of max(1, 64 // t) rows when t <= 64, the whole group otherwise;
* lm_head (and the pick behind it) in contiguous cuts of <= 64 rows of a pass;
* a pass carries the variant table only if one of its rows has a variant;
* a greedy request draws nothing, a sampled one exactly one uniform for its first token."""
import pytest
import torch

from moondream_amd import synth
from moondream_amd.config import get_config
from moondream_amd.continuous import ContinuousEngine

pytestmark = pytest.mark.gpu
PREFIX = 730  # bos + 729 image positions


@pytest.fixture(scope="module")
def model():
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config("tiny")
    sd = synth.synthetic_state_dict(cfg, seed=1, device="cuda")
    return MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=8)


def prompt(n, salt=0):
    return [1 + (7 * i + salt) % 1000 for i in range(n)]


def admit(model, monkeypatch, max_live, requests, **engine_kw):
    """One admission of ``requests`` (dicts of ``submit`` arguments) with the model's decoder pass, lm_head and
    EncodedImage load recorded: returns (engine, requests, what ``_admit`` returned, the log)."""
    log = []
    forward, head, load = model._text_forward, model._lm_head, model.load_encoded_image

    def rec_forward(x, pos0, rows=0, *a, keep="all", **kw):
        log.append(("forward", x.shape[0], x.shape[1], pos0, keep, rows.kind, rows.slots.tolist()))
        return forward(x, pos0, rows, *a, keep=keep, **kw)

    def rec_head(hidden, *a, **kw):
        log.append(("lm_head", hidden.shape[0]))
        return head(hidden, *a, **kw)

    def rec_load(image, slot=0):
        log.append(("load", slot))
        return load(image, slot)

    eng = ContinuousEngine(model, max_live=max_live, **engine_kw)
    for kw in requests:
        eng.submit(**kw)
    reqs = eng.sched.take_admissions()
    assert [r.slot for r in reqs] == list(range(len(requests)))  # a new engine hands out slots 0, 1, ...
    with torch.inference_mode():
        eng._prepare_run()
        monkeypatch.setattr(model, "_text_forward", rec_forward)
        monkeypatch.setattr(model, "_lm_head", rec_head)
        monkeypatch.setattr(model, "load_encoded_image", rec_load)
        out = eng._admit(reqs)
    monkeypatch.undo()
    return eng, reqs, out, log


def test_fused_one_pass_per_prompt_length(model, monkeypatch):
    lens = [3, 5, 3, 5, 3]
    reqs = [dict(image=synth.synthetic_image(i, 1), prompt_ids=prompt(n, i)) for i, n in enumerate(lens)]
    eng, _, out, log = admit(model, monkeypatch, 8, reqs)
    assert log == [
        ("forward", 3, PREFIX + 3, 0, "last", "_slots", [0, 2, 4]), ("lm_head", 3),
        ("forward", 2, PREFIX + 5, 0, "last", "_slots", [1, 3]), ("lm_head", 2),
    ]
    assert [o[1] for o in out] == [PREFIX + n for n in lens]
    assert eng.stats.prefill_passes == 2


def test_two_pass_short_prompt_in_launches_of_64_rows(model, monkeypatch):
    enc = model.encode_image(synth.synthetic_image(0, 1))
    assert enc.pos == PREFIX
    eng, _, out, log = admit(model, monkeypatch, 70, [dict(image=enc, prompt_ids=prompt(3, i)) for i in range(70)])
    want = [("load", s) for s in range(70)]
    for s0, s1 in ((0, 21), (21, 42), (42, 63), (63, 70)):  # 64 // 3 = 21 rows per launch
        want += [("forward", s1 - s0, 3, PREFIX, "last", "_slots", list(range(s0, s1))), ("lm_head", s1 - s0)]
    assert log == want
    assert [o[1] for o in out] == [PREFIX + 3] * 70
    assert eng.stats.prefill_passes == 4


def test_two_pass_long_prompt_one_pass_lm_head_in_cuts_of_64(model, monkeypatch):
    enc = model.encode_image(synth.synthetic_image(0, 1))
    eng, _, out, log = admit(model, monkeypatch, 70, [dict(image=enc, prompt_ids=prompt(70, i)) for i in range(70)])
    assert log == [("load", s) for s in range(70)] + [
        ("forward", 70, 70, PREFIX, "last", "_slots", list(range(70))), ("lm_head", 64), ("lm_head", 6)]
    assert [o[1] for o in out] == [PREFIX + 70] * 70
    assert eng.stats.prefill_passes == 1


def test_mixed_images_take_two_passes(model, monkeypatch):
    assert model.fused_prefill
    enc = [model.encode_image(synth.synthetic_image(i, 1)) for i in (2, 3)]
    images = [synth.synthetic_image(0, 1), synth.synthetic_image(1, 1)] + enc
    lens = [4, 4, 4, 6]
    eng, _, out, log = admit(model, monkeypatch, 8, [dict(image=im, prompt_ids=prompt(n, i))
                                                     for i, (im, n) in enumerate(zip(images, lens))])
    assert log == [
        ("forward", 2, PREFIX, 0, "none", "_slots", [0, 1]), ("load", 2), ("load", 3),
        ("forward", 3, 4, PREFIX, "last", "_slots", [0, 1, 2]), ("lm_head", 3),
        ("forward", 1, 6, PREFIX, "last", "_slots", [3]), ("lm_head", 1),
    ]
    assert [o[1] for o in out] == [PREFIX + n for n in lens]
    assert eng.stats.prefill_passes == 3


def test_variant_table_only_on_passes_with_a_lora_row(model, monkeypatch):
    model.register_variant("admit", synth.synthetic_lora(model.config, seed=1, rank=8, device="cuda"))
    lens, variants = [3, 3, 5, 5], ["admit", None, None, None]
    reqs = [dict(image=synth.synthetic_image(i, 1), prompt_ids=prompt(n, i), variant=v)
            for i, (n, v) in enumerate(zip(lens, variants))]
    eng, _, _, log = admit(model, monkeypatch, 8, reqs)
    assert log == [
        ("forward", 2, PREFIX + 3, 0, "last", "_multi_lora", [0, 1]), ("lm_head", 2),
        ("forward", 2, PREFIX + 5, 0, "last", "_slots", [2, 3]), ("lm_head", 2),
    ]
    assert eng.stats.prefill_passes == 2


def test_a_sampled_request_draws_one_uniform_a_greedy_one_none(model, monkeypatch):
    reqs = [dict(image=synth.synthetic_image(0, 1), prompt_ids=prompt(4), seed=5, temperature=0.7, top_p=0.9),
            dict(image=synth.synthetic_image(1, 1), prompt_ids=prompt(4, 1), seed=9)]
    _, (sampled, greedy), _, log = admit(model, monkeypatch, 8, reqs)
    assert log == [("forward", 2, PREFIX + 4, 0, "last", "_slots", [0, 1]), ("lm_head", 2)]
    fresh = torch.Generator().manual_seed(5)
    torch.rand(1, dtype=torch.float32, generator=fresh)  # the first token's draw
    assert torch.equal(torch.rand(4, generator=sampled.generator), torch.rand(4, generator=fresh))
    assert greedy.generator is None
