"""Captured chunks across a reallocation of what they bake in (moondream_amd/graph_store.py): the KV slabs and the
logits buffer grown by a larger batch, and the variant table grown by a longer mixed batch.  Every call under ``compile()``
gives the ids of the same call run eagerly, and no graph captured before the growth is left to be replayed."""
import pytest
import torch

from moondream_amd import synth
from moondream_amd.config import get_config

pytestmark = pytest.mark.gpu
MAX_TOKENS = 6


def build(max_batch):
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config("tiny")
    model = MoondreamModel(cfg, synth.synthetic_state_dict(cfg, seed=1, device="cuda"), device="cuda", tokenizer=IdTokenizer(),
                           max_batch=max_batch)
    cap = list(cfg.tokenizer.templates["caption"]["normal"])
    return model, [synth.synthetic_image(i, 1) for i in range(3)], [cap, model._query_prompts(["5 6 7"])[0], cap]


def run_compiled_then_eager(model, calls):
    """[ids of every call under compile(), in order], [the graph keys stored after each], [ids of the same calls run once
    more, eager]."""
    model.compile()
    try:
        got, keys = [], []
        for call in calls:
            got.append(call())
            keys.append(set(model._graphs))
    finally:
        model.use_graphs = False
    return got, keys, [call() for call in calls]


def test_a_larger_batch_grows_the_slabs_and_the_logits_and_leaves_no_stale_graph():
    model, imgs, prompts = build(max_batch=2)
    gen = lambda b: lambda: model.batch_generate_ids(imgs[:b], prompts[:b], max_tokens=MAX_TOKENS, ignore_eos=True)
    kv, before = model._kv_k, []

    def growing():
        before.append(model._decode_logits(1))  # first: what the first call left, sized for two rows
        return gen(3)()

    got, keys, want = run_compiled_then_eager(model, [gen(2), growing, gen(2)])
    logits = before[0]
    assert logits.shape[0] == 2 and model._decode_logits(1).shape[0] >= 3 and model._decode_logits(1) is not logits
    assert kv.shape[1] == 2 and model._kv_k.shape[1] >= 3
    assert got == want and all(len(ids) == MAX_TOKENS for call in got for ids in call)
    assert keys[0] and not keys[0] & keys[1], "a graph captured before the growth is still stored"
    assert keys[2] > keys[1] and not keys[0] & keys[2]  # the third call captured again, over the new addresses


def test_a_longer_mixed_batch_regrows_the_variant_table():
    model, imgs, prompts = build(max_batch=4)
    model.register_variant("synthetic", synth.synthetic_lora(model.config, seed=1, rank=8, device="cuda"))
    # the table as a first mixed call of two rows would leave it WITHOUT the 64 rows of head room: three rows must regrow it
    small = model._store.grow("variants", 2, lambda: torch.empty(2, dtype=torch.int32, device="cuda"))
    names = ["synthetic", None, "synthetic"]
    gen = lambda b: lambda: model.batch_generate_ids(imgs[:b], prompts[:b], max_tokens=MAX_TOKENS, ignore_eos=True, variants=names[:b])
    tables = []

    def three_rows():
        tables.append(model._store._grown["variants"])  # what the first call used
        return gen(3)()

    got, keys, want = run_compiled_then_eager(model, [gen(2), three_rows, gen(2)])
    assert tables[0] is small and len(model._store._grown["variants"]) >= 3
    assert got == want
    assert keys[0] and not keys[0] & keys[1] and not keys[0] & keys[2]
