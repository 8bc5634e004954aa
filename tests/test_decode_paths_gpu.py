"""Every path through the generation layer's decode loops against what the commit before the decode-chunk runner
computed: tests/golden/decode_paths_tiny.json holds the ids, ranks (ints) and log-probabilities (raw fp32 words) of the
tiny synthetic model over lockstep greedy / sampled / shared-prefix / LoRA / mixed-variant / single-sequence decoding,
the continuous engine and the streaming ``query``, eager and from captured graphs.  The comparison is exact.

Run as a script, this file is the recorder: ``python tests/test_decode_paths_gpu.py [OUT.json]`` writes the fixture from
the checkout it runs in.  It refuses to write unless at least half of the tokens sampled at the hot setting differ from
the greedy ids of the same rows (otherwise the recording would not see the random stream)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from moondream_amd import synth  # noqa: E402
from moondream_amd.config import get_config  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(REPO, "tests", "golden", "decode_paths_tiny.json")
MAX_TOKENS = 12
MILD = (0.5, 0.3)
HOT_TOP_P = 0.999
HOT_TEMPERATURES = (4.0, 8.0, 16.0)  # the recorder takes the first at which the hot recordings see the random stream
MIN_HOT_SHARE = 0.5


def words(logprobs):
    return [np.asarray(row, dtype=np.float32).view(np.uint32).tolist() for row in logprobs]


def with_logprobs(out):
    ids, lp, rk = out
    return {"ids": ids, "logprob_words": words(lp), "ranks": rk}


def run_paths(hot_temperature):
    """name -> recorded value of every path, in one fixed order on one model; ``hot[name]`` = (sampled ids, greedy ids of
    the same rows) for the recordings at the hot setting."""
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config("tiny")
    sd = synth.synthetic_state_dict(cfg, seed=1, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=8)
    model.register_variant("synthetic", synth.synthetic_lora(cfg, seed=1, rank=8, device="cuda"))
    imgs = [synth.synthetic_image(i, 1) for i in range(3)]
    cap = list(cfg.tokenizer.templates["caption"]["normal"])
    prompts = [cap, model._query_prompts(["5 6 7"])[0], cap]  # two lengths
    assert len({len(p) for p in prompts}) == 2
    repeated = [imgs[0], imgs[1], imgs[0]]  # share_prefix: rows 0 and 2 read one prefix
    hot_setting = (hot_temperature, HOT_TOP_P)
    rec, hot = {}, {}

    def gen(seed):
        return torch.Generator(device="cuda").manual_seed(seed)

    def modes():
        """(name, runs) per launch mode: eager once; with graphs twice -- the capture, then one replay."""
        try:
            for name, graphs, runs in (("eager", False, 1), ("graphs", True, 2)):
                model.use_graphs = graphs
                model._graphs.clear()
                for k in range(runs):
                    yield name if runs == 1 else f"{name}{k}"
        finally:
            model.use_graphs = False
            model._graphs.clear()

    for mode in modes():
        greedy = model.batch_generate_ids(imgs, prompts, max_tokens=MAX_TOKENS)
        rec[f"greedy.{mode}"] = greedy
        greedy_shared = model.batch_generate_ids(repeated, prompts, max_tokens=MAX_TOKENS, share_prefix=True)
        rec[f"greedy_shared.{mode}"] = greedy_shared
        for tag, (temp, top_p) in (("mild", MILD), ("hot", hot_setting)):
            got = model.batch_generate_ids(imgs, prompts, max_tokens=MAX_TOKENS, temperature=temp, top_p=top_p, generator=gen(7))
            rec[f"sampled_{tag}.{mode}"] = got
            shared = model.batch_generate_ids(repeated, prompts, max_tokens=MAX_TOKENS, temperature=temp, top_p=top_p,
                                              generator=gen(8), share_prefix=True)
            rec[f"sampled_shared_{tag}.{mode}"] = shared
            if tag == "hot":
                hot[f"sampled_hot.{mode}"] = (got, greedy)
                hot[f"sampled_shared_hot.{mode}"] = (shared, greedy_shared)
        rec[f"variants.{mode}"] = model.batch_generate_ids(imgs, prompts, max_tokens=MAX_TOKENS, variants=["synthetic", None, "synthetic"])
        model.single_sequence_kernel = True
        rec[f"single.{mode}"] = with_logprobs(model.batch_generate_ids(imgs[:1], prompts[:1], max_tokens=MAX_TOKENS, return_logprobs=True))
        rec[f"single.{mode}"]["persistent_kernel"] = bool(model._b1_used)
        cont_greedy = model.batch_generate_ids_continuous(imgs, prompts, max_tokens=MAX_TOKENS, max_live=2, chunk=4)
        rec[f"continuous_greedy.{mode}"] = cont_greedy
        cont = model.batch_generate_ids_continuous(imgs, prompts, max_tokens=MAX_TOKENS, max_live=2, chunk=4,
                                                   temperature=[0.0, MILD[0], hot_temperature], top_p=[0.3, MILD[1], HOT_TOP_P],
                                                   seeds=[1, 2, 3], return_logprobs=True)
        rec[f"continuous.{mode}"] = with_logprobs(cont)
        hot[f"continuous.{mode}"] = (cont[0][2:], cont_greedy[2:])

    # a LoRA ``variant=``: the eager loop from the step's pieces, greedy and sampled, with log-probabilities
    lora_greedy = model.batch_generate_ids(imgs, prompts, max_tokens=MAX_TOKENS, variant="synthetic", return_logprobs=True)
    rec["lora_greedy"] = with_logprobs(lora_greedy)
    for tag, (temp, top_p) in (("mild", MILD), ("hot", hot_setting)):
        got = model.batch_generate_ids(imgs, prompts, max_tokens=MAX_TOKENS, variant="synthetic", temperature=temp, top_p=top_p,
                                       generator=gen(9), return_logprobs=True)
        rec[f"lora_sampled_{tag}"] = with_logprobs(got)
        if tag == "hot":
            hot["lora_sampled_hot"] = (got[0], lora_greedy[0])

    # the sequential API: streaming pieces of a sampled answer (its draws come from the device's default generator)
    torch.manual_seed(11)
    pieces = model.query(imgs[0], "5 6 7", reasoning=False, stream=True, settings={"temperature": MILD[0], "max_tokens": MAX_TOKENS})["answer"]
    rec["query_stream"] = "".join(pieces)
    return rec, hot


def hot_share(hot):
    """Per hot recording, the share of sampled tokens that differ from the greedy id at their place."""
    shares = {}
    for name, (sampled, greedy) in hot.items():
        pairs = [(s, g) for srow, grow in zip(sampled, greedy) for s, g in zip(srow, grow)]
        assert pairs, name
        shares[name] = sum(s != g for s, g in pairs) / len(pairs)
    return shares


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed(fixture):
    return run_paths(fixture["hot_temperature"])


def test_every_recorded_path_is_reproduced_exactly(fixture, computed):
    rec, _ = computed
    want = fixture["paths"]
    assert sorted(rec) == sorted(want)
    wrong = [name for name in sorted(want) if rec[name] != want[name]]
    assert not wrong, {name: (rec[name], want[name]) for name in wrong[:2]}


def main(out):
    for temp in HOT_TEMPERATURES:
        rec, hot = run_paths(temp)
        shares = hot_share(hot)
        print(f"hot temperature {temp}: differing share per recording {shares}", flush=True)
        if min(shares.values()) >= MIN_HOT_SHARE:
            break
    else:
        raise SystemExit("no hot temperature at which half of the sampled tokens differ from the greedy ids: nothing written")
    rec = json.loads(json.dumps(rec))  # (what a reader of the file gets back)
    with open(out, "w") as f:  # one path per line
        f.write('{"hot_temperature": %s, "paths": {\n' % json.dumps(temp))
        f.write(",\n".join(f"{json.dumps(name)}: {json.dumps(rec[name], separators=(',', ':'))}" for name in sorted(rec)))
        f.write("\n}}\n")
    print(f"wrote {out}: {len(rec)} paths, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
