"""The decoding settings end to end on the tiny model (4 rows of two prompt lengths, 12 tokens, ``ignore_eos``), against
values recorded on the commit before the settings travelled as one record (tests/golden/settings_record.json): the
lockstep call greedy and sampled, the continuous engine with refilled slots, and the string API.  The device code is the
same, so nothing is compared with a tolerance: ids and ranks are equal, log-probabilities and alternatives are equal as
float32 bit patterns."""
import json
import os

import numpy as np
import pytest
import torch

from moondream_amd import synth
from moondream_amd.config import get_config
from PIL import Image

pytestmark = pytest.mark.gpu
N = 12
HOT = dict(temperature=4.0, top_p=0.999)
REPETITION = [1.0, 1.3, 1.0, 1.1]  # row 0 (and 2) neutral
PRESENCE = [0.0, 0.5, 0.0, 0.0]
FREQUENCY = [0.0, 0.0, 0.0, 0.25]
TOP_K = [0, 3, 2, 5]               # row 0 neutral
MIN_P = [0.0, 0.0, 0.0, 0.2]
CASES = ("lockstep_greedy", "lockstep_sampled", "continuous", "string_greedy", "string_sampled", "query_many")


class Tiny:
    pass


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def bits(x):
    """A nested list of results with every float replaced by its float32 bit pattern (ints stay)."""
    if isinstance(x, float):
        return int(np.asarray(x, dtype=np.float32).view(np.int32))
    if isinstance(x, (list, tuple)):
        return [bits(v) for v in x]
    return x


def build_tiny(golden_dir):
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    t = Tiny()
    g = np.load(os.path.join(golden_dir, "tiny_seed1.npz"))
    t.cfg = get_config("tiny")
    sd = synth.synthetic_state_dict(t.cfg, seed=int(g["seed"]), device="cuda")
    t.model = MoondreamModel(t.cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=8)
    image = lambda i: Image.fromarray(synth.synthetic_image_array(int(g["image_index"][i]), int(g["seed"]), tuple(g[f"img{i}.cap.size"])), "RGB")
    imgs = [image(i) for i in range(3)]
    t.images = imgs + imgs[:1]  # rows 0 and 3: the same image object
    t.prompts = [g[f"img{i}.cap.prompt"].tolist() for i in range(3)] + [[1, 708, 9, 3]]  # two lengths: two prefill groups
    t.kw = dict(max_tokens=N, ignore_eos=True)
    t.choice = t.model.choice_constraint(["10 11 12", "10 11", "20"])
    # ids below 10 are the tokenizer's special ids; every other id spells one byte
    t.vocab = [b""] * 10 + [bytes([i % 256]) for i in range(t.cfg.text.vocab_size - 10)]
    return t


def run_case(t, name):
    m = t.model
    pen = dict(repetition_penalty=REPETITION, presence_penalty=PRESENCE, frequency_penalty=FREQUENCY)
    if name == "lockstep_greedy":
        return bits(m.batch_generate_ids(t.images, t.prompts, **t.kw, **pen, constraints=[None, None, t.choice, None],
                                         return_logprobs=True, top_logprobs=3))
    if name == "lockstep_sampled":
        return bits(m.batch_generate_ids(t.images, t.prompts, **t.kw, **HOT, generator=gen(11), top_k=TOP_K, min_p=MIN_P,
                                         repetition_penalty=[1.0, 1.0, 1.0, 1.4], share_prefix=True))
    if name == "continuous":
        return bits(m.batch_generate_ids_continuous(
            t.images, t.prompts, **t.kw, max_live=2, chunk=4, temperature=[0.0, 4.0, 4.0, 4.0], top_p=[0.3, 0.999, 0.999, 0.999],
            seeds=[21, 22, 23, 24], return_logprobs=True, top_logprobs=3, **pen, constraints=[t.choice, None, None, None],
            top_k=TOP_K, min_p=MIN_P))
    st = {"max_tokens": N, "repetition_penalty": 1.3, "frequency_penalty": 0.25, "top_k": 3, "regex": "[0-9a-f]{2,9}",
          "vocab_bytes": t.vocab}
    if name in ("string_greedy", "string_sampled"):
        st.update({"temperature": 0} if name == "string_greedy" else HOT)
        torch.manual_seed(5)
        out = [m.query(t.images[0], "5", settings=st)["answer"], m.caption(t.images[1], settings=st)["caption"]]
        return out + [m.batch_query(t.images[:2], ["5", "6 7"], settings=st)]
    if name == "query_many":
        st = {"max_tokens": N, **HOT, "generator": gen(7), "repetition_penalty": REPETITION[:3], "presence_penalty": 0.5,
              "top_k": TOP_K[:3], "min_p": [0.0, 0.1, 0.0]}
        return m.query_many(t.images[0], ["5", "6 7", "8"], settings=st)
    raise KeyError(name)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    assert torch.cuda.is_available(), "GPU tests need a device"
    t = build_tiny(golden_dir)
    with open(os.path.join(golden_dir, "settings_record.json")) as f:
        t.golden = json.load(f)
    return t


@pytest.mark.parametrize("compiled", [False, True], ids=["eager", "compiled"])
@pytest.mark.parametrize("name", CASES)
def test_the_recorded_values(tiny, name, compiled):
    m = tiny.model
    if compiled:
        m.compile()
    try:
        got = run_case(tiny, name)
    finally:
        m.use_graphs = False
        m._graphs.clear()
    assert json.loads(json.dumps(got)) == tiny.golden[name]
