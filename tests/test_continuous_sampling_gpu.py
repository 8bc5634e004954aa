"""Per-request sampling settings in the continuous-batching engine on the MI355X: a request's ids are a function of its own
(temperature, top_p, seed) only, one set of captured chunks serves every mix of settings, and engine-wide settings still
give what they gave.  All comparisons are exact; the yardstick is the engine built with one engine-wide pair, running
each request alone."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from moondream_amd import synth
from moondream_amd.config import get_config
from moondream_amd.continuous import MAX_GRAPHS, ContinuousEngine

pytestmark = pytest.mark.gpu

MAX_TOKENS = [12, 5, 9, 12, 3, 7, 12, 2]
CYCLE = [(0.0, 0.3), (0.5, 0.3), (4.0, 0.999), (1.0, 0.8)]  # (temperature, top_p); the first is greedy
SETTINGS = [CYCLE[i % 4] for i in range(8)]
SEEDS = [100 + i for i in range(8)]
HOT = [i for i in range(8) if SETTINGS[i][0] == 4.0]


def load_golden(golden_dir, name):
    path = os.path.join(golden_dir, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not generated")
    return np.load(path)


def build(cfg_name, seed, max_batch=4):
    from moondream_amd.moondream import MoondreamModel, IdTokenizer

    cfg = get_config(cfg_name)
    sd = synth.synthetic_state_dict(cfg, seed=seed, device="cuda")
    return cfg, sd, MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=max_batch)


def golden_image(g, idx, kind="cap"):
    src = int(g["image_index"][idx])
    arr = synth.synthetic_image_array(src, int(g["seed"]), tuple(g[f"img{idx}.{kind}.size"]))
    return Image.fromarray(arr, "RGB")


@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = load_golden(golden_dir, "tiny_seed1.npz")
    cfg, sd, model = build("tiny", int(g["seed"]), max_batch=8)
    return g, cfg, sd, model


@pytest.fixture(scope="module")
def work(tiny):
    g, cfg, sd, model = tiny
    return [golden_image(g, i % 3) for i in range(8)], g["img0.cap.prompt"].tolist()


def mixed_run(model, work, settings=SETTINGS, seeds=SEEDS):
    images, pr = work
    eng = ContinuousEngine(model, max_live=8, chunk=4)
    ids = eng.generate(images, [pr] * 8, max_tokens=MAX_TOKENS, ignore_eos=True, seeds=seeds,
                       temperature=[s[0] for s in settings], top_p=[s[1] for s in settings])
    return ids, eng


@pytest.fixture(scope="module")
def alone(tiny, work):
    """Request i alone on an engine built with its (temperature, top_p) engine-wide, eager: computed once."""
    g, cfg, sd, model = tiny
    images, pr = work
    assert not model.use_graphs
    out = []
    for i in range(8):
        t, p = SETTINGS[i]
        eng = ContinuousEngine(model, max_live=8, chunk=4, temperature=t, top_p=p)
        out.append(eng.generate(images[i : i + 1], [pr], max_tokens=MAX_TOKENS[i], ignore_eos=True, seeds=[SEEDS[i]])[0])
    return out


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_a_requests_ids_depend_on_its_own_settings_only(tiny, work, alone, use_graphs):
    g, cfg, sd, model = tiny
    model.use_graphs = use_graphs
    try:
        got, eng = mixed_run(model, work)
        other, _ = mixed_run(model, work, seeds=[s + 100 for s in SEEDS])
    finally:
        model.use_graphs = False
    for i in range(8):
        assert got[i] == alone[i] and len(got[i]) == MAX_TOKENS[i], (i, SETTINGS[i], got[i], alone[i])
    greedy = [i for i in range(8) if SETTINGS[i][0] == 0]
    for i in greedy:  # a greedy request ignores its seed
        assert other[i] == got[i], i
    assert any(other[i] != got[i] for i in HOT), "the T = 4 rows do not depend on the seed: nothing was sampled"
    if use_graphs:
        assert eng.stats.graph_captures <= MAX_GRAPHS


def test_one_set_of_graphs_for_every_mix(golden_dir, work):
    """The second mix has other values in every sampled request and the same shapes: it replays the first one's chunks
    (no capture), and still reads its own settings (its ids are those of an eager run)."""
    g = load_golden(golden_dir, "tiny_seed1.npz")
    cfg, sd, model = build("tiny", int(g["seed"]), max_batch=8)  # its own model: the captures are counted from none
    swap = {0.5: (2.0, 0.9), 4.0: (0.7, 0.5), 1.0: (3.0, 0.95)}
    second = [s if s[0] == 0 else swap[s[0]] for s in SETTINGS]
    eager_second, _ = mixed_run(model, work, settings=second)
    model.use_graphs = True
    try:
        ids1, e1 = mixed_run(model, work)
        n_keys = sum(1 for k in model._graphs if isinstance(k, tuple) and k and k[0] == "continuous")
        ids2, e2 = mixed_run(model, work, settings=second)
    finally:
        model.use_graphs = False
    assert 0 < e1.stats.graph_captures <= MAX_GRAPHS
    assert e2.stats.graph_captures == 0
    keys = [k for k in model._graphs if isinstance(k, tuple) and k and k[0] == "continuous"]
    assert len(keys) == n_keys <= MAX_GRAPHS
    assert ids2 == eager_second
    assert any(ids1[i] != ids2[i] for i in range(8) if SETTINGS[i][0] != 0)  # (the settings do reach the replayed kernel)


def test_engine_wide_settings_give_what_per_request_settings_give(tiny, work):
    """Old callers: an engine built with (4.0, 0.999) and no per-request arguments == every request submitted with those
    settings to an engine built with the defaults, seed for seed."""
    g, cfg, sd, model = tiny
    images, pr = work
    old = ContinuousEngine(model, max_live=8, chunk=4, temperature=4.0, top_p=0.999)
    want = old.generate(images, [pr] * 8, max_tokens=MAX_TOKENS, ignore_eos=True, seeds=SEEDS)
    new = ContinuousEngine(model, max_live=8, chunk=4)
    rids = [new.submit(images[i], pr, max_tokens=MAX_TOKENS[i], ignore_eos=True, seed=SEEDS[i], temperature=4.0, top_p=0.999)
            for i in range(8)]
    got = dict(new.run())
    assert [got[r] for r in rids] == want
    assert [len(x) for x in want] == MAX_TOKENS
    greedy = ContinuousEngine(model, max_live=8, chunk=4).generate(images, [pr] * 8, max_tokens=MAX_TOKENS, ignore_eos=True)
    assert want != greedy  # (at T = 4 the draws leave the argmax)
