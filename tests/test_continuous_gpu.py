"""Continuous batching on the MI355X: the slot-table entry points give the bits of the contiguous ones, and the engine's ids
equal the lockstep path's (and the reference goldens) while requests leave and join mid-decode."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

from moondream_amd import _lib, synth
from moondream_amd.config import get_config
from moondream_amd.continuous import MAX_GRAPHS, ContinuousEngine, Request, SlotScheduler

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


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


# ------------------------------------------------------------------ library: md_text_forward_slots
class Slab:
    """K / V slabs [L][n_slots][H][ctx][64] (+ the e4m3 copy with fixed per-layer scales) and their md_kv_cache."""

    def __init__(self, cfg, n_slots, kv8):
        t = cfg.text
        self.k = torch.zeros(t.n_layers, n_slots, t.n_kv_heads, t.max_context, t.head_dim, dtype=BF16, device="cuda")
        self.v = torch.zeros_like(self.k)
        bs = t.n_kv_heads * t.max_context * t.head_dim
        self.kv = _lib.MdKvCache(self.k.data_ptr(), self.v.data_ptr(), n_slots * bs, bs, t.max_context)
        self.k8 = self.v8 = None
        if kv8:
            self.k8 = torch.zeros(self.k.shape, dtype=torch.uint8, device="cuda")
            self.v8 = torch.zeros_like(self.k8)
            self.scales = ((C.c_float * t.n_layers)(*[0.02] * t.n_layers), (C.c_float * t.n_layers)(*[0.03] * t.n_layers))
            self.kv.k8, self.kv.v8 = self.k8.data_ptr(), self.v8.data_ptr()
            self.kv.k_scale = C.cast(self.scales[0], C.c_void_p)
            self.kv.v_scale = C.cast(self.scales[1], C.c_void_p)

    def tensors(self):
        return [x for x in (self.k, self.v, self.k8, self.v8) if x is not None]


def forward(model, slab, x, pos0, slots=None):
    lib, text = model.lib, model.w.text
    b, t, _ = x.shape
    hidden = torch.empty_like(x)
    pos = torch.full((b,), pos0, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.md_text_workspace_bytes(C.byref(text), b, t), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if slots is None:
        st = lib.md_text_forward(C.byref(text), x.data_ptr(), hidden.data_ptr(), b, t, pos.data_ptr(), C.byref(slab.kv),
                                 ws.data_ptr(), ws.numel(), stream)
    else:
        sl = torch.tensor(slots, dtype=torch.int32, device="cuda")
        st = lib.md_text_forward_slots(C.byref(text), x.data_ptr(), hidden.data_ptr(), b, t, pos.data_ptr(), sl.data_ptr(),
                                       slab.k.shape[1], C.byref(slab.kv), ws.data_ptr(), ws.numel(), stream)
    _lib.check(st, "forward")
    torch.cuda.synchronize()
    return hidden


def rand_x(b, t, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, t, d, generator=g) * 0.5).to(BF16).cuda()


def assert_slabs_permuted(ref, perm, slots):
    used = set(slots)
    for a, b in zip(ref.tensors(), perm.tensors()):
        assert torch.equal(b[:, list(slots)], a), "K / V rows in the permuted slots differ from the contiguous ones"
        rest = [s for s in range(b.shape[1]) if s not in used]
        assert not b[:, rest].any(), "a slot outside the table was written"


def check_permuted(model, cfg, batch, n_slots, slots, prefill_len, kv8):
    """Prefill (prefill_len rows at position 0), a 5-token prompt pass and a decode step: hidden states and every K / V
    row (and e4m3 row) of the slot-table call equal the contiguous call's, bit for bit."""
    model._select_kernels(2)
    d = cfg.text.dim
    ref, perm = Slab(cfg, batch, kv8), Slab(cfg, n_slots, kv8)
    pos = 0
    for t, seed in ((prefill_len, 1), (5, 2), (1, 3)):
        x = rand_x(batch, t, d, seed)
        h_ref = forward(model, ref, x, pos)
        h_perm = forward(model, perm, x, pos, slots)
        assert torch.equal(h_perm, h_ref), f"hidden states differ (q_len {t})"
        assert_slabs_permuted(ref, perm, slots)
        pos += t
    return ref, perm, pos


@pytest.mark.parametrize("kv8", [False, True])
def test_forward_slots_permuted_table_is_bit_identical(tiny, kv8):
    g, cfg, sd, model = tiny
    slots = [5, 2, 7]
    ref, perm, pos = check_permuted(model, cfg, 3, 8, slots, 730, kv8)
    # idle rows: a decode step with slot -1 in row 1 leaves the whole slab as it was outside rows 0 and 2's writes, and
    # rows 0 and 2 get the same outputs as with row 1 live
    x = rand_x(3, 1, cfg.text.dim, 4)
    before = [a.clone() for a in perm.tensors()]
    h_full = forward(model, perm, x, pos, slots)
    full = [a.clone() for a in perm.tensors()]
    for a, b in zip(perm.tensors(), before):
        a.copy_(b)
    h_idle = forward(model, perm, x, pos, [5, -1, 7])
    assert torch.equal(h_idle[0], h_full[0]) and torch.equal(h_idle[2], h_full[2])
    for a, f, b in zip(perm.tensors(), full, before):
        assert torch.equal(a[:, [5, 7]], f[:, [5, 7]])
        others = [s for s in range(8) if s not in (5, 7)]
        assert torch.equal(a[:, others], b[:, others]), "an idle row touched the slab"


@pytest.mark.parametrize("kv8", [False, True])
def test_forward_slots_decode_step_over_more_than_128_rows(tiny, kv8):
    """The block split of a decode step (128-row tall pass + rest; 64-row blocks with the e4m3 copy) advances the slot
    table, not the slab base."""
    g, cfg, sd, model = tiny
    rng = np.random.default_rng(7)
    slots = [int(s) for s in rng.permutation(140)[:132]]
    check_permuted(model, cfg, 132, 140, slots, 8, kv8)


# ------------------------------------------------------------------ engine
def twelve_requests(g, rng, n):
    images = [golden_image(g, i % 3) for i in range(12)]
    base = [g[f"img{i % 3}.cap.prompt"].tolist() for i in range(12)]
    prompts = [p if i % 2 == 0 else p + p[:2] for i, p in enumerate(base)]  # two prompt lengths
    mt = [int(x) for x in rng.integers(2, n + 1, 12)]
    return images, prompts, mt


def test_engine_equals_lockstep_and_reference(tiny):
    g, cfg, sd, model = tiny
    n = len(g["img0.cap.tokens"])
    images, prompts, mt = twelve_requests(g, np.random.default_rng(1), n)
    lock = model.batch_generate_ids(images, prompts, max_tokens=max(mt))
    eng = ContinuousEngine(model, max_live=4, chunk=4)
    got = eng.generate(images, prompts, max_tokens=mt)
    for i in range(12):
        assert got[i] == lock[i][: mt[i]], (i, got[i], lock[i][: mt[i]])
        if i % 2 == 0:  # the caption prompt: the reference's ids
            assert got[i] == g[f"img{i % 3}.cap.tokens"].tolist()[: mt[i]], i
    assert eng.stats.admissions > 1
    # the model-level wrapper
    assert model.batch_generate_ids_continuous(images, prompts, max_tokens=mt, max_live=4, chunk=4) == got


def predicted_stats(streams, mt, eos, pos, max_live, chunk, max_context):
    """SlotScheduler over known token streams (streams[i][k]: token k of request i, k = 0 the prefill's pick)."""
    sched = SlotScheduler(max_live, max_context, chunk)
    for i in range(len(streams)):
        sched.submit(Request(i, None, [0], mt[i], eos[i]))

    def admit(reqs):
        return [(streams[r.rid][0], pos[r.rid]) for r in reqs]

    def step(plan):
        out = np.zeros((plan.n, plan.bucket), dtype=np.int32)
        for j, r in enumerate(plan.rows):
            for i in range(plan.n):
                k = r.steps + i + 1
                out[i, j] = streams[r.rid][k] if k < len(streams[r.rid]) else 0
        return out

    done = {r.rid: r.ids for r in sched.run(admit, step)}
    return sched.stats, [done[i] for i in range(len(streams))]


def test_engine_eos_exit_per_request(tiny):
    g, cfg, sd, model = tiny
    n = len(g["img0.cap.tokens"])
    images = [golden_image(g, i % 3) for i in range(6)]
    prompts = [g[f"img{i % 3}.cap.prompt"].tolist() for i in range(6)]
    gold = [g[f"img{i % 3}.cap.tokens"].tolist() for i in range(6)]
    ks = [1, 3, 6, 10, 15, 0]
    eos = [gold[i][ks[i]] for i in range(6)]
    eng = ContinuousEngine(model, max_live=3, chunk=4)
    rids = [eng.submit(images[i], prompts[i], max_tokens=n, eos_id=eos[i]) for i in range(6)]
    got = dict(eng.run())
    for i in range(6):
        want = model.batch_generate_ids(images, prompts, max_tokens=n, eos_id=eos[i])[i]
        assert got[rids[i]] == want, (i, got[rids[i]], want)
        assert want == gold[i][: gold[i].index(eos[i])]
    pos = [730 + len(p) for p in prompts]
    stats, ids = predicted_stats(gold, [n] * 6, eos, pos, 3, 4, cfg.text.max_context)
    assert ids == [got[r] for r in rids]
    assert (eng.stats.decode_steps, eng.stats.padded_row_steps, eng.stats.live_row_steps) == \
        (stats.decode_steps, stats.padded_row_steps, stats.live_row_steps)


def test_engine_graph_replay_equals_eager(tiny):
    g, cfg, sd, model = tiny
    n = len(g["img0.cap.tokens"])
    images, prompts, mt = twelve_requests(g, np.random.default_rng(2), n)
    eager = ContinuousEngine(model, max_live=4, chunk=4).generate(images, prompts, max_tokens=mt)
    model.compile()
    try:
        e1 = ContinuousEngine(model, max_live=4, chunk=4)
        first = e1.generate(images, prompts, max_tokens=mt)
        e2 = ContinuousEngine(model, max_live=4, chunk=4)
        second = e2.generate(images, prompts, max_tokens=mt)
    finally:
        model.use_graphs = False
    assert first == eager and second == eager
    assert 0 < e1.stats.graph_captures <= MAX_GRAPHS and e2.stats.graph_captures == 0
    assert sum(1 for k in model._graphs if isinstance(k, tuple) and k[0] == "continuous") <= MAX_GRAPHS


@pytest.mark.parametrize("temperature,top_p", [(0.5, 0.3), (4.0, 0.999)])
def test_engine_sampling_does_not_depend_on_the_mix(tiny, temperature, top_p):
    """A seeded request draws the same ids alone and mixed with 7 others.  (The conditioned checkpoint's margins make the
    reference's default settings all but greedy; at T = 4, top_p = 0.999 the draws really vary.)"""
    g, cfg, sd, model = tiny
    images = [golden_image(g, i % 3) for i in range(8)]
    pr = g["img0.cap.prompt"].tolist()
    eng = ContinuousEngine(model, max_live=8, chunk=4, temperature=temperature, top_p=top_p)
    alone = eng.generate(images[:1], [pr], max_tokens=12, ignore_eos=True, seeds=[1234])[0]
    mixed = eng.generate(images, [pr] * 8, max_tokens=[12, 5, 9, 12, 3, 7, 12, 2], ignore_eos=True,
                         seeds=[1234, 1, 2, 3, 4, 5, 6, 7])[0]
    assert alone == mixed and len(alone) == 12
    if temperature > 1:
        others = [eng.generate(images[:1], [pr], max_tokens=12, ignore_eos=True, seeds=[s])[0] for s in (99, 100, 101)]
        assert any(o != alone for o in others)  # (the draws do depend on the seed)


def test_engine_row_steps_below_lockstep(tiny):
    g, cfg, sd, model = tiny
    images = [golden_image(g, i % 3) for i in range(16)]
    pr = g["img0.cap.prompt"].tolist()
    mt = [int(x) for x in np.random.default_rng(3).integers(2, 24, 16)]
    eng = ContinuousEngine(model, max_live=8, chunk=4)
    eng.generate(images, [pr] * 16, max_tokens=mt, ignore_eos=True)
    streams = [[1] * 64] * 16  # without EOS the schedule depends on the lengths only
    stats, _ = predicted_stats(streams, mt, [None] * 16, [730 + len(pr)] * 16, 8, 4, cfg.text.max_context)
    assert eng.stats.padded_row_steps == stats.padded_row_steps and eng.stats.live_row_steps == stats.live_row_steps
    lockstep = 16 * max(mt)
    assert eng.stats.padded_row_steps < lockstep
    assert eng.stats.live_row_steps == sum(x - 1 for x in mt)


def test_engine_2b_ragged_bench_images_vs_reference(golden_dir):
    gb = load_golden(golden_dir, "md2b_bench64.npz")
    cfg, sd, model = build("2b", int(gb["seed"]), max_batch=32)
    imgs = [synth.synthetic_image(i, int(gb["seed"])) for i in range(64)]
    pr = gb["prompt"].tolist()
    ref = gb["tokens"].tolist()
    mt = [int(x) for x in np.random.default_rng(4).integers(1, 33, 64)]
    eng = ContinuousEngine(model, max_live=32, chunk=16)
    got = eng.generate(imgs, [pr] * 64, max_tokens=mt, ignore_eos=True)
    bad = [i for i in range(64) if got[i] != ref[i][: mt[i]]]
    assert not bad, (bad[:5], [(got[i], ref[i][: mt[i]]) for i in bad[:2]])
    assert eng.stats.admissions > 1
