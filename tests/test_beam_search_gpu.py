"""Beam search end to end on the tiny model under ``set_strict_batch_invariance`` (3 requests, W = 3, 6 tokens).

Exact replay: the test runs its own beam search on the host with tests/beam_ref.py's rules.  At each step every live
hypothesis's logits row comes from ``teacher_forced_logits`` over the whole vocabulary -- the batched decode step on a
private KV that is never reordered -- goes back to the device as bf16 and gives its candidates through
``model._topk_logprobs``.  ``batch_beam_search_ids`` must return the same ids, logprob and score bit for bit: a beam that
read a wrong tail, or a one-position error in the copied range, changes a later row's logits."""
import os

import numpy as np
import pytest
import torch

import beam_ref as ref
from moondream_amd import synth
from moondream_amd.config import get_config
from PIL import Image

pytestmark = pytest.mark.gpu
W, N = 3, 6


class Tiny:
    pass


def golden_image(g, idx, kind="cap"):
    src = int(g["image_index"][idx])
    arr = synth.synthetic_image_array(src, int(g["seed"]), tuple(g[f"img{idx}.{kind}.size"]))
    return Image.fromarray(arr, "RGB")


def host_beam_search(model, images, prompts, w, max_tokens, eos, length_penalty, early, n_ret):
    """The oracle: beam_ref's rules over logits rows that never saw a reordered cache."""
    cfg = model.config
    r_n, v = len(images), cfg.text.vocab_size
    norm = ref.inv_norm_table(cfg.text.max_context + 2, length_penalty)
    state = ref.new_state(r_n, w, [0] * r_n)
    hyps = [[[] for _ in range(w)] for _ in range(r_n)]
    tok_planes, par_planes, out = [], [], None
    for t in range(max_tokens):
        beams_in = 1 if t == 0 else w
        live = [(g, j) for g in range(r_n) for j in range(beams_in) if not state["done"][g] and state["cum"][g * w + j] != ref.NEG_INF]
        if not live:
            break
        forced = np.asarray([hyps[g][j] for g, j in live], dtype=np.int32).reshape(len(live), t)
        idx = np.broadcast_to(np.arange(v, dtype=np.int64), (len(live), t + 1, v)).copy()
        vals = model.teacher_forced_logits([images[g] for g, _ in live], [prompts[g] for g, _ in live], forced, idx)
        rows = vals[:, t].to(torch.bfloat16).cuda().contiguous()
        top_ids = torch.zeros(len(live), 2 * w, dtype=torch.int32, device="cuda")
        top_lp = torch.zeros(len(live), 2 * w, dtype=torch.float32, device="cuda")
        with torch.inference_mode():
            model._topk_logprobs(rows, None, -1 if t == 0 else cfg.tokenizer.answer_id, top_ids, top_lp)
        cand_ids = np.full((r_n * w, 2 * w), -1, np.int32)
        cand_lp = np.full((r_n * w, 2 * w), np.nan, np.float32)
        for n, (g, j) in enumerate(live):
            cand_ids[g * w + j], cand_lp[g * w + j] = top_ids[n].cpu().numpy(), top_lp[n].cpu().numpy()
        state, out = ref.select(state, cand_ids, cand_lp, w, beams_in, eos, early, norm, out)
        tok_planes.append(out["tokens"].reshape(r_n, w).copy())
        par_planes.append(out["parent"].reshape(r_n, w).copy())
        tok, par = tok_planes[-1], par_planes[-1]
        hyps = [[hyps[g][par[g][n]] + [int(tok[g][n])] if par[g][n] >= 0 else [] for n in range(w)] for g in range(r_n)]
    toks, pars = np.stack(tok_planes), np.stack(par_planes)
    return [ref.finalize(state, g, w, toks[:, g], pars[:, g], norm, n_ret) for g in range(r_n)]


def as_tuples(hyps):
    return [[(h.ids, np.float32(h.score), np.float32(h.logprob), h.finished) for h in req] for req in hyps]


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    assert torch.cuda.is_available(), "GPU tests need a device"
    t = Tiny()
    g = np.load(os.path.join(golden_dir, "tiny_seed1.npz"))
    t.cfg = get_config("tiny")
    sd = synth.synthetic_state_dict(t.cfg, seed=int(g["seed"]), device="cuda")
    t.model = MoondreamModel(t.cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=3 * (1 + 2 * W))
    t.model.set_strict_batch_invariance(True)
    t.images = [golden_image(g, i) for i in range(3)]
    t.prompts = [g["img0.cap.prompt"].tolist(), g["img1.cap.prompt"].tolist(), [1, 708, 9, 3]]  # two lengths
    t.eos = t.cfg.tokenizer.eos_id
    t.kw = dict(max_tokens=N, length_penalty=1.0, early_stopping=False, num_return_sequences=W)
    t.got = t.model.batch_beam_search_ids(t.images, t.prompts, W, **t.kw)
    t.trace = t.model.last_beam_trace
    return t


def test_exact_replay(tiny):
    want = host_beam_search(tiny.model, tiny.images, tiny.prompts, W, N, tiny.eos, 1.0, False, W)
    got = as_tuples(tiny.got)
    assert got == want
    # the reorder was exercised: some step had a child whose parent is another beam
    par = tiny.trace["parents"][1:]
    crossed = (par >= 0) & (par != np.arange(W)[None, None, :])
    assert crossed.any(), tiny.trace["parents"].tolist()


def test_one_beam_is_greedy(tiny):
    m = tiny.model
    ids, lps, _ = m.batch_generate_ids(tiny.images, tiny.prompts, max_tokens=N, ignore_eos=True, return_logprobs=True)
    got = m.batch_beam_search_ids(tiny.images, tiny.prompts, 1, max_tokens=N, ignore_eos=True)
    for r in range(3):
        assert got[r][0].ids == ids[r]
        total = np.float32(0.0)
        for x in lps[r]:
            total = np.float32(total + np.float32(x))
        assert np.float32(got[r][0].logprob) == total and not got[r][0].finished


def test_ignore_eos_runs_to_max_tokens(tiny):
    got = tiny.model.batch_beam_search_ids(tiny.images, tiny.prompts, W, max_tokens=N, ignore_eos=True, num_return_sequences=W)
    for req in got:
        assert len(req) == W and all(len(h.ids) == N and not h.finished for h in req)


def test_return_sequences_distinct_and_sorted(tiny):
    for req in tiny.got:
        assert len(req) == W
        assert len({tuple(h.ids) + (h.finished,) for h in req}) == W
        assert [h.score for h in req] == sorted((h.score for h in req), reverse=True)
    best = tiny.model.batch_beam_search_ids(tiny.images, tiny.prompts, W, max_tokens=N)
    assert [as_tuples([r])[0][0] for r in best] == [as_tuples([r])[0][0] for r in tiny.got]


def test_alone_and_in_a_batch(tiny):
    alone = tiny.model.batch_beam_search_ids(tiny.images[1:2], tiny.prompts[1:2], W, **tiny.kw)
    assert as_tuples(alone) == as_tuples(tiny.got[1:2])


def test_caption_returns_the_best_hypothesis(tiny):
    m = tiny.model
    text = m.batch_caption(tiny.images[:2], "normal", settings={"num_beams": W, "max_tokens": N})
    prompt = tiny.cfg.tokenizer.templates["caption"]["normal"]
    want = m.batch_beam_search_ids(tiny.images[:2], [prompt] * 2, W, max_tokens=N)
    assert text == [m.tokenizer.decode(h[0].ids) for h in want]
    assert m.caption(tiny.images[0], settings={"num_beams": W, "max_tokens": N})["caption"] == \
        m.batch_caption(tiny.images[:1], "normal", settings={"num_beams": W, "max_tokens": N})[0]


def test_captured_run_equals_eager_and_replays(tiny):
    m = tiny.model
    m.compile()
    try:
        got = m.batch_beam_search_ids(tiny.images, tiny.prompts, W, **tiny.kw)
        assert as_tuples(got) == as_tuples(tiny.got)
        stream = torch.cuda.current_stream().cuda_stream
        n_graphs = m._store.count("beam", stream)
        assert n_graphs >= 1
        # other prompts of the same lengths (and the images in another order): the same shapes, other prompt-derived state
        other = [tiny.images[1], tiny.images[0], tiny.images[2]]
        prompts = [[(t + 7) % 1000 + 4 for t in p] for p in tiny.prompts]
        assert prompts != tiny.prompts and [len(p) for p in prompts] == [len(p) for p in tiny.prompts]
        again = m.batch_beam_search_ids(other, prompts, W, **tiny.kw)
        assert m._store.count("beam", stream) == n_graphs  # replayed: no new capture
        m.use_graphs = False
        assert as_tuples(again) == as_tuples(m.batch_beam_search_ids(other, prompts, W, **tiny.kw))
        assert as_tuples(again) != as_tuples(tiny.got)
    finally:
        m.use_graphs = False
