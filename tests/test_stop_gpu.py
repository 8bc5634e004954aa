"""Stop strings and stop ids end to end on the tiny model, greedy, with a synthetic vocabulary of its size: every row's stop
set is made from that row's own free output, so it is certain to occur, and what the call returns is the free output cut
by the rule of tests/stop_ref.py -- eagerly and from captured chunks, over a shared prefix, with penalties, with
log-probabilities, and through the string-level calls."""
import os

import numpy as np
import pytest
import torch

from moondream_amd import synth
from moondream_amd.config import get_config
from moondream_amd.stop import Finish
from PIL import Image
from stop_ref import stop_ref

pytestmark = pytest.mark.gpu
N = 20
NEVER = "\x01\x02"  # bytes the synthetic vocabulary's multi-byte tokens never spell in a row


class Tiny:
    pass


def cross_token_string(vocab, row):
    """A substring of the row's text that starts inside one token and ends inside the next (both of >= 2 bytes)."""
    for j in range(2, len(row) - 1):
        a, b = vocab[row[j]], vocab[row[j + 1]]
        if len(a) >= 2 and len(b) >= 2:
            return (a[1:] + b[:1]).decode("latin-1")
    raise AssertionError("no two neighbouring tokens of two bytes in the row")


def cut(vocab, row, strings, ids, eos, include=False):
    """The rule restated on a row's FREE ids (generated with the eos ignored): (ids, Finish, text bytes)."""
    data = [vocab[t] for t in row]
    at, keep, which = stop_ref(data, [s.encode("latin-1") for s in strings], row, ids)
    eos_at = row.index(eos) if eos in row else None
    if at >= 0 and (eos_at is None or at < eos_at):
        if which < len(strings):
            n = keep + (len(strings[which].encode("latin-1")) if include else 0)
            return row[: at + 1], Finish("stop", strings[which], n), b"".join(data[: at + 1])[:n]
        return row[:at], Finish("stop", ids[which - len(strings)], None), b"".join(data[:at])
    if eos_at is not None:
        return row[:eos_at], Finish("eos"), b"".join(data[:eos_at])
    return row, Finish("length"), b"".join(data)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    assert torch.cuda.is_available(), "GPU tests need a device"
    t = Tiny()
    g = np.load(os.path.join(golden_dir, "tiny_seed1.npz"))
    t.cfg = get_config("tiny")
    sd = synth.synthetic_state_dict(t.cfg, seed=int(g["seed"]), device="cuda")
    t.model = MoondreamModel(t.cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=8)
    image = lambda i: Image.fromarray(synth.synthetic_image_array(int(g["image_index"][i]), int(g["seed"]), tuple(g[f"img{i}.cap.size"])), "RGB")
    imgs = [image(i) for i in range(3)]
    t.images = imgs + [imgs[0]]
    t.prompts = [g[f"img{i}.cap.prompt"].tolist() for i in range(3)] + [g["img1.cap.prompt"].tolist()]
    # every id spells latin-1 text of >= 2 bytes, so that any two neighbours make a cross-token string
    t.vocab = [bytes([97 + i % 23, 65 + (i // 23) % 26]) + (b"" if i % 3 else bytes([48 + i % 10])) for i in range(t.cfg.text.vocab_size)]
    t.kw = dict(max_tokens=N, ignore_eos=True)
    t.free = t.model.batch_generate_ids(t.images, t.prompts, **t.kw)
    assert all(len(r) == N for r in t.free)
    t.strings = [[cross_token_string(t.vocab, t.free[0]), NEVER], [], None, [NEVER]]
    t.ids = [[], [t.free[1][6], t.free[1][3]], None, []]
    t.stop = [s if s else None for s in t.strings]
    t.stop_ids = [i if i else None for i in t.ids]
    t.eos = t.free[3][7]  # an "eos" for the calls that honour one: row 3 ends on it
    return t


def want(t, eos, include=False, free=None):
    rows = free or t.free
    return [cut(t.vocab, rows[r], t.strings[r] or [], t.ids[r] or [], eos, include) for r in range(4)]


def test_ids_finish_and_text(tiny):
    """Fails without the feature: the arguments do not exist."""
    m = tiny.model
    for eos in (None, tiny.eos):
        kw = dict(max_tokens=N, ignore_eos=eos is None, eos_id=eos)
        for include in (False, True):
            ids, fin = m.batch_generate_ids(tiny.images, tiny.prompts, **kw, stop=tiny.stop, stop_token_ids=tiny.stop_ids,
                                            include_stop_str_in_output=include, vocab_bytes=tiny.vocab, return_finish=True)
            w = want(tiny, -1 if eos is None else eos, include)
            assert ids == [x[0] for x in w] and fin == [x[1] for x in w], (eos, include)
        assert not m._b1_used
    w = want(tiny, -1)
    assert w[0][1].reason == "stop" and w[0][1].text_bytes is not None and len(w[0][0]) < N
    assert w[1][1] == Finish("stop", w[1][1].stop, None) and w[1][1].stop in tiny.ids[1] and w[1][1].stop not in w[1][0]
    assert want(tiny, tiny.eos)[3][1].reason == "eos" and w[3][1].reason == "length" and w[2][1].reason == "length"
    # include_stop_str_in_output adds exactly the string
    a, b = want(tiny, -1, False)[0], want(tiny, -1, True)[0]
    assert b[2] == a[2] + a[1].stop.encode("latin-1") and a[0] == b[0]
    # without return_finish the value is the ids alone; a row with no stop set is the free row, bit for bit
    ids = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, stop=tiny.stop, stop_token_ids=tiny.stop_ids, vocab_bytes=tiny.vocab)
    assert ids == [x[0] for x in want(tiny, -1)] and ids[2] == tiny.free[2] and ids[3] == tiny.free[3]


def test_a_lone_sequence_and_ids_alone(tiny):
    m = tiny.model
    for r in (0, 1):
        ids, fin = m.batch_generate_ids(tiny.images[r : r + 1], tiny.prompts[r : r + 1], **tiny.kw, stop=tiny.stop[r],
                                        stop_token_ids=tiny.stop_ids[r], vocab_bytes=tiny.vocab if r == 0 else None, return_finish=True)
        assert not m._b1_used  # a lone sequence with a stop set decodes on the batched kernels
        m.single_sequence_kernel = False  # so does the free sequence it is compared with
        try:
            lone = m.batch_generate_ids(tiny.images[r : r + 1], tiny.prompts[r : r + 1], **tiny.kw)[0]
        finally:
            m.single_sequence_kernel = True
        w = cut(tiny.vocab, lone, tiny.strings[r] or [], tiny.ids[r] or [], -1)
        assert fin[0].reason == "stop" and (ids[0], fin[0]) == w[:2]
    with pytest.raises(ValueError, match="the IdTokenizer stand-in spells no bytes; pass vocab_bytes"):
        m.batch_generate_ids(tiny.images[:1], tiny.prompts[:1], **tiny.kw, stop="ab")
    with pytest.raises(ValueError, match="vocab_bytes: 5 entries"):
        m.batch_generate_ids(tiny.images[:1], tiny.prompts[:1], **tiny.kw, stop="ab", vocab_bytes=[b"a"] * 5)


def test_compiled_equals_eager_and_graphs_are_shared(tiny):
    m = tiny.model
    seen = []
    inner = m._stop_rows
    m._stop_rows = lambda *a, **k: (seen.append(1), inner(*a, **k))[1]
    call = lambda **kw: m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, vocab_bytes=tiny.vocab, return_finish=True, **kw)
    eager = call(stop=tiny.stop, stop_token_ids=tiny.stop_ids)
    m.compile()
    try:
        assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw) == tiny.free
        keys = set(m._graphs)
        del seen[:]
        assert m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, stop=[None] * 4, stop_token_ids=None) == tiny.free
        assert set(m._graphs) == keys and not seen and not any("stop" in k for k in keys if isinstance(k, tuple))
        for _ in range(2):  # the capturing call, then a replay
            assert call(stop=tiny.stop, stop_token_ids=tiny.stop_ids) == eager
        n_graphs = len(m._graphs)
        assert any(isinstance(k, tuple) and "stop" in k for k in m._graphs)
        # other strings whose table has the same power-of-two capacity: the same buffers, so the same graphs
        other = [[NEVER + "q"], cross_token_string(tiny.vocab, tiny.free[1]), None, None]
        ids, fin = call(stop=other)
        assert len(m._graphs) == n_graphs
        w = [cut(tiny.vocab, tiny.free[r], [other[r]] if isinstance(other[r], str) else (other[r] or []), [], -1) for r in range(4)]
        assert ids == [x[0] for x in w] and fin == [x[1] for x in w] and fin[1].reason == "stop"
    finally:
        del m._stop_rows
        m.use_graphs = False
        m._graphs.clear()


def test_rows_that_all_stop_end_the_loop_early(tiny):
    m = tiny.model
    steps = []
    inner = m._decode_step
    m._decode_step = lambda *a, **k: (steps.append(1), inner(*a, **k))[1]
    try:
        long = dict(max_tokens=64, ignore_eos=True)
        free = m.batch_generate_ids(tiny.images, tiny.prompts, **long)
        n_free = len(steps)
        del steps[:]
        ids, fin = m.batch_generate_ids(tiny.images, tiny.prompts, **long, stop_token_ids=[[r[4]] for r in free], return_finish=True)
        assert len(steps) == 16 < n_free  # the first all-done check, after one chunk of 16 steps
        assert all(f.reason == "stop" for f in fin) and ids == [r[: r.index(r[4])] for r in free]
    finally:
        del m._decode_step


def test_logprobs_shared_prefix_and_penalties(tiny):
    m = tiny.model
    args = dict(stop=tiny.stop, stop_token_ids=tiny.stop_ids, vocab_bytes=tiny.vocab)
    ids, lp, rk, alts, fin = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **args, return_logprobs=True, top_logprobs=3,
                                                  return_finish=True)
    f_ids, f_lp, f_rk, f_alts = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, return_logprobs=True, top_logprobs=3)
    w = want(tiny, -1)
    assert ids == [x[0] for x in w] and fin == [x[1] for x in w] and f_ids == tiny.free
    for r in range(4):  # cut to the ids' length, and the free call's values
        n = len(ids[r])
        assert (lp[r], rk[r], alts[r]) == (f_lp[r][:n], f_rk[r][:n], f_alts[r][:n])
    for kw in (dict(share_prefix=True), dict(repetition_penalty=[1.0, 1.3, 1.0, 1.2], presence_penalty=[0.5, 0.0, 0.0, 0.0])):
        free = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **kw)
        ids, fin = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **kw, **args, return_finish=True)
        w = want(tiny, -1, free=free)
        assert ids == [x[0] for x in w] and fin == [x[1] for x in w], kw


def test_string_level_calls(tiny):
    m = tiny.model
    tpl = tiny.cfg.tokenizer.templates["caption"]["normal"]
    st = {"temperature": 0, "max_tokens": N}
    free = m.batch_generate_ids(tiny.images[:3], [tpl] * 3, max_tokens=N)
    plain = m.batch_caption(tiny.images[:3], "normal", st)
    assert plain == [m.tokenizer.decode(r) for r in free]
    s0 = cross_token_string(tiny.vocab, free[0])
    for include in (False, True):
        stops = {**st, "stop": [s0, None, NEVER], "stop_token_ids": [None, [free[1][5]], None], "vocab_bytes": tiny.vocab,
                 "include_stop_str_in_output": include}
        got = m.batch_caption(tiny.images[:3], "normal", stops)
        w0 = cut(tiny.vocab, free[0], [s0], [], m.config.tokenizer.eos_id, include)
        w1 = cut(tiny.vocab, free[1], [], [free[1][5]], m.config.tokenizer.eos_id)
        assert got == [w0[2].decode("utf-8", errors="replace"), m.tokenizer.decode(w1[0]), plain[2]]
        assert w0[1].reason == "stop" and (w0[2].endswith(s0.encode("latin-1")) == include)
    one = {**st, "stop": s0, "vocab_bytes": tiny.vocab}  # one image: the batched route with one row
    got = m.caption(tiny.images[0], "normal", settings=one)
    assert got == {"caption": m.batch_caption(tiny.images[:1], "normal", one)[0]}
    assert got != m.caption(tiny.images[0], "normal", settings=st) and " " not in got["caption"]  # bytes, not the stand-in's ids


def test_what_is_not_served_raises(tiny):
    m = tiny.model
    im, st = tiny.images[0], {"temperature": 0, "max_tokens": 4, "stop_token_ids": [11]}
    refused = [
        lambda: m.query(im, "1 2", reasoning=True, settings=st),
        lambda: m.batch_query([im], ["1 2"], settings=st, reasoning=True),
        lambda: m.query_many_reasoning(im, ["1 2"], settings=st),
        lambda: m.batch_caption([im], "normal", {**st, "num_beams": 2}),
        lambda: m.caption(im, "normal", stream=True, settings=st),
        lambda: m.query(im, "1 2", stream=True, settings=st),
        lambda: m.batch_detect([im], ["1 2"], settings=st),
        lambda: m.batch_point([im], ["1 2"], settings=st),
        lambda: m.detect_many(im, ["1 2"], settings=st),
        lambda: m.point_many(im, ["1 2"], settings=st),
        lambda: list(m.batch_detect_pipelined([([im], ["1 2"])], settings=st)),
        lambda: list(m.batch_generate_ids_pipelined([([im], [tiny.prompts[0]])], max_tokens=4, stop_token_ids=[11])),
        lambda: m.score_ids([im], [tiny.prompts[0]], [[5, 6]], stop="ab"),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(ValueError, match="stop / stop_token_ids are not served|not served by beam search"):
            call()
            pytest.fail(f"call {i} was served")
    from moondream_amd.hf_moondream import _refuse_extensions

    with pytest.raises(ValueError, match="stop / stop_token_ids are not served by HfMoondream"):
        _refuse_extensions({"settings": st})


def test_query_calls_cut_their_text(tiny):
    """``batch_query``, ``query_many`` (one shared prefix) and ``query`` about an image, each with a stop string made from
    its own free answer: the text is the free answer's bytes in front of the string."""
    m = tiny.model
    st = {"temperature": 0, "max_tokens": N}
    qs = ["11 12 13", "14 15"]
    spell = lambda ids: b"".join(tiny.vocab[t] for t in ids)
    eos = m.config.tokenizer.eos_id
    for name, call, images in (("batch_query", lambda s: m.batch_query(tiny.images[:2], qs, s), tiny.images[:2]),
                               ("query_many", lambda s: [a["answer"] for a in m.query_many(tiny.images[0], qs, s)], None)):
        if images is not None:
            free = m.batch_generate_ids(images, m._query_prompts(qs), max_tokens=N)
        else:
            enc = m.encode_image(tiny.images[0])
            free = m.batch_generate_ids([enc, enc], m._query_prompts(qs), max_tokens=N, share_prefix=True)
        assert call(st) == [m.tokenizer.decode(r) for r in free], name
        s0 = cross_token_string(tiny.vocab, free[0])
        got = call({**st, "stop": [s0, None], "vocab_bytes": tiny.vocab})
        w0 = cut(tiny.vocab, free[0], [s0], [], eos)
        assert got == [w0[2].decode("utf-8", errors="replace"), m.tokenizer.decode(free[1])], name
        assert w0[1].reason == "stop" and spell(free[0]).startswith(w0[2]) and len(w0[2]) < len(spell(free[0]))
    one = {**st, "stop": s0, "vocab_bytes": tiny.vocab}
    got = m.query(tiny.images[0], qs[0], settings=one)
    assert got == {"answer": m.batch_query(tiny.images[:1], qs[:1], one)[0]} and " " not in got["answer"]
    with pytest.raises(ValueError, match="stop / stop_token_ids are served for a query about an image"):
        m.query(None, qs[0], settings=one)


def test_continuous_engine_equals_the_lockstep_call(tiny):
    """Requests with string stops, id stops and none through two KV slots: the ids and ``Finish`` records of the lockstep
    call, eagerly and from captured chunks; the stopped requests' slots are refilled; ``run_text`` cuts the text."""
    from moondream_amd.continuous import ContinuousEngine

    m = tiny.model
    args = dict(stop=tiny.stop, stop_token_ids=tiny.stop_ids, vocab_bytes=tiny.vocab)
    for include in (False, True):
        lock = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **args, include_stop_str_in_output=include, return_finish=True)
        assert lock == ([x[0] for x in want(tiny, -1, include)], [x[1] for x in want(tiny, -1, include)])
        for compiled in (False, True):
            if compiled:
                m.compile()
            try:
                eng = ContinuousEngine(m, max_live=2, chunk=4)
                got = eng.generate(tiny.images, tiny.prompts, **tiny.kw, **args, include_stop_str_in_output=include, return_finish=True)
                assert got == lock, (include, compiled)
                assert eng.stats.admissions > 1
                assert eng.generate(tiny.images[:3], tiny.prompts[:3], **tiny.kw) == tiny.free[:3]  # stale matcher words do not leak
            finally:
                m.use_graphs = False
                m._graphs.clear()
    got = m.batch_generate_ids_continuous(tiny.images, tiny.prompts, **tiny.kw, max_live=2, chunk=4, **args, return_finish=True)
    assert got == m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **args, return_finish=True)
    ids, lp, rk, fin = m.batch_generate_ids_continuous(tiny.images, tiny.prompts, **tiny.kw, max_live=2, chunk=4, **args,
                                                       return_logprobs=True, return_finish=True)
    l_ids, l_lp, l_rk, l_fin = m.batch_generate_ids(tiny.images, tiny.prompts, **tiny.kw, **args, return_logprobs=True, return_finish=True)
    assert (ids, rk, fin) == (l_ids, l_rk, l_fin) and [len(x) for x in lp] == [len(x) for x in ids]
    eng = ContinuousEngine(m, max_live=2, chunk=4)
    rid = eng.submit(tiny.images[0], tiny.prompts[0], **tiny.kw, stop=tiny.stop[0], vocab_bytes=tiny.vocab)
    free_rid = eng.submit(tiny.images[2], tiny.prompts[2], **tiny.kw)
    texts = dict(eng.run_text())
    assert texts[rid] == want(tiny, -1)[0][2].decode("utf-8", errors="replace") and texts[free_rid] == m.tokenizer.decode(tiny.free[2])
    assert eng.finishes[rid] == want(tiny, -1)[0][1] and eng.finishes[free_rid] == Finish("length")
    with pytest.raises(ValueError, match="the IdTokenizer stand-in spells no bytes"):
        eng.submit(tiny.images[0], tiny.prompts[0], stop="ab")
    with pytest.raises(ValueError, match="one vocab_bytes object per engine"):
        eng.submit(tiny.images[0], tiny.prompts[0], stop="ab", vocab_bytes=list(tiny.vocab))


def test_continuous_engine_makes_fewer_steps_when_requests_stop_early(tiny):
    from moondream_amd.continuous import ContinuousEngine

    m = tiny.model
    images, prompts = tiny.images * 2, tiny.prompts * 2
    long = dict(max_tokens=48, ignore_eos=True)
    eng = ContinuousEngine(m, max_live=2, chunk=4)
    free = eng.generate(images, prompts, **long)
    free_steps = eng.stats.decode_steps
    ids, fin = eng.generate(images, prompts, **long, stop_token_ids=[[r[3]] for r in free], return_finish=True)
    assert all(f.reason == "stop" for f in fin) and ids == [r[: r.index(r[3])] for r in free]
    assert eng.stats.decode_steps < free_steps / 2, (eng.stats.decode_steps, free_steps)
