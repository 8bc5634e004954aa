"""Beam search without a GPU: the argument checks and refusals (all raised before any device work: the model here has
no device at all), the host finalisation and backtracking on hand-made planes and pools, and the beam chunk's launch
order and graph key through the recording stand-in model of the decode-chunk tests."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import beam_ref as ref
from moondream_amd import beam as hb
from moondream_amd.decode_loop import Beam, DecodeChunk, run_chunk
from moondream_amd.moondream import MoondreamModel
from test_decode_chunk_cpu import N, PAD, STREAM, Recorder, Rows, make_chunk, same


# ----------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("bad", [0, 17, -1, 2.0, "3", None, True])
def test_num_beams_refused(bad):
    with pytest.raises(ValueError, match="num_beams"):
        hb.check_beams(bad)


def test_other_arguments_refused():
    assert hb.check_beams(4, 4, -0.5, True) == (4, 4, -0.5, True)
    assert hb.check_beams(np.int64(16)) == (16, 1, 1.0, False)
    for n in (0, 5, 1.0, True):
        with pytest.raises(ValueError, match="num_return_sequences"):
            hb.check_beams(4, n)
    for lp in (float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="length_penalty"):
            hb.check_beams(4, 1, lp)
    for es in (0, 1, "never", None):
        with pytest.raises(ValueError, match="early_stopping"):
            hb.check_beams(4, 1, 1.0, es)


def test_settings_entries():
    assert hb.beams_of(None) is None and hb.beams_of({}) is None and hb.beams_of({"num_beams": 1}) is None
    assert hb.beams_of({"num_beams": None, "length_penalty": 2.0}) is None
    assert hb.beams_of({"num_beams": 3, "length_penalty": 0.5, "early_stopping": True}) == (3, 0.5, True)
    with pytest.raises(ValueError, match="length_penalty"):  # checked even where it is unused
        hb.beams_of({"length_penalty": float("nan")})
    hb.refuse_beams({"num_beams": 1}, "x")
    with pytest.raises(ValueError, match="not served by the engine"):
        hb.refuse_beams({"num_beams": 2}, "the engine")


class NoDevice(MoondreamModel):
    """A model with no weights and no device: any GPU work raises AttributeError, not ValueError."""

    def __init__(self, kv8=None):
        from moondream_amd.config import get_config

        from moondream_amd.moondream import IdTokenizer

        self.config = get_config("tiny")
        self.tokenizer = IdTokenizer()  # host only
        self._kv8_scales = kv8


def test_public_calls_refuse_before_device_work():
    m = NoDevice()
    img, p = object(), [[1, 2]]
    with pytest.raises(ValueError, match="num_beams"):
        m.batch_beam_search_ids([img], p, 0)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.batch_beam_search_ids([img], p, 2, num_return_sequences=3)
    with pytest.raises(ValueError, match="length_penalty"):
        m.batch_beam_search_ids([img], p, 2, length_penalty=float("inf"))
    with pytest.raises(ValueError, match="early_stopping"):
        m.batch_beam_search_ids([img], p, 2, early_stopping="yes")
    with pytest.raises(ValueError, match="max_tokens"):
        m.batch_beam_search_ids([img], p, 2, max_tokens=0)
    with pytest.raises(ValueError, match="empty prompt"):
        m.batch_beam_search_ids([img], [[]], 2)
    with pytest.raises(ValueError, match="images and"):
        m.batch_beam_search_ids([img], [[1], [2]], 2)
    with pytest.raises(ValueError, match="fp8 KV"):
        NoDevice(kv8=object()).batch_beam_search_ids([img], p, 2)


NOT_SERVED = [
    ({"repetition_penalty": 1.2}, "penalty"), ({"presence_penalty": 0.5}, "penalty"), ({"frequency_penalty": 0.1}, "penalty"),
    ({"variant": "v"}, "variant"), ({"variants": ["v"]}, "variant"),
]


@pytest.mark.parametrize("extra,word", NOT_SERVED)
def test_string_api_refuses_what_beams_do_not_serve(extra, word):
    m = NoDevice()
    st = {"num_beams": 3, **extra}
    for call in (lambda: m.batch_caption([object()], "normal", st), lambda: m.batch_query([object()], ["5 6"], st),
                 lambda: m.batch_generate([object()], None, st), lambda: m.caption(object(), settings=st),
                 lambda: m.query(object(), "5 6", settings=st)):
        with pytest.raises(ValueError, match=word):
            call()


def test_constraints_refused_with_beams():
    from moondream_amd.constraint import TokenAutomaton

    m = NoDevice()
    st = {"num_beams": 2, "constraints": TokenAutomaton.allowed_tokens([5, 6])}
    with pytest.raises(ValueError, match="constraints are not served by beam search"):
        m.batch_caption([object()], "normal", st)


def test_modes_that_do_not_serve_beams():
    m = NoDevice()
    st = {"num_beams": 2}
    with pytest.raises(ValueError, match="stream=True"):
        m.caption(object(), stream=True, settings=st)
    with pytest.raises(ValueError, match="reasoning=True or stream=True"):
        m.query(object(), "5 6", reasoning=True, settings=st)
    with pytest.raises(ValueError, match="reasoning=True or stream=True"):
        m.query(object(), "5 6", stream=True, settings=st)
    with pytest.raises(ValueError, match="reasoning"):
        m.batch_query([object()], ["5 6"], st, reasoning=True)
    with pytest.raises(ValueError, match="reasoning"):
        m.query_many_reasoning(object(), ["5 6"], st)
    for call in (m.batch_detect, m.batch_point):
        with pytest.raises(ValueError, match="not served by"):
            call([object()], ["7"], st)
    for call in (m.detect_many, m.point_many):
        with pytest.raises(ValueError, match="not served by"):
            call(object(), ["7"], st)
    with pytest.raises(ValueError, match="not served by"):
        next(iter(m.batch_detect_pipelined([([object()], ["7"])], st)))
    with pytest.raises(ValueError, match="num_beams"):  # a value that is none is an error everywhere
        m.batch_caption([object()], "normal", {"num_beams": 99})


def test_hf_wrapper_refuses_beams():
    from moondream_amd.hf_moondream import HfMoondream

    hf = HfMoondream.__new__(HfMoondream)
    st = {"num_beams": 2}
    for call in (lambda: hf.answer_question(object(), "5 6", settings=st), lambda: hf.batch_answer([object()], ["5 6"], settings=st),
                 lambda: hf.generate(object(), "5 6", settings=st)):
        with pytest.raises(ValueError, match="HfMoondream"):
            call()


# ----------------------------------------------------------------------------- host finalisation
def test_inv_norm_table():
    t = hb.inv_norm_table(6, 1.5)
    assert t.dtype == np.float32 and t[0] == 1.0
    assert all(t[k] == np.float32(1.0 / float(k) ** 1.5) for k in range(1, 6))
    assert np.array_equal(t, ref.inv_norm_table(6, 1.5))


def planes():
    """Three decisions of one request, W = 3.  Decision 1 crosses: beam 0 continues beam 1."""
    tokens = np.array([[10, 11, 12], [20, 21, 22], [30, 31, 32]])
    parents = np.array([[0, 0, 0], [1, 0, 2], [0, 0, 1]])
    return tokens, parents


def test_backtrack():
    tokens, parents = planes()
    assert hb.backtrack(tokens, parents, 0, 3) == [11, 20, 30]
    assert hb.backtrack(tokens, parents, 2, 3) == [10, 21, 32]
    assert hb.backtrack(tokens, parents, 1, 1) == [11]
    assert hb.backtrack(tokens, parents, 2, 0) == []
    assert hb.backtrack(tokens, parents, 2, 2) == ref.backtrack(tokens, parents, 2, 2) == [12, 22]


def finalize(done, pool, cum, n_ret=3, w=3, length=3, lp=1.0):
    tokens, parents = planes()
    pad = lambda xs, dt: np.array(list(xs) + [0] * (w - len(xs)), dtype=dt)
    return hb.finalize(w, n_ret, length, done, np.asarray(cum, np.float32), len(pool), pad([e[0] for e in pool], np.float32),
                       pad([e[1] for e in pool], np.float32), pad([e[2] for e in pool], np.int32),
                       pad([e[3] for e in pool], np.int32), tokens, parents, hb.inv_norm_table(8, lp))


def test_finalize_done_request_uses_the_pool_alone():
    out = finalize(True, [(-1.0, -2.0, 1, 1), (-0.5, -1.5, 0, 2)], [-0.1, -0.2, -0.3])
    assert [(h.ids, h.score, h.logprob, h.finished) for h in out] == [([11, 20], -0.5, -1.5, True), ([11], -1.0, -2.0, True)]


def test_finalize_unfinished_beams_enter_under_the_insert_rule():
    inv3 = np.float32(1.0 / 3.0)
    cum = np.array([-0.3, -6.0, -np.inf], np.float32)
    out = finalize(False, [(-1.0, -2.0, 1, 1), (-1.0, -1.5, 0, 2)], cum)
    # beam 0 (score -0.1) is appended; beam 1 (-2.0) meets a full pool whose worst is better; the dead beam is not a hypothesis
    assert [h.finished for h in out] == [False, True, True]
    assert out[0].ids == [11, 20, 30] and out[0].score == float(np.float32(cum[0] * inv3)) and out[0].logprob == float(cum[0])
    assert [h.ids for h in out[1:]] == [[11], [11, 20]]  # equal scores: pool order
    # a full pool: the worst entry is the LAST of the equal scores, replaced only by a strictly greater score
    full = [(-1.0, -2.0, 1, 1), (-1.0, -1.5, 0, 2), (-0.2, -0.4, 2, 2)]
    out = finalize(False, full, np.array([-0.3, -3.0, -np.inf], np.float32))
    assert [h.ids for h in out] == [[11, 20, 30], [12, 22], [11]]  # entry 1 went, entry 0 stayed; -3.0 / 3 == -1.0 is not greater
    assert len(finalize(False, full, cum, n_ret=1)) == 1


def test_finalize_agrees_with_the_oracle():
    tokens, parents = planes()
    state = ref.new_state(1, 3, [4])
    state["len"][:] = 3
    state["cum"][:] = np.array([-0.7, -0.9, -2.5], np.float32)
    state["pool_n"][:] = 2
    state["pool_score"][0, :2] = [-0.4, -0.8]
    state["pool_sum"][0, :2] = [-0.8, -2.4]
    state["pool_parent"][0, :2] = [2, 0]
    state["pool_step"][0, :2] = [1, 2]
    norm = ref.inv_norm_table(8, 0.7)
    want = ref.finalize(state, 0, 3, tokens, parents, norm, 3)
    got = hb.finalize(3, 3, 3, False, state["cum"], 2, state["pool_score"][0], state["pool_sum"][0], state["pool_parent"][0],
                      state["pool_step"][0], tokens, parents, norm)
    assert [(h.ids, np.float32(h.score), np.float32(h.logprob), h.finished) for h in got] == want


# ----------------------------------------------------------------------------- the chunk
class BeamRecorder(Recorder):
    def _beam_select(self, logits, suppress_id, beam, beams_in, tokens_out, parents_out):
        self.calls.append(("select", logits, suppress_id, beam.num_beams, beams_in, tokens_out, parents_out))

    def _kv_copy_tail(self, kv, beam):
        self.calls.append(("copy", kv.slot0, beam.src))


def make_beam(b=4, w=2):
    t = lambda: torch.zeros(b, dtype=torch.int32)
    keep = (torch.zeros(b), t())
    return Beam(w, 0, False, object(), torch.zeros(N + PAD, b, dtype=torch.int32), t(), t(), t(), t(), 12, keep)


def test_beam_chunk_launch_order():
    m = BeamRecorder()
    c = make_chunk(b=4, beam=make_beam())
    run_chunk(m, c, N)
    kinds = [x[0] for x in m.calls]
    assert kinds == ["step", "select", "copy"] * N
    lg = m.logits[:4]
    for i in range(N):
        step, sel, cp = m.calls[3 * i : 3 * i + 3]
        assert same(step[2], c.tokens[i]) and same(step[3], c.tokens[i + 1])
        assert same(sel[1], lg) and sel[2] == 7 and sel[3] == 2 and sel[4] == 2
        assert same(sel[5], c.tokens[i + 1]) and same(sel[6], c.beam.parents[i])
        assert cp[1] == 0 and cp[2] is c.beam.src


def test_beam_chunk_graph_key():
    m = BeamRecorder()
    plain = make_chunk(b=4)
    run_chunk(m, plain, N, capture_stream=STREAM)
    key_plain = m.key
    assert "beam" not in key_plain
    c = replace(plain, beam=make_beam())
    run_chunk(m, c, N, capture_stream=STREAM)
    key = m.key
    assert key[: len(key_plain)] == key_plain and key[len(key_plain)] == "beam"
    assert key[len(key_plain) + 1 : len(key_plain) + 5] == (2, 0, False, 12)
    for name in ("parents", "src", "dst", "frm", "to"):  # every address the launches bake in tells two chunks apart
        other = replace(c, beam=replace(c.beam, **{name: torch.zeros_like(getattr(c.beam, name))}))
        run_chunk(m, other, N, capture_stream=STREAM)
        assert m.key != key, name
    for change in (dict(num_beams=3), dict(eos_id=-1), dict(early_stopping=True), dict(n_slots=13),
                   dict(keep=(torch.zeros(4), c.beam.keep[1]))):
        run_chunk(m, replace(c, beam=replace(c.beam, **change)), N, capture_stream=STREAM)
        assert m.key != key, change
    run_chunk(m, c, N, capture_stream=STREAM)  # the same record again: replayed
    assert m.key == key and m.calls[-1] == ("replay",)


def test_chunk_without_the_record_is_todays():
    """No beam record: the launches and the key of a plain chunk, written out literally as the parent commit makes them
    (decode_loop.run_chunk before the field existed): one fused step per step and nothing else, and the 17-entry key
    (tag, stream, b, n, suppress, tokens, pos, workspace, k, k8, logits, b1, pick, uniforms) + the routing's three."""
    m = BeamRecorder()
    c = make_chunk(b=2)
    assert c.beam is None
    run_chunk(m, c, N, capture_stream=STREAM)
    lg = m.logits
    # the first chunk of a key runs eagerly, then the capture records the same body once more
    assert [x[0] for x in m.calls] == ["step"] * N + ["capture"] + ["step"] * N
    for i, call in enumerate(m.calls[:N]):
        name, rows, tin, tout, pos, b, sup, logits, ws, slot0 = call
        assert (name, rows, b, sup, slot0) == ("step", f"step{i}", 2, 7, 0)
        assert same(tin, c.tokens[i]) and same(tout, c.tokens[i + 1]) and pos is c.pos and logits is lg and ws is m.ws
    assert m.key == ("decode", STREAM, 2, N, 7, c.tokens.data_ptr(), c.pos.data_ptr(), m.ws.data_ptr(), 1000, 0, lg.data_ptr(),
                     False, None, 0, "step0", None, None)
    assert m.ws_asked == (48, 2)


def test_beam_record_excludes_the_other_optional_fields():
    m = BeamRecorder()
    from moondream_amd.decode_loop import Sampling

    with pytest.raises(AssertionError):
        run_chunk(m, make_chunk(b=4, pick="scalar", beam=make_beam()), N)
    with pytest.raises(AssertionError):
        run_chunk(m, make_chunk(b=1, b1=True, beam=make_beam(1, 1)), N)
