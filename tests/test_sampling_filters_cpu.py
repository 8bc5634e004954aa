"""Per-request top-k / min-p sampling without a GPU: the torch restatement (tests/sampling_filter_ref.py) against the
oracle's top-p restatement and against hand-made rows, every Python entry point's argument checks (before any device
work, no library loaded), and the launch and graph key of a chunk whose ``Sampling`` carries the two fields, on the
recording stand-in of tests/test_decode_chunk_cpu.py."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from moondream_amd.continuous import ContinuousEngine, Request  # noqa: F401  (the engine's module imports without a device)
from moondream_amd.decode_loop import FILTER_NEUTRAL, Sampling, check_filters, filters_of, refuse_filters, run_chunk
from moondream_amd.hf_moondream import HfMoondream
from oracle import moondream_oracle as O
from sampling_filter_ref import draw, filter_probs
from test_decode_chunk_cpu import N, STREAM, Recorder, assert_calls, expected_calls, make_chunk
from test_logprobs_cpu import IMG, FakeEngine, FakeModel, host_model

BF16 = torch.bfloat16


def bits(t):
    return t.view(torch.int16)


def kept(q):
    return (q.float() > 0).nonzero().flatten().tolist()


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("temperature,top_p", [(0.5, 0.3), (1.0, 0.9), (2.0, 1.0), (0.05, 0.3)])
def test_with_both_filters_off_it_is_the_oracles_top_p(temperature, top_p):
    g = torch.Generator().manual_seed(int(temperature * 100))
    for vocab in (37, 1025, 4096):
        logits = (torch.randn(3, vocab, generator=g) * 3).to(BF16)
        logits[1, 5] = logits[1, vocab - 3] = logits[1].max()  # a tie at the top
        for r in range(3):
            p = O.sampling_probs(logits[r], temperature)
            want = O.apply_top_p(p, top_p)
            for off in ((0, 0.0), (vocab, 0.0), (vocab + 5, 0.0)):
                assert torch.equal(bits(filter_probs(p, top_p, *off)), bits(want)), (vocab, r, off)


def row(values):
    return torch.tensor(values, dtype=torch.float32).to(BF16)


def test_top_k_keeps_the_first_k_of_the_stable_descending_order():
    # a tie that straddles k: ids 1, 4, 6 share the second value; k = 3 keeps the best and the two LOWEST of them
    p = row([0.0625, 0.125, 0.03125, 0.5, 0.125, 0.015625, 0.125, 0.015625])
    assert kept(filter_probs(p, 1.0, top_k=3)) == [1, 3, 4]
    assert kept(filter_probs(p, 1.0, top_k=1)) == [3]
    assert kept(filter_probs(p, 1.0, top_k=4)) == [1, 3, 4, 6]
    assert kept(filter_probs(p, 1.0, top_k=8)) == kept(filter_probs(p, 1.0)) == list(range(8))
    q = filter_probs(p, 1.0, top_k=3).float()  # renormalised by the bf16 sum 0.75, each quotient rounded to bf16
    assert q[3] == (torch.tensor(0.5) / 0.75).to(BF16).float() and q[1] == q[4] == (torch.tensor(0.125) / 0.75).to(BF16).float()
    # the cuts are prefixes of one order: the shortest wins, whichever rule it is
    assert kept(filter_probs(p, 0.3, top_k=3)) == [3]              # top-p: only the best has preceding mass <= 0.3
    assert kept(filter_probs(p, 0.6, top_k=5)) == [1, 3]           # top-p 0.6: the mass before id 4 is 0.625
    assert kept(filter_probs(p, 1.0, top_k=5, min_p=0.25)) == [1, 3, 4, 6]


def test_min_p_keeps_what_reaches_its_share_of_the_best():
    p = row([0.0625, 0.125, 0.03125, 0.5, 0.125, 0.015625, 0.125, 0.015625])
    assert kept(filter_probs(p, 1.0, min_p=1.0)) == [3]                      # the best always survives
    assert kept(filter_probs(p, 1.0, min_p=0.25)) == [1, 3, 4, 6]            # >= 0.125, the value itself included
    assert kept(filter_probs(p, 1.0, min_p=0.26)) == [3]
    assert kept(filter_probs(p, 1.0, min_p=0.03125)) == list(range(8))       # 0.015625 = 0.03125 * 0.5
    tie = row([0.25, 0.125, 0.25, 0.25, 0.125])
    assert kept(filter_probs(tie, 1.0, min_p=1.0)) == [0, 2, 3]              # everything tied for best
    # the threshold is a bf16 number: bf16(float32(0.3) * 0.5) = 0.150390625 > 0.15 = what a float product would test
    edge = row([0.5, 0.150390625, 0.1494140625])
    assert kept(filter_probs(edge, 1.0, min_p=0.3)) == [0, 1]


def test_draw_rule_on_a_small_row():
    q = row([0.0, 0.25, 0.0, 0.5, 0.25])
    assert [draw(q, u) for u in (0.0, 0.2, 0.25, 0.74, 0.75, 0.999)] == [1, 1, 3, 3, 4, 4]


# ------------------------------------------------------------------ argument checks
def test_check_filters():
    assert check_filters(0, 0.0, 3) is None and check_filters(None, None, 2) is None and check_filters([0, 0], np.float32(0), 2) is None
    assert check_filters(40, 0.0, 2) == [(40, 0.0), (40, 0.0)]
    assert check_filters([1, 0], [0, 0.5], 2) == [(1, 0.0), (0, 0.5)]
    assert check_filters(np.int64(7), 1, 1) == [(7, 1.0)]
    for bad in ((-1, 0), (True, 0), (1.5, 0), ("3", 0), (object(), 0), (0, 1.5), (0, -0.1), (0, float("nan")), (0, float("inf")),
                (0, "x"), (0, True), ([1], 0), (0, [0.1] * 3), ([1, -1], 0)):
        with pytest.raises(ValueError):
            check_filters(*bad, 2)
    assert filters_of(None) == dict(zip(("top_k", "min_p"), FILTER_NEUTRAL))
    refuse_filters({"top_k": 0, "min_p": 0.0}, "x")
    with pytest.raises(ValueError, match="not served by the thing"):
        refuse_filters({"min_p": 0.1}, "the thing")


BAD = [{"top_k": -1}, {"top_k": True}, {"top_k": 2.5}, {"min_p": 1.5}, {"min_p": float("nan")}, {"min_p": -0.01}]


def test_value_errors_precede_any_device_work():
    m = host_model()  # any device work raises AttributeError
    for bad in BAD:
        for call in (lambda: m.batch_generate_ids([IMG], [[1, 2]], **bad),
                     lambda: m.batch_generate_ids_continuous([IMG], [[1, 2]], **bad),
                     lambda: m.batch_caption([IMG], settings=bad), lambda: m.batch_query([IMG], ["q"], settings=bad),
                     lambda: m.batch_generate([IMG], settings=bad), lambda: m.query_many(IMG, ["q"], settings=bad),
                     lambda: m.caption(IMG, settings=bad), lambda: m.query(IMG, "q", settings=bad),
                     lambda: FakeEngine(FakeModel(), max_live=2).submit(IMG, [5], **bad),
                     lambda: FakeEngine(FakeModel(), max_live=2).generate([IMG], [[5]], **bad)):
            with pytest.raises(ValueError):
                call()
    for wrong_length in (dict(top_k=[3]), dict(min_p=[0.5, 0.5, 0.5])):
        with pytest.raises(ValueError):
            m.batch_generate_ids([IMG, IMG], [[1, 2], [1, 2]], **wrong_length)
        with pytest.raises(ValueError):
            m.batch_generate_ids_continuous([IMG, IMG], [[1, 2], [1, 2]], **wrong_length)
        with pytest.raises(ValueError):
            FakeEngine(FakeModel(), max_live=2).generate([IMG, IMG], [[5], [5]], **wrong_length)
    with pytest.raises(ValueError):
        FakeEngine(FakeModel(), max_live=2).submit(IMG, [5], top_k=[3])  # one value per request


def test_what_is_not_served_says_so():
    m = host_model()
    hf = object.__new__(HfMoondream)
    for on in ({"top_k": 40}, {"min_p": 0.1}):
        refused = [lambda: m.batch_query([IMG], ["q"], settings=on, reasoning=True), lambda: m.query(IMG, "q", reasoning=True, settings=on),
                   lambda: m.query_many_reasoning(IMG, ["q"], settings=on),
                   lambda: m.batch_detect([IMG], ["cat"], settings=on), lambda: m.batch_point([IMG], ["cat"], settings=on),
                   lambda: m.detect_many(IMG, ["cat"], settings=on), lambda: m.point_many(IMG, ["cat"], settings=on),
                   lambda: m.detect(IMG, "cat", settings=on), lambda: m.point(IMG, "cat", settings=on),
                   lambda: next(m.batch_detect_pipelined([([IMG], ["cat"])], settings=on)),
                   lambda: m.batch_generate_ids_pipelined([([IMG], [[1, 2]])], **on),
                   lambda: hf.answer_question(IMG, "q", settings=on), lambda: hf.batch_answer([IMG], ["q"], settings=on),
                   lambda: hf.generate(IMG, "p", settings=on)]
        for call in refused:
            with pytest.raises(ValueError, match="top_k / min_p are not served"):
                call()


def test_engine_takes_the_settings_per_request():
    eng = FakeEngine(FakeModel(), max_live=2, chunk=4)
    eng.submit(IMG, [5], max_tokens=2)
    eng.submit(IMG, [5], max_tokens=2, temperature=0.5, top_k=40, min_p=0.1)
    eng.submit(IMG, [5], max_tokens=2, top_k=40)  # greedy: accepted, and no filtered row
    assert [(r.settings.top_k, r.settings.min_p, r.settings.filtered) for r in eng.sched.queue] == [(0, 0.0, False), (40, 0.1, True), (40, 0.0, False)]
    eng2 = FakeEngine(FakeModel(), max_live=2, chunk=4)
    seen = []
    eng2._step = lambda plan: seen.extend((r.settings.top_k, r.settings.min_p) for r in plan.rows) or np.zeros((plan.n, plan.bucket), dtype=np.int32)
    eng2.generate([IMG] * 2, [[5]] * 2, max_tokens=3, ignore_eos=True, top_k=[0, 7], min_p=0.25)
    assert seen[:2] == [(0, 0.25), (7, 0.25)]


# ------------------------------------------------------------------ the chunk runner
class FilterRecorder(Recorder):
    def _pick_rows_filtered(self, logits, temperature_dev, top_p_dev, top_k_dev, min_p_dev, suppress_id, uniforms, out=None):
        self.calls.append(("pick_rows_filtered", logits, temperature_dev, top_p_dev, top_k_dev, min_p_dev, suppress_id, uniforms, out))


def with_filters(pick, b=2):
    return replace(pick, top_k=torch.zeros(b, dtype=torch.int32), min_p=torch.zeros(b))


@pytest.mark.parametrize("pick,logprobs", [("none", False), ("scalar", True), ("rows", False), ("rows", True)])
def test_a_sampling_record_without_the_fields_is_the_parents_chunk(pick, logprobs):
    m = FilterRecorder()
    c = make_chunk(pick=pick, logprobs=logprobs)
    assert c.pick is None or (c.pick.top_k is None and c.pick.min_p is None and not c.pick.filtered)
    run_chunk(m, c, N, "continuous", STREAM)
    want = expected_calls(m, c, N)
    assert_calls(m.calls, want + [("capture",)] + want)
    assert "pick_rows_filtered" not in {call[0] for call in m.calls} and "filtered" not in str(m.key)
    # the key, element for element, as the runner built it before the fields existed
    kv = m._kv_struct(0)
    if pick == "rows":
        pk = ("rows", c.pick.temperature.data_ptr(), c.pick.top_p.data_ptr())
    else:
        pk = None if c.pick is None else (0.5, 0.3)
    key = ("continuous", STREAM, c.b, N, 7, c.tokens.data_ptr(), c.pos.data_ptr(), m.ws.data_ptr(), kv.k, 0, m.logits.data_ptr(), False,
           pk, c.uniforms.data_ptr() if c.uniforms is not None else 0) + ("step0", None, None)
    if logprobs:
        key += ("logprobs", c.logprobs[0].data_ptr(), c.logprobs[1].data_ptr())
    assert m.key == key


def test_with_the_fields_every_step_picks_through_the_filtered_launch_and_the_key_names_them():
    m = FilterRecorder()
    plain = make_chunk(pick="rows", logprobs=True)
    c = replace(plain, pick=with_filters(plain.pick))
    assert c.pick.filtered and c.pick.per_row
    assert run_chunk(m, c, N) is False
    lg = m.logits[: c.b]
    want = []
    for i in range(N):
        want += [("step", f"step{i}", c.tokens[i], c.tokens[i + 1], c.pos, c.b, 7, m.logits, m.ws, 0),
                 ("pick_rows_filtered", lg, c.pick.temperature, c.pick.top_p, c.pick.top_k, c.pick.min_p, 7, c.uniforms[i], c.tokens[i + 1]),
                 ("logprobs", lg, c.tokens[i + 1], 7, c.logprobs[0][i], c.logprobs[1][i])]
    assert_calls(m.calls, want)
    # the key: the parent's, with the two addresses inside its pick element
    run_chunk(m, plain, N, "continuous", STREAM)
    key_plain = m.key
    run_chunk(m, c, N, "continuous", STREAM)
    key = m.key
    at = key_plain.index(("rows", plain.pick.temperature.data_ptr(), plain.pick.top_p.data_ptr()))
    assert key[:at] == key_plain[:at] and key[at + 1 :] == key_plain[at + 1 :]
    assert key[at] == key_plain[at] + ("filtered", c.pick.top_k.data_ptr(), c.pick.min_p.data_ptr())
    other = replace(c, pick=with_filters(plain.pick))
    run_chunk(m, other, N, "continuous", STREAM)
    assert m.key != key  # other tables: another graph


def test_the_fields_need_per_row_settings():
    m = FilterRecorder()
    c = make_chunk(pick="scalar")
    with pytest.raises(AssertionError):
        run_chunk(m, replace(c, pick=with_filters(c.pick)), N)
    assert not m.calls


def test_golden_greedy_captions_have_no_near_tie(golden_dir):
    """What tests/test_sampling_filters_gpu.py builds on: in the three recorded greedy captions the best two logits of
    every decision are far more than 2^-6 apart (a logit gap is the log-probability gap), so top_k = 1 must reproduce all
    of every sequence: 0 of 3 sequences fall under that test's near-tie exemption."""
    import os

    g = np.load(os.path.join(golden_dir, "tiny_seed1.npz"))
    for i in range(3):
        margins = g[f"img{i}.cap.margins"][:12]
        assert len(margins) == 12 and float(margins.min()) > 1.0 > 2.0 ** -6
