"""Repetition / presence / frequency penalties without a GPU: the numpy restatement of md_penalize_rows' rule against
hand-worked values, the entry point's and every Python entry point's argument checks (before any device work), the
launch order and graph key of a chunk with a penalty record on the recording stand-in of tests/test_decode_chunk_cpu.py,
and the scheduler's part: a refilled slot's history starts empty."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from moondream_amd import _lib
from moondream_amd.continuous import IDLE_SLOT, ContinuousEngine, Request, SlotScheduler
from moondream_amd.decode_loop import PENALTY_NEUTRAL, Penalty, Sampling, check_penalties, penalties_of, refuse_penalties, run_chunk
from moondream_amd.hf_moondream import HfMoondream
from penalty_ref import bf16_bits_to_f32, f32_to_bf16_bits, penalize_rows, penalize_value
from test_decode_chunk_cpu import N, STREAM, Recorder, assert_calls, expected_calls, make_chunk
from test_logprobs_cpu import IMG, PREFIX, FakeEngine, FakeModel, host_model
from util import bits_to_bf16

F = np.float32


# ------------------------------------------------------------------ the restatement
def test_restatement_against_hand_worked_values():
    assert penalize_value(6.0, 5, 1.0, 0.0, 0.5) == F(3.5)
    assert penalize_value(6.0, 1, 2.0, 0.0, 0.0) == F(3.0) and penalize_value(-6.0, 1, 2.0, 0.0, 0.0) == F(-12.0)
    assert penalize_value(6.0, 1, 0.5, 0.0, 0.0) == F(12.0) and penalize_value(-6.0, 1, 0.5, 0.0, 0.0) == F(-3.0)
    assert penalize_value(0.0, 3, 1.7, 0.0, 0.0) == F(0.0)  # zero stays zero under the repetition rule
    assert penalize_value(0.0, 3, 1.7, 0.25, 0.5) == F(-1.75)
    assert penalize_value(1.0, 2, 1.0, -1e4, 4e3) == F(2001.0)  # a negative presence penalty is a bonus
    assert penalize_value(float("-inf"), 2, 1.3, -5.0, 1.0) == F("-inf")
    # separately rounded: 0.1f * 3 is rounded before the add (a fused multiply-add would give another last bit)
    p = F(F(0.3) + F(F(0.1) * F(3)))
    assert penalize_value(1.0, 3, 1.0, 0.3, 0.1) == F(F(1.0) - p)
    # 6 / 0.7 = 8.5714.. ; - 2.5 = 6.0714.. ; bf16 (spacing 1/32 in [4, 8)): 6.0625
    assert bf16_bits_to_f32(f32_to_bf16_bits(np.array([penalize_value(6.0, 5, 0.7, 0.0, 0.5)])))[0] == F(6.0625)
    # round to nearest EVEN: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 -> 1; 1 + 3 * 2^-8 is a tie -> 1 + 2^-6
    assert bf16_bits_to_f32(f32_to_bf16_bits(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=F))).tolist() == [1.0, 1 + 2.0 ** -6]


def test_restatement_of_a_launch():
    vocab, ld = 16, 19
    lg = f32_to_bf16_bits(np.arange(3 * ld, dtype=F).reshape(3, ld) - 20)
    hist = np.full((4, 4), -9, dtype=np.int32)
    hist[2, :2], hist[0, :4] = [5, 5], [1, 2, 3, 1]
    lens = np.array([4, 0, 2, 0], dtype=np.int32)
    out, h, n = penalize_rows(lg, vocab, [7, 9, 5], [2, -1, 0], 0, hist, lens, [1.0, 2.0, 2.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0])
    assert n.tolist() == [4, 0, 3, 0] and h[2, :3].tolist() == [5, 5, 7] and (h[[0, 1, 3]] == hist[[0, 1, 3]]).all()
    val = lambda bits: bf16_bits_to_f32(bits).tolist()
    assert (out[1] == lg[1]).all()  # idle
    # row 0 (slot 2): token 5 twice, token 7 once, frequency 1
    assert val(out[0, [5, 7]]) == [-15.0 - 2.0, -13.0 - 1.0] and (np.delete(out[0], [5, 7]) == np.delete(lg[0], [5, 7])).all()
    # row 2 (slot 0, full: 5 is dropped): tokens 1, 2, 3 at repetition 2 -- logits 19, 20, 21 are positive: halved
    assert val(out[2, [1, 2, 3]]) == [9.5, 10.0, 10.5] and out[2, 5] == lg[2, 5]


# ------------------------------------------------------------------ argument checks
def test_check_penalties():
    assert check_penalties(1.0, 0.0, 0.0, 3) is None and check_penalties(None, None, None, 2) is None
    assert check_penalties([1, 1], 0, np.float32(0), 2) is None
    assert check_penalties(1.2, 0.0, [0.0, -0.5], 2) == [(1.2, 0.0, 0.0), (1.2, 0.0, -0.5)]
    assert check_penalties(1, -1e4, 4e3, 1) == [(1.0, -1e4, 4e3)]
    for bad in ((0.0, 0, 0), (-1.0, 0, 0), (float("nan"), 0, 0), (float("inf"), 0, 0), (1, float("inf"), 0), (1, 0, float("nan")),
                ([1.0], 0, 0), (1, [0.0] * 3, 0), ("x", 0, 0), (1, object(), 0), (True, 0, 0)):
        with pytest.raises(ValueError):
            check_penalties(*bad, 2)
    assert penalties_of(None) == dict(zip(("repetition_penalty", "presence_penalty", "frequency_penalty"), PENALTY_NEUTRAL))
    refuse_penalties({"presence_penalty": 0.0, "repetition_penalty": 1}, "x")
    with pytest.raises(ValueError, match="not served by the thing"):
        refuse_penalties({"frequency_penalty": 0.1}, "the thing")


def test_entry_point_rejects_bad_arguments_without_a_device():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.int32).ctypes.data  # a non-NULL address: nothing is launched, nothing reads it
    good = dict(logits=buf, ld=8, batch=1, vocab=8, tokens_in=buf, slots=None, slot0=0, hist=buf, hist_cap=4, hist_len=buf,
                repetition=buf, presence=buf, frequency=buf)
    call = lambda **kw: lib.md_penalize_rows(*{**good, **kw}.values(), None)
    for name in ("logits", "tokens_in", "hist", "hist_len", "repetition", "presence", "frequency"):
        assert call(**{name: None}) == 1, name  # MD_ERR_INVALID_ARG
    assert call(batch=-1) == 1 and call(vocab=0) == 1 and call(ld=7) == 1 and call(hist_cap=0) == 1
    assert call(hist_cap=_lib.MD_PENALTY_HIST_MAX + 1) == 1
    assert call(batch=0) == 0  # MD_OK, nothing launched
    assert lib.md_abi_version() == 5


BAD = [{"repetition_penalty": 0.0}, {"repetition_penalty": float("nan")}, {"presence_penalty": float("inf")},
       {"frequency_penalty": "much"}]


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
    with pytest.raises(ValueError):
        m.batch_generate_ids([IMG, IMG], [[1, 2], [1, 2]], presence_penalty=[0.5])  # one per row
    with pytest.raises(ValueError):
        FakeEngine(FakeModel(), max_live=2).submit(IMG, [5], presence_penalty=[0.5])  # one number per request


def test_what_is_not_served_says_so():
    m = host_model()
    on = {"presence_penalty": 0.5}
    hf = object.__new__(HfMoondream)
    refused = [lambda: m.batch_query([IMG], ["q"], settings=on, reasoning=True), lambda: m.query(IMG, "q", reasoning=True, settings=on),
               lambda: m.query_many_reasoning(IMG, ["q"], settings=on),
               lambda: m.batch_detect([IMG], ["cat"], settings=on), lambda: m.batch_point([IMG], ["cat"], settings=on),
               lambda: m.detect_many(IMG, ["cat"], settings=on), lambda: m.point_many(IMG, ["cat"], settings=on),
               lambda: m.detect(IMG, "cat", settings=on), lambda: m.point(IMG, "cat", settings=on),
               lambda: next(m.batch_detect_pipelined([([IMG], ["cat"])], settings=on)),
               lambda: m.batch_generate_ids_pipelined([([IMG], [[1, 2]])], frequency_penalty=0.5),
               lambda: m.score_ids([IMG], [[1, 2]], [[5]], repetition_penalty=1.2),
               lambda: hf.answer_question(IMG, "q", settings=on), lambda: hf.batch_answer([IMG], ["q"], settings=on),
               lambda: hf.generate(IMG, "p", settings=on)]
    for call in refused:
        with pytest.raises(ValueError, match="not served"):
            call()


# ------------------------------------------------------------------ the chunk runner
class PenaltyRecorder(Recorder):
    def _penalize(self, logits, tok_in, rows, pen):
        self.calls.append(("penalize", logits, tok_in, rows.name, pen))

    def _topk_logprobs(self, logits, gate, suppress_id, top_ids, top_logprobs, suppress_rows=None):
        self.calls.append(("topk", logits, gate, suppress_id, top_ids, top_logprobs))


def record(b=2, by_slot=False):
    return Penalty(torch.ones(b), torch.zeros(b), torch.zeros(b), torch.zeros(b, 16, dtype=torch.int32),
                   torch.zeros(b, dtype=torch.int32), 16, by_slot)


def expected_with_penalty(m, c, n):
    lg = m.logits[: c.b]
    out = []
    for i in range(n):
        tin, tout = c.tokens[i], c.tokens[i + 1]
        out.append(("step", f"step{i}", tin, tout, c.pos, c.b, 7, m.logits, m.ws, 0))
        out.append(("penalize", lg, tin, f"step{i}", c.penalty))
        if c.pick is not None and c.pick.per_row:
            out.append(("pick_rows", lg, c.pick.temperature, c.pick.top_p, 7, c.uniforms[i], tout))
        elif c.pick is not None:
            out.append(("pick", lg, 0.5, 0.3, 7, None, c.uniforms[i], tout))
        else:  # greedy: the fused step's argmax saw the raw logits -- the argmax launch again
            out.append(("pick", lg, 0.0, 0.0, 7, None, None, tout))
        if c.logprobs is not None:
            out.append(("logprobs", lg, tout, 7, c.logprobs[0][i], c.logprobs[1][i]))
        if c.topk is not None:
            out.append(("topk", lg, tout, 7, c.topk[0][i], c.topk[1][i]))
    return out


@pytest.mark.parametrize("pick", ["none", "scalar", "rows"])
@pytest.mark.parametrize("scored", [False, True])
def test_step_then_penalise_then_pick_then_logprobs_then_topk(pick, scored):
    m = PenaltyRecorder()
    c = make_chunk(pick=pick, logprobs=scored, penalty=record())
    if scored:
        c = replace(c, topk=(torch.zeros(N + 2, 2, 3, dtype=torch.int32), torch.zeros(N + 2, 2, 3)))
    assert run_chunk(m, c, N) is False
    want = expected_with_penalty(m, c, N)
    assert_calls(m.calls, want)
    assert [x[0] for x in want[: len(want) // N]] == ["step", "penalize", "pick_rows" if pick == "rows" else "pick"] + \
           (["logprobs", "topk"] if scored else [])
    assert all(call[4] is c.penalty for call in m.calls if call[0] == "penalize")


@pytest.mark.parametrize("pick,logprobs", [("none", False), ("scalar", True), ("rows", False)])
def test_without_a_record_launches_and_key_are_todays(pick, logprobs):
    m = PenaltyRecorder()
    c = make_chunk(pick=pick, logprobs=logprobs)
    assert c.penalty is None
    run_chunk(m, c, N, "continuous", STREAM)
    want = expected_calls(m, c, N)
    assert_calls(m.calls, want + [("capture",)] + want)
    assert "penalize" not in {call[0] for call in m.calls} and "penalty" not in m.key
    # the key, element for element, as the runner has always built it
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
    # with a record: the same key, then the record's part; another record, another key
    pen = record()
    run_chunk(m, replace(c, penalty=pen), N, "continuous", STREAM)
    assert m.key[: len(key)] == key and m.key[len(key)] == "penalty" and m.key[len(key) :] == pen.key()
    for other in (replace(pen, hist=torch.zeros_like(pen.hist)), replace(pen, hist_len=torch.zeros_like(pen.hist_len)),
                  replace(pen, presence=torch.zeros_like(pen.presence)), replace(pen, hist_cap=8), replace(pen, by_slot=True)):
        assert other.key() != pen.key()


def test_the_single_sequence_kernel_is_never_combined_with_penalties():
    m = PenaltyRecorder()
    with pytest.raises(AssertionError):
        run_chunk(m, make_chunk(b=1, b1=True, penalty=record(1)), N)
    assert not m.calls


# ------------------------------------------------------------------ the continuous engine's part
def test_scheduler_marks_a_refilled_slot_and_its_history_starts_empty():
    """Two slots, five requests: every request's first chunk names its slot in ``plan.fresh``, later chunks do not.  Kept
    as the engine keeps it -- fresh slots' lengths zeroed before the chunk, every live row's slot one token longer per
    step -- the length of a request's slot is the number of tokens it has generated itself."""
    s = SlotScheduler(max_live=2, max_context=2048, chunk=4)
    limits = [6, 3, 9, 2, 5]
    for rid, n in enumerate(limits):
        s.submit(Request(rid, IMG, [5], n, None))
    hist_len = np.zeros(2, dtype=np.int64)
    first_chunk_seen, reused = set(), 0
    slot_users = {0: [], 1: []}

    def admit(reqs):
        for r in reqs:
            slot_users[r.slot].append(r.rid)
        return [(100 + r.rid, PREFIX + 1) for r in reqs]

    def step(plan):
        nonlocal reused
        assert plan.fresh.shape == (plan.bucket,) and plan.fresh.dtype == np.int32
        for i, r in enumerate(plan.rows):
            assert plan.fresh[i] == (r.slot if r.rid not in first_chunk_seen else IDLE_SLOT), (r.rid, plan.fresh)
            if r.rid not in first_chunk_seen and hist_len[r.slot] > 0:
                reused += 1  # the previous user of the slot left its tokens behind
            first_chunk_seen.add(r.rid)
        assert (plan.fresh[len(plan.rows) :] == IDLE_SLOT).all()
        hist_len[plan.fresh[plan.fresh >= 0]] = 0
        for i, r in enumerate(plan.rows):
            assert hist_len[r.slot] == len(r.ids) - 1, (r.rid, hist_len, r.ids)  # all but the token step 0 consumes
        hist_len[:] += np.bincount(plan.slots[plan.slots >= 0], minlength=2)
        return np.full((plan.n, plan.bucket), 7, dtype=np.int32)

    done = list(s.run(admit, step))
    assert sorted(r.rid for r in done) == list(range(5)) and [len(r.ids) for r in sorted(done, key=lambda r: r.rid)] == limits
    assert reused >= 3 and all(len(u) >= 2 for u in slot_users.values())


def test_engine_takes_the_settings_per_request():
    eng = FakeEngine(FakeModel(), max_live=2, chunk=4)
    eng.submit(IMG, [5], max_tokens=2)
    eng.submit(IMG, [5], max_tokens=2, repetition_penalty=1.3, frequency_penalty=-0.5)
    assert [r.settings.penalties for r in eng.sched.queue] == [PENALTY_NEUTRAL, (1.3, 0.0, -0.5)]
    list(eng.run())
    eng.generate([IMG] * 3, [[5]] * 3, max_tokens=0, presence_penalty=[0.0, 1.0, 0.0], repetition_penalty=2)
    eng2 = FakeEngine(FakeModel(), max_live=2, chunk=4)
    seen = []
    eng2._step = lambda plan: seen.extend(r.settings.penalties for r in plan.rows) or np.zeros((plan.n, plan.bucket), dtype=np.int32)
    eng2.generate([IMG] * 2, [[5]] * 2, max_tokens=3, ignore_eos=True, presence_penalty=[0.0, 1.0], repetition_penalty=2)
    assert seen[:2] == [(2.0, 0.0, 0.0), (2.0, 1.0, 0.0)]


def test_golden_greedy_captions_never_repeat_a_token(golden_dir):
    """What tests/test_penalties_gpu.py builds on: a positive penalty cannot change these greedy ids, so its end-to-end
    checks use boosts."""
    import os

    g = np.load(os.path.join(golden_dir, "tiny_seed1.npz"))
    for i in range(3):
        toks = g[f"img{i}.cap.tokens"].tolist()
        assert len(toks) == 24 and len(set(toks)) == 24
