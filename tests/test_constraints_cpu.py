"""Constrained decoding without a GPU: the automaton's constructors, ``walk``, ``validate`` and ``pack`` (the packed
table walked by the numpy restatement of md_constrain_rows), every Python entry point's argument checks (before any device
work), the launch order and graph key of a chunk with a constraint record on the recording stand-in of
tests/test_decode_chunk_cpu.py, the scheduler's part -- a refilled slot starts in its request's start state -- and the
agreement of header, binding and exported symbol."""
import os
import re
from dataclasses import replace

import numpy as np
import pytest
import torch

from constraint_ref import constrain_rows
from moondream_amd import _lib
from moondream_amd.constraint import (DEAD, FORBID, FREE, TokenAutomaton, check_constraints, pack, pow2_at_least,
                                      refuse_constraints)
from moondream_amd.continuous import Request, SlotScheduler
from moondream_amd.decode_loop import Constraint, run_chunk
from moondream_amd.hf_moondream import HfMoondream
from moondream_amd.settings import RowSettings
from test_decode_chunk_cpu import N, STREAM, assert_calls, expected_calls, make_chunk
from test_logprobs_cpu import IMG, PREFIX, FakeEngine, FakeModel, host_model
from test_penalties_cpu import PenaltyRecorder, expected_with_penalty
from test_penalties_cpu import record as penalty_record

NEG_INF = np.int16(-128)
VOCAB = 1024  # the tiny model's


# ------------------------------------------------------------------ the host object
def test_constructors_and_walk():
    a = TokenAutomaton.allowed_tokens([7, 5, 9])
    assert a.edges == (((5, 0), (7, 0), (9, 0)),) and a.default == (FORBID,)
    assert a.walk([5, 9, 9, 7]) == 0 and a.walk([5, 6, 7]) == DEAD and a.walk([]) == 0
    b = TokenAutomaton.banned_tokens([3, 1])
    assert b.edges == (((1, FORBID), (3, FORBID)),) and b.default == (0,)
    assert b.walk([0, 2, 900]) == 0 and b.walk([0, 3]) == DEAD
    s = TokenAutomaton.sequence([4, 4, 8])
    assert s.n_states == 3 and s.n_edges == 3 and s.default == (FORBID,) * 3
    assert s.walk([4]) == 1 and s.walk([4, 4]) == 2 and s.walk([4, 4, 8]) == FREE and s.walk([4, 4, 8, 1, 2]) == FREE
    assert s.walk([4, 8]) == DEAD and s.walk([8], state=2) == FREE and s.walk([1], state=DEAD) == DEAD
    c = TokenAutomaton.choices([[10, 11, 12], [10, 11], [20]], eos_id=0)
    assert c.walk([10, 11]) >= 0 and c.walk([10, 11, 0]) == FREE and c.walk([10, 11, 12, 0]) == FREE and c.walk([20, 0]) == FREE
    assert c.walk([10, 0]) == DEAD and c.walk([20, 20]) == DEAD and c.walk([0]) == DEAD and c.walk([10, 11, 12, 12]) == DEAD
    q = c.walk([10, 11])
    assert sorted(t for t, n in c.edges[q] if n != FORBID) == [0, 12], "a choice that is a prefix of another keeps both"
    m = TokenAutomaton.min_tokens(3, eos_id=0)
    assert m.n_states == 3 and m.walk([5, 5]) == 2 and m.walk([5, 5, 5]) == FREE and m.walk([5, 5, 5, 0]) == FREE
    assert m.walk([5, 0]) == DEAD and m.walk([0]) == DEAD
    f = TokenAutomaton.from_states([({9: 1, 2: FORBID}, 0), ({}, FREE)])
    assert f.edges[0] == ((2, FORBID), (9, 1)) and f.walk([5, 9]) == 1 and f.walk([5, 9, 2]) == FREE and f.walk([2]) == DEAD
    for bad in (lambda: TokenAutomaton.sequence([]), lambda: TokenAutomaton.choices([], 0), lambda: TokenAutomaton.choices([[]], 0),
                lambda: TokenAutomaton.choices([[1, 0]], 0), lambda: TokenAutomaton.min_tokens(0, 0), lambda: TokenAutomaton([], [])):
        with pytest.raises(ValueError):
            bad()


def test_validate():
    for good in (TokenAutomaton.allowed_tokens([1, 2]), TokenAutomaton.banned_tokens([3]), TokenAutomaton.sequence([5, 6]),
                 TokenAutomaton.choices([[4, 5], [4]], 0), TokenAutomaton.min_tokens(4, 0),
                 TokenAutomaton.allowed_tokens([3, 4])):  # the suppressed id beside another one
        good.validate(VOCAB, 3)
    bad = [
        TokenAutomaton([[(5, 0), (4, 0)]], [FORBID]),           # not sorted
        TokenAutomaton([[(5, 0), (5, 0)]], [FORBID]),           # not unique
        TokenAutomaton.allowed_tokens([VOCAB]),                 # a token outside the vocabulary
        TokenAutomaton.allowed_tokens([-1, 4]),
        TokenAutomaton([[(5, 1)]], [FORBID]),                   # a next value that is no state
        TokenAutomaton([[(5, DEAD)]], [FORBID]),                # DEAD is never stored
        TokenAutomaton([[(5, 0)]], [-4]),
        TokenAutomaton([[]], [FORBID]),                         # nothing allowed
        TokenAutomaton.allowed_tokens([3]),                     # only the suppressed id
        TokenAutomaton.sequence([7, 3, 7]),                     # ... in a later state
        TokenAutomaton([[(5, FORBID)]], [FORBID]),
        TokenAutomaton.banned_tokens(range(0, VOCAB)),          # default-allow with everything listed as forbidden
        TokenAutomaton.banned_tokens([t for t in range(VOCAB) if t != 3]),  # ... everything but the suppressed id
    ]
    for a in bad:
        with pytest.raises(ValueError):
            a.validate(VOCAB, 3)
    TokenAutomaton.allowed_tokens([3]).validate(VOCAB, -1)  # nothing suppressed: fine
    TokenAutomaton.banned_tokens([t for t in range(VOCAB) if t != 3]).validate(VOCAB, -1)


def test_pack_rebases_and_the_reference_walks_the_table():
    a = TokenAutomaton.sequence([3, 15, 4])
    b = TokenAutomaton.from_states([({9: FORBID, 2: 1}, 0), ({1: 0, 5: FREE}, FORBID)])
    t = pack([a, b])
    assert t.starts == (0, 3) and t.n_states == 5 and t.n_edges == 7
    assert t.row_ptr.tolist() == [0, 1, 2, 3, 5, 7] and t.default_next.tolist() == [FORBID] * 3 + [3, FORBID]
    assert t.edge_tok.tolist() == [3, 15, 4, 2, 9, 1, 5] and t.edge_next.tolist() == [1, 2, FREE, 4, FORBID, 3, FREE]
    assert all(x.dtype == np.int32 for x in (t.row_ptr, t.default_next, t.edge_tok, t.edge_next))
    cont = pack([b], state0=3, edge0=3)  # the same automaton appended to a table that holds ``a``
    assert cont.starts == (3,) and cont.row_ptr.tolist() == [3, 5, 7] and cont.edge_next.tolist() == [4, FORBID, 3, FREE]
    # two rows, one in each automaton, through the restated kernel: the states are those of ``walk``, rebased
    vocab, ld = 16, 19
    table = (t.row_ptr, t.default_next, t.edge_tok, t.edge_next)
    paths = ([3, 15, 4, 7], [7, 2, 1, 2, 1, 9])
    state = np.asarray(t.starts, dtype=np.int32)
    lg0 = np.arange(2 * ld, dtype=np.int16).reshape(2, ld)
    lg, state = constrain_rows(lg0, vocab, None, None, 0, state, *table, t.n_states)
    assert state.tolist() == [0, 3]
    assert np.flatnonzero(lg[0, :vocab] != NEG_INF).tolist() == [3] and np.flatnonzero(lg[1] != lg0[1]).tolist() == [9]
    assert (lg[:, vocab:] == lg0[:, vocab:]).all()
    for j in range(6):
        toks = [p[j] if j < len(p) else 0 for p in paths]
        lg, state = constrain_rows(lg0, vocab, toks, None, 0, state, *table, t.n_states)
        for r, (auto, p) in enumerate(zip((a, b), paths)):
            want = auto.walk(p[: j + 1])
            assert state[r] == (want + t.starts[r] if want >= 0 else want), (r, j)
            if want >= 0:
                allowed = [v for v in range(vocab) if auto.next(want, v) != FORBID]
                assert np.flatnonzero(lg[r, :vocab] != NEG_INF).tolist() == allowed
            else:
                assert (lg[r] == lg0[r]).all()
    assert state.tolist() == [FREE, DEAD]
    # the rules the walk does not reach: a token that is no id, a state past the table, an idle row
    lg, st = constrain_rows(lg0, vocab, [vocab, 2], [1, -1], 0, np.asarray([3, 3], dtype=np.int32), *table, t.n_states)
    assert st.tolist() == [3, DEAD] and (lg == lg0).all()
    lg, st = constrain_rows(lg0, vocab, None, None, 0, np.asarray([5, 2], dtype=np.int32), *table, t.n_states)
    assert st.tolist() == [DEAD, 2] and (lg[0] == lg0[0]).all() and np.flatnonzero(lg[1, :vocab] != NEG_INF).tolist() == [4]
    assert pow2_at_least(1) == 16 and pow2_at_least(16) == 16 and pow2_at_least(17) == 32 and pow2_at_least(3000) == 4096


# ------------------------------------------------------------------ argument checks
def test_check_constraints():
    a, b = TokenAutomaton.sequence([5]), TokenAutomaton.banned_tokens([9])
    assert check_constraints(None, 3, VOCAB, 3) is None and check_constraints([None, None], 2, VOCAB, 3) is None
    assert check_constraints(a, 2, VOCAB, 3) == [a, a] and check_constraints([a, None, b], 3, VOCAB, 3) == [a, None, b]
    for bad in ([a], [a, b, None], "digits", 5, [a, "x"], [a, TokenAutomaton.allowed_tokens([3])],
                [TokenAutomaton.allowed_tokens([VOCAB]), None]):
        with pytest.raises(ValueError):
            check_constraints(bad, 2, VOCAB, 3)
    refuse_constraints(None, "x")
    refuse_constraints({"constraints": None}, "x")
    refuse_constraints({"constraints": [None, None]}, "x")
    with pytest.raises(ValueError, match="not served by the thing"):
        refuse_constraints({"constraints": a}, "the thing")


BAD = [{"constraints": "digits"}, {"constraints": [TokenAutomaton.sequence([5])] * 3},
       {"constraints": TokenAutomaton.allowed_tokens([3])}, {"constraints": TokenAutomaton.allowed_tokens([VOCAB])},
       {"constraints": TokenAutomaton([[(5, 0), (4, 0)]], [FORBID])}]


def test_value_errors_precede_any_device_work():
    m = host_model()  # any device work raises AttributeError
    for bad in BAD:
        for call in (lambda: m.batch_generate_ids([IMG], [[1, 2]], **bad),
                     lambda: m.batch_generate_ids_continuous([IMG], [[1, 2]], **bad),
                     lambda: m.batch_caption([IMG], settings=bad), lambda: m.batch_query([IMG], ["q"], settings=bad),
                     lambda: m.batch_generate([IMG], settings=bad), lambda: m.query_many(IMG, ["5"], settings=bad),
                     lambda: m.caption(IMG, settings=bad), lambda: m.query(IMG, "5", settings=bad),
                     lambda: FakeEngine(FakeModel(), max_live=2).generate([IMG], [[5]], **bad)):
            with pytest.raises(ValueError):
                call()
    for bad in ("digits", [TokenAutomaton.sequence([5])], TokenAutomaton.allowed_tokens([3])):
        with pytest.raises(ValueError):
            FakeEngine(FakeModel(), max_live=2).submit(IMG, [5], constraint=bad)
    with pytest.raises(ValueError, match="full"):
        FakeEngine(FakeModel(), max_live=2, constraint_states=4).submit(IMG, [5], constraint=TokenAutomaton.sequence([5] * 5))
    with pytest.raises(ValueError, match="full"):
        FakeEngine(FakeModel(), max_live=2, constraint_edges=2).submit(IMG, [5], constraint=TokenAutomaton.allowed_tokens([5, 6, 7]))
    with pytest.raises(ValueError):
        FakeEngine(FakeModel(), max_live=2, constraint_states=0)


def test_what_is_not_served_says_so():
    m = host_model()
    on = {"constraints": TokenAutomaton.sequence([5, 6])}
    hf = object.__new__(HfMoondream)
    refused = [lambda: m.batch_query([IMG], ["q"], settings=on, reasoning=True), lambda: m.query(IMG, "q", reasoning=True, settings=on),
               lambda: m.query_many_reasoning(IMG, ["q"], settings=on),
               lambda: m.batch_detect([IMG], ["cat"], settings=on), lambda: m.batch_point([IMG], ["cat"], settings=on),
               lambda: m.detect_many(IMG, ["cat"], settings=on), lambda: m.point_many(IMG, ["cat"], settings=on),
               lambda: m.detect(IMG, "cat", settings=on), lambda: m.point(IMG, "cat", settings=on),
               lambda: next(m.batch_detect_pipelined([([IMG], ["cat"])], settings=on)),
               lambda: m.batch_generate_ids_pipelined([([IMG], [[1, 2]])], constraints=on["constraints"]),
               lambda: m.score_ids([IMG], [[1, 2]], [[5]], constraints=on["constraints"]),
               lambda: hf.answer_question(IMG, "q", settings=on), lambda: hf.batch_answer([IMG], ["q"], settings=on),
               lambda: hf.generate(IMG, "p", settings=on)]
    for call in refused:
        with pytest.raises(ValueError, match="not served"):
            call()


def test_choice_constraint_uses_the_models_tokenizer_and_eos():
    m = host_model()
    a = m.choice_constraint(["10 11", "20"])
    eos = m.config.tokenizer.eos_id
    assert a.walk([10, 11, eos]) == FREE and a.walk([20, eos]) == FREE and a.walk([10, eos]) == DEAD
    a.validate(m.config.text.vocab_size, m.config.tokenizer.answer_id)


# ------------------------------------------------------------------ the chunk runner
class ConstraintRecorder(PenaltyRecorder):
    def _constrain(self, logits, tok_in, rows, con, row0=0):
        self.calls.append(("constrain", logits, tok_in, rows.name, con))


def record(b=2, by_slot=False, s_cap=16, e_cap=16):
    z = lambda n: torch.zeros(n, dtype=torch.int32)
    return Constraint(z(s_cap + 1), z(s_cap), z(e_cap), z(e_cap), z(b), s_cap, by_slot)


def expected_with_constraint(m, c, n):
    """The penalties' expectation with the constraint launch after the penalty's and before the pick."""
    out = []
    for call in expected_with_penalty(m, c, n):
        if call[0] == "penalize" and c.penalty is None:
            continue
        if call[0] in ("pick", "pick_rows"):
            step = len([x for x in out if x[0] == "step"]) - 1
            out.append(("constrain", m.logits[: c.b], c.tokens[step], f"step{step}", c.constraint))
        out.append(call)
    return out


@pytest.mark.parametrize("pick", ["none", "scalar", "rows"])
@pytest.mark.parametrize("scored", [False, True])
@pytest.mark.parametrize("penalised", [False, True])
def test_step_then_penalty_then_constraint_then_pick_then_logprobs_then_topk(pick, scored, penalised):
    m = ConstraintRecorder()
    c = make_chunk(pick=pick, logprobs=scored, constraint=record(), penalty=penalty_record() if penalised else None)
    if scored:
        c = replace(c, topk=(torch.zeros(N + 2, 2, 3, dtype=torch.int32), torch.zeros(N + 2, 2, 3)))
    assert run_chunk(m, c, N) is False
    want = expected_with_constraint(m, c, N)
    assert_calls(m.calls, want)
    assert [x[0] for x in want[: len(want) // N]] == ["step"] + (["penalize"] if penalised else []) + [
        "constrain", "pick_rows" if pick == "rows" else "pick"] + (["logprobs", "topk"] if scored else [])
    assert all(call[4] is c.constraint for call in m.calls if call[0] == "constrain")
    if pick == "none":  # greedy: the fused step's argmax saw the raw logits -- the argmax launch again
        assert [call[2:4] for call in m.calls if call[0] == "pick"] == [(0.0, 0.0)] * N


def test_a_step_from_pieces_is_constrained_too():
    """The eager LoRA step: the constraint launch takes the logits that step returned."""
    m = ConstraintRecorder()
    lg = torch.zeros(2, 11)
    c = make_chunk(pick="scalar", constraint=record(), step=lambda tok_in: lg)
    run_chunk(m, c, N)
    assert [call[0] for call in m.calls] == ["constrain", "pick"] * N
    assert all(call[1] is lg for call in m.calls)


@pytest.mark.parametrize("pick,logprobs", [("none", False), ("scalar", True), ("rows", False)])
def test_without_a_record_launches_and_key_are_todays(pick, logprobs):
    m = ConstraintRecorder()
    c = make_chunk(pick=pick, logprobs=logprobs)
    assert c.constraint is None
    run_chunk(m, c, N, "continuous", STREAM)
    want = expected_calls(m, c, N)
    assert_calls(m.calls, want + [("capture",)] + want)
    assert "constrain" not in {call[0] for call in m.calls} and "constraint" not in m.key
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
    # with a record: the same key, then the record's part (after a penalty's); another record, another key
    con = record()
    run_chunk(m, replace(c, constraint=con), N, "continuous", STREAM)
    assert m.key[: len(key)] == key and m.key[len(key)] == "constraint" and m.key[len(key) :] == con.key()
    pen = penalty_record()
    run_chunk(m, replace(c, constraint=con, penalty=pen), N, "continuous", STREAM)
    assert m.key == key + pen.key() + con.key()
    for other in (replace(con, state=torch.zeros_like(con.state)), replace(con, row_ptr=torch.zeros_like(con.row_ptr)),
                  replace(con, default_next=torch.zeros_like(con.default_next)), replace(con, edge_tok=torch.zeros_like(con.edge_tok)),
                  replace(con, edge_next=torch.zeros_like(con.edge_next)), replace(con, state_cap=8), replace(con, by_slot=True)):
        assert other.key() != con.key()


def test_the_single_sequence_kernel_is_never_combined_with_constraints():
    m = ConstraintRecorder()
    with pytest.raises(AssertionError):
        run_chunk(m, make_chunk(b=1, b1=True, constraint=record(1)), N)
    assert not m.calls


# ------------------------------------------------------------------ the continuous engine's part
def test_scheduler_resets_a_refilled_slots_state():
    """Two slots, five requests, three of them constrained: kept as the engine keeps it -- ``state_resets`` applied
    before a chunk, every live row's state advanced per step -- a request's slot holds the request's OWN state (start
    state plus its own steps) in every chunk, never what the slot's last occupant left, and a free request's is FREE."""
    s = SlotScheduler(max_live=2, max_context=2048, chunk=4)
    limits = [6, 3, 9, 2, 5]
    starts = [100, FREE, 200, 300, FREE]
    for rid, (n, st) in enumerate(zip(limits, starts)):
        s.submit(Request(rid, IMG, [5], n, None, settings=RowSettings(constraint=None if st == FREE else TokenAutomaton.sequence([1])),
                         constraint_start=st))
    spare = 2
    state = np.full(3, 777, dtype=np.int64)  # slot 0, slot 1, the spare entry
    refills = 0

    def step(plan):
        nonlocal refills
        idx, val = SlotScheduler.state_resets(plan, spare)
        assert idx.shape == val.shape == (plan.bucket,) and idx.dtype == np.int64 and val.dtype == np.int32
        for i, r in enumerate(plan.rows):
            if r.steps == 0:
                assert (idx[i], val[i]) == (r.slot, r.constraint_start)
                refills += state[r.slot] != 777
            else:
                assert (idx[i], val[i]) == (spare, FREE)
        assert (idx[len(plan.rows) :] == spare).all() and (val[len(plan.rows) :] == FREE).all()
        state[idx] = val
        for r in plan.rows:
            assert state[r.slot] == (FREE if r.settings.constraint is None else r.constraint_start + r.steps), (r.rid, state)
        for row in plan.slots:  # a step of the stand-in automaton: a constrained state counts its tokens
            live = row[row >= 0]
            state[live] += state[live] >= 0
        return np.full((plan.n, plan.bucket), 7, dtype=np.int32)

    done = list(s.run(lambda reqs: [(100 + r.rid, PREFIX + 1) for r in reqs], step))
    assert sorted(r.rid for r in done) == list(range(5)) and refills >= 3


def test_engine_takes_a_constraint_per_request_and_packs_each_automaton_once():
    model = FakeModel()
    model.tokenizer = host_model().tokenizer
    eng = FakeEngine(model, max_live=2, chunk=4)
    a, b = TokenAutomaton.sequence([5, 6, 7]), TokenAutomaton.allowed_tokens([8, 9])
    eng.submit(IMG, [5], max_tokens=2)
    eng.submit(IMG, [5], max_tokens=2, constraint=a)
    eng.submit_caption(IMG, max_tokens=2, constraint=b)
    eng.submit_query(IMG, "5 6", max_tokens=2, constraint=a)
    assert [(r.settings.constraint, r.constraint_start) for r in eng.sched.queue] == [(None, FREE), (a, 0), (b, 3), (a, 0)]
    assert eng._con_used == [4, 5] and eng._con_pending == [a, b]
    list(eng.run())
    seen = []
    eng._step = lambda plan: seen.extend((r.settings.constraint, r.constraint_start) for r in plan.rows) or np.zeros((plan.n, plan.bucket), dtype=np.int32)
    eng.generate([IMG] * 2, [[5]] * 2, max_tokens=3, ignore_eos=True, constraints=[b, None])
    assert seen[:2] == [(b, 3), (None, FREE)] and eng._con_used == [4, 5]
    with pytest.raises(ValueError):
        eng.generate([IMG] * 2, [[5]] * 2, constraints=[a])


# ------------------------------------------------------------------ header, binding, symbol
def test_header_binding_and_symbol_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "moondream_hip.h")).read()
    assert re.search(r"#define\s+MD_ABI_VERSION\s+5\b", text) and _lib.ABI_VERSION == 5
    m = re.search(r"md_status\s+md_constrain_rows\s*\(([^;]*)\)\s*;", text)
    assert m, "md_constrain_rows is declared in the header"
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).split(",")]
    kinds = ["ptr" if "*" in p else p.split()[0] for p in params]
    want = ["ptr", "int64_t", "int32_t", "int32_t", "ptr", "ptr", "int32_t", "ptr", "ptr", "ptr", "ptr", "ptr", "int32_t", "ptr"]
    assert kinds == want
    c = {"ptr": _lib.c_void_p, "int64_t": _lib.c_int64, "int32_t": _lib.c_int32}
    res, args = _lib.SIGNATURES["md_constrain_rows"]
    assert args == [c[k] for k in want]
    assert int(re.search(r"#define\s+MD_CONSTRAIN_VOCAB_MAX\s+(\d+)", text).group(1)) == _lib.MD_CONSTRAIN_VOCAB_MAX
    for name, val in (("FREE", FREE), ("DEAD", DEAD), ("FORBID", FORBID)):
        assert int(re.search(rf"#define\s+MD_CONSTRAINT_{name}\s+\((-\d+)\)", text).group(1)) == val
    lib = _lib.load()
    assert lib.md_abi_version() == 5 and hasattr(lib, "md_constrain_rows")


def test_entry_point_rejects_bad_arguments_without_a_device():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.int32).ctypes.data  # a non-NULL address: nothing is launched, nothing reads it
    good = dict(logits=buf, ld=8, batch=1, vocab=8, tokens_in=buf, slots=None, slot0=0, state=buf, row_ptr=buf, default_next=buf,
                edge_tok=buf, edge_next=buf, state_cap=4)
    call = lambda **kw: lib.md_constrain_rows(*{**good, **kw}.values(), None)
    for name in ("logits", "state", "row_ptr", "default_next", "edge_tok", "edge_next"):
        assert call(**{name: None}) == 1, name  # MD_ERR_INVALID_ARG
    assert call(batch=-1) == 1 and call(vocab=0) == 1 and call(ld=7) == 1 and call(state_cap=0) == 1
    big = _lib.MD_CONSTRAIN_VOCAB_MAX + 1
    assert call(vocab=big, ld=big) == 1
    assert call(batch=0) == 0 and call(batch=0, tokens_in=None) == 0  # MD_OK, nothing launched
