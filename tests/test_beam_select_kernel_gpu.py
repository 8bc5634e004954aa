"""md_beam_select on the MI355X through the C ABI against tests/beam_ref.py, EXACT: every state array, every output array
and the candidate scratch, bit for bit (floats compared as their 32-bit patterns).  The oracle takes md_topk_logprobs' own
output on the same logits (pinned by tests/test_topk_logprobs_gpu.py) and does the merge, walk, pool, done rule and slot
hand-off in numpy fp32."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_ref as ref
from moondream_amd import _lib

pytestmark = pytest.mark.gpu
MD_ERR_INVALID_ARG = 1  # include/moondream_hip.h
GROUPS = 3
POISON = -7  # what an output a call must not write holds (beam_ref.select's default)
STATE = ("cum", "cur", "own", "len", "done", "prefix_len", "pool_n", "pool_score", "pool_sum", "pool_parent", "pool_step")
OUT = ("tokens", "parent", "src", "dst", "from", "to")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def bf16_rows(x, ld=None):
    """float array [rows][vocab] -> device bf16 [rows][ld] (padding columns NaN)."""
    t = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16)
    full = torch.full((t.shape[0], ld or t.shape[1]), float("nan"), dtype=torch.bfloat16)
    full[:, : t.shape[1]] = t
    return full.cuda()


def random_logits(rows, vocab, seed, eos=None, boost_rows=()):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((rows, vocab)) * 4.0).astype(np.float32)
    for r in boost_rows:
        x[r, eos] = 30.0
    return x


def topk(lib, d_lg, vocab, k, suppress_id, gate):
    rows = d_lg.shape[0]
    ids = torch.zeros(rows, k, dtype=torch.int32).cuda()
    lp = torch.zeros(rows, k, dtype=torch.float32).cuda()
    st = lib.md_topk_logprobs(d_lg.data_ptr(), d_lg.stride(0), rows, vocab, suppress_id, None, dev(np.asarray(gate, np.int32)).data_ptr(),
                              k, ids.data_ptr(), lp.data_ptr(), stream())
    assert st == 0, st
    torch.cuda.synchronize()
    return ids.cpu().numpy(), lp.cpu().numpy()


def step(lib, state, logits, vocab, w, beams_in, eos, early, inv_norm, suppress_id=-1, prev_out=None, ld=None):
    """One md_beam_select call on copies of ``state``, compared whole with the oracle; returns the oracle's (state, out)."""
    rows = GROUPS * w
    k = 2 * w
    d_lg = bf16_rows(logits, ld)
    assert d_lg.shape[0] == (GROUPS if beams_in == 1 else rows)
    # the oracle's candidates: md_topk_logprobs on each live beam's logits row; a dead beam's row is gated off (-1 / NaN)
    live = [(r % w) < beams_in and state["cum"][r] != ref.NEG_INF for r in range(rows)]
    if beams_in == 1:
        t_ids, t_lp = topk(lib, d_lg, vocab, k, suppress_id, [0 if live[g * w] else -1 for g in range(GROUPS)])
        off_ids, off_lp = topk(lib, d_lg[:1], vocab, k, suppress_id, [-1])
        cand_ids = np.repeat(off_ids, rows, 0)
        cand_lp = np.repeat(off_lp, rows, 0)
        cand_ids[::w], cand_lp[::w] = t_ids, t_lp
    else:
        cand_ids, cand_lp = topk(lib, d_lg, vocab, k, suppress_id, [0 if x else -1 for x in live])
    want_state, want_out = ref.select(state, cand_ids, cand_lp, w, beams_in, eos, early, inv_norm, prev_out)
    ref.check_copy_contract(want_out)

    d = {n: dev(state[n]) for n in STATE}
    d_norm = dev(inv_norm)
    d_cand_ids = torch.full((rows, k), POISON, dtype=torch.int32).cuda()
    d_cand_lp = torch.full((rows, k), float(POISON), dtype=torch.float32).cuda()
    d_out = {n: dev(prev_out[n] if prev_out is not None else np.full(rows, POISON, np.int32)) for n in OUT}
    st = _lib.MdBeamState(*(d[n].data_ptr() for n in STATE), d_norm.data_ptr(), len(inv_norm), d_cand_ids.data_ptr(),
                          d_cand_lp.data_ptr())
    status = lib.md_beam_select(d_lg.data_ptr(), d_lg.stride(0), GROUPS, w, beams_in, vocab, suppress_id, None, eos, int(early),
                                C.byref(st), *(d_out[n].data_ptr() for n in OUT), stream())
    assert status == 0, status
    torch.cuda.synchronize()
    for n in STATE:
        got, want = bits(d[n].cpu().numpy()), bits(want_state[n])
        assert np.array_equal(got, want), (n, d[n].cpu().numpy().tolist(), want_state[n].tolist())
    for n in OUT:
        assert np.array_equal(d_out[n].cpu().numpy(), want_out[n]), (n, d_out[n].cpu().tolist(), want_out[n].tolist())
    # the scratch: md_topk_logprobs' entries bit for bit; a done group's rows untouched
    for g in range(GROUPS):
        sl = slice(g * w, (g + 1) * w)
        if state["done"][g]:
            assert (d_cand_ids[sl].cpu().numpy() == POISON).all() and (d_cand_lp[sl].cpu().numpy() == POISON).all()
        else:
            assert np.array_equal(d_cand_ids[sl].cpu().numpy(), cand_ids[sl])
            assert np.array_equal(bits(d_cand_lp[sl].cpu().numpy()), bits(cand_lp[sl]))
    return want_state, want_out


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("w", [1, 2, 3, 4, 16])
def test_random_steps(lib, w, early):
    """Vocabulary 37 (no multiple of 8, ld 40), 3 groups: the first decision (beams_in 1) and four more over fresh logits,
    the eos boosted in some rows so that hypotheses finish; answer_id-style suppression from the second decision on."""
    vocab, eos = 37, 5
    norm = ref.inv_norm_table(16, 1.3)
    state = ref.new_state(GROUPS, w, [11, 3, 20])
    state, out = step(lib, state, random_logits(GROUPS, vocab, 1), vocab, w, 1, eos, early, norm, ld=40)
    assert (out["to"] == out["from"]).all()  # nothing to move yet
    pooled = 0
    for t in range(4):
        boost = [r for r in range(GROUPS * w) if (r + t) % 3 == 0]
        state, out = step(lib, state, random_logits(GROUPS * w, vocab, 10 + t, eos, boost), vocab, w, w, eos, early, norm,
                          suppress_id=3, prev_out=out, ld=40)
        pooled = max(pooled, int(state["pool_n"].max()))
    assert pooled >= 1


def test_large_vocabulary(lib):
    vocab, w, eos = 51200, 4, 0
    norm = ref.inv_norm_table(8, 1.0)
    state = ref.new_state(GROUPS, w, [730, 731, 740])
    state, out = step(lib, state, random_logits(GROUPS, vocab, 3), vocab, w, 1, eos, False, norm)
    step(lib, state, random_logits(GROUPS * w, vocab, 4, eos, [1, 6]), vocab, w, w, eos, False, norm, suppress_id=3, prev_out=out)


def test_tie_order(lib):
    """Equal bf16 logits in every row and equal cum: every candidate has one score.  The order is beam ascending, then
    entry ascending -- so all 2W walked candidates are beam 0's, tokens 0, 1, .. in id order."""
    vocab, w = 37, 3
    norm = ref.inv_norm_table(8, 1.0)
    state = ref.new_state(GROUPS, w, [4, 4, 4])
    state["cum"][:] = np.float32(-1.5)
    state["len"][:] = 2
    state, out = step(lib, state, np.zeros((GROUPS * w, vocab), np.float32), vocab, w, w, -1, False, norm)
    assert out["parent"].tolist() == [0] * (GROUPS * w)
    assert out["tokens"].tolist() == [0, 1, 2] * GROUPS
    # equal scores across beams only: each row has ONE token that is not -inf (log-probability exactly 0 wherever it sits),
    # so the rows' best scores are equal -> beams in ascending order; the -inf candidates exist and come after them
    x = np.full((GROUPS * w, vocab), -np.inf, np.float32)
    for r in range(GROUPS * w):
        x[r, 30 - r] = 20.0
    state2 = ref.new_state(GROUPS, w, [4, 4, 4])
    state2["cum"][:] = np.float32(-1.5)
    state2["len"][:] = 2
    state2, out2 = step(lib, state2, x, vocab, w, w, -1, False, norm)
    assert out2["parent"].tolist() == [0, 1, 2] * GROUPS
    assert out2["tokens"].tolist() == [30 - r for r in range(GROUPS * w)]


def shaped_rows(vocab, w, tops):
    """Rows whose beam 0 ranks ``tops`` (token ids, best first) ahead of everything and whose other beams are flat (and
    far behind: log-probability -log(vocab) against beam 0's > -log(vocab) for its listed tokens)."""
    x = np.zeros((GROUPS * w, vocab), np.float32)
    for g in range(GROUPS):
        for i, t in enumerate(tops):
            x[g * w, t] = 12.0 - i
    return x


def live_state(w, length=2):
    state = ref.new_state(GROUPS, w, [6, 7, 8])
    state["cum"][:] = np.float32(-2.0)
    state["len"][:] = length
    return state


def test_eos_enters_the_pool_or_is_dropped(lib):
    vocab, w, eos = 37, 2, 1
    norm = ref.inv_norm_table(8, 2.0)
    # walk index 0 < W: a finished hypothesis with h = s * inv_norm[len + 1]
    state, _ = step(lib, live_state(w), shaped_rows(vocab, w, [eos, 10, 11, 12]), vocab, w, w, eos, False, norm)
    assert state["pool_n"].tolist() == [1] * GROUPS and state["pool_step"][:, 0].tolist() == [2] * GROUPS
    assert state["pool_parent"][:, 0].tolist() == [0] * GROUPS
    assert np.array_equal(state["pool_score"][:, 0], (state["pool_sum"][:, 0] * norm[3]).astype(np.float32))
    # walk index 2 >= W: dropped, and the two live beams are the candidates before it
    state, out = step(lib, live_state(w), shaped_rows(vocab, w, [10, 11, eos, 12]), vocab, w, w, eos, False, norm)
    assert state["pool_n"].tolist() == [0] * GROUPS and out["tokens"].tolist() == [10, 11] * GROUPS
    # eos_id < 0: nothing ever finishes, the eos token is a token like any other
    state, out = step(lib, live_state(w), shaped_rows(vocab, w, [eos, 10, 11, 12]), vocab, w, w, -1, False, norm)
    assert state["pool_n"].tolist() == [0] * GROUPS and out["tokens"].tolist() == [eos, 10] * GROUPS


def test_full_pool_replaced_or_kept(lib):
    """A full pool: an eos candidate replaces the worst entry (lowest score, highest index among equal ones) only when its
    score is strictly greater.  The candidate's own h comes from the oracle's first run."""
    vocab, w, eos = 37, 2, 1
    norm = ref.inv_norm_table(8, 1.0)
    x = shaped_rows(vocab, w, [eos, 10, 11, 12])
    probe, _ = step(lib, live_state(w), x, vocab, w, w, eos, False, norm)
    h = probe["pool_score"][0, 0]
    for worst, replaced in ((np.nextafter(h, np.float32(-np.inf)), True), (h, False)):
        state = live_state(w)
        state["pool_n"][:] = w
        state["pool_score"][:] = np.array([worst, worst], np.float32)  # equal scores: index 1 is the one to go
        state["pool_sum"][:] = np.float32(-9.0)
        state["pool_parent"][:] = 1
        state["pool_step"][:] = 1
        after, _ = step(lib, state, x, vocab, w, w, eos, False, norm)
        assert after["pool_n"].tolist() == [w] * GROUPS
        assert (after["pool_step"][:, 0] == 1).all()  # entry 0 is never the one replaced
        assert (after["pool_step"][:, 1] == (2 if replaced else 1)).all()


def test_dead_beam_and_small_vocabulary(lib):
    """Vocabulary 3 with eos 0 and W = 4: the first decision finds two non-eos tokens, so two beams are dead (cum -inf,
    parent -1, an idle row whose token is an id the next step can embed); their logits rows are never read afterwards --
    they hold NaN here -- and the next decision revives them from the live beams' candidates."""
    vocab, w, eos = 3, 4, 0
    norm = ref.inv_norm_table(8, 1.0)
    state = ref.new_state(GROUPS, w, [5, 5, 5])
    x = np.tile(np.array([[1.0, 3.0, 2.0]], np.float32), (GROUPS, 1))
    state, out = step(lib, state, x, vocab, w, 1, eos, False, norm, ld=8)
    assert out["tokens"].tolist() == [1, 2, 0, 0] * GROUPS and out["parent"].tolist() == [0, 0, -1, -1] * GROUPS
    assert state["cur"].reshape(GROUPS, w)[:, 2:].tolist() == [[-1, -1]] * GROUPS
    assert state["pool_n"].tolist() == [1] * GROUPS  # the eos at walk index 2 < W
    x = np.tile(np.array([[-9.0, 3.0, 2.0]], np.float32), (GROUPS * w, 1))
    x[[r for r in range(GROUPS * w) if r % w >= 2]] = np.nan
    state, out = step(lib, state, x, vocab, w, w, eos, False, norm, prev_out=out, ld=8)
    assert (out["parent"] >= 0).all() and (state["cur"] >= 0).all()


def test_done_group_is_left_alone(lib):
    """Group 1 is done: its state, its outputs and its scratch keep what they held (NaN logits: never read).  Group 0 has a
    full pool that its best beam cannot beat and becomes done in this call, whatever early_stopping says; group 2 has the
    same pool and a beam that can, and is done only with early_stopping."""
    vocab, w, eos = 37, 2, 1
    norm = ref.inv_norm_table(8, 1.0)
    for early in (False, True):
        state = live_state(w)
        state["done"][1] = 1
        state["cur"][w : 2 * w] = -1
        state["pool_n"][:] = w
        state["pool_score"][:] = np.float32(-3.0)
        state["cum"][: w] = np.float32(-50.0)  # best live -50.x / 3 < -3: cannot beat the pool
        state["cum"][2 * w :] = np.float32(-0.5)
        x = shaped_rows(vocab, w, [10, 11, 12, 13])
        x[w : 2 * w] = np.nan
        after, out = step(lib, state, x, vocab, w, w, eos, early, norm)
        assert after["done"].tolist() == [1, 1, 1 if early else 0]
        assert (after["cur"][: w] == -1).all() and (out["src"][: w] == -1).all() and (out["dst"][: w] == -1).all()
        assert (out["tokens"][w : 2 * w] == POISON).all()


def test_invalid_arguments(lib):
    w, vocab = 2, 37
    state = ref.new_state(GROUPS, w, [1, 1, 1])
    d = {n: dev(state[n]) for n in STATE}
    norm = dev(ref.inv_norm_table(4, 1.0))
    scratch = torch.zeros(GROUPS * w * 2 * w, dtype=torch.int32).cuda()
    lg = bf16_rows(np.zeros((GROUPS * w, vocab), np.float32))
    outs = [torch.zeros(GROUPS * w, dtype=torch.int32).cuda() for _ in OUT]

    def call(groups=GROUPS, beams=w, beams_in=w, voc=vocab, early=0, n_norm=4, null_state=None, null_out=None, logits=lg):
        ptrs = [None if n == null_state else d[n].data_ptr() for n in STATE]
        st = _lib.MdBeamState(*ptrs, None if null_state == "inv_norm" else norm.data_ptr(), n_norm,
                              None if null_state == "cand_ids" else scratch.data_ptr(), scratch.data_ptr())
        o = [None if i == null_out else t.data_ptr() for i, t in enumerate(outs)]
        return lib.md_beam_select(logits.data_ptr() if logits is not None else None, lg.stride(0), groups, beams, beams_in, voc, -1,
                                  None, 0, early, C.byref(st), *o, stream())

    assert call(groups=0) == 0
    for kw in (dict(groups=-1), dict(beams=0), dict(beams=17, beams_in=17), dict(beams_in=3), dict(voc=0), dict(voc=vocab + 1),
               dict(early=2), dict(n_norm=0), dict(logits=None), dict(null_state="inv_norm"), dict(null_state="cand_ids")):
        assert call(**kw) == MD_ERR_INVALID_ARG, kw
    for n in STATE:
        assert call(null_state=n) == MD_ERR_INVALID_ARG, n
    for i in range(len(OUT)):
        assert call(null_out=i) == MD_ERR_INVALID_ARG, i
    torch.cuda.synchronize()
