"""The decode-chunk runner (moondream_amd/decode_loop.py) without a GPU: a stand-in model records every call the runner
makes of it; CPU tensors stand for the fixed-address buffers.  Checked: the order step -> pick -> logprobs of every step
and the buffer rows each call carries, the launches that must be absent, what the graph key tells apart, and that a
refused capture stores nothing."""
import itertools
from dataclasses import replace

import pytest
import torch

from moondream_amd.decode_loop import DecodeChunk, Sampling, run_chunk

V = 11
STREAM = 0x5EED


class Rows:
    """Stand-in for ``_Rows``: what the runner reads of a routing."""

    def __init__(self, name, slot0=0):
        self.name, self.slot0 = name, slot0

    def key(self):
        return (self.name, None, None)


class Kv:
    def __init__(self, slot0, k8):
        self.k, self.k8, self.slot0 = 1000 + slot0, k8, slot0


class Recorder:
    """The handful of ``MoondreamModel`` methods the runner may use; each records (name, arguments)."""

    def __init__(self, k8=None):
        self.calls, self.graphs, self.k8 = [], {}, k8
        self.logits = torch.zeros(8, V)
        self.ws = torch.zeros(64, dtype=torch.uint8)

    def _decode_logits(self, b):
        return self.logits

    def _workspace(self, nbytes, which=0):
        self.ws_asked = (nbytes, which)
        return self.ws

    def _kv_struct(self, slot0=0):
        return Kv(slot0, self.k8)

    def _decode_step(self, rows, tok_in, tok_out, pos, b, suppress_id, logits, ws, kv):
        self.calls.append(("step", rows.name, tok_in, tok_out, pos, b, suppress_id, logits, ws, kv.slot0))

    def _decode_step_b1(self, tok_in, tok_out, pos, suppress_id, logits, ws, kv):
        self.calls.append(("b1", tok_in, tok_out, pos, suppress_id, logits, ws, kv.slot0))

    def _pick(self, logits, temperature, top_p, suppress_id=-1, generator=None, probs_out=None, row_perm=None, uniforms=None,
              out=None):
        self.calls.append(("pick", logits, temperature, top_p, suppress_id, generator, uniforms, out))

    def _pick_rows(self, logits, temperature_dev, top_p_dev, suppress_id, uniforms, out=None):
        self.calls.append(("pick_rows", logits, temperature_dev, top_p_dev, suppress_id, uniforms, out))

    def _token_logprobs(self, logits, targets, suppress_id, logprob, rank, suppress_rows=None):
        self.calls.append(("logprobs", logits, targets, suppress_id, logprob, rank))

    def _replay_or_capture(self, key, body, may_capture=None):
        """As MoondreamModel's, with "capturing" = running the body a second time and storing the key."""
        self.key = key
        if key in self.graphs:
            self.calls.append(("replay",))
            return False
        body()
        if may_capture is not None and not may_capture():
            return False
        self.calls.append(("capture",))
        body()
        self.graphs[key] = True
        return True


def same(a, b):
    """The same buffer row: address, shape and strides."""
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


N, PAD = 3, 2  # steps run; further rows the buffers have (the runner must not need exact sizes)


def make_chunk(b=2, pick="none", logprobs=False, b1=False, **kw):
    rows = [Rows(f"step{i}") for i in range(N + PAD)]
    picks = {"none": None, "scalar": Sampling(0.5, 0.3), "rows": Sampling(torch.zeros(b), torch.ones(b))}
    planes = (torch.zeros(N + PAD, b), torch.zeros(N + PAD, b, dtype=torch.int32)) if logprobs else None
    chunk = DecodeChunk(b, torch.zeros(N + 1 + PAD, b, dtype=torch.int32), torch.zeros(b, dtype=torch.int32), lambda i: rows[i], 7, 48,
                        picks[pick], torch.zeros(N + PAD, b) if pick != "none" else None, planes, b1)
    return replace(chunk, **kw)


CASES = [(pick, lp, b1) for pick, lp, b1 in itertools.product(("none", "scalar", "rows"), (False, True), (False, True))
         if not (b1 and pick != "none")]


def expected_calls(m, c, n):
    lg = m.logits[: c.b]
    out = []
    for i in range(n):
        tin, tout = c.tokens[i], c.tokens[i + 1]
        if c.b1:
            out.append(("b1", tin, tout, c.pos, 7, m.logits, m.ws, 0))
        else:
            out.append(("step", f"step{i}", tin, tout, c.pos, c.b, 7, m.logits, m.ws, 0))
        if c.pick is not None and c.pick.per_row:
            out.append(("pick_rows", lg, c.pick.temperature, c.pick.top_p, 7, c.uniforms[i], tout))
        elif c.pick is not None:
            out.append(("pick", lg, 0.5, 0.3, 7, None, c.uniforms[i], tout))
        if c.logprobs is not None:
            out.append(("logprobs", lg, tout, 7, c.logprobs[0][i], c.logprobs[1][i]))
    return out


def assert_calls(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert len(g) == len(w), g[0]
        for j, (x, y) in enumerate(zip(g, w)):
            assert same(x, y) if torch.is_tensor(y) else x == y, (g[0], j)


@pytest.mark.parametrize("pick,logprobs,b1", CASES)
@pytest.mark.parametrize("captured", [False, True], ids=["eager", "capture-miss"])
def test_every_step_is_step_then_pick_then_logprobs_over_the_right_rows(pick, logprobs, b1, captured):
    m = Recorder()
    c = make_chunk(b=1 if b1 else 2, pick=pick, logprobs=logprobs, b1=b1)
    assert run_chunk(m, c, N, capture_stream=STREAM if captured else None) is captured
    assert m.ws_asked == (48, 2)
    want = expected_calls(m, c, N)
    if captured:  # a miss: the eager run, then the same body under capture; then a replay launches nothing from Python
        want = want + [("capture",)] + want
    assert_calls(m.calls, want)
    names = {call[0] for call in m.calls}
    if pick == "none":  # greedy keeps the step's argmax: no pick launch
        assert not names & {"pick", "pick_rows"}
    if not logprobs:
        assert "logprobs" not in names
    assert ("b1" in names) == b1 and ("step" in names) == (not b1)
    if captured:
        m.calls.clear()
        assert run_chunk(m, c, N, capture_stream=STREAM) is False
        assert m.calls == [("replay",)]


def test_a_step_from_pieces_replaces_the_fused_step_and_its_logits():
    m = Recorder()
    lg = torch.zeros(2, V)
    gen = object()
    seen = []

    def pieces(tok_in):
        seen.append(tok_in)
        m.calls.append(("pieces",))
        return lg

    c = replace(make_chunk(logprobs=True), pick=Sampling(0.0, 0.0, gen), step=pieces)
    assert run_chunk(m, c, N) is False
    want = []
    for i in range(N):
        want += [("pieces",), ("pick", lg, 0.0, 0.0, 7, gen, None, c.tokens[i + 1]),
                 ("logprobs", lg, c.tokens[i + 1], 7, c.logprobs[0][i], c.logprobs[1][i])]
    assert_calls(m.calls, want)
    assert all(same(s, c.tokens[i]) for i, s in enumerate(seen))
    with pytest.raises(AssertionError):  # never captured
        run_chunk(m, c, N, capture_stream=STREAM)


def key_of(chunk, n=N, tag="decode", stream=STREAM, k8=None):
    m = Recorder(k8)
    run_chunk(m, chunk, n, tag, stream)
    return m.key, m


def test_identical_chunks_share_a_key_and_each_baked_in_thing_changes_it():
    base = make_chunk(pick="scalar", logprobs=True)
    m = Recorder()
    run_chunk(m, base, N, capture_stream=STREAM)
    key = m.key
    m.calls.clear()
    run_chunk(m, replace(base), N, capture_stream=STREAM)  # an equal description over the same buffers: a replay
    assert m.key == key and m.calls == [("replay",)]

    def differs(chunk, **kw):
        other, om = key_of(chunk, **kw)
        # (the stand-in's logits / workspace are per recorder: compare with a key from the same recorder's buffers)
        ref, _ = key_of(base)
        strip = lambda k, r: tuple(x for x in k if x not in (r.logits.data_ptr(), r.ws.data_ptr()))
        return strip(other, om) != strip(ref, _)

    b3 = make_chunk(b=3, pick="scalar", logprobs=True)
    assert differs(b3)
    assert differs(base, n=N - 1)
    assert differs(replace(base, suppress_id=8))
    assert differs(base, stream=STREAM + 1)
    for name in ("tokens", "pos", "uniforms"):  # a buffer address, one at a time
        assert differs(replace(base, **{name: torch.zeros_like(getattr(base, name))})), name
    assert differs(replace(base, logprobs=(torch.zeros_like(base.logprobs[0]), base.logprobs[1])))
    assert differs(replace(base, logprobs=(base.logprobs[0], torch.zeros_like(base.logprobs[1]))))
    assert differs(replace(base, pick=Sampling(0.5, 0.31)))          # the scalar settings
    assert differs(replace(base, pick=Sampling(0.6, 0.3)))
    assert differs(replace(base, pick=None, uniforms=None))          # "has a sampling launch"
    assert differs(replace(base, pick=Sampling(torch.zeros(2), torch.ones(2))))
    assert differs(replace(base, logprobs=None))                     # the logprob flag
    assert differs(replace(base, rows_of=lambda i: Rows("other")))   # _Rows.key()
    assert differs(replace(base, rows_of=lambda i: Rows("step0", slot0=2)))  # (the KV struct's base)
    assert differs(base, k8=4096)                                    # the e4m3 copy
    assert differs(base, tag="continuous")
    one = make_chunk(b=1, logprobs=True)
    k_plain, mp = key_of(one)
    k_b1, mb = key_of(replace(one, b1=True))
    assert [x for x in k_plain if x not in (mp.logits.data_ptr(), mp.ws.data_ptr())] != \
           [x for x in k_b1 if x not in (mb.logits.data_ptr(), mb.ws.data_ptr())]
    # the logits and workspace addresses are in the key too
    assert m.logits.data_ptr() in key and m.ws.data_ptr() in key


def test_the_logprob_flag_off_leaves_the_key_alone():
    m = Recorder()
    c = make_chunk(pick="rows")
    run_chunk(m, c, N, "continuous", STREAM)
    plain = m.key
    run_chunk(m, replace(c, logprobs=(torch.zeros(N, 2), torch.zeros(N, 2, dtype=torch.int32))), N, "continuous", STREAM)
    assert m.key[: len(plain)] == plain and m.key[len(plain)] == "logprobs"
    assert "logprobs" not in plain


def test_continuous_keys_start_with_the_tag_and_the_stream():
    key, _ = key_of(make_chunk(pick="rows"), tag="continuous")
    assert key[0] == "continuous" and key[1] == STREAM


def test_a_refused_capture_stores_nothing():
    m = Recorder()
    c = make_chunk(pick="rows", logprobs=True)
    asked = []
    assert run_chunk(m, c, N, "continuous", STREAM, may_capture=lambda: asked.append(1) or False) is False
    assert asked == [1] and not m.graphs
    assert_calls(m.calls, expected_calls(m, c, N))  # it ran, eagerly, once
    assert run_chunk(m, c, N, "continuous", STREAM, may_capture=lambda: True) is True
    assert list(m.graphs) == [m.key]
