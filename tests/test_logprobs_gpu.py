"""Token log-probabilities on the MI355X: md_token_logprobs through the C ABI against a float64 reference (rank exact,
log-probability within a bound derived from the kernel's documented summation order), then the layers above it on the tiny
model -- generation logprobs (lockstep, captured, continuous), the prefill-based scorer and query_choices -- against the
reference's recorded logits and against the bit promises the project already makes (batch == alone, shared prefix ==
copy path, continuous == lockstep)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from moondream_amd import _lib, synth
from moondream_amd.config import get_config
from moondream_amd.continuous import ContinuousEngine
from util import bits_to_bf16

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
THREADS = 1024       # LOGPROB_THREADS of csrc/sampling_region.hip
SENT_LP = -12345.0   # what logprob / rank hold before a launch
SENT_RK = -77
NAN_BITS = 0x7FC0    # a bf16 NaN: the padding columns and the rows that must not be read
U = 2.0 ** -24       # unit roundoff of fp32

# The log-probability bound.  got = (x_t - m) - log(s), s the fp32 sum of e_v = exp(x_v - m) over the live tokens in the order
# the kernel documents: n_t = ceil(vocab / 1024) terms per thread sequentially, then log2(1024) = 10 butterfly levels.  Every
# term passes through at most (n_t - 1) + 10 additions, each of relative error <= U, all terms >= 0: the sum itself adds a
# relative error <= (n_t + 9) U to s, i.e. that much absolute error to log(s).  The constant C_ROUND covers the rest:
#   exp:       expf is good to 2 ulp = 4 U relative per term, hence <= 4 U relative in s                                 4
#   subtract:  x_v - m is a rounded fp32 difference of two bf16 values, absolute error <= U d_v with d_v = m - x_v, which
#              changes e_v by the factor exp(+-U d_v): relative error of s <= U sum_v p_v d_v, and with p_v = e_v / s that
#              sum is the entropy of p minus log(s) <= ln(vocab) <= ln(51200) < 11                                       11
#   slack for the products of the (1 + U)-factors above (second order, < 1e-5 of the total)                              1
# The remaining roundings are relative to quantities bounded by |ref| (m - x_t >= 0 and log(s) >= 0 add up to |ref|): log(s)
# 2 U |log s|, x_t - m U |x_t - m|, the final subtraction U |ref|: 4 U |ref| together, far inside the (1 + |ref|) factor.
C_ROUND = 16


def bound(vocab, ref):
    n_t = -(-vocab // THREADS)
    return (n_t + math.log2(THREADS) + C_ROUND) * U * (1.0 + abs(ref))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------ kernel
def reference(x, t, sup):
    """float64 (logprob, rank, max share, logprob with the largest live term left out of the sum) of token t in row x
    (float64 values of the bf16 logits); ``sup``: the suppressed id of this row or -1."""
    vocab = x.shape[0]
    if t < 0 or t >= vocab:
        return float("nan"), -1, None, None
    if t == sup:
        return float("-inf"), -1, None, None
    live = np.ones(vocab, dtype=bool)
    if sup >= 0:
        live[sup] = False
    m = x[live].max()
    e = np.exp(x[live] - m)
    s = e.sum()
    lp = (x[t] - m) - math.log(s)
    ids = np.arange(vocab)
    rank = int((live & (x > x[t])).sum() + (live & (ids < t) & (x == x[t])).sum())
    rest = s - e.max()  # (0 when one token holds all of the mass: the spike rows, which are not "normal" rows)
    lp_omit = (x[t] - m) - math.log(rest) if rest > 0 else float("inf")
    return float(lp), rank, float(e.max() / s), float(lp_omit)


def make_cases(vocab):
    """(name, logits row [vocab] bf16, target, suppress_rows flag, normal?) -- fixed seed per vocabulary.  The suppressed id
    is vocab // 3 in every launch."""
    gen = torch.Generator().manual_seed(vocab)
    scale = 8.0  # the logit scale of tests/golden/tiny_seed1.npz's step_logits (std 7.6 .. 8.2)
    sid = vocab // 3
    normal = lambda: (torch.randn(vocab, generator=gen) * scale).to(BF16)
    cases = []
    a = normal()
    t_a = int(torch.randint(0, vocab, (1,), generator=gen))
    t_a = t_a + 1 if t_a == sid else t_a
    cases.append(("normal, unsuppressed", a, t_a, 0, True))
    cases.append(("the same logits, suppressed", a.clone(), t_a, 1, True))
    b = normal()
    cases.append(("target is the argmax", b, int(torch.argmax(b.float())), 0, True))
    sp = normal()
    sp_at = vocab - 3
    sp[sp_at] = float(sp.float().max()) + 80.0
    cases.append(("spike of +80, target the spike", sp, sp_at, 1, False))
    cases.append(("spike of +80, target another token", sp.clone(), 5, 1, False))
    cases.append(("all equal", torch.full((vocab,), 1.5).to(BF16), vocab // 2, 0, False))
    tie = normal()
    t_tie = vocab // 2 + 1
    for i in (7, t_tie - 1, t_tie + 100):  # ties on both sides of the target: the two lower ids come first
        tie[i] = tie[t_tie]
    assert sid not in (7, t_tie - 1, t_tie, t_tie + 100)
    cases.append(("target ties three others", tie, t_tie, 1, True))
    blk = normal()
    blk[100:300] = float("-inf")
    cases.append(("a block of -inf", blk, 50, 1, True))
    top = normal()
    top[sid] = float(top.float().max()) + 5.0
    cases.append(("the maximum is the suppressed id, suppressed", top, 11, 1, True))
    cases.append(("the maximum is the suppressed id, unsuppressed", top.clone(), 11, 0, True))
    cases.append(("target is the suppressed id, suppressed", a.clone(), sid, 1, False))
    cases.append(("target is the suppressed id, unsuppressed", a.clone(), sid, 0, True))
    nan_row = torch.full((vocab,), NAN_BITS, dtype=torch.int16).view(BF16)
    cases.append(("target -1", nan_row, -1, 1, False))
    cases.append(("target vocab", nan_row.clone(), vocab, 0, False))
    return sid, cases


_TABLES = {}


def table(lib, vocab):
    """Per vocabulary, built once: the cases, their float64 references with per-row suppression and with every row suppressed
    (suppress_rows == NULL), and md_argmax_bf16's id for every row under both."""
    if vocab in _TABLES:
        return _TABLES[vocab]
    sid, cases = make_cases(vocab)
    ld = vocab + 8
    k = len(cases)
    logits = torch.full((k, ld), NAN_BITS, dtype=torch.int16).view(BF16)
    for r, c in enumerate(cases):
        logits[r, :vocab] = c[1]
    x64 = logits[:, :vocab].double().numpy()
    refs = {mode: [reference(x64[r], c[2], sid if (mode == "null" or c[3]) else -1) for r, c in enumerate(cases)]
            for mode in ("rows", "null")}
    dev = logits.cuda()
    argmaxes = {"rows": [], "null": []}
    nxt = torch.zeros(1, dtype=torch.int32, device="cuda")
    for mode in argmaxes:
        for r, c in enumerate(cases):
            if not 0 <= c[2] < vocab:
                argmaxes[mode].append(None)  # an all-NaN row
                continue
            sup = sid if (mode == "null" or c[3]) else -1
            _lib.check(lib.md_argmax_bf16(dev[r].data_ptr(), ld, 1, vocab, sup, nxt.data_ptr(), stream()))
            torch.cuda.synchronize()
            argmaxes[mode].append(int(nxt[0]))
    _TABLES[vocab] = (sid, cases, ld, dev, refs, argmaxes)
    return _TABLES[vocab]


def launch(lib, dev_logits, ld, vocab, sid, targets, flags, with_rank=True):
    """One md_token_logprobs launch over len(targets) rows; the output buffers carry two sentinel rows past them."""
    rows = len(targets)
    lp = torch.full((rows + 2,), SENT_LP, dtype=torch.float32, device="cuda")
    rk = torch.full((rows + 2,), SENT_RK, dtype=torch.int32, device="cuda")
    tg = torch.tensor(targets, dtype=torch.int32, device="cuda")
    fl = torch.tensor(flags, dtype=torch.int32, device="cuda") if flags is not None else None
    st = lib.md_token_logprobs(dev_logits.data_ptr(), ld, rows, vocab, sid, ptr(fl), tg.data_ptr(), lp.data_ptr(),
                               rk.data_ptr() if with_rank else None, stream())
    assert st == 0, st
    torch.cuda.synchronize()
    lp, rk = lp.cpu().numpy(), rk.cpu().numpy()
    assert (lp[rows:] == np.float32(SENT_LP)).all() and (rk[rows:] == SENT_RK).all(), "rows past `rows` were written"
    return lp[:rows], rk[:rows]


def check_rows(vocab, names, got_lp, got_rk, want, argmaxes, targets):
    worst = 0.0
    for r, name in enumerate(names):
        ref_lp, ref_rk, _, _ = want[r]
        assert int(got_rk[r]) == ref_rk, (name, int(got_rk[r]), ref_rk)
        if argmaxes[r] is not None and ref_rk >= 0:
            assert (int(got_rk[r]) == 0) == (argmaxes[r] == targets[r]), (name, int(got_rk[r]), argmaxes[r], targets[r])
        if math.isnan(ref_lp):
            assert math.isnan(float(got_lp[r])), (name, float(got_lp[r]))
        elif math.isinf(ref_lp):
            assert float(got_lp[r]) == ref_lp, (name, float(got_lp[r]))
        else:
            err, lim = abs(float(got_lp[r]) - ref_lp), bound(vocab, ref_lp)
            worst = max(worst, err / lim)
            assert err <= lim, (name, float(got_lp[r]), ref_lp, err, lim)
    return worst


@pytest.mark.parametrize("rows", [1, 3, 65])
@pytest.mark.parametrize("vocab", [520, 1504, 51200])
def test_kernel_against_float64(lib, vocab, rows):
    """520: fewer tokens than threads; 1504: ragged thread shares; 51200: the model's.  1 / 3 / 65 rows per launch: the
    cases in launches of that many rows (65: the case list repeated cyclically), so a grid or row-index slip moves a row's
    result.  ld = vocab + 8 with NaN in the padding columns: a kernel that reads them returns NaN."""
    sid, cases, ld, dev, refs, argmaxes = table(lib, vocab)
    k = len(cases)
    names = [c[0] for c in cases]

    # the test's own sensitivity, on the CPU: leaving ONE live token of share >= 1e-3 out of the sum is outside the bound
    for mode in ("rows", "null"):
        for r, c in enumerate(cases):
            if c[4] and math.isfinite(refs[mode][r][0]):
                ref_lp, _, share, lp_omit = refs[mode][r]
                assert share >= 1e-3, (c[0], share)
                assert abs(lp_omit - ref_lp) > bound(vocab, ref_lp), (c[0], lp_omit, ref_lp)

    worst = 0.0
    if rows >= k:
        idx = [r % k for r in range(rows)]
        batches = [idx]
    else:
        batches = [list(range(r0, min(k, r0 + rows))) for r0 in range(0, k, rows)]
    for idx in batches:
        sel = dev[idx].contiguous() if idx != list(range(idx[0], idx[0] + len(idx))) else dev[idx[0] : idx[0] + len(idx)]
        targets, flags = [cases[i][2] for i in idx], [cases[i][3] for i in idx]
        for mode, fl in (("rows", flags), ("null", None)):
            lp, rk = launch(lib, sel, ld, vocab, sid, targets, fl)
            worst = max(worst, check_rows(vocab, [names[i] for i in idx], lp, rk, [refs[mode][i] for i in idx],
                                          [argmaxes[mode][i] for i in idx], targets))
    # rank is optional: the same log-probabilities, the rank buffer untouched
    idx = batches[0]
    sel = dev[idx].contiguous()
    targets, flags = [cases[i][2] for i in idx], [cases[i][3] for i in idx]
    lp_a, _ = launch(lib, sel, ld, vocab, sid, targets, flags)
    lp_b, rk_b = launch(lib, sel, ld, vocab, sid, targets, flags, with_rank=False)
    assert lp_a.view(np.int32).tolist() == lp_b.view(np.int32).tolist() and (rk_b == SENT_RK).all()
    print(f"vocab {vocab} rows {rows}: worst |got - ref| / bound = {worst:.3f}")


def test_kernel_argument_checks(lib):
    vocab = 520
    logits = torch.zeros(2, vocab, dtype=BF16, device="cuda")
    tg = torch.zeros(2, dtype=torch.int32, device="cuda")
    lp = torch.full((2,), SENT_LP, dtype=torch.float32, device="cuda")
    rk = torch.full((2,), SENT_RK, dtype=torch.int32, device="cuda")

    def call(lg=logits, t=tg, out=lp, rows=2, v=vocab, ld=vocab):
        return lib.md_token_logprobs(ptr(lg), ld, rows, v, -1, None, ptr(t), ptr(out), rk.data_ptr(), stream())

    assert call(lg=None) == 1 and call(t=None) == 1 and call(out=None) == 1  # MD_ERR_INVALID_ARG
    assert call(rows=-1) == 1 and call(v=0) == 1 and call(v=-5) == 1 and call(ld=vocab - 1) == 1
    assert call(rows=0) == 0  # MD_OK, nothing launched
    torch.cuda.synchronize()
    assert lp.tolist() == [SENT_LP] * 2 and rk.tolist() == [SENT_RK] * 2
    assert call() == 0
    torch.cuda.synchronize()
    assert rk.tolist() == [0, 0]  # all-equal logits, target 0: the lowest id is the argmax
    assert all(abs(x + math.log(vocab)) <= bound(vocab, math.log(vocab)) for x in lp.tolist())


# ------------------------------------------------------------------ model
def golden_image(g, idx, kind="cap"):
    src = int(g["image_index"][idx])
    arr = synth.synthetic_image_array(src, int(g["seed"]), tuple(g[f"img{idx}.{kind}.size"]))
    return Image.fromarray(arr, "RGB")


def words(x):
    """fp32 bit patterns: equality of these is bit equality."""
    return np.asarray(x, dtype=np.float32).view(np.int32).tolist()


def ref_logprobs(g, cfg, i, tokens, kind="cap"):
    """float64 log-softmax of the reference's recorded logits at ``tokens``; answer_id suppressed from decision 1 on."""
    lg = bits_to_bf16(g[f"img{i}.{kind}.step_logits"]).double()[: len(tokens)].clone()
    lg[1:, cfg.tokenizer.answer_id] = float("-inf")
    return torch.log_softmax(lg, dim=1)[torch.arange(len(tokens)), torch.tensor(tokens)].tolist()


class Tiny:
    pass


@pytest.fixture(scope="module")
def tiny(golden_dir):
    """The tiny model of tests/test_model_gpu.py with the three golden captions, and the lockstep results every test below
    compares with, computed once."""
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    assert torch.cuda.is_available(), "GPU tests need a device"
    t = Tiny()
    t.g = g = np.load(os.path.join(golden_dir, "tiny_seed1.npz"))
    t.cfg = get_config("tiny")
    sd = synth.synthetic_state_dict(t.cfg, seed=int(g["seed"]), device="cuda")
    t.model = MoondreamModel(t.cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=8)
    t.images = [golden_image(g, i) for i in range(3)]
    t.prompts = [g[f"img{i}.cap.prompt"].tolist() for i in range(3)]
    t.tokens = [g[f"img{i}.cap.tokens"].tolist() for i in range(3)]
    t.n = len(t.tokens[0])
    t.plain = t.model.batch_generate_ids(t.images, t.prompts, max_tokens=t.n)
    t.ids, t.lp, t.rk = t.model.batch_generate_ids(t.images, t.prompts, max_tokens=t.n, return_logprobs=True)
    return t


def alone(model, fn):
    """``fn()`` with a lone sequence on the batched kernels."""
    was = model.single_sequence_kernel
    model.single_sequence_kernel = False
    try:
        return fn()
    finally:
        model.single_sequence_kernel = was


def test_flag_changes_no_id(tiny):
    m = tiny.model
    assert tiny.ids == tiny.plain == tiny.tokens
    assert all(len(tiny.lp[i]) == len(tiny.rk[i]) == len(tiny.ids[i]) for i in range(3))
    gen = lambda: torch.Generator(device="cuda").manual_seed(5)
    kw = dict(max_tokens=12, temperature=8.0, top_p=0.95, ignore_eos=True)  # hot: the golden margins are >= 11
    a = m.batch_generate_ids(tiny.images, tiny.prompts, generator=gen(), **kw)
    b, lp, rk = m.batch_generate_ids(tiny.images, tiny.prompts, generator=gen(), return_logprobs=True, **kw)
    assert a == b and a != [s[:12] for s in tiny.tokens], "the sampled call must leave the greedy path for the check to mean anything"
    for i in range(3):
        assert len(lp[i]) == len(rk[i]) == len(b[i]) == 12
        assert all(math.isfinite(x) and x <= 0 for x in lp[i]) and all(r >= 0 for r in rk[i])
        assert any(r > 0 for s in rk for r in s)  # a sampled token off the argmax carries its rank
    # one sequence on the persistent single-sequence kernel, which leaves its logits in the buffer too
    one = m.batch_generate_ids(tiny.images[:1], tiny.prompts[:1], max_tokens=tiny.n)
    one_lp = m.batch_generate_ids(tiny.images[:1], tiny.prompts[:1], max_tokens=tiny.n, return_logprobs=True)
    assert one_lp[0] == one and all(r == 0 for r in one_lp[2][0])
    want = ref_logprobs(tiny.g, tiny.cfg, 0, one[0])
    assert max(abs(a_ - b_) for a_, b_ in zip(one_lp[1][0], want)) <= 1.0


def test_greedy_logprobs_against_the_reference(tiny):
    """Within 1.0 of the float64 log-softmax of the reference's step logits: twice the project's logit bound of 0.5
    (tests/test_model_gpu.py), once for the target logit and once for the log-sum-exp.  Every greedy rank is 0."""
    worst = 0.0
    for i in range(3):
        want = ref_logprobs(tiny.g, tiny.cfg, i, tiny.tokens[i])
        worst = max(worst, max(abs(a - b) for a, b in zip(tiny.lp[i], want)))
        assert tiny.rk[i] == [0] * tiny.n
    print(f"max |logprob - reference| over the golden captions: {worst:.3e}")
    assert worst <= 1.0


def test_a_row_of_the_batch_equals_the_row_alone(tiny):
    m = tiny.model
    for i in (0, 2):
        ids, lp, rk = alone(m, lambda: m.batch_generate_ids([tiny.images[i]], [tiny.prompts[i]], max_tokens=tiny.n,
                                                              return_logprobs=True))
        assert ids[0] == tiny.ids[i] and rk[0] == tiny.rk[i]
        assert words(lp[0]) == words(tiny.lp[i])


def test_truncation_keeps_ids_and_values_aligned(tiny):
    m = tiny.model
    stop = tiny.tokens[0][4]
    ids, lp, rk = m.batch_generate_ids(tiny.images, tiny.prompts, max_tokens=9, eos_id=stop, return_logprobs=True)
    assert ids[0] == tiny.tokens[0][:4] and ids[1] == tiny.tokens[1][:9]
    for i in range(3):
        assert words(lp[i]) == words(tiny.lp[i][: len(ids[i])]) and rk[i] == tiny.rk[i][: len(ids[i])]


def test_captured_chunks_equal_eager(tiny):
    m = tiny.model
    m.compile()
    try:
        for _ in range(2):  # the capturing call, then a replay
            ids, lp, rk = m.batch_generate_ids(tiny.images, tiny.prompts, max_tokens=tiny.n, return_logprobs=True)
            assert ids == tiny.ids and rk == tiny.rk and [words(x) for x in lp] == [words(x) for x in tiny.lp]
        assert m.batch_generate_ids(tiny.images, tiny.prompts, max_tokens=tiny.n) == tiny.ids
        eng = ContinuousEngine(m, max_live=4, chunk=4, logprobs=True)
        for _ in range(2):
            ids, lp, rk = eng.generate(tiny.images, tiny.prompts, max_tokens=tiny.n, return_logprobs=True)
            assert ids == tiny.ids and rk == tiny.rk and [words(x) for x in lp] == [words(x) for x in tiny.lp]
    finally:
        m.use_graphs = False
        m._graphs.clear()


def test_continuous_engine_equals_lockstep(tiny):
    """Ragged lengths and three requests in a bucket of four rows: idle and padding rows exist in every chunk."""
    m = tiny.model
    mt = [tiny.n, 3, 9]
    eng = ContinuousEngine(m, max_live=4, chunk=4, logprobs=True)
    ids, lp, rk = eng.generate(tiny.images, tiny.prompts, max_tokens=mt, return_logprobs=True)
    for i in range(3):
        assert ids[i] == tiny.ids[i][: mt[i]] and len(lp[i]) == len(rk[i]) == len(ids[i]) == mt[i]
        assert not any(math.isnan(x) for x in lp[i])
        assert words(lp[i]) == words(tiny.lp[i][: mt[i]]) and rk[i] == tiny.rk[i][: mt[i]]
    assert eng.stats.padded_row_steps > eng.stats.live_row_steps
    # the same through the model's wrapper; an engine without the flag still yields pairs
    got = m.batch_generate_ids_continuous(tiny.images, tiny.prompts, max_tokens=mt, max_live=4, chunk=4, return_logprobs=True)
    assert got[0] == ids and [words(x) for x in got[1]] == [words(x) for x in lp] and got[2] == rk
    off = ContinuousEngine(m, max_live=4, chunk=4)
    rids = [off.submit(tiny.images[i], tiny.prompts[i], max_tokens=mt[i]) for i in range(3)]
    out = list(off.run())
    assert all(len(item) == 2 for item in out) and dict(out) == {r: ids[i] for i, r in enumerate(rids)}
    on = ContinuousEngine(m, max_live=4, chunk=4, logprobs=True)
    on.submit(tiny.images[0], tiny.prompts[0], max_tokens=3)
    assert all(len(item) == 2 for item in on.run())
    with pytest.raises(ValueError):
        list(off.run(with_logprobs=True))


def test_shared_prefix_equals_the_copy_path(tiny):
    m = tiny.model
    enc = m.encode_image(tiny.images[0])
    prompts = [tiny.prompts[0], [1, 708, 9, 3], [1, 17, 708, 2, 382, 9, 3]]
    kw = dict(max_tokens=10, ignore_eos=True, return_logprobs=True)
    a = m.batch_generate_ids([enc] * 3, prompts, share_prefix=True, **kw)
    b = m.batch_generate_ids([enc] * 3, prompts, **kw)
    assert a[0] == b[0] and a[2] == b[2] and [words(x) for x in a[1]] == [words(x) for x in b[1]]
    conts = [a[0][0][:1], a[0][1][:3], a[0][2]]
    sa = m.score_ids([enc] * 3, prompts, conts, share_prefix=True)
    sb = m.score_ids([enc] * 3, prompts, conts)
    assert sa[1] == sb[1] and [words(x) for x in sa[0]] == [words(x) for x in sb[0]]
    assert all(r == 0 for row in sa[1] for r in row)  # the model's own greedy tokens


def test_score_ids_against_the_reference_and_alone(tiny):
    m = tiny.model
    lp, rk = m.score_ids(tiny.images, tiny.prompts, tiny.tokens)
    worst = 0.0
    for i in range(3):
        assert rk[i] == [0] * tiny.n
        want = ref_logprobs(tiny.g, tiny.cfg, i, tiny.tokens[i])
        worst = max(worst, max(abs(a - b) for a, b in zip(lp[i], want)))
    print(f"score_ids: max |logprob - reference| over the golden captions: {worst:.3e}")
    assert worst <= 1.0
    # continuations of 1, 3 and all tokens in one call; every row equals the row scored alone
    conts = [tiny.tokens[0][:1], tiny.tokens[1][:3], tiny.tokens[2]]
    rag = m.score_ids(tiny.images, tiny.prompts, conts)
    assert [len(x) for x in rag[0]] == [len(x) for x in rag[1]] == [1, 3, tiny.n]
    for i in range(3):
        one = alone(m, lambda: m.score_ids([tiny.images[i]], [tiny.prompts[i]], [conts[i]]))
        assert one[1][0] == rag[1][i] and words(one[0][0]) == words(rag[0][i]), i
    full2 = alone(m, lambda: m.score_ids([tiny.images[2]], [tiny.prompts[2]], [tiny.tokens[2]]))
    assert words(full2[0][0]) == words(lp[2]) and words(rag[0][2]) == words(lp[2])


def test_score_ids_is_causal_and_suppresses_like_generation(tiny):
    m = tiny.model
    cfg = tiny.cfg
    base = alone(m, lambda: m.score_ids([tiny.images[0]], [tiny.prompts[0]], [tiny.tokens[0]]))
    at = 5
    swapped = list(tiny.tokens[0])
    swapped[at] = (swapped[at] + 1) % cfg.text.vocab_size
    assert swapped[at] != cfg.tokenizer.answer_id
    got = alone(m, lambda: m.score_ids([tiny.images[0]], [tiny.prompts[0]], [swapped]))
    assert got[1][0][at] > 0 and got[0][0][at] < base[0][0][at]
    assert words(got[0][0][:at]) == words(base[0][0][:at]) and got[1][0][:at] == base[1][0][:at]
    assert words(got[0][0][at + 1 :]) != words(base[0][0][at + 1 :])  # the later decisions saw another token
    # answer_id itself: live at decision 0, suppressed from decision 1 on
    a = cfg.tokenizer.answer_id
    lp, rk = m.score_ids([tiny.images[0]], [tiny.prompts[0]], [[a, a]])
    assert math.isfinite(lp[0][0]) and rk[0][0] >= 0
    assert lp[0][1] == float("-inf") and rk[0][1] == -1


def test_query_choices(tiny):
    m, g = tiny.model, tiny.g
    prompt = g["img0.vqa.prompt"].tolist()
    question = " ".join(str(t) for t in prompt[3:-2])
    assert m._query_prompts([question])[0] == prompt
    gold = g["img0.vqa.tokens"].tolist()[:4]
    v = tiny.cfg.text.vocab_size
    others = [[(t + 7) % v for t in gold], [(t + 301) % v for t in gold[:3]]]
    choices = [others[0], gold, others[1]]
    image = golden_image(g, 0, "vqa")
    out = m.query_choices(image, question, [" ".join(map(str, c)) for c in choices])
    assert out["best"] == 1 and out["best_normalized"] == 1
    assert [len(p) for p in out["per_token"]] == [5, 5, 4]  # eos appended
    enc = m.encode_image(image)
    conts = [c + [tiny.cfg.tokenizer.eos_id] for c in choices]
    lp, _ = m.score_ids([enc] * 3, [prompt] * 3, conts)
    assert [words(x) for x in out["per_token"]] == [words(x) for x in lp]
    for i in range(3):
        assert out["logprobs"][i] == pytest.approx(sum(lp[i])) and out["mean_logprobs"][i] == pytest.approx(sum(lp[i]) / len(lp[i]))
    want = ref_logprobs(g, tiny.cfg, 0, gold, "vqa")
    assert max(abs(a_ - b_) for a_, b_ in zip(out["per_token"][1][:4], want)) <= 1.0
