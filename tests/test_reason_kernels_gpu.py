"""The two kernels of the batched reasoning query and its fused step on the MI355X: md_reason_route and
md_mask_logits_rows exactly against numpy restatements written here, and one md_decode_step_reason on the tiny model
bit for bit against the same step assembled from the existing pieces."""
import ctypes as C

import numpy as np
import pytest
import torch

from moondream_amd import _lib, synth
from moondream_amd.config import get_config
from moondream_amd.decode_loop import ReasonChunk

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
IDLE, REASON, ANSWER, DONE = -1, 0, 1, 2
K_NONE, K_REASON, K_SUFFIX, K_ANSWER = 0, 1, 2, 3
ANSWER_ID, EOS_ID, SIZE_ID, COORD_ID, SUFFIX_ID = 3, 0, 6, 5, 4  # suffix_id != answer_id here: the two must not be confused
MAX_REASON, MAX_ANSWER = 4, 3
VOCAB, DIM = 40, 64
SENT = -77  # what idle rows' outputs are pre-filled with


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dtype=torch.int32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


# every branch of the rule: (name, phase, token, forced, n_reason, n_answer)
CASES = [
    ("reason, ordinary token", REASON, 17, -1, 1, 0),
    ("reason, coordinate token", REASON, COORD_ID, -1, 0, 0),
    ("reason ends on answer_id", REASON, ANSWER_ID, -1, 2, 0),
    ("reason ends on the budget", REASON, 17, -1, MAX_REASON, 0),
    ("reason, last token inside the budget", REASON, 18, -1, MAX_REASON - 1, 0),
    ("answer continues", ANSWER, 20, -1, 2, 1),
    ("answer, answer_id as a token", ANSWER, ANSWER_ID, -1, 2, 0),
    ("answer ends on eos_id", ANSWER, EOS_ID, -1, 2, 1),
    ("answer ends on the budget", ANSWER, 21, -1, 2, MAX_ANSWER),
    ("done", DONE, 22, -1, 3, 2),
    ("done, id past the table", DONE, VOCAB + 100, -1, 3, 2),
    ("done, negative id", DONE, -5, -1, 3, 2),
    ("idle", IDLE, 23, -1, 1, 1),
    ("idle, forced", IDLE, 23, 9, 1, 1),
    ("forced: an ordinary token becomes answer_id", REASON, 17, ANSWER_ID, 1, 0),
    ("forced: answer_id becomes the coordinate token", REASON, ANSWER_ID, COORD_ID, 1, 0),
    ("forced: eos becomes a token", ANSWER, EOS_ID, 24, 2, 1),
    ("forced: a token becomes eos", ANSWER, 24, EOS_ID, 2, 1),
    ("forced 0 is a forced eos, not 'unforced'", REASON, 17, 0, 1, 0),
]


def route_ref(phase, tok, forced, nr, na, coord_bin, wte, coord_emb, x0, kind0, ground0, sup0):
    """numpy restatement of md_reason_route (include/moondream_hip.h); returns the expected outputs."""
    b = len(phase)
    ph, nr, na = phase.copy(), nr.copy(), na.copy()
    x, kind, ground, sup = x0.copy(), kind0.copy(), ground0.copy(), sup0.copy()
    for r in range(b):
        if phase[r] < 0:
            continue
        t = int(forced[r]) if forced is not None and forced[r] >= 0 else int(tok[r])
        src, from_coord = t, False
        kind[r], ground[r], sup[r] = K_NONE, -1, (-1, -1)
        if phase[r] == REASON:
            if t == ANSWER_ID or nr[r] >= MAX_REASON:
                ph[r], kind[r], src = ANSWER, K_SUFFIX, SUFFIX_ID
            else:
                kind[r], sup[r] = K_REASON, (EOS_ID, SIZE_ID)
                nr[r] += 1
                if t == COORD_ID:
                    from_coord, ground[r] = True, coord_bin[r]
        elif phase[r] == ANSWER:
            if t == EOS_ID or na[r] >= MAX_ANSWER:
                ph[r] = DONE
            else:
                kind[r], sup[r] = K_ANSWER, (ANSWER_ID, -1)
                na[r] += 1
        if not 0 <= src < wte.shape[0]:
            src = 0
        x[r, :DIM] = coord_emb[r, :DIM] if from_coord else wte[src, :DIM]
    return ph, nr, na, kind, ground, sup, x


def run_route(lib, rows, with_forced):
    b = len(rows)
    rng = np.random.default_rng(100 + b)
    ld_w, ld_c, ld_x = DIM + 8, DIM + 16, DIM + 24  # every row stride padded beyond D
    wte = rng.integers(-32768, 32767, (VOCAB, ld_w), dtype=np.int16)
    coord_emb = rng.integers(-32768, 32767, (b, ld_c), dtype=np.int16)
    x0 = np.full((b, ld_x), SENT, dtype=np.int16)
    phase = np.array([c[1] for c in rows], dtype=np.int32)
    tok = np.array([c[2] for c in rows], dtype=np.int32)
    forced = np.array([c[3] for c in rows], dtype=np.int32) if with_forced else None
    nr = np.array([c[4] for c in rows], dtype=np.int32)
    na = np.array([c[5] for c in rows], dtype=np.int32)
    coord_bin = rng.integers(0, 1024, b).astype(np.int32)
    kind0, ground0, sup0 = (np.full(s, SENT, dtype=np.int32) for s in ((b,), (b,), (b, 2)))
    want = route_ref(phase, tok, forced, nr, na, coord_bin, wte, coord_emb, x0, kind0, ground0, sup0)
    d = dict(phase=dev(phase), nr=dev(nr), na=dev(na), kind=dev(kind0), ground=dev(ground0), sup=dev(sup0), bin=dev(coord_bin),
             forced=dev(forced) if forced is not None else None, tok=dev(tok), wte=dev(wte, torch.int16), emb=dev(coord_emb, torch.int16),
             x=dev(x0, torch.int16))
    st = _lib.MdReasonState(d["phase"].data_ptr(), d["nr"].data_ptr(), d["na"].data_ptr(), d["kind"].data_ptr(), d["ground"].data_ptr(),
                            d["sup"].data_ptr(), d["bin"].data_ptr(), None, d["forced"].data_ptr() if forced is not None else None,
                            MAX_REASON, MAX_ANSWER, ANSWER_ID, EOS_ID, SIZE_ID, COORD_ID, SUFFIX_ID)
    _lib.check(lib.md_reason_route(C.byref(st), d["tok"].data_ptr(), d["wte"].data_ptr(), ld_w, VOCAB, d["emb"].data_ptr(), ld_c,
                                   d["x"].data_ptr(), ld_x, b, DIM, stream()), "md_reason_route")
    torch.cuda.synchronize()
    got = tuple(d[k].cpu().numpy() for k in ("phase", "nr", "na", "kind", "ground", "sup", "x"))
    # the inputs the kernel must not write
    assert np.array_equal(d["tok"].cpu().numpy(), tok) and np.array_equal(d["bin"].cpu().numpy(), coord_bin)
    assert np.array_equal(d["wte"].cpu().numpy(), wte) and np.array_equal(d["emb"].cpu().numpy(), coord_emb)
    return got, want


@pytest.mark.parametrize("batch", [1, 3, 65])
def test_reason_route_every_branch_exact(batch):
    lib = _lib.load()
    n = len(CASES)
    seen = set()
    for j in range((n + batch - 1) // batch if batch < n else 1):
        rows = [CASES[(j * batch + r) % n] for r in range(batch)]
        seen.update(c[0] for c in rows)
        for with_forced in (True, False):
            rows_f = rows if with_forced else [c[:3] + (-1,) + c[4:] for c in rows]
            got, want = run_route(lib, rows_f, with_forced)
            for name, g, w in zip(("phase", "n_reason", "n_answer", "kind", "ground", "suppress", "x"), got, want):
                assert np.array_equal(g, w), (name, [c[0] for c in rows_f], g.tolist()[:8], w.tolist()[:8])
            for r, c in enumerate(rows_f):  # idle rows: every output still holds the sentinel
                if c[1] < 0:
                    assert got[3][r] == SENT and got[4][r] == SENT and (got[5][r] == SENT).all() and (got[6][r] == SENT).all()
                else:  # x beyond D: the padding of the row stays
                    assert (got[6][r, DIM:] == SENT).all()
            if not with_forced:  # forced == NULL equals an all -1 plane
                got_m1, _ = run_route(lib, rows_f, True)
                for g, g1 in zip(got, got_m1):
                    assert np.array_equal(g, g1)
    assert seen == {c[0] for c in CASES}


def test_reason_route_expected_values_of_the_named_branches():
    """The restatement itself, pinned on the branches the contract spells out (so that a shared mistake cannot hide)."""
    lib = _lib.load()
    got, _ = run_route(lib, CASES, True)
    phase, nr, na, kind, ground, sup, x = got
    by = {c[0]: i for i, c in enumerate(CASES)}
    i = by["reason, coordinate token"]
    assert (phase[i], nr[i], kind[i]) == (REASON, 1, K_REASON) and ground[i] >= 0 and sup[i].tolist() == [EOS_ID, SIZE_ID]
    i = by["reason ends on answer_id"]
    assert (phase[i], nr[i], kind[i], ground[i]) == (ANSWER, 2, K_SUFFIX, -1) and sup[i].tolist() == [-1, -1]
    i = by["reason ends on the budget"]
    assert (phase[i], nr[i], kind[i]) == (ANSWER, MAX_REASON, K_SUFFIX)
    i = by["reason, last token inside the budget"]
    assert (phase[i], nr[i], kind[i]) == (REASON, MAX_REASON, K_REASON)
    i = by["answer continues"]
    assert (phase[i], na[i], kind[i]) == (ANSWER, 2, K_ANSWER) and sup[i].tolist() == [ANSWER_ID, -1]
    i = by["answer ends on eos_id"]
    assert (phase[i], na[i], kind[i]) == (DONE, 1, K_NONE) and sup[i].tolist() == [-1, -1]
    i = by["answer ends on the budget"]
    assert (phase[i], na[i], kind[i]) == (DONE, MAX_ANSWER, K_NONE)
    i = by["forced: an ordinary token becomes answer_id"]
    assert (phase[i], kind[i]) == (ANSWER, K_SUFFIX)
    i = by["forced 0 is a forced eos, not 'unforced'"]
    assert (phase[i], kind[i], nr[i]) == (REASON, K_REASON, 2)  # eos_id is an ordinary token while reasoning


@pytest.mark.parametrize("vocab,ld", [(51200, 51208), (1021, 1030)])
def test_mask_logits_rows_exact(vocab, ld):
    lib = _lib.load()
    ids = np.array([[5, 17], [vocab - 1, -1], [-1, -1], [9, 9], [-1, vocab - 1], [0, vocab - 2], [vocab, 3], [-7, vocab + 5]], dtype=np.int32)
    b = len(ids)
    rng = np.random.default_rng(vocab)
    buf = rng.integers(-32768, 32767, (b, ld), dtype=np.int16)
    want = buf.copy()
    for r in range(b):
        for k in range(2):
            if 0 <= ids[r, k] < vocab:
                want[r, ids[r, k]] = np.int16(-128)  # 0xff80: bf16 -inf
    lg, idd = dev(buf, torch.int16), dev(ids)
    _lib.check(lib.md_mask_logits_rows(lg.data_ptr(), ld, b, vocab, idd.data_ptr(), stream()), "md_mask_logits_rows")
    torch.cuda.synchronize()
    got = lg.cpu().numpy()
    assert np.array_equal(got, want)  # every other bit, the padding columns included
    assert np.array_equal(got[2], buf[2]) and np.array_equal(got[7], buf[7])  # rows with nothing to mask: untouched
    assert np.array_equal(idd.cpu().numpy(), ids)
    assert torch.isinf(lg.view(BF16)[0, 5]) and float(lg.view(BF16)[0, 5]) < 0


# ------------------------------------------------------------------ one fused step against its pieces
@pytest.fixture(scope="module")
def tiny_prefilled():
    from moondream_amd.moondream import IdTokenizer, MoondreamModel, _Rows

    cfg = get_config("tiny")
    sd = synth.synthetic_state_dict(cfg, seed=1, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=4)
    tk = cfg.tokenizer
    tpl = tk.templates["query"]
    prompt = list(tpl["prefix"]) + [11, 12, 13] + list(tpl["suffix"]) + [tk.thinking_id]
    imgs = [synth.synthetic_image(i, 1) for i in range(4)]
    with torch.inference_mode():
        prep = model._prepare_sequences(imgs, [prompt] * 4, rows=_Rows())
    assert list(prep.order) == [0, 1, 2, 3]
    return cfg, model, prep.hidden_last.clone(), prep.next_pos


def fused_step(model, cfg, hidden, tokens, pos, rows):
    """One md_decode_step_reason through the model's own call site, over fresh state."""
    b = len(tokens)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    st = dict(phase=i32(b), nr=i32(b), na=i32(b), sup=torch.full((b, 2), -9, dtype=torch.int32, device="cuda"), bin=i32(b),
              hp=hidden.clone(), kind=i32(1, b), ground=i32(1, b))
    region = model._region_coord()
    reason = ReasonChunk(st["phase"], st["nr"], st["na"], st["sup"], st["bin"], st["hp"], st["kind"], st["ground"], 8, 8, region)
    need = model.lib.md_decode_reason_workspace_bytes(C.byref(model.w.text), C.byref(region), b)
    logits = model._decode_logits(b)
    pos_buf = dev(pos)
    model._decode_step_reason(rows, reason, 0, dev(tokens), pos_buf, b, logits, model._workspace(need, 2), model._kv_struct(0))
    torch.cuda.synchronize()
    return st, logits[:b].clone(), pos_buf


def pieces_step(model, cfg, hidden, tokens, pos, rows):
    """The same step from the existing pieces, at the same batch size."""
    tk = cfg.tokenizer
    b = len(tokens)
    bins = torch.zeros(b, 1, dtype=torch.int32, device="cuda")
    coord = model._region_pick_encode(hidden, "coord", bins)
    ends = torch.tensor([t == tk.answer_id for t in tokens], device="cuda")
    fed = [tk.templates["query"]["suffix"][0] if t == tk.answer_id else t for t in tokens]
    emb = model._embed(torch.tensor(fed, dtype=torch.int32).reshape(b, 1)).reshape(b, -1)
    is_coord = torch.tensor([t == tk.coord_id for t in tokens], device="cuda")
    x = torch.where(is_coord[:, None], coord, emb)
    h = model._text_forward(x.reshape(b, 1, -1), pos, rows)
    logits = model._lm_head(h).clone()
    keep = torch.nonzero(~ends).reshape(-1)
    for tid in (tk.eos_id, tk.size_id):
        logits[keep, tid] = float("-inf")
    return bins.reshape(-1), h.reshape(b, -1), logits, is_coord, ends


def test_decode_step_reason_equals_the_step_from_pieces(tiny_prefilled):
    from moondream_amd.moondream import _Rows

    cfg, model, hidden, next_pos = tiny_prefilled
    tk = cfg.tokenizer
    seq_tokens = [tk.coord_id, 17, tk.coord_id, tk.answer_id]  # per SEQUENCE (= KV slot)
    bits = lambda t: t.contiguous().view(torch.int16)
    results = {}
    with torch.inference_mode():
        for name, perm in (("plain", [0, 1, 2, 3]), ("slots", [2, 0, 3, 1])):
            rows = _Rows() if name == "plain" else _Rows(slots=dev(perm), n_slots=4)
            tokens = [seq_tokens[s] for s in perm]  # row r carries sequence perm[r]
            hid, pos = hidden[perm].contiguous(), [next_pos[s] for s in perm]
            bins, h, lg, is_coord, ends = pieces_step(model, cfg, hid, tokens, pos, rows)
            st, lg_f, pos_buf = fused_step(model, cfg, hid, tokens, pos, rows)
            assert torch.equal(bits(st["hp"]), bits(h)), name            # hidden_prev (out)
            assert torch.equal(bits(lg_f), bits(lg)), name               # the masked logits, -inf included
            assert torch.equal(st["bin"], bins), name                    # the coordinate bin of every row
            assert pos_buf.tolist() == [p + 1 for p in pos]
            want_kind = [K_SUFFIX if e else K_REASON for e in ends.tolist()]
            assert st["kind"][0].tolist() == want_kind
            assert st["phase"].tolist() == [ANSWER if e else REASON for e in ends.tolist()]
            assert st["nr"].tolist() == [0 if e else 1 for e in ends.tolist()] and st["na"].tolist() == [0] * 4
            assert st["ground"][0].tolist() == [int(bins[r]) if c else -1 for r, c in enumerate(is_coord.tolist())]
            assert st["sup"].tolist() == [[-1, -1] if e else [tk.eos_id, tk.size_id] for e in ends.tolist()]
            for r in range(4):  # the mask is where the rule says, and nowhere on the row that feeds the suffix
                masked = torch.isinf(lg_f[r].float()) & (lg_f[r].float() < 0)
                assert masked.nonzero().reshape(-1).tolist() == ([] if ends[r] else sorted({tk.eos_id, tk.size_id}))
            results[name] = (perm, st["hp"].clone(), lg_f, st["bin"].clone())
    # the slot table changes addresses only: a sequence gets the same bits in whichever row it travels
    perm, hp, lg, bn = results["slots"]
    _, hp0, lg0, bn0 = results["plain"]
    for r, s in enumerate(perm):
        assert torch.equal(bits(hp[r]), bits(hp0[s])) and torch.equal(bits(lg[r]), bits(lg0[s])) and int(bn[r]) == int(bn0[s])
