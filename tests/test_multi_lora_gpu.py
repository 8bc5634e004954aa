"""Mixed LoRA variants on the MI355X: the grouped shrink / expand kernels against fp32 torch and their row independence, the
mixed decoder call against per-variant calls and against md_text_forward_lora, and mixed batch_generate_ids against the
reference's recorded ids (tests/golden/*_lora.npz)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

from moondream_amd import _lib, synth
from moondream_amd.config import get_config
from moondream_amd.moondream import _Rows

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
QKV_PROJ_FC1 = _lib.MD_LORA_QKV | _lib.MD_LORA_PROJ | _lib.MD_LORA_FC1


def load_golden(golden_dir, name):
    path = os.path.join(golden_dir, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not generated")
    return np.load(path)


def build(cfg_name, seed, max_batch=4):
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(cfg_name)
    sd = synth.synthetic_state_dict(cfg, seed=seed, device="cuda")
    return cfg, sd, MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=max_batch)


def dev(a):
    return torch.tensor(list(a), dtype=torch.int32, device="cuda")


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def tiny128():
    cfg, sd, model = build("tiny", 7, max_batch=128)
    # four variants: ranks 8, 64, 256, and one without fc2 in layer 1 and without proj anywhere
    odd = synth.synthetic_lora(cfg, seed=4, rank=8, device="cuda")
    del odd["text"]["blocks"]["1"]["mlp"]["fc2"]
    for blk in odd["text"]["blocks"].values():
        del blk["attn"]["proj"]
    variants = {"r8": synth.synthetic_lora(cfg, seed=1, rank=8, device="cuda"),
                "r64": synth.synthetic_lora(cfg, seed=2, rank=64, device="cuda"),
                "r256": synth.synthetic_lora(cfg, seed=3, rank=256, device="cuda"), "odd": odd}
    for k, v in variants.items():
        model.register_variant(k, v)
        model._bank_index(k)
    return cfg, model, variants


def pair_of(variants, name, layer, pair):
    group = "attn" if pair in ("qkv", "proj") else "mlp"
    return variants[name]["text"]["blocks"][str(layer)][group].get(pair)


def random_table(rng, batch, n_var):
    return [int(v) for v in rng.integers(-1, n_var, batch)]


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("batch,q_len", [(1, 1), (7, 1), (64, 1), (65, 1), (128, 1), (3, 730), (2, 33)])
def test_shrink_and_expand_match_fp32_torch(tiny128, batch, q_len):
    cfg, model, variants = tiny128
    lib, bank = model.lib, model._bank
    names = sorted(bank.index, key=bank.index.get)
    rng = np.random.default_rng(batch * 1000 + q_len)
    table = random_table(rng, batch, len(names))
    table[0] = 2 if batch > 1 else table[0]  # the rank-256 variant is always present
    M, D, layer = batch * q_len, cfg.text.dim, 1
    g = torch.Generator(device="cuda").manual_seed(batch + q_len)
    # asymmetric data: a row- and column-dependent offset (an identity-like A would hide a transposed operand)
    x = (torch.randn(M, D, generator=g, device="cuda") + torch.linspace(-1, 2, D, device="cuda")).to(BF16)
    ldt = max(16, max(sum(bank.struct.rank[v][:3]) for v in range(len(names))))
    t = torch.full((M, ldt), float("nan"), dtype=BF16, device="cuda")
    vt = dev(table)
    _lib.check(lib.md_lora_shrink_grouped(C.byref(bank.struct), layer, QKV_PROJ_FC1, vt.data_ptr(), batch, q_len, x.data_ptr(), D, D,
                                          t.data_ptr(), ldt, stream()), "shrink")
    # expand of the fc1 pair with GELU from column 64, in place on a random base
    n = cfg.text.ff_dim
    base = (torch.randn(M, n, generator=g, device="cuda") * 2).to(BF16)
    out = base.clone()
    _lib.check(lib.md_lora_expand_grouped(C.byref(bank.struct), layer, 2, QKV_PROJ_FC1, vt.data_ptr(), batch, q_len, t.data_ptr(), ldt,
                                          out.data_ptr(), n, n, _lib.MD_LORA_ADD, 64, stream()), "expand")
    delta = torch.full((M, D), float("nan"), dtype=BF16, device="cuda")
    _lib.check(lib.md_lora_expand_grouped(C.byref(bank.struct), layer, 1, QKV_PROJ_FC1, vt.data_ptr(), batch, q_len, t.data_ptr(), ldt,
                                          delta.data_ptr(), D, D, _lib.MD_LORA_DELTA, -1, stream()), "expand delta")
    torch.cuda.synchronize()
    gelu = lambda v: torch.nn.functional.gelu(v, approximate="tanh")
    for b in range(batch):
        rows = slice(b * q_len, (b + 1) * q_len)
        v = table[b]
        if v < 0:
            assert torch.equal(out[rows, :64], base[rows, :64])
            assert (out[rows, 64:].float() - gelu(base[rows, 64:].float())).abs().max() < 2e-2
            assert not delta[rows].float().any()
            continue
        off = 0
        for q, pname in enumerate(("qkv", "proj", "fc1")):
            r = bank.struct.rank[v][q]
            p = pair_of(variants, names[v], layer, pname)
            if p is None:
                continue
            want = x[rows].float() @ p["A"].float().T
            got = t[rows, off : off + p["A"].shape[0]].float()
            assert torch.allclose(got, want, rtol=1e-2, atol=1e-2 * want.abs().max().item()), (b, pname)
            off += r
        f1 = pair_of(variants, names[v], layer, "fc1")
        rf1 = f1["A"].shape[0]
        off_fc1 = bank.struct.rank[v][0] + bank.struct.rank[v][1]
        d_ref = (t[rows, off_fc1 : off_fc1 + rf1].float() @ f1["B"].float().T).to(BF16).float()
        want = (base[rows].float() + d_ref).to(BF16).float()
        want[:, 64:] = gelu(want[:, 64:])
        assert torch.allclose(out[rows].float(), want, rtol=2e-2, atol=2e-2 * want.abs().max().item()), b
        pj = pair_of(variants, names[v], layer, "proj")
        if pj is None:
            assert not delta[rows].float().any()
        else:
            off_pj = bank.struct.rank[v][0]
            d_ref = t[rows, off_pj : off_pj + pj["A"].shape[0]].float() @ pj["B"].float().T
            assert torch.allclose(delta[rows].float(), d_ref, rtol=2e-2, atol=2e-2 * d_ref.abs().max().item()), b

    # row independence: the sequences permuted and every OTHER row's variant changed -> each row's bits unchanged
    if batch > 1:
        perm = rng.permutation(batch)
        table2 = [table[p] for p in perm]
        src = torch.tensor(perm, device="cuda")
        x2 = x.view(batch, q_len, D)[src].reshape(M, D).contiguous()
        # change the variant of every row but the first of the permuted order, and compare that row only
        keep = int(perm[0])
        table3 = [table2[0]] + [(v + 2) % len(names) - 1 for v in table2[1:]]
        for tab in (table2, table3):
            t2 = torch.full_like(t, float("nan"))
            vt2 = dev(tab)
            _lib.check(lib.md_lora_shrink_grouped(C.byref(bank.struct), layer, QKV_PROJ_FC1, vt2.data_ptr(), batch, q_len, x2.data_ptr(),
                                                  D, D, t2.data_ptr(), ldt, stream()), "shrink")
            out2 = base.view(batch, q_len, n)[src].reshape(M, n).contiguous()
            _lib.check(lib.md_lora_expand_grouped(C.byref(bank.struct), layer, 2, QKV_PROJ_FC1, vt2.data_ptr(), batch, q_len,
                                                  t2.data_ptr(), ldt, out2.data_ptr(), n, n, _lib.MD_LORA_ADD, 64, stream()), "expand")
            torch.cuda.synchronize()
            check = range(batch) if tab is table2 else range(1)
            for i in check:
                s0, s1 = int(perm[i]) * q_len, (int(perm[i]) + 1) * q_len
                w = bank.struct.rank[table[perm[i]]] if table[perm[i]] >= 0 else None
                width = sum(w[:3]) if w is not None else 0
                assert torch.equal(t2[i * q_len : (i + 1) * q_len, :width], t[s0:s1, :width]), (i, keep)
                assert torch.equal(out2[i * q_len : (i + 1) * q_len], out[s0:s1]), i


# ------------------------------------------------------------------ decoder: mixed vs uniform calls
def decode_logits(model, x, pos, multi=None, lora=None):
    h = model._text_forward(x, pos, _Rows(variants=multi, bank=model._bank if multi is not None else None, lora=lora))
    return model._lm_head(h)


@pytest.mark.parametrize("batch", [64, 128])
def test_mixed_step_rows_equal_uniform_calls(tiny128, batch):
    """A decode-shaped call (q_len 1) with mixed variants: every row's logits are bit-identical to the same-size call in which
    EVERY row carries that row's variant; each call writes only position pos of its rows' slots."""
    cfg, model, variants = tiny128
    names = sorted(model._bank.index, key=model._bank.index.get)
    rng = np.random.default_rng(batch)
    table = random_table(rng, batch, len(names))
    g = torch.Generator(device="cuda").manual_seed(batch)
    x = torch.randn(batch, 1, cfg.text.dim, generator=g, device="cuda").to(BF16)
    pos = [int(p) for p in rng.integers(1, 40, batch)]
    with torch.inference_mode():
        mixed = decode_logits(model, x, pos, multi=model._variant_table(table)).clone()
        for v in sorted(set(table)):
            uni = decode_logits(model, x, pos, multi=model._variant_table([v] * batch)).clone()
            rows = [i for i in range(batch) if table[i] == v]
            assert torch.equal(mixed[rows], uni[rows]), (v, rows[:4])
        # the base rows also equal the base path within bf16 noise (two roundings of the fused GELU differ)
        base = decode_logits(model, x, pos).clone()
        rows = [i for i in range(batch) if table[i] < 0]
        if rows:
            assert (mixed[rows].float() - base[rows].float()).abs().max() < 0.5


def test_uniform_variant_agrees_with_the_single_variant_path(tiny128):
    cfg, model, variants = tiny128
    g = torch.Generator(device="cuda").manual_seed(5)
    for name in ("r8", "r64"):
        for b, t in ((4, 1), (2, 20)):
            x = torch.randn(b, t, cfg.text.dim, generator=g, device="cuda").to(BF16)
            with torch.inference_mode():
                idx = model._bank.index[name]
                got = decode_logits(model, x, 3, multi=model._variant_table([idx] * b)).clone()
                want = decode_logits(model, x, 3, lora=model._lora({"variant": name})).clone()
            top = want.float().topk(8, dim=-1).indices
            assert (got.float().gather(1, top) - want.float().gather(1, top)).abs().max() < 0.5, name


def test_variant_table_follows_the_slot_order_of_the_prompt_lengths(tiny128):
    """Prompt lengths [5, 3, 4]: the slots are not in the caller's order, and each row must still carry ITS variant.  Every
    row's ids are bit-equal to its ids in the same mixed call with the caller's rows already in length order (where the
    table needs no permutation)."""
    cfg, model, variants = tiny128
    imgs = [synth.synthetic_image(i, 5) for i in range(3)]
    prompts = [[11, 12, 13, 14, 15], [21, 22, 23], [31, 32, 33, 34]]
    names = ["r8", None, "r64"]
    by_length = [1, 2, 0]
    pick = lambda xs, idx: [xs[i] for i in idx]
    got = model.batch_generate_ids(imgs, prompts, max_tokens=6, ignore_eos=True, variants=names)
    want = model.batch_generate_ids(pick(imgs, by_length), pick(prompts, by_length), max_tokens=6, ignore_eos=True,
                                    variants=pick(names, by_length))
    assert pick(got, by_length) == want
    # the check can see a table left in the caller's order: slot s holds caller by_length[s], so callers 1 and 2 would trade
    # the base model for an adapter, which flips their ids by construction (synth.synthetic_lora)
    misplaced = model.batch_generate_ids(imgs, prompts, max_tokens=6, ignore_eos=True, variants=["r64", "r8", None])
    assert misplaced[1] != got[1] and misplaced[2] != got[2]


# ------------------------------------------------------------------ goldens through batch_generate_ids
def mixed_goldens(model, cfg, g, use_graphs):
    model.register_variant("synthetic", synth.synthetic_lora(cfg, seed=int(g["seed"]), rank=int(g["rank"]), device="cuda"))
    imgs = [Image.fromarray(synth.synthetic_image_array(int(g[f"case{i}.image_index"]), int(g["seed"]), (378, 378)), "RGB")
            for i in range(2)]
    n = len(g["case0.tokens"])
    prompt = cfg.tokenizer.templates["caption"]["normal"]
    want = [g["case0.tokens"].tolist(), g["case0.base_tokens"].tolist(), g["case1.tokens"].tolist(), g["case1.base_tokens"].tolist()]
    assert want[0][0] != want[1][0]
    prev = model.use_graphs
    try:
        model.use_graphs = use_graphs
        for _ in range(2 if use_graphs else 1):  # with graphs: capture, then replay
            got = model.batch_generate_ids([imgs[0], imgs[0], imgs[1], imgs[1]], [prompt] * 4, max_tokens=n,
                                           variants=["synthetic", None, "synthetic", None])
            assert got == want
        # the string API: settings={"variants": [...]}
        caps = model.batch_caption([imgs[0], imgs[1]], settings={"temperature": 0, "max_tokens": n, "variants": ["synthetic", None]})
        assert [[int(t) for t in c.split()] for c in caps] == [want[0], want[3]]
        # another order of the same requests
        got = model.batch_generate_ids([imgs[1], imgs[0], imgs[1], imgs[0]], [prompt] * 4, max_tokens=n,
                                       variants=[None, None, "synthetic", "synthetic"])
        assert got == [want[3], want[1], want[2], want[0]]
    finally:
        model.use_graphs = prev


def test_mixed_batch_matches_reference_tiny(golden_dir):
    g = load_golden(golden_dir, "tiny_lora.npz")
    cfg, sd, model = build(str(g["cfg"]), 0, max_batch=4)
    mixed_goldens(model, cfg, g, use_graphs=False)
    mixed_goldens(model, cfg, g, use_graphs=True)


def test_mixed_batch_matches_reference_2b(golden_dir):
    g = load_golden(golden_dir, "md2b_lora.npz")
    cfg, sd, model = build("2b", 0, max_batch=128)
    mixed_goldens(model, cfg, g, use_graphs=True)
    engine_goldens(model, cfg, g)
    # two LoRA variants in one B = 64 decode-shaped call: per-row logits equal the uniform calls'
    model.register_variant("s1", synth.synthetic_lora(cfg, seed=1, rank=8, device="cuda"))
    model.register_variant("s2", synth.synthetic_lora(cfg, seed=2, rank=64, device="cuda"))
    ids = [-1, model._bank_index("s1"), model._bank_index("s2")]
    for batch in (64, 128):
        table = [ids[i % 3] for i in range(batch)]
        gen = torch.Generator(device="cuda").manual_seed(batch)
        x = torch.randn(batch, 1, cfg.text.dim, generator=gen, device="cuda").to(BF16)
        with torch.inference_mode():
            mixed = decode_logits(model, x, 800, multi=model._variant_table(table)).clone()
            for v in ids:
                uni = decode_logits(model, x, 800, multi=model._variant_table([v] * batch)).clone()
                rows = [i for i in range(batch) if table[i] == v]
                assert torch.equal(mixed[rows], uni[rows]), (batch, v)
    with torch.inference_mode():
        x = torch.randn(4, 1, cfg.text.dim, generator=gen, device="cuda").to(BF16)
        got = decode_logits(model, x, 800, multi=model._variant_table([ids[2]] * 4)).float()
        want = decode_logits(model, x, 800, lora=model._lora({"variant": "s2"})).float()
    top = want.topk(8, dim=-1).indices
    assert (got.gather(1, top) - want.gather(1, top)).abs().max() < 0.5


# ------------------------------------------------------------------ md_decode_step_multi_lora directly
def decode_step(model, bank, table, tokens, pos, batch):
    """One md_decode_step_multi_lora over slots 0 .. batch-1 (bank None: the md_decode_step_slots case); returns (logits, next)."""
    t = model.config.text
    logits = torch.empty(batch, t.vocab_size, dtype=BF16, device="cuda")
    nxt = torch.empty(batch, dtype=torch.int32, device="cuda")
    pos_d = pos.clone()
    bp = C.byref(bank.struct) if bank is not None else None
    need = model.lib.md_decode_multi_lora_workspace_bytes(C.byref(model.w.text), bp, batch)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    kv = model._kv_struct(0)
    _lib.check(model.lib.md_decode_step_multi_lora(C.byref(model.w.text), bp, table.data_ptr() if table is not None else None,
                                                   tokens.data_ptr(), nxt.data_ptr(), pos_d.data_ptr(), batch, None, 0, C.byref(kv),
                                                   model.config.tokenizer.answer_id, logits.data_ptr(), t.vocab_size, ws.data_ptr(),
                                                   ws.numel(), stream()), "md_decode_step_multi_lora")
    torch.cuda.synchronize()
    assert torch.equal(pos_d, pos + 1)
    return logits, nxt


@pytest.mark.parametrize("batch", [64, 128])
def test_decode_step_entry_point_rows_equal_uniform_steps(tiny128, batch):
    cfg, model, variants = tiny128
    bank = model._bank
    rng = np.random.default_rng(7 + batch)
    table = random_table(rng, batch, len(bank.index))
    tokens = dev(rng.integers(10, cfg.text.vocab_size, batch))
    pos = dev(rng.integers(1, 40, batch))
    with torch.inference_mode():
        mixed, nxt = decode_step(model, bank, dev(table), tokens, pos, batch)
        for v in sorted(set(table)):
            uni, unxt = decode_step(model, bank, dev([v] * batch), tokens, pos, batch)
            rows = [i for i in range(batch) if table[i] == v]
            assert torch.equal(mixed[rows], uni[rows]) and torch.equal(nxt[rows], unxt[rows]), v
        # NULL bank: exactly md_decode_step_slots
        a, an = decode_step(model, None, None, tokens, pos, batch)
        ws = torch.empty(model.lib.md_decode_workspace_bytes(C.byref(model.w.text), batch), dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        bn = torch.empty_like(an)
        pos_d = pos.clone()
        kv = model._kv_struct(0)
        _lib.check(model.lib.md_decode_step_slots(C.byref(model.w.text), tokens.data_ptr(), bn.data_ptr(), pos_d.data_ptr(), batch, None, 0,
                                                  C.byref(kv), cfg.tokenizer.answer_id, b.data_ptr(), cfg.text.vocab_size, ws.data_ptr(),
                                                  ws.numel(), stream()), "md_decode_step_slots")
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(an, bn)


def test_block_split_of_a_mixed_step_equals_per_block_steps():
    """md_decode_step_multi_lora over 130 rows -- the smallest step that enters the block split of the C layer (blocks of 64 or
    128 rows) and leaves a ragged last block -- with a permuted slot table, one idle row and a table mixing base rows with two
    variants, against three calls over rows [0, 64), [64, 128), [128, 130) with the sub-tables: next, pos, the logits and the
    K / V slabs are bit-equal.  What the split must get right is the advance of every per-row table at once."""
    rows = 130
    cfg, sd, model = build("tiny", 7, max_batch=rows)
    for name, seed, rank in (("a", 1, 8), ("b", 2, 64)):
        model.register_variant(name, synth.synthetic_lora(cfg, seed=seed, rank=rank, device="cuda"))
        model._bank_index(name)
    bank, t, lib = model._bank, cfg.text, model.lib
    rng = np.random.default_rng(rows)
    slot_list = [int(v) for v in rng.permutation(rows)]
    idle = 70  # in the second block of 64, and not a block's first row
    slot_list[idle] = -1
    table = [(-1, 0, 1)[i % 3] for i in rng.permutation(rows)]
    # every block mixes the three kinds of row, and no block's sub-table equals the first block's: a table that does not
    # advance with the block changes the result
    assert {-1, 0, 1} == set(table[:64]) == set(table[64:128]) and table[64:128] != table[:64] and table[128:] != table[:2]
    tokens, pos0 = dev(rng.integers(10, t.vocab_size, rows)), dev(rng.integers(1, 40, rows))
    slots, variant = dev(slot_list), dev(table)
    g = torch.Generator(device="cuda").manual_seed(rows)
    k0 = torch.randn(model._kv_k.shape, generator=g, device="cuda").to(BF16)
    v0 = torch.randn(model._kv_v.shape, generator=g, device="cuda").to(BF16)
    ws = torch.empty(lib.md_decode_multi_lora_workspace_bytes(C.byref(model.w.text), C.byref(bank.struct), rows), dtype=torch.uint8,
                     device="cuda")
    kv = model._kv_struct(0)

    def run(blocks):
        model._kv_k.copy_(k0)
        model._kv_v.copy_(v0)
        logits = torch.zeros(rows, t.vocab_size, dtype=BF16, device="cuda")
        nxt = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
        pos = pos0.clone()
        for r0, r1 in blocks:
            _lib.check(lib.md_decode_step_multi_lora(C.byref(model.w.text), C.byref(bank.struct), variant[r0:].data_ptr(),
                                                     tokens[r0:].data_ptr(), nxt[r0:].data_ptr(), pos[r0:].data_ptr(), r1 - r0,
                                                     slots[r0:].data_ptr(), rows, C.byref(kv), cfg.tokenizer.answer_id,
                                                     logits[r0:].data_ptr(), t.vocab_size, ws.data_ptr(), ws.numel(), stream()),
                       "md_decode_step_multi_lora")
        torch.cuda.synchronize()
        return logits, nxt, pos, model._kv_k.clone(), model._kv_v.clone()

    with torch.inference_mode():
        one = run([(0, rows)])
        three = run([(0, 64), (64, 128), (128, rows)])
    for name, a, b in zip(("logits", "next", "pos", "K", "V"), one, three):
        assert torch.equal(a, b), name
    logits, nxt, pos, k1, v1 = one
    assert torch.equal(pos, pos0 + 1)
    # the step wrote exactly one K / V row per live row: position pos0 of its own slot
    live = [i for i in range(rows) if i != idle]
    changed = (k1 != k0).any(dim=-1).any(dim=0).any(dim=1)  # [slot][position]
    want = torch.zeros_like(changed)
    want[slots[live].long(), pos0[live].long()] = True
    assert torch.equal(changed, want)


def test_reregistered_variant_replaces_the_bank_copy(tiny128):
    cfg, model, variants = tiny128
    model.register_variant("rr", synth.synthetic_lora(cfg, seed=11, rank=8, device="cuda"))
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(4, 1, cfg.text.dim, generator=g, device="cuda").to(BF16)
    with torch.inference_mode():
        idx = model._bank_index("rr")
        gen0 = model._bank.generation
        old = decode_logits(model, x, 5, multi=model._variant_table([idx] * 4)).float()
        model.register_variant("rr", synth.synthetic_lora(cfg, seed=12, rank=64, device="cuda"))
        assert model._bank_index("rr") == idx and model._bank.generation > gen0 and model._bank.struct.rank[idx][0] == 64
        got = decode_logits(model, x, 5, multi=model._variant_table([idx] * 4)).float()
        want = decode_logits(model, x, 5, lora=model._lora({"variant": "rr"})).float()
    top = want.topk(8, dim=-1).indices
    assert (got.gather(1, top) - want.gather(1, top)).abs().max() < 0.5
    assert (old.gather(1, top) - want.gather(1, top)).abs().max() > 0.5  # the old adapter is no longer served


# ------------------------------------------------------------------ ContinuousEngine with variants
def engine_goldens(model, cfg, g):
    from moondream_amd.continuous import ContinuousEngine

    imgs = [Image.fromarray(synth.synthetic_image_array(int(g[f"case{i}.image_index"]), int(g["seed"]), (378, 378)), "RGB")
            for i in range(2)]
    n = len(g["case0.tokens"])
    prompt = cfg.tokenizer.templates["caption"]["normal"]
    want = [g["case0.tokens"].tolist(), g["case0.base_tokens"].tolist(), g["case1.tokens"].tolist(), g["case1.base_tokens"].tolist()]
    prev = model.use_graphs
    try:
        model.use_graphs = True
        for _ in range(2):  # capture, then replay
            eng = ContinuousEngine(model, max_live=4, chunk=4)
            rids = [eng.submit(im, prompt, max_tokens=n, variant=v)
                    for im, v in zip([imgs[0], imgs[0], imgs[1], imgs[1]], ["synthetic", None, "synthetic", None])]
            got = dict(eng.run())
            assert [got[r] for r in rids] == want
    finally:
        model.use_graphs = prev


def test_engine_mixed_variants_match_reference_tiny(golden_dir):
    g = load_golden(golden_dir, "tiny_lora.npz")
    cfg, sd, model = build(str(g["cfg"]), 0, max_batch=4)
    model.register_variant("synthetic", synth.synthetic_lora(cfg, seed=int(g["seed"]), rank=int(g["rank"]), device="cuda"))
    engine_goldens(model, cfg, g)


def test_engine_mixed_variants_eos_refill_and_sampling(tiny128):
    """Seven LoRA requests over four variants through three slots: refilled and permuted slots, idle bucket rows, per-request
    EOS.  Greedy ids equal batch_generate_ids(variants=...) truncated at each request's EOS; sampling with per-request seeds is
    reproducible."""
    from moondream_amd.continuous import ContinuousEngine

    cfg, model, variants = tiny128
    names = ["r8", "r64", "r256", "odd", "r64", "r8", "r256"]
    imgs = [synth.synthetic_image(i, 5) for i in range(len(names))]
    prompt = cfg.tokenizer.templates["caption"]["normal"]
    with torch.inference_mode():
        ref = model.batch_generate_ids(imgs, [prompt] * len(imgs), max_tokens=12, ignore_eos=True, variants=names)
    eos = [ref[i][2 + i % 5] for i in range(len(names))]
    want = [r[: r.index(e)] for r, e in zip(ref, eos)]
    prev = model.use_graphs
    try:
        for use_graphs in (False, True):
            model.use_graphs = use_graphs
            eng = ContinuousEngine(model, max_live=3, chunk=4)
            rids = [eng.submit(im, prompt, max_tokens=12, eos_id=e, variant=v) for im, e, v in zip(imgs, eos, names)]
            got = dict(eng.run())
            assert [got[r] for r in rids] == want, use_graphs
        runs = []
        for _ in range(2):
            eng = ContinuousEngine(model, max_live=3, chunk=4, temperature=0.7, top_p=0.9)
            rids = [eng.submit(im, prompt, max_tokens=10, seed=100 + i, ignore_eos=True, variant=v)
                    for i, (im, v) in enumerate(zip(imgs, names))]
            got = dict(eng.run())
            runs.append([got[r] for r in rids])
        assert runs[0] == runs[1] and all(len(r) == 10 for r in runs[0])
    finally:
        model.use_graphs = prev
