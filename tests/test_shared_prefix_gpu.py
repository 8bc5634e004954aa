"""Shared image prefix on the MI355X: the grouped decode kernel, md_text_forward_shared / md_decode_step_shared and the
model's shared mode give, bit for bit, what the slot-table functions give over slots into which the prefix was copied."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

from moondream_amd import _lib, synth
from moondream_amd.config import get_config

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
CTX = 2048


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


# ------------------------------------------------------------------ kernel: md_attention_decode_shared
def make_case(batch, n_heads, n_kv, plens_by_prefix, layout, seed, idle_every=0, per_row_plen=None, one_slot=False):
    """3 prefix slots (0..2) and one own slot per row (3 + b).  Returns the tables and two slab pairs: SHARED (own slots hold
    NaN below the row's prefix end -- a read there poisons the output) and COPY (the prefix copied into the own slot)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    n_slots = 3 + batch
    shape = (n_slots, n_kv, CTX, 64)
    k = (torch.randn(shape, generator=g, device="cuda") * 0.5).to(BF16)
    v = (torch.randn(shape, generator=g, device="cuda") * 0.5).to(BF16)
    pref, plen, kvl, slots = [], [], [], []
    for b in range(batch):
        p = 0 if one_slot else (b % 3) if layout == "interleaved" else (3 * b) // batch
        pl = per_row_plen[b % len(per_row_plen)] if per_row_plen else plens_by_prefix[p]
        pref.append(p if pl > 0 else -1)
        plen.append(pl)
        kvl.append(min(CTX, pl + 1 + int(rng.integers(0, 40))))
        slots.append(-1 if idle_every and b % idle_every == idle_every - 1 else 3 + b)
    ks, vs = k.clone(), v.clone()
    kc, vc = k.clone(), v.clone()
    nan = torch.tensor(float("nan"), dtype=BF16, device="cuda")
    for b in range(batch):
        s, p, pl = slots[b], pref[b], plen[b]
        if s < 0 or pl == 0:
            continue
        ks[s, :, :pl] = nan
        vs[s, :, :pl] = nan
        kc[s, :, :pl] = k[p, :, :pl]
        vc[s, :, :pl] = v[p, :, :pl]
    return dict(slots=slots, pref=pref, plen=plen, kvl=kvl, n_slots=n_slots, shared=(ks, vs), copy=(kc, vc))


def attend(lib, fused, q, kv, c, n_heads, n_kv, prefix):
    k, v = kv
    batch = len(c["slots"])
    o = torch.full((batch, n_heads * 64), 7.0, dtype=BF16, device="cuda")
    bs = n_kv * CTX * 64
    sl, kl = dev(c["slots"]), dev(c["kvl"])
    ps, pl = (dev(c["pref"]), dev(c["plen"])) if prefix else (None, None)
    ps_p = ps.data_ptr() if prefix else None
    pl_p = pl.data_ptr() if prefix else None
    scale = 1.0 / 8.0
    if fused:
        freqs = synth_freqs()
        st = lib.md_attention_decode_rope_shared(q.data_ptr(), q.shape[1], o.data_ptr(), o.shape[1], freqs.data_ptr(), k.data_ptr(),
                                                 v.data_ptr(), bs, CTX, kl.data_ptr(), batch, n_heads, 64, 32, scale, sl.data_ptr(),
                                                 c["n_slots"], ps_p, pl_p, stream())
    else:
        st = lib.md_attention_decode_shared(q.data_ptr(), q.shape[1], o.data_ptr(), o.shape[1], k.data_ptr(), v.data_ptr(), bs, CTX,
                                            kl.data_ptr(), batch, n_heads, n_kv, 64, scale, sl.data_ptr(), c["n_slots"], ps_p, pl_p,
                                            stream())
    _lib.check(st, "decode attention")
    torch.cuda.synchronize()
    return o


_FREQS = None


def synth_freqs():
    global _FREQS
    if _FREQS is None:
        pos = torch.arange(CTX, dtype=torch.float32)[:, None]
        inv = 1.0 / (10000 ** (torch.arange(16, dtype=torch.float32) / 16))
        ang = pos * inv
        _FREQS = torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous().cuda()
    return _FREQS


def check_kernel(batch, fused, layout, plens_by_prefix=(730, 128, 2000), n_heads=8, n_kv=8, idle_every=0, per_row_plen=None, seed=0,
                 one_slot=False):
    lib = _lib.load()
    c = make_case(batch, n_heads, n_kv, plens_by_prefix, layout, seed, idle_every, per_row_plen, one_slot)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    width = (n_heads + 2 * n_kv) * 64 if fused else n_heads * 64
    q = (torch.randn(batch, width, generator=g, device="cuda")).to(BF16)
    ks0, vs0 = (t.clone() for t in c["shared"])
    ref = attend(lib, fused, q, c["copy"], c, n_heads, n_kv, prefix=False)   # the slot-table launch over copied prefixes
    got = attend(lib, fused, q, c["shared"], c, n_heads, n_kv, prefix=True)  # the grouped kernel
    live = [b for b in range(batch) if c["slots"][b] >= 0]
    idle = [b for b in range(batch) if c["slots"][b] < 0]
    assert torch.isfinite(got[live].float()).all(), "a NaN key below a row's prefix end was read"
    bad = [b for b in live if not torch.equal(got[b], ref[b])]
    assert not bad, f"rows {bad[:8]} differ (plen {[c['plen'][b] for b in bad[:8]]}, kv_len {[c['kvl'][b] for b in bad[:8]]})"
    if idle:
        assert not got[idle].float().any() and not ref[idle].float().any()
    ks, vs = c["shared"]
    kc, vc = c["copy"]
    # the prefix slots and every slot no live row owns are untouched; own slots: the rows at and past the prefix end equal
    # the copy path's (FUSED: including the new K / V row at kv_len - 1)
    untouched = [0, 1, 2] + [3 + b for b in idle]
    for a, a0 in ((ks, ks0), (vs, vs0)):
        assert torch.equal(a[untouched].view(torch.int16), a0[untouched].view(torch.int16)), "a prefix or idle slot was written"
    for b in live:
        s, pl = c["slots"][b], c["plen"][b]
        assert torch.equal(ks[s, :, pl:], kc[s, :, pl:]) and torch.equal(vs[s, :, pl:], vc[s, :, pl:])
        if not fused:
            assert torch.equal(ks[s, :, pl:], ks0[s, :, pl:])


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("batch", [1, 7, 64, 128, 160])
@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_decode_kernel_equals_copied_slots(batch, fused, layout):
    """One prefix length per prefix slot: whole groups share a prefix (the one-load-per-group path) where rows are
    contiguous; interleaved rows mix slots inside a group (the per-row path).  batch * 8 heads spans both wave shapes of
    the reference kernel."""
    check_kernel(batch, fused, layout, idle_every=5 if batch >= 7 else 0)


@pytest.mark.parametrize("fused", [False, True])
def test_decode_kernel_prefix_lengths_and_ragged_groups(fused):
    """prefix_len in {0, 1, 127, 128, 730, 2000} per row (0: no shared prefix), ragged kv_len inside a group."""
    for layout in ("contiguous", "interleaved"):
        check_kernel(64, fused, layout, per_row_plen=[730, 730, 1, 127, 128, 0, 2000, 730], seed=3)
    for pl in (1, 127, 128, 730, 2000):
        check_kernel(32, fused, "contiguous", plens_by_prefix=(pl, pl, pl), seed=pl)


@pytest.mark.parametrize("fused", [False, True])
def test_decode_kernel_one_prefix_slot_different_prefix_lengths(fused):
    """Every row of a group on one prefix slot, prefix lengths all >= 128 but different: the shared rounds stop at the
    group's smallest prefix end and each row reads its remaining prefix keys from the prefix slot on its own."""
    check_kernel(16, fused, "contiguous", per_row_plen=[730, 2000, 300, 1000], seed=21, one_slot=True)
    check_kernel(12, fused, "contiguous", per_row_plen=[1000, 129, 640, 1999, 256, 383], seed=22, one_slot=True)


def test_decode_kernel_grouped_kv_heads():
    """n_kv_heads < n_heads (the non-FUSED kernel supports it)."""
    check_kernel(64, False, "contiguous", n_heads=8, n_kv=2, idle_every=9)
    check_kernel(7, False, "interleaved", n_heads=8, n_kv=4)


def test_decode_kernel_masked_rounds_add_exact_zeros():
    """A group whose rows' kv_len differ by several 128-key rounds: the short rows run the long row's rounds masked."""
    check_kernel(8, False, "contiguous", per_row_plen=[130, 1500], seed=11)
    check_kernel(8, True, "contiguous", per_row_plen=[1900, 5], seed=12)


# ------------------------------------------------------------------ library: md_text_forward_shared / md_decode_step_shared
class Slab:
    def __init__(self, cfg, n_slots):
        t = cfg.text
        self.k = torch.zeros(t.n_layers, n_slots, t.n_kv_heads, t.max_context, t.head_dim, dtype=BF16, device="cuda")
        self.v = torch.zeros_like(self.k)
        bs = t.n_kv_heads * t.max_context * t.head_dim
        self.kv = _lib.MdKvCache(self.k.data_ptr(), self.v.data_ptr(), n_slots * bs, bs, t.max_context)
        self.n_slots = n_slots


def rand_x(b, t, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, t, d, generator=g) * 0.5).to(BF16).cuda()


def forward(model, slab, x, pos, slots, prefix=None):
    lib, text = model.lib, model.w.text
    b, t, _ = x.shape
    hidden = torch.empty_like(x)
    pos0 = dev(pos)
    ws = torch.empty(lib.md_text_workspace_bytes(C.byref(text), b, t), dtype=torch.uint8, device="cuda")
    sl = dev(slots)
    if prefix is None:
        st = lib.md_text_forward_slots(C.byref(text), x.data_ptr(), hidden.data_ptr(), b, t, pos0.data_ptr(), sl.data_ptr(),
                                       slab.n_slots, C.byref(slab.kv), ws.data_ptr(), ws.numel(), stream())
    else:
        ps, pl = dev(prefix[0]), dev(prefix[1])
        st = lib.md_text_forward_shared(C.byref(text), x.data_ptr(), hidden.data_ptr(), b, t, pos0.data_ptr(), sl.data_ptr(),
                                        slab.n_slots, ps.data_ptr(), pl.data_ptr(), C.byref(slab.kv), ws.data_ptr(), ws.numel(),
                                        stream())
    _lib.check(st, "forward")
    torch.cuda.synchronize()
    return hidden


def decode_step(model, slab, tokens, pos, slots, prefix=None):
    lib, text, t = model.lib, model.w.text, model.config.text
    b = len(tokens)
    tok, nxt, posd = dev(tokens), torch.zeros(b, dtype=torch.int32, device="cuda"), dev(pos)
    logits = torch.empty(b, t.vocab_size, dtype=BF16, device="cuda")
    ws = torch.empty(lib.md_decode_workspace_bytes(C.byref(text), b), dtype=torch.uint8, device="cuda")
    sl = dev(slots)
    if prefix is None:
        st = lib.md_decode_step_slots(C.byref(text), tok.data_ptr(), nxt.data_ptr(), posd.data_ptr(), b, sl.data_ptr(), slab.n_slots,
                                      C.byref(slab.kv), -1, logits.data_ptr(), t.vocab_size, ws.data_ptr(), ws.numel(), stream())
    else:
        ps, pl = dev(prefix[0]), dev(prefix[1])
        st = lib.md_decode_step_shared(C.byref(text), tok.data_ptr(), nxt.data_ptr(), posd.data_ptr(), b, sl.data_ptr(), slab.n_slots,
                                       ps.data_ptr(), pl.data_ptr(), C.byref(slab.kv), -1, logits.data_ptr(), t.vocab_size,
                                       ws.data_ptr(), ws.numel(), stream())
    _lib.check(st, "decode step")
    torch.cuda.synchronize()
    return nxt, logits, posd


@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = load_golden(golden_dir, "tiny_seed1.npz")
    cfg, sd, model = build("tiny", int(g["seed"]), max_batch=8)
    return g, cfg, sd, model


@pytest.mark.parametrize("batch", [7, 130])
def test_library_prefill_and_decode_equal_copied_slots(tiny, batch):
    """Image prefixes of 3 prefix slots prefilled once; a 5-token prompt pass (q_len > 1) and two decode steps of `batch`
    rows (130: the 128-row block split) through the shared functions equal the slot-table functions on slabs into which
    the prefixes were copied: hidden states, logits, next ids, positions and every K / V row written."""
    g, cfg, sd, model = tiny
    model._select_kernels(2)
    d, P = cfg.text.dim, cfg.text.prefix_attn
    n_slots = 3 + batch
    shared, copy = Slab(cfg, n_slots), Slab(cfg, n_slots)
    forward(model, shared, rand_x(3, P, d, 1), [0] * 3, [0, 1, 2])
    pref = [(b * 5) % 3 for b in range(batch)]  # interleaved and in runs
    pref = sorted(pref[: batch // 2]) + pref[batch // 2 :]
    plen = [P] * batch
    own = [3 + b for b in range(batch)]
    copy.k.copy_(shared.k)
    copy.v.copy_(shared.v)
    for b in range(batch):
        copy.k[:, own[b], :, :P] = shared.k[:, pref[b], :, :P]
        copy.v[:, own[b], :, :P] = shared.v[:, pref[b], :, :P]
    k_prefix, v_prefix = shared.k[:, :3].clone(), shared.v[:, :3].clone()
    x = rand_x(batch, 5, d, 2)
    h_c = forward(model, copy, x, [P] * batch, own)
    h_s = forward(model, shared, x, [P] * batch, own, (pref, plen))
    assert torch.equal(h_s, h_c)
    pos = [P + 5] * batch
    toks = [int(t) for t in np.random.default_rng(0).integers(0, cfg.text.vocab_size, batch)]
    for step in range(2):
        n_c, l_c, p_c = decode_step(model, copy, toks, pos, own)
        n_s, l_s, p_s = decode_step(model, shared, toks, pos, own, (pref, plen))
        assert torch.equal(l_s, l_c) and torch.equal(n_s, n_c) and torch.equal(p_s, p_c), f"step {step}"
        toks, pos = n_c.tolist(), p_c.tolist()
    for a, b in ((shared.k, copy.k), (shared.v, copy.v)):
        assert torch.equal(a[:, 3:, :, P:], b[:, 3:, :, P:]), "K / V rows written differ"
        assert not a[:, 3:, :, :P].any(), "a row wrote into its shared prefix range"
    assert torch.equal(shared.k[:, :3], k_prefix) and torch.equal(shared.v[:, :3], v_prefix), "a prefix slot was written"


# ------------------------------------------------------------------ model: share_prefix=True against the copy path
def images3(cfg):
    return [synth.synthetic_image(i, 5) for i in range(3)]


def rows(encs, n, seed):
    rng = np.random.default_rng(seed)
    imgs = [encs[(i * 7) % 3] for i in range(n)]
    prompts = [[int(t) for t in rng.integers(1, 200, int(rng.integers(3, 7)))] for _ in range(n)]
    return imgs, prompts


@pytest.mark.parametrize("graphs", [False, True])
def test_generate_shared_equals_copy_path(tiny, graphs):
    g, cfg, sd, model = tiny
    model.use_graphs = graphs
    try:
        encs = [model.encode_image(im) for im in images3(cfg)]
        for n, seed in ((10, 1), (140, 2)):
            imgs, prompts = rows(encs, n, seed)
            ref = model.batch_generate_ids(imgs, prompts, max_tokens=12, ignore_eos=True)
            got = model.batch_generate_ids(imgs, prompts, max_tokens=12, ignore_eos=True, share_prefix=True)
            assert got == ref, n
            for temp in (0.5, 1.0):
                gr, gs = (torch.Generator(device="cuda").manual_seed(9) for _ in range(2))
                ref = model.batch_generate_ids(imgs, prompts, max_tokens=12, ignore_eos=True, temperature=temp, top_p=0.9, generator=gr)
                got = model.batch_generate_ids(imgs, prompts, max_tokens=12, ignore_eos=True, temperature=temp, top_p=0.9, generator=gs,
                                               share_prefix=True)
                assert got == ref, (n, temp)
    finally:
        model.use_graphs = False


def test_generate_shared_raw_images_equal_copy_path(tiny):
    """Raw images in the shared mode (one ViT batch, prefilled into the prefix slots) == the copy path over their
    EncodedImages, when those are encoded on the batched kernels (single_sequence_kernel off)."""
    g, cfg, sd, model = tiny
    model.single_sequence_kernel = False
    try:
        raw = images3(cfg)
        encs = [model.encode_image(im) for im in raw]
        imgs_raw, prompts = rows(raw, 9, 4)
        imgs_enc = [encs[raw.index(im)] for im in imgs_raw]
        ref = model.batch_generate_ids(imgs_enc, prompts, max_tokens=10, ignore_eos=True)
        assert model.batch_generate_ids(imgs_raw, prompts, max_tokens=10, ignore_eos=True, share_prefix=True) == ref
    finally:
        model.single_sequence_kernel = True


def test_prepared_record_of_the_shared_route_matches_batch_generate_ids(tiny):
    """``_prepare_sequences(share_prefix=True)`` over 2 EncodedImages x 2 prompt lengths: the record carries the shared routing,
    and its first tokens, put in the caller's order, are the first ids of the public call."""
    g, cfg, sd, model = tiny
    encs = [model.encode_image(im) for im in images3(cfg)[:2]]
    imgs = [encs[0], encs[1], encs[0], encs[1]]
    prompts = [[11, 12, 13, 14, 15], [21, 22, 23], [31, 32, 33], [41, 42, 43, 44, 45]]
    with torch.inference_mode():
        prep = model._prepare_sequences(imgs, prompts, share_prefix=True)
    assert prep.rows.kind == "_shared"
    assert sorted(prep.order) == [0, 1, 2, 3] and list(prep.order) != [0, 1, 2, 3]
    first = prep.in_caller_order(prep.first.tolist())
    ids = model.batch_generate_ids(imgs, prompts, share_prefix=True, max_tokens=1, ignore_eos=True)
    assert ids == [[t] for t in first]


def test_query_detect_point_many_equal_batch_calls(tiny, golden_dir):
    g, cfg, sd, model = tiny
    dg = load_golden(golden_dir, "tiny_detect.npz")
    img = Image.fromarray(synth.synthetic_image_array(int(dg["detect0.image_index"]), int(dg["seed"]), (378, 378)), "RGB")
    qs = ["11 12 13", "14", "15 16 17 18", "11 12 13", "19 20"]
    st = {"temperature": 0, "max_tokens": 8}
    enc = model.encode_image(img)
    assert model.query_many(img, qs, st) == [{"answer": a} for a in model.batch_query([enc] * len(qs), qs, st)]
    objects = ["7 8", "7 8 9 10", "5", "7 8"]
    st = {"max_objects": 2}
    assert model.detect_many(img, objects, st) == model.batch_detect([enc] * len(objects), objects, st)
    assert model.point_many(img, objects, st) == model.batch_point([enc] * len(objects), objects, st)


# ------------------------------------------------------------------ 2B
@pytest.fixture(scope="module")
def md2b(golden_dir):
    gv = load_golden(golden_dir, "md2b_vqa64.npz")
    cfg, sd, model = build("2b", int(gv["seed"]), max_batch=8)
    return gv, cfg, model


def test_2b_shared_vqa64_reproduces_reference(md2b):
    """64 distinct raw images (64 prefix slots) in the shared mode: the reference's ids, 64 / 64."""
    gv, cfg, model = md2b
    imgs = [synth.synthetic_image(i, int(gv["seed"])) for i in range(64)]
    got = model.batch_generate_ids(imgs, gv["prompt"].tolist(), max_tokens=32, ignore_eos=True, share_prefix=True)
    ref = gv["tokens"].tolist()
    bad = [i for i in range(64) if got[i] != ref[i]]
    assert not bad, bad[:8]


def test_2b_query_many_equals_copy_path(md2b, golden_dir):
    gv, cfg, model = md2b
    gb = load_golden(golden_dir, "md2b_bench64.npz")
    img = synth.synthetic_image(0, int(gb["seed"]))
    prompts = [synth.synthetic_vqa_prompt(cfg, i, int(gv["seed"])) for i in range(64)]
    enc = model.encode_image(img)
    ref = model.batch_generate_ids([enc] * 64, prompts, max_tokens=32, ignore_eos=True)
    got = model.batch_generate_ids([enc] * 64, prompts, max_tokens=32, ignore_eos=True, share_prefix=True)
    assert got == ref
    qs = [" ".join(str(t) for t in p) for p in prompts[:16]]
    st = {"temperature": 0, "max_tokens": 16}
    assert model.query_many(img, qs, st) == [{"answer": a} for a in model.batch_query([enc] * 16, qs, st)]


def test_2b_detect_many_equals_batch_detect(md2b, golden_dir):
    gv, cfg, model = md2b
    g = load_golden(golden_dir, "md2b_detect13.npz")
    size = tuple(int(x) for x in g["size"])
    img = synth.synthetic_image(0, int(g["seed"]), size)
    obj = " ".join(str(t) for t in g["object_ids"].tolist())
    objects = [obj, obj + " " + obj, obj]
    st = {"max_objects": int(g["max_objects"])}
    enc = model.encode_image(img)
    assert model.detect_many(img, objects, st) == model.batch_detect([enc] * len(objects), objects, st)
