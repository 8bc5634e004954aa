"""Shared image prefix in the fp8 KV mode on the MI355X: the grouped decode kernel over the e4m3 copy of the cache,
md_text_forward_shared / md_decode_step_shared with a complete copy and the model's shared mode under ``enable_fp8(kv_cache=True)``
give, bit for bit, what the one-row kernel / the slot-table functions / the copy path give over slots into which the prefix
was copied -- outputs and every byte written to the bf16 and the e4m3 slabs."""
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
H = 8              # heads of every kernel case (MHA)
SCALE8 = 2.0**-7   # value ~= SCALE8 * e4m3: randn * 0.5 stays inside +-448
NAN8 = 0x7F        # the e4m3fn NaN byte


def dev(a):
    return torch.tensor(list(a), dtype=torch.int32, device="cuda")


def stream():
    return torch.cuda.current_stream().cuda_stream


_FREQS = None


def synth_freqs():
    global _FREQS
    if _FREQS is None:
        pos = torch.arange(CTX, dtype=torch.float32)[:, None]
        inv = 1.0 / (10000 ** (torch.arange(16, dtype=torch.float32) / 16))
        ang = pos * inv
        _FREQS = torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous().cuda()
    return _FREQS


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t


# ------------------------------------------------------------------ kernel: md_attention_decode_rope_f8_shared
def quantize(lib, k, v):
    """The e4m3 slabs of bf16 slabs [n_slots][H][CTX][64], by the library's own md_kv_quantize_f8."""
    n_slots = k.shape[0]
    k8, v8 = (torch.zeros(k.shape, dtype=torch.uint8, device="cuda") for _ in range(2))
    bs = H * CTX * 64
    ks, vs = (C.c_float * 1)(SCALE8), (C.c_float * 1)(SCALE8)
    kv = _lib.MdKvCache(k.data_ptr(), v.data_ptr(), n_slots * bs, bs, CTX)
    kv.k8, kv.v8 = k8.data_ptr(), v8.data_ptr()
    kv.k_scale, kv.v_scale = C.cast(ks, C.c_void_p), C.cast(vs, C.c_void_p)
    _lib.check(lib.md_kv_quantize_f8(C.byref(kv), 1, n_slots, H, None, 0, CTX, stream()), "md_kv_quantize_f8")
    torch.cuda.synchronize()
    return k8, v8


def make_case(lib, batch, layout, seed, idle_every=0, per_row_plen=None, plens_by_prefix=(730, 128, 2000), one_slot=False, kv_len=None):
    """3 prefix slots (0..2) and one own slot per row (3 + b); four slabs each for SHARED (own slots hold NaN below the row's
    prefix end, in both copies: a read there poisons the output) and COPY (the prefix copied into the own slot).  Both hold NaN
    at positions >= kv_len[b] of the own slots: neither kernel may read there."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    n_slots = 3 + batch
    shape = (n_slots, H, CTX, 64)
    k = (torch.randn(shape, generator=g, device="cuda") * 0.5).to(BF16)
    v = (torch.randn(shape, generator=g, device="cuda") * 0.5).to(BF16)
    k8, v8 = quantize(lib, k, v)
    pref, plen, kvl, slots = [], [], [], []
    for b in range(batch):
        p = 0 if one_slot else (b % 3) if layout == "interleaved" else (3 * b) // batch
        pl = per_row_plen[b % len(per_row_plen)] if per_row_plen else plens_by_prefix[p]
        pref.append(p if pl > 0 else -1)
        plen.append(pl)
        kvl.append(kv_len[b % len(kv_len)] if kv_len else min(CTX, pl + 1 + int(rng.integers(0, 40))))
        slots.append(-1 if idle_every and b % idle_every == idle_every - 1 else 3 + b)
    shared = [t.clone() for t in (k, v, k8, v8)]
    copy = [t.clone() for t in (k, v, k8, v8)]
    nan = torch.tensor(float("nan"), dtype=BF16, device="cuda")
    for b in range(batch):
        s, p, pl, kl = slots[b], pref[b], plen[b], kvl[b]
        if s < 0:
            continue
        for slabs in (shared, copy):
            slabs[0][s, :, kl:] = nan
            slabs[1][s, :, kl:] = nan
            slabs[2][s, :, kl:] = NAN8
            slabs[3][s, :, kl:] = NAN8
        if pl == 0:
            continue
        shared[0][s, :, :pl] = nan
        shared[1][s, :, :pl] = nan
        shared[2][s, :, :pl] = NAN8
        shared[3][s, :, :pl] = NAN8
        for i, base in enumerate((k, v, k8, v8)):
            copy[i][s, :, :pl] = base[p, :, :pl]
    return dict(slots=slots, pref=pref, plen=plen, kvl=kvl, n_slots=n_slots, shared=shared, copy=copy)


def attend(lib, q, slabs, c, prefix, entry="shared"):
    k, v, k8, v8 = slabs
    batch = q.shape[0]
    o = torch.full((batch, H * 64), 7.0, dtype=BF16, device="cuda")
    bs = H * CTX * 64
    kl = dev(c["kvl"])
    freqs = synth_freqs()
    if entry == "one_row":  # the entry point this change does not touch: row b in slot b
        st = lib.md_attention_decode_rope_f8(q.data_ptr(), q.shape[1], o.data_ptr(), o.shape[1], freqs.data_ptr(), k.data_ptr(),
                                             v.data_ptr(), k8.data_ptr(), v8.data_ptr(), bs, CTX, kl.data_ptr(), batch, H, 32, 0.125,
                                             SCALE8, SCALE8, stream())
    else:
        sl = dev(c["slots"])
        ps, pl = (dev(c["pref"]), dev(c["plen"])) if prefix else (None, None)
        st = lib.md_attention_decode_rope_f8_shared(q.data_ptr(), q.shape[1], o.data_ptr(), o.shape[1], freqs.data_ptr(), k.data_ptr(),
                                                    v.data_ptr(), k8.data_ptr(), v8.data_ptr(), bs, CTX, kl.data_ptr(), batch, H, 32,
                                                    0.125, SCALE8, SCALE8, sl.data_ptr(), c["n_slots"],
                                                    ps.data_ptr() if prefix else None, pl.data_ptr() if prefix else None, stream())
    _lib.check(st, "decode attention")
    torch.cuda.synchronize()
    return o


def check_kernel(batch, layout, seed=0, **kw):
    lib = _lib.load()
    c = make_case(lib, batch, layout, seed, **kw)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    q = torch.randn(batch, 3 * H * 64, generator=g, device="cuda").to(BF16)
    before = [t.clone() for t in c["shared"]]
    ref = attend(lib, q, c["copy"], c, prefix=False)   # the one-row kernel (slot-table launch) over copied prefixes
    got = attend(lib, q, c["shared"], c, prefix=True)  # the grouped kernel
    live = [b for b in range(batch) if c["slots"][b] >= 0]
    idle = [b for b in range(batch) if c["slots"][b] < 0]
    assert torch.isfinite(got[live].float()).all(), "a NaN byte below a row's prefix end or past its kv_len was read"
    assert torch.isfinite(ref[live].float()).all()
    bad = [b for b in live if not torch.equal(bits(got[b]), bits(ref[b]))]
    assert not bad, f"rows {bad[:8]} differ (plen {[c['plen'][b] for b in bad[:8]]}, kv_len {[c['kvl'][b] for b in bad[:8]]})"
    if idle:
        assert not got[idle].float().any() and not ref[idle].float().any()
    # the prefix slots and every slot no live row owns are untouched; own slots: the rows at and past the prefix end equal the
    # one-row kernel's, the new row at kv_len - 1 included -- in the bf16 and in the e4m3 slabs
    untouched = [0, 1, 2] + [3 + b for b in idle]
    names = ("K", "V", "e4m3 K", "e4m3 V")
    for a, a0, name in zip(c["shared"], before, names):
        assert torch.equal(bits(a[untouched]), bits(a0[untouched])), f"{name}: a prefix or idle slot was written"
    for b in live:
        s, pl = c["slots"][b], c["plen"][b]
        for a, a0, ac, name in zip(c["shared"], before, c["copy"], names):
            assert torch.equal(bits(a[s, :, pl:]), bits(ac[s, :, pl:])), f"{name} rows of row {b} differ from the one-row kernel's"
            assert torch.equal(bits(a[s, :, :pl]), bits(a0[s, :, :pl])), f"{name}: row {b} wrote into its shared prefix range"


def test_slot_table_launch_equals_the_existing_entry_point():
    """Identity slot table, no prefix table: the new entry point is md_attention_decode_rope_f8 bit for bit, outputs and all
    four slabs -- which ties the reference of every test below to code this feature does not touch."""
    lib = _lib.load()
    batch = 7
    g = torch.Generator(device="cuda").manual_seed(5)
    k = (torch.randn((batch, H, CTX, 64), generator=g, device="cuda") * 0.5).to(BF16)
    v = (torch.randn((batch, H, CTX, 64), generator=g, device="cuda") * 0.5).to(BF16)
    k8, v8 = quantize(lib, k, v)
    q = torch.randn(batch, 3 * H * 64, generator=g, device="cuda").to(BF16)
    c = dict(slots=list(range(batch)), kvl=[1, 2, 64, 65, 731, 2047, 2048], n_slots=batch)
    a = [t.clone() for t in (k, v, k8, v8)]
    b = [t.clone() for t in (k, v, k8, v8)]
    o_a = attend(lib, q, a, c, prefix=False, entry="one_row")
    o_b = attend(lib, q, b, c, prefix=False)
    assert torch.isfinite(o_a.float()).all() and torch.equal(bits(o_a), bits(o_b))
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))
    assert not torch.equal(a[2], k8), "the new row was not written to the e4m3 copy"


@pytest.mark.parametrize("batch", [1, 7, 64, 70])
@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_grouped_kernel_equals_one_row_kernel_over_copied_slots(batch, layout):
    """One prefix length per prefix slot: whole groups share a prefix (the one-load-per-group path) where rows are contiguous;
    interleaved rows mix slots inside a group (the per-row path); 70 rows: a last group with absent rows."""
    check_kernel(batch, layout, idle_every=5 if batch >= 7 else 0)


def test_grouped_kernel_prefix_lengths_and_ragged_groups():
    """prefix_len from {0, 1, 63, 64, 65, 127, 128, 730, 2000} inside one group (0: no shared prefix), ragged kv_len: on three
    prefix slots in both layouts, and on ONE prefix slot, where the shared rounds stop at the group's smallest prefix end."""
    plens = [730, 0, 1, 63, 2000, 64, 65, 127, 128, 730, 63, 2000, 64, 128, 65, 1]
    for layout in ("contiguous", "interleaved"):
        check_kernel(32, layout, per_row_plen=plens, seed=3)
    check_kernel(32, "contiguous", per_row_plen=[p for p in plens if p > 0], seed=4, one_slot=True)
    for pl in (1, 63, 64, 65, 127, 128, 730, 2000):
        check_kernel(8, "contiguous", plens_by_prefix=(pl, pl, pl), seed=pl)


def test_grouped_kernel_one_prefix_slot_different_prefix_lengths():
    """Every row of a group on one prefix slot, prefix lengths all >= 64 but different: each row reads its remaining prefix
    keys from the prefix slot on its own."""
    check_kernel(16, "contiguous", per_row_plen=[730, 2000, 300, 1000], seed=21, one_slot=True)
    check_kernel(12, "contiguous", per_row_plen=[1000, 129, 640, 1999, 256, 383], seed=22, one_slot=True)


def test_grouped_kernel_short_rows_skip_the_long_rows_rounds():
    """A group whose rows' kv_len differ by many 64-key rounds: a short row adds nothing in the rounds only a longer row needs
    and never reads at or beyond its own kv_len (NaN bytes there)."""
    check_kernel(8, "contiguous", per_row_plen=[1900, 5], seed=12)
    check_kernel(8, "contiguous", per_row_plen=[130, 1500], seed=11)
    check_kernel(8, "contiguous", per_row_plen=[1900, 5], seed=13, one_slot=True)
    check_kernel(8, "contiguous", per_row_plen=[130, 1500], seed=14, one_slot=True)


def test_grouped_kernel_full_context_row():
    """kv_len == 2048: the last round is the last of the score buffer."""
    check_kernel(4, "contiguous", per_row_plen=[2000, 730, 2047, 730], kv_len=[2048, 735, 2048, 2048], seed=31, one_slot=True)
    check_kernel(5, "interleaved", per_row_plen=[2000], kv_len=[2048, 2001, 2030, 2048, 2047], seed=32)


# ------------------------------------------------------------------ library: md_text_forward_shared / md_decode_step_shared
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


@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = load_golden(golden_dir, "tiny_seed1.npz")
    cfg, sd, model = build("tiny", int(g["seed"]), max_batch=8)
    return g, cfg, sd, model


class Slab8:
    """bf16 slabs plus a COMPLETE e4m3 copy (both slabs, both scale arrays)."""

    def __init__(self, cfg, n_slots):
        t = cfg.text
        self.k = torch.zeros(t.n_layers, n_slots, t.n_kv_heads, t.max_context, t.head_dim, dtype=BF16, device="cuda")
        self.v = torch.zeros_like(self.k)
        self.k8 = torch.zeros(self.k.shape, dtype=torch.uint8, device="cuda")
        self.v8 = torch.zeros_like(self.k8)
        self.scales = ((C.c_float * t.n_layers)(*[2.0**-4] * t.n_layers), (C.c_float * t.n_layers)(*[2.0**-5] * t.n_layers))
        bs = t.n_kv_heads * t.max_context * t.head_dim
        self.kv = _lib.MdKvCache(self.k.data_ptr(), self.v.data_ptr(), n_slots * bs, bs, t.max_context)
        self.kv.k8, self.kv.v8 = self.k8.data_ptr(), self.v8.data_ptr()
        self.kv.k_scale, self.kv.v_scale = C.cast(self.scales[0], C.c_void_p), C.cast(self.scales[1], C.c_void_p)
        self.n_slots = n_slots

    def all(self):
        return (self.k, self.v, self.k8, self.v8)


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


@pytest.mark.parametrize("batch", [7, 70])
def test_library_prefill_and_decode_equal_copied_slots(tiny, batch):
    """Image prefixes of 3 prefix slots prefilled once (which quantises them); a 5-position prompt pass and three decode steps
    of `batch` rows (70: across the 64-row block of the e4m3 mode) through the shared functions equal the slot-table functions
    on slabs into which the prefixes were copied: hidden rows, logits, next ids and every row written to the four slabs."""
    g, cfg, sd, model = tiny
    model._select_kernels(2)
    d, P = cfg.text.dim, cfg.text.prefix_attn
    n_slots = 3 + batch
    shared, copy = Slab8(cfg, n_slots), Slab8(cfg, n_slots)
    forward(model, shared, rand_x(3, P, d, 1), [0] * 3, [0, 1, 2])
    assert int((shared.k8[:, :3, :, :P] != 0).sum()) > 0, "the image prefill did not quantise the prefix slots"
    pref = [(b * 5) % 3 for b in range(batch)]  # in runs, then interleaved
    pref = sorted(pref[: batch // 2]) + pref[batch // 2 :]
    plen = [P] * batch
    own = [3 + b for b in range(batch)]
    for a, b_ in zip(copy.all(), shared.all()):
        a.copy_(b_)
        for b in range(batch):
            a[:, own[b], :, :P] = b_[:, pref[b], :, :P]
    prefix_before = [a[:, :3].clone() for a in shared.all()]
    x = rand_x(batch, 5, d, 2)
    h_c = forward(model, copy, x, [P] * batch, own)
    h_s = forward(model, shared, x, [P] * batch, own, (pref, plen))
    assert torch.equal(bits(h_s), bits(h_c))
    pos = [P + 5] * batch
    toks = [int(t) for t in np.random.default_rng(0).integers(0, cfg.text.vocab_size, batch)]
    for step in range(3):
        n_c, l_c, p_c = decode_step(model, copy, toks, pos, own)
        n_s, l_s, p_s = decode_step(model, shared, toks, pos, own, (pref, plen))
        assert torch.equal(bits(l_s), bits(l_c)) and torch.equal(n_s, n_c) and torch.equal(p_s, p_c), f"step {step}"
        toks, pos = n_c.tolist(), p_c.tolist()
    names = ("K", "V", "e4m3 K", "e4m3 V")
    for a, b_, before, name in zip(shared.all(), copy.all(), prefix_before, names):
        assert torch.equal(bits(a[:, 3:, :, P:]), bits(b_[:, 3:, :, P:])), f"{name} rows written differ"
        assert int((a[:, 3:, :, P : P + 8] != 0).sum()) > 0, f"{name}: no row was written"
        assert not bits(a[:, 3:, :, :P]).any(), f"{name}: a row wrote into its shared prefix range"
        assert torch.equal(bits(a[:, :3]), bits(before)), f"{name}: a prefix slot was written"


# ------------------------------------------------------------------ model: share_prefix=True under enable_fp8(kv_cache=True)
def images3():
    return [synth.synthetic_image(i, 5) for i in range(3)]


def rows(encs, n, seed):
    rng = np.random.default_rng(seed)
    imgs = [encs[(i * 7) % 3] for i in range(n)]
    prompts = [[int(t) for t in rng.integers(1, 200, int(rng.integers(3, 7)))] for _ in range(n)]
    return imgs, prompts


class SharedRoute:
    """Counts the calls of ``_shared_routing`` (one per preparation on the shared route, none on the copy path): without it
    every test below passes on the copy-path fallback."""

    def __init__(self, model):
        self.model, self.calls = model, 0
        self.inner = model._shared_routing

    def __enter__(self):
        def counted(*a, **kw):
            self.calls += 1
            return self.inner(*a, **kw)

        self.model._shared_routing = counted
        return self

    def __exit__(self, *exc):
        del self.model._shared_routing


@pytest.fixture()
def tiny_fp8(tiny):
    g, cfg, sd, model = tiny
    cal = images3()
    model.enable_fp8(cal, g["img0.cap.prompt"].tolist(), kv_cache=True)
    try:
        assert model._kv8_scales is not None
        yield g, cfg, sd, model
    finally:
        model.use_graphs = False
        model.fused_prefill = True
        model.single_sequence_kernel = True
        model.enable_fp8(on=False)


@pytest.mark.parametrize("graphs", [False, True])
def test_generate_shared_equals_copy_path(tiny_fp8, graphs):
    """Repeated EncodedImages, greedy and sampled with a seed, with ``compile()``'s captured steps and without; 70 rows cross
    the 64-row block."""
    g, cfg, sd, model = tiny_fp8
    model.use_graphs = graphs
    encs = [model.encode_image(im) for im in images3()]
    assert model._shares_prefix(None)
    for n, seed in ((10, 1), (70, 2)):
        imgs, prompts = rows(encs, n, seed)
        ref = model.batch_generate_ids(imgs, prompts, max_tokens=10, ignore_eos=True, share_prefix=False)
        with SharedRoute(model) as route:
            got = model.batch_generate_ids(imgs, prompts, max_tokens=10, ignore_eos=True, share_prefix=True)
        assert route.calls == 1, "share_prefix=True took the copy path"
        assert got == ref, n
        gr, gs = (torch.Generator(device="cuda").manual_seed(9) for _ in range(2))
        ref = model.batch_generate_ids(imgs, prompts, max_tokens=10, ignore_eos=True, temperature=0.5, top_p=0.9, generator=gr)
        with SharedRoute(model) as route:
            got = model.batch_generate_ids(imgs, prompts, max_tokens=10, ignore_eos=True, temperature=0.5, top_p=0.9, generator=gs,
                                           share_prefix=True)
        assert route.calls == 1 and got == ref, n


def test_generate_shared_raw_images_equal_copy_path(tiny_fp8):
    """Repeated raw images: one ViT batch and one prefill per distinct image against share_prefix=False, which encodes and
    prefills every row's image.  Both on the batched kernels in two passes (``fused_prefill`` off: the one-pass [image | prompt]
    prefill of share_prefix=False is another association of the same sums)."""
    g, cfg, sd, model = tiny_fp8
    model.single_sequence_kernel = False
    model.fused_prefill = False
    raw = images3()
    imgs, prompts = rows(raw, 9, 4)
    ref = model.batch_generate_ids(imgs, prompts, max_tokens=10, ignore_eos=True, share_prefix=False)
    assert model._shares_prefix(None)
    with SharedRoute(model) as route:
        got = model.batch_generate_ids(imgs, prompts, max_tokens=10, ignore_eos=True, share_prefix=True)
    assert route.calls == 1, "share_prefix=True took the copy path"
    assert got == ref


def test_query_detect_point_many_equal_batch_calls(tiny_fp8, golden_dir):
    g, cfg, sd, model = tiny_fp8
    dg = load_golden(golden_dir, "tiny_detect.npz")
    img = Image.fromarray(synth.synthetic_image_array(int(dg["detect0.image_index"]), int(dg["seed"]), (378, 378)), "RGB")
    qs = ["11 12 13", "14", "15 16 17 18", "11 12 13", "19 20"]
    st = {"temperature": 0, "max_tokens": 8}
    enc = model.encode_image(img)
    assert model._shares_prefix(None)
    with SharedRoute(model) as route:
        got = model.query_many(img, qs, st)
    assert route.calls == 1 and got == [{"answer": a} for a in model.batch_query([enc] * len(qs), qs, st)]
    objects = ["7 8", "7 8 9 10", "5", "7 8"]
    st = {"max_objects": 2}
    with SharedRoute(model) as route:
        got_d = model.detect_many(img, objects, st)
        got_p = model.point_many(img, objects, st)
    assert route.calls == 2
    assert got_d == model.batch_detect([enc] * len(objects), objects, st)
    assert got_p == model.batch_point([enc] * len(objects), objects, st)
