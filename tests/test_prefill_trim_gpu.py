"""md_text_forward_trim on the MI355X: a prefill whose caller keeps the last row of every sequence (or no hidden row) gives,
bit for bit, the last rows and the K / V rows of the all-rows entry points -- where the last block is trimmed (more than 64
rows on the pinned tile) and where the call falls back to the full computation."""
import ctypes as C

import pytest
import torch

from moondream_amd import _lib, synth
from moondream_amd.config import get_config

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
POISON = 0x7FC1  # a bf16 NaN pattern no kernel writes


@pytest.fixture(scope="module")
def tiny():
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config("tiny")  # dim 256, 4 heads of 64, ff 704, 3 layers: the RoPE-epilogue shape conditions hold
    sd = synth.synthetic_state_dict(cfg, seed=1, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=4)
    model._select_kernels(2)  # MD_TILE_PINNED, as every batched call
    return cfg, model


class Slab:
    def __init__(self, cfg, n_slots):
        t = cfg.text
        self.k = torch.zeros(t.n_layers, n_slots, t.n_kv_heads, t.max_context, t.head_dim, dtype=BF16, device="cuda")
        self.v = torch.zeros_like(self.k)
        bs = t.n_kv_heads * t.max_context * t.head_dim
        self.kv = _lib.MdKvCache(self.k.data_ptr(), self.v.data_ptr(), n_slots * bs, bs, t.max_context)
        self.n_slots = n_slots

    def copy(self, cfg):
        other = Slab(cfg, self.n_slots)
        other.k.copy_(self.k)
        other.v.copy_(self.v)
        return other


def dev(a):
    return torch.tensor(list(a), dtype=torch.int32, device="cuda")


def stream():
    return torch.cuda.current_stream().cuda_stream


def rand_x(b, t, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, t, d, generator=g) * 0.5).to(BF16).cuda()


def text_struct(model, prefix_len=None, tile_policy=None):
    st = type(model.w.text).from_buffer_copy(model.w.text)
    if prefix_len is not None:
        st.prefix_len = prefix_len
    if tile_policy is not None:
        st.tile_policy = tile_policy
    return st


def all_rows(model, text, slab, x, pos, slots=None, prefix=None):
    """hidden [b, t, d] of md_text_forward / _slots / _shared: the form the tables select."""
    lib = model.lib
    b, t, _ = x.shape
    hidden = torch.empty_like(x)
    pos0 = dev(pos)
    ws = torch.empty(lib.md_text_workspace_bytes(C.byref(text), b, t), dtype=torch.uint8, device="cuda")
    head = (C.byref(text), x.data_ptr(), hidden.data_ptr(), b, t, pos0.data_ptr())
    tail = (C.byref(slab.kv), ws.data_ptr(), ws.numel(), stream())
    if slots is None:
        st = lib.md_text_forward(*head, *tail)
    elif prefix is None:
        sl = dev(slots)
        st = lib.md_text_forward_slots(*head, sl.data_ptr(), slab.n_slots, *tail)
    else:
        sl, ps, pl = dev(slots), dev(prefix[0]), dev(prefix[1])
        st = lib.md_text_forward_shared(*head, sl.data_ptr(), slab.n_slots, ps.data_ptr(), pl.data_ptr(), *tail)
    _lib.check(st, "all-rows forward")
    torch.cuda.synchronize()
    return hidden


def trimmed(model, text, slab, x, pos, mode, slots=None, prefix=None):
    """md_text_forward_trim over the same tables; returns (hidden_last [b, d], poisoned before the call; the working rows)."""
    lib = model.lib
    b, t, d = x.shape
    hidden = torch.empty_like(x)
    last = torch.full((b, d), POISON, dtype=torch.int16, device="cuda").view(BF16)
    pos0 = dev(pos)
    ws = torch.empty(lib.md_text_workspace_bytes(C.byref(text), b, t), dtype=torch.uint8, device="cuda")
    sl = dev(slots) if slots is not None else None
    ps, pl = (dev(prefix[0]), dev(prefix[1])) if prefix is not None else (None, None)
    ptr = lambda tab: tab.data_ptr() if tab is not None else None
    st = lib.md_text_forward_trim(C.byref(text), x.data_ptr(), hidden.data_ptr(), last.data_ptr(), mode, b, t, pos0.data_ptr(), ptr(sl),
                                  slab.n_slots if slots is not None else 0, ptr(ps), ptr(pl), C.byref(slab.kv), ws.data_ptr(),
                                  ws.numel(), stream())
    _lib.check(st, "md_text_forward_trim")
    torch.cuda.synchronize()
    return last, hidden


def bits(t):
    return t.contiguous().view(torch.int16)


def check_case(cfg, model, text, slab0, x, pos, slots=None, prefix=None, trims=True):
    """The all-rows form and both trimmed modes from the same starting slab: last rows and every layer's K / V rows."""
    ref_slab = slab0.copy(cfg)
    ref = all_rows(model, text, ref_slab, x, pos, slots, prefix)
    assert torch.isfinite(ref.float()).all()
    last_slab = slab0.copy(cfg)
    last, work = trimmed(model, text, last_slab, x, pos, _lib.MD_HIDDEN_LAST, slots, prefix)
    if trims:  # the working rows are unspecified; that the other rows did NOT get the last block shows the trimmed path ran
        assert not torch.equal(bits(work[:, :-1]), bits(ref[:, :-1])), "the call was expected to trim the last block"
    assert torch.equal(bits(last), bits(ref[:, -1, :])), "hidden_last differs from the all-rows output's last rows"
    none_slab = slab0.copy(cfg)
    none, _ = trimmed(model, text, none_slab, x, pos, _lib.MD_HIDDEN_NONE, slots, prefix)
    assert bool((bits(none) == torch.tensor(POISON, dtype=torch.int16)).all()), "mode none wrote a hidden row"
    for name, s in (("last", last_slab), ("none", none_slab)):
        for l in range(cfg.text.n_layers):
            assert torch.equal(bits(s.k[l]), bits(ref_slab.k[l])), f"mode {name}: K rows of layer {l} differ"
            assert torch.equal(bits(s.v[l]), bits(ref_slab.v[l])), f"mode {name}: V rows of layer {l} differ"
    assert bool(ref_slab.k[-1].any()) and bool(ref_slab.v[-1].any())  # the last layer's rows were written at all


def test_two_query_blocks_and_the_prefix_lm_rule(tiny):
    """batch 3, q_len 131: two query blocks, the last one holding 3 rows; bidirectional prefix of 100 positions."""
    cfg, model = tiny
    check_case(cfg, model, text_struct(model, prefix_len=100), Slab(cfg, 3), rand_x(3, 131, cfg.text.dim, 1), [0, 0, 0])


def test_prompt_pass_over_an_existing_prefix_ragged_positions(tiny):
    """batch 2, q_len 40 (80 rows > 64, one query block) behind 110 prefilled positions, pos0 100 and 107."""
    cfg, model = tiny
    text = text_struct(model, prefix_len=100)
    slab = Slab(cfg, 2)
    all_rows(model, text, slab, rand_x(2, 110, cfg.text.dim, 2), [0, 0])
    check_case(cfg, model, text, slab, rand_x(2, 40, cfg.text.dim, 3), [100, 107])


def test_slot_table_permuted(tiny):
    """batch 2, q_len 129 into slots 3 and 1 of four."""
    cfg, model = tiny
    check_case(cfg, model, text_struct(model), Slab(cfg, 4), rand_x(2, 129, cfg.text.dim, 4), [0, 0], slots=[3, 1])


def test_shared_prefix_table(tiny):
    """batch 2, q_len 129 at position 100, both rows reading keys [0, 100) from slot 0."""
    cfg, model = tiny
    text = text_struct(model, prefix_len=100)
    slab = Slab(cfg, 4)
    all_rows(model, text, slab, rand_x(1, 100, cfg.text.dim, 5), [0], slots=[0])
    check_case(cfg, model, text, slab, rand_x(2, 129, cfg.text.dim, 6), [100, 100], slots=[2, 3], prefix=([0, 0], [100, 100]))


def test_calls_that_fall_back_to_the_full_computation(tiny):
    """At most 64 rows (the decode-regime kernels), a by-shape call and a decode step: no trim, the same results."""
    cfg, model = tiny
    d = cfg.text.dim
    check_case(cfg, model, text_struct(model), Slab(cfg, 1), rand_x(1, 20, d, 7), [0], trims=False)
    check_case(cfg, model, text_struct(model, prefix_len=100, tile_policy=_lib.MD_TILE_BY_SHAPE), Slab(cfg, 3), rand_x(3, 131, d, 8), [0] * 3,
               trims=False)
    slab = Slab(cfg, 3)
    all_rows(model, text_struct(model), slab, rand_x(3, 30, d, 9), [0] * 3)
    check_case(cfg, model, text_struct(model), slab, rand_x(3, 1, d, 10), [30] * 3, trims=False)


def test_batch_generate_ids_equals_the_untrimmed_model(tiny):
    """3 raw images through the fused [bos | image | prompt] pass: ids and first-step logits with and without the trim."""
    cfg, model = tiny
    images = [synth.synthetic_image(i, 5) for i in range(3)]
    prompts = [[11, 12, 13], [14, 15, 16], [17, 18, 19, 20]]
    out = {}
    try:
        for trim in (False, True):
            model.prefill_trim = trim
            ids = model.batch_generate_ids(images, prompts, max_tokens=8, ignore_eos=True)
            cap = torch.empty(3, cfg.text.vocab_size, dtype=BF16, device="cuda")
            with torch.inference_mode():
                model._select_kernels(3)
                prep = model._prepare_sequences(list(images), prompts, fuse=True, logits_capture=cap)
            torch.cuda.synchronize()
            out[trim] = (ids, list(prep.order), prep.first.tolist(), bits(cap).cpu(), bits(prep.hidden_last).cpu())
    finally:
        model.prefill_trim = True
    assert out[True][:3] == out[False][:3]
    assert torch.equal(out[True][3], out[False][3]), "first-step logits differ"
    assert torch.equal(out[True][4], out[False][4]), "hidden_last differs"
