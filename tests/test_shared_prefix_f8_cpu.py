"""Shared image prefix over the e4m3 copy of the KV cache: what the new entry point and the shared decoder calls refuse on the
host, before anything touches a device."""
import ctypes

from moondream_amd import _lib

ERR_ARG = 1  # MD_ERR_INVALID_ARG
D = ctypes.c_void_p(0x10)  # never dereferenced: every call below fails its host checks first


def attend(ldq=3 * 2 * 64, ctx=16, k8=D, v8=D, k_scale=0.5, v_scale=0.5, slots=D, n_slots=4, prefix_slots=D, prefix_len=D, n_heads=2):
    lib = _lib.load()
    return lib.md_attention_decode_rope_f8_shared(D, ldq, D, n_heads * 64, D, D, D, k8, v8, n_heads * 16 * 64, ctx, D, 2, n_heads, 32,
                                                  0.125, k_scale, v_scale, slots, n_slots, prefix_slots, prefix_len, None)


def test_symbol_is_bound():
    assert "md_attention_decode_rope_f8_shared" in _lib.exported_symbols()
    assert hasattr(_lib.load(), "md_attention_decode_rope_f8_shared")


def test_grouped_e4m3_entry_point_validates_on_the_host():
    assert attend(slots=None) == ERR_ARG                      # a prefix table without the slot table
    assert attend(prefix_len=None) == ERR_ARG                 # ... without the prefix lengths
    assert attend(n_slots=0) == ERR_ARG
    assert attend(n_slots=0, prefix_slots=None, prefix_len=None) == ERR_ARG
    assert attend(k8=None) == ERR_ARG                         # no e4m3 copy: the bf16 kernels have their own entry points
    assert attend(v8=None) == ERR_ARG
    for kw in ({}, {"prefix_slots": None, "prefix_len": None}):  # the grouped launch and the slot-table launch
        assert attend(k_scale=0.0, **kw) == ERR_ARG
        assert attend(k_scale=-1.0, **kw) == ERR_ARG
        assert attend(v_scale=0.0, **kw) == ERR_ARG
        assert attend(ctx=4096, **kw) == ERR_ARG              # the scores of a context live in LDS: at most 2048 positions
        assert attend(ldq=3 * 2 * 64 - 8, **kw) == ERR_ARG    # ldq < 3 * n_heads * 64


def kv_struct(k8=False, scales=None):
    kv = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    if k8:
        kv.k8, kv.v8 = 0x3000, 0x4000
    if scales == "k":
        kv.k_scale = 0x5000
    if scales == "v":
        kv.v_scale = 0x5000
    return kv


def test_shared_decoder_calls_still_refuse_a_copy_without_scales():
    lib = _lib.load()
    m = _lib.MdTextModel()
    for kv in (kv_struct(k8=True), kv_struct(k8=True, scales="k"), kv_struct(k8=True, scales="v")):  # no scales; one of the two
        kvp = ctypes.byref(kv)
        assert lib.md_text_forward_shared(ctypes.byref(m), D, D, 2, 1, D, D, 4, D, D, kvp, D, 1 << 20, None) == ERR_ARG
        assert lib.md_text_forward_shared(ctypes.byref(m), D, D, 2, 5, D, D, 4, D, D, kvp, D, 1 << 20, None) == ERR_ARG
        assert lib.md_decode_step_shared(ctypes.byref(m), D, D, D, 2, D, 4, D, D, kvp, 0, D, 64, D, 1 << 20, None) == ERR_ARG
        assert lib.md_text_forward_trim(ctypes.byref(m), D, D, D, 0, 2, 5, D, D, 4, D, D, kvp, D, 1 << 20, None) == ERR_ARG
