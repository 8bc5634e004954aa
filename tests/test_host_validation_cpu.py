"""The host-side argument checks of the row-routed entry points, without a GPU: the loaded library, called with null
streams and pointers that are never dereferenced, refuses before any launch.  The codes below are the ones the library
returned before the C host layer was routed through one row map (csrc/text_internal.hpp); the test passed unchanged
against that library."""
import ctypes

from moondream_amd import _lib

ERR_ARG, ERR_UNSUPPORTED = 1, 4
D = ctypes.c_void_p(0x10)  # never dereferenced: every call below fails its host checks first


def decode_shared(lib, *, ldq=64, head_dim=64, slots=D, n_slots=4, pfx_slots=D, pfx_len=D):
    return lib.md_attention_decode_shared(D, ldq, D, 64, D, D, 64, 16, D, 2, 1, 1, head_dim, 0.125, slots, n_slots, pfx_slots,
                                          pfx_len, None)


def decode_rope_shared(lib, *, ldq=192, head_dim=64, slots=D, n_slots=4, pfx_slots=D, pfx_len=D):
    return lib.md_attention_decode_rope_shared(D, ldq, D, 64, D, D, D, 64, 16, D, 2, 1, head_dim, 32, 0.125, slots, n_slots,
                                               pfx_slots, pfx_len, None)


def test_decode_attention_entry_points_refuse_bad_row_tables_and_shapes():
    lib = _lib.load()
    for call, ldq_small in ((decode_shared, 56), (decode_rope_shared, 184)):
        assert call(lib, slots=None) == ERR_ARG          # prefix_slots without slots
        assert call(lib, pfx_len=None) == ERR_ARG        # prefix_slots without prefix_len
        assert call(lib, n_slots=0) == ERR_ARG           # a table with n_slots 0
        assert call(lib, n_slots=0, pfx_slots=None, pfx_len=None) == ERR_ARG  # ... with or without a prefix table
        assert call(lib, head_dim=72) == ERR_ARG
        assert call(lib, head_dim=72, pfx_slots=None, pfx_len=None) == ERR_ARG
        assert call(lib, ldq=ldq_small) == ERR_ARG       # ldq below (3 x) n_heads x 64
        assert call(lib, ldq=ldq_small, pfx_slots=None, pfx_len=None) == ERR_ARG
    assert decode_rope_shared(lib, ldq=128) == ERR_ARG   # wide enough for q alone, not for the fused [q | k | v] row


def tiny_text_model():
    m = _lib.MdTextModel()
    m.n_layers, m.n_heads, m.n_kv_heads, m.dim = 3, 4, 4, 256
    blocks = (_lib.MdTextBlock * 3)()
    m.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.MdTextBlock))
    return m, blocks


def test_shared_entry_points_refuse_the_e4m3_copy():
    lib = _lib.load()
    m, _blocks = tiny_text_model()
    kv8 = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    kv8.k8, kv8.v8 = 0x3000, 0x4000
    assert lib.md_text_forward_shared(ctypes.byref(m), D, D, 2, 1, D, D, 4, D, D, ctypes.byref(kv8), D, 1 << 20, None) == ERR_ARG
    assert lib.md_decode_step_shared(ctypes.byref(m), D, D, D, 2, D, 4, D, D, ctypes.byref(kv8), 0, D, 64, D, 1 << 20,
                                     None) == ERR_ARG
    # ... also without a prefix table
    assert lib.md_text_forward_shared(ctypes.byref(m), D, D, 2, 1, D, D, 4, None, None, ctypes.byref(kv8), D, 1 << 20,
                                      None) == ERR_ARG
    assert lib.md_decode_step_shared(ctypes.byref(m), D, D, D, 2, D, 4, None, None, ctypes.byref(kv8), 0, D, 64, D, 1 << 20,
                                     None) == ERR_ARG


def test_multi_lora_entry_points_refuse_bad_tables_layers_and_fp8():
    lib = _lib.load()
    m, _blocks = tiny_text_model()
    bank = _lib.MdLoraBank()
    bank.n_layers, bank.n_variants, bank.table = 3, 1, 0x1000
    bank.rank[0][0] = 16
    kv = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    mp, bp, kvp = ctypes.byref(m), ctypes.byref(bank), ctypes.byref(kv)

    def forward(variant=D, kvp=kvp):
        return lib.md_text_forward_multi_lora(mp, bp, variant, D, D, 2, 1, D, None, 0, kvp, D, 1 << 20, None)

    def step(variant=D, kvp=kvp):
        return lib.md_decode_step_multi_lora(mp, bp, variant, D, D, D, 2, None, 0, kvp, 0, D, 64, D, 1 << 20, None)

    for call in (forward, step):
        assert call(variant=None) == ERR_ARG  # no variant table
        bank.n_layers = 4                     # not the model's
        assert call() == ERR_ARG
        bank.n_layers = 3
        kv8 = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
        kv8.k8, kv8.v8 = 0x3000, 0x4000
        assert call(kvp=ctypes.byref(kv8)) == ERR_UNSUPPORTED  # the e4m3 copy of the cache
        fp8_blocks = (_lib.MdTextBlockFp8 * 3)()  # the fp8 weight copies
        fp8 = _lib.MdTextFp8(ctypes.cast(fp8_blocks, ctypes.POINTER(_lib.MdTextBlockFp8)))
        m.fp8 = ctypes.pointer(fp8)
        assert call() == ERR_UNSUPPORTED
        m.fp8 = None
        f8 = _lib.MdTextF8()                      # the FP8 prefill mode
        m.f8 = ctypes.pointer(f8)
        assert call() == ERR_UNSUPPORTED
        m.f8 = None


def test_slot_table_without_slots_is_refused():
    lib = _lib.load()
    m, _blocks = tiny_text_model()
    kv = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    assert lib.md_text_forward_slots(ctypes.byref(m), D, D, 2, 1, D, D, 0, ctypes.byref(kv), D, 1 << 20, None) == ERR_ARG
    assert lib.md_decode_step_slots(ctypes.byref(m), D, D, D, 2, D, 0, ctypes.byref(kv), 0, D, 64, D, 1 << 20, None) == ERR_ARG
