"""The host-side argument checks of md_text_forward_trim, without a GPU: called with a null stream and pointers that are
never dereferenced, the library refuses a bad hidden mode or a missing / misaligned hidden_last before any launch."""
import ctypes

from moondream_amd import _lib

ERR_ARG = 1
D = ctypes.c_void_p(0x10)  # never dereferenced: every call below fails its host checks first


def tiny_text_model():
    m = _lib.MdTextModel()
    m.n_layers, m.n_heads, m.n_kv_heads, m.dim = 3, 4, 4, 256
    blocks = (_lib.MdTextBlock * 3)()
    m.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.MdTextBlock))
    return m, blocks


def trim(lib, m, kv, *, mode, hidden_last=D, slots=None, n_slots=0, pfx_slots=None, pfx_len=None, batch=2, q_len=40):
    return lib.md_text_forward_trim(ctypes.byref(m), D, D, hidden_last, mode, batch, q_len, D, slots, n_slots, pfx_slots, pfx_len,
                                    ctypes.byref(kv), D, 1 << 20, None)


def test_hidden_modes_are_the_three_values():
    assert (_lib.MD_HIDDEN_ALL, _lib.MD_HIDDEN_LAST, _lib.MD_HIDDEN_NONE) == (0, 1, 2)
    assert _lib.MD_TILE_PINNED_ANY_ROWS == 3
    lib = _lib.load()
    m, _blocks = tiny_text_model()
    kv = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    for mode in (-1, 3, 7):
        assert trim(lib, m, kv, mode=mode) == ERR_ARG
        assert trim(lib, m, kv, mode=mode, hidden_last=None) == ERR_ARG


def test_last_mode_needs_an_aligned_hidden_last():
    lib = _lib.load()
    m, _blocks = tiny_text_model()
    kv = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    assert trim(lib, m, kv, mode=_lib.MD_HIDDEN_LAST, hidden_last=None) == ERR_ARG
    assert trim(lib, m, kv, mode=_lib.MD_HIDDEN_LAST, hidden_last=ctypes.c_void_p(0x18)) == ERR_ARG
    assert trim(lib, m, kv, mode=_lib.MD_HIDDEN_LAST, hidden_last=None, slots=D, n_slots=4) == ERR_ARG


def test_row_tables_are_checked_as_in_the_all_rows_entry_points():
    lib = _lib.load()
    m, _blocks = tiny_text_model()
    kv = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
    for mode in (_lib.MD_HIDDEN_ALL, _lib.MD_HIDDEN_LAST, _lib.MD_HIDDEN_NONE):
        assert trim(lib, m, kv, mode=mode, slots=D, n_slots=0) == ERR_ARG               # a slot table with n_slots 0
        assert trim(lib, m, kv, mode=mode, pfx_slots=D, pfx_len=D) == ERR_ARG           # a prefix table without a slot table
        assert trim(lib, m, kv, mode=mode, slots=D, n_slots=4, pfx_slots=D) == ERR_ARG  # ... without prefix_len
        kv8 = _lib.MdKvCache(0x1000, 0x2000, 4 * 64, 64, 16)
        kv8.k8, kv8.v8 = 0x3000, 0x4000
        assert trim(lib, m, kv8, mode=mode, slots=D, n_slots=4, pfx_slots=D, pfx_len=D) == ERR_ARG  # the e4m3 copy with a prefix table
        assert trim(lib, m, kv, mode=mode, batch=0) == ERR_ARG
        assert trim(lib, m, kv, mode=mode, q_len=0) == ERR_ARG
