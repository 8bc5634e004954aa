"""The host half of the bf16 GEMM dispatch (csrc/gemm_bf16.hip), without a GPU: the loaded library answers its host-only
questions (workspace bytes, partial slices) and refuses bad launches before anything is launched.

Every expected value below was recorded from the library of the commit BEFORE the dispatch got its tile table, decode-config
selector, split-K geometry and launch plan -- built on the same machine, not from the code under test -- and this file passed
unchanged against that library.  Pointers are dummies (non-null, 16-byte aligned) that no host check dereferences; the tests
that hand them to a launching entry point run only where there is no device to launch on."""
import ctypes as C

import pytest
import torch

from moondream_amd import _lib

OK, ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED = 0, 1, 2, 4
P = 0x1000  # never dereferenced
# a call that slipped past the host checks would LAUNCH on the dummy pointers where a device is present
no_device = pytest.mark.skipif(torch.cuda.is_available(),
                               reason="hands dummy pointers to launching entry points: only without a device")

# (k, n) of the tiny, 0.5B and 2B layers of test_decode_regime_configs_agree_bitwise / test_decode_tall_gpu.py
LAYERS = [(2048, 14336), (2048, 2048), (8192, 2048), (2048, 51200), (704, 256), (1152, 1000), (256, 1024), (4352, 1152)]
MS = [1, 64, 65, 128, 129]


def linear(k, n):
    up = lambda x: (x + 63) // 64 * 64
    return _lib.MdLinear(P, P, n, k, up(n), up(k))


PARTIAL_SLICES = [1, 8, 8, 1, 8, 8, 4, 8]  # per layer of LAYERS

# md_gemm_workspace_bytes: one row per layer of LAYERS; columns = m of MS with store_pad_cols 0, then the same with 1
NO_SPLIT = [[0] * 10 for _ in LAYERS]  # "decode_slices" = 1
BY_SHAPE_64 = [  # "decode_slices" = 0 under the 64-wide configs
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [4202496, 4202496, 8396800, 8396800, 0, 4202496, 4202496, 8396800, 8396800, 0],
    [4202496, 4202496, 8396800, 8396800, 0, 4202496, 4202496, 8396800, 8396800, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [270336, 270336, 532480, 532480, 0, 270336, 270336, 532480, 532480, 0],
    [2105344, 2105344, 4202496, 4202496, 0, 2105344, 2105344, 4202496, 4202496, 0],
    [532480, 532480, 1056768, 1056768, 0, 532480, 532480, 1056768, 1056768, 0],
    [2367488, 2367488, 4726784, 4726784, 0, 2367488, 2367488, 4726784, 4726784, 0],
]
# "decode_slices" = 0 under the 128-wide config (3): the widest fused layer splits at <= 64 rows, and the tall sizes stay
BY_SHAPE_128 = [
    [7348224, 7348224, 0, 0, 0, 7348224, 7348224, 0, 0, 0],
] + BY_SHAPE_64[1:]
FOUR_SLICES = [  # "decode_slices" = 4, every config
    [14688256, 14688256, 29368320, 29368320, 0, 14688256, 14688256, 29368320, 29368320, 0],
    [2105344, 2105344, 4202496, 4202496, 0, 2105344, 2105344, 4202496, 4202496, 0],
    [2105344, 2105344, 4202496, 4202496, 0, 2105344, 2105344, 4202496, 4202496, 0],
    [52436992, 52436992, 104865792, 104865792, 0, 52436992, 52436992, 104865792, 104865792, 0],
    [270336, 270336, 532480, 532480, 0, 270336, 270336, 532480, 532480, 0],
    [1056768, 1056768, 2105344, 2105344, 0, 1056768, 1056768, 2105344, 2105344, 0],
    [1056768, 1056768, 2105344, 2105344, 0, 1056768, 1056768, 2105344, 2105344, 0],
    [1187840, 1187840, 2367488, 2367488, 0, 1187840, 1187840, 2367488, 2367488, 0],
]
WORKSPACE_BYTES = {  # (decode_cfg, decode_slices)
    (16, 0): BY_SHAPE_64, (16, 1): NO_SPLIT, (16, 4): FOUR_SLICES,
    (17, 0): BY_SHAPE_64, (17, 1): NO_SPLIT, (17, 4): FOUR_SLICES,
    (10, 0): BY_SHAPE_64, (10, 1): NO_SPLIT, (10, 4): FOUR_SLICES,
    (3, 0): BY_SHAPE_128, (3, 1): NO_SPLIT, (3, 4): FOUR_SLICES,
}


@pytest.mark.parametrize("cfg,slices", sorted(WORKSPACE_BYTES))
def test_workspace_bytes_and_partial_slices_are_what_they_were(cfg, slices):
    lib = _lib.load()
    try:
        _lib.check(lib.md_gemm_set_tuning(b"decode_cfg", cfg))
        _lib.check(lib.md_gemm_set_tuning(b"decode_slices", slices))
        for (k, n), want, want_slices in zip(LAYERS, WORKSPACE_BYTES[(cfg, slices)], PARTIAL_SLICES):
            st = linear(k, n)
            got = [lib.md_gemm_workspace_bytes(C.byref(st), m, pad) for pad in (0, 1) for m in MS]
            assert got == want, (cfg, slices, k, n)
            assert lib.md_gemm_partial_slices(C.byref(st)) == want_slices, (cfg, slices, k, n)
    finally:
        lib.md_gemm_set_tuning(b"decode_cfg", 16)
        lib.md_gemm_set_tuning(b"decode_slices", 0)
    assert lib.md_gemm_workspace_bytes(None, 1, 0) == 0
    assert lib.md_gemm_partial_slices(None) == 0


# every key md_gemm_set_tuning takes, with the value the library starts from (Knobs' initialisers, g_attn_skip_dead, g_w4_grid)
TUNING_DEFAULTS = dict(tile=-1, w4=1, w4_grid=0, decode_cfg=16, decode_slices=0, rope_fuse=1, group_m=0, persist=1, decode_nt=0,
                       small_m_rule=1, attn_skip_dead=3)
# keys of the measurement variants that were retired with their kernels: unknown keys now
RETIRED_TUNING_KEYS = ["w4_variant", "w4_dbg_lo", "w4_dbg_hi"]


def test_tuning_keys_the_kept_ones_and_the_retired_ones():
    lib = _lib.load()
    try:
        for key in RETIRED_TUNING_KEYS:
            assert lib.md_gemm_set_tuning(key.encode(), 0) == ERR_ARG, key
        for key, default in TUNING_DEFAULTS.items():
            assert lib.md_gemm_set_tuning(key.encode(), default) == OK, key
    finally:  # (there is no getter: the defaults are what the other tests of this process expect)
        for key, default in TUNING_DEFAULTS.items():
            lib.md_gemm_set_tuning(key.encode(), default)
    assert lib.md_gemm_set_tuning(None, 0) == ERR_ARG


def gemm_args(**kw):
    """A launch every host check accepts: 100 rows of the (2048, 2048) layer."""
    f = dict(a=P, lda=2048, n=2048, k=2048, n_pad=2048, k_pad=2048, w=P, c=P, ldc=2048, r=None, ldr=0, res_row_mod=0, m=100,
             epilogue=_lib.MD_EPI_BIAS, store_pad_cols=0, gelu_from_col=0, tile_policy=_lib.MD_TILE_BY_SHAPE)
    f.update(kw)
    lin = _lib.MdLinear(f["w"], P, f["n"], f["k"], f["n_pad"], f["k_pad"])
    return _lib.MdGemmArgs(f["a"], f["lda"], lin, f["c"], f["ldc"], f["r"], f["ldr"], f["res_row_mod"], f["m"], f["epilogue"],
                           f["store_pad_cols"], f["gelu_from_col"], None, 0, f["tile_policy"])


def status(**kw):
    args = gemm_args(**kw)
    return _lib.load().md_gemm_bf16(C.byref(args), None)


RES = dict(epilogue=_lib.MD_EPI_RESIDUAL, r=P, ldr=2048)
BAD_ARGS = [
    dict(a=None),
    dict(c=None),
    dict(w=None),
    dict(m=0),
    dict(n=0),
    dict(k=0),
    dict(k_pad=2080, lda=2080),            # k_pad % 64
    dict(k=2049),                          # k_pad < k
    dict(n_pad=2080),                      # n_pad % 64
    dict(n=2056),                          # n_pad < n
    dict(n=2044),                          # n % 8 without store_pad_cols
    dict(gelu_from_col=-8),
    dict(gelu_from_col=4),
    dict(lda=2040),                        # lda < k_pad
    dict(lda=2052),                        # lda % 8
    dict(ldc=2052),                        # ldc % 8
    dict(a=P + 8),
    dict(c=P + 8),
    dict(w=P + 8),
    dict(n=1000, n_pad=1024, ldc=992),     # ldc < n
    dict(n=1000, n_pad=1024, ldc=1000, store_pad_cols=1),  # ldc < n_pad when the pad columns are stored
    dict(tile_policy=4),
    dict(tile_policy=-1),
    dict(tile_policy=7),
    dict(RES, r=None),
    dict(RES, ldr=2052),
    dict(RES, r=P + 8),
    dict(epilogue=3),
]


@no_device
@pytest.mark.parametrize("bad", BAD_ARGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_dispatch_refuses_each_bad_argument(bad):
    assert status(**bad) == ERR_ARG
    assert _lib.load().md_gemm_bf16(None, None) == ERR_ARG


@no_device
def test_pinned_launch_the_four_wave_kernel_cannot_take():
    """m * lda * 2 >= 4 GiB is beyond the four-wave kernel's 32-bit offsets: under MD_TILE_PINNED the launch is cut into row
    blocks, and what cannot be cut -- a broadcast residual -- is refused.  The launch that CAN be cut passes every host check,
    so without a device it ends in MD_ERR_LAUNCH."""
    big = dict(m=(1 << 32) // (2048 * 2) + 5, tile_policy=_lib.MD_TILE_PINNED)
    assert status(**big, **RES, res_row_mod=729) == ERR_UNSUPPORTED
    assert status(**dict(big, tile_policy=_lib.MD_TILE_PINNED_ANY_ROWS), **RES, res_row_mod=729) == ERR_UNSUPPORTED
    assert status(**big) == ERR_LAUNCH
    assert status(**big, **RES) == ERR_LAUNCH
    assert status() == ERR_LAUNCH
    assert status(m=1) == ERR_LAUNCH


@no_device
def test_partial_entry_points_refuse_too_many_rows_and_misaligned_partials():
    lib = _lib.load()
    st = linear(2048, 2048)
    ref = C.byref(st)

    def one(m=64, partial=P, ld=2048, stride=None):
        return lib.md_gemm_partial_f32(P, 2048, ref, m, partial, ld, m * ld if stride is None else stride, None)

    def pair(m=64, partial0=P, partial1=P, ld=2048, stride=None):
        return lib.md_gemm_partial_f32_pair(P, 2048, ref, partial0, P, 2048, ref, partial1, m, ld,
                                            m * ld if stride is None else stride, None)

    for call in (one, pair):
        assert call(m=129) == ERR_ARG
        assert call(m=0) == ERR_ARG
        assert call(ld=2046) == ERR_ARG                 # ld_partial % 4
        assert call(ld=2044) == ERR_ARG                 # ld_partial < n
        assert call(stride=64 * 2048 - 4) == ERR_ARG    # slices overlap
        assert call(stride=64 * 2048 + 2) == ERR_ARG    # slice_stride % 4
    assert one(partial=P + 8) == ERR_ARG
    assert one(partial=None) == ERR_ARG
    assert pair(partial0=P + 8) == ERR_ARG
    assert pair(partial1=P + 8) == ERR_ARG
    assert one() == ERR_LAUNCH and one(m=128) == ERR_LAUNCH  # these pass the host checks
    assert pair() == ERR_LAUNCH and pair(m=128) == ERR_LAUNCH
