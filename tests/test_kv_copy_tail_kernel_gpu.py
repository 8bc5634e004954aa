"""md_kv_copy_tail on the MI355X through the C ABI: EXACT equality of every byte of both slabs with a numpy restatement --
the named runs copied, in K and V and in every layer and head, and the whole rest of the slabs as before the call (a
one-position or one-head overrun shows there)."""
import ctypes as C

import numpy as np
import pytest
import torch

from moondream_amd import _lib

pytestmark = pytest.mark.gpu
LAYERS, HEADS, CTX, SLOTS, HD = 2, 3, 40, 7, 64
MD_ERR_INVALID_ARG = 1  # include/moondream_hip.h


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def slabs():
    """K and V int16 [LAYERS][SLOTS][HEADS][CTX][HD], every element a function of its own address (and of K / V)."""
    n = LAYERS * SLOTS * HEADS * CTX * HD
    idx = np.arange(n, dtype=np.int64)
    k = ((idx * 2654435761) >> 7).astype(np.int16).reshape(LAYERS, SLOTS, HEADS, CTX, HD)
    v = ((idx * 40503 + 12345) >> 3).astype(np.int16).reshape(LAYERS, SLOTS, HEADS, CTX, HD)
    return k, v


def kv_struct(d_k, d_v, k8=None):
    bs = HEADS * CTX * HD
    kv = _lib.MdKvCache(d_k.data_ptr(), d_v.data_ptr(), SLOTS * bs, bs, CTX)
    if k8 is not None:
        kv.k8, kv.v8 = k8.data_ptr(), k8.data_ptr()
    return kv


def reference(k, v, rows):
    k2, v2 = k.copy(), v.copy()
    for s, d, p0, p1 in rows:
        if d < 0 or s < 0 or s == d or p1 <= p0:
            continue
        k2[:, d, :, p0:p1] = k[:, s, :, p0:p1]
        v2[:, d, :, p0:p1] = v[:, s, :, p0:p1]
    return k2, v2


def launch(lib, rows):
    k, v = slabs()
    d_k, d_v = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    cols = [torch.tensor([r[c] for r in rows], dtype=torch.int32).cuda() for c in range(4)]
    kv = kv_struct(d_k, d_v)
    st = lib.md_kv_copy_tail(C.byref(kv), LAYERS, HEADS, SLOTS, len(rows), *(t.data_ptr() for t in cols), stream())
    assert st == 0, st
    torch.cuda.synchronize()
    return (k, v), (d_k.cpu().numpy(), d_v.cpu().numpy())


# (src, dst, from, to): run lengths 0, 1, 5 and 39; two children of parent slot 0; a src == dst row, a dst = -1 row, a
# src = -1 row.  Live dsts {2, 3, 5} are distinct and none is a live src {0, 4}: the caller contract.
ROWS = [(0, 1, 3, 3), (0, 2, 1, 2), (0, 3, 0, 5), (4, 5, 1, 40), (6, 6, 0, 10), (4, -1, 0, 10), (-1, 6, 0, 4)]


def test_runs_copied_and_nothing_else(lib):
    (k, v), (gk, gv) = launch(lib, ROWS)
    wk, wv = reference(k, v, ROWS)
    for name, got, want, before in (("k", gk, wk, k), ("v", gv, wv, v)):
        for s, d, p0, p1 in ROWS:  # every named run, in every layer and head
            if d >= 0 and s >= 0 and s != d and p1 > p0:
                assert np.array_equal(got[:, d, :, p0:p1], before[:, s, :, p0:p1]), (name, s, d, p0, p1)
        bad = np.argwhere(got != want)  # and the whole slab: the rest is what it was
        assert bad.size == 0, (name, len(bad), bad[:6].tolist())
    assert not np.array_equal(gk, k) and not np.array_equal(gv, v)  # (something was copied)


def test_skipped_rows_and_empty_launch(lib):
    """Only rows the contract skips -- and slots / positions outside the slabs, for which no address may be formed: both
    slabs byte for byte as before.  rows == 0 is MD_OK without a launch."""
    rows = [(2, 2, 0, 40), (3, -1, 0, 40), (-1, 3, 0, 40), (1, 2, 7, 7), (1, 2, 9, 3), (1, SLOTS, 0, 4), (SLOTS, 1, 0, 4),
            (1, 2, -1, 4), (1, 2, 30, CTX + 1)]
    (k, v), (gk, gv) = launch(lib, rows)
    assert np.array_equal(gk, k) and np.array_equal(gv, v)
    d = torch.zeros(8, dtype=torch.int32).cuda()
    kv = kv_struct(d, d)
    assert lib.md_kv_copy_tail(C.byref(kv), LAYERS, HEADS, SLOTS, 0, *([d.data_ptr()] * 4), stream()) == 0


def test_invalid_arguments(lib):
    k, v = slabs()
    d_k, d_v = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    a = torch.zeros(4, dtype=torch.int32).cuda()
    p = a.data_ptr()
    kv = kv_struct(d_k, d_v)
    call = lambda kv_, rows=1, n_slots=SLOTS, ptrs=(p, p, p, p): lib.md_kv_copy_tail(
        C.byref(kv_) if kv_ is not None else None, LAYERS, HEADS, n_slots, rows, *ptrs, stream())
    assert call(None) == MD_ERR_INVALID_ARG
    assert call(kv, rows=-1) == MD_ERR_INVALID_ARG
    assert call(kv, n_slots=0) == MD_ERR_INVALID_ARG
    assert call(kv, n_slots=SLOTS + 1) == MD_ERR_INVALID_ARG  # more slots than a layer holds
    for i in range(4):
        assert call(kv, ptrs=tuple(None if j == i else p for j in range(4))) == MD_ERR_INVALID_ARG
    assert call(kv_struct(d_k, d_v, k8=d_k)) == MD_ERR_INVALID_ARG  # the e4m3 copy attached: not served
    torch.cuda.synchronize()
    assert np.array_equal(d_k.cpu().numpy(), k) and np.array_equal(d_v.cpu().numpy(), v)
