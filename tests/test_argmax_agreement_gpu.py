"""The three entry points whose pick ends in the one (value, index) reduction of csrc/row_reduce.hpp -- md_argmax_bf16,
md_sample_rows at temperature 0 and md_region_pick_encode with one group -- give the same id on rows built to break a
reduction.  The expected id comes from the documented rule, restated on the host: the greater value wins, equal values go
to the lower id, a NaN never wins, the suppressed id counts as -inf, and a row in which nothing wins gives id 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from moondream_amd import _lib

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
VOCAB = 2048 + 8   # md_argmax_bf16: 257 16-byte chunks over 5 waves; the sampling row: 3 ids in 8 threads, 2 in the rest;
LD = VOCAB + 24    # the region pick (256 threads): 9 bins in 8 threads, 8 in the rest.  Padding columns hold NaN.
SUPPRESS = 333
HALF = 8
FILL_ID = -7
NAN = float("nan")


def host_pick(row, suppress):
    """The documented rule, sequentially over ascending ids in fp32."""
    best, bi = -np.inf, 0x7FFFFFFF
    for i, v in enumerate(row):
        v = -np.inf if i == suppress else float(v)
        if v > best or (v == best and i < bi):
            best, bi = v, i
    return bi if bi < len(row) else 0


def make_rows():
    g = torch.Generator().manual_seed(2056)
    x = (torch.randn(7, VOCAB, generator=g) * 3).float()
    assert float(x.abs().max()) < 20.0
    names = []
    x[0, 100] = x[0, 1700] = 25.0  # different waves in all three kernels' strides
    names.append("tie across waves")
    x[1, 1030] = x[1, 40] = 25.0   # sampling row and region pick: one wave, the HIGHER id in the lower lane (6 and 40)
    names.append("tie inside a wave")
    x[2, SUPPRESS] = 25.0
    x[2, 1999] = 22.0
    names.append("maximum at the suppressed id")
    x[3, :] = float("-inf")
    names.append("all -inf")
    x[4, :] = NAN
    names.append("all NaN")
    x[5, 1500] = 25.0
    for i in (0, 1, 63, 64, 1023, 1024, 1499, 1501, 1500 - 256, 1500 - 1024, VOCAB - 1):
        x[5, i] = NAN
    x[5, 8 * 187 : 8 * 187 + 4] = NAN  # the first half of the maximum's own 16-byte chunk (ids 1496 .. 1499)
    names.append("NaNs around a finite maximum")
    x[6, VOCAB - 1] = 25.0
    names.append("maximum at the last column")
    return names, x.to(BF16)


@pytest.fixture(scope="module")
def picks():
    """(names, {suppress: expected ids}, {(entry, suppress): ids}); every launch made once, -1: nothing suppressed."""
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    names, rows = make_rows()
    n = rows.shape[0]
    host = rows.float().numpy()
    want = {sup: [host_pick(host[r], sup) for r in range(n)] for sup in (-1, SUPPRESS)}
    padded = torch.full((n, LD), NAN, dtype=torch.float32).to(BF16)
    padded[:, :VOCAB] = rows
    logits = padded.cuda()
    zero = torch.zeros(n, dtype=torch.float32, device="cuda")
    table = (torch.arange(VOCAB) / VOCAB).to(BF16).cuda()
    w = torch.ones(1, HALF).to(BF16).cuda()
    feats = torch.zeros(n, 2 * HALF, dtype=BF16, device="cuda")

    def fresh():
        return torch.full((n,), FILL_ID, dtype=torch.int32, device="cuda")

    got = {}
    for sup in (-1, SUPPRESS):
        got["md_argmax_bf16", sup] = nxt = fresh()
        _lib.check(lib.md_argmax_bf16(logits.data_ptr(), LD, n, VOCAB, sup, nxt.data_ptr(), stream))
        got["md_sample_rows", sup] = nxt = fresh()
        _lib.check(lib.md_sample_rows(logits.data_ptr(), LD, n, VOCAB, sup, zero.data_ptr(), zero.data_ptr(), zero.data_ptr(),
                                      nxt.data_ptr(), None, 0, stream))
    got["md_region_pick_encode", -1] = nxt = fresh()  # the region pick takes no suppressed id
    _lib.check(lib.md_region_pick_encode(logits.data_ptr(), LD, n, 1, VOCAB, table.data_ptr(), w.data_ptr(), HALF, nxt.data_ptr(), 1,
                                         feats.data_ptr(), 2 * HALF, stream))
    torch.cuda.synchronize()
    return names, want, {k: v.cpu().tolist() for k, v in got.items()}


def test_the_rows_are_the_cases_they_are_named_for(picks):
    """The host rule alone.  With an id suppressed, an all-NaN row gives that id, not 0: the rule reads the suppressed logit as
    -inf, which is no NaN and ties with the value the scan starts from."""
    names, want, _ = picks
    assert dict(zip(names, zip(want[-1], want[SUPPRESS]))) == {
        "tie across waves": (100, 100),
        "tie inside a wave": (40, 40),
        "maximum at the suppressed id": (SUPPRESS, 1999),
        "all -inf": (0, 0),
        "all NaN": (0, SUPPRESS),
        "NaNs around a finite maximum": (1500, 1500),
        "maximum at the last column": (VOCAB - 1, VOCAB - 1),
    }


@pytest.mark.parametrize("entry,suppress", [("md_argmax_bf16", -1), ("md_sample_rows", -1), ("md_region_pick_encode", -1),
                                            ("md_argmax_bf16", SUPPRESS), ("md_sample_rows", SUPPRESS)])
def test_every_entry_picks_the_host_rule_id(picks, entry, suppress):
    names, want, got = picks
    print(entry, suppress, dict(zip(names, zip(got[entry, suppress], want[suppress]))))
    assert dict(zip(names, got[entry, suppress])) == dict(zip(names, want[suppress]))
