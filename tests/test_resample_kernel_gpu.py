"""md_image_resample_crops on the MI355X through the C ABI: EXACT equality of every byte of the crops buffer with
``image_crops.overlap_crop_image`` run on the host (its PIL branch), over one launch on a mixed chunk -- row lengths that
are no multiple of 4, the identity, a one-pixel shrink, multi-tile downscales and an upscale -- with sentinels around the
buffer, and the same chunk again in another order so that every descriptor offset differs."""
import ctypes as C

import numpy as np
import pytest
import torch

from moondream_amd import _lib, image_crops, resample
from moondream_amd.config import get_config

pytestmark = pytest.mark.gpu
MD_ERR_INVALID_ARG, MD_ERR_WORKSPACE = 1, 3  # include/moondream_hip.h
V = get_config("tiny").vision
CROP, WINDOW, MARGIN_PX = 378, 266, 56
CROP_BYTES = CROP * CROP * 3
# (H, W): W * 3 not a multiple of 4 (33x41, 97x1301), the identity, one axis identity, multi-tile downscales ((3, 3) and (5, 2)),
# a one-pixel shrink (2, 4), the upscale (4, 2), a multi-tile upscale (2, 4)
SIZES = [(33, 41), (1000, 1400), (378, 378), (97, 1301), (491, 379), (379, 378), (1400, 600), (645, 1177), (500, 700)]
GUARD = 4096


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    if image_crops.resize_backend() != "pil":
        pytest.skip("the device path implements the PIL branch")
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def image(h, w):
    """Random bytes with saturated 0 / 255 stripes over a quarter of the rows and columns: both clamps fire."""
    img = np.random.default_rng(h * 20011 + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[: max(h // 4, 1)] = ((np.arange(w) & 1) * 255).astype(np.uint8)[None, :, None]
    img[:, : max(w // 4, 1)] = ((np.arange(h) & 1) * 255).astype(np.uint8)[:, None, None]
    return img


@pytest.fixture(scope="module")
def host():
    """size -> (image, the host path's crops): computed once."""
    out = {}
    for h, w in SIZES:
        img = image(h, w)
        out[(h, w)] = (img, image_crops.overlap_crop_image(img, V.overlap_margin, V.max_crops)["crops"].copy())
    return out


def launch(lib, sizes, host, dedup=False):
    """One call over the chunk -> (crops uint8 [slots, 378, 378, 3], guard bytes before, after, the layout, the records)."""
    records = resample.plan(sizes, V)
    lay = resample.layout(records, V, dedup=dedup)
    buf = np.zeros(lay.nbytes, dtype=np.uint8)
    lay.write(buf, [host[s][0] for s in sizes])
    packed = torch.from_numpy(buf).cuda()
    need = lib.md_image_resample_workspace_bytes(lay.desc.ctypes.data, len(sizes))
    assert need == lay.ws_bytes
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    pattern = (np.arange(GUARD * 2 + lay.out_crops * CROP_BYTES, dtype=np.int64) * 37 + 11).astype(np.uint8)
    out = torch.from_numpy(pattern.copy()).cuda()
    st = lib.md_image_resample_crops(packed.data_ptr(), packed.numel(), lay.desc.ctypes.data, len(sizes), CROP, WINDOW, MARGIN_PX,
                                     out.data_ptr() + GUARD, lay.out_crops, ws.data_ptr(), ws.numel(), stream())
    assert st == 0, st
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:GUARD], pattern[:GUARD]) and np.array_equal(got[-GUARD:], pattern[-GUARD:]), "sentinels overwritten"
    return got[GUARD:-GUARD].reshape(lay.out_crops, CROP, CROP, 3), lay, records


def check_chunk(crops, sizes, records, host, dedup=False):
    slot = 0
    for size, r in zip(sizes, records):
        want = host[size][1]
        assert want.shape[0] == r.n_crops
        if r.both_slots:
            assert np.array_equal(want[0], want[1])
            if dedup:
                want = want[:1]
            else:
                assert np.array_equal(crops[slot], crops[slot + 1]), size  # crop 0 == crop 1
        got = crops[slot : slot + want.shape[0]]
        bad = np.argwhere(got != want)
        assert bad.size == 0, (size, r.tiling, len(bad), bad[:4].tolist())
        slot += want.shape[0]
    assert slot == crops.shape[0]


def test_mixed_chunk_equals_the_host_crops(lib, host):
    crops, lay, records = launch(lib, SIZES, host)
    assert lay.out_crops == sum(r.n_crops for r in records) == 2 * 4 + 10 + 11 + 9 + 9 + 9
    check_chunk(crops, SIZES, records, host)


def test_same_chunk_in_another_order(lib, host):
    sizes = SIZES[::-1][2:] + SIZES[::-1][:2]
    crops, lay, records = launch(lib, sizes, host)
    check_chunk(crops, sizes, records, host)


def test_single_slot_mode(lib, host):
    """Images of tiling (1, 1) written to one slot (what ``dedup_identical_crops`` asks for), between images that keep all theirs."""
    sizes = [(97, 1301), (491, 379), (33, 41), (378, 378)]
    crops, lay, records = launch(lib, sizes, host, dedup=True)
    assert lay.out_crops == 1 + 9 + 1 + 1 and lay.expand == [0, 0] + list(range(1, 10)) + [10, 10, 11, 11]
    check_chunk(crops, sizes, records, host, dedup=True)


def test_invalid_arguments(lib, host):
    sizes = [(33, 41), (491, 379)]
    records = resample.plan(sizes, V)
    lay = resample.layout(records, V)
    buf = np.zeros(lay.nbytes, dtype=np.uint8)
    lay.write(buf, [host[s][0] for s in sizes])
    packed = torch.from_numpy(buf).cuda()
    ws = torch.empty(lay.ws_bytes, dtype=torch.uint8, device="cuda")
    before = torch.full((lay.out_crops * CROP_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
    out = before.clone()

    def call(desc=lay.desc, packed_ptr=None, nbytes=lay.nbytes, n=len(sizes), geometry=(CROP, WINDOW, MARGIN_PX), out_ptr=None,
             total=lay.out_crops, ws_ptr=None, ws_bytes=lay.ws_bytes):
        return lib.md_image_resample_crops(
            packed.data_ptr() if packed_ptr is None else packed_ptr, nbytes, desc.ctypes.data if desc is not None else None, n, *geometry,
            out.data_ptr() if out_ptr is None else out_ptr, total, ws.data_ptr() if ws_ptr is None else ws_ptr, ws_bytes, stream())

    def edited(image, word, value):
        d = lay.desc.copy()
        d[image, word] = value
        return d

    assert call(desc=None) == MD_ERR_INVALID_ARG
    assert call(packed_ptr=0) == MD_ERR_INVALID_ARG and call(out_ptr=0) == MD_ERR_INVALID_ARG and call(ws_ptr=0) == MD_ERR_INVALID_ARG
    assert call(packed_ptr=packed.data_ptr() + 4) == MD_ERR_INVALID_ARG  # the pixels' alignment starts at the base
    assert call(n=0) == MD_ERR_INVALID_ARG and call(n=-1) == MD_ERR_INVALID_ARG
    assert call(nbytes=lay.nbytes - 1) == MD_ERR_INVALID_ARG  # the last image would end outside the buffer
    assert call(geometry=(CROP, WINDOW, MARGIN_PX + 1)) == MD_ERR_INVALID_ARG
    assert call(total=lay.out_crops - 1) == MD_ERR_INVALID_ARG and call(total=lay.out_crops + 1) == MD_ERR_INVALID_ARG
    assert call(ws_bytes=lay.ws_bytes - 1) == MD_ERR_WORKSPACE
    assert call(desc=edited(0, resample.D_SRC_H, 0)) == MD_ERR_INVALID_ARG
    assert call(desc=edited(0, resample.D_SRC_W, 16385)) == MD_ERR_INVALID_ARG
    assert call(desc=edited(1, resample.D_MODE, 3)) == MD_ERR_INVALID_ARG
    assert call(desc=edited(1, resample.D_CROP0, 3)) == MD_ERR_INVALID_ARG
    assert call(desc=edited(1, resample.D_PIXELS, int(lay.desc[1, resample.D_PIXELS]) + 4)) == MD_ERR_INVALID_ARG
    assert call(desc=edited(1, resample.D_TH, 5)) == MD_ERR_INVALID_ARG  # the tiled target is not the geometry's
    t1 = resample.D_TARGET0 + resample.D_TARGET_WORDS
    assert call(desc=edited(1, t1 + resample.T_KX, lay.nbytes)) == MD_ERR_INVALID_ARG
    assert call(desc=edited(1, t1 + resample.T_VBLK0, 0)) == MD_ERR_INVALID_ARG
    assert lib.md_image_resample_workspace_bytes(None, 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)  # nothing was launched
