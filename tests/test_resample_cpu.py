"""The host plan of the device-side preprocessing (moondream_amd/resample.py) without a GPU: the coefficient tables applied
in numpy (tests/resample_ref.py) reproduce ``PIL.Image.resize(LANCZOS)`` byte for byte, the plan reproduces the tilings of
``image_crops``, the packed upload round-trips, and the model's switch refuses pyvips and falls back over the size limit."""
import types

import numpy as np
import pytest
from PIL import Image

import resample_ref
from moondream_amd import image_crops, resample
from moondream_amd.config import get_config

# (in H x W) -> (out H x W)
PAIRS = [((500, 700), (644, 1176)), ((1000, 1400), (910, 910)), ((1400, 600), (1442, 644)), ((645, 1177), (644, 1176)),
         ((491, 379), (1176, 644)), ((379, 378), (378, 378)), ((33, 41), (378, 378)), ((97, 1301), (378, 378)),
         ((378, 378), (378, 378))]
TILINGS = {(500, 700): (2, 4), (1000, 1400): (3, 3), (1400, 600): (5, 2), (491, 379): (4, 2), (379, 378): (1, 1), (33, 41): (1, 1),
           (97, 1301): (1, 1), (378, 378): (1, 1)}
V = get_config("tiny").vision


def random_image(h, w, seed=0):
    return np.random.default_rng(seed + 7919 * h + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def striped_image(h, w):
    """Alternating 0 / 255 rows and columns: the Lanczos lobes overshoot on both sides, so both clamps fire."""
    y, x = np.arange(h)[:, None, None], np.arange(w)[None, :, None]
    return np.broadcast_to((((y ^ x) & 1) * 255).astype(np.uint8), (h, w, 3)).copy()


def pil_resize(img, height, width):
    return np.asarray(Image.fromarray(img).resize((width, height), resample=Image.Resampling.LANCZOS))


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in PAIRS])
def test_restatement_equals_pil(src, dst):
    for img in (random_image(*src), striped_image(*src)):
        want = pil_resize(img, *dst)
        got = resample_ref.resize(img, *dst)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (len(bad), bad[:4].tolist())


def test_clamps_fire_on_the_stripes():
    """The striped input is only a clamp test if the unclamped sums leave 0 .. 255 on both sides."""
    img = striped_image(491, 379).transpose(1, 0, 2).astype(np.int64)  # the horizontal pass
    bounds, k = resample.coeffs(379, 644)
    lo = hi = 0
    for i in range(bounds.shape[0]):
        x0, n = bounds[i]
        acc = ((img[x0 : x0 + n] * k[i, :n, None, None].astype(np.int64)).sum(axis=0) + (1 << 21)) >> 22
        lo, hi = min(lo, acc.min()), max(hi, acc.max())
    assert lo < 0 and hi > 255, (lo, hi)


def test_coeffs_tables():
    bounds, k = resample.coeffs(378, 378)
    assert k.shape == (378, 1) and (k == 1 << 22).all() and (bounds[:, 0] == np.arange(378)).all() and (bounds[:, 1] == 1).all()
    assert resample.coeffs(378, 378)[1] is k  # cached by (in, out)
    bounds, k = resample.coeffs(1400, 910)
    scale = 1400 / 910
    assert k.shape == (910, int(np.ceil(3 * scale)) * 2 + 1) and k.dtype == np.int32 and bounds.dtype == np.int32
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 1400).all() and (bounds[:, 1] >= 1).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(axis=1)) >= 0).all()  # the kernels' staged span relies on it
    for i in (0, 455, 909):  # nothing beyond a row's taps, and a row sums to one within the rounding of its taps
        assert (k[i, bounds[i, 1] :] == 0).all()
        assert abs(int(k[i].sum()) - (1 << 22)) <= bounds[i, 1]
    with pytest.raises(ValueError):
        resample.coeffs(0, 10)


def test_plan_reproduces_the_tilings():
    sizes = list(TILINGS)
    records = resample.plan(sizes, V)
    crop, window, margin_px = resample.geometry(V)
    assert (crop, window, margin_px) == (378, 266, 56) and V.overlap_margin == 4 and V.max_crops == 12
    for (h, w), r in zip(sizes, records):
        n, tiling = image_crops.crop_count(h, w, V.overlap_margin, V.max_crops)
        assert r.tiling == tiling == TILINGS[(h, w)] and r.n_crops == n == tiling[0] * tiling[1] + 1
        if tiling == (1, 1):
            assert r.targets == ((378, 378),) and r.both_slots  # one resize for both crop slots
        else:
            assert r.targets == ((378, 378), (tiling[0] * 266 + 112, tiling[1] * 266 + 112)) and not r.both_slots
    # the targets of the multi-tile sizes are the out sizes of PAIRS
    assert records[0].targets[1] == (644, 1176) and records[1].targets[1] == (910, 910) and records[2].targets[1] == (1442, 644)
    assert records[3].targets[1] == (1176, 644)


@pytest.mark.parametrize("size", [(33, 41), (491, 379)])
def test_plan_crops_equal_overlap_crop_image(size):
    """The plan's two resizes and window offsets, applied on the host, are ``overlap_crop_image``'s crops."""
    if image_crops.resize_backend() != "pil":
        pytest.skip("the device path implements the PIL branch")
    img = random_image(*size, seed=3)
    want = image_crops.overlap_crop_image(img, V.overlap_margin, V.max_crops)["crops"]
    got = resample_ref.crops_from_plan(img, resample.plan([size], V)[0], V)
    assert np.array_equal(got, want)


def test_limits_send_the_whole_call_to_the_host():
    assert resample.plan([(33, 41), (0, 10)], V) is None
    assert resample.plan([(10, 16385), (33, 41)], V) is None
    assert resample.plan([(16384, 1)], V) is not None


@pytest.mark.parametrize("dedup", [False, True])
def test_packed_layout_round_trips(dedup):
    sizes = [(33, 41), (491, 379), (97, 1301), (33, 41), (500, 700)]
    records = resample.plan(sizes, V)
    lay = resample.layout(records, V, dedup=dedup)
    arrays = [random_image(h, w, seed=i) for i, (h, w) in enumerate(sizes)]
    buf = np.full(lay.nbytes, 0xA5, dtype=np.uint8)
    lay.write(buf, arrays)
    slot = 0
    for (d, pixels, tables), r, a, off in zip(resample.unpack(buf, len(sizes)), records, arrays, lay.pixel_off):
        assert off % 16 == 0 and int(d[resample.D_PIXELS]) == off
        assert np.array_equal(pixels, a)
        assert (int(d[resample.D_SRC_H]), int(d[resample.D_SRC_W])) == (r.height, r.width)
        assert (int(d[resample.D_TH]), int(d[resample.D_TW])) == r.tiling and int(d[resample.D_CROP0]) == slot
        one = r.both_slots and dedup
        assert int(d[resample.D_MODE]) == (resample.MODE_TWO_TARGETS if not r.both_slots else 2 if one else 1)
        slot += 1 if one else r.n_crops
        assert len(tables) == len(r.targets)
        for (oh, ow), (bx, kx, by, ky) in zip(r.targets, tables):
            for got, want in zip((bx, kx), resample.coeffs(r.width, ow)):
                assert np.array_equal(got, want)
            for got, want in zip((by, ky), resample.coeffs(r.height, oh)):
                assert np.array_equal(got, want)
    assert lay.out_crops == slot
    if dedup:
        assert lay.expand == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 11, 11] + list(range(12, 21))
    else:
        assert lay.expand is None and slot == sum(r.n_crops for r in records)
    assert lay.ws_bytes == sum(r.height * resample.inter_pitch(ow) for r in records for _, ow in r.targets)
    # images that do not overlap, each inside the buffer, the last one ending it
    ends = [off + r.height * r.width * 3 for off, r in zip(lay.pixel_off, records)]
    assert all(e <= nxt for e, nxt in zip(ends, lay.pixel_off[1:])) and ends[-1] == lay.nbytes and lay.pixel_off[0] >= lay.head.size
    with pytest.raises(ValueError):
        lay.write(buf, [a[:-1] for a in arrays])


def test_pyvips_backend_is_refused(monkeypatch):
    from moondream_amd.moondream import MoondreamModel

    stand_in = types.SimpleNamespace(_device_preprocess=False)
    monkeypatch.setattr(image_crops, "_pyvips", object())  # resize_backend() == "pyvips"
    with pytest.raises(ValueError, match="MOONDREAM_RESIZE=pil"):
        MoondreamModel.device_preprocess.fset(stand_in, True)
    assert stand_in._device_preprocess is False
    MoondreamModel.device_preprocess.fset(stand_in, False)  # switching it off is always allowed
    monkeypatch.setattr(image_crops, "_pyvips", None)
    MoondreamModel.device_preprocess.fset(stand_in, True)
    assert MoondreamModel.device_preprocess.fget(stand_in) is True


def test_over_limit_side_falls_back_to_the_host_path():
    from moondream_amd.moondream import MoondreamModel

    small, huge = Image.new("RGB", (41, 33)), Image.new("RGB", (16385, 2))
    stand_in = types.SimpleNamespace(_device_preprocess=True, config=types.SimpleNamespace(vision=V),
                                     _staging=types.SimpleNamespace(prefetched={}))
    assert [r.tiling for r in MoondreamModel._device_plan(stand_in, [small, small])] == [(1, 1), (1, 1)]
    assert MoondreamModel._device_plan(stand_in, [small, huge]) is None       # one image over the limit: the whole call
    stand_in._staging.prefetched[(id(small),)] = object()
    assert MoondreamModel._device_plan(stand_in, [small]) is None             # prefetched host crops are used, not redone
    stand_in._device_preprocess = False
    assert MoondreamModel._device_plan(stand_in, [small, small]) is None      # the default
