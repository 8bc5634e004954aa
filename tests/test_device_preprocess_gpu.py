"""``model.device_preprocess`` on the MI355X, tiny model with synthetic weights: resize and tiling on the device hand the ViT
the bytes the host path does, so everything behind it is bit-identical -- image caches, generated ids, detections -- in
one chunk and split over chunks, with and without ``dedup_identical_crops``.  While the switch is on the host tiling is
replaced by functions that raise: the host path is provably not taken."""
import pytest
import torch
from PIL import Image

from moondream_amd import image_crops, synth
from moondream_amd.config import get_config

pytestmark = pytest.mark.gpu
SIZES = [(500, 700), (33, 41), (378, 378), (491, 379)]  # (H, W): tilings (2, 4), (1, 1), (1, 1), (4, 2)


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    """The tiny model, four images of different sizes, and the flag-off results, computed once before the switch is ever on."""
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    assert torch.cuda.is_available(), "GPU tests need a device"
    if image_crops.resize_backend() != "pil":
        pytest.skip("the device path implements the PIL branch")
    c = Ctx()
    c.cfg = cfg = get_config("tiny")
    c.model = m = MoondreamModel(cfg, synth.synthetic_state_dict(cfg, seed=1, device="cuda"), device="cuda", tokenizer=IdTokenizer(),
                                 max_batch=4)
    assert m.device_preprocess is False  # opt-in
    c.images = [Image.fromarray(synth.synthetic_image_array(10 + i, 1, s), "RGB") for i, s in enumerate(SIZES)]
    c.prompts = [list(cfg.tokenizer.templates["caption"]["normal"])] * len(SIZES)
    c.objects = ["7 8", "5", "7 8 9 10", "7 8"]
    c.enc = [m.encode_image(im) for im in c.images[:2]]
    c.ids = m.batch_generate_ids(c.images, c.prompts, max_tokens=6)
    c.det = m.batch_detect(c.images, c.objects, {"max_objects": 2})
    return c


@pytest.fixture()
def on(ctx, monkeypatch):
    """The switch on and the host tiling unreachable; off again afterwards."""
    from moondream_amd import moondream as M

    def refuse(*a, **k):
        raise AssertionError("host tiling ran with device_preprocess on")

    monkeypatch.setattr(M, "overlap_crop_image", refuse)
    monkeypatch.setattr(M, "_crop_into", refuse)
    monkeypatch.setattr(ctx.model._staging, "crop_into", refuse)  # (the stager holds the function it was built with)
    ctx.model.device_preprocess = True
    yield ctx.model
    ctx.model.device_preprocess = False
    ctx.model.dedup_identical_crops = False
    ctx.model.vit_chunk_crops = 128


def test_the_guard_really_guards(ctx, on):
    """With the switch off again the replaced host functions are what a call reaches: the monkeypatch is on the live path."""
    on.device_preprocess = False
    with pytest.raises(AssertionError, match="host tiling ran"):
        on.encode_image(ctx.images[1])


def test_encode_image_caches_are_bit_identical(ctx, on):
    for im, want in zip(ctx.images[:2], ctx.enc):
        got = on.encode_image(im)
        assert got.pos == want.pos and len(got.caches) == len(want.caches)
        for (gk, gv), (wk, wv) in zip(got.caches, want.caches):
            assert torch.equal(gk, wk) and torch.equal(gv, wv)


@pytest.mark.parametrize("chunk", [4, 128])
def test_batch_generate_ids_one_chunk_and_split(ctx, on, chunk):
    on.vit_chunk_crops = chunk  # 4: crop counts 9, 2, 2, 9 -> the batch is split over chunks
    assert on.batch_generate_ids(ctx.images, ctx.prompts, max_tokens=6) == ctx.ids


def test_batch_detect_returns_the_same_dicts(ctx, on):
    assert on.batch_detect(ctx.images, ctx.objects, {"max_objects": 2}) == ctx.det


def test_dedup_identical_crops_on_and_off(ctx, on):
    on.dedup_identical_crops = True
    assert on.batch_generate_ids(ctx.images, ctx.prompts, max_tokens=6) == ctx.ids
    on.dedup_identical_crops = False
    assert on.batch_generate_ids(ctx.images, ctx.prompts, max_tokens=6) == ctx.ids


def test_flag_off_results_are_what_they_were(ctx):
    m = ctx.model
    assert m.device_preprocess is False
    assert m.batch_generate_ids(ctx.images, ctx.prompts, max_tokens=6) == ctx.ids
    assert m.batch_detect(ctx.images, ctx.objects, {"max_objects": 2}) == ctx.det
    got = m.encode_image(ctx.images[0])
    for (gk, gv), (wk, wv) in zip(got.caches, ctx.enc[0].caches):
        assert torch.equal(gk, wk) and torch.equal(gv, wv)
