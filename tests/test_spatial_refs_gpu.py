"""Spatial references in the batched queries on the MI355X (tiny model): the reference's recorded ids through every
batched entry point, row independence, that the refs reach the prompt embeddings of their own row alone, the single
path's values, reasoning, and the refusals."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from moondream_amd import synth
from moondream_amd.config import get_config
from moondream_amd.continuous import ContinuousEngine
from moondream_amd.shared_prefix import plan_rows
from util import elementwise_excess

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def ids_of(text):
    return [int(t) for t in text.split()]


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    path = os.path.join(golden_dir, "tiny_detect.npz")
    if not os.path.exists(path):
        pytest.skip("tiny_detect.npz not generated")
    g = np.load(path)
    cfg = get_config("tiny")
    sd = synth.synthetic_state_dict(cfg, seed=int(g["seed"]), device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=16)
    img = Image.fromarray(synth.synthetic_image_array(int(g["spatial.image_index"]), int(g["seed"]), (378, 378)), "RGB")
    refs = [tuple(g["spatial.refs_point"].tolist()), tuple(g["spatial.refs_box"].tolist())]
    q = " ".join(str(t) for t in g["spatial.question"].tolist())
    return g, cfg, model, img, refs, q


def image(g, k):
    return Image.fromarray(synth.synthetic_image_array(1000 + k, int(g["seed"]), (378, 378)), "RGB")


def test_golden_ids_through_every_batched_entry_point(tiny):
    g, cfg, model, img, refs, q = tiny
    want = g["spatial.tokens"].tolist()
    assert float(g["spatial.margins"].min()) >= 4.0
    st = {"temperature": 0, "max_tokens": len(want)}
    assert ids_of(model.batch_query([img], [q], settings=st, spatial_refs=[refs])[0]) == want          # the fused prefill
    enc = model.encode_image(img)
    assert ids_of(model.batch_query([enc], [q], settings=st, spatial_refs=[refs])[0]) == want          # two passes
    many = model.query_many(img, [q, q], settings={**st, "spatial_refs": [refs, None]})
    assert ids_of(many[0]["answer"]) == want
    assert many[1] == model.query_many(img, [q, q], settings=st)[1]                                    # the ref-less row
    assert ids_of(model.query(img, q, spatial_refs=refs, settings=st)["answer"]) == want              # the single path
    for im in (img, enc):
        eng = ContinuousEngine(model, max_live=4, chunk=4)
        rid = eng.submit_query(im, q, spatial_refs=refs, max_tokens=len(want))
        other = eng.submit_query(im, q + " 14", max_tokens=len(want))  # (a ref-less request beside it, of another length)
        got = dict(eng.run())
        assert got[rid] == want and len(got[other]) <= len(want)


ROW_REFS = [None, [(0.25, 0.75)], [(0.125, 0.25, 0.5, 0.875)], [(0.3, 0.6), (0.2, 0.1, 0.7, 0.4)],
            [(0.1, 0.1, 0.3, 0.3), (0.55, 0.45, 0.95, 0.85)], "golden", [], [(0.4, 0.2, 0.6, 0.9), (0.8, 0.15), (0.05, 0.5, 0.35, 0.7)]]


def eight_rows(tiny):
    g, cfg, model, img, refs, q = tiny
    imgs = [img, image(g, 1), image(g, 2)]
    images = [imgs[i % 3] for i in range(8)]
    questions = [q if i % 2 == 0 else q + " 14 15" for i in range(8)]  # two question lengths
    row_refs = [refs if r == "golden" else r for r in ROW_REFS]
    return images, questions, row_refs


def test_rows_are_independent_under_strict_batch_invariance(tiny):
    g, cfg, model, img, refs, q = tiny
    images, questions, row_refs = eight_rows(tiny)
    st = {"temperature": 0, "max_tokens": 6}
    model.set_strict_batch_invariance(True)
    try:
        enc = {id(im): model.encode_image(im) for im in images}
        encs = [enc[id(im)] for im in images]
        for ims in (images, encs):
            got = model.batch_query(ims, questions, settings=st, spatial_refs=row_refs)
            for i in range(8):
                assert got[i] == model.batch_query([ims[i]], [questions[i]], settings=st, spatial_refs=[row_refs[i]])[0], i
            plain = model.batch_query(ims, questions, settings=st)
            assert [got[i] for i in (0, 6)] == [plain[i] for i in (0, 6)]
            assert model.batch_query(ims, questions, settings=st, spatial_refs=[None] * 7 + [[]]) == plain
        dec = model.tokenizer.decode
        built = model._query_prompts_spatial(encs, questions, row_refs)
        shared = model._string_ids_spatial(encs, st, built, share_prefix=True)
        copied = model._string_ids_spatial(encs, st, built, share_prefix=False)
        assert shared == copied and [dec(s) for s in copied] == got
    finally:
        model.set_strict_batch_invariance(False)


def prompt_embeddings(model, images, questions, row_refs, fused):
    """Every row's prompt embedding rows [B, T, D] through the hook the prefill reads (rows of ONE prompt length)."""
    prompts, rec = model._query_prompts_spatial(images, questions, row_refs)
    assert len({len(p) for p in prompts}) == 1
    with torch.inference_mode():
        embed = model._sequence_embeddings(prompts, images if fused else None, spatial=rec)
        x = embed(0, len(prompts))
    torch.cuda.synchronize()
    return prompts, rec, x[:, x.shape[1] - len(prompts[0]) :].clone()


@pytest.mark.parametrize("fused", [False, True], ids=["prompt", "fused"])
def test_refs_reach_their_own_rows_embeddings_alone(tiny, fused):
    g, cfg, model, img, refs, q = tiny
    tk = cfg.tokenizer
    images = [img, image(g, 1), img, image(g, 2)]
    questions = [q] * 4
    row_refs = [refs, [(0.3, 0.6), (0.2, 0.1, 0.7, 0.4)], [(0.8, 0.15), (0.05, 0.5, 0.35, 0.7)], [(0.5, 0.5), (0.25, 0.5, 0.5, 1.0)]]
    prompts, rec, x = prompt_embeddings(model, images, questions, row_refs, fused)
    head = len(tk.templates["query"]["prefix"])
    assert prompts[0][head : head + 5] == [tk.coord_id, tk.coord_id, tk.coord_id, tk.coord_id, tk.size_id]
    # moving row 2's box changes row 2's placeholder rows and nothing else
    moved = list(row_refs)
    moved[2] = [(0.8, 0.15), (0.1, 0.5, 0.4, 0.7)]
    _, _, y = prompt_embeddings(model, images, questions, moved, fused)
    changed = (x.view(torch.int16) != y.view(torch.int16)).any(dim=2)  # [B, T]
    assert changed[2, head + 2 : head + 5].any() and not changed[2, : head + 2].any() and not changed[2, head + 5 :].any()
    assert not changed[[0, 1, 3]].any()
    # everything but the placeholder rows is the plain embedding of the ids
    bare, none, plain = prompt_embeddings(model, images, questions, [None] * 4, fused)  # no refs: no record, the ids' rows
    assert none is None and torch.equal(plain, model._embed(torch.tensor(bare, dtype=torch.int32)))
    ids = torch.tensor(prompts)
    is_ref = ((ids == tk.coord_id) | (ids == tk.size_id)).cuda()
    plain_ids = model._embed(ids.to(torch.int32))
    assert torch.equal(x[~is_ref], plain_ids[~is_ref]) and not torch.equal(x[is_ref], plain_ids[is_ref])


def batched_prompt_rows(model, images, questions, row_refs, fused):
    """Row i's prompt embedding rows [T_i, D], in the caller's order, as a batched call makes them: the rows in the
    plan's slot order (stable by total prompt length), the record reordered with them, one ``embed`` per length group."""
    prompts, rec = model._query_prompts_spatial(images, questions, row_refs)
    plan = plan_rows(list(images), [len(p) for p in prompts], False)
    assert len(plan.groups) > 2  # several lengths: several passes over slices of ONE table
    out = [None] * len(prompts)
    with torch.inference_mode():
        embed = model._sequence_embeddings([prompts[i] for i in plan.order], [images[i] for i in plan.order] if fused else None,
                                           spatial=rec.reorder(plan.order))
        for r0, r1 in plan.groups:
            x = embed(r0, r1)
            for j in range(r0, r1):
                i = plan.order[j]
                out[i] = x[j - r0, x.shape[1] - len(prompts[i]) :].clone()
    torch.cuda.synchronize()
    return prompts, out


@pytest.mark.parametrize("fused", [False, True], ids=["prompt", "fused"])
def test_every_layout_of_refs_is_within_the_bound_of_the_single_path(tiny, fused):
    """The eight rows of the row-independence test -- none, a point, a box, point + box, two boxes, the golden pair, an
    empty list, box / point / box -- in ONE batched preparation: every placeholder row against ``encode_spatial_refs`` of
    the row's refs.  The single path's row and the batched row are two roundings of the same contraction of the same
    bf16 features and weights (md_gemm_bf16's order, the row kernel's order), so EACH must lie within the kernel test's
    per-element bound of the float64 contraction -- which holds them within twice the bound of each other; asserting
    |batched - single| <= one bound would refuse two correct results that round to different sides.  Positions and value
    tensors are derived from each row's refs with the reference's arithmetic (region.py:96-136)."""
    g, cfg, model, img, refs, q = tiny
    tk = cfg.tokenizer
    head = len(tk.templates["query"]["prefix"])
    images, questions, row_refs = eight_rows(tiny)
    prompts, rows = batched_prompt_rows(model, images, questions, row_refs, fused)
    r, _ = model._region()
    checked = 0
    for i, row in enumerate(row_refs):
        ids = torch.tensor(prompts[i], dtype=torch.int32)
        plain = model._embed(ids.unsqueeze(0))[0]
        if not row:
            assert torch.equal(rows[i], plain), i  # a ref-less row: the embedding of its ids
            continue
        coords, sizes, c_at, s_at, pos = [], [], [], [], head
        for ref in row:
            if len(ref) == 2:
                coords += [ref[0], ref[1]]
            else:
                coords += [(ref[0] + ref[2]) / 2, (ref[1] + ref[3]) / 2]
                sizes.append([ref[2] - ref[0], ref[3] - ref[1]])
            c_at += [pos, pos + 1]
            pos += 2
            if len(ref) == 4:
                s_at.append(pos)
                pos += 1
        assert [prompts[i][p] for p in c_at] == [tk.coord_id] * len(c_at) and [prompts[i][p] for p in s_at] == [tk.size_id] * len(s_at)
        other = torch.ones(len(prompts[i]), dtype=torch.bool)
        other[c_at + s_at] = False
        assert torch.equal(rows[i][other.cuda()], plain[other.cuda()]), i  # nothing but the placeholder rows differs
        single = model.encode_spatial_refs(row)
        assert (single["sizes"] is None) == (not sizes)
        parts = [(c_at, single["coords"], torch.tensor(coords, dtype=BF16).view(-1, 1), "coord_features", "coord_encoder")]
        if sizes:
            parts.append((s_at, single["sizes"], torch.tensor(sizes, dtype=BF16), "size_features", "size_encoder"))
        for at, one, vals, fw, lin in parts:
            with torch.inference_mode():
                feats = model._fourier(vals, r[fw])
            w, bias = r[lin].w[: r[lin].n, : r[lin].k], r[lin].b[: r[lin].n]
            got = rows[i][torch.tensor(at, device="cuda")]
            assert got.shape == one.shape
            for name, x in (("batched", got), ("single", one)):
                ex = elementwise_excess(x, feats, w, bias, rounded=True)
                live = ex[ex != 0]  # (an all-zero encoder row has error 0 and bound 0)
                print(f"row {i} {lin} {name}: worst excess {float(ex.max()):.3e}, {float(live.max()) if live.numel() else 0.0:.3e} "
                      f"among the {live.numel()} of {ex.numel()} elements with a non-zero bound (<= 0 passes)")
                assert float(ex.max()) <= 0, (name, i, lin, float(ex.max()))
            checked += len(at)
    assert checked == sum(2 * len(row) + sum(len(ref) == 4 for ref in row) for row in row_refs if row) == 2 + 3 + 5 + 6 + 5 + 8


def test_reasoning_with_refs(tiny):
    g, cfg, model, img, refs, q = tiny
    st = {"temperature": 0, "max_tokens": 6}
    one = model.query(img, q, reasoning=True, spatial_refs=refs, settings=st)
    model.set_strict_batch_invariance(True)
    try:
        b1 = model.batch_query([img], [q], settings=st, reasoning=True, spatial_refs=[refs])
        b4 = model.batch_query([img, image(g, 1), img, img], [q, q, q + " 14", q], settings=st, reasoning=True,
                               spatial_refs=[refs, [(0.5, 0.5)], None, refs])
        many = model.query_many_reasoning(img, [q, q], settings=st, spatial_refs=[refs, None])
        lone2 = model.batch_query([img], [q + " 14"], settings=st, reasoning=True)[0]
    finally:
        model.set_strict_batch_invariance(False)
    assert set(b1[0]) == set(one) == {"reasoning", "answer"} and set(b1[0]["reasoning"]) == set(one["reasoning"])
    assert isinstance(b1[0]["answer"], str) and isinstance(b1[0]["reasoning"]["grounding"], list)
    assert b4[0] == b1[0] and b4[3] == b1[0] and many[0] == b1[0]
    assert b4[2] == lone2


def test_what_is_not_served_raises_before_any_launch(tiny):
    g, cfg, model, img, refs, q = tiny
    launches = []

    class Spy:  # every entry point of the library goes through ``model.lib``
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            launches.append(name)
            return getattr(self._lib, name)

    orig, lib, encode = model._sequence_embeddings, model.lib, model.encode_image
    model._sequence_embeddings = lambda *a, **k: launches.append("embed") or orig(*a, **k)
    model.encode_image = lambda *a, **k: launches.append("encode_image") or encode(*a, **k)
    model.lib = Spy(lib)
    try:
        for call in (lambda: model.batch_query([img], [q], settings={"num_beams": 2}, spatial_refs=[refs]),
                     lambda: model.query_many(img, [q], settings={"num_beams": 2, "spatial_refs": [refs]}),
                     lambda: model.score_ids([img], [[1, 2]], [[5]], spatial_refs=[refs]),
                     lambda: model.query_choices(img, q, ["5"], spatial_refs=[refs]),
                     lambda: model.batch_generate_ids_pipelined([([img], [[1, 2]])], spatial_refs=[refs]),
                     lambda: model.batch_query([img], [q], spatial_refs=[refs, refs]),
                     lambda: model.batch_query([img], [f"{cfg.tokenizer.coord_id} 12"], spatial_refs=[refs])):
            with pytest.raises(ValueError):
                call()
    finally:
        del model._sequence_embeddings, model.encode_image
        model.lib = lib
    assert not launches
