"""Detection confidence on the MI355X, tiny model: ``settings={"return_scores": True}`` through every public detect / point
call.  Boxes and points are those of the unscored call (which tests/test_model_gpu.py pins to the reference); the coordinate
log-probabilities are compared with the float64 log-softmax of the reference's recorded region-head logits, the token
decisions with the CPU oracle's trace; then the equalities the project already promises for the boxes (batch == sequential,
one-image forms == batch over copies, pipelined == per batch), scores included."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from detect_score_ref import region_scores
from moondream_amd import synth
from moondream_amd.config import get_config
from test_logprobs_gpu import bound as token_bound
from test_region_scored_kernel_gpu import bound as region_bound
from util import leading_wide_objects

pytestmark = pytest.mark.gpu
CASES = ("detect0", "detect1", "point0", "point1")
LOGIT_TOL = 1.0  # twice the project's logit bound of 0.5 (tests/test_logprobs_gpu.py): one for the logit, one for the normaliser
BOX_KEYS = {"detect": ("x_min", "y_min", "x_max", "y_max"), "point": ("x", "y")}
LP_KEYS = {"detect": ("object", "x", "y", "w", "h"), "point": ("object", "x", "y")}


class Ctx:
    pass


def kind_of(case):
    return "detect" if case.startswith("detect") else "point"


def strip(res):
    """A scored result without what the feature adds: what the unscored call must return."""
    key = "objects" if "objects" in res else "points"
    return {key: [{k: v for k, v in o.items() if k not in ("logprobs", "score")} for o in res[key]]}


def lsm(logits, token):
    return float(torch.log_softmax(logits.double().reshape(-1), dim=0)[int(token)])


@pytest.fixture(scope="module")
def ctx(golden_dir):
    """The tiny model, the golden detect cases, and per case -- computed once -- the CPU oracle's decisions, the unscored
    call and the scored calls at windows 0 and 8."""
    from moondream_amd.moondream import IdTokenizer, MoondreamModel
    from oracle import moondream_oracle as O

    assert torch.cuda.is_available(), "GPU tests need a device"
    c = Ctx()
    c.g = g = np.load(os.path.join(golden_dir, "tiny_detect.npz"))
    c.g0 = np.load(os.path.join(golden_dir, "tiny_seed1.npz"))
    c.cfg = cfg = get_config("tiny")
    seed = int(g["seed"])
    c.model = MoondreamModel(cfg, synth.synthetic_state_dict(cfg, seed=seed, device="cuda"), device="cuda", tokenizer=IdTokenizer(),
                             max_batch=8)
    orc = O.Oracle(cfg, synth.synthetic_state_dict(cfg, seed=seed))
    c.obj = " ".join(str(t) for t in g["object_ids"].tolist())
    c.max_objects = int(g["max_objects"])
    c.arr, c.img, c.first_logits, c.trace, c.plain, c.scored, c.wide = {}, {}, {}, {}, {}, {}, {}
    for case in CASES:
        kind = kind_of(case)
        c.arr[case] = arr = synth.synthetic_image_array(int(g[f"{case}.image_index"]), seed, (378, 378))
        c.img[case] = Image.fromarray(arr, "RGB")
        # Oracle.detect_like with its prompt pass's logits kept: the decision that opens the first object
        tpl = cfg.tokenizer.templates[kind]
        pos, kv = orc.encode_image(np.stack([arr, arr]), (1, 1))
        logits, h, pos = orc.prefill_prompt(list(tpl["prefix"]) + g["object_ids"].tolist() + list(tpl["suffix"]), pos, kv)
        c.first_logits[case] = logits.clone()
        c.trace[case] = []
        orc.generate_points(h[-1:].clone(), int(torch.argmax(logits.float())), pos, kv, kind == "detect", c.max_objects, c.trace[case])
        fn = c.model.detect if kind == "detect" else c.model.point
        c.plain[case] = fn(c.img[case], c.obj, {"max_objects": c.max_objects})
        c.scored[case] = fn(c.img[case], c.obj, {"max_objects": c.max_objects, "return_scores": True})
        c.wide[case] = fn(c.img[case], c.obj, {"max_objects": c.max_objects, "return_scores": True, "score_window": 8})
    return c


def objects_of(res):
    return res["objects" if "objects" in res else "points"]


@pytest.mark.parametrize("case", CASES)
def test_scores_against_the_reference_logits_and_the_oracle(ctx, case):
    g, kind = ctx.g, kind_of(case)
    res, plain = ctx.scored[case], ctx.plain[case]
    assert set(plain) == {"objects" if kind == "detect" else "points"} and set(res) == set(plain) | {"stop_logprob"}
    assert strip(res) == plain
    objs = objects_of(res)
    n_ok = leading_wide_objects(g[f"{case}.margins"], 4.0)  # past a narrow decision two correct implementations may part ways
    assert n_ok >= 1 and len(objs) >= n_ok
    n_bins = ctx.cfg.region.coord_out_dim
    _, clp = region_scores(g[f"{case}.decode_coordinate.out"], 1, n_bins, 0)
    slp = None
    if kind == "detect":
        sz = g[f"{case}.decode_size.out"]
        _, slp = region_scores(sz, 2, sz.shape[1] // 2, 0)
    nexts = [lg for k, lg in ctx.trace[case] if k == "next"]
    nxt_tok = [int(torch.argmax(lg.float())) for lg in nexts]
    worst = 0.0
    for k, o in enumerate(objs):
        assert tuple(o)[: len(BOX_KEYS[kind])] == BOX_KEYS[kind] and tuple(o["logprobs"]) == LP_KEYS[kind]
        assert o["score"] == math.exp(math.fsum(o["logprobs"].values()))
        assert all(math.isfinite(v) and v <= 0.0 for v in o["logprobs"].values()) and 0.0 <= o["score"] <= 1.0
        if k >= n_ok:
            continue
        want = {"x": clp[2 * k, 0], "y": clp[2 * k + 1, 0]}
        if kind == "detect":
            want.update(w=slp[k, 0], h=slp[k, 1])
        if k == 0:
            want["object"] = lsm(ctx.first_logits[case], torch.argmax(ctx.first_logits[case].float()))
        else:
            want["object"] = lsm(nexts[k - 1], nxt_tok[k - 1])
        for name, ref in want.items():
            gap = abs(o["logprobs"][name] - float(ref))
            worst = max(worst, gap)
            assert gap <= LOGIT_TOL, (case, k, name, o["logprobs"][name], float(ref))
    print(f"{case}: worst |logprob - reference| over {n_ok} objects = {worst:.4f} (allowed {LOGIT_TOL})")
    # the golden lists are cut by max_objects (the reference's next token after the last object is no eos)
    eos = ctx.cfg.tokenizer.eos_id
    if len(objs) == ctx.max_objects and nxt_tok[ctx.max_objects - 1] != eos and n_ok == ctx.max_objects:
        assert res["stop_logprob"] is None
    fn = ctx.model.detect if kind == "detect" else ctx.model.point
    cut = fn(ctx.img[case], ctx.obj, {"max_objects": 1, "return_scores": True})
    assert cut["stop_logprob"] is None and objects_of(cut) == objs[:1]


@pytest.mark.parametrize("case", CASES)
def test_a_wider_window_changes_no_box_and_lowers_no_logprob(ctx, case):
    a, b = ctx.scored[case], ctx.wide[case]
    assert strip(a) == strip(b) == ctx.plain[case] and a["stop_logprob"] == b["stop_logprob"]
    for oa, ob in zip(objects_of(a), objects_of(b)):
        assert ob["logprobs"]["object"] == oa["logprobs"]["object"]
        for name in LP_KEYS[kind_of(case)][1:]:
            assert 0.0 >= ob["logprobs"][name] >= oa["logprobs"][name], (case, name, oa, ob)
        assert ob["score"] == math.exp(math.fsum(ob["logprobs"].values())) >= oa["score"]


@pytest.mark.parametrize("case", ["detect0", "point1"])
def test_stop_logprob_is_the_eos_decisions(ctx, case):
    """The tiny model never stops on its own inside the golden lists, so the pick of one decision is replaced by eos: after
    the second object, and at the prompt pass.  The log-probability reported is the model's own log P(eos) there."""
    m, kind = ctx.model, kind_of(case)
    eos = ctx.cfg.tokenizer.eos_id
    fn = m.detect if kind == "detect" else m.point
    nexts = [lg for k, lg in ctx.trace[case] if k == "next"]
    orig = m._pick
    for at, ref_logits, n_objects in ((2, nexts[1], 2), (0, ctx.first_logits[case], 0)):
        calls = [0]

        def pick(logits, *a, **k):
            calls[0] += 1
            out = orig(logits, *a, **k)
            return torch.full_like(out, eos) if calls[0] == at + 1 else out

        m._pick = pick
        try:
            res = fn(ctx.img[case], ctx.obj, {"max_objects": ctx.max_objects, "return_scores": True})
        finally:
            m._pick = orig
        objs = objects_of(res)
        assert len(objs) == n_objects and objs == objects_of(ctx.scored[case])[:n_objects]
        want = lsm(ref_logits, eos)
        print(f"{case}: eos forced at decision {at}: stop_logprob {res['stop_logprob']:.4f}, oracle {want:.4f}")
        assert res["stop_logprob"] is not None and abs(res["stop_logprob"] - want) <= LOGIT_TOL


def close(a, b, ctx):
    """Two scored result lists: equal boxes, stop decisions both present or both absent, every log-probability within the
    bound of the kernel that produced it.  Returns the worst |a - b| / bound."""
    worst = 0.0
    assert [strip(x) for x in a] == [strip(x) for x in b]
    n_bins, vocab = ctx.cfg.region.coord_out_dim, ctx.cfg.text.vocab_size
    for ra, rb in zip(a, b):
        pairs = [(ra["stop_logprob"], rb["stop_logprob"], token_bound(vocab, 0.0))]
        for oa, ob in zip(objects_of(ra), objects_of(rb)):
            for name in oa["logprobs"]:
                ref = oa["logprobs"][name]
                pairs.append((ref, ob["logprobs"][name], token_bound(vocab, ref) if name == "object" else region_bound(n_bins, ref)))
        for x, y, lim in pairs:
            assert (x is None) == (y is None)
            if x is not None:
                worst = max(worst, abs(x - y) / lim)
    return worst


def test_batches_equal_the_sequential_calls(ctx):
    """Mixed raw and EncodedImage inputs, ragged object prompts.  With set_strict_batch_invariance: bit for bit.  Without:
    the boxes are equal and the scores within the kernels' bounds."""
    m = ctx.model
    imgs = [ctx.img[c] for c in ("detect0", "detect1", "point0")]
    objects = ["7 8", "7 8 9 10", "5"]
    st = {"max_objects": 2, "return_scores": True, "score_window": 1}
    for strict in (True, False):
        m.set_strict_batch_invariance(strict)
        try:
            mixed = [imgs[0], m.encode_image(imgs[1]), imgs[2]]
            for batch, one in ((m.batch_detect, m.detect), (m.batch_point, m.point)):
                seq = [one(im, o, st) for im, o in zip(imgs, objects)]
                got = batch(mixed, objects, st)
                assert all(len(objects_of(r)) == 2 for r in got)
                if strict:
                    assert got == seq
                else:
                    worst = close(seq, got, ctx)
                    print(f"{batch.__name__} against sequential, default mode: worst |difference| / kernel bound = {worst:.3g}")
                    assert worst <= 1.0
        finally:
            m.set_strict_batch_invariance(False)


def test_one_image_forms_and_the_pipeline_equal_the_batch_calls(ctx):
    m = ctx.model
    img = ctx.img["detect0"]
    objects = ["7 8", "7 8 9 10", "5", "7 8"]
    st = {"max_objects": 2, "return_scores": True}
    enc = m.encode_image(img)
    many = m.detect_many(img, objects, st)
    assert many == m.batch_detect([enc] * len(objects), objects, st)
    assert many[0] == many[3] and all("stop_logprob" in r and "score" in r["objects"][0] for r in many)
    assert m.point_many(img, objects, st) == m.batch_point([enc] * len(objects), objects, st)
    imgs = [ctx.img[c] for c in ("detect0", "detect1", "point0")]
    batches = [(imgs[:2], ["7 8", "5"]), (imgs[2:], ["7 8 9 10"]), (imgs[:1], ["5"])]
    for kind, run in (("detect", m.batch_detect), ("point", m.batch_point)):
        assert list(m.batch_detect_pipelined(batches, st, kind=kind)) == [run(i, o, st) for i, o in batches]


def test_lora_variant_and_fp8_kv_are_served(ctx):
    m, g0 = ctx.model, ctx.g0
    img = ctx.img["detect1"]
    m.register_variant("scores-test", synth.synthetic_lora(ctx.cfg, seed=3, rank=8, device="cuda"))
    runs = [lambda st: m.detect(img, ctx.obj, st), lambda st: m.point(img, ctx.obj, st), lambda st: m.detect_many(img, [ctx.obj, "5"], st)]

    def check(extra):
        for run in runs:
            plain = run({"max_objects": 2, **extra})
            res = run({"max_objects": 2, "return_scores": True, **extra})
            pl, rs = (plain, res) if isinstance(plain, list) else ([plain], [res])
            assert [strip(r) for r in rs] == pl
            for r in rs:
                assert objects_of(r) and all(math.isfinite(o["score"]) and all(math.isfinite(v) for v in o["logprobs"].values())
                                             for o in objects_of(r))

    check({"variant": "scores-test"})
    images = [Image.fromarray(synth.synthetic_image_array(int(g0["image_index"][i]), int(g0["seed"]), tuple(g0[f"img{i}.cap.size"])), "RGB")
              for i in range(3)]
    m.enable_fp8(images, g0["img0.cap.prompt"].tolist(), kv_cache=True)
    try:
        assert m._kv8_scales is not None
        check({})
    finally:
        m.enable_fp8(on=False)


def test_without_the_setting_the_results_are_the_old_ones(ctx):
    m = ctx.model
    img = ctx.img["detect0"]
    for st in ({"max_objects": 2}, {"max_objects": 2, "return_scores": False}):
        d, p = m.detect(img, ctx.obj, st), m.point(img, ctx.obj, st)
        assert set(d) == {"objects"} and all(tuple(o) == BOX_KEYS["detect"] for o in d["objects"]) and d["objects"]
        assert set(p) == {"points"} and all(tuple(o) == BOX_KEYS["point"] for o in p["points"]) and p["points"]
    for r in m.detect_many(img, [ctx.obj, "5"], {"max_objects": 1}) + m.batch_detect([img], [ctx.obj], {"max_objects": 1}):
        assert set(r) == {"objects"} and all(tuple(o) == BOX_KEYS["detect"] for o in r["objects"])
    assert m.detect(img, ctx.obj, {"max_objects": 2}) == strip(m.detect(img, ctx.obj, {"max_objects": 2, "return_scores": True}))
