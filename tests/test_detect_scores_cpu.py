"""Detection confidence without a GPU: the float64 restatement of md_region_pick_encode_scored (tests/detect_score_ref.py)
against torch and against the reference's own recorded region-head logits, the settings validation of every detect / point
call, and the new entry point's place in the header, the ctypes table and the library."""
import math
import os
import re

import numpy as np
import pytest
import torch

from detect_score_ref import bf16_bits_to_f64, boxes, coord_value, group_logprob, pick_bin, region_scores, window_bounds
from moondream_amd import _lib
from moondream_amd.config import get_config
from moondream_amd.decode_loop import check_score_settings
from test_logprobs_cpu import IMG, host_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def bits(t):
    return t.to(BF16).view(torch.int16).numpy().copy()


def random_rows(b, n, seed, scale=8.0):
    return (torch.randn(b, n, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n_bins", [1024, 1000])
def test_window_zero_is_the_log_softmax_of_the_pick(n_bins):
    lg = random_rows(4, 2 * n_bins, n_bins)
    got_bins, got = region_scores(bits(lg), 2, n_bins, 0)
    for g in range(2):
        x = lg[:, g * n_bins : (g + 1) * n_bins].double()
        want_bins = torch.argmax(x, dim=1)
        assert got_bins[:, g].tolist() == want_bins.tolist()
        want = torch.log_softmax(x, dim=1)[torch.arange(4), want_bins]
        assert np.abs(got[:, g] - want.numpy()).max() <= 1e-12


@pytest.mark.parametrize("n_bins", [1024, 1000])
def test_a_window_over_every_bin_gives_exactly_zero(n_bins):
    lg = random_rows(3, n_bins, 7)
    for window in (n_bins - 1, n_bins, 5 * n_bins):
        _, got = region_scores(bits(lg), 1, n_bins, window)
        assert got.tolist() == [[0.0]] * 3
    _, almost = region_scores(bits(lg), 1, n_bins, n_bins - 2)  # one bin short: a pick at either end leaves the other end out
    picks = [pick_bin(bf16_bits_to_f64(bits(lg))[r]) for r in range(3)]
    assert all((lp == 0.0) == (0 < p < n_bins - 1) for lp, p in zip(almost[:, 0], picks))


def test_the_window_is_clamped_at_both_ends():
    n = 16
    assert window_bounds(0, 3, n) == (0, 3) and window_bounds(15, 3, n) == (12, 15) and window_bounds(7, 0, n) == (7, 7)
    assert window_bounds(2, 5, n) == (0, 7) and window_bounds(13, 100, n) == (0, 15)
    x = np.zeros(n)
    x[0] = 1.0  # the pick at bin 0: a window of 2 holds bins 0, 1, 2
    s = math.e + 15
    assert group_logprob(x, 0, 2) == pytest.approx(math.log(math.e + 2) - math.log(s), abs=1e-14)
    x = np.zeros(n)
    x[n - 1] = 1.0
    assert pick_bin(x) == n - 1
    assert group_logprob(x, n - 1, 2) == pytest.approx(math.log(math.e + 2) - math.log(s), abs=1e-14)
    assert group_logprob(x, n - 1, 0) == pytest.approx(1.0 - math.log(s), abs=1e-14)


def test_ties_go_to_the_lowest_bin_and_nan_is_never_picked():
    x = np.array([1.0, 3.0, 3.0, 0.0, 3.0])
    assert pick_bin(x) == 1
    assert group_logprob(x, 1, 0) == pytest.approx(-math.log(3 + math.exp(-2) + math.exp(-3)), abs=1e-14)
    assert group_logprob(x, 1, 1) == pytest.approx(math.log(2 + math.exp(-2)) - math.log(3 + math.exp(-2) + math.exp(-3)), abs=1e-14)
    assert pick_bin(np.full(8, 2.5)) == 0 and group_logprob(np.full(8, 2.5), 0, 0) == pytest.approx(-math.log(8), abs=1e-14)
    y = np.array([np.nan, 1.0, 2.0])
    assert pick_bin(y) == 2 and math.isnan(group_logprob(y, 2, 0))
    assert pick_bin(np.full(4, np.nan)) == 0 and math.isnan(group_logprob(np.full(4, np.nan), 0, 0))


def test_minus_infinity_bins_add_nothing():
    x = np.array([-np.inf, 0.0, 1.0, -np.inf, 0.0])
    assert pick_bin(x) == 2
    assert group_logprob(x, 2, 0) == pytest.approx(-math.log(1 + 2 * math.exp(-1)), abs=1e-14)
    assert group_logprob(x, 2, 1) == pytest.approx(math.log(1 + math.exp(-1)) - math.log(1 + 2 * math.exp(-1)), abs=1e-14)
    lg = torch.tensor([[float("-inf"), 0.0, 1.0, float("-inf"), 0.0]])
    b, lp = region_scores(bits(lg), 1, 5, 0)
    assert b.tolist() == [[2]] and lp[0, 0] == group_logprob(x, 2, 0)


@pytest.mark.parametrize("case", ["detect0", "detect1", "point0", "point1"])
def test_the_references_own_logits_give_its_objects(golden_dir, case):
    """The restatement on the logits the reference recorded: its bins, through the reference's bin -> value rules, are the
    golden objects, and every log-probability is finite and <= 0, wider windows never smaller."""
    g = np.load(os.path.join(golden_dir, "tiny_detect.npz"))
    n_bins = get_config(str(g["cfg"])).region.coord_out_dim
    cb, clp = region_scores(g[f"{case}.decode_coordinate.out"], 1, n_bins, 0)
    xb, yb = cb[0::2, 0], cb[1::2, 0]
    ref = g[f"{case}.objects"]
    planes = [clp]
    if case.startswith("detect"):
        sz = g[f"{case}.decode_size.out"]
        sb, slp = region_scores(sz, 2, sz.shape[1] // 2, 0)
        planes.append(slp)
        assert boxes(xb, yb, sb[:, 0], sb[:, 1], n_bins) == ref.tolist()
        wide = region_scores(sz, 2, sz.shape[1] // 2, 8)
        assert (wide[0] == sb).all() and (wide[1] >= slp).all() and (wide[1] <= 0).all()
    else:
        assert [list(p) for p in zip(coord_value(xb, n_bins), coord_value(yb, n_bins))] == ref.tolist()
    for lp in planes:
        assert np.isfinite(lp).all() and (lp <= 0).all()
    wide = region_scores(g[f"{case}.decode_coordinate.out"], 1, n_bins, 8)
    assert (wide[0] == cb).all() and (wide[1] >= clp).all() and (wide[1] <= 0).all()


# ------------------------------------------------------------------ settings
N_BINS = get_config("tiny").region.coord_out_dim
BAD = [
    {"return_scores": 1}, {"return_scores": "yes"}, {"return_scores": None}, {"return_scores": np.bool_(True)},
    {"return_scores": True, "score_window": -1}, {"return_scores": True, "score_window": N_BINS},
    {"return_scores": True, "score_window": 1.0}, {"return_scores": True, "score_window": "2"},
    {"return_scores": True, "score_window": True}, {"return_scores": True, "score_window": None},
    {"score_window": 0}, {"score_window": 4}, {"return_scores": False, "score_window": 2},
]


def test_check_score_settings():
    assert check_score_settings(None, N_BINS) is None and check_score_settings({}, N_BINS) is None
    assert check_score_settings({"return_scores": False}, N_BINS) is None
    assert check_score_settings({"return_scores": True}, N_BINS) == 0
    assert check_score_settings({"return_scores": True, "score_window": 0}, N_BINS) == 0
    assert check_score_settings({"return_scores": True, "score_window": np.int64(8)}, N_BINS) == 8
    assert check_score_settings({"return_scores": True, "score_window": N_BINS - 1}, N_BINS) == N_BINS - 1
    for bad in BAD:
        with pytest.raises(ValueError):
            check_score_settings(bad, N_BINS)


def test_value_errors_precede_any_device_work():
    m = host_model()  # any device work raises AttributeError
    calls = [lambda st: m.detect(IMG, "cat", st), lambda st: m.point(IMG, "cat", st),
             lambda st: m.batch_detect([IMG], ["cat"], st), lambda st: m.batch_point([IMG], ["cat"], st),
             lambda st: m.detect_many(IMG, ["cat"], st), lambda st: m.point_many(IMG, ["cat"], st),
             lambda st: next(m.batch_detect_pipelined([([IMG], ["cat"])], st)),
             lambda st: next(m.batch_detect_pipelined([([IMG], ["cat"])], st, kind="point"))]
    for bad in BAD:
        for call in calls:
            with pytest.raises(ValueError, match="return_scores|score_window"):
                call(bad)
    with pytest.raises(AttributeError):  # a good value passes the host checks and reaches the device
        m.detect(IMG, "cat", {"return_scores": True, "score_window": 8})


# ------------------------------------------------------------------ the entry point
def test_the_new_symbol_is_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "moondream_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bmd_region_pick_encode_scored\s*\((.*?)\)\s*;", text, flags=re.S)
    plain = re.search(r"\bmd_region_pick_encode\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m and plain
    params = [p.strip() for p in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES["md_region_pick_encode_scored"]
    assert len(params) == len(argtypes) == len(_lib.SIGNATURES["md_region_pick_encode"][1]) + 3 == 16
    assert [p.split()[-1].lstrip("*") for p in params[-4:]] == ["window", "logprobs", "ld_logprobs", "stream"]
    assert params[:12] == [p.strip() for p in plain.group(1).split(",")][:12]  # md_region_pick_encode's arguments first
    assert re.search(r"#define\s+MD_ABI_VERSION\s+5\b", text) and _lib.ABI_VERSION == 5
    _lib.build_library(verbose=False)
    assert hasattr(_lib.load(), "md_region_pick_encode_scored")


def test_entry_point_rejects_bad_arguments_without_a_device():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.int32).ctypes.data  # a non-NULL address: nothing is launched, nothing reads it
    good = dict(logits=buf, ld=2048, batch=1, n_groups=2, n_bins=1024, table=buf, fw=buf, half=64, bins=buf, ld_bins=2, feats=buf,
                ld_feats=128, window=0, logprobs=buf, ld_logprobs=2)
    call = lambda **kw: lib.md_region_pick_encode_scored(*{**good, **kw}.values(), None)
    for bad in (dict(window=-1), dict(window=-(2 ** 31)), dict(logprobs=None), dict(ld_logprobs=1), dict(logits=None), dict(bins=None),
                dict(feats=None), dict(table=None), dict(fw=None), dict(batch=0), dict(n_bins=0), dict(n_groups=3), dict(ld=2047),
                dict(ld_bins=1), dict(ld_feats=127)):
        assert call(**bad) == 1, bad  # MD_ERR_INVALID_ARG
