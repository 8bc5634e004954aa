"""The ``Scores`` record (moondream_amd/scores.py) on CPU tensors, where ``.cpu()`` is the identity: its planes are views
into one word allocation, an index yields views at the addresses hand slicing gives, ``chunk_fields`` hands the very plane
tensors to ``DecodeChunk``, and ``to_host`` carries every bit -- NaN payloads, -0.0 and denormals included."""
import math
import struct

import numpy as np
import pytest
import torch

from moondream_amd.scores import HostScores, Scores

# fp32 words a value conversion would damage: a NaN with a non-default payload, -0.0, the smallest denormal, and two plain ones
ODD_WORDS = [0x7FC12345, -(1 << 31), 1, 0x3F800000, -0x40800000]  # as int32


def fill_distinct(scores, seed):
    """Distinct words in every plane (the odd fp32 words first in the float planes); returns the planes as int32 words."""
    rng = np.random.default_rng(seed)
    out = []
    for plane in scores._planes():
        words = rng.integers(-(1 << 31), 1 << 31, size=plane.numel(), dtype=np.int64).astype(np.int32)
        if plane.dtype == torch.float32:
            words[: len(ODD_WORDS)] = ODD_WORDS[: words.size]
        plane.view(torch.int32).copy_(torch.from_numpy(words).view(plane.shape))
        out.append(words.reshape(tuple(plane.shape)))
    return out


@pytest.mark.parametrize("k", [0, 3])
def test_new_is_one_allocation_and_fill_marks_every_plane_unreached(k):
    s = Scores.new((4, 2), k, "cpu", fill=True)
    assert s.k == k and s.words.dtype == torch.int32 and s.words.numel() == 8 * (2 + 2 * k)
    assert s.logprob.dtype == torch.float32 and s.logprob.shape == (4, 2) and bool(torch.isnan(s.logprob).all())
    assert s.rank.dtype == torch.int32 and s.rank.shape == (4, 2) and bool((s.rank == -1).all())
    base = s.words.data_ptr()
    assert (s.logprob.data_ptr(), s.rank.data_ptr()) == (base, base + 4 * 8)
    if not k:
        assert s.top_ids is None and s.top_logprobs is None
        return
    assert s.top_ids.dtype == torch.int32 and s.top_ids.shape == (4, 2, k) and bool((s.top_ids == -1).all())
    assert s.top_logprobs.dtype == torch.float32 and s.top_logprobs.shape == (4, 2, k) and bool(torch.isnan(s.top_logprobs).all())
    assert (s.top_ids.data_ptr(), s.top_logprobs.data_ptr()) == (base + 4 * 16, base + 4 * (16 + 8 * k))
    # the fill is what torch.full writes: the default NaN
    assert s.logprob.view(torch.int32).unique().tolist() == [0x7FC00000] == s.top_logprobs.view(torch.int32).unique().tolist()


def test_an_index_yields_views_at_the_addresses_of_hand_slicing():
    s = Scores.new((4, 3), 2, "cpu", fill=True)
    row = s[1:][0]
    row.logprob.fill_(-0.5)
    row.rank.fill_(7)
    row.top_ids.copy_(torch.arange(6, dtype=torch.int32).view(3, 2))
    row.top_logprobs.fill_(-2.0)
    assert s.logprob[1].tolist() == [-0.5] * 3 and s.rank[1].tolist() == [7] * 3
    assert s.top_ids[1].tolist() == [[0, 1], [2, 3], [4, 5]] and s.top_logprobs[1].tolist() == [[-2.0] * 2] * 3
    for r in (0, 2, 3):  # the other rows keep their fill
        assert bool(torch.isnan(s.logprob[r]).all()) and bool((s.top_ids[r] == -1).all())
    part = s[2:4]
    for mine, plane in zip(part._planes(), s._planes()):
        by_hand = plane[2:4]
        assert (mine.data_ptr(), mine.shape, mine.stride()) == (by_hand.data_ptr(), by_hand.shape, by_hand.stride())
    assert part.k == 2 and part.words is None and s[:4].words is s.words and s[0].logprob.shape == (3,)


@pytest.mark.parametrize("k", [0, 2])
def test_chunk_fields_are_the_very_planes(k):
    s = Scores.new((5, 3), k, "cpu")[2:]
    f = s.chunk_fields()
    assert sorted(f) == ["logprobs", "topk"]
    same = lambda a, b: (a.data_ptr(), a.shape, a.stride(), a.dtype) == (b.data_ptr(), b.shape, b.stride(), b.dtype)
    assert same(f["logprobs"][0], s.logprob) and same(f["logprobs"][1], s.rank)
    if k:
        assert same(f["topk"][0], s.top_ids) and same(f["topk"][1], s.top_logprobs)
    else:
        assert f["topk"] is None


def test_copy_copies_every_plane_into_a_slice():
    src = Scores.new((2, 3), 2, "cpu")
    want = fill_distinct(src, 1)
    dst = Scores.new((4, 3), 2, "cpu", fill=True)
    dst[1:3].copy_(src)
    for plane, words in zip(dst._planes(), want):
        assert np.array_equal(plane.view(torch.int32)[1:3].numpy(), words)
    assert bool(torch.isnan(dst.logprob[0]).all()) and bool((dst.rank[3] == -1).all())  # rows outside the slice: untouched


@pytest.mark.parametrize("k", [0, 1, 32])
@pytest.mark.parametrize("shape", [(1,), (1, 1), (3, 2)])
@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("sliced", [False, True])
def test_to_host_round_trips_bit_for_bit(k, shape, with_ids, sliced):
    full = Scores.new(shape, k, "cpu")
    want = fill_distinct(full, 7)
    s = full[:2] if sliced else full
    if sliced:
        want = [w[:2] for w in want]
        assert (s.words is None) == (shape[0] > 2)  # two of three rows: no longer the whole allocation
    ids = torch.arange(100, 100 + s.rank.numel(), dtype=torch.int32).view(s.rank.shape)
    host = s.to_host(*([ids] if with_ids else []))
    assert isinstance(host, HostScores)
    got = (host.logprob, host.rank) + ((host.top_ids, host.top_logprobs) if k else ())
    assert (host.top_ids is None and host.top_logprobs is None) or k
    for g, w, dtype in zip(got, want, (np.float32, np.int32, np.int32, np.float32)):
        assert g.dtype == dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.int32), w)  # as words: the NaN payload, -0.0 and the denormal survive
    if with_ids:
        assert len(host.extra) == 1 and host.extra[0].dtype == np.int32 and np.array_equal(host.extra[0], ids.numpy())
    else:
        assert host.extra == ()


def test_the_odd_words_are_what_they_claim():
    f = [struct.unpack("<f", struct.pack("<i", w))[0] for w in ODD_WORDS]
    assert math.isnan(f[0]) and ODD_WORDS[0] != 0x7FC00000
    assert f[1] == 0.0 and math.copysign(1.0, f[1]) == -1.0
    assert 0.0 < f[2] < 1.2e-38  # a denormal
    assert f[3:] == [1.0, -1.0]


def test_alternatives_are_python_pairs_in_rank_order():
    s = Scores.new((2, 2), 3, "cpu")
    s.top_ids.copy_(torch.arange(12, dtype=torch.int32).view(2, 2, 3))
    s.top_logprobs.copy_(-torch.arange(12, dtype=torch.float32).view(2, 2, 3) / 4)
    host = s.to_host()
    pairs = host.alternatives((1, 0))
    assert pairs == [(6, -1.5), (7, -1.75), (8, -2.0)]
    assert all(type(t) is int and type(x) is float for t, x in pairs)
    assert s[1].to_host().alternatives(0) == pairs  # an int indexes a record over one leading dimension
    # an index that leaves a leading dimension: the decisions it covers, nested; none: an empty list
    assert host.alternatives((slice(2), 0)) == [host.alternatives((0, 0)), pairs] and host.alternatives((slice(0), 0)) == []
    assert host.alternatives(1) == [pairs, host.alternatives((1, 1))]
    one = HostScores(None, None, np.array([5, 9], dtype=np.int32), np.array([-0.25, -3.0], dtype=np.float32)).alternatives()
    assert one == [(5, -0.25), (9, -3.0)] and type(one[0][0]) is int and type(one[0][1]) is float
