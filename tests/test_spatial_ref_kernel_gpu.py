"""md_spatial_ref_embed alone, no model: weights drawn here, passed as raw pointers.

  * features exact: with an identity encoder and a zero bias the stored rows ARE md_fourier_features' rows, bit for bit;
  * the encoder per element: against a float64 contraction of the same bf16 features and weights, every element within
    half a bf16 spacing of the result plus (K + 1) * 2^-23 * (sum_k |feat[k] * W[n][k]| + |bias[n]|) -- util.compare_elementwise's
    derived bound (each of the K fp32 accumulation steps and the bias add charged 2^-23 of the running magnitude, in any
    order; one rounding to bf16), at the tiny dimensions and at 2B's;
  * invariance: a token's row does not depend on the table's length, its index in it, or its destination;
  * scatter: rows and padding columns no descriptor names keep a canary, bit for bit; bad arguments are refused on the host.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from moondream_amd import _lib
from util import compare_elementwise

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
COORD, SIZE = 0, 1
CANARY = 0x7FC1  # int16 view of a NaN pattern no computation produces


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def draw_weights(dim, cf=256, sf=512, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF16).cuda()
    return {"cfw": r(1, cf // 2, scale=10.0), "cw": r(dim, cf, scale=cf ** -0.5), "cb": r(dim, scale=0.1),
            "sfw": r(2, sf // 2, scale=10.0), "sw": r(dim, sf, scale=sf ** -0.5), "sb": r(dim, scale=0.1)}


def draw_tokens(n, seed=1):
    """(kind [n], values bf16 [n, 2]) with both kinds mixed; values in (0.05, 0.95): away from 0, where a feature can be
    -0.0 and a sum of products +0.0."""
    g = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, 2, (n,), generator=g)
    vals = (0.05 + 0.9 * torch.rand(n, 2, generator=g)).to(BF16)
    return kind, vals


def table(kind, vals, dst):
    bits = vals.view(torch.int16).to(torch.int32) & 0xFFFF
    t = torch.stack([torch.as_tensor(dst, dtype=torch.int32), kind.to(torch.int32), bits[:, 0],
                     torch.where(kind == SIZE, bits[:, 1], torch.zeros_like(bits[:, 1]))], dim=1)
    return t.contiguous().cuda()


def launch(desc, w, emb, dst0=0, over=None):
    dim = w["cw"].shape[0]
    a = dict(desc=desc.data_ptr(), n=desc.shape[0], cfw=w["cfw"].data_ptr(), cf=w["cw"].shape[1],
             cw=w["cw"].data_ptr(), cld=w["cw"].stride(0), cb=w["cb"].data_ptr(), sfw=w["sfw"].data_ptr(), sf=w["sw"].shape[1],
             sw=w["sw"].data_ptr(), sld=w["sw"].stride(0), sb=w["sb"].data_ptr(), dim=dim, emb=emb.data_ptr(), ld=emb.stride(0),
             dst0=dst0, rows=emb.shape[0])
    a.update(over or {})
    return _lib.load().md_spatial_ref_embed(a["desc"], a["n"], a["cfw"], a["cf"], a["cw"], a["cld"], a["cb"], a["sfw"], a["sf"],
                                            a["sw"], a["sld"], a["sb"], a["dim"], a["emb"], a["ld"], a["dst0"], a["rows"], stream())


def embed(kind, vals, w, dst=None, rows=None, ld=None):
    """The kernel's rows for the tokens, in table order."""
    n, dim = len(kind), w["cw"].shape[0]
    dst = list(range(n)) if dst is None else list(dst)
    emb = torch.full((rows or n, ld or dim), CANARY, dtype=torch.int16, device="cuda").view(BF16)
    assert launch(table(kind, vals, dst), w, emb) == 0
    torch.cuda.synchronize()
    return emb[torch.tensor(dst, device="cuda"), :dim]


def fourier(vals, fw):
    """md_fourier_features of bf16 values [n, in_dim]."""
    x = vals.cuda().contiguous()
    half = fw.shape[1]
    out = torch.empty(x.shape[0], 2 * half, dtype=BF16, device="cuda")
    assert _lib.load().md_fourier_features(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], fw.data_ptr(), half, out.data_ptr(),
                                           out.stride(0), stream()) == 0
    return out


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("which", [COORD, SIZE])
def test_identity_encoder_stores_the_fourier_features_bit_for_bit(which):
    feat = 256 if which == COORD else 512
    w = draw_weights(feat)  # dim == this kind's feature width
    w["cw" if which == COORD else "sw"] = torch.eye(feat, dtype=BF16, device="cuda")
    w["cb" if which == COORD else "sb"] = torch.zeros(feat, dtype=BF16, device="cuda")
    kind, vals = draw_tokens(37)
    got = embed(kind, vals, w)
    mine = (kind == which).cuda()
    want = fourier(vals[:, : which + 1], w["cfw" if which == COORD else "sfw"])
    assert int(mine.sum()) > 4 and int((~mine).sum()) > 4
    assert torch.equal(bits(got[mine]), bits(want[mine]))


@pytest.mark.parametrize("dim", [256, 2048], ids=["tiny", "2b"])
def test_encoder_rows_are_within_the_per_element_bound(dim):
    w = draw_weights(dim, seed=dim)
    kind, vals = draw_tokens(37, seed=3)
    got = embed(kind, vals, w)
    for which, fw, ew, eb in ((COORD, "cfw", "cw", "cb"), (SIZE, "sfw", "sw", "sb")):
        mine = (kind == which).cuda()
        feats = fourier(vals[:, : which + 1], w[fw])[mine]
        compare_elementwise(f"spatial_ref_embed dim {dim} kind {which}", got[mine], feats, w[ew], w[eb], rounded=True)


def test_a_tokens_row_depends_on_nothing_but_its_values():
    w = draw_weights(256, seed=7)
    kind, vals = draw_tokens(193, seed=5)
    probes = {COORD: torch.tensor([[0.3125, 0.0]]).to(BF16), SIZE: torch.tensor([[0.171875, 0.71875]]).to(BF16)}
    for which, pv in probes.items():
        alone = embed(torch.tensor([which]), pv, w)
        assert not torch.equal(bits(alone), torch.full_like(bits(alone), CANARY))
        for n in (1, 15, 16, 17, 193):
            for at in sorted({0, 15, 16, n - 1} & set(range(n))):
                k, v = kind[:n].clone(), vals[:n].clone()
                k[at], v[at] = which, pv[0]
                for dst in (list(range(n)), [3 * (n - 1 - i) + 2 for i in range(n)]):
                    got = embed(k, v, w, dst=dst, rows=3 * n + 2)
                    assert torch.equal(bits(got[at : at + 1]), bits(alone)), (which, n, at, dst[at])


def test_only_the_named_rows_are_written():
    dim, ld, rows, dst0 = 256, 256 + 8, 61, 1000
    w = draw_weights(dim, seed=9)
    kind, vals = draw_tokens(20, seed=11)
    dst = [dst0 + r for r in (60, 0, 7, 8, 30, 31, 33, 59, 2, 45, 12, 50, 13, 22, 5, 41)] + [dst0 - 1, dst0 + rows, 0, dst0 + 17]
    kind[19] = 2  # no such kind: nothing stored for it; the three before it point outside the tensor
    emb = torch.full((rows, ld), CANARY, dtype=torch.int16, device="cuda").view(BF16)
    guard = torch.full((2, rows, ld), CANARY, dtype=torch.int16, device="cuda")  # (allocated around it: the canary again)
    assert launch(table(kind, vals, dst), w, emb, dst0=dst0) == 0
    torch.cuda.synchronize()
    named = torch.zeros(rows, dtype=torch.bool, device="cuda")
    named[torch.tensor([d - dst0 for d in dst[:16]], device="cuda")] = True
    b = bits(emb)
    assert bool((b[~named] == CANARY).all()) and bool((b[:, dim:] == CANARY).all()) and bool((guard == CANARY).all())
    assert bool((b[named][:, :dim] != CANARY).all())
    want = embed(kind[:16], vals[:16], w)  # the same tokens, densely
    assert torch.equal(bits(emb[torch.tensor([d - dst0 for d in dst[:16]], device="cuda"), :dim]), bits(want))


def test_bad_arguments_are_refused_on_the_host():
    w = draw_weights(256)
    kind, vals = draw_tokens(4)
    desc = table(kind, vals, range(4))
    emb = torch.full((4, 256), CANARY, dtype=torch.int16, device="cuda").view(BF16)
    bad = [dict(desc=None), dict(emb=None), dict(cw=None), dict(sb=None), dict(cfw=None), dict(n=0), dict(n=-3), dict(rows=0),
           dict(dim=0), dict(dim=254), dict(ld=255), dict(ld=258), dict(cf=0), dict(cf=252), dict(sf=4096), dict(cld=128),
           dict(sld=514), dict(desc=desc.data_ptr() + 4), dict(emb=emb.data_ptr() + 2)]
    for over in bad:
        assert launch(desc, w, emb, over=over) == 1, over
    torch.cuda.synchronize()
    assert bool((bits(emb) == CANARY).all())
