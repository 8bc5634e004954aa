"""The 65 .. 128-row decode path (MD_TILE_DECODE_TALL) at the widths that ship, on a real MI355X: tile 21 of md_gemm_bf16 (128 x 64
weight-streaming tile, in-launch split-K), the 128-row instantiations behind md_gemm_partial_f32 / md_gemm_partial_f32_pair, the
block tail over 65 .. 128 rows of those partials, the launch chain under graph replay and one model-level run at 0.5B widths.

Three instruments throughout:
  * the header's promise, bit for bit: a row gets the same bits in a launch of 65 .. 128 rows as in one of <= 64;
  * util.compare_elementwise: a derived per-element bound against float64 (an error of the size of a bias in one edge column
    does not hide in it, as it does in the aggregate util.compare);
  * guards: every result lives inside a larger buffer of sentinels (rows below, columns to the right, a tail behind the
    workspace / the partial slices) that must be intact afterwards, so a store outside the result is seen."""
import ctypes as C
import math

import pytest
import torch

from moondream_amd import _lib, synth
from moondream_amd.config import get_config
from moondream_amd.weights import PackedLinear, PackedLayerNorm
from util import compare, compare_elementwise

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
TALL = _lib.MD_TILE_DECODE_TALL
BIAS, GELU, RESIDUAL = _lib.MD_EPI_BIAS, _lib.MD_EPI_GELU, _lib.MD_EPI_RESIDUAL
ROWS = [65, 96, 97, 127, 128]  # 65: one row past the 64-row regime; 97: one row into the fourth compute wave's 32
TICKET_BYTES = 8192

# (k, n, epilogue, gelu_from, store_pad_cols)
LAYERS = {
    "2b-fused": (2048, 14336, GELU, 6144, 0),
    "05b-fused": (1024, 7168, GELU, 3072, 0),
    "tiny-fused": (256, 1472, GELU, 768, 0),
    "proj-residual": (2048, 2048, RESIDUAL, 0, 0),
    "fc2-residual-splitk": (8192, 2048, RESIDUAL, 0, 0),
    "fc2-bias-splitk": (8192, 2048, BIAS, 0, 0),
    "ragged-n": (1152, 1000, BIAS, 0, 1),
    "k704": (704, 256, BIAS, 0, 0),
    "k588": (588, 1152, BIAS, 0, 0),       # k_pad 640
    "lm-head": (2048, 51200, BIAS, 0, 0),  # >= 16384 columns: the by-shape config under the tall policy
}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def randn(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF16).cuda()


def pad_k(a, k_pad):
    out = torch.zeros(a.shape[0], k_pad, dtype=BF16, device="cuda")
    out[:, : a.shape[1]] = a
    return out


SENTINEL16 = 0x7FC1      # a bf16 NaN with a payload no kernel produces
SENTINEL32 = 0x7FC00123  # the same for fp32
SENTINEL8 = 0xA5


class GuardedOut:
    """An m x width bf16 result inside a (m + 64) x (width + 64) buffer of sentinels: ldc > width, 64 rows below row m - 1."""

    def __init__(self, m, width):
        self.m, self.width = m, width
        self.raw = torch.full((m + 64, width + 64), SENTINEL16, dtype=torch.int16, device="cuda")
        self.c = self.raw.view(BF16)[:m, :width]

    def intact(self):
        return bool((self.raw[self.m :] == SENTINEL16).all()) and bool((self.raw[: self.m, self.width :] == SENTINEL16).all())


class GuardedWorkspace:
    """Exactly md_gemm_workspace_bytes bytes, zeroed, with a sentinel tail behind them."""

    def __init__(self, need):
        self.need = need
        self.raw = torch.zeros(need + 4096, dtype=torch.uint8, device="cuda")
        self.raw[need:] = SENTINEL8

    def ptr(self):
        return self.raw.data_ptr() if self.need else None

    def intact(self):
        tickets_zero = bool((self.raw[: min(self.need, TICKET_BYTES)] == 0).all())
        return bool((self.raw[self.need :] == SENTINEL8).all()) and tickets_zero


class Launch:
    """One md_gemm_bf16 problem over guarded buffers; run() launches it (again) over the same buffers."""

    def __init__(self, lib, a, lin, *, epi, gelu_from=0, store_pad=0, r=None, in_place=False, use_ws=True, policy=TALL):
        self.lib, self.a, self.lin, self.m = lib, a, lin, a.shape[0]
        self.epi, self.gelu_from, self.store_pad, self.policy = epi, gelu_from, store_pad, policy
        self.out = GuardedOut(self.m, lin.n_pad if store_pad else lin.n)
        self.r, self.in_place = r, in_place
        st = lin.struct()
        # (the need is asked for under the tuning in force: it is part of what the A/B knobs change)
        self.ws = GuardedWorkspace(lib.md_gemm_workspace_bytes(C.byref(st), self.m, store_pad) if use_ws else 0)

    def run(self):
        c = self.out.c
        r, ldr = None, 0
        if self.epi == RESIDUAL:
            if self.in_place:
                c.copy_(self.r)
                r, ldr = c.data_ptr(), c.stride(0)
            else:
                r, ldr = self.r.data_ptr(), self.r.stride(0)
        args = _lib.MdGemmArgs(self.a.data_ptr(), self.a.stride(0), self.lin.struct(), c.data_ptr(), c.stride(0), r, ldr, 0, self.m,
                               self.epi, self.store_pad, self.gelu_from, self.ws.ptr(), self.ws.need, self.policy)
        status = self.lib.md_gemm_bf16(C.byref(args), stream())
        torch.cuda.synchronize()
        return status

    def result(self, what):
        """Launch, insist on MD_OK and intact guards, return a copy of the m x width result."""
        assert self.run() == 0, f"{what}: status"
        self.check_guards(what)
        return self.out.c.clone()

    def check_guards(self, what):
        assert self.out.intact(), f"{what}: a store outside the {self.m} x {self.out.width} result (sentinel rows / columns overwritten)"
        assert self.ws.intact(), f"{what}: the split-K workspace was overrun or its tickets were not left zero"


_LAYER = {}


def layer(name):
    """Operands of one layer, for 128 rows (kept for the consecutive row counts of the same layer)."""
    if name not in _LAYER:
        _LAYER.clear()
        torch.cuda.empty_cache()
        k, n, epi, gelu_from, store_pad = LAYERS[name]
        seed = 7000 + 10 * list(LAYERS).index(name)
        a, w = randn(128, k, seed=seed), randn(n, k, scale=1 / math.sqrt(k), seed=seed + 1)
        # (the per-element bound grows with sqrt(K): 0.06 at K = 8192, where a bias of scale 0.1 would sit inside it)
        b = randn(n, scale=0.5 if k >= 8192 else 0.1, seed=seed + 2)
        lin = PackedLinear(w, b, "cuda")
        _LAYER[name] = (a, w, b, lin, pad_k(a, lin.k_pad), randn(128, n, seed=seed + 3))
    return _LAYER[name]


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("name", list(LAYERS))
def test_tall_gemm_has_the_bits_of_two_64_row_launches_and_stays_inside_its_buffers(lib, name, m):
    """md_gemm_bf16 under MD_TILE_DECODE_TALL at 65 .. 128 rows.  Rows [0, 64) equal a launch of the first 64 rows and rows
    [64, m) a launch of the rest, bit for bit, with the split-K workspace and with splitk_ws = NULL on both sides; BIAS layers are
    held to the per-element bound against float64; every launch runs inside sentinels; four launches over the same buffers agree
    (race screen for the six-wave ring); the in-place residual equals the out-of-place one.

    decode_cfg A/B knob (17, 10, 3): a tall launch gives the bits it gives under 16, or a non-zero status.  The tall tile is 64
    columns wide whatever the knob says.  Until this test existed gemm_dispatch and md_gemm_workspace_bytes counted a tall
    launch's slices, tickets and slabs in decode_bn()-wide tiles -- 128 under decode_cfg = 3 -- while tile 21 indexes
    tile_id * slices * 8192 floats over ceil(n / 64) tiles: at (8192 -> 2048) the kernel would have touched 8 MiB of slabs in a
    4 MiB workspace that passed the size check (a real overrun, established from the code and never launched), and the slice
    count of the 2B fused layer became 2 instead of 1 (other bits).  Both now count in the 64-wide tiles that run; the launches
    below pin that: same bits as under 16 and an intact sentinel tail behind exactly md_gemm_workspace_bytes bytes."""
    k, n, epi, gelu_from, store_pad = LAYERS[name]
    a, w, b, lin, ap, res = layer(name)
    kw = dict(epi=epi, gelu_from=gelu_from, store_pad=store_pad)
    tag = f"{name} m={m}"
    by_ws = {}
    for use_ws in (True, False):
        r = lambda lo, hi: dict(r=res[lo:hi]) if epi == RESIDUAL else {}
        tall = Launch(lib, ap[:m], lin, use_ws=use_ws, **kw, **r(0, m))
        got = tall.result(f"{tag} ws={use_ws}")
        lo = Launch(lib, ap[:64], lin, use_ws=use_ws, **kw, **r(0, 64)).result(f"{tag} first 64 rows ws={use_ws}")
        hi = Launch(lib, ap[64:m], lin, use_ws=use_ws, **kw, **r(64, m)).result(f"{tag} rows 64.. ws={use_ws}")
        assert torch.equal(got[:64], lo), f"{tag} ws={use_ws}: rows [0, 64) differ from the 64-row launch in {(got[:64] != lo).sum().item()} elements"
        assert torch.equal(got[64:], hi), f"{tag} ws={use_ws}: rows [64, {m}) differ from the {m - 64}-row launch in {(got[64:] != hi).sum().item()} elements"
        if store_pad:
            assert bool((tall.out.raw[:m, n : lin.n_pad] == 0).all()), f"{tag}: pad columns [n, n_pad) are not exact zeros"
        if epi == BIAS:
            compare_elementwise(f"{tag} ws={use_ws}", got[:, :n], a[:m], w, b, rounded=True)
        else:
            ref = (a[:m].float() @ w.float().t() + b.float()).to(BF16).float()
            if epi == GELU:
                ref[:, gelu_from:] = torch.nn.functional.gelu(ref[:, gelu_from:], approximate="tanh")
            else:
                ref = ref + res[:m].float()
            compare(f"{tag} ws={use_ws}", got[:, :n], ref.to(BF16), 3e-3, 2e-2)
        for rep in range(4):
            assert tall.run() == 0
            tall.check_guards(f"{tag} ws={use_ws} rep {rep}")
            assert torch.equal(tall.out.c, got), f"{tag} ws={use_ws} rep {rep}: {(tall.out.c != got).sum().item()} elements differ"
        if epi == RESIDUAL:
            inp = Launch(lib, ap[:m], lin, use_ws=use_ws, in_place=True, **kw, **r(0, m)).result(f"{tag} in place ws={use_ws}")
            assert torch.equal(inp, got), f"{tag} ws={use_ws}: in-place residual differs"
        by_ws[use_ws] = got
    try:
        for cfg in (17, 10, 3):
            _lib.check(lib.md_gemm_set_tuning(b"decode_cfg", cfg))
            knob = Launch(lib, ap[:m], lin, **kw, **(dict(r=res[:m]) if epi == RESIDUAL else {}))
            status = knob.run()
            knob.check_guards(f"{tag} decode_cfg={cfg}")
            if status == 0:
                assert torch.equal(knob.out.c, by_ws[True]), f"{tag}: other bits under decode_cfg={cfg} than under 16"
    finally:
        lib.md_gemm_set_tuning(b"decode_cfg", 16)


# ---------------------------------------------------------------------------------------------- K-slice partials
class GuardedPartials:
    """slices x rows x dim fp32 partial products with gaps: ld_partial = dim + 16, slice_stride = (rows + 8) * ld_partial, and a
    tail behind the last slice -- all sentinels."""

    def __init__(self, slices, rows, dim):
        self.slices, self.rows, self.dim = slices, rows, dim
        self.ld = dim + 16
        self.stride = (rows + 8) * self.ld
        self.raw = torch.full((slices * self.stride + 4096,), SENTINEL32, dtype=torch.int32, device="cuda")
        self.p = self.raw[: slices * self.stride].view(torch.float32).view(slices, rows + 8, self.ld)

    def values(self, rows=None):
        return self.p[:, : (rows or self.rows), : self.dim].clone()

    def gaps_intact(self, rows=None):
        """everything but the [slices][rows][dim] block still holds the sentinel (rows=0: nothing was written at all)"""
        rows = self.rows if rows is None else rows
        probe = self.raw.clone()
        probe[: self.slices * self.stride].view(self.slices, self.rows + 8, self.ld)[:, :rows, : self.dim] = SENTINEL32
        return bool((probe == SENTINEL32).all())


def partial_single(lib, a, lin, rows, buf):
    st = lin.struct()
    return lib.md_gemm_partial_f32(a.data_ptr(), a.stride(0), C.byref(st), rows, buf.p.data_ptr(), buf.ld, buf.stride, stream())


def partial_pair(lib, a0, l0, b0, a1, l1, b1, rows):
    s0, s1 = l0.struct(), l1.struct()
    assert b0.ld == b1.ld and b0.stride == b1.stride
    return lib.md_gemm_partial_f32_pair(a0.data_ptr(), a0.stride(0), C.byref(s0), b0.p.data_ptr(), a1.data_ptr(), a1.stride(0), C.byref(s1),
                                        b1.p.data_ptr(), rows, b0.ld, b0.stride, stream())


_TAIL = {}


def tail_operands(dim, ka, kb):
    key = (dim, ka, kb)
    if key not in _TAIL:
        _TAIL.clear()
        a1, w1, b1 = randn(129, ka, seed=8070), randn(dim, ka, scale=1 / math.sqrt(ka), seed=8071), randn(dim, scale=0.1, seed=8072)
        a2, w2, b2 = randn(129, kb, seed=8073), randn(dim, kb, scale=1 / math.sqrt(kb), seed=8074), randn(dim, scale=0.1, seed=8075)
        la, lb = PackedLinear(w1, b1, "cuda"), PackedLinear(w2, b2, "cuda")
        _TAIL[key] = (a1, w1, b1, la, pad_k(a1, la.k_pad), a2, w2, b2, lb, pad_k(a2, lb.k_pad))
    return _TAIL[key]


TAIL_SHAPES = [(2048, 2048, 8192), (1024, 1024, 4096), (256, 256, 704)]


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("dim,ka,kb", TAIL_SHAPES)
def test_tall_partials_have_the_bits_of_two_64_row_launches_and_stay_inside_their_slices(lib, dim, ka, kb, m):
    """md_gemm_partial_f32 / _pair at 65 .. 128 rows (the 128 x 64 tile; the pair on its three-stage ring): md_gemm_partial_slices
    slices, each of whose rows [0, 64) and [64, m) equal the partials of the two <= 64-row launches bit for bit; pair == the two
    single launches; the slice sums (fp32, slice order) within the per-element fp32 bound against float64; nothing written into
    the gaps between rows, between slices or behind the last slice."""
    a1, w1, _, la, A1, a2, w2, _, lb, A2 = tail_operands(dim, ka, kb)
    sa, sb = la.struct(), lb.struct()
    na, nb = lib.md_gemm_partial_slices(C.byref(sa)), lib.md_gemm_partial_slices(C.byref(sb))
    assert 1 <= na <= 8 and 1 <= nb <= 8

    def singles(lo, hi):
        rows = hi - lo
        pa, pb = GuardedPartials(na, rows, dim), GuardedPartials(nb, rows, dim)
        assert partial_single(lib, A1[lo:hi], la, rows, pa) == 0 and partial_single(lib, A2[lo:hi], lb, rows, pb) == 0
        torch.cuda.synchronize()
        assert pa.gaps_intact() and pb.gaps_intact(), f"rows [{lo}, {hi}): a partial launch wrote outside its [slices][rows][dim] block"
        va, vb = pa.values(), pb.values()
        # (fewer slices written than md_gemm_partial_slices says would leave sentinels here, more would hit the tail)
        assert torch.isfinite(va).all() and torch.isfinite(vb).all(), f"rows [{lo}, {hi}): unwritten partials"
        return va, vb

    va, vb = singles(0, m)
    pa, pb = GuardedPartials(na, m, dim), GuardedPartials(nb, m, dim)
    for rep in range(4):
        assert partial_pair(lib, A1[:m], la, pa, A2[:m], lb, pb, m) == 0
        torch.cuda.synchronize()
        assert pa.gaps_intact() and pb.gaps_intact(), "the pair launch wrote outside its [slices][rows][dim] blocks"
        assert torch.equal(pa.values(), va) and torch.equal(pb.values(), vb), f"pair launch (rep {rep}) differs from the two single launches"
    lo_a, lo_b = singles(0, 64)
    hi_a, hi_b = singles(64, m)
    for s_ in range(na):
        assert torch.equal(va[s_, :64], lo_a[s_]) and torch.equal(va[s_, 64:], hi_a[s_]), f"layer a slice {s_}: other bits than the <= 64-row launches"
    for s_ in range(nb):
        assert torch.equal(vb[s_, :64], lo_b[s_]) and torch.equal(vb[s_, 64:], hi_b[s_]), f"layer b slice {s_}: other bits than the <= 64-row launches"
    for v, a, w, what in ((va, a1, w1, "a"), (vb, a2, w2, "b")):
        acc = torch.zeros_like(v[0])
        for s_ in range(v.shape[0]):
            acc = acc + v[s_]
        compare_elementwise(f"partial slice sums, layer {what} dim={dim} m={m}", acc, a[:m], w, None, rounded=False)


@pytest.mark.parametrize("dim,ka,kb", TAIL_SHAPES)
def test_partials_refuse_129_rows_and_write_nothing(lib, dim, ka, kb):
    _, _, _, la, A1, _, _, _, lb, A2 = tail_operands(dim, ka, kb)
    sa, sb = la.struct(), lb.struct()
    na, nb = lib.md_gemm_partial_slices(C.byref(sa)), lib.md_gemm_partial_slices(C.byref(sb))
    pa, pb = GuardedPartials(na, 129, dim), GuardedPartials(nb, 129, dim)   # (room for the rows, were they written)
    assert partial_single(lib, A1, la, 129, pa) == 1 and partial_single(lib, A2, lb, 129, pb) == 1  # MD_ERR_INVALID_ARG
    assert partial_pair(lib, A1, la, pa, A2, lb, pb, 129) == 1
    torch.cuda.synchronize()
    assert pa.gaps_intact(rows=0) and pb.gaps_intact(rows=0)


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("dim,ka,kb", TAIL_SHAPES)
def test_block_tail_over_tall_partials(lib, dim, ka, kb, m):
    """The partials of 65 .. 128 rows through md_reduce_residual_layernorm: x equals the exact model of the roundings
    (test_block_tail_partials_then_reduce_residual_layernorm's) bit for bit, y is the layer norm of it, rows [0, 64) of both
    are the bits of a 64-row call and rows [64, m) those of an (m - 64)-row call."""
    a1, w1, b1, la, A1, a2, w2, b2, lb, A2 = tail_operands(dim, ka, kb)
    x0 = randn(128, dim, seed=8076)
    lw, lbn = randn(dim, scale=0.1, seed=8077) + 1.0, randn(dim, scale=0.1, seed=8078)
    ln = PackedLayerNorm(lw, lbn, "cuda")
    sa, sb = la.struct(), lb.struct()
    na, nb = lib.md_gemm_partial_slices(C.byref(sa)), lib.md_gemm_partial_slices(C.byref(sb))

    def run(lo, hi):
        rows = hi - lo
        pa, pb = GuardedPartials(na, rows, dim), GuardedPartials(nb, rows, dim)
        _lib.check(partial_pair(lib, A1[lo:hi], la, pa, A2[lo:hi], lb, pb, rows))
        x = x0[lo:hi].clone()
        ld = (dim + 63) // 64 * 64
        y = torch.zeros(rows, ld, dtype=BF16, device="cuda")
        st = ln.struct()
        _lib.check(lib.md_reduce_residual_layernorm(x.data_ptr(), dim, pa.p.data_ptr(), na, la.b.data_ptr(), pb.p.data_ptr(), nb,
                                                    lb.b.data_ptr(), pa.ld, pa.stride, y.data_ptr(), ld, C.byref(st), rows, dim,
                                                    1e-5, stream()))
        torch.cuda.synchronize()
        assert pa.gaps_intact() and pb.gaps_intact()
        return x, y, pa.values(), pb.values()

    x, y, pa, pb = run(0, m)
    acc_a = torch.zeros_like(pa[0])
    for s_ in range(na):
        acc_a = acc_a + pa[s_]
    acc_b = torch.zeros_like(pb[0])
    for s_ in range(nb):
        acc_b = acc_b + pb[s_]
    t1 = (acc_a + b1.float()).to(BF16)
    x1 = (x0[:m].float() + t1.float()).to(BF16)
    t2 = (acc_b + b2.float()).to(BF16)
    x2 = (x1.float() + t2.float()).to(BF16)
    assert torch.equal(x, x2)
    ref = torch.nn.functional.layer_norm(x2.float(), (dim,), lw.float(), lbn.float(), 1e-5).to(BF16)
    compare(f"tall tail layernorm dim={dim} m={m}", y[:, :dim], ref, 2e-3, 1e-2)
    assert torch.count_nonzero(y[:, dim:]) == 0
    x64, y64, _, _ = run(0, 64)
    assert torch.equal(x[:64], x64) and torch.equal(y[:64], y64)
    xr, yr, _, _ = run(64, m)
    assert torch.equal(x[64:], xr) and torch.equal(y[64:], yr)


# ---------------------------------------------------------------------------------------------- graph replay
@pytest.mark.parametrize("m", [100, 128])
def test_tall_decode_block_chain_under_graph_replay(lib, m):
    """test_decode_block_chain_under_graph_replay at 65 .. 128 rows and 2B widths (dim 2048, ff 8192), two blocks: the fused
    [qkv | fc1] GEMM under the tall policy, proj + fc2 as one launch of 128-row K-slice partials (three-stage ring), the block
    tail.  The 2B fused layer has enough column tiles not to split K, so each block also launches fc2 as a tall BIAS GEMM with
    its in-launch split-K workspace (tickets) into a side buffer.  replay(A), replay(B), replay(A) ... equal the eager launches
    bit for bit."""
    dim, ff = 2048, 8192
    n_fused = 3 * dim + ff
    blocks = []
    for b in range(2):
        w_f, b_f = randn(n_fused, dim, scale=1 / math.sqrt(dim), seed=9900 + 10 * b), randn(n_fused, scale=0.1, seed=9901 + 10 * b)
        w_p, b_p = randn(dim, dim, scale=1 / math.sqrt(dim), seed=9902 + 10 * b), randn(dim, scale=0.1, seed=9903 + 10 * b)
        w_2, b_2 = randn(dim, ff, scale=1 / math.sqrt(ff), seed=9904 + 10 * b), randn(dim, scale=0.1, seed=9905 + 10 * b)
        lw, lb = randn(dim, scale=0.1, seed=9906 + 10 * b) + 1.0, randn(dim, scale=0.1, seed=9907 + 10 * b)
        blocks.append((PackedLinear(w_f, b_f, "cuda"), PackedLinear(w_p, b_p, "cuda"), PackedLinear(w_2, b_2, "cuda"), PackedLayerNorm(lw, lb, "cuda")))
    x = torch.zeros(m, dim, dtype=BF16, device="cuda")       # residual stream (updated in place by the tail)
    h = torch.zeros(m, dim, dtype=BF16, device="cuda")       # ln(x): the fused GEMM's operand, rewritten by the tail
    fused = torch.zeros(m, n_fused, dtype=BF16, device="cuda")
    side_out = torch.zeros(2, m, dim, dtype=BF16, device="cuda")  # the in-launch split-K GEMM of each block
    sf, s2 = blocks[0][0].struct(), blocks[0][2].struct()
    ws_f = GuardedWorkspace(lib.md_gemm_workspace_bytes(C.byref(sf), m, 0))
    ws_2 = GuardedWorkspace(lib.md_gemm_workspace_bytes(C.byref(s2), m, 0))
    assert ws_2.need > TICKET_BYTES, "the (8192 -> 2048) layer splits K inside the launch"
    sp = blocks[0][1].struct()
    na, nb = lib.md_gemm_partial_slices(C.byref(sp)), lib.md_gemm_partial_slices(C.byref(s2))
    pa = torch.zeros(na, m, dim, dtype=torch.float32, device="cuda")
    pb = torch.zeros(nb, m, dim, dtype=torch.float32, device="cuda")

    def chain():
        for i, (lf, lp, l2, ln) in enumerate(blocks):
            args = _lib.MdGemmArgs(h.data_ptr(), h.stride(0), lf.struct(), fused.data_ptr(), fused.stride(0), None, 0, 0, m, GELU, 0,
                                   3 * dim, ws_f.ptr(), ws_f.need, TALL)
            _lib.check(lib.md_gemm_bf16(C.byref(args), stream()), "fused gemm")
            act = fused[:, 3 * dim :]
            args = _lib.MdGemmArgs(act.data_ptr(), act.stride(0), l2.struct(), side_out[i].data_ptr(), side_out[i].stride(0), None, 0, 0, m,
                                   BIAS, 0, 0, ws_2.ptr(), ws_2.need, TALL)
            _lib.check(lib.md_gemm_bf16(C.byref(args), stream()), "split-K gemm")
            # (the "attention output" of this toy block is the q section of the fused row)
            spp, s22 = lp.struct(), l2.struct()
            _lib.check(lib.md_gemm_partial_f32_pair(fused.data_ptr(), fused.stride(0), C.byref(spp), pa.data_ptr(),
                                                    act.data_ptr(), fused.stride(0), C.byref(s22), pb.data_ptr(),
                                                    m, dim, m * dim, stream()))
            stn = ln.struct()
            _lib.check(lib.md_reduce_residual_layernorm(x.data_ptr(), dim, pa.data_ptr(), na, lp.b.data_ptr(), pb.data_ptr(), nb,
                                                        l2.b.data_ptr(), dim, m * dim, h.data_ptr(), dim, C.byref(stn), m, dim, 1e-5, stream()))

    inputs = {k: (randn(m, dim, seed=9950 + i), randn(m, dim, seed=9960 + i)) for i, k in enumerate("AB")}

    def load(k):
        x.copy_(inputs[k][0])
        h.copy_(inputs[k][1])

    eager = {}
    for k in "AB":
        load(k)
        chain()
        torch.cuda.synchronize()
        eager[k] = (x.clone(), h.clone(), fused.clone(), side_out.clone())
        assert all(bool(torch.isfinite(t.float()).all()) for t in eager[k])
    assert not torch.equal(eager["A"][0], eager["B"][0])
    assert ws_f.intact() and ws_2.intact()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        load("A")
        with torch.cuda.graph(g, stream=side):
            chain()
        for rep, k in enumerate("ABAAB"):
            load(k)
            g.replay()
            side.synchronize()
            for name, got, want in zip(("x", "ln(x)", "fused row", "split-K gemm"), (x, h, fused, side_out), eager[k]):
                assert torch.equal(got, want), f"replay {rep} ({k}): {name} differs from the eager launches of the same inputs"
    torch.cuda.current_stream().wait_stream(side)
    assert ws_f.intact() and ws_2.intact()
    # and the split-K launch computes what it claims (inputs B, block 1: whatever activations the chain produced)
    load("B")
    chain()
    torch.cuda.synchronize()
    l2 = blocks[1][2]
    compare_elementwise(f"chain split-K gemm m={m}", side_out[1], fused[:, 3 * dim :], l2.w[:dim, :ff], l2.b[:dim], rounded=True)


# ---------------------------------------------------------------------------------------------- model level, real widths
def test_decode_step_of_100_sequences_at_05b_widths_has_the_bits_of_64_plus_36():
    """test_decode_step_of_128_sequences_is_one_pass_with_the_bits_of_two_passes_of_64 at widths that ship (0.5B synthetic config:
    K = 1024 / 4096, fused N = 7168, lm_head 51200): 100 sequences in one tall pass give the ids of the same sequences decoded as
    64 + 36, and one step's logits and written K rows are bit-identical."""
    from moondream_amd.moondream import MoondreamModel, IdTokenizer

    cfg = get_config("0.5b")
    sd = synth.synthetic_state_dict(cfg, seed=1, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=128)
    pr = list(cfg.tokenizer.templates["caption"]["normal"])
    imgs = [synth.synthetic_image(i, 1) for i in range(100)]
    n = 4
    ref = model.batch_generate_ids(imgs[:64], [pr] * 64, max_tokens=n, ignore_eos=True)
    ref += model.batch_generate_ids(imgs[64:], [pr] * 36, max_tokens=n, ignore_eos=True)
    got = model.batch_generate_ids(imgs, [pr] * 100, max_tokens=n, ignore_eos=True)
    assert all(len(s) == n for s in got)
    assert got == ref, [i for i in range(100) if got[i] != ref[i]][:5]
    # logits and cache rows of one step: 100 rows at once vs 64 + 36
    p0 = 730 + len(pr)
    model.batch_generate_ids(imgs, [pr] * 100, max_tokens=2, ignore_eos=True)
    k100, lg100 = model._kv_k[:, :100, :, p0 : p0 + 2].clone(), model._decode_logits(100)[:100].clone()
    model.batch_generate_ids(imgs[:64], [pr] * 64, max_tokens=2, ignore_eos=True)
    k_a, lg_a = model._kv_k[:, :64, :, p0 : p0 + 2].clone(), model._decode_logits(64)[:64].clone()
    model.batch_generate_ids(imgs[64:], [pr] * 36, max_tokens=2, ignore_eos=True)
    k_b, lg_b = model._kv_k[:, :36, :, p0 : p0 + 2].clone(), model._decode_logits(36)[:36].clone()
    assert torch.isfinite(lg100.float()).all() and lg100.float().abs().max() > 0
    assert torch.equal(k100[:, :64], k_a) and torch.equal(k100[:, 64:], k_b)
    assert torch.equal(lg100[:64], lg_a) and torch.equal(lg100[64:], lg_b)
    del model
    torch.cuda.empty_cache()
