"""The attention kernels against an exact (float64) softmax attention, element by element, on inputs built so that ONE key
wrongly admitted or wrongly dropped cannot hide.

With N(0, 1) operands attention over n keys is close to uniform and a one-key masking error moves an output by ~|v| / n, below any
aggregate tolerance.  Two probes make it an O(1) error against the derived bound of util.compare_attention_elementwise:

  * boundary spikes: per head, every query row r gets one target key t(r) whose K row is overwritten with
    ALPHA * q_r / (scale * |q_r|^2), a score of ALPHA = 12 (e^12 times the other keys).  Head 0 targets the last key the row may
    see, head 1 the first key it may NOT see (possibly a stale slab row at or past kv_len), head 2 key 0, head 3 a random visible
    key; more heads cycle through these.  When several rows want one key the lowest row gets it.  Slab rows at or past kv_len
    carry V = +-3e4 (finite: the interface promises nothing about NaN in dead rows).
  * uniform checksum: q = 0 and integer V in [-8, 8]: every probability is exactly 1, every output (integer sum) / n, and the bound
    collapses to one bf16 rounding plus the fp32 sums -- a key lost or gained ANYWHERE (a skipped half tile, a skipped round)
    shows in most features.

The visibility rule is stated here independently of the kernels (oracle.prefix_lm_allowed and j < kv_len).  Every launch has
per-sequence q_pos0 / kv_len that differ between batch elements and an output buffer with guard rows and guard columns.  The
generators and the rule are device-agnostic: tests/test_util_cpu.py checks on the CPU that the bound accepts a float32 model of
the kernels on these inputs and rejects every one-key mask error."""
import ctypes as C
import math

import pytest
import torch

from moondream_amd import _lib
from moondream_amd.weights import rope_table
from oracle.moondream_oracle import apply_rope, prefix_lm_allowed, rope_table as o_rope_table
from util import compare_attention_elementwise

BF16 = torch.bfloat16
F8 = torch.float8_e4m3fn
ALPHA = 12.0
DEAD_V = 3.0e4
GUARD_BITS = 0x7FC1  # a bf16 NaN with a payload no kernel produces
GUARD_ROWS, GUARD_COLS = 3, 16


# ---------------------------------------------------------------------------------------------------------------------
# the visibility rule and the probe inputs (no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------
def visibility(pos0, q_len, kv_len, prefix, ctx):
    """bool [q_len, ctx]: key j is visible to the query at position p = pos0 + r iff it exists (j < kv_len) and the prefix-LM
    rule admits it.  Second result: per row, the first key the RULE alone hides (max(prefix, p + 1) inside the prefix, else p + 1)."""
    pos = torch.arange(pos0, pos0 + q_len)
    allowed = prefix_lm_allowed(pos, ctx, prefix) & (torch.arange(ctx) < kv_len).unsqueeze(0)
    edge = torch.where(pos < prefix, torch.clamp(pos + 1, min=prefix), pos + 1)
    return allowed, edge


def _rand(shape, gen, device):
    return torch.randn(*shape, generator=gen).to(BF16).to(device)


def _kill_dead_rows(v, kv_lens, gen):
    """slab rows no row of the call may see: V = +-3e4"""
    b, hk, ctx, d = v.shape
    for bi in range(b):
        n = int(kv_lens[bi])
        if n < ctx:
            sign = torch.randint(0, 2, (hk, ctx - n, d), generator=gen).float() * 2 - 1
            v[bi, :, n:] = (sign * DEAD_V).to(BF16).to(v.device)


def pick_targets(allowed, edge, n_heads, n_kv_heads, gen):
    """The spike targets of one sequence: int64 [n_heads, rows], -1 = none.  Head h is of kind h % 4 (0: last visible key, 1: first
    key not visible -- the end of the row's visible range, else the rule's own edge --, 2: key 0, 3: a random visible key).  A key
    row of a KV head is given once: to the lowest row, and within a row to the lowest head of the group."""
    rows, ctx = allowed.shape
    n_vis = allowed.sum(1)
    assert bool((allowed == (torch.arange(ctx).unsqueeze(0) < n_vis.unsqueeze(1))).all()), "visible keys form a range from key 0"
    group = n_heads // n_kv_heads
    out = torch.full((n_heads, rows), -1, dtype=torch.int64)
    for hk in range(n_kv_heads):
        claimed = set()
        for r in range(rows):
            n = int(n_vis[r])
            for h in range(hk * group, (hk + 1) * group):
                kind = h % 4
                cands = [[n - 1], [n, int(edge[r])], [0], [int(torch.randint(0, n, (1,), generator=gen))]][kind]
                for t in cands:
                    if 0 <= t < ctx and t not in claimed:
                        claimed.add(t)
                        out[h, r] = t
                        break
    return out


def write_spikes(q, k, targets, scale):
    """k[kv head of h, t(h, r)] = ALPHA * q[h, r] / (scale * |q[h, r]|^2) for one sequence (q [H, rows, d], k [HK, ctx, d])."""
    group = q.shape[0] // k.shape[0]
    targets = targets.to(q.device)
    h_idx, r_idx = torch.nonzero(targets >= 0, as_tuple=True)
    qq = q[h_idx, r_idx].float()
    k[h_idx // group, targets[h_idx, r_idx]] = (qq * (ALPHA / scale) / qq.pow(2).sum(-1, keepdim=True)).to(BF16)


def spike_probe(vis, n_heads, n_kv_heads, d, ctx, kv_lens, scale, seed, device="cpu"):
    """vis: per sequence (allowed [rows, ctx], edge [rows]).  Returns q [B, H, rows, d], k / v [B, HK, ctx, d] (bf16) and the
    targets [B, H, rows]."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    b, rows = len(vis), vis[0][0].shape[0]
    q, k, v = _rand((b, n_heads, rows, d), gen, device), _rand((b, n_kv_heads, ctx, d), gen, device), _rand((b, n_kv_heads, ctx, d), gen, device)
    _kill_dead_rows(v, kv_lens, gen)
    targets = torch.stack([pick_targets(a, e, n_heads, n_kv_heads, gen) for a, e in vis])
    for bi in range(b):
        write_spikes(q[bi], k[bi], targets[bi], scale)
    return q, k, v, targets


def uniform_probe(vis, n_heads, n_kv_heads, d, ctx, kv_lens, scale, seed, device="cpu"):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    b, rows = len(vis), vis[0][0].shape[0]
    q = torch.zeros(b, n_heads, rows, d, dtype=BF16, device=device)
    k = _rand((b, n_kv_heads, ctx, d), gen, device)
    v = torch.randint(-8, 9, (b, n_kv_heads, ctx, d), generator=gen).to(BF16).to(device)
    _kill_dead_rows(v, kv_lens, gen)
    return q, k, v, torch.full((b, n_heads, rows), -1, dtype=torch.int64)


PROBES = {"spikes": spike_probe, "uniform": uniform_probe}


def check_rows(name, got, q, k, v, vis, scale):
    """got [B, H, rows, d] against the exact attention of every sequence (KV heads repeated over their group)."""
    group = q.shape[1] // k.shape[1]
    for bi, (allowed, _) in enumerate(vis):
        kk, vv = k[bi].repeat_interleave(group, 0), v[bi].repeat_interleave(group, 0)
        compare_attention_elementwise(f"{name} seq {bi}", got[bi], q[bi], kk, vv, allowed.to(got.device).unsqueeze(0), scale)


# ---------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def i32(x):
    return torch.tensor([int(i) for i in x], dtype=torch.int32, device="cuda")


class Guarded:
    """bf16 output [batch, rows, width] inside a buffer with GUARD_ROWS rows after every sequence's last row and GUARD_COLS columns
    past the row, all GUARD_BITS; check() asserts that the kernel wrote the payload only."""

    def __init__(self, batch, rows, width):
        self.raw = torch.full((batch, rows + GUARD_ROWS, width + GUARD_COLS), GUARD_BITS, dtype=torch.int16, device="cuda")
        self.rows, self.width = rows, width
        self.ld, self.bs = width + GUARD_COLS, (rows + GUARD_ROWS) * (width + GUARD_COLS)

    def ptr(self):
        return self.raw.data_ptr()

    def check(self, name):
        assert bool((self.raw[:, self.rows:] == GUARD_BITS).all()), f"{name}: rows after the last query row were written"
        assert bool((self.raw[:, :, self.width:] == GUARD_BITS).all()), f"{name}: columns past n_heads * head_dim were written"
        return self.raw.view(BF16)[:, : self.rows, : self.width]


def prefill(lib, q, k, v, pos0, kv_lens, prefix, vit_layout):
    """q [B, H, rows, d], k / v [B, HK, ctx, d] -> o [B, H, rows, d].  Slab layout as md_text_forward passes it, or (vit_layout) the
    fused [B, T, 3 * H * d] activation of md_vit_encode: q | k | v side by side, token stride 3 D, head stride d."""
    b, h, rows, d = q.shape
    hk, ctx = k.shape[1], k.shape[2]
    a = _lib.MdAttnArgs()
    if vit_layout:
        assert hk == h and ctx == rows
        D = h * d
        qkv = torch.cat([t.permute(0, 2, 1, 3).reshape(b, rows, D) for t in (q, k, v)], dim=-1).contiguous()
        base, esz = qkv.data_ptr(), 2
        a.q, a.k, a.v = base, base + D * esz, base + 2 * D * esz
        a.q_bs = a.k_bs = a.v_bs = rows * 3 * D
        a.q_ts = a.k_ts = a.v_ts = 3 * D
        a.q_hs = a.k_hs = a.v_hs = d
    else:
        qq = q.permute(0, 2, 1, 3).contiguous()  # [B, rows, H, d]
        kk, vv = k.contiguous(), v.contiguous()
        a.q, a.q_bs, a.q_ts, a.q_hs = qq.data_ptr(), rows * h * d, h * d, d
        a.k, a.k_bs, a.k_ts, a.k_hs = kk.data_ptr(), hk * ctx * d, d, ctx * d
        a.v, a.v_bs, a.v_ts, a.v_hs = vv.data_ptr(), hk * ctx * d, d, ctx * d
    out = Guarded(b, rows, h * d)
    a.o, a.o_bs, a.o_ts, a.o_hs = out.ptr(), out.bs, out.ld, d
    a.batch, a.n_heads, a.n_kv_heads, a.head_dim = b, h, hk, d
    a.q_len, a.kv_len_all = rows, 0
    p0, kl = i32(pos0), i32(kv_lens)
    a.q_pos0, a.kv_len = p0.data_ptr(), kl.data_ptr()
    a.prefix_len, a.scale = prefix, 1.0 / math.sqrt(d)
    _lib.check(lib.md_attention_prefill(C.byref(a), stream()), "attn")
    torch.cuda.synchronize()
    return out.check("prefill").reshape(b, rows, h, d).permute(0, 2, 1, 3)


# (id, head_dim, n_heads, n_kv_heads, prefix, q_len, ctx, pos0 per sequence, vit layout)
def _prefill_cases():
    cases = [("causal-129", 64, 4, 4, 0, 129, 256, (0, 3), False),          # two query blocks, a wave with one live row
             ("prefix70-200", 64, 4, 4, 70, 200, 256, (0, 3), False)]       # the prefix ends inside a wave
    for prefix in (64, 128):                                                 # the prefix ends on a tile edge
        for q_len in (97, 160):
            cases.append((f"prefix{prefix}-{q_len}", 64, 4, 4, prefix, q_len, 256, (0, 3), False))
    for q_len, pos in ((5, 725), (10, 725), (1, 735), (33, 731)):            # continuation across the prefix end (730)
        cases.append((f"cont-{q_len}at{pos}", 64, 4, 4, 730, q_len, 768, (pos, pos - 3), False))
    for hd in (72, 64):                                                      # no mask, the ViT's strides
        for t in (33, 64, 65, 96, 97, 729):
            cases.append((f"nomask-hd{hd}-{t}", hd, 4, 4, t + 3, t, t, (0, 3), True))
    for hk in (2, 4):                                                        # grouped KV heads
        cases.append((f"gqa8over{hk}-causal-129", 64, 8, hk, 0, 129, 256, (0, 3), False))
        cases.append((f"gqa8over{hk}-prefix70-200", 64, 8, hk, 70, 200, 256, (0, 3), False))
    return cases


def prefill_geometry(prefix, q_len, ctx, pos0, no_mask):
    """per sequence: kv_len and the visibility.  Masked cases: kv_len = pos0 + q_len.  No-mask cases (ctx = q_len keys, prefix past
    every position): the second sequence's last 3 key rows do not exist."""
    kv_lens = [ctx - p for p in pos0] if no_mask else [p + q_len for p in pos0]
    return kv_lens, [visibility(p, q_len, n, prefix, ctx) for p, n in zip(pos0, kv_lens)]


@pytest.mark.parametrize("probe", list(PROBES))
@pytest.mark.parametrize("case", _prefill_cases(), ids=lambda c: c[0])
def test_prefill_exact(lib, case, probe):
    name, hd, h, hk, prefix, q_len, ctx, pos0, vit = case
    scale = 1.0 / math.sqrt(hd)
    kv_lens, vis = prefill_geometry(prefix, q_len, ctx, pos0, vit)
    q, k, v, _ = PROBES[probe](vis, h, hk, hd, ctx, kv_lens, scale, seed=sum(name.encode()) + q_len, device="cuda")
    try:
        for skip in (3, 0):  # the exact work skipping on, and the full computation
            _lib.check(lib.md_gemm_set_tuning(b"attn_skip_dead", skip))
            o = prefill(lib, q, k, v, pos0, kv_lens, prefix, vit)
            check_rows(f"prefill {name} {probe} skip_dead={skip}", o, q, k, v, vis, scale)
    finally:
        lib.md_gemm_set_tuning(b"attn_skip_dead", 3)


# ---------------------------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------------------------
DEC_LENS = [1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048]
DEC_CTX, ROT = 2048, 32
# (id, n_heads, n_kv_heads, rows): <= 512 (row, head) pairs launch 16 waves per workgroup, more launch 4
DEC_SHAPES = [("16wave", 4, 4, 16), ("4wave", 9, 9, 64), ("gqa-16wave", 8, 2, 16), ("gqa-4wave", 8, 2, 80)]


def decode_geometry(rows):
    lens = (DEC_LENS * ((rows + len(DEC_LENS) - 1) // len(DEC_LENS)))[:rows]
    return lens, [visibility(n - 1, 1, n, 0, DEC_CTX) for n in lens]   # one query at position kv_len - 1: keys j < kv_len


def rope_rows(x, pos):
    """apply_rope of the oracle for one token per sequence: x [B, H, 64] at positions pos [B] -> [B, H, 64]"""
    cos, sin = o_rope_table(ROT // 2, DEC_CTX)
    return apply_rope(x.permute(1, 0, 2), cos.to(x.device), sin.to(x.device), pos.to(x.device), ROT).permute(1, 0, 2)


@pytest.mark.parametrize("probe", list(PROBES))
@pytest.mark.parametrize("shape", DEC_SHAPES, ids=lambda s: s[0])
def test_decode_exact(lib, shape, probe):
    name, h, hk, rows = shape
    lens, vis = decode_geometry(rows)
    q, k, v, _ = PROBES[probe](vis, h, hk, 64, DEC_CTX, lens, 0.125, seed=90 + rows + h, device="cuda")
    qbuf = torch.zeros(rows, h * 64 + 64, dtype=BF16, device="cuda")  # a leading dimension larger than the row
    qbuf[:, : h * 64] = q.reshape(rows, h * 64)
    out, kl = Guarded(1, rows, h * 64), i32(lens)
    k_in, v_in = k.clone(), v.clone()
    _lib.check(lib.md_attention_decode(qbuf.data_ptr(), qbuf.stride(0), out.ptr(), out.ld, k.data_ptr(), v.data_ptr(), hk * DEC_CTX * 64,
                                       DEC_CTX, kl.data_ptr(), rows, h, hk, 64, 0.125, stream()))
    torch.cuda.synchronize()
    o = out.check(f"decode {name}")[0].reshape(rows, h, 1, 64)
    assert torch.equal(k, k_in) and torch.equal(v, v_in)
    check_rows(f"decode {name} {probe}", o, q, k, v, vis, 0.125)


def fused_inputs(probe, h, rows, lens, vis, seed, k_quant=None, v_quant=None):
    """The fused activation [rows, q | k | v] and the slabs of md_attention_decode_rope, with the probe's structure on the ROTATED
    operands: a spike whose target is the new key (position kv_len - 1) is planted by making the raw k parallel to the raw q
    (RoPE is a rotation: the alignment survives it), every other one in the slab row against the rotated q.  Returns the
    activation, the slabs handed to the kernel (row kv_len - 1 still holds its stale content), and the operands of the
    reference: rotated q, and K / V as the kernel must see them -- new row included, through k_quant / v_quant when given."""
    pos = torch.tensor(lens) - 1  # (moved to the device below, once the CPU-side target bookkeeping is done)
    q, k, v, targets = PROBES[probe](vis, h, h, 64, DEC_CTX, lens, 0.125, seed=seed, device="cuda")
    gen = torch.Generator(device="cpu").manual_seed(seed + 1)
    q_raw = q[:, :, 0].clone()                                    # [rows, H, 64]
    k_raw, v_raw = _rand((rows, h, 64), gen, "cuda"), _rand((rows, h, 64), gen, "cuda")
    if probe == "uniform":
        v_raw = torch.randint(-8, 9, (rows, h, 64), generator=gen).to(BF16).cuda()
    new_key = (targets[:, :, 0] == pos.unsqueeze(1)).cuda()      # [rows, H]: the spike is the new row
    qf = q_raw.float()
    k_raw = torch.where(new_key.unsqueeze(-1), (qf * (ALPHA / 0.125) / qf.pow(2).sum(-1, keepdim=True).clamp_min(1e-30)).to(BF16), k_raw)
    q_rot, k_new = rope_rows(q_raw, pos), rope_rows(k_raw, pos)
    # the slab spikes against the rotated q (the probe wrote them against the raw one)
    for bi in range(rows):
        t = targets[bi].clone()
        t[t == int(pos[bi])] = -1
        write_spikes(q_rot[bi].unsqueeze(1), k[bi], t, 0.125)
    act = torch.zeros(rows, 3 * h * 64 + 64, dtype=BF16, device="cuda")
    act[:, : 3 * h * 64] = torch.cat([q_raw.reshape(rows, -1), k_raw.reshape(rows, -1), v_raw.reshape(rows, -1)], dim=1)
    k_slab, v_slab = k.clone(), v.clone()
    k_eff = k_quant(k) if k_quant else k.clone()
    v_eff = v_quant(v) if v_quant else v.clone()
    bi, pos = torch.arange(rows, device="cuda"), pos.cuda()
    k_eff[bi, :, pos] = k_quant(k_new) if k_quant else k_new
    v_eff[bi, :, pos] = v_quant(v_raw) if v_quant else v_raw
    return act, k_slab, v_slab, q_rot.unsqueeze(2), k_eff, v_eff, k_new, v_raw, pos


def expect_new_rows(slab, new, pos):
    want = slab.clone()
    want[torch.arange(slab.shape[0], device=slab.device), :, pos.to(slab.device)] = new
    return want


@pytest.mark.parametrize("probe", list(PROBES))
@pytest.mark.parametrize("shape", DEC_SHAPES[:2], ids=lambda s: s[0])
def test_decode_rope_exact(lib, shape, probe):
    """md_attention_decode_rope: the output against the exact attention over the rotated operands (the new row from the oracle's
    apply_rope), the K / V rows it writes bit for bit against apply_rope, and no other slab byte or activation byte changed."""
    name, h, _, rows = shape
    lens, vis = decode_geometry(rows)
    act, k_slab, v_slab, q_rot, k_eff, v_eff, k_new, v_new, pos = fused_inputs(probe, h, rows, lens, vis, seed=120 + rows)
    act_in, k_in, v_in = act.clone(), k_slab.clone(), v_slab.clone()
    out, kl = Guarded(1, rows, h * 64), i32(lens)
    freqs = rope_table(ROT, DEC_CTX).cuda()
    _lib.check(lib.md_attention_decode_rope(act.data_ptr(), act.stride(0), out.ptr(), out.ld, freqs.data_ptr(), k_slab.data_ptr(),
                                            v_slab.data_ptr(), h * DEC_CTX * 64, DEC_CTX, kl.data_ptr(), rows, h, 64, ROT, 0.125, stream()))
    torch.cuda.synchronize()
    o = out.check(f"decode_rope {name}")[0].reshape(rows, h, 1, 64)
    assert torch.equal(act, act_in)
    assert torch.equal(k_slab, expect_new_rows(k_in, k_new, pos)) and torch.equal(v_slab, expect_new_rows(v_in, v_new, pos))
    check_rows(f"decode_rope {name} {probe}", o, q_rot, k_eff, v_eff, vis, 0.125)


K_SCALE, V_SCALE = 2.0 ** -4, 2.0 ** -5  # powers of two: x / scale and x * (1 / scale) are the same number


def quant(x, scale):
    return (x.float() / scale).clamp(-448.0, 448.0).to(F8)


@pytest.mark.parametrize("probe", list(PROBES))
def test_decode_rope_f8_exact(lib, probe):
    """md_attention_decode_rope_f8: the reference runs over the DEQUANTISED e4m3 slabs, the new row quantised then dequantised;
    the same bound, with the operands as the kernel sees them.  Both copies of the new row are checked bit for bit."""
    h, rows = 4, 16
    lens, vis = decode_geometry(rows)
    kq, vq = (lambda x: quant(x, K_SCALE).float() * K_SCALE), (lambda x: quant(x, V_SCALE).float() * V_SCALE)
    act, k_slab, v_slab, q_rot, k_eff, v_eff, k_new, v_new, pos = fused_inputs(probe, h, rows, lens, vis, seed=150, k_quant=kq, v_quant=vq)
    k8, v8 = quant(k_slab, K_SCALE).view(torch.uint8).contiguous(), quant(v_slab, V_SCALE).view(torch.uint8).contiguous()
    act_in, k_in, v_in, k8_in, v8_in = act.clone(), k_slab.clone(), v_slab.clone(), k8.clone(), v8.clone()
    out, kl = Guarded(1, rows, h * 64), i32(lens)
    freqs = rope_table(ROT, DEC_CTX).cuda()
    _lib.check(lib.md_attention_decode_rope_f8(act.data_ptr(), act.stride(0), out.ptr(), out.ld, freqs.data_ptr(), k_slab.data_ptr(),
                                               v_slab.data_ptr(), k8.data_ptr(), v8.data_ptr(), h * DEC_CTX * 64, DEC_CTX,
                                               kl.data_ptr(), rows, h, ROT, 0.125, K_SCALE, V_SCALE, stream()))
    torch.cuda.synchronize()
    o = out.check("decode_rope_f8")[0].reshape(rows, h, 1, 64)
    assert torch.equal(act, act_in)
    assert torch.equal(k_slab, expect_new_rows(k_in, k_new, pos)) and torch.equal(v_slab, expect_new_rows(v_in, v_new, pos))
    assert torch.equal(k8, expect_new_rows(k8_in, quant(k_new, K_SCALE).view(torch.uint8), pos))
    assert torch.equal(v8, expect_new_rows(v8_in, quant(v_new, V_SCALE).view(torch.uint8), pos))
    check_rows(f"decode_rope_f8 {probe}", o, q_rot, k_eff, v_eff, vis, 0.125)


@pytest.mark.parametrize("q_len", [9, 1])
def test_rope_kv_write_grouped_heads(lib, q_len):
    """md_rope_kv_write with n_kv_heads < n_heads (8 over 2): rotated q in place, rotated k and v in the slab, bit for bit against the
    oracle's apply_rope; the k and v columns of the activation, its pad columns and every other slab row untouched."""
    b, h, hk, hd, ctx = 2, 8, 2, 64, 256
    gen = torch.Generator(device="cpu").manual_seed(33 + q_len)
    width = (h + 2 * hk) * hd
    qkv = _rand((b * q_len, width + 64), gen, "cuda")
    orig = qkv.clone()
    freqs = rope_table(ROT, ctx).cuda()
    pos0 = [100, 7]
    ks, vs = _rand((b, hk, ctx, hd), gen, "cuda"), _rand((b, hk, ctx, hd), gen, "cuda")
    ks_in, vs_in = ks.clone(), vs.clone()
    _lib.check(lib.md_rope_kv_write(qkv.data_ptr(), qkv.stride(0), freqs.data_ptr(), i32(pos0).data_ptr(), ks.data_ptr(), vs.data_ptr(),
                                    hk * ctx * hd, ctx, b, q_len, h, hk, hd, ROT, stream()))
    torch.cuda.synchronize()
    cos, sin = o_rope_table(ROT // 2, ctx)
    want_k, want_v = ks_in.cpu(), vs_in.cpu()
    o = orig.cpu().view(b, q_len, -1)
    got = qkv.cpu().view(b, q_len, -1)
    for bi in range(b):
        pos = torch.arange(pos0[bi], pos0[bi] + q_len)
        q_raw = o[bi, :, : h * hd].reshape(q_len, h, hd).permute(1, 0, 2)
        k_raw = o[bi, :, h * hd : (h + hk) * hd].reshape(q_len, hk, hd).permute(1, 0, 2)
        v_raw = o[bi, :, (h + hk) * hd : width].reshape(q_len, hk, hd).permute(1, 0, 2)
        assert torch.equal(got[bi, :, : h * hd].reshape(q_len, h, hd).permute(1, 0, 2), apply_rope(q_raw, cos, sin, pos, ROT))
        want_k[bi][:, pos] = apply_rope(k_raw, cos, sin, pos, ROT)
        want_v[bi][:, pos] = v_raw
    assert torch.equal(ks.cpu(), want_k) and torch.equal(vs.cpu(), want_v)
    assert torch.equal(got[:, :, h * hd :], o[:, :, h * hd :])  # k, v and the pad columns of the activation
