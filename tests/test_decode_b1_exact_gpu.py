"""decode_b1_kernel (csrc/decode_b1.hip: md_decode_b1_layers and md_decode_step_b1) against independent float64 references.

The model under test is built here: md_text_model structs over weights the test chooses (PackedLayerNorm, FusedLinear,
PackedLinear), its own KV slabs, workspace and ONE zeroed 16 KiB sync state for the whole module, so that the barrier epoch is
carried across the layers entry, the step entry and 1 / 2 / 3 layers in whatever order the tests run; after every launch word
704 must be 0.  test_case_list_takes_every_branch restates the kernel's work-list expressions (util.b1_branches) with the
device's CU count and fails if the cases below no longer reach a branch.

Tier 1, exact probes.  Facts of the kernel they rest on:
  * ln.w = 0 makes the layer-norm output ln.b bit for bit ((v - mean) * rstd * 0 + b) for any finite x;
  * at pos = 0 the RoPE table is (1, 0): the rotation is the reference's interleaving permutation alone (util.rope64);
  * q weights and bias zero make every score 0, every probability exp2(0) = 1.0: a slice's partial is max = 0, sum = its key
    count, out = the plain sum of its V rows; with one key (pos = 0) the attention row IS the new v;
  * operands are small integers over a power of two, so that every product and every partial sum in any order is exact in
    fp32: the stored bf16 must equal round_to_bf16(float64), GELU outputs lie in util.gelu_interval.
Tier 2, random operands (all randn): hidden, the new K / V rows and the step's logits against util.b1_block_ref(rounded=False),
with the batched kernels (md_text_forward at q_len 1 on the same weights, cache and input) as the yardstick: RMS error at most
1.5 x theirs, maximum error at most theirs + 2 bf16 spacings.  The error of an element is counted in the bf16 spacing at the
largest of |truth| and the addends the kernel rounds on the way to it (hidden: x, proj + bp, fc2 + b2; logits: lm_w . ln), see
util.err_in_spacings: counted in the spacing of a cancelled sum alone, one rounding of the fc2 term that falls the other way
under another summation order is 32 to 64 spacings (seen at S2 and S4) although no sum is wrong.

S4 costs: test_integer_block_is_exact launches twice there too (fc1 rows live for the act row, then fc1 biases with an exactly
known GELU for the residual chain), and test_proj_fc2_columns plants ONE (k1, k2) pair at S4, so that at dim 4096 / ff 8192
both sides of the half boundaries are covered by the full-row integer block only.

Measured on an MI355X (256 CUs), persistent | batched kernels, in the unit above:
  hidden, S1 - S4 at positions 0 / 8 / 777 / 2047 (13 cases): RMS 0.795 - 1.058 | 0.810 - 1.038 spacings, RMS ratio 0.973 - 1.057
    (S1 pos 8 the largest); maximum 3.71 - 22.15 | 3.71 - 21.15, persistent minus batched between -1.00 and +2.00 (S2 pos 777:
    13.27 against 11.27, ON the margin; S3 pos 2047: +1.00; eight cases +0.00).  The maxima sit where proj or fc2 is itself a
    cancelled dot product that carries the layer norm's and the gelu row's roundings: shared by both families;
  new K and V rows (spacing of the truth): bit for bit the batched kernels' in all 13 cases, RMS ratio 1.000;
  step entry (S1, vocabulary 4616, pos 777): hidden RMS 0.785 | 0.767 (ratio 1.024), maximum 5.01 | 5.01; logits RMS 3.801 | 3.993
    (ratio 0.952), maximum 119.40 | 155.40.

The instruments (reference, mutations, branch map) are tested without a GPU in tests/test_util_cpu.py."""
import ctypes as C
import pytest
import torch

from moondream_amd import _lib
from moondream_amd.weights import FusedLinear, PackedLayerNorm, PackedLinear, rope_table
import functools

import util as U
from util import (B1_BRANCHES, B1_ERR_WORD, B1_MAX_EXTRA, B1_PART, B1_RMS_RATIO, B1_SLICES, KEY_COUNTS, SAFE_GELU, TIER2_CASES, TIER2_CTX,
                  TIER2_STEP, assert_exact_block, b1_barriers, b1_block_ref, b1_branches, b1_case_list, b1_layout, b1_logits_ref,
                  b1_shapes as shapes, compare_attention_elementwise, err_in_spacings, gelu_interval, hidden_terms, residual_chain, rint,
                  rope64, round_to_bf16)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
# the input builders of util.py on the device
gen, zero_weights, int_weights, int_x, slice_probe_inputs, tier2_inputs, tier2_step_inputs = (
    functools.partial(f, dev=DEV) for f in (U.gen, U.zero_weights, U.int_weights, U.int_x, U.slice_probe_inputs, U.tier2_inputs, U.tier2_step_inputs))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return _lib.load()


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Sync:
    """The one barrier state of the module and the barrier counts of the launches it has carried."""
    def __init__(self):
        self.state = torch.zeros(4096, dtype=torch.int32, device=DEV)
        self.counts = []
        self.launches = set()  # (dim, ff, n_layers, L, ctx, vocab; 0: the layers entry) of every launch

    def after(self, case_id, rig, step):
        n_layers = rig.n_layers
        self.launches.add((rig.dim, rig.ff, n_layers, int(rig.pos) + (0 if step else 1), rig.ctx, rig.vocab if step else 0))
        self.counts.append(b1_barriers(n_layers, step))
        assert int(self.state[B1_ERR_WORD]) == 0, f"{case_id}: a grid barrier timed out (word 704 raised)"
        assert int(self.state[0]) == sum(self.counts), f"{case_id}: epoch {int(self.state[0])} after {sum(self.counts)} barriers"


@pytest.fixture(scope="module")
def sync(lib):
    return Sync()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Rig:
    """md_text_model + md_kv_cache + workspace over ``weights`` (one dict of float64 tensors with bf16 values per layer, see
    util.b1_block_ref).  The slabs have one layer more than the model, which must keep its bits; they start as NaN."""
    def __init__(self, lib, sync, name, weights, *, ctx, rot=32, head=None):
        self.lib, self.sync, self.name, self.W = lib, sync, name, weights
        w0 = weights[0]
        self.dim, self.ff, self.n_layers, self.ctx, self.rot = w0["ln_w"].numel(), w0["w2"].shape[1], len(weights), ctx, rot
        self.H = self.dim // 64
        self.keep = []
        self.blocks = (_lib.MdTextBlock * self.n_layers)()
        self.ln, self.fused, self.proj, self.fc2 = [], [], [], []
        d = self.dim
        for l, w in enumerate(weights):
            ln = PackedLayerNorm(w["ln_w"], w["ln_b"], DEV)
            fu = FusedLinear(w["w1"][: 3 * d], w["b1"][: 3 * d], w["w1"][3 * d:], w["b1"][3 * d:], DEV)
            pr, f2 = PackedLinear(w["wp"], w["bp"], DEV), PackedLinear(w["w2"], w["b2"], DEV)
            blk = self.blocks[l]
            blk.ln, blk.qkv, blk.fc1, blk.qkv_fc1, blk.proj, blk.fc2 = ln.struct(), fu.struct_a(), fu.struct_b(), fu.struct(), pr.struct(), f2.struct()
            self.ln.append(ln), self.fused.append(fu), self.proj.append(pr), self.fc2.append(f2)
        self.ff_pad = self.fused[0].nb_pad
        self.freqs = rope_table(rot, ctx).to(DEV)
        if head is None:  # post_w, post_b [D], lm_w [V, D], lm_b [V], wte [V, D]; the layers entry reads none of them
            head = dict(post_w=torch.zeros(d), post_b=torch.zeros(d), lm_w=torch.zeros(256, d), lm_b=torch.zeros(256), wte=torch.zeros(256, d))
        self.head = head
        self.vocab = head["lm_w"].shape[0]
        self.post, self.lm = PackedLayerNorm(head["post_w"], head["post_b"], DEV), PackedLinear(head["lm_w"], head["lm_b"], DEV)
        self.wte = head["wte"].to(device=DEV, dtype=BF16).contiguous()
        self.model = _lib.MdTextModel(
            d, self.H, self.H, self.n_layers, self.ff, self.vocab, ctx, 0, rot, C.cast(self.blocks, C.POINTER(_lib.MdTextBlock)),
            self.post.struct(), self.lm.struct(), self.wte.data_ptr(), self.freqs.data_ptr())
        self.k = torch.full((self.n_layers + 1, self.H, ctx, 64), float("nan"), dtype=BF16, device=DEV)
        self.v = torch.full_like(self.k, float("nan"))
        self.kv = self.kv_struct(self.k, self.v)
        need = lib.md_decode_b1_workspace_bytes(C.byref(self.model))
        self.lay = b1_layout(d, self.ff_pad, self.H)
        assert need == self.lay["total"], f"{name}: workspace {need} bytes, the layout helper says {self.lay['total']}"
        self.ws = torch.zeros(max(need, lib.md_decode_step_b1_workspace_bytes(C.byref(self.model))), dtype=torch.uint8, device=DEV)
        self.pos = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert lib.md_decode_step_b1_supported(C.byref(self.model), C.byref(self.kv)) == 1, f"{name}: md_decode_step_b1_supported says no"

    def kv_struct(self, k, v):
        return _lib.MdKvCache(k.data_ptr(), v.data_ptr(), self.H * self.ctx * 64, self.H * self.ctx * 64, self.ctx)

    def supported(self):
        return self.lib.md_decode_step_b1_supported(C.byref(self.model), C.byref(self.kv))

    # workspace views
    def act(self):
        o = self.lay["act"]
        return self.ws[o: o + 2 * (3 * self.dim + self.ff)].view(BF16)

    def part(self):
        o = self.lay["part"]
        return self.ws[o: o + 4 * self.H * B1_SLICES * B1_PART].view(torch.float32).view(self.H, B1_SLICES, B1_PART)

    def x_buf(self, i):
        o = self.lay["x1" if i else "x0"]
        return self.ws[o: o + 2 * self.dim].view(BF16)

    def layers(self, case_id, x, pos, in_place=False):
        """md_decode_b1_layers at ``pos``; returns hidden [D] bf16.  in_place: x_in == hidden."""
        self.pos.fill_(pos)
        x = x.to(device=DEV, dtype=BF16).contiguous().clone()
        hidden = x if in_place else torch.full_like(x, float("nan"))
        st = self.lib.md_decode_b1_layers(C.byref(self.model), x.data_ptr(), hidden.data_ptr(), self.pos.data_ptr(), C.byref(self.kv),
                                          self.ws.data_ptr(), self.ws.numel(), self.sync.state.data_ptr(), stream())
        _lib.check(st, f"md_decode_b1_layers [{case_id}]")
        torch.cuda.synchronize()
        self.sync.after(case_id, self, False)
        return hidden

    def step(self, case_id, token, pos, suppress):
        """md_decode_step_b1; returns (next, pos afterwards, logits [V] bf16)."""
        self.pos.fill_(pos)
        tok = torch.tensor([token], dtype=torch.int32, device=DEV)
        nxt = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        logits = torch.full((self.vocab,), float("nan"), dtype=BF16, device=DEV)
        st = self.lib.md_decode_step_b1(C.byref(self.model), tok.data_ptr(), nxt.data_ptr(), self.pos.data_ptr(), C.byref(self.kv), suppress,
                                        logits.data_ptr(), self.vocab, self.ws.data_ptr(), self.ws.numel(), self.sync.state.data_ptr(), stream())
        _lib.check(st, f"md_decode_step_b1 [{case_id}]")
        torch.cuda.synchronize()
        self.sync.after(case_id, self, True)
        return int(nxt), int(self.pos), logits


def bits(t):
    return t.contiguous().view(torch.int16)


def assert_bits(name, got, want64):
    """got (bf16) must BE round_to_bf16(want64): compared as values and as bit patterns (so -0 and NaN count)."""
    want = round_to_bf16(want64.double()).to(BF16)
    g = got.reshape(want.shape)
    bad = bits(g) != bits(want)
    bad &= ~((g.float() == 0) & (want.float() == 0))  # the sign of an exact zero sum is not part of any claim
    n = int(bad.sum())
    if n:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {n} of {bad.numel()} elements differ; first at {i}: got {float(g.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r}")


def assert_within(name, got, lo, hi):
    g = got.double().reshape(lo.shape)
    bad = ~((g >= lo) & (g <= hi))
    n = int(bad.sum())
    if n:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {n} of {bad.numel()} elements outside their interval; first at {i}: got {float(g.reshape(-1)[i])!r}, "
                             f"[{float(lo.reshape(-1)[i])!r}, {float(hi.reshape(-1)[i])!r}]")


def slab_unchanged(name, rig, snap_k, snap_v, pos):
    """Every slab element but row ``pos`` of the model's layers keeps its bits: rows below pos, the NaN rows above it in every
    head, and the layer past n_layers."""
    for what, now, snap in (("K", rig.k, snap_k), ("V", rig.v, snap_v)):
        same = bits(now) == bits(snap)
        same[: rig.n_layers, :, pos] = True
        assert bool(same.all()), f"{name}: {int((~same).sum())} {what} slab elements outside row {pos} changed"


def rope_rows_f32(rig, v64, pos):
    """The new slab row as the kernel makes it: four separately rounded fp32 products, one subtraction, one addition, bf16."""
    hr = rig.rot // 2
    cs, sn = rig.freqs[pos, :, 0], rig.freqs[pos, :, 1]
    v = v64.float()
    re, im = v[..., :hr], v[..., hr: rig.rot]
    out = v.clone()
    out[..., 0: rig.rot: 2] = re * cs - im * sn
    out[..., 1: rig.rot: 2] = re * sn + im * cs
    return out.to(BF16)


# ---- the case list reaches every branch ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S4"])
def test_supported_says_yes(lib, sync, n_cu, name):
    """Every rig asserts md_decode_step_b1_supported == 1 when it is built; here at ctx 2048, and the refusals next to it."""
    s = shapes(n_cu)[name]
    rig = Rig(lib, sync, name, [zero_weights(s["dim"], s["ff"])], ctx=2048)
    assert rig.supported() == 1
    wte, rig.model.wte = rig.model.wte, None
    assert rig.supported() == 0  # the step entry needs the embedding table
    rig.model.wte = wte
    rig.kv.ctx = 2049
    assert rig.supported() == 0  # sc[] holds 2048 / 8 scores
    rig.kv.ctx = 2048
    assert rig.supported() == 1


# ---- Tier 1.1: fused rows -------------------------------------------------------------------------------------------------------
def check_phase_a(name, rig, w, lnb, x_any, *, layer=0):
    """One launch at pos = 0 with ln.w = 0: act must be W1 lnb + b1 rounded once (GELU interval on the fc1 part), slab rows 0 the
    permuted k and v.  Returns the observed gelu row (float64) for the fc2 expectation."""
    d = rig.dim
    pre = w["w1"] @ lnb + w["b1"]
    act = rig.act()
    assert_bits(f"{name}: q | k | v of act", act[: 3 * d], pre[: 3 * d])
    lo, hi = gelu_interval(round_to_bf16(pre[3 * d:]))
    assert_within(f"{name}: gelu(fc1) of act", act[3 * d:], lo, hi)
    qkv = round_to_bf16(pre[: 3 * d]).view(3, rig.H, 64)
    one, zero = torch.ones(rig.rot // 2, dtype=torch.float64, device=DEV), torch.zeros(rig.rot // 2, dtype=torch.float64, device=DEV)
    assert_bits(f"{name}: K slab row 0", rig.k[layer, :, 0], rope64(qkv[1], one, zero, rig.rot))
    assert_bits(f"{name}: V slab row 0", rig.v[layer, :, 0], qkv[2])
    return act[3 * d:].double()


def test_fused_rows_every_column(lib, sync, n_cu):
    """ln.w = 0, ln.b = e_k: the fused row must be column k of [Wqkv | Wfc1] plus bias, for every k at S1 (every lane and
    element position of the 16-byte weight loads, idle waves, the ff tail)."""
    s = shapes(n_cu)["S1"]
    d, ff = s["dim"], s["ff"]
    w = int_weights(d, ff, 11)
    w["w1"][:d] = rint(gen(12), -8, 8, d, d) / 64  # q rows live too (one key: no effect on att)
    rig = Rig(lib, sync, "S1 columns", [w], ctx=64)
    x = int_x(d, 13)
    for k in range(d):
        lnb = torch.zeros(d, dtype=torch.float64, device=DEV)
        lnb[k] = 1.0
        rig.ln[0].b.copy_(lnb)
        rig.k.fill_(float("nan")), rig.v.fill_(float("nan"))
        rig.layers(f"S1 column {k}", x, 0)
        check_phase_a(f"S1 column {k}", rig, w, lnb, x)


@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S4"])
def test_integer_block_is_exact(lib, sync, n_cu, name):
    """The whole block at pos = 0 with integer operands over the full rows: act, slab rows, and hidden = the residual chain of
    the one-key attention row (the new v) and the gelu row the kernel stored.  The chain's double rounding is live: asserted
    on the reference."""
    s = shapes(n_cu)[name]
    d, ff = s["dim"], s["ff"]
    w = int_weights(d, ff, 21)
    rig = Rig(lib, sync, name, [w], ctx=64)
    x = int_x(d, 22)
    rig.layers(f"{name} integer rows", x, 0)
    check_phase_a(name, rig, w, w["ln_b"], x)
    # second launch: the fc1 rows replaced by biases whose GELU is known exactly, so that fc2's operand is
    w["w1"][3 * d:] = 0
    w["b1"][3 * d:] = torch.tensor(SAFE_GELU, dtype=torch.float64, device=DEV)[rint(gen(23), 0, 5, ff).long()]
    rig.fused[0].w[3 * d: 3 * d + ff] = 0
    rig.fused[0].b[3 * d: 3 * d + ff] = w["b1"][3 * d:].to(BF16)
    rig.k.fill_(float("nan")), rig.v.fill_(float("nan"))
    hidden = rig.layers(f"{name} integer block", x, 0)
    gel = check_phase_a(name, rig, w, w["ln_b"], x)
    assert torch.equal(gel, w["b1"][3 * d:]), f"{name}: gelu of {SAFE_GELU} is not the identity in bf16"
    att = round_to_bf16(w["w1"][2 * d: 3 * d] @ w["ln_b"] + w["b1"][2 * d: 3 * d])
    assert_exact_block(name, w, att, gel)
    want, single, swapped = residual_chain(x, att, gel, w)
    for other, what in ((single, "one rounding"), (swapped, "fc2 first")):
        share = float((other != want).double().mean())
        print(f"{name}: {what} differs from the kernel's chain on {share:.3f} of {d} elements")
        assert share >= 0.05, (what, share)
    assert_bits(f"{name}: hidden", hidden, want)


# ---- Tier 1.2: key slices -------------------------------------------------------------------------------------------------------


def slice_probe(lib, sync, name, dim, ff, L, ctx, rot=32, seed=31):
    """q = 0, k bias random, v bias = the planted row of key pos, identity proj, x = 0: every (head, slice) partial and the
    combined row through hidden."""
    H, pos = dim // 64, L - 1
    w, vplant, kcache = slice_probe_inputs(dim, ff, L, seed)
    rig = Rig(lib, sync, name, [w], ctx=ctx, rot=rot)
    kcache = kcache.to(BF16)
    rig.k[0, :, :pos] = kcache[:, :pos]
    rig.v[0, :, :pos] = vplant[:, :pos].to(BF16)
    rig.k[1, :, :pos], rig.v[1, :, :pos] = 1.0, 1.0  # the layer past the model: finite rows a wrong layer stride would read
    snap_k, snap_v = rig.k.clone(), rig.v.clone()
    assert bool(torch.isnan(rig.k[0, :, pos:]).all()) and bool(torch.isnan(rig.v[0, :, pos:]).all())
    hidden = rig.layers(name, torch.zeros(dim), pos)
    slab_unchanged(name, rig, snap_k, snap_v, pos)
    knew = w["b1"][dim: 2 * dim].view(H, 64)
    assert torch.equal(bits(rig.k[0, :, pos]), bits(rope_rows_f32(rig, knew, pos))), f"{name}: K slab row {pos} is not the new rotated k"
    assert_bits(f"{name}: V slab row {pos}", rig.v[0, :, pos], vplant[:, pos])
    part = rig.part().double()
    assert not bool(torch.isnan(part).any()) and not bool(torch.isnan(hidden.float()).any()), f"{name}: a NaN row of the slab reached an output"
    chunk = (L + B1_SLICES - 1) // B1_SLICES
    for sl in range(B1_SLICES):
        j0, j1 = sl * chunk, min(L, sl * chunk + chunk)
        if j0 >= j1:
            assert bool((part[:, sl, 0] == float("-inf")).all()) and bool((part[:, sl, 1] == 0).all()) and bool((part[:, sl, 4:] == 0).all()), \
                f"{name}: empty slice {sl} is not the -inf partial"
            continue
        assert bool((part[:, sl, 0] == 0).all()), f"{name}: slice {sl} max {part[:, sl, 0].tolist()}"
        assert bool((part[:, sl, 1] == j1 - j0).all()), f"{name}: slice {sl} counts {part[:, sl, 1].tolist()} keys, has {j1 - j0}"
        want = vplant[:, j0:j1].sum(1)
        bad = part[:, sl, 4:] != want
        assert not bool(bad.any()), f"{name}: slice {sl} sum differs in heads {torch.nonzero(bad.any(1)).reshape(-1).tolist()}"
    exact = vplant.sum(1).reshape(-1) / L
    e = 2.0 ** -22 * exact.abs()  # v_rcp_f32 or a division (<= 2^-23) and one product (2^-24), then one bf16 rounding
    assert_within(f"{name}: combined attention row", hidden, round_to_bf16(exact - e), round_to_bf16(exact + e))


@pytest.mark.parametrize("L", KEY_COUNTS)
def test_key_slices_s1(lib, sync, n_cu, L):
    s = shapes(n_cu)["S1"]
    slice_probe(lib, sync, f"S1 L={L}", s["dim"], s["ff"], L, 2048)


@pytest.mark.parametrize("ctx", [40, 34])
def test_key_slices_last_position(lib, sync, n_cu, ctx):
    """pos = ctx - 1; at ctx 34 the last slice is empty and starts past ctx: load_kv's clamp keeps its loads inside the slab."""
    s = shapes(n_cu)["S1"]
    slice_probe(lib, sync, f"S1 ctx={ctx}", s["dim"], s["ff"], ctx, ctx)


@pytest.mark.parametrize("name,L", [("S2", 17), ("S3", 7), ("S3", 9), ("S3", 2048), ("S4", 2048)])
def test_key_slices_wide(lib, sync, n_cu, name, L):
    """More heads: at S3 / S4 a workgroup takes a second (head, slice) item and reloads its K / V rows."""
    s = shapes(n_cu)[name]
    slice_probe(lib, sync, f"{name} L={L}", s["dim"], s["ff"], L, 2048)


@pytest.mark.parametrize("rot", [16, 64])
def test_key_slices_other_rot_dims(lib, sync, n_cu, rot):
    """rot_dim 16 and 64 next to the shipping 32: the thread ranges of the rotated and the passed columns change."""
    s = shapes(n_cu)["S1"]
    for L in (1, 9, 17):
        slice_probe(lib, sync, f"S1 rot={rot} L={L}", s["dim"], s["ff"], L, 2048, rot=rot)


@pytest.mark.parametrize("rot", [16, 32, 64])
def test_dominant_key_in_another_slice(lib, sync, n_cu, rot):
    """One key whose score dominates sits in slice 1, the new position in the last slice: the cross-slice rescale
    exp2(m_slice - M) is live.  Held to util.compare_attention_elementwise through an identity proj."""
    s = shapes(n_cu)["S1"]
    d, ff, H, L = s["dim"], s["ff"], s["dim"] // 64, 41
    pos = L - 1
    g = gen(41 + rot)
    w = zero_weights(d, ff)
    w["b1"][: 3 * d] = rint(g, -16, 16, 3 * d) / 8
    w["b1"][d: 2 * d] /= 8  # the new key's score stays small
    w["wp"] = torch.eye(d, dtype=torch.float64, device=DEV)
    rig = Rig(lib, sync, f"dominant rot={rot}", [w], ctx=2048, rot=rot)
    q, knew, vnew = w["b1"][: 3 * d].view(3, H, 64)
    qr = rope_rows_f32(rig, q, pos)
    kc = (rint(g, -8, 8, H, L, 64) / 64).to(BF16)
    kc[:, 8] = (qr.float() * 0.25).to(BF16)  # slice 1 of chunk 6: score 0.125 * 0.25 |q|^2, several units above the rest
    vc = (rint(g, -64, 64, H, L, 64) / 8).to(BF16)
    rig.k[0, :, :pos], rig.v[0, :, :pos] = kc[:, :pos], vc[:, :pos]
    snap_k, snap_v = rig.k.clone(), rig.v.clone()
    hidden = rig.layers(rig.name, torch.zeros(d), pos)
    slab_unchanged(rig.name, rig, snap_k, snap_v, pos)
    keys, vals = kc.clone(), vc.clone()
    keys[:, pos], vals[:, pos] = rope_rows_f32(rig, knew, pos), vnew.to(BF16)
    m = rig.part()[:, :, 0]
    assert bool((m[:, 1] > m[:, pos // 6] + 2).all()), "the planted key does not dominate the slice of the new position"
    compare_attention_elementwise(rig.name, hidden.view(H, 1, 64), qr.view(H, 1, 64), keys, vals, None, 0.125)


# ---- Tier 1.3: proj, fc2 and the residual adds, one column at a time ------------------------------------------------------------
def boundary_columns(k):
    """Both K halves of set_rows_c and both sides of every edge: the half boundary, the 512-feature chunks, the row ends."""
    b = 512 * (((k + 511) // 512) // 2)
    c = {0, 1, 7, 8, k - 9, k - 8, k - 1, k // 2}
    for e in (b, 512, 512 * ((k - 1) // 512)):
        if 0 < e < k:
            c |= {e - 8, e - 1, e, e + 7}
    return sorted(x for x in c if 0 <= x < k)


@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S4"])
def test_proj_fc2_columns(lib, sync, n_cu, name):
    """att = 64 e_k1 (one key, v bias) and gelu(fc1) = 8 e_k2 (fc1 bias 8: its GELU rounds to 8): every output row pair must be
    bf16(bf16(x + bf16(64 Wp[:, k1] + bp)) + bf16(8 W2[:, k2] + b2)).  S4: one launch."""
    s = shapes(n_cu)[name]
    d, ff = s["dim"], s["ff"]
    w = int_weights(d, ff, 51)
    w["w1"].zero_(), w["b1"].zero_(), w["ln_b"].zero_()
    rig = Rig(lib, sync, name, [w], ctx=64)
    x = int_x(d, 52)
    c1, c2 = boundary_columns(d), boundary_columns(ff)
    n = 1 if name == "S4" else max(len(c1), len(c2))
    live = 0.0
    for i in range(n):
        k1, k2 = (c1[-4], c2[len(c2) // 2]) if name == "S4" else (c1[i % len(c1)], c2[i % len(c2)])
        b1 = torch.zeros(3 * d + ff, dtype=torch.float64, device=DEV)
        b1[2 * d + k1], b1[3 * d + k2] = 64.0, 8.0
        rig.fused[0].b[: 3 * d] = b1[: 3 * d].to(BF16)
        rig.fused[0].b[3 * d: 3 * d + ff] = b1[3 * d:].to(BF16)
        hidden = rig.layers(f"{name} k1={k1} k2={k2}", x, 0)
        act = rig.act().double()
        assert torch.equal(act, b1), f"{name} k1={k1} k2={k2}: the planted att / gelu rows are not what act holds"
        want, single, _ = residual_chain(x, b1[2 * d: 3 * d], b1[3 * d:], w)
        live = max(live, float((single != want).double().mean()))
        assert_bits(f"{name} k1={k1} k2={k2}: hidden", hidden, want)
    print(f"{name}: {n} column pairs; a single rounding would differ on up to {live:.3f} of the elements")
    assert live >= 0.05, live


# ---- Tier 1.4: layers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_layers", [("S1", 1), ("S1", 2), ("S1", 3), ("S2", 2), ("S3", 2)])
@pytest.mark.parametrize("in_place", [False, True])
def test_layers_use_their_own_weights_and_slab(lib, sync, n_cu, name, n_layers, in_place):
    """Distinct integer weights per layer, ln.w = 0 everywhere (x feeds the residual only): layer l writes rows 0 of slab layer l
    with ITS k and v, hidden is the chain of all layers, with x_in == hidden (one layer: through the workspace and the copy) and
    x_in != hidden; the slab layer past the model keeps its bits."""
    s = shapes(n_cu)[name]
    d, ff = s["dim"], s["ff"]
    W = [int_weights(d, ff, 61 + l, fc1_live=False) for l in range(n_layers)]
    rig = Rig(lib, sync, name, W, ctx=64)
    snap_k, snap_v = rig.k.clone(), rig.v.clone()
    x = int_x(d, 60)
    hidden = rig.layers(f"{name} {n_layers} layers in_place={in_place}", x, 0, in_place=in_place)
    slab_unchanged(name, rig, snap_k, snap_v, 0)
    one, zero = torch.ones(16, dtype=torch.float64, device=DEV), torch.zeros(16, dtype=torch.float64, device=DEV)
    want = x
    for l, w in enumerate(W):
        pre = w["w1"] @ w["ln_b"] + w["b1"]
        qkv = round_to_bf16(pre[: 3 * d]).view(3, rig.H, 64)
        assert_exact_block(f"{name} layer {l}", w, qkv[2].reshape(-1), pre[3 * d:])
        assert_bits(f"{name}: K slab layer {l}", rig.k[l, :, 0], rope64(qkv[1], one, zero, 32))
        assert_bits(f"{name}: V slab layer {l}", rig.v[l, :, 0], qkv[2])
        want = residual_chain(want, qkv[2].reshape(-1), pre[3 * d:], w)[0]
    assert_bits(f"{name}: hidden after {n_layers} layers", hidden, want)
    if n_layers == 1 and in_place:
        assert torch.equal(bits(rig.x_buf(1)), bits(hidden)), "hidden is not the workspace's x[1] row"




def batched_block(rig, x, pos, k, v):
    """md_text_forward at batch 1, q_len 1 on the rig's weights over its own copy of the slabs."""
    kv = rig.kv_struct(k, v)
    ws = torch.empty(rig.lib.md_text_workspace_bytes(C.byref(rig.model), 1, 1), dtype=torch.uint8, device=DEV)
    pos0 = torch.tensor([pos], dtype=torch.int32, device=DEV)
    xin = x.to(device=DEV, dtype=BF16).contiguous().clone()
    hidden = torch.full_like(xin, float("nan"))
    _lib.check(rig.lib.md_text_forward(C.byref(rig.model), xin.data_ptr(), hidden.data_ptr(), 1, 1, pos0.data_ptr(), C.byref(kv), ws.data_ptr(),
                                       ws.numel(), stream()), "md_text_forward")
    torch.cuda.synchronize()
    return hidden




# ---- Tier 1.5: the whole step ---------------------------------------------------------------------------------------------------
def tie_columns(n_cu, vocab):
    """Per lm_head column the ids that hold the equal maximum.  Pair p of the vocabulary runs in workgroup p % n_cu, wave
    (p // n_cu) % 8, as that wave's pair number p // (8 n_cu).
      column 0: different workgroups and waves, the last one in the last pair of the vocabulary;
      column 2: the two ids of ONE pair (the v1-against-v0 rule inside finish());
    and with more than 8 n_cu pairs (a workgroup with two pairs per wave):
      column 3: ONE workgroup, the lower id in the HIGHER wave -- thread 0's walk over the waves meets the higher id first and
                must let `best_i[ww] < bi` decide;
      column 4: ONE wave, its first and its second pair (the strict `>` of the running best)."""
    np_d = vocab // 2
    pairs = [5 % np_d, (n_cu - 56 + 3 * n_cu) % np_d, np_d - 1] + ([8 * n_cu] if np_d > 8 * n_cu else [])
    cols = {0: sorted({2 * p + (i & 1) for i, p in enumerate(pairs)}), 2: [18, 19]}
    if np_d > 8 * n_cu:
        cols[3] = [2 * (3 * n_cu) + 1, 2 * (8 * n_cu)]   # workgroup 0: wave 3, and wave 0's second pair
        cols[4] = [1, 2 * (8 * n_cu) + 1]                # workgroup 0, wave 0: first and second pair
    assert len({(i // 2) % n_cu for i in cols[0]}) >= 2
    return cols


@pytest.mark.parametrize("vocab", [256, 4610])
def test_whole_step_logits_and_greedy_choice(lib, sync, n_cu, vocab):
    """post_ln.w = 0, post_ln.b = e_k: the logits are column k of lm_head plus bias.  Column 0 holds equal maxima in different
    waves and workgroups (lowest id wins; suppressed: the next one), column 1 one maximum (suppressed: the runner-up), columns
    2 - 4 the ties of tie_columns that only the reductions INSIDE a pair, a workgroup and a wave decide; pos is incremented
    once; with zero proj / fc2 the residual row left in the workspace is wte[token]."""
    s = shapes(n_cu)["S1"]
    d, ff = s["dim"], s["ff"]
    g = gen(71)
    w = zero_weights(d, ff)
    cols = tie_columns(n_cu, vocab)
    ties = cols[0]
    lm_w = rint(g, -128, 128, vocab, d) / 64
    lm_b = rint(g, -32, 32, vocab) / 64
    for col, ids in cols.items():
        lm_w[ids, col], lm_b[ids] = 3.0, 0.0
    lm_w[ties[1], 1], lm_w[ties[2], 1] = 3.0, 2.75
    head = dict(post_w=torch.zeros(d), post_b=torch.zeros(d), lm_w=lm_w, lm_b=lm_b, wte=rint(g, -255, 255, vocab, d) / 128)
    rig = Rig(lib, sync, f"step V={vocab}", [w], ctx=64, head=head)
    rig.k[0, :, :8], rig.v[0, :, :8] = 1.0, 1.0
    # (column, token, suppressed id, expected next, pos)
    runs = [(0, 0, -1, ties[0], 0), (0, vocab - 1, ties[0], ties[1], 5), (1, 0, -1, ties[1], 0), (1, vocab - 1, ties[1], ties[2], 5),
            (0, 1, ties[-1], ties[0], 0)]
    runs += [(col, 2, -1, min(ids), 0) for col, ids in cols.items() if col >= 2] + [(2, 3, 18, 19, 5)]
    for col, token, suppress, want_next, pos in runs:
        e = torch.zeros(d, dtype=torch.float64, device=DEV)
        e[col] = 1.0
        rig.post.b.copy_(e)
        case = f"step V={vocab} column {col} token {token} suppress {suppress}"
        nxt, pos_after, logits = rig.step(case, token, pos, suppress)
        want = lm_w[:, col] + lm_b
        assert_bits(f"{case}: logits", logits, want)
        top = want.clone()
        if suppress >= 0:
            top[suppress] = float("-inf")
        assert int(torch.nonzero(top == top.max())[0]) == want_next, f"{case}: the planted maximum is not where the case says"
        assert nxt == want_next, f"{case}: next {nxt}, want {want_next} (ties {cols})"
        assert pos_after == pos + 1, f"{case}: pos {pos_after} after a step at {pos}"
        assert torch.equal(bits(rig.x_buf(1)), bits(rig.wte[token])), f"{case}: the residual row is not wte[{token}]"


# ---- Tier 2: random operands against float64, the batched kernels as the yardstick ---------------------------------------------
def batched_block(rig, x, pos, k, v):
    """md_text_forward at batch 1, q_len 1 on the rig's weights over its own copy of the slabs."""
    kv = rig.kv_struct(k, v)
    ws = torch.empty(rig.lib.md_text_workspace_bytes(C.byref(rig.model), 1, 1), dtype=torch.uint8, device=DEV)
    pos0 = torch.tensor([pos], dtype=torch.int32, device=DEV)
    xin = x.to(device=DEV, dtype=BF16).contiguous().clone()
    hidden = torch.full_like(xin, float("nan"))
    _lib.check(rig.lib.md_text_forward(C.byref(rig.model), xin.data_ptr(), hidden.data_ptr(), 1, 1, pos0.data_ptr(), C.byref(kv), ws.data_ptr(),
                                       ws.numel(), stream()), "md_text_forward")
    torch.cuda.synchronize()
    return hidden


def judge(case, what, got, yard, truth, terms, fails):
    (rg, mg), (ry, my) = err_in_spacings(got, truth, *terms), err_in_spacings(yard, truth, *terms)
    print(f"{case} {what}: persistent rms {rg:.3f} max {mg:.2f} | batched rms {ry:.3f} max {my:.2f} | rms ratio {rg / max(ry, 1e-30):.3f}, "
          f"max - max {mg - my:+.2f} spacings")
    if rg > B1_RMS_RATIO * ry or mg > my + B1_MAX_EXTRA:
        fails.append(f"{case} {what}: rms {rg:.3f} vs {ry:.3f}, max {mg:.2f} vs {my:.2f}")


@pytest.mark.parametrize("name,positions", TIER2_CASES)
def test_random_operands_track_float64(lib, sync, n_cu, name, positions):
    """randn operands, one block: hidden and the new K / V rows of the persistent kernel and of the batched kernels against the
    float64 truth.  The persistent kernel may have 1.5 x the batched RMS error and 2 spacings more at the maximum."""
    s = shapes(n_cu)[name]
    d, ff = s["dim"], s["ff"]
    w, kc, vc, x = tier2_inputs(d, ff)
    rig = Rig(lib, sync, name, [w], ctx=TIER2_CTX)
    fails = []
    for pos in positions:
        case = f"{name} pos={pos}"
        rig.k.fill_(float("nan")), rig.v.fill_(float("nan"))
        rig.k[0, :, :pos], rig.v[0, :, :pos] = kc[:, :pos], vc[:, :pos]
        k2, v2 = rig.k.clone(), rig.v.clone()
        hidden = rig.layers(case, x, pos)
        yard = batched_block(rig, x, pos, k2, v2)
        cs, sn = rig.freqs[pos, :, 0].double(), rig.freqs[pos, :, 1].double()
        truth = b1_block_ref(x.double(), w, kc.double(), vc.double(), pos, cs, sn, 32, rounded=False)
        judge(case, "hidden", hidden, yard, truth["hidden"], hidden_terms(truth), fails)
        judge(case, "K row", rig.k[0, :, pos], k2[0, :, pos], truth["k"], (), fails)
        judge(case, "V row", rig.v[0, :, pos], v2[0, :, pos], truth["v"], (), fails)
    assert not fails, fails


def test_random_step_logits_track_float64(lib, sync, n_cu):
    """The step entry with randn operands at S1: logits against the float64 truth, md_text_forward + md_lm_head as the yardstick;
    the step must pick the truth's token when its margin is wide."""
    s = shapes(n_cu)["S1"]
    d, ff, ctx = s["dim"], s["ff"], TIER2_CTX
    vocab, pos, token = TIER2_STEP["vocab"], TIER2_STEP["pos"], TIER2_STEP["token"]
    w, head, kc, vc = tier2_step_inputs(d, ff)
    rig = Rig(lib, sync, "S1 step random", [w], ctx=ctx, head=head)
    rig.k[0, :, :pos], rig.v[0, :, :pos] = kc[:, :pos], vc[:, :pos]
    k2, v2 = rig.k.clone(), rig.v.clone()
    nxt, _, logits = rig.step("S1 step random", token, pos, -1)
    x = head["wte"][token]
    hid_b = batched_block(rig, x, pos, k2, v2)
    lg_b = torch.full((1, vocab), float("nan"), dtype=BF16, device=DEV)
    ws = torch.empty(lib.md_lm_head_workspace_bytes(C.byref(rig.model), 1), dtype=torch.uint8, device=DEV)
    _lib.check(lib.md_lm_head(C.byref(rig.model), hid_b.data_ptr(), 1, 1, lg_b.data_ptr(), vocab, ws.data_ptr(), ws.numel(), stream()), "md_lm_head")
    torch.cuda.synchronize()
    cs, sn = rig.freqs[pos, :, 0].double(), rig.freqs[pos, :, 1].double()
    truth = b1_block_ref(x, w, kc.double(), vc.double(), pos, cs, sn, 32, rounded=False)
    lt, dot = b1_logits_ref(truth["hidden"], head["post_w"], head["post_b"], head["lm_w"], head["lm_b"], rounded=False, parts=True)
    fails = []
    judge("S1 step", "hidden", rig.x_buf(1), hid_b, truth["hidden"], hidden_terms(truth), fails)
    judge("S1 step", "logits", logits, lg_b[0], lt, (dot,), fails)
    assert not fails, fails
    top = torch.topk(lt, 2)
    if float(top.values[0] - top.values[1]) > 0.25:
        assert nxt == int(top.indices[0]), (nxt, int(top.indices[0]))


# ---- last: what ran is what was planned, and it took every branch ----------------------------------------------------------------
def test_launches_took_every_branch(sync, n_cu):
    """Runs last, over the launches the tests above recorded (run the whole module): they are exactly util.b1_case_list(), the list
    the CPU tests hold to the branch map at 256 CUs, and with THIS device's CU count they take every branch of util.B1_BRANCHES;
    four different barrier counts went through the one sync state."""
    sh = shapes(n_cu)
    planned = {(sh[n]["dim"], sh[n]["ff"], nl, L, ctx, v) for n, nl, L, ctx, v in b1_case_list()}
    assert sync.launches == planned, f"not planned: {sorted(sync.launches - planned)}; not run: {sorted(planned - sync.launches)}"
    taken = set()
    for dim, ff, _, L, ctx, vocab in sync.launches:
        taken |= b1_branches(n_cu, dim=dim, n_heads=dim // 64, ff=ff, L=L, ctx=ctx, vocab=vocab)
    missing = [b for b in B1_BRANCHES if b not in taken]
    assert not missing, f"with {n_cu} CUs no launch of this module takes: {missing}"
    assert len(set(sync.counts)) >= 4, set(sync.counts)
