"""Shared helpers for the parity tests."""
import numpy as np
import torch


def bits_to_bf16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).copy()).view(torch.bfloat16)


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """spacing of bf16 at |x| (8 significand bits)."""
    ax = x.float().abs().clamp_min(2.0 ** -120)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


def compare(name, got: torch.Tensor, ref: torch.Tensor, rel_rms: float, max_frac: float = None):
    """Tolerance check for bf16 activations of two implementations that share
    rounding points but not accumulation order: the RMS error relative to the
    RMS of the reference must stay below ``rel_rms``; ``max_frac`` optionally
    bounds the largest absolute error as a fraction of the largest |ref|."""
    g, r = got.detach().float().cpu(), ref.detach().float().cpu()
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    err = (g - r)
    rms = float(err.pow(2).mean().sqrt() / r.pow(2).mean().sqrt().clamp_min(1e-30))
    mx = float(err.abs().max() / r.abs().max().clamp_min(1e-30))
    msg = f"{name}: rel-rms {rms:.3e} (tol {rel_rms:.1e}), max-err/max-ref {mx:.3e}"
    print(msg)
    assert rms <= rel_rms, msg
    if max_frac is not None:
        assert mx <= max_frac, msg
    return rms, mx


def elementwise_excess(got: torch.Tensor, a: torch.Tensor, w: torch.Tensor, bias, *, rounded: bool) -> torch.Tensor:
    """``|got - exact| - bound`` per element (float64, on ``got``'s device) for ``got ~ a @ w^T + bias``; positive = violation.
    See compare_elementwise for the bound.  ``a`` [m, K] and ``w`` [n, K] are the bf16 operands, ``bias`` [n] or None."""
    dev = got.device
    a64, w64 = a.detach().to(dev).double(), w.detach().to(dev).double()
    b64 = torch.zeros(w.shape[0], dtype=torch.float64, device=dev) if bias is None else bias.detach().to(dev).double()
    assert a64.dim() == 2 and w64.dim() == 2 and a64.shape[1] == w64.shape[1]
    assert tuple(got.shape) == (a64.shape[0], w64.shape[0]), f"shape {tuple(got.shape)} vs {(a64.shape[0], w64.shape[0])}"
    k = a64.shape[1]
    exact = a64 @ w64.t() + b64
    mag = a64.abs() @ w64.abs().t() + b64.abs()
    g = got.detach().double()
    bound = (k + 1) * 2.0 ** -23 * mag
    if rounded:
        big = torch.maximum(g.abs(), exact.abs())
        _, e = torch.frexp(big)                       # big = f * 2^e, f in [0.5, 1): the bf16 spacing at big is 2^(e - 8)
        ulp = torch.ldexp(torch.ones_like(big), e.clamp_min(-125) - 8)
        bound = bound + 0.5 * torch.where(big > 0, ulp, torch.zeros_like(ulp))
    excess = (g - exact).abs() - bound
    return torch.where(torch.isfinite(g), excess, torch.full_like(excess, float("inf")))


def compare_elementwise(name, got: torch.Tensor, a: torch.Tensor, w: torch.Tensor, bias, *, rounded: bool):
    """Per-element bound for a GEMM with fp32 accumulation, derived and not measured.  With ``exact = a @ w^T + bias`` and
    ``mag = |a| @ |w|^T + |bias|`` evaluated in float64 from the bf16 operands, EVERY element must satisfy

        |got - exact| <= (0.5 * ulp_bf16(max(|got|, |exact|)) if rounded else 0) + (K + 1) * 2^-23 * mag

    Each of the K fp32 accumulate steps and the bias add is charged a relative error of 2^-23 of the running magnitude (which
    covers a truncating as well as a round-to-nearest accumulator) -- in any summation order and any split-K association; the
    single rounding to bf16 adds half a bf16 spacing at the larger of the two values, so a result that rounds across a binade
    is no false alarm.  ``rounded=False``: fp32 results (K-slice partial sums).  No element is excluded and there is no slack
    factor.  Returns ``|got - exact| - bound`` per element."""
    excess = elementwise_excess(got, a, w, bias, rounded=rounded)
    bad = excess > 0
    n_bad = int(bad.sum())
    flat = int(torch.argmax(excess))
    row, col = divmod(flat, excess.shape[1])
    msg = f"{name}: {n_bad} of {excess.numel()} elements exceed the per-element bound; worst ({row}, {col}) by {float(excess[row, col]):.3e}"
    print(msg if n_bad else f"{name}: all {excess.numel()} elements within the per-element bound (closest ({row}, {col}): {float(-excess[row, col]):.3e} to spare)")
    assert n_bad == 0, msg
    return excess


def attention_exact(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, allowed, scale: float):
    """Softmax attention in float64 from the operands as the kernel sees them (bf16, or dequantised e4m3), with NO intermediate
    rounding.  q [..., rows, d], k / v [..., keys, d], ``allowed`` bool [..., rows, keys] (None: every key); every row must see
    at least one key.  Returns ``exact = P V`` and ``mag = P |V|`` ([..., rows, d], float64, on q's device)."""
    return _attention_terms(q, k, v, allowed, scale)[:2]


def _attention_terms(q, k, v, allowed, scale):
    """attention_exact plus what the bound needs per row: the number of visible keys and A = scale * max_j sum_i |q_i| |k_ji|."""
    dev = q.device
    q64, k64, v64 = q.detach().double(), k.detach().to(dev).double(), v.detach().to(dev).double()
    scale = float(np.float32(scale))                         # the C ABI hands the kernels a float
    s = (q64 @ k64.transpose(-1, -2)) * scale
    a = (q64.abs() @ k64.abs().transpose(-1, -2)) * abs(scale)
    if allowed is None:
        allowed = torch.ones(s.shape, dtype=torch.bool, device=dev)
    allowed = allowed.to(dev).expand(s.shape)
    n_vis = allowed.sum(-1, keepdim=True)
    assert int(n_vis.min()) > 0, "a row without a visible key has no softmax"
    s = s.masked_fill(~allowed, float("-inf"))
    p = torch.softmax(s, dim=-1)
    a_row = a.masked_fill(~allowed, 0.0).amax(-1, keepdim=True)
    return p @ v64, p @ v64.abs(), n_vis.double(), a_row


ATTN_TAIL_OPS = 8  # the constant c of compare_attention_elementwise


def attention_excess(got: torch.Tensor, q, k, v, allowed, scale) -> torch.Tensor:
    """``|got - exact| - bound`` per element (float64, on ``got``'s device); positive = violation, a non-finite ``got`` is +inf.
    See compare_attention_elementwise for the bound."""
    exact, mag, n_vis, a_row = _attention_terms(q.to(got.device), k, v, allowed, scale)
    assert tuple(got.shape) == tuple(exact.shape), f"shape {tuple(got.shape)} vs {tuple(exact.shape)}"
    hd = q.shape[-1]
    assert int(n_vis.max()) <= 64 * hd, "the rescale count of the bound is derived for at most 64 * head_dim visible keys"
    u = 2.0 ** -23
    spread = a_row > 0                                       # rows whose scores are not all exactly equal
    ds = torch.where(spread, (hd + 2) * u * a_row + u, torch.zeros_like(a_row))
    p_round = torch.where(spread, torch.full_like(a_row, 2.0 ** -8), torch.zeros_like(a_row))
    rel = p_round + 2 * ds + (n_vis + hd + ATTN_TAIL_OPS) * u
    g = got.detach().double()
    big = torch.maximum(g.abs(), exact.abs())
    _, e = torch.frexp(big)                                  # big = f * 2^e, f in [0.5, 1): the bf16 spacing at big is 2^(e - 8)
    ulp = torch.ldexp(torch.ones_like(big), e.clamp_min(-125) - 8)
    vmax = v.detach().to(got.device).double().abs().amax(dim=(-1, -2), keepdim=True)
    bound = 0.5 * torch.where(big > 0, ulp, torch.zeros_like(ulp)) + rel * mag + n_vis * 2.0 ** -126 * vmax
    excess = (g - exact).abs() - bound
    return torch.where(torch.isfinite(g), excess, torch.full_like(excess, float("inf")))


def compare_attention_elementwise(name, got: torch.Tensor, q, k, v, allowed, scale):
    """Per-element bound for softmax attention, derived and not measured.  With ``exact = P V`` and ``mag = P |V|`` of
    attention_exact (float64, from the operands the kernel reads), n the number of keys the row may see, d = head_dim,
    u = 2^-23 and A = scale * max_j sum_i |q_i| |k_ji| over the row's visible keys (so |s_j| <= A for its scores
    s_j = scale * q . k_j), EVERY element must satisfy

        |got - exact| <= 0.5 * ulp_bf16(max(|got|, |exact|)) + (2^-8 + 2 ds + (n + d + c) u) * mag + n * 2^-126 * max|V|
        ds = (d + 2) u A + u,      c = 8

    Where each term comes from (attn_prefill_dma_kernel, attn_decode_kernel, attn_decode_f8_kernel); every kernel computes
    o = bf16((sum_j P~_j v_j) / (sum_j p^_j)) with p^_j = exp2((s^_j - m) c2), c2 = fp32(scale * log2 e), m a reference
    common to the row, P~_j = bf16(p^_j):
      * 0.5 ulp_bf16: the single rounding of the output, at the larger of the two values so that a result which rounds across
        a binade is no false alarm.
      * 2^-8: P~_j = p^_j (1 + r_j), |r_j| <= 2^-8 for truncation (2^-9 for round-to-nearest): the probabilities enter the P V
        product as bf16 while the row sum l adds their fp32 values, so the factor does not cancel.  The products P~_j v_j
        (8 x 8 significand bits, or 8 x 4 for e4m3) are exact in fp32.
      * 2 ds: a score error |s^_j - s_j| <= ds turns p_j into p_j e^(+-ds); numerator and denominator of o each move by that
        factor, e^(2 ds) - 1 -> 2 ds of mag.  ds in units of u A:  d for the head_dim accumulates of q . k_j, charged u of the
        running magnitude each as compare_elementwise does (any order; covers a truncating MFMA accumulator; the decode
        kernels' rounding of q_i * c2 and their FMA chain of 8 + 3 or 16 + 2 steps are 2^-24 each and stay far below it);
        1 for the one rounding of (s^_j - m) c2 -- the FMA of the prefill kernel, the subtraction of the decode kernels -- 2^-24
        of |s_j - m| c2 <= 2 A c2;  1 for c2 itself: the reference uses float32(scale), as the kernel receives it, which
        leaves the rounding of the literal log2(e) (2^-26.2) and of the product (2^-24), 1.22 * 2^-24 of |s_j - m| <= 2 A --
        the 0.22 u A beyond the unit is covered by the matrix cores rounding to nearest (their d accumulates cost d / 2).
        The fp8 kernel folds k_scale into the same constant: one more 2^-24, inside the same margin (its chain is 18 deep).
        The final + u: v_exp_f32 is accurate to 1 ulp (CDNA ISA), a relative error of p^_j of at most 2^-23 = an exponent
        error of u.  Errors of the reference m itself are common to all keys of the row and cancel in o.
      * n u: each visible key enters two fp32 sums, P V and the row sum l, by one round-to-nearest accumulate each: 2^-24 of
        the running magnitude (<= the final one: the terms of l are positive, mag sums |.|) apiece, in any order and any
        partition into classes, tiles or lanes.  Masked keys add exact zeros.
      * d u: the online-softmax rescales of the prefill kernel: O and l are both multiplied by alpha (alpha itself is common
        and cancels), 2 * 2^-24 = u per rescale, at most one per 64-key tile over the row's own keys: n / 64 <= d (asserted:
        n <= 64 d; the longest context of this project is 2048).
      * c = 8: three more rescales in the tiles past the row's own keys that its 128-row block still walks (3); the last
        cross-lane add of l (1, prefill); the normalisation, v_rcp_f32 (1 ulp) and a multiply in the prefill kernel, a
        division of <= 2.5 ulp in the decode kernels (3); the v_scale multiply of the fp8 kernel (1).
      * n * 2^-126 * max|V|: a probability below the smallest normal fp32 / bf16 number is flushed to zero, an absolute
        error of at most 2^-126 per key against l >= 1 (the largest p^_j of a row is >= 1).
    A row whose scores are all exactly equal (A = 0: q = 0) has s^_j = m = 0 in any arithmetic and p^_j = exp2(0) = 1, exact
    in fp32 and bf16: its 2^-8 and ds terms are dropped, and the bound is one output rounding plus the fp32 sums.  That is
    what lets the uniform probe see ONE key dropped or added among 2048.
    No element is excluded and there is no slack factor.  Returns ``|got - exact| - bound`` per element."""
    excess = attention_excess(got, q, k, v, allowed, scale)
    bad = excess > 0
    n_bad = int(bad.sum())
    flat = int(torch.argmax(excess))
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(excess.shape)))
    worst = float(excess.flatten()[flat])
    msg = f"{name}: {n_bad} of {excess.numel()} elements exceed the per-element bound; worst {idx} by {worst:.3e}"
    print(msg if n_bad else f"{name}: all {excess.numel()} elements within the per-element bound (closest {idx}: {-worst:.3e} to spare)")
    assert n_bad == 0, msg
    return excess


def margin_aware_mismatches(got, ref, margins, thr=0.5):
    """Greedy ids of two correct bf16 implementations can only part ways at a decision whose
    reference top-1/top-2 logit margin is within bf16 noise.  For every sequence: the first
    position where ``got`` and ``ref`` differ must have reference margin <= thr (margins[i][j] is the
    margin of the decision that produced token j); after that the sequences are unrelated.
    Returns (number of exactly equal sequences, list of violations)."""
    exact, bad = 0, []
    for i, (g, r) in enumerate(zip(got, ref)):
        g, r = list(g), list(r)
        n = min(len(g), len(r))
        j = next((t for t in range(n) if g[t] != r[t]), None)
        if j is None:
            exact += 1
        elif float(margins[i][j]) > thr:
            bad.append((i, j, g[j], r[j], float(margins[i][j])))
    return exact, bad


def leading_wide_objects(margins: np.ndarray, thr: float) -> int:
    """detect/point goldens: number of leading objects all of whose decisions (and every decision
    before them) have a reference margin >= thr bf16 ulps."""
    n = 0
    for row in margins:
        if float(row.min()) < thr:
            break
        n += 1
    return n


def vit_fp64(x_bchw: torch.Tensor, sd, cfg) -> torch.Tensor:
    """The ViT encoder as a function of its bf16 weights and bf16 input, evaluated in float64 with
    NO intermediate rounding (reference structure: vision.py:44-74, layers.py:118-166) -- the
    "truth" both bf16 implementations approximate."""
    v = cfg.vision
    f = lambda k: sd[k].detach().cpu().double()
    x = x_bchw.detach().cpu().double()
    B, C, H, W = x.shape
    P = v.enc_patch_size
    x = x.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // P) * (W // P), C * P * P)
    x = x @ f("vision.patch_emb.weight").t() + f("vision.patch_emb.bias") + f("vision.pos_emb")
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (t.shape[-1],), f(p + ".weight"), f(p + ".bias"), 1e-5)
    hd = v.enc_dim // v.enc_n_heads
    for i in range(v.enc_n_layers):
        p = f"vision.blocks.{i}"
        h = ln(x, p + ".ln1")
        qkv = h @ f(p + ".attn.qkv.weight").t() + f(p + ".attn.qkv.bias")
        q, k, vv = [t.reshape(B, -1, v.enc_n_heads, hd).transpose(1, 2) for t in qkv.chunk(3, dim=-1)]
        a = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1) @ vv
        a = a.transpose(1, 2).reshape(B, -1, v.enc_dim)
        x = x + a @ f(p + ".attn.proj.weight").t() + f(p + ".attn.proj.bias")
        h = ln(x, p + ".ln2")
        h = torch.nn.functional.gelu(h @ f(p + ".mlp.fc1.weight").t() + f(p + ".mlp.fc1.bias"), approximate="tanh")
        x = x + h @ f(p + ".mlp.fc2.weight").t() + f(p + ".mlp.fc2.bias")
    return ln(x, "vision.post_ln")


def quantize_int4(w, group=128, zero_shift=0.0):
    """The checkpoint format dequantize_int4 / the int4 weight stream read (reference layers.py:38-74), from a float weight."""
    rows = w.float().cpu().reshape(-1, group)
    lo, hi = rows.min(1, keepdim=True).values, rows.max(1, keepdim=True).values
    scale = ((hi - lo) / 15).clamp_min(1e-8)
    zero = -lo / scale + zero_shift
    q = torch.clamp(torch.round(rows / scale + zero), 0, 15).to(torch.uint8)
    step = q.shape[0] // 2
    return (q[:step] << 4) | q[step:], scale, zero
