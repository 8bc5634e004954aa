"""The rule of md_penalize_rows (include/moondream_hip.h) restated in numpy, for the tests: fp32 with every operation
rounded on its own (numpy float32 scalars never fuse a multiply with an add), the result rounded to bf16 by torch on the
CPU (round to nearest even).  Logits travel as the int16 bit patterns of their bf16 values."""
import numpy as np
import torch

F = np.float32


def bf16_bits_to_f32(bits):
    """int16 bit patterns of bf16 values -> their float32 values (exact)."""
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x):
    """float32 -> the int16 bit patterns of round-to-nearest-even bf16."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().copy()


def penalize_value(x, count, repetition, presence, frequency):
    """One logit ``x`` (float32) of a token seen ``count`` times -> the penalised float32 value, before the bf16 rounding."""
    x, repetition, presence, frequency = F(x), F(repetition), F(presence), F(frequency)
    with np.errstate(all="ignore"):
        if repetition != F(1):
            x = F(x / repetition) if x > 0 else F(x * repetition)
        return F(x - F(presence + F(frequency * F(count))))


def penalize_rows(logits_bits, vocab, tokens_in, slots, slot0, hist, hist_len, repetition, presence, frequency):
    """One launch.  ``logits_bits`` int16 [batch, ld]; ``slots`` an int list or None; ``hist`` int32 [n_slots, hist_cap] and
    ``hist_len`` int32 [n_slots].  Returns new (logits_bits, hist, hist_len); the arguments are left unchanged."""
    out, hist, hist_len = np.array(logits_bits, copy=True), np.array(hist, copy=True), np.array(hist_len, copy=True)
    cap = hist.shape[1]
    for r in range(out.shape[0]):
        s = slots[r] if slots is not None else slot0 + r
        if s < 0:
            continue
        t = int(tokens_in[r])
        if 0 <= t < vocab and hist_len[s] < cap:
            hist[s, hist_len[s]] = t
            hist_len[s] += 1
        if F(repetition[r]) == F(1) and F(presence[r]) == F(0) and F(frequency[r]) == F(0):
            continue
        ids, counts = np.unique(hist[s, : hist_len[s]], return_counts=True)
        for v, c in zip(ids.tolist(), counts.tolist()):
            x = bf16_bits_to_f32(out[r, v : v + 1])[0]
            out[r, v] = f32_to_bf16_bits(np.array([penalize_value(x, c, repetition[r], presence[r], frequency[r])]))[0]
    return out, hist, hist_len
