"""The rule of md_region_pick_encode_scored (include/moondream_hip.h) restated in numpy float64, for the tests: bf16 logits
(as the int16 bit patterns of their values), the number of groups and a window -> the picked bins and the log of the mass
within the window of each pick.  Also the reference's bin -> value rules (moondream.py:673-721), for the goldens."""
import numpy as np
import torch


def bf16_bits_to_f64(bits):
    """int16 bit patterns of bf16 values -> their float64 values (exact)."""
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def pick_bin(x):
    """md_region_pick_encode's pick in one group x (float64 [n_bins]): the largest value, ties to the lowest bin, NaN never
    picked, an all-NaN group -> bin 0."""
    ok = ~np.isnan(x)
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (x == x[ok].max()))[0])


def window_bounds(pick, window, n_bins):
    """The bins with |i - pick| <= window, clamped to the group: [lo, hi]."""
    return max(pick - window, 0), min(pick + window, n_bins - 1)


def group_logprob(x, pick, window):
    """log(W) - log(S) of one group x (float64 [n_bins]): S over every bin, W over the window around ``pick``, both of
    exp(x - x[pick]).  A window that covers the group takes the SAME sum for both, so the result is exactly 0."""
    lo, hi = window_bounds(pick, window, x.shape[0])
    with np.errstate(all="ignore"):
        e = np.exp(x - x[pick])
        return float(np.log(e[lo : hi + 1].sum()) - np.log(e[0 : x.shape[0]].sum()))


def region_scores(logits_bits, n_groups, n_bins, window):
    """One launch.  ``logits_bits`` int16 [B, >= n_groups * n_bins] -> (bins int64 [B, n_groups], logprobs float64 [B, n_groups])."""
    x = bf16_bits_to_f64(logits_bits)
    b = x.shape[0]
    bins = np.zeros((b, n_groups), dtype=np.int64)
    lps = np.zeros((b, n_groups), dtype=np.float64)
    for r in range(b):
        for g in range(n_groups):
            xg = x[r, g * n_bins : (g + 1) * n_bins]
            bins[r, g] = pick_bin(xg)
            lps[r, g] = group_logprob(xg, int(bins[r, g]), window)
    return bins, lps


def coord_value(bins, n_bins):
    """moondream.py:673-674: argmax / size(-1), an int64 tensor over an int -> fp32, read back as a Python float."""
    return (torch.as_tensor(np.asarray(bins), dtype=torch.int64) / n_bins).tolist()


def size_value(bins):
    """moondream.py:699-701: 2^(bin / 1023 * 10 - 10) in fp32."""
    return torch.pow(2.0, (torch.as_tensor(np.asarray(bins), dtype=torch.int64).float() / 1023.0) * 10.0 - 10.0).tolist()


def boxes(xb, yb, wb, hb, n_bins):
    """moondream.py:703-721: (x_min, y_min, x_max, y_max) per object from its four bins."""
    out = []
    for x, y, w, h in zip(coord_value(xb, n_bins), coord_value(yb, n_bins), size_value(wb), size_value(hb)):
        out.append([x - w / 2, y - h / 2, x + w / 2, y + h / 2])
    return out
