"""The sampling filters restated in torch on the CPU, over bf16 tensors (no kernel code, no oracle import): what
md_sample_rows_filtered must compute for one sampled row.  The filter has the shape of the reference's ``_apply_top_p``
(sort, cumulative sum, mask, divide by the sum, scatter) with two more masks; the draw is the kernel's documented rule."""
import numpy as np
import torch

BF16 = torch.bfloat16
THREADS = 1024  # the kernel's workgroup: the draw walks the ids in 1024 contiguous chunks


def filter_probs(probs: torch.Tensor, top_p: float, top_k: int = 0, min_p: float = 0.0) -> torch.Tensor:
    """One row of bf16 probabilities -> the renormalised survivors, bf16, at their ids.  The tokens in descending
    probability, ties by ascending id (a stable sort); each rule keeps a prefix of that order and all three look at the
    same unrenormalised row: past ``top_k`` everything goes (0, or >= the row's length: off), below
    ``bf16(float32(min_p) * best)`` everything goes (0: off), and top-p is the reference's mask with its bf16 roundings."""
    assert probs.dim() == 1 and probs.dtype == BF16
    probs_sort, probs_idx = torch.sort(probs, descending=True, stable=True)
    gone = torch.zeros(probs.numel(), dtype=torch.bool)
    if 0 < top_k < probs.numel():
        gone[top_k:] = True
    if min_p > 0:
        floor = (torch.tensor(min_p, dtype=torch.float32) * probs_sort[0].float()).to(BF16)
        gone |= probs_sort < floor
    probs_sum = torch.cumsum(probs_sort, dim=-1)   # fp32 running sum, rounded to bf16 per element
    gone |= (probs_sum - probs_sort) > top_p       # a bf16 subtraction; the python scalar compares as bf16
    probs_sort = probs_sort.clone()
    probs_sort[gone] = 0.0
    probs_sort.div_(probs_sort.sum(dim=-1, keepdim=True))
    return torch.zeros_like(probs).scatter_(0, probs_idx, probs_sort)


def draw(q: torch.Tensor, u: float) -> int:
    """The kernel's draw from the bf16 row ``q`` with the uniform ``u`` in [0, 1): inverse CDF over token ids, in fp32, in
    the kernel's order.  The ids are cut into 1024 contiguous chunks of ceil(V / 1024); a chunk's mass is the sequential
    fp32 sum of its values; the chunk masses go through a Hillis-Steele inclusive scan (offsets 1, 2, .., 512); the target
    is u * (the scan's last entry).  The chunk whose interval [scan - mass, scan) holds the target owns the draw: inside
    it the running sum starts at the interval's lower end and the first surviving token whose sum exceeds the target is
    drawn, the chunk's last surviving token if rounding leaves none.  Without an owner: the row's last surviving token."""
    v = q.numel()
    chunk = (v + THREADS - 1) // THREADS
    vals = np.zeros(THREADS * chunk, dtype=np.float32)
    vals[:v] = q.float().numpy()
    vals = vals.reshape(THREADS, chunk)
    mass = np.zeros(THREADS, dtype=np.float32)
    for j in range(chunk):
        mass = (mass + vals[:, j]).astype(np.float32)
    scan = mass.copy()
    off = 1
    while off < THREADS:
        scan[off:] = (scan[off:] + scan[:-off]).astype(np.float32)
        off *= 2
    target = np.float32(np.float32(u) * scan[-1])
    lo = (scan - mass).astype(np.float32)
    for t in range(THREADS):
        if mass[t] > 0 and lo[t] <= target < scan[t]:
            acc, last = lo[t], -1
            for j in range(chunk):
                if vals[t, j] > 0:
                    last = t * chunk + j
                    acc = np.float32(acc + vals[t, j])
                    if target < acc:
                        return last
            return last
    kept = np.nonzero(vals.reshape(-1) > 0)[0]
    return int(kept[-1]) if kept.size else 0
