"""Host-side planning of batched generation with a SHARED image prefix (md_text_forward_shared / md_decode_step_shared).

Rows whose image is the same object -- the same ``EncodedImage`` or the same PIL image, by identity -- read their image prefix
from one KV slot instead of a copy in each row's own slot.  The P distinct images take prefix slots [0, P), the B rows take
their own slots [P, P + B).  Pure Python: no GPU, no torch.
"""
from dataclasses import dataclass
from typing import Any, List, Sequence, Tuple


@dataclass
class SharedPlan:
    distinct: List[Any]            # the P distinct image objects, in order of first appearance; image k -> prefix slot k
    order: List[int]               # order[r] = caller index of row r (rows sorted by prompt length, then image, then caller)
    own_slots: List[int]           # own_slots[r] = P + r
    prefix_slots: List[int]        # prefix_slots[r] = prefix slot of row r's image
    groups: List[Tuple[int, int]]  # [r0, r1): the rows of one prompt length (one prefill launch each)
    copy_rank: List[int]           # copy_rank[r] = row of the same sequence in the copy path's order (stable sort by length)

    @property
    def n_slots(self) -> int:
        return len(self.distinct) + len(self.order)


def plan_shared_prefix(images: Sequence[Any], prompt_lens: Sequence[int]) -> SharedPlan:
    """Rows of one prompt length form one prefill group; inside it, each image's rows are contiguous (so that a decode
    workgroup's consecutive rows tend to share a prefix slot).  Row order changes memory traffic, never a row's bits."""
    if len(images) != len(prompt_lens) or not images:
        raise ValueError("need one prompt per image and at least one row")
    index = {}
    distinct: List[Any] = []
    img_of = []
    for im in images:
        k = index.get(id(im))
        if k is None:
            k = index[id(im)] = len(distinct)
            distinct.append(im)
        img_of.append(k)
    b, p = len(images), len(distinct)
    order = sorted(range(b), key=lambda i: (prompt_lens[i], img_of[i], i))
    copy_order = sorted(range(b), key=lambda i: prompt_lens[i])  # _prepare_sequences' row order
    copy_row = {src: r for r, src in enumerate(copy_order)}
    groups = []
    r0 = 0
    while r0 < b:
        r1 = r0
        while r1 < b and prompt_lens[order[r1]] == prompt_lens[order[r0]]:
            r1 += 1
        groups.append((r0, r1))
        r0 = r1
    return SharedPlan(distinct=distinct, order=order, own_slots=[p + r for r in range(b)],
                      prefix_slots=[img_of[i] for i in order], groups=groups, copy_rank=[copy_row[i] for i in order])


def check_shared_table(own_slots: Sequence[int], prefix_slots: Sequence[int], prefix_len: Sequence[int],
                       pos0: Sequence[int], n_slots: int) -> None:
    """The caller contract of md_text_forward_shared, on the host: slots in range, every row writes at or after the end of
    its shared prefix, and no row's own slot is another row's prefix slot (or another row's own slot)."""
    if not (len(own_slots) == len(prefix_slots) == len(prefix_len) == len(pos0)):
        raise ValueError("slot / prefix tables of different lengths")
    own = set()
    for s in own_slots:
        if not 0 <= s < n_slots:
            raise ValueError(f"own slot {s} outside [0, {n_slots})")
        if s in own:
            raise ValueError(f"two rows write slot {s}")
        own.add(s)
    for s, ps, pl, p0 in zip(own_slots, prefix_slots, prefix_len, pos0):
        if ps < 0:
            continue
        if ps >= n_slots:
            raise ValueError(f"prefix slot {ps} outside [0, {n_slots})")
        if ps in own:
            raise ValueError(f"prefix slot {ps} is also a row's own slot")
        if p0 < pl:
            raise ValueError(f"row of slot {s} writes position {p0} inside its shared prefix of {pl} positions")
