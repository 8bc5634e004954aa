"""Host-side planning of batched generation with a SHARED image prefix (md_text_forward_shared / md_decode_step_shared).

Rows whose image is the same object -- the same ``EncodedImage`` or the same PIL image, by identity -- read their image prefix
from one KV slot instead of a copy in each row's own slot.  The P distinct images take prefix slots [0, P), the B rows take
their own slots [P, P + B).  Pure Python: no GPU, no torch.
"""
from dataclasses import dataclass
from typing import Any, List, Sequence, Tuple


@dataclass
class RowPlan:
    """The rows of one batched call: which images are placed into which KV slots, and the rows' order, slots and prefill
    groups.  One record for both routings (``plan_rows``)."""

    placed: List[Any]              # the images to place, image k -> slot k: the P distinct ones (shared), every row's own (copy)
    order: List[int]               # order[r] = caller index of row r (rows sorted by prompt length; shared: then image, caller)
    own_slots: List[int]           # own_slots[r]: P + r (shared), r (copy)
    prefix_slots: List[int]        # prefix_slots[r] = prefix slot of row r's image; copy: [] (no prefix table)
    groups: List[Tuple[int, int]]  # [r0, r1): the rows of one prompt length (one prefill launch each)
    copy_rank: List[int]           # copy_rank[r] = row of the same sequence in the copy path's order (stable sort by length)

    @property
    def n_slots(self) -> int:
        return self.own_slots[-1] + 1

    @property
    def distinct(self) -> List[Any]:
        """``placed`` under the shared routing's name: the P distinct image objects, in order of first appearance."""
        return self.placed


def plan_rows(images: Sequence[Any], prompt_lens: Sequence[int], share: bool) -> RowPlan:
    """Rows of one prompt length form one prefill group.  ``share``: the P distinct images (by identity, in order of first
    appearance) take prefix slots [0, P) and the rows their own slots [P, P + B); inside a group each image's rows are
    contiguous (so that a decode workgroup's consecutive rows tend to share a prefix slot).  Otherwise (the copy path) row
    r's image goes into row r's slot r, rows in stable order of prompt length.  Row order changes memory traffic, never a
    row's bits."""
    if len(images) != len(prompt_lens) or not images:
        raise ValueError("need one prompt per image and at least one row")
    b = len(images)
    copy_order = sorted(range(b), key=lambda i: prompt_lens[i])
    if share:
        index = {}
        placed: List[Any] = []
        img_of = []
        for im in images:
            k = index.get(id(im))
            if k is None:
                k = index[id(im)] = len(placed)
                placed.append(im)
            img_of.append(k)
        order = sorted(range(b), key=lambda i: (prompt_lens[i], img_of[i], i))
        prefix_slots = [img_of[i] for i in order]
    else:
        order, placed, prefix_slots = copy_order, [images[i] for i in copy_order], []
    copy_row = {src: r for r, src in enumerate(copy_order)}
    groups = []
    r0 = 0
    while r0 < b:
        r1 = r0
        while r1 < b and prompt_lens[order[r1]] == prompt_lens[order[r0]]:
            r1 += 1
        groups.append((r0, r1))
        r0 = r1
    p = len(placed) if share else 0
    return RowPlan(placed=placed, order=order, own_slots=[p + r for r in range(b)], prefix_slots=prefix_slots,
                      groups=groups, copy_rank=[copy_row[i] for i in order])


def plan_shared_prefix(images: Sequence[Any], prompt_lens: Sequence[int]) -> RowPlan:
    return plan_rows(images, prompt_lens, share=True)


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
