"""Spatial references in batched queries, the host side: a point ``(x, y)`` or a box ``(x0, y0, x1, y1)`` in front of a
question (reference: moondream.py:577-604 builds the ids, region.py:96-136 encodes, moondream.py:293-301 places).  A point
takes two coordinate placeholders in the prompt, a box two coordinates (its centre) and one size.  This module is the only
place that knows the layout: the checks (``check_spatial_refs``), the placeholder ids (``placeholders``) and the record
of every reference TOKEN of a call (``SpatialRecord``), whose table md_spatial_ref_embed reads on the device -- one
descriptor per token, addressed by the POSITION of the placeholder it replaces, never by matching ids.  Host only: numpy
and CPU torch (for the reference's own float -> bf16 conversion), no kernels.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

KIND_COORD, KIND_SIZE = 0, 1  # md_spatial_ref_embed's descriptor kinds
Refs = List[Tuple[float, ...]]


def refs_of(settings: Optional[dict], spatial_refs=None):
    """A call's references: its ``spatial_refs`` argument, or ``settings["spatial_refs"]`` (the form ``query_many``
    takes them in: its three-parameter signature is part of its contract).  ValueError when both are given."""
    in_settings = (settings or {}).get("spatial_refs")
    if spatial_refs is not None and in_settings is not None:
        raise ValueError("spatial_refs given both as an argument and in settings")
    return in_settings if spatial_refs is None else spatial_refs


def _is_off(spatial_refs) -> bool:
    """None, or a per-row list whose every entry is None or empty: the call without the argument."""
    if spatial_refs is None:
        return True
    return isinstance(spatial_refs, (list, tuple)) and all(r is None or (isinstance(r, (list, tuple)) and len(r) == 0)
                                                           for r in spatial_refs)


def refuse_spatial_refs(spatial_refs, where: str) -> None:
    """An entry point that does not serve spatial references: ValueError naming ``where`` when it is given some."""
    if not _is_off(spatial_refs):
        raise ValueError(f"spatial_refs are not served by {where}")


def check_refs(refs) -> Refs:
    """One row's references, checked: a list of 2-tuples (points) / 4-tuples (boxes) of finite numbers.  Ranges are not
    checked (the reference checks none)."""
    if not isinstance(refs, (list, tuple)):
        raise ValueError(f"spatial_refs of a row: a list of (x, y) / (x0, y0, x1, y1) tuples, not {refs!r}")
    out = []
    for ref in refs:
        if not isinstance(ref, (list, tuple)) or len(ref) not in (2, 4):
            raise ValueError(f"a spatial ref is a point (x, y) or a box (x0, y0, x1, y1), not {ref!r}")
        vals = []
        for v in ref:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"a spatial ref holds finite numbers, not {v!r} (in {ref!r})")
            vals.append(float(v))
        out.append(tuple(vals))
    return out


def check_spatial_refs(spatial_refs, n_rows: int, has_image: Sequence[bool], questions: Sequence[Sequence[int]],
                       coord_id: int, size_id: int, has_region: bool) -> Optional[List[Refs]]:
    """``spatial_refs`` of a batch of ``n_rows`` rows, checked before any GPU work -> one list of refs per row (empty: the
    row has none), or None when no row has any (the call without the argument).  ``questions[i]``: the ids of row i's own
    question.  ValueError: not one entry per row; an entry that is no list of 2- / 4-tuples of finite numbers; refs on a
    row without an image; refs on a row whose question itself contains ``coord_id`` or ``size_id`` (the reference's
    placement by id would misplace there).  NotImplementedError: refs on a checkpoint without a region head."""
    if spatial_refs is None:
        return None
    if not isinstance(spatial_refs, (list, tuple)) or len(spatial_refs) != n_rows:
        raise ValueError(f"spatial_refs: one entry per row ({n_rows}): None, or a list of points / boxes")
    rows = [[] if r is None else check_refs(r) for r in spatial_refs]
    if not any(rows):
        return None
    if not has_region:
        raise NotImplementedError("spatial_refs need a region head: checkpoint has no region head")
    for i, refs in enumerate(rows):
        if not refs:
            continue
        if not has_image[i]:
            raise ValueError("spatial_refs can only be used with an image.")
        if coord_id in questions[i] or size_id in questions[i]:
            raise ValueError(f"row {i}: a question whose tokens contain the coordinate / size placeholder ids "
                             f"({coord_id}, {size_id}) is not served with spatial_refs")
    return rows


def placeholders(refs: Refs, coord_id: int, size_id: int) -> List[int]:
    """The placeholder ids of one row's refs: [coord, coord] per point, [coord, coord, size] per box (moondream.py:577-584)."""
    out: List[int] = []
    for ref in refs:
        out += [coord_id, coord_id] if len(ref) == 2 else [coord_id, coord_id, size_id]
    return out


def spatial_prompt_ids(head: Sequence[int], refs: Refs, tail: Sequence[int], coord_id: int, size_id: int) -> List[int]:
    """``head + placeholders + tail``: ``query``'s prompt (moondream.py:586-604; head = the template's prefix, tail =
    question + suffix (+ suffix or the thinking token))."""
    return list(head) + placeholders(refs, coord_id, size_id) + list(tail)


def ref_values(refs: Refs) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The bf16 tensors ``encode_spatial_refs`` builds from one row's refs (region.py:96-136): coordinates [2 * n_refs]
    -- a point's x, y, a box's centre ``(a + b) / 2`` -- and sizes [n_boxes, 2], ``b - a`` (None without a box); Python
    float arithmetic, then ONE rounding to bf16."""
    coords, sizes = [], []
    for ref in refs:
        if len(ref) == 2:
            coords += [ref[0], ref[1]]
        else:
            coords += [(ref[0] + ref[2]) / 2, (ref[1] + ref[3]) / 2]
            sizes.append([ref[2] - ref[0], ref[3] - ref[1]])
    return torch.tensor(coords, dtype=torch.bfloat16), (torch.tensor(sizes, dtype=torch.bfloat16) if sizes else None)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().astype(np.int32) & 0xFFFF


@dataclass(frozen=True)
class SpatialRecord:
    """Every reference token of a call.  ``tokens`` int32 [N, 5], in row order: (row, position in the row's prompt, kind,
    value bits, value bits) -- a coordinate's second value is 0; ``row_ptr`` int64 [rows + 1]: row r's tokens are
    ``tokens[row_ptr[r] : row_ptr[r + 1]]``; ``prompt_len`` [rows]: every row's prompt length, placeholders included."""

    tokens: np.ndarray
    row_ptr: np.ndarray
    prompt_len: Tuple[int, ...]

    @classmethod
    def build(cls, rows: Sequence[Refs], head_len, prompt_len: Sequence[int]) -> "SpatialRecord":
        """``rows[r]``: row r's checked refs, whose placeholders start at position ``head_len`` of its prompt (one int,
        or one per row)."""
        toks, ptr = [], [0]
        heads = [head_len] * len(rows) if isinstance(head_len, int) else list(head_len)
        for r, refs in enumerate(rows):
            if refs:
                c, s = ref_values(refs)
                cb, sb = _bits(c), (_bits(s) if s is not None else None)
                pos, ci, si = heads[r], 0, 0
                for ref in refs:
                    toks += [(r, pos, KIND_COORD, cb[ci], 0), (r, pos + 1, KIND_COORD, cb[ci + 1], 0)]
                    ci, pos = ci + 2, pos + 2
                    if len(ref) == 4:
                        toks.append((r, pos, KIND_SIZE, sb[si, 0], sb[si, 1]))
                        si, pos = si + 1, pos + 1
                if pos > prompt_len[r]:
                    raise ValueError(f"row {r}: the placeholders end at {pos}, beyond its prompt of {prompt_len[r]} ids")
            ptr.append(len(toks))
        return cls(np.asarray(toks, dtype=np.int32).reshape(-1, 5), np.asarray(ptr, dtype=np.int64),
                   tuple(int(t) for t in prompt_len))

    @property
    def n_rows(self) -> int:
        return len(self.prompt_len)

    def __len__(self) -> int:
        return int(self.tokens.shape[0])

    def reorder(self, order: Sequence[int]) -> "SpatialRecord":
        """The record of the rows ``order`` (new row j = old row order[j]): the caller's order -> the plan's slot order."""
        parts, ptr = [], [0]
        for j, i in enumerate(order):
            t = self.tokens[self.row_ptr[i] : self.row_ptr[i + 1]].copy()
            t[:, 0] = j
            parts.append(t)
            ptr.append(ptr[-1] + len(t))
        toks = np.concatenate(parts) if parts else self.tokens[:0]
        return SpatialRecord(toks.reshape(-1, 5), np.asarray(ptr, dtype=np.int64), tuple(self.prompt_len[i] for i in order))

    def table(self, lead: int = 0) -> np.ndarray:
        """md_spatial_ref_embed's descriptors, int32 [N, 4]: (dst, kind, value bits, value bits), with ``dst`` the token's
        row in a tensor that holds row r's ``lead + prompt_len[r]`` embedding rows behind those of rows 0 .. r-1 of ITS
        length: ``dst = r * (lead + prompt_len[r]) + lead + position``.  A pass over rows [r0, r1) of one length T reads
        ``table[row_ptr[r0] : row_ptr[r1]]`` with ``dst0 = r0 * (lead + T)`` (``dst0_of``).  ``lead``: the positions in
        front of the prompt in the pass's tensor (the fused prefill's [bos | image])."""
        out = np.empty((len(self), 4), dtype=np.int32)
        if len(self):
            r = self.tokens[:, 0].astype(np.int64)
            stride = np.asarray(self.prompt_len, dtype=np.int64)[r] + lead
            dst = r * stride + lead + self.tokens[:, 1]
            if dst.max() >= 2 ** 31:
                raise ValueError("spatial_refs: the batch's embedding rows do not fit a 32-bit row index")
            out[:, 0] = dst
            out[:, 1:] = self.tokens[:, 2:]
        return out

    def span(self, r0: int, r1: int) -> Tuple[int, int]:
        """The descriptors of rows [r0, r1): [i0, i1) of the table."""
        return int(self.row_ptr[r0]), int(self.row_ptr[r1])

    def dst0_of(self, r0: int, lead: int = 0) -> int:
        return r0 * (lead + self.prompt_len[r0])
