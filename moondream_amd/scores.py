"""The per-decision outputs of generation and scoring as ONE record: every token's log-probability and rank and, with
k > 0, its decision's k alternatives.  ``Scores`` holds the device planes and is what the prefill, the decode loops and the
scorer hand each other; ``HostScores`` is its single copy on the host.  The packing of the words lives here alone."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np


@dataclass(frozen=True, eq=False)
class HostScores:
    """``Scores`` on the host: numpy planes (fp32 reinterpreted, never converted); ``extra``: the int32 tensors of the same copy."""

    logprob: Any
    rank: Any
    top_ids: Any = None
    top_logprobs: Any = None
    extra: tuple = ()

    def alternatives(self, index=()) -> list:
        """The decision at ``index`` (over the leading shape) as (token_id, logprob) pairs in rank order; an index that leaves
        leading dimensions gives nested lists of them.  The one place that builds the pairs."""
        def pairs(ids, lps):
            return [pairs(a, b) for a, b in zip(ids, lps)] if ids and isinstance(ids[0], list) else list(zip(ids, lps))

        return pairs(np.asarray(self.top_ids)[index].tolist(), np.asarray(self.top_logprobs)[index].tolist())


@dataclass(frozen=True, eq=False)
class Scores:
    """Device planes over a leading shape S ((B,), (T, B) or (R,)): ``logprob`` fp32 [*S], ``rank`` int32 [*S] and, with
    alternatives, ``top_ids`` int32 [*S, k] and ``top_logprobs`` fp32 [*S, k].  ``words``: the int32 allocation the planes
    tile, kept only by a record that covers all of it (such a record goes to the host in one direct copy)."""

    logprob: Any
    rank: Any
    top_ids: Any = None
    top_logprobs: Any = None
    words: Any = None

    @property
    def k(self) -> int:
        return 0 if self.top_ids is None else int(self.top_ids.shape[-1])

    def _planes(self) -> tuple:
        return tuple(p for p in (self.logprob, self.rank, self.top_ids, self.top_logprobs) if p is not None)

    @classmethod
    def new(cls, shape, k: int, device, fill: bool = False) -> "Scores":
        """One allocation of words [logprob | rank | top ids | top logprobs].  ``fill``: every plane says "never reached"
        (NaN, -1, -1, NaN), what the lockstep history keeps for the steps after an early exit."""
        import torch

        n = int(np.prod(shape))
        words = torch.empty(n * (2 + 2 * k), dtype=torch.int32, device=device)
        lp, rk, ti, tl = words.split([n, n, n * k, n * k])
        top = (ti.view(*shape, k), tl.view(torch.float32).view(*shape, k)) if k else ()
        s = cls(lp.view(torch.float32).view(*shape), rk.view(*shape), *top, words=words)
        if fill:
            for plane, value in zip(s._planes(), (float("nan"), -1, -1, float("nan"))):
                plane.fill_(value)
        return s

    def __getitem__(self, idx) -> "Scores":
        """The same leading index on every plane: a record of views, at the addresses slicing the planes by hand gives."""
        lp, rk, *top = (p[idx] for p in self._planes())
        whole = lp.shape == self.logprob.shape and lp.data_ptr() == self.logprob.data_ptr()
        return Scores(lp, rk, *top, words=self.words if whole else None)

    def copy_(self, other: "Scores") -> None:
        for mine, theirs in zip(self._planes(), other._planes()):
            mine.copy_(theirs)

    def chunk_fields(self) -> dict:
        """What ``DecodeChunk`` takes: its ``logprobs`` and ``topk`` fields."""
        return {"logprobs": (self.logprob, self.rank), "topk": (self.top_ids, self.top_logprobs) if self.k else None}

    def to_host(self, *extra) -> HostScores:
        """ONE device-to-host copy of ``extra`` (int32 tensors: the id history) and the record's words."""
        import torch

        tensors = extra + self._planes()
        direct = self.words is not None and not extra  # else packed with a single cat
        flat = (self.words if direct else torch.cat([t.view(torch.int32).reshape(-1) for t in tensors])).cpu().numpy()
        parts = [w.reshape(tuple(t.shape)).view(np.float32 if t.dtype == torch.float32 else np.int32)
                 for w, t in zip(np.split(flat, np.cumsum([t.numel() for t in tensors])[:-1]), tensors)]
        return HostScores(*parts[len(extra) :], extra=tuple(parts[: len(extra)]))
