"""The host side of beam search (``MoondreamModel.batch_beam_search_ids``): the argument checks, the length-normalisation
table the device multiplies by, and what happens after the last chunk -- live beams of unfinished requests enter the pool,
hypotheses are read back through the parent planes.  numpy fp32 throughout, so that every score is the bits a restatement
of md_beam_select's rules gives.  No torch here."""
from __future__ import annotations

import math
import operator
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

BEAM_MAX = 16  # MD_BEAM_MAX of include/moondream_hip.h
BEAM_SETTINGS = ("num_beams", "length_penalty", "early_stopping")
F32 = np.float32


@dataclass(frozen=True)
class Hypothesis:
    """One result of a beam search: ``ids`` without the eos, ``score`` = ``logprob`` normalised by the length penalty
    (what hypotheses are ranked by), ``logprob`` the raw sum of the tokens' log-probabilities (the eos's included when
    ``finished``), ``finished``: it ended in the eos (False: cut at ``max_tokens``)."""

    ids: List[int]
    score: float
    logprob: float
    finished: bool


def check_beams(num_beams, num_return_sequences=1, length_penalty=1.0, early_stopping=False) -> Tuple[int, int, float, bool]:
    """The beam arguments -> (num_beams, num_return_sequences, length_penalty, early_stopping).  ValueError for a
    ``num_beams`` that is not an integer in 1 .. BEAM_MAX (a bool is none), a ``num_return_sequences`` outside
    1 .. num_beams, a ``length_penalty`` that is not finite, an ``early_stopping`` that is not a bool: host values only,
    before any GPU work."""
    def index(x):
        try:
            return -1 if isinstance(x, bool) else operator.index(x)
        except TypeError:
            return -1

    w = index(num_beams)
    if not 1 <= w <= BEAM_MAX:
        raise ValueError(f"num_beams must be an integer in 1 .. {BEAM_MAX}, not {num_beams!r}")
    n = index(num_return_sequences)
    if not 1 <= n <= w:
        raise ValueError(f"num_return_sequences must be an integer in 1 .. num_beams ({w}), not {num_return_sequences!r}")
    try:
        lp = float("nan") if isinstance(length_penalty, (bool, str)) else float(length_penalty)
    except (TypeError, ValueError):
        lp = float("nan")
    if not math.isfinite(lp):
        raise ValueError(f"length_penalty must be a finite number, not {length_penalty!r}")
    if not isinstance(early_stopping, bool):
        raise ValueError(f"early_stopping must be a bool, not {early_stopping!r}")
    return w, n, lp, early_stopping


def beams_of(settings: Optional[dict]) -> Optional[Tuple[int, float, bool]]:
    """The beam entries of a ``settings`` dict, checked -> (num_beams, length_penalty, early_stopping), or None when
    ``num_beams`` is absent, None or 1: the call as it is without beam search (the other two entries are then checked and
    unused)."""
    st = settings or {}
    w, _, lp, es = check_beams(1 if st.get("num_beams") is None else st["num_beams"], 1, st.get("length_penalty", 1.0),
                               st.get("early_stopping", False))
    return None if w == 1 else (w, lp, es)


def refuse_beams(settings: Optional[dict], where: str) -> None:
    """An entry point that does not serve beam search: ValueError naming ``where`` when ``settings`` asks for more than
    one beam (and ``check_beams``' errors for a value that is none)."""
    if beams_of(settings) is not None:
        raise ValueError(f"num_beams > 1 (beam search) is not served by {where}")


def inv_norm_table(n: int, length_penalty: float) -> np.ndarray:
    """fp32 [n]: entry k = float32(1 / k ** length_penalty), computed in float64 (entry 0: 1) -- the table md_beam_select
    multiplies a hypothesis's summed log-probability by."""
    k = np.arange(n, dtype=np.float64)
    k[0] = 1.0
    return (1.0 / k ** float(length_penalty)).astype(F32)


def backtrack(tokens: np.ndarray, parents: np.ndarray, beam: int, step: int) -> List[int]:
    """The ``step`` tokens of the hypothesis in beam ``beam`` after decision ``step - 1``: ``tokens[t]`` / ``parents[t]``
    (int [W]) are decision t's planes of one request."""
    ids, j = [], int(beam)
    for t in range(int(step) - 1, -1, -1):
        ids.append(int(tokens[t][j]))
        j = int(parents[t][j])
    return ids[::-1]


def pool_insert(pool: list, w: int, entry: tuple) -> None:
    """md_beam_select's insert rule on a host pool of (score, ...) tuples: appended while fewer than ``w``; otherwise it
    replaces the entry of lowest score -- among equal scores the highest index -- and only if its score is strictly greater."""
    if len(pool) < w:
        pool.append(entry)
        return
    at = 0
    for q in range(1, w):
        if pool[q][0] <= pool[at][0]:
            at = q
    if entry[0] > pool[at][0]:
        pool[at] = entry


def finalize(w: int, n_return: int, length: int, done: bool, cum: np.ndarray, pool_n: int, pool_score: np.ndarray,
             pool_sum: np.ndarray, pool_parent: np.ndarray, pool_step: np.ndarray, tokens: np.ndarray, parents: np.ndarray,
             inv_norm: np.ndarray) -> List[Hypothesis]:
    """One request's hypotheses, best first, from what the device left: its pool (``pool_*`` [W], ``pool_n`` valid), and --
    when the request is not ``done`` (it ran into ``max_tokens``) -- every live beam (``cum`` [W] != -inf) as an unfinished
    hypothesis of score cum * inv_norm[length] under the pool's insert rule.  ``tokens`` / ``parents`` [steps, W]: the
    request's planes.  Order: score descending, equal scores in pool order."""
    pool = [(F32(pool_score[q]), F32(pool_sum[q]), int(pool_parent[q]), int(pool_step[q]), True) for q in range(int(pool_n))]
    if not done:
        norm = F32(inv_norm[min(int(length), len(inv_norm) - 1)])
        for j in range(w):
            c = F32(cum[j])
            if c != F32(-np.inf):
                pool_insert(pool, w, (F32(c * norm), c, j, int(length), False))
    order = sorted(range(len(pool)), key=lambda q: (-float(pool[q][0]), q))
    return [Hypothesis(backtrack(tokens, parents, pool[q][2], pool[q][3]), float(pool[q][0]), float(pool[q][1]), pool[q][4])
            for q in order[:n_return]]
