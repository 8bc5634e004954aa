"""Beam search restated on the host in numpy fp32: the group phase of md_beam_select (merge, walk, pool, done rule, slot
hand-off), the check of md_kv_copy_tail's contract, and the host side (finalisation at max_tokens, backtracking).  The
per-row candidates are an INPUT: md_topk_logprobs' own output on the same logits, which its own tests pin."""
import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)


def inv_norm_table(n, length_penalty):
    """inv_norm[k] = float32(1 / k ** length_penalty) computed in float64; entry 0 is 1."""
    k = np.arange(n, dtype=np.float64)
    k[0] = 1.0
    return (1.0 / k ** float(length_penalty)).astype(F32)


def pool_insert(pool, w, h, s, parent, step):
    """``pool``: list of (h, s, parent, step), at most ``w``.  Appended while not full; otherwise it replaces the entry of
    lowest score -- among equal scores the highest index -- and only if h is strictly greater."""
    if len(pool) < w:
        pool.append((F32(h), F32(s), int(parent), int(step)))
        return
    at = 0
    for q in range(1, w):
        if pool[q][0] <= pool[at][0]:
            at = q
    if F32(h) > pool[at][0]:
        pool[at] = (F32(h), F32(s), int(parent), int(step))


def new_state(groups, w, prefix_len, n_prefix_slots=None):
    """The caller-owned state before the first decision.  Row r owns slots base + 2r and base + 2r + 1."""
    rows = groups * w
    base = groups if n_prefix_slots is None else n_prefix_slots
    own = (base + 2 * np.arange(rows, dtype=np.int32)[:, None] + np.arange(2, dtype=np.int32)[None, :]).astype(np.int32)
    cum = np.full(rows, NEG_INF, dtype=F32)
    cum[::w] = 0.0
    return dict(cum=cum, cur=own[:, 0].copy(), own=own, len=np.zeros(groups, np.int32), done=np.zeros(groups, np.int32),
                prefix_len=np.asarray(prefix_len, np.int32).copy(), pool_n=np.zeros(groups, np.int32),
                pool_score=np.zeros((groups, w), F32), pool_sum=np.zeros((groups, w), F32),
                pool_parent=np.zeros((groups, w), np.int32), pool_step=np.zeros((groups, w), np.int32))


def select(state, cand_ids, cand_lp, w, beams_in, eos_id, early_stopping, inv_norm, prev_out=None):
    """One md_beam_select call after its row phase: ``cand_ids`` / ``cand_lp`` [rows][2w] are md_topk_logprobs(k = 2w)'s
    entries of every beam's logits row.  Returns (new state, out) with out = dict(tokens, parent, src, dst, from, to), each
    int32 [rows]; the rows of a done group keep ``prev_out``'s values (nothing of it is written)."""
    st = {k: np.array(v, copy=True) for k, v in state.items()}
    groups = len(st["len"])
    rows = groups * w
    k2 = 2 * w
    names = ("tokens", "parent", "src", "dst", "from", "to")
    out = {n: (np.array(prev_out[n], copy=True) if prev_out is not None else np.full(rows, -7, np.int32)) for n in names}
    for g in range(groups):
        if state["done"][g]:
            continue
        r0 = g * w
        cum = [state["cum"][r0 + j] if j < beams_in else NEG_INF for j in range(w)]
        cur = [int(state["cur"][r0 + j]) for j in range(w)]
        ln, p = int(state["len"][g]), int(state["prefix_len"][g])
        cands = []
        for j in range(w):
            if cum[j] == NEG_INF:
                continue
            for i in range(k2):
                if cand_ids[r0 + j][i] < 0:
                    continue
                cands.append((F32(F32(cum[j]) + F32(cand_lp[r0 + j][i])), j, i, int(cand_ids[r0 + j][i])))
        cands.sort(key=lambda c: (-float(c[0]), c[1], c[2]))  # s descending, beam ascending, entry ascending
        pool = [(st["pool_score"][g][q], st["pool_sum"][g][q], int(st["pool_parent"][g][q]), int(st["pool_step"][g][q]))
                for q in range(int(st["pool_n"][g]))]
        norm1 = F32(inv_norm[min(ln + 1, len(inv_norm) - 1)])
        live = []
        for wi, (s, j, i, tok) in enumerate(cands[:k2]):
            if eos_id >= 0 and tok == eos_id:
                if wi < w:
                    pool_insert(pool, w, F32(s * norm1), s, j, ln)
                continue
            if len(live) < w:
                live.append((tok, j, s))
        done = len(live) == 0
        if not done and len(pool) == w:
            lowest = min(e[0] for e in pool)
            done = bool(early_stopping) or bool(F32(live[0][2] * norm1) <= lowest)
        st["len"][g] = ln + 1
        st["done"][g] = int(done)
        st["pool_n"][g] = len(pool)
        for q, e in enumerate(pool):
            st["pool_score"][g][q], st["pool_sum"][g][q], st["pool_parent"][g][q], st["pool_step"][g][q] = e
        for n in range(w):
            r = r0 + n
            is_live = n < len(live)
            out["tokens"][r] = live[n][0] if is_live else 0
            out["parent"][r] = live[n][1] if is_live else -1
            st["cum"][r] = live[n][2] if is_live else NEG_INF
            c = s_ = d = -1
            if is_live and not done:
                par = live[n][1]
                if par == n and cur[n] >= 0:
                    c = s_ = d = cur[n]
                else:
                    o0, o1 = (int(x) for x in state["own"][r])
                    c = d = o1 if cur[n] == o0 else o0
                    s_ = cur[par]
            st["cur"][r] = c
            out["src"][r], out["dst"][r], out["from"][r], out["to"][r] = s_, d, p, p + ln
    return st, out


def check_copy_contract(out):
    """md_kv_copy_tail's caller contract over one call's rows: no dst of a live row is any live row's src, live dsts are
    distinct."""
    live = [r for r in range(len(out["src"])) if out["dst"][r] >= 0 and out["src"][r] >= 0 and out["src"][r] != out["dst"][r]
            and out["to"][r] > out["from"][r]]
    dsts = [int(out["dst"][r]) for r in live]
    srcs = {int(out["src"][r]) for r in live}
    assert len(set(dsts)) == len(dsts), ("two live rows write one slot", dsts)
    assert not (set(dsts) & srcs), ("a slot is read and written in one launch", dsts, sorted(srcs))


def backtrack(tokens, parents, beam, step):
    """The ``step`` tokens of the hypothesis that sits in beam ``beam`` after decision step - 1: ``tokens[t]`` /
    ``parents[t]`` int [w] are decision t's planes of one group."""
    ids = []
    j = int(beam)
    for t in range(int(step) - 1, -1, -1):
        ids.append(int(tokens[t][j]))
        j = int(parents[t][j])
    return ids[::-1]


def finalize(state, g, w, tokens, parents, inv_norm, n_return):
    """The ``n_return`` best hypotheses of group g: its pool, joined -- when the group is not done -- by every live beam as
    an unfinished hypothesis of score cum * inv_norm[len] under the same insert rule.  Returns a list of (ids, score,
    logprob, finished), best first (score descending, then pool order)."""
    ln = int(state["len"][g])
    entries = [(state["pool_score"][g][q], state["pool_sum"][g][q], int(state["pool_parent"][g][q]), int(state["pool_step"][g][q]),
                True) for q in range(int(state["pool_n"][g]))]
    if not state["done"][g]:
        norm = F32(inv_norm[min(ln, len(inv_norm) - 1)])
        for j in range(w):
            c = F32(state["cum"][g * w + j])
            if c == NEG_INF:
                continue
            h = F32(c * norm)
            if len(entries) < w:
                entries.append((h, c, j, ln, False))
                continue
            at = 0
            for q in range(1, w):
                if entries[q][0] <= entries[at][0]:
                    at = q
            if h > entries[at][0]:
                entries[at] = (h, c, j, ln, False)
    order = sorted(range(len(entries)), key=lambda q: (-float(entries[q][0]), q))
    return [(backtrack(tokens, parents, entries[q][2], entries[q][3]), F32(entries[q][0]), F32(entries[q][1]), entries[q][4])
            for q in order[:n_return]]
