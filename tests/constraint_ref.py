"""md_constrain_rows restated in numpy, on bf16 bit patterns (int16 arrays): the contract of include/moondream_hip.h,
one row at a time, nothing clever.  Returns new arrays; the arguments are left unchanged."""
import numpy as np

FREE, DEAD, FORBID = -1, -2, -3
NEG_INF = np.int16(-128)  # 0xFF80


def next_value(q, t, row_ptr, default_next, edge_tok, edge_next):
    """The next value of token ``t`` in state ``q`` of the table: its edge's, otherwise the default."""
    for e in range(int(row_ptr[q]), int(row_ptr[q + 1])):
        if int(edge_tok[e]) == t:
            return int(edge_next[e])
    return int(default_next[q])


def forbidden_columns(q, vocab, row_ptr, default_next, edge_tok, edge_next):
    """Boolean [vocab]: the tokens whose next value in state ``q`` is FORBID."""
    out = np.full(vocab, int(default_next[q]) == FORBID)
    for e in range(int(row_ptr[q]), int(row_ptr[q + 1])):
        v = int(edge_tok[e])
        if 0 <= v < vocab:
            out[v] = int(edge_next[e]) == FORBID
    return out


def constrain_rows(logits, vocab, tokens_in, slots, slot0, state, row_ptr, default_next, edge_tok, edge_next, state_cap):
    """-> (logits bits int16 [batch, ld], state int32 [n_slots]) after one launch.  ``tokens_in`` / ``slots`` may be None."""
    logits, state = np.array(logits, copy=True), np.array(state, dtype=np.int32, copy=True)
    table = (row_ptr, default_next, edge_tok, edge_next)
    for r in range(logits.shape[0]):
        s = int(slots[r]) if slots is not None else slot0 + r
        if s < 0:
            continue
        q = int(state[s])
        if q < 0:
            continue
        if q >= state_cap:
            state[s] = DEAD
            continue
        if tokens_in is not None:
            t = int(tokens_in[r])
            q = next_value(q, t, *table)
            if t < 0 or t >= vocab or q == FORBID or q >= state_cap or q < FORBID:
                q = DEAD
            state[s] = q
            if q < 0:
                continue
        logits[r, :vocab][forbidden_columns(q, vocab, *table)] = NEG_INF
    return logits, state
