"""A plain numpy reference of the token lift and its compaction (moondream_amd/grammar.py, csrc/automaton.hip): what the
device computes, written position by position over the whole (state, token) matrix instead of walk by walk.  Shared by
the CPU and GPU grammar tests and by tools/bench_regex_compile.py; not a test module itself."""
import numpy as np

FREE, FORBID = -1, -3


def lift(trans, accept, vocab_bytes, eos_id, forbidden):
    """next int32 [S][V]: column v is the state after token v's bytes from every state, FORBID once dead; FORBID for an
    empty or forbidden token; the eos column is FREE at accepting states and FORBID elsewhere."""
    trans, accept = np.asarray(trans, dtype=np.int64), np.asarray(accept, dtype=bool)
    s, v = trans.shape[0], len(vocab_bytes)
    lens = np.array([len(b) for b in vocab_bytes], dtype=np.int64)
    longest = int(lens.max()) if v else 0
    padded = np.zeros((v, max(longest, 1)), dtype=np.int64)
    for i, b in enumerate(vocab_bytes):
        padded[i, : len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    dead_row = np.full((1, 256), s, dtype=np.int64)  # state s: the dead sink, so that indexing never sees -1
    table = np.concatenate([np.where(trans >= 0, trans, s), dead_row], axis=0)
    cur = np.repeat(np.arange(s, dtype=np.int64)[:, None], v, axis=1)
    for i in range(longest):
        cols = np.flatnonzero(lens > i)
        cur[:, cols] = table[cur[:, cols], padded[cols, i][None, :]]
    out = np.where(cur == s, FORBID, cur)
    out[:, (lens == 0) | (np.asarray(forbidden) != 0)] = FORBID
    out[:, eos_id] = np.where(accept, FREE, FORBID)
    return out.astype(np.int32)


def compact(nxt):
    """(row_ptr, default_next, edge_tok, edge_next) of a next matrix: the default is each row's most frequent value, ties to
    the smallest; the edges are the other columns, ascending."""
    s, v = nxt.shape
    default = np.zeros(s, dtype=np.int32)
    toks, vals, ptr = [], [], [0]
    for q in range(s):
        values, counts = np.unique(nxt[q], return_counts=True)  # ascending values: argmax takes the smallest of a tie
        default[q] = values[np.argmax(counts)]
        cols = np.flatnonzero(nxt[q] != default[q])
        toks.append(cols)
        vals.append(nxt[q, cols])
        ptr.append(ptr[-1] + cols.size)
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)
    return np.asarray(ptr, dtype=np.int32), default, cat(toks), cat(vals)


def prune(row_ptr, default_next, edge_tok, edge_next):
    """Keep the states some token sequence reaches from state 0, renumbered in ascending order of their old ids."""
    s = len(default_next)
    seen, stack = {0}, [0]
    while stack:
        q = stack.pop()
        for n in list(edge_next[row_ptr[q] : row_ptr[q + 1]]) + [default_next[q]]:
            if n >= 0 and int(n) not in seen:
                seen.add(int(n))
                stack.append(int(n))
    old = sorted(seen)
    new = {q: i for i, q in enumerate(old)}
    re = lambda n: new[int(n)] if n >= 0 else int(n)
    ptr, dflt, toks, vals = [0], [], [], []
    for q in old:
        lo, hi = row_ptr[q], row_ptr[q + 1]
        toks += [int(t) for t in edge_tok[lo:hi]]
        vals += [re(n) for n in edge_next[lo:hi]]
        dflt.append(re(default_next[q]))
        ptr.append(len(toks))
    as32 = lambda x: np.asarray(x, dtype=np.int32)
    return as32(ptr), as32(dflt), as32(toks), as32(vals)


def compile_arrays(dfa, vocab_bytes, eos_id, forbidden_ids=()):
    """The four arrays ``compile_regex`` must return for ``dfa`` over ``vocab_bytes``."""
    forbidden = np.zeros(len(vocab_bytes), dtype=np.uint8)
    forbidden[list(forbidden_ids)] = 1
    return prune(*compact(lift(dfa.trans, dfa.accept, vocab_bytes, eos_id, forbidden)))


def states_of(arrays):
    """The arrays as ``TokenAutomaton.from_states``' argument: ``[({token: next}, default), ...]``."""
    row_ptr, default_next, edge_tok, edge_next = arrays
    return [({int(t): int(n) for t, n in zip(edge_tok[row_ptr[q] : row_ptr[q + 1]], edge_next[row_ptr[q] : row_ptr[q + 1]])},
             int(default_next[q])) for q in range(len(default_next))]


def synthetic_vocab(v, seed, alphabet=b"0123456789.-yesnomaybtru{}[]\":,", longest=6):
    """``v`` tokens: the 256 single bytes first (as far as ``v`` reaches), then seeded random strings over ``alphabet``,
    among them zero-length tokens, tokens with bytes >= 0x80 and one 128-byte token."""
    rng = np.random.default_rng(seed)
    out = [bytes([b]) for b in range(min(v, 256))]
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    while len(out) < v:
        i = len(out)
        if i % 97 == 5:
            out.append(b"")
        elif i % 89 == 7:
            out.append(bytes(rng.integers(0x80, 0x100, size=int(rng.integers(1, 4))).astype(np.uint8)))
        elif i == 300:
            out.append(bytes(rng.choice(letters[:10], size=128)))
        else:
            out.append(bytes(rng.choice(letters, size=int(rng.integers(2, longest + 1)))))
    return out
