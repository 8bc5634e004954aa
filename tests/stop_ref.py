"""The stop rule by its naive definition, independent of any automaton: concatenate the generated tokens' bytes and, for
each end offset in ascending order, take the longest stop string the text up to there ends with; stop ids are judged per
token.  ``stop_ref`` -> ``(at, keep, which)`` as md_stop_rows and ``moondream_amd.stop.walk`` define them."""
from typing import Optional, Sequence, Tuple


def stop_ref(token_bytes: Sequence[bytes], strings: Sequence[bytes], tokens: Optional[Sequence[int]] = None,
             stop_ids: Sequence[int] = ()) -> Tuple[int, int, int]:
    """``token_bytes[i]``: the bytes of generated token i (``tokens[i]`` its id).  ``at``: the index of the token in which
    the earliest match completed (-1: none), ``keep``: the bytes of text in front of the matched string (in front of the
    token, for a stop id), ``which``: the string's index -- the first of equal strings -- or ``len(strings) + j`` for the
    j-th stop id.  A stop id wins over the bytes of its own token; tokens are judged in order."""
    stop_ids = list(stop_ids)
    text = b""
    for i, data in enumerate(token_bytes):
        if tokens is not None and int(tokens[i]) in stop_ids:
            return i, len(text), len(strings) + stop_ids.index(int(tokens[i]))
        for e in range(len(text) + 1, len(text) + len(data) + 1):
            upto = (text + bytes(data))[:e]
            best = -1
            for k, s in enumerate(strings):
                if upto.endswith(s) and (best < 0 or len(s) > len(strings[best])):
                    best = k
            if best >= 0:
                return i, e - len(strings[best]), best
        text += bytes(data)
    return -1, 0, -1


def named_cases():
    """(name, vocabulary bytes, token ids, stop strings (str), stop ids) -- the cases the CPU and the kernel tests share."""
    v = [b"", b"a", b"b", b"ab", b"xa", b"b!", b"hello", b" wor", b"ld.", b"\n", b"\n\nQ", b"abab", b"\xc3", b"\xa9t\xc3\xa9",
         b"zz", b"x" * 48, b"xab", b"END", b"c"]
    return [
        ("spans three tokens", v, [14, 6, 7, 8, 1], ["lo world"], []),
        ("ends in mid-token", v, [1, 10, 2], ["\n\n"], []),
        ("two matches in one token: the earlier end", v, [14, 11, 1], ["bab", "ab"], []),
        ("ab and xab end at the same byte: the longer", v, [14, 16, 1], ["ab", "xab"], []),
        ("ab and xab across tokens", v, [4, 2, 1], ["ab", "xab"], []),
        ("a proper prefix of another", v, [14, 6, 1], ["hel", "hello"], []),
        ("a stop id whose bytes would complete a string", v, [1, 2, 18], ["ab"], [2]),
        ("zero-byte tokens between the halves", v, [1, 0, 0, 2, 1], ["ab"], []),
        ("multi-byte UTF-8 split across tokens", v, [14, 12, 13, 1], ["été"], []),
        ("a 48-byte token, match at its end", v, [1, 15, 1], ["x" * 40], []),
        ("a match past the first 16 bytes of a token", v, [1, 15, 2], ["ax" + "x" * 19], []),
        ("no match", v, [6, 7, 8, 9], ["zzz", "Q:"], [17]),
        ("ids alone", v, [6, 7, 17, 1], [], [3, 17]),
    ]
