"""The unit rule of include/tokenmonster_hip.h (character offsets) in a few lines of numpy: byte pairs of a document -> pairs in code points or
UTF-16 units.  Calls nothing of the library (shared by tests/test_unit_recipe.py and tests/test_gpu_char_offsets.py)."""
import numpy as np

BYTES, CODEPOINTS, UTF16 = 0, 1, 2


def U_table(doc, unit):
    """int64 [len + 1]: U(x) for every x in 0..len"""
    d = np.frombuffer(bytes(doc), dtype=np.uint8)
    if unit == BYTES:
        return np.arange(d.size + 1, dtype=np.int64)
    per = ((d & 0xC0) != 0x80).astype(np.int64)
    if unit == UTF16:
        per = per + (d >= 0xF0)
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(per, dtype=np.int64)])


def char_start_table(doc):
    """int64 [len + 1]: char_start(x) for every x in 0..len"""
    d = np.frombuffer(bytes(doc), dtype=np.uint8)
    n = d.size
    cont = np.concatenate([(d & 0xC0) == 0x80, np.zeros(1, bool)])      # (x == len is no continuation byte)
    x = np.arange(n + 1, dtype=np.int64)
    cs = x.copy()
    todo = cont.copy()                                                   # continuation bytes that have not found their character's begin
    for k in (1, 2, 3):                                                  # the nearest first
        hit = todo & (x >= k) & ~cont[np.maximum(x - k, 0)]
        cs[hit] = x[hit] - k
        todo &= ~hit
    return cs


def D_table(doc, unit):
    """int64 [len + 1]: D(x) = U(char_start(x))"""
    if unit == BYTES:
        return np.arange(len(bytes(doc)) + 1, dtype=np.int64)
    return U_table(doc, unit)[char_start_table(doc)]


def convert(spans, doc, unit):
    """byte pairs int [n, 2] of `doc` -> int64 [n, 2] in `unit`: (D(b), U(e)) if e > b, (D(b), D(b)) otherwise"""
    s = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    U, D = U_table(doc, unit), D_table(doc, unit)
    out = np.empty_like(s)
    out[:, 0] = D[s[:, 0]]
    out[:, 1] = np.where(s[:, 1] > s[:, 0], U[s[:, 1]], D[s[:, 0]])
    return out
