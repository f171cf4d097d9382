"""The expected byte spans of a document's ids, from the pinned oracle alone (shared by tests/test_span_recipe.py and tests/test_gpu_spans.py).

The oracle's walk (oracle/tm_oracle.c: walk_range_padded) stands at byte i when it emits an id and then adds the token's advance: the id's span
is [i, i + adv).  The oracle does not report spans, but its scoring mode can be entered at any token boundary in either forward-delete state
(tmo_score_range) and says where and in which state it leaves: chained one boundary at a time, from boundary b in state fd over the range
[b, b + 1), it takes exactly the steps that begin at b.

  - next boundary b + 1 + (exit >> 1), next state exit & 1
  - a non-empty missing set: the step was a character without a token; it carries an id (the unk token) only if the vocabulary has one
  - else the range consumed tokens_in_text ids: if the new state is 1 the last of them is a delete token with the empty span at the new
    boundary; of the others all but the last took no byte - the empty span [b, b) - and the last has [b, next)
"""
import ctypes as C

import numpy as np


class SpanStats:
    def __init__(self):
        self.docs = self.ids = self.zero = self.delete = self.missing_unk = self.missing_nounk = 0

    def add(self, o):
        for k in vars(self):
            setattr(self, k, getattr(self, k) + getattr(o, k))

    def __repr__(self):
        return "SpanStats(%s)" % ", ".join("%s=%d" % kv for kv in vars(self).items())


def _bind(orc):
    fn = orc.L.tmo_score_range
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint32)]
    return fn


def oracle_spans(orc, doc, has_unk, stats=None):
    """-> int64 [n, 2]: (begin, end) of every id Oracle.tokenize(doc) returns, in order.  Oracle.score_range(doc, b, b + 1, entry_state=fd) one
    boundary at a time (called through its C entry with buffers that are reused: a step of a vocabulary of 70 000 ids would clear as many scores)"""
    fn = _bind(orc)
    d = np.ascontiguousarray(np.frombuffer(bytes(doc), dtype=np.uint8))
    n = int(d.size)
    scores = getattr(orc, "_span_scores", None)
    if scores is None:
        scores = orc._span_scores = np.zeros(orc.n_ids(), dtype=np.uint32)
    ms = np.zeros(32, dtype=np.uint8)
    tit, ex = C.c_uint64(0), C.c_uint32(0)
    out = []
    st = SpanStats()
    st.docs = 1
    b, fd = 0, 0
    while b < n:
        ms[:] = 0
        tit.value = 0
        fn(orc.h, d.ctypes.data, n, b, fd, b + 1, scores.ctypes.data, C.byref(tit), ms.ctypes.data, C.byref(ex))
        nxt, nfd = b + 1 + (ex.value >> 1), ex.value & 1
        if ms.any():
            assert tit.value == 1 and nxt == b + 1 and nfd == 0
            if has_unk:
                out.append((b, b + 1))
                st.missing_unk += 1
            else:
                st.missing_nounk += 1
        else:
            k = int(tit.value)
            assert k >= 1 + nfd
            for _ in range(k - nfd - 1):
                out.append((b, b))
                st.zero += 1
            out.append((b, nxt))
            if nfd:
                out.append((nxt, nxt))
                st.delete += 1
        b, fd = nxt, nfd
    st.ids = len(out)
    if stats is not None:
        stats.add(st)
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def check_order(spans):
    """begins never decrease, ends never lie before begins, no two spans overlap"""
    s = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    assert (s[:, 1] >= s[:, 0]).all()
    assert (s[1:, 0] >= s[:-1, 1]).all()
