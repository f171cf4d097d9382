"""Fixed-shape id tensors for code that lives beside this library in one PyTorch-ROCm process: text -> [rows, L] CUDA tensors and back,
without an id crossing the host link (tm_batch_collate / tm_batch_windows / tm_batch_pair / tm_batch_pack / tm_batch_load_ids, include/tokenmonster_hip.h).

    encode_batch   one document per row: padded or truncated, BOS / EOS, attention mask, lengths
    encode_windows every id kept: a long document as several rows that overlap, with the row -> document map
    encode_pairs   two documents per row, [bos] A [sep] B [eos]: pair truncation, token type ids
    encode_pair_windows   the QA form: A in every row, B slides over several rows that overlap
    pack_batch     the pre-training form: one EOS-separated id stream cut into rows, with document numbers and positions
    decode_batch   a [rows, L] tensor of ids -> list of bytes

torch is imported on first use; nothing else in the package imports this module.  A program that uses it imports torch BEFORE
tokenmonster_amd: torch ships a HIP runtime of its own, the one loaded first serves the whole process, and only torch's serves both.  The kernels run on torch's CURRENT stream of the
vocabulary's device (the text upload is the library's synchronous one and is complete before anything is launched), so the tensors
returned are ordered like any other torch result.  The device workspaces are cached per vocabulary and only ever grow, like the lanes of
the host-buffer entry points: a second call of the same size allocates nothing on the library's side."""
import ctypes as C
import weakref

import numpy as np

from . import _native as N
from .vocab import pack_documents, span_unit

PAD_LEFT, KEEP_TAIL = 1, 2


class _Collate(C.Structure):
    """tm_collate"""
    _fields_ = [(n, C.c_uint32) for n in ("first_doc", "ndocs", "row_len", "id_bytes", "pad_id", "bos_id", "eos_id", "flags")]


def _torch():
    import torch
    if not torch.cuda.is_available() and N.lib.tm_device_count() > 0:
        raise RuntimeError("torch sees no device although the library does: torch brings a HIP runtime of its own and a process drives the device "
                           "through one - `import torch` BEFORE `import tokenmonster_amd`, so that the library shares torch's")
    return torch


def _id_dtypes(torch):
    """torch dtype -> bytes of an id (the signed forms hold the same bits)"""
    d = {torch.int64: 8, torch.int32: 4, torch.int16: 2}
    for name, size in (("uint16", 2), ("uint32", 4)):
        if hasattr(torch, name):
            d[getattr(torch, name)] = size
    return d


def _special(x):
    return N.TM_NONE if x is None else int(x)


def _device(vocab, device):
    torch = _torch()
    if device is None:
        device = getattr(vocab, "device_index", 0)
    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


def _stream(dev):
    return C.c_void_p(_torch().cuda.current_stream(dev).cuda_stream)


# ---- the cached workspaces: per vocabulary one for each direction, grow-only ------------------------------------------------------------
class _Workspaces:
    def __init__(self):
        self.batches = {}          # "encode" / "decode" -> [handle, max_bytes, max_docs]
        self.last_stream = None    # of the last encode

    def get(self, vocab, kind, need_bytes, need_docs):
        cur = self.batches.get(kind)
        if cur is not None and cur[1] >= need_bytes and cur[2] >= need_docs:
            return cur[0]
        max_bytes = max(need_bytes, cur[1] if cur else 0)
        max_docs = max(need_docs, cur[2] if cur else 0)
        if cur is not None:
            N.lib.tm_batch_free(cur[0])
            del self.batches[kind]
        h = C.c_void_p()
        N.check(N.lib.tm_batch_create(vocab.handle, max_bytes, max_docs, C.byref(h)))
        self.batches[kind] = [h, max_bytes, max_docs]
        return h

    def close(self):
        for h, _, _ in self.batches.values():
            N.lib.tm_batch_free(h)
        self.batches = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_cache = weakref.WeakKeyDictionary()      # Vocab -> _Workspaces


def _workspaces(vocab):
    ws = _cache.get(vocab)
    if ws is None:
        ws = _cache[vocab] = _Workspaces()
    return ws


def device_bytes(vocab):
    """HBM the cached workspaces of this vocabulary hold (tm_batch_device_bytes of each)"""
    ws = _cache.get(vocab)
    return sum(int(N.lib.tm_batch_device_bytes(b[0])) for b in ws.batches.values()) if ws else 0


def release(vocab):
    """frees the cached workspaces of a vocabulary (before Vocab.close(), or to give the memory back)"""
    ws = _cache.pop(vocab, None)
    if ws:
        ws.close()


def _pow2(n):
    return 1 << max(int(n) - 1, 1).bit_length()


def _tokenize(vocab, docs, raw, stream):
    """documents -> a workspace that holds their ids (tm_batch_run enqueued on `stream`), number of documents"""
    docs = [d.encode("utf-8") if isinstance(d, str) else d for d in docs]
    text, offsets = pack_documents(docs)
    nd = offsets.size - 1
    # (raw text grows under normalization: the rule of Vocab.tokenize)
    ws = _workspaces(vocab)
    if ws.last_stream not in (None, stream.value):          # the last call's kernels may still read what this one overwrites
        _torch().cuda.synchronize()
    ws.last_stream = stream.value
    b = ws.get(vocab, "encode", _pow2(int(text.size) * (4 if raw else 1) + 16 * nd + 1024), _pow2(max(nd, 1)))
    if raw:
        N.check(N.lib.tm_batch_upload_raw(b, N.ptr(text), N.ptr(offsets), nd))
        N.check(N.lib.tm_batch_normalize(b, stream))
    else:
        N.check(N.lib.tm_batch_upload(b, N.ptr(text), N.ptr(offsets), nd))
    N.check(N.lib.tm_batch_run(b, stream))
    return b, nd


def _check_dtype(torch, dtype):
    sizes = _id_dtypes(torch)
    if dtype not in sizes:
        raise ValueError("ids of dtype %s: int64, int32, int16, uint16 or uint32" % (dtype,))
    return sizes[dtype]


def encode_batch(vocab, docs, max_length, *, pad_id, bos_id=None, eos_id=None, pad_left=False, keep_tail=False, dtype=None, raw=True, device=None, return_offsets=False,
                 offset_unit="bytes"):
    """documents (bytes or str; raw=False: already normalized bytes) -> {"input_ids" [rows, max_length] of `dtype` (default int64),
    "attention_mask" [rows, max_length] bool, "lengths" [rows] int32}, CUDA tensors on the vocabulary's device.  Row r is
    [bos] ids [eos] pad...: the ids cut to max_length less the specials given (their head; keep_tail: their tail), the padding on the
    right (pad_left: on the left).  return_offsets=True adds "offset_mapping" [rows, max_length, 2] int64: (begin, end) of the bytes the id
    of a column came from, counted from the document's start in the normalized text the tokenizer walks (raw=True: what Vocab.normalize
    makes of the document), and (0, 0) on BOS, EOS and padding (tm_batch_collate_spans).  return_offsets="raw" (with raw=True only): the same
    pairs counted in the bytes of the document as it was passed in (tm_batch_collate_raw_spans).  offset_unit "bytes" | "chars" | "utf16"
    (any return_offsets): what the pairs count - bytes, code points or UTF-16 units, by the rule of include/tokenmonster_hip.h
    (tm_batch_collate_spans_in).  With str documents, return_offsets="raw" and offset_unit="chars", doc[b:e] is the text of the id."""
    unit = span_unit(offset_unit)
    if isinstance(return_offsets, str):
        if return_offsets != "raw":
            raise ValueError("return_offsets %r: False, True or \"raw\"" % (return_offsets,))
        if not raw:
            raise ValueError("return_offsets=\"raw\" needs raw=True: normalized documents have no raw text to point into")
    torch = _torch()
    dtype = dtype or torch.int64
    id_bytes = _check_dtype(torch, dtype)
    max_length = int(max_length)
    if max_length < (bos_id is not None) + (eos_id is not None) or max_length < 1:
        raise ValueError("max_length %d holds no row" % max_length)
    dev = _device(vocab, device)
    with torch.cuda.device(dev):
        st = _stream(dev)
        b, nd = _tokenize(vocab, docs, raw, st)
        ids = torch.empty((nd, max_length), dtype=dtype, device=dev)
        mask = torch.empty((nd, max_length), dtype=torch.uint8, device=dev)
        lengths = torch.empty((nd,), dtype=torch.int32, device=dev)
        how = _Collate(0, nd, max_length, id_bytes, int(pad_id), _special(bos_id), _special(eos_id), (PAD_LEFT if pad_left else 0) | (KEEP_TAIL if keep_tail else 0))
        N.check(N.lib.tm_batch_collate(b, C.byref(how), st, ids.data_ptr(), mask.data_ptr(), lengths.data_ptr()))
        res = {"input_ids": ids, "attention_mask": mask.view(torch.bool), "lengths": lengths}
        if return_offsets:
            spans = torch.empty((nd, max_length, 2), dtype=torch.int64, device=dev)
            text = N.TM_TEXT_RAW if return_offsets == "raw" else N.TM_TEXT_NORMALIZED
            N.check(N.lib.tm_batch_collate_spans_in(b, C.byref(how), st, text, unit, spans.data_ptr(), 8))
            res["offset_mapping"] = spans
    return res


def encode_windows(vocab, docs, max_length, overlap, *, pad_id, bos_id=None, eos_id=None, pad_left=False, dtype=None, raw=True, device=None, return_offsets=False,
                   offset_unit="bytes"):
    """documents -> overlapping rows, every id kept: a document with more ids than a row holds takes several rows, consecutive rows of a
    document share `overlap` ids (the stride / return_overflowing_tokens of other tokenizers; tm_batch_windows).  {"input_ids" [rows,
    max_length] of `dtype` (default int64), "attention_mask" [rows, max_length] bool, "lengths" [rows] int32, "overflow_to_sample_mapping"
    [rows] int32 - the document of a row -, "window_start" [rows] int32 - the index inside the document of the row's first id}.  Row k of a
    document is [bos] ids[k * step : k * step + room] [eos] pad..., room = max_length less the specials given, step = room - overlap; the
    ids are those of the one walk over the whole document.  return_offsets as for encode_batch: "offset_mapping" [rows, max_length, 2]
    int64 counts from the DOCUMENT's start in every row (tm_batch_windows_spans / tm_batch_windows_raw_spans); offset_unit "bytes" |
    "chars" | "utf16" as for encode_batch (tm_batch_windows_spans_in): with str documents, return_offsets="raw" and offset_unit="chars",
    doc[b:e] is the text of the id."""
    unit = span_unit(offset_unit)
    if isinstance(return_offsets, str):
        if return_offsets != "raw":
            raise ValueError("return_offsets %r: False, True or \"raw\"" % (return_offsets,))
        if not raw:
            raise ValueError("return_offsets=\"raw\" needs raw=True: normalized documents have no raw text to point into")
    torch = _torch()
    dtype = dtype or torch.int64
    id_bytes = _check_dtype(torch, dtype)
    max_length, overlap = int(max_length), int(overlap)
    room = max_length - (bos_id is not None) - (eos_id is not None)
    if room < 1:
        raise ValueError("max_length %d holds no id beside the specials" % max_length)
    if not 0 <= overlap < room:
        raise ValueError("overlap %d: 0 .. %d (rows of %d ids beside the specials)" % (overlap, room - 1, room))
    dev = _device(vocab, device)
    with torch.cuda.device(dev):
        st = _stream(dev)
        b, nd = _tokenize(vocab, docs, raw, st)
        how = _Collate(0, nd, max_length, id_bytes, int(pad_id), _special(bos_id), _special(eos_id), PAD_LEFT if pad_left else 0)
        rows = C.c_uint64()
        N.check(N.lib.tm_batch_window_rows(b, C.byref(how), overlap, C.byref(rows)))
        rows = int(rows.value)
        ids = torch.empty((rows, max_length), dtype=dtype, device=dev)
        mask = torch.empty((rows, max_length), dtype=torch.uint8, device=dev)
        lengths, row_doc, row_start = (torch.empty((rows,), dtype=torch.int32, device=dev) for _ in range(3))
        if rows:
            N.check(N.lib.tm_batch_windows(b, C.byref(how), overlap, st, rows, ids.data_ptr(), mask.data_ptr(), lengths.data_ptr(), row_doc.data_ptr(), row_start.data_ptr()))
        res = {"input_ids": ids, "attention_mask": mask.view(torch.bool), "lengths": lengths, "overflow_to_sample_mapping": row_doc, "window_start": row_start}
        if return_offsets:
            spans = torch.empty((rows, max_length, 2), dtype=torch.int64, device=dev)
            text = N.TM_TEXT_RAW if return_offsets == "raw" else N.TM_TEXT_NORMALIZED
            if rows:
                N.check(N.lib.tm_batch_windows_spans_in(b, C.byref(how), overlap, st, rows, text, unit, spans.data_ptr(), 8))
            res["offset_mapping"] = spans
    return res


_TRUNCATION = {"longest_first": N.TM_PAIR_LONGEST_FIRST, "only_first": N.TM_PAIR_ONLY_FIRST, "only_second": N.TM_PAIR_ONLY_SECOND}


def _pair_args(torch, first, second, max_length, pad_id, bos_id, sep_id, sep_count, eos_id, truncation, pad_left, dtype, raw, return_offsets, offset_unit):
    """the checks both pair calls share, every one before any device call -> (unit, id_bytes, dtype, room, tm_pair without its ranges)"""
    unit = span_unit(offset_unit)
    if isinstance(return_offsets, str):
        if return_offsets != "raw":
            raise ValueError("return_offsets %r: False, True or \"raw\"" % (return_offsets,))
        if not raw:
            raise ValueError("return_offsets=\"raw\" needs raw=True: normalized documents have no raw text to point into")
    if len(first) != len(second):
        raise ValueError("%d first and %d second documents: a pair takes one of each" % (len(first), len(second)))
    if truncation not in _TRUNCATION:
        raise ValueError("truncation %r: \"longest_first\", \"only_first\" or \"only_second\"" % (truncation,))
    dtype = dtype or torch.int64
    id_bytes = _check_dtype(torch, dtype)
    sep_count = int(sep_count) if sep_id is not None else 0
    if sep_id is not None and sep_count not in (1, 2):
        raise ValueError("sep_count %d: 1 or 2" % sep_count)
    max_length = int(max_length)
    room = max_length - (bos_id is not None) - sep_count - (eos_id is not None)
    if room < 0 or max_length < 1:
        raise ValueError("max_length %d holds no row" % max_length)
    how = N.Pair(0, 0, 0, max_length, id_bytes, int(pad_id), _special(bos_id), _special(sep_id), _special(eos_id), sep_count, _TRUNCATION[truncation],
                 PAD_LEFT if pad_left else 0)
    return unit, id_bytes, dtype, room, how


def encode_pairs(vocab, first, second, max_length, *, pad_id, bos_id=None, sep_id=None, sep_count=1, eos_id=None, truncation="longest_first", pad_left=False, dtype=None,
                 raw=True, device=None, return_offsets=False, offset_unit="bytes"):
    """two lists of documents of equal length (bytes or str; raw=False: already normalized bytes) -> one pair per row, the text / text_pair
    form of other tokenizers (tm_batch_pair): {"input_ids" [rows, max_length] of `dtype` (default int64), "attention_mask" [rows, max_length]
    bool, "token_type_ids" [rows, max_length] uint8 - 0 on BOS, the first side and the separators, 1 on the second side and EOS, 0 on
    padding; `.long()` for a model that wants int64 -, "kept" [rows, 2] int32 - the ids kept of either side}.  Row r is
    [bos] first[r] [sep]*sep_count second[r] [eos] pad... (pad_left: the padding on the left); the two sides are tokenized as separate
    documents.  truncation, when the two do not fit max_length less the specials: "longest_first" takes one id at a time from the end of
    the longer side (from the first on a tie), "only_second" cuts the second side and "only_first" the first (the other one only where it
    alone overflows the row).  sep_count: 1, or 2 for models that double the separator; ignored without sep_id.  return_offsets and
    offset_unit as for encode_batch: "offset_mapping" [rows, max_length, 2] int64, each side's pairs counted from its own document's
    start, (0, 0) on specials and padding (tm_batch_pair_spans_in).  With str documents, return_offsets="raw" and offset_unit="chars",
    first[r][b:e] or second[r][b:e] - by token_type_ids - is the text of the id."""
    torch = _torch()
    unit, id_bytes, dtype, _, how = _pair_args(torch, first, second, max_length, pad_id, bos_id, sep_id, sep_count, eos_id, truncation, pad_left, dtype, raw, return_offsets,
                                               offset_unit)
    max_length = how.row_len
    dev = _device(vocab, device)
    with torch.cuda.device(dev):
        st = _stream(dev)
        b, nd = _tokenize(vocab, list(first) + list(second), raw, st)      # ONE batch: the first sides, then the second
        n = nd // 2
        how.first_a, how.first_b, how.npairs = 0, n, n
        ids = torch.empty((n, max_length), dtype=dtype, device=dev)
        mask = torch.empty((n, max_length), dtype=torch.uint8, device=dev)
        types = torch.empty((n, max_length), dtype=torch.uint8, device=dev)
        kept = torch.empty((n, 2), dtype=torch.int32, device=dev)
        N.check(N.lib.tm_batch_pair(b, C.byref(how), st, ids.data_ptr(), mask.data_ptr(), types.data_ptr(), kept.data_ptr()))
        res = {"input_ids": ids, "attention_mask": mask.view(torch.bool), "token_type_ids": types, "kept": kept}
        if return_offsets:
            spans = torch.empty((n, max_length, 2), dtype=torch.int64, device=dev)
            text = N.TM_TEXT_RAW if return_offsets == "raw" else N.TM_TEXT_NORMALIZED
            N.check(N.lib.tm_batch_pair_spans_in(b, C.byref(how), st, text, unit, spans.data_ptr(), 8))
            res["offset_mapping"] = spans
    return res


def encode_pair_windows(vocab, first, second, max_length, overlap, max_first, *, pad_id, bos_id=None, sep_id=None, sep_count=1, eos_id=None, truncation="only_second",
                        pad_left=False, dtype=None, raw=True, device=None, return_offsets=False, offset_unit="bytes"):
    """the extractive-QA form of encode_pairs (tm_batch_pair_windows): the first side (the question), cut to max_first ids, stands in every
    row of its pair, and every id of the second side (the context) is kept - a pair whose second side does not fit takes several rows, and
    consecutive rows of a pair share `overlap` ids of it (stride / return_overflowing_tokens).  The keys of encode_pairs - "kept" [rows, 2]
    holds the ids of the first side and those of the second in THIS row - and "overflow_to_sample_mapping" [rows] int32, the pair of a row,
    and "window_start" [rows] int32, the index inside the second document of the row's first id of it.  Per pair the second side has
    room = max_length - specials - min(ids of first, max_first) ids per row, rows are room - overlap ids apart; max_first + overlap must
    be smaller than max_length less the specials.  truncation must be "only_second" (the default here).  "offset_mapping": the second
    side's pairs count from its document's start in every row (tm_batch_pair_windows_spans_in)."""
    torch = _torch()
    unit, id_bytes, dtype, room, how = _pair_args(torch, first, second, max_length, pad_id, bos_id, sep_id, sep_count, eos_id, truncation, pad_left, dtype, raw, return_offsets,
                                                  offset_unit)
    if truncation != "only_second":
        raise ValueError("truncation %r: pair windows cut the second side only (\"only_second\")" % (truncation,))
    max_length, overlap, max_first = how.row_len, int(overlap), int(max_first)
    if not 0 <= max_first <= room or overlap < 0 or room - max_first <= overlap:
        raise ValueError("max_first %d and overlap %d: both >= 0 and max_first + overlap < %d (the ids a row holds beside the specials)" % (max_first, overlap, room))
    dev = _device(vocab, device)
    with torch.cuda.device(dev):
        st = _stream(dev)
        b, nd = _tokenize(vocab, list(first) + list(second), raw, st)
        n = nd // 2
        how.first_a, how.first_b, how.npairs = 0, n, n
        rows = C.c_uint64()
        N.check(N.lib.tm_batch_pair_window_rows(b, C.byref(how), overlap, max_first, C.byref(rows)))
        rows = int(rows.value)
        ids = torch.empty((rows, max_length), dtype=dtype, device=dev)
        mask = torch.empty((rows, max_length), dtype=torch.uint8, device=dev)
        types = torch.empty((rows, max_length), dtype=torch.uint8, device=dev)
        kept = torch.empty((rows, 2), dtype=torch.int32, device=dev)
        row_pair, row_start = (torch.empty((rows,), dtype=torch.int32, device=dev) for _ in range(2))
        if rows:
            N.check(N.lib.tm_batch_pair_windows(b, C.byref(how), overlap, max_first, st, rows, ids.data_ptr(), mask.data_ptr(), types.data_ptr(), kept.data_ptr(),
                                                row_pair.data_ptr(), row_start.data_ptr()))
        res = {"input_ids": ids, "attention_mask": mask.view(torch.bool), "token_type_ids": types, "kept": kept, "overflow_to_sample_mapping": row_pair,
               "window_start": row_start}
        if return_offsets:
            spans = torch.empty((rows, max_length, 2), dtype=torch.int64, device=dev)
            text = N.TM_TEXT_RAW if return_offsets == "raw" else N.TM_TEXT_NORMALIZED
            if rows:
                N.check(N.lib.tm_batch_pair_windows_spans_in(b, C.byref(how), overlap, max_first, st, rows, text, unit, spans.data_ptr(), 8))
            res["offset_mapping"] = spans
    return res


def pack_batch(vocab, docs, seq_len, *, eos_id, pad_id, dtype=None, raw=True, device=None):
    """documents -> the stream ids(doc 0) eos ids(doc 1) eos ... cut into rows of seq_len (eos_id None: no separator), the last row filled
    with pad_id: {"input_ids" [rows, seq_len] of `dtype` (default int64), "doc_index" [rows, seq_len] int32 - the document of every
    position, -1 on padding -, "position" [rows, seq_len] int32 - its index inside the document, the EOS being the document's last}"""
    torch = _torch()
    dtype = dtype or torch.int64
    id_bytes = _check_dtype(torch, dtype)
    seq_len = int(seq_len)
    if seq_len < 1:
        raise ValueError("seq_len %d" % seq_len)
    dev = _device(vocab, device)
    with torch.cuda.device(dev):
        st = _stream(dev)
        b, nd = _tokenize(vocab, docs, raw, st)
        how = _Collate(0, nd, seq_len, id_bytes, int(pad_id), N.TM_NONE, _special(eos_id), 0)
        rows = C.c_uint64()
        N.check(N.lib.tm_batch_pack_rows(b, C.byref(how), C.byref(rows)))
        rows = int(rows.value)
        ids = torch.empty((rows, seq_len), dtype=dtype, device=dev)
        doc_index = torch.empty((rows, seq_len), dtype=torch.int32, device=dev)
        position = torch.empty((rows, seq_len), dtype=torch.int32, device=dev)
        N.check(N.lib.tm_batch_pack(b, C.byref(how), st, rows, ids.data_ptr(), doc_index.data_ptr(), position.data_ptr()))
    return {"input_ids": ids, "doc_index": doc_index, "position": position}


def decode_batch(vocab, ids, *, lengths=None, pad_id=None, bos_id=None, eos_id=None, device=None):
    """a [rows, L] CUDA tensor of ids (int16 / uint16, int32 or int64, contiguous, on the vocabulary's device) -> list of bytes, one per row.
    What of a row is text: a leading run of pad_id is skipped, then the row extends over lengths[r] entries (a [rows] integer tensor as
    encode_batch returns it; None: to its end), one leading bos_id is skipped and the first eos_id ends it."""
    torch = _torch()
    dev = _device(vocab, device)
    # every check before any device call
    if not isinstance(ids, torch.Tensor) or not ids.is_cuda or ids.device != dev:
        raise ValueError("ids must be a CUDA tensor on %s" % (dev,))
    if ids.dim() != 2:
        raise ValueError("ids must be [rows, L]")
    if not ids.is_contiguous():
        raise ValueError("ids must be contiguous")
    sizes = _id_dtypes(torch)
    if ids.dtype not in sizes:
        raise ValueError("ids of dtype %s: int16, uint16, int32 or int64" % (ids.dtype,))
    nrows, L = int(ids.shape[0]), int(ids.shape[1])
    if lengths is not None:
        if not isinstance(lengths, torch.Tensor) or lengths.device != dev or lengths.dim() != 1 or lengths.shape[0] != nrows or lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError("lengths must be an int32 or int64 CUDA tensor [rows] on %s" % (dev,))
    if nrows == 0 or L == 0:
        return [b""] * nrows
    with torch.cuda.device(dev):
        st = _stream(dev)
        if lengths is not None:
            lengths = lengths.to(torch.int32).contiguous()
        b = _workspaces(vocab).get(vocab, "decode", 4096, _pow2(nrows))
        N.check(N.lib.tm_batch_load_ids(b, ids.data_ptr(), nrows, L, sizes[ids.dtype], lengths.data_ptr() if lengths is not None else None,
                                        _special(pad_id), _special(bos_id), _special(eos_id), st))
        nbytes, host_docs = C.c_uint64(), C.c_uint32()
        N.check(N.lib.tm_batch_decode(b, 0, st, C.byref(nbytes), C.byref(host_docs)))
        off = np.zeros(nrows + 1, dtype=np.uint64)
        cap = int(nbytes.value) * 2 + 64
        while True:
            out = np.empty(cap, dtype=np.uint8)
            rc = N.lib.tm_batch_decoded_download(b, N.ptr(out), cap, N.ptr(off))
            if rc == N.TM_E_NOSPACE:
                cap = int(off[nrows])
                continue
            N.check(rc)
            break
    return [out[int(off[r]):int(off[r + 1])].tobytes() for r in range(nrows)]
