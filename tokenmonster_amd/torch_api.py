"""Fixed-shape id tensors for code that lives beside this library in one PyTorch-ROCm process: text -> [rows, L] CUDA tensors and back,
without an id crossing the host link (tm_batch_collate / tm_batch_windows / tm_batch_pair / tm_batch_pack / tm_batch_load_ids, include/tokenmonster_hip.h).

    encode_batch   one document per row: padded or truncated, BOS / EOS, attention mask, lengths
    encode_windows every id kept: a long document as several rows that overlap, with the row -> document map
    encode_pairs   two documents per row, [bos] A [sep] B [eos]: pair truncation, token type ids
    encode_pair_windows   the QA form: A in every row, B slides over several rows that overlap
    pack_batch     the pre-training form: one EOS-separated id stream cut into rows, with document numbers and positions
    decode_batch   a [rows, L] tensor of ids -> list of bytes
    tokenize_resident   tokenize once, draw batches many times: the documents' length order and encode_batch's rows by document number
    Masking        masked-LM corruption of encode_batch's and ResidentBatch.collate's rows on the device, with "labels" (masking=..., seed=...)
    SpanCorruption T5 / UL2 span corruption of the same rows: sentinel inputs, and the spans as "labels" (denoise=..., target_length=..., seed=...)

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


class Masking:
    """Masked-LM corruption for encode_batch(masking=...) and ResidentBatch.collate(masking=...) (tm_batch_collate_masked; the rule:
    include/tokenmonster_hip.h).  An id of a document opens a span with probability `probability` / mean span length, a span covers
    span[0] .. span[1] ids (uniform; (1, 1): token masking as BERT and RoBERTa do it, (1, 10) or so: SpanBERT-like), and an id a span covers
    becomes mask_id with probability mask_share, a random id of random_ids = (lo, n) - lo .. lo + n - 1; None: every id of the vocabulary -
    with random_share, and else stays as it is.  "labels" holds the original id in every covered column and `ignore` elsewhere (BOS, EOS
    and padding are never covered).  Spans may overlap and are cut at their document's end, so the share of ids covered comes out somewhat
    below `probability` - the more so the longer the spans.  The masks depend on the seed and on the place of an id in the batch of
    documents alone, not on the row layout: pass a new seed per step for dynamic masking."""

    def __init__(self, *, mask_id, probability=0.15, span=(1, 1), mask_share=0.8, random_share=0.1, random_ids=None, ignore=-100):
        lo, hi = int(span[0]), int(span[1])
        if not 1 <= lo <= hi <= 32:
            raise ValueError("span %r: 1 <= span[0] <= span[1] <= 32" % (span,))
        if not (0 <= probability <= 1 and 0 <= mask_share and 0 <= random_share and mask_share + random_share <= 1):
            raise ValueError("probability, mask_share, random_share and mask_share + random_share: 0 .. 1")
        self.mask_id, self.span, self.random_ids, self.ignore = int(mask_id), (lo, hi), random_ids, int(ignore)
        self.start_thr = min(round((1 << 32) * probability / ((lo + hi) / 2)), 1 << 32)
        self.mask_thr = round((1 << 32) * mask_share)
        self.random_thr = min(round((1 << 32) * random_share), (1 << 32) - self.mask_thr)

    def struct(self, vocab, seed):
        """tm_masking under `seed`"""
        lo, n = self.random_ids if self.random_ids is not None else (0, vocab.n_ids())
        return N.Masking(int(seed) & 0xFFFFFFFFFFFFFFFF, self.start_thr, self.span[0], self.span[1], self.mask_thr, self.random_thr, self.mask_id, int(lo), int(n), self.ignore)


class SpanCorruption:
    """T5 / UL2 span corruption for encode_batch(denoise=...) and ResidentBatch.collate(denoise=...) (tm_batch_collate_denoise; the rule:
    include/tokenmonster_hip.h).  An id of a document opens a noise span with probability noise_density / mean span length, a span covers
    span[0] .. span[1] ids (uniform), exactly as Masking selects.  Noise span k of a row becomes the ONE id sentinel_first + k * sentinel_step
    in "input_ids" (T5's <extra_id_k> count down from the vocabulary's end: sentinel_step -1), and "labels" [rows, target_length] holds every
    span behind its sentinel, then the EOS, then `ignore`.  A row uses at most sentinel_n sentinels: later spans stay as they are.
    "target_lengths" holds the uncut length of every target row, so a row cut at target_length shows.  The spans depend on the seed and on
    the place of an id in the batch of documents alone: pass a new seed per step."""

    def __init__(self, sentinel_first, sentinel_step=-1, sentinel_n=100, noise_density=0.15, span=(1, 5), ignore=-100):
        lo, hi = int(span[0]), int(span[1])
        if not 1 <= lo <= hi <= 32:
            raise ValueError("span %r: 1 <= span[0] <= span[1] <= 32" % (span,))
        if not 0 <= noise_density <= 1:
            raise ValueError("noise_density: 0 .. 1")
        if int(sentinel_step) == 0 or int(sentinel_n) < 1:
            raise ValueError("sentinel_step 0 or sentinel_n < 1")
        self.sentinel_first, self.sentinel_step, self.sentinel_n, self.span, self.ignore = int(sentinel_first), int(sentinel_step), int(sentinel_n), (lo, hi), int(ignore)
        self.start_thr = min(round((1 << 32) * noise_density / ((lo + hi) / 2)), 1 << 32)

    def struct(self, target_length, seed):
        """tm_denoise under `seed`"""
        return N.Denoise(int(seed) & 0xFFFFFFFFFFFFFFFF, self.start_thr, self.span[0], self.span[1], self.sentinel_first, self.sentinel_step, self.sentinel_n,
                         int(target_length), self.ignore)


def _check_denoise(denoise, target_length, masking, regions, pad_left):
    if denoise is not None:
        if masking is not None or regions is not None or pad_left:
            raise ValueError("denoise beside masking, regions or pad_left: span corruption writes \"labels\" of its own and pads on the right")
        if target_length is None or int(target_length) < 1:
            raise ValueError("denoise needs target_length >= 1: the columns of \"labels\"")


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
                 offset_unit="bytes", regions=None, ignore_label=-100, masking=None, seed=0, denoise=None, target_length=None):
    """documents (bytes or str; raw=False: already normalized bytes) -> {"input_ids" [rows, max_length] of `dtype` (default int64),
    "attention_mask" [rows, max_length] bool, "lengths" [rows] int32}, CUDA tensors on the vocabulary's device.  Row r is
    [bos] ids [eos] pad...: the ids cut to max_length less the specials given (their head; keep_tail: their tail), the padding on the
    right (pad_left: on the left).  return_offsets=True adds "offset_mapping" [rows, max_length, 2] int64: (begin, end) of the bytes the id
    of a column came from, counted from the document's start in the normalized text the tokenizer walks (raw=True: what Vocab.normalize
    makes of the document), and (0, 0) on BOS, EOS and padding (tm_batch_collate_spans).  return_offsets="raw" (with raw=True only): the same
    pairs counted in the bytes of the document as it was passed in (tm_batch_collate_raw_spans).  offset_unit "bytes" | "chars" | "utf16"
    (any return_offsets): what the pairs count - bytes, code points or UTF-16 units, by the rule of include/tokenmonster_hip.h
    (tm_batch_collate_spans_in).  With str documents, return_offsets="raw" and offset_unit="chars", doc[b:e] is the text of the id.
    regions=(regions, reg_offsets) adds "labels" [rows, max_length], int64 beside 8-byte ids and int32 otherwise: regions [R, 3] (begin, end,
    label) counted in offset_unit from its document's start - in the document as passed in with raw=True, else in the normalized text -, sorted
    and without overlap inside a document, reg_offsets [rows + 1]; both host arrays or tensors of the vocabulary's device (int64 / int32
    regions, int64 offsets).  A column holds the label of the first region its id meets, ignore_label elsewhere and on BOS, EOS and padding
    (tm_batch_collate_region_labels; the rule: include/tokenmonster_hip.h).
    masking=Masking(...) (not beside regions) corrupts "input_ids" for a masked-LM step under `seed` and adds "labels" [rows, max_length] of
    `dtype`: the original id where an id was selected, masking.ignore elsewhere (tm_batch_collate_masked).
    denoise=SpanCorruption(...) (not beside masking, regions or pad_left) makes the rows the input of a T5-style denoising step under `seed`:
    every noise span of "input_ids" one sentinel, "labels" [rows, target_length] of `dtype` the spans behind their sentinels, and
    "target_lengths" [rows] int32 their uncut lengths (tm_batch_collate_denoise).  "lengths" counts the compacted rows."""
    unit = span_unit(offset_unit)
    _check_denoise(denoise, target_length, masking, regions, pad_left)
    if masking is not None and regions is not None:
        raise ValueError("masking and regions both write \"labels\": one of them")
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
        res = {"input_ids": ids, "attention_mask": mask.view(torch.bool), "lengths": lengths}
        if denoise is not None:
            res["labels"] = torch.empty((nd, int(target_length)), dtype=dtype, device=dev)
            res["target_lengths"] = torch.empty((nd,), dtype=torch.int32, device=dev)
            N.check(N.lib.tm_batch_collate_denoise(b, C.byref(how), C.byref(denoise.struct(target_length, seed)), None, st, ids.data_ptr(), res["labels"].data_ptr(),
                                                   mask.data_ptr(), lengths.data_ptr(), res["target_lengths"].data_ptr(), None))
        elif masking is None:
            N.check(N.lib.tm_batch_collate(b, C.byref(how), st, ids.data_ptr(), mask.data_ptr(), lengths.data_ptr()))
        else:
            res["labels"] = torch.empty((nd, max_length), dtype=dtype, device=dev)
            N.check(N.lib.tm_batch_collate_masked(b, C.byref(how), C.byref(masking.struct(vocab, seed)), None, st, ids.data_ptr(), res["labels"].data_ptr(), mask.data_ptr(),
                                                  lengths.data_ptr(), None))
        if return_offsets:
            spans = torch.empty((nd, max_length, 2), dtype=torch.int64, device=dev)
            text = N.TM_TEXT_RAW if return_offsets == "raw" else N.TM_TEXT_NORMALIZED
            N.check(N.lib.tm_batch_collate_spans_in(b, C.byref(how), st, text, unit, spans.data_ptr(), 8))
            res["offset_mapping"] = spans
        if regions is not None:
            # (int32 holds a region's three numbers as the library reads them: offsets are 32 bits, a label is an int32_t)
            roff = torch.as_tensor(regions[1]).to(device=dev, dtype=torch.int64).contiguous()
            reg = torch.as_tensor(regions[0]).to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
            if roff.numel() != nd + 1:
                raise ValueError("reg_offsets: %d entries for %d documents" % (roff.numel(), nd))
            label_bytes = 8 if id_bytes == 8 else 4
            labels = torch.empty((nd, max_length), dtype=torch.int64 if label_bytes == 8 else torch.int32, device=dev)
            rg = N.Regions(roff.data_ptr(), reg.data_ptr(), N.TM_TEXT_RAW if raw else N.TM_TEXT_NORMALIZED, unit, int(ignore_label))
            N.check(N.lib.tm_batch_collate_region_labels(b, C.byref(how), st, C.byref(rg), labels.data_ptr(), label_bytes, None))
            res["labels"] = labels
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


def pack_batch(vocab, docs, seq_len, *, eos_id, pad_id, dtype=None, raw=True, device=None, whole=False):
    """documents -> the stream ids(doc 0) eos ids(doc 1) eos ... cut into rows of seq_len (eos_id None: no separator), the last row filled
    with pad_id: {"input_ids" [rows, seq_len] of `dtype` (default int64), "doc_index" [rows, seq_len] int32 - the document of every
    position, -1 on padding -, "position" [rows, seq_len] int32 - its index inside the document, the EOS being the document's last}.
    whole=True: the documents are packed WHOLE instead - a row is closed with pad_id when the next document does not fit, only a document
    longer than a row is cut (tm_batch_fit) - and "lengths" [rows] int32 (entries of a row), "row_doc" [rows] int32 (the document of a
    row's first entry) and "row_start" [rows] int32 (that entry's index inside its document) come beside the three."""
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
        N.check((N.lib.tm_batch_fit_rows if whole else N.lib.tm_batch_pack_rows)(b, C.byref(how), C.byref(rows)))
        rows = int(rows.value)
        ids = torch.empty((rows, seq_len), dtype=dtype, device=dev)
        doc_index = torch.empty((rows, seq_len), dtype=torch.int32, device=dev)
        position = torch.empty((rows, seq_len), dtype=torch.int32, device=dev)
        res = {"input_ids": ids, "doc_index": doc_index, "position": position}
        if whole:
            per_row = [torch.empty((rows,), dtype=torch.int32, device=dev) for _ in range(3)]
            if rows:
                N.check(N.lib.tm_batch_fit(b, C.byref(how), st, rows, ids.data_ptr(), doc_index.data_ptr(), position.data_ptr(), *[x.data_ptr() for x in per_row]))
            res.update(zip(("lengths", "row_doc", "row_start"), per_row))
        else:
            N.check(N.lib.tm_batch_pack(b, C.byref(how), st, rows, ids.data_ptr(), doc_index.data_ptr(), position.data_ptr()))
    return res


class ResidentBatch:
    """What tokenize_resident returns: the ids of `docs` resident on the device, in a workspace of its own (no other call of this module
    touches it), to draw batches from by document number until close().
        ndocs                      the documents
        counts()                   [ndocs] int64: the id count of every document
        length_order(descending)   [ndocs] int64: the document numbers in a stable order of their id counts (tm_batch_length_order)
        collate(indices, ...)      the rows of encode_batch for the documents `indices` names (tm_batch_collate_select)
    Everything runs on torch's current stream of the device and nothing is read back: no id and no index crosses the host link."""

    def __init__(self, vocab, docs, raw, device):
        torch = _torch()
        docs = [d.encode("utf-8") if isinstance(d, str) else d for d in docs]
        text, offsets = pack_documents(docs)
        self.vocab, self.ndocs, self.dev = vocab, offsets.size - 1, _device(vocab, device)
        self.handle = C.c_void_p()
        self._order_stream = None
        with torch.cuda.device(self.dev):
            st = _stream(self.dev)
            N.check(N.lib.tm_batch_create(vocab.handle, _pow2(int(text.size) * (4 if raw else 1) + 16 * self.ndocs + 1024), max(self.ndocs, 1), C.byref(self.handle)))
            try:
                if raw:
                    N.check(N.lib.tm_batch_upload_raw(self.handle, N.ptr(text), N.ptr(offsets), self.ndocs))
                    N.check(N.lib.tm_batch_normalize(self.handle, st))
                else:
                    N.check(N.lib.tm_batch_upload(self.handle, N.ptr(text), N.ptr(offsets), self.ndocs))
                N.check(N.lib.tm_batch_run(self.handle, st))
            except Exception:
                self.close()
                raise

    def _order(self, descending):
        """(order, counts of the order's documents), both int64, by one tm_batch_length_order"""
        torch = _torch()
        with torch.cuda.device(self.dev):
            st = _stream(self.dev)
            if self._order_stream not in (None, st.value):      # the last order's kernels may still use the scratch this one rewrites
                torch.cuda.synchronize()
            self._order_stream = st.value
            order, counts = (torch.empty((self.ndocs,), dtype=torch.int32, device=self.dev) for _ in range(2))
            N.check(N.lib.tm_batch_length_order(self.handle, 0, self.ndocs, 1 if descending else 0, st, order.data_ptr(), counts.data_ptr()))
            return order.to(torch.int64) & 0xFFFFFFFF, counts.to(torch.int64) & 0xFFFFFFFF

    def counts(self):
        order, sorted_counts = self._order(False)
        out = _torch().empty_like(sorted_counts)
        out[order] = sorted_counts
        return out

    def length_order(self, descending=False):
        return self._order(descending)[0]

    def collate(self, indices, max_length, *, pad_id, bos_id=None, eos_id=None, pad_left=False, keep_tail=False, dtype=None, masking=None, seed=0, denoise=None,
                target_length=None):
        """row r = the row encode_batch gives document indices[r]: {"input_ids" [rows, max_length] of `dtype` (default int64), "attention_mask"
        [rows, max_length] bool, "lengths" [rows] int32, "bad_indices" int32 scalar on the device: the entries of `indices` that name no
        document - their rows are padding only}.  indices: an integer tensor (moved to the device if it is not there) or a sequence; a
        document may stand in any number of rows.  masking=Masking(...): the rows corrupted for a masked-LM step under `seed`, and "labels"
        [rows, max_length] of `dtype` beside them, as encode_batch gives them (tm_batch_collate_masked): a document is masked the same way in
        whatever row or batch it stands, and differently under every seed.  denoise=SpanCorruption(...) (not beside masking or pad_left): the
        rows as the input of a T5-style denoising step, "labels" [rows, target_length] and "target_lengths" [rows] beside them, as encode_batch
        gives them (tm_batch_collate_denoise)."""
        _check_denoise(denoise, target_length, masking, None, pad_left)
        torch = _torch()
        dtype = dtype or torch.int64
        id_bytes = _check_dtype(torch, dtype)
        max_length = int(max_length)
        if max_length < (bos_id is not None) + (eos_id is not None) or max_length < 1:
            raise ValueError("max_length %d holds no row" % max_length)
        with torch.cuda.device(self.dev):
            st = _stream(self.dev)
            idx = torch.as_tensor(indices).to(device=self.dev).reshape(-1)
            if idx.numel() and (idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool):      # (an empty list has no dtype to speak of)
                raise ValueError("indices of dtype %s: an integer tensor or a sequence of integers" % (idx.dtype,))
            idx = idx.to(torch.int64)
            idx = torch.where((idx < 0) | (idx > 0xFFFFFFFF), torch.full_like(idx, 0xFFFFFFFF), idx).to(torch.int32).contiguous()      # (the bits of a uint32)
            rows = idx.numel()
            ids = torch.empty((rows, max_length), dtype=dtype, device=self.dev)
            mask = torch.empty((rows, max_length), dtype=torch.uint8, device=self.dev)
            lengths = torch.empty((rows,), dtype=torch.int32, device=self.dev)
            bad = torch.empty((), dtype=torch.int32, device=self.dev)
            how = _Collate(0, rows, max_length, id_bytes, int(pad_id), _special(bos_id), _special(eos_id), (PAD_LEFT if pad_left else 0) | (KEEP_TAIL if keep_tail else 0))
            res = {"input_ids": ids, "attention_mask": mask.view(torch.bool), "lengths": lengths, "bad_indices": bad}
            if masking is not None:
                res["labels"] = torch.empty((rows, max_length), dtype=dtype, device=self.dev)
            if denoise is not None:
                res["labels"] = torch.empty((rows, int(target_length)), dtype=dtype, device=self.dev)
                res["target_lengths"] = torch.empty((rows,), dtype=torch.int32, device=self.dev)
            if not rows:
                bad.zero_()
            elif denoise is not None:
                N.check(N.lib.tm_batch_collate_denoise(self.handle, C.byref(how), C.byref(denoise.struct(target_length, seed)), idx.data_ptr(), st, ids.data_ptr(),
                                                       res["labels"].data_ptr(), mask.data_ptr(), lengths.data_ptr(), res["target_lengths"].data_ptr(), bad.data_ptr()))
            elif masking is None:
                N.check(N.lib.tm_batch_collate_select(self.handle, C.byref(how), idx.data_ptr(), st, ids.data_ptr(), mask.data_ptr(), lengths.data_ptr(), bad.data_ptr()))
            else:
                N.check(N.lib.tm_batch_collate_masked(self.handle, C.byref(how), C.byref(masking.struct(self.vocab, seed)), idx.data_ptr(), st, ids.data_ptr(),
                                                      res["labels"].data_ptr(), mask.data_ptr(), lengths.data_ptr(), bad.data_ptr()))
        return res

    def close(self):
        if self.handle:
            N.lib.tm_batch_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tokenize_resident(vocab, docs, *, raw=True, device=None):
    """documents (bytes or str; raw=False: already normalized bytes) tokenized ONCE, their ids kept on the device -> ResidentBatch: batches in
    any order, as often as wanted - a shuffled batch per step, batches of documents of similar length padded to their own maximum."""
    return ResidentBatch(vocab, docs, raw, device)


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
