"""Vocab: host-side mirror of the reference's tokenize API over the HIP library.

Method names follow python/tokenmonster.py (tokenize :410, tokenize_count :497, len, max_token_length,
capcode, charset, unk_token_id ...) and go/tokenmonster.go:953-1014; every tokenize variant is a batch
call into libtokenmonster_hip.so.  Decoding, vocabulary editing, YAML import/export and the training
CLIs are out of scope and are not provided."""
import ctypes as C

import numpy as np

from . import _native as N
from . import synth as _synth


def pack_documents(docs):
    """list of bytes-like -> (text u8[n], offsets u64[len+1]) : the packed layout of the C ABI"""
    docs = [bytes(d) if not isinstance(d, (bytes, bytearray)) else d for d in docs]
    offsets = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        np.cumsum([len(d) for d in docs], out=offsets[1:])
    text = np.frombuffer(b"".join(docs), dtype=np.uint8) if docs else np.zeros(0, np.uint8)
    return text, offsets


SPAN_UNITS = {"bytes": N.TM_UNIT_BYTES, "chars": N.TM_UNIT_CODEPOINTS, "utf16": N.TM_UNIT_UTF16}


def span_unit(name):
    """"bytes" | "chars" | "utf16" -> TM_UNIT_* (ValueError for anything else, before any device call)"""
    if name not in SPAN_UNITS:
        raise ValueError('offset unit %r: "bytes", "chars" or "utf16"' % (name,))
    return SPAN_UNITS[name]


class VocabBlock(C.Structure):
    """tm_vocab_block (include/tokenmonster_hip.h): what a process needs besides the bytes of a vocabulary's device block"""
    _fields_ = [("bytes", C.c_uint64), ("part_bytes", C.c_uint64 * 8)] + [(n, C.c_uint32) for n in (
        "idle_off", "n_da", "n_info", "max_len", "off", "bstart", "spl_hint", "link_off", "direct_off", "delete_id", "unk_id",
        "n_ids", "vocab_size", "capcode", "charset", "norm_flag", "level", "reserve", "n_nodes", "pad")]


class Vocab:
    def __init__(self, image, sample=None):
        """tm_vocab_load; with `sample` (normalized text the vocabulary will be used on) tm_vocab_load_sample: tables laid out by use from the start"""
        self._image = bytes(image)
        h = C.c_void_p()
        buf = np.frombuffer(self._image, dtype=np.uint8)
        if sample is None:
            N.check(N.lib.tm_vocab_load(N.ptr(buf), buf.size, C.byref(h)))
        else:
            data = np.ascontiguousarray(sample, dtype=np.uint8)
            N.check(N.lib.tm_vocab_load_sample(N.ptr(buf), buf.size, N.ptr(data), data.size, C.byref(h)))
        self._h = h

    # ---- the device block from process to process (tm_vocab_block_export / _import: the data-parallel scoring mode) ----
    def export_block(self):
        """-> (description as bytes, device pointer of the block, its size): send the description, broadcast the block"""
        m, p = VocabBlock(), C.c_void_p()
        N.check(N.lib.tm_vocab_block_export(self._h, C.byref(m), C.byref(p)))
        return bytes(m), int(p.value), int(m.bytes)

    @classmethod
    def import_block(cls, description, device=0):
        """an empty vocabulary of the described shape on `device` -> (Vocab, device pointer to fill with the exporter's block before use)"""
        m = VocabBlock.from_buffer_copy(description)
        h, p = C.c_void_p(), C.c_void_p()
        N.check(N.lib.tm_vocab_block_import(C.byref(m), int(device), C.byref(h), C.byref(p)))
        v = cls.__new__(cls)
        v._image, v._h = b"", h
        return v, int(p.value), int(m.bytes)

    @classmethod
    def from_tokens(cls, tokens, capcode=0, charset=1, norm_flag=0, level=5, with_unk=False, special=None, device=0):
        """a vocabulary straight from a token list (tm_vocab_build: the trainvocab worker's per-candidate step, training/trainvocab.go:530-907),
        without the .vocab image in between; `image()` writes it on request"""
        tokens = [bytes(t) for t in tokens]
        blob = np.frombuffer(b"".join(tokens), dtype=np.uint8) if tokens else np.zeros(0, np.uint8)
        off = np.zeros(len(tokens) + 1, dtype=np.uint32)
        np.cumsum([len(t) for t in tokens], out=off[1:])
        sp = None if special is None else np.ascontiguousarray(np.asarray(special, dtype=np.uint8))
        h = C.c_void_p()
        N.check(N.lib.tm_vocab_build(N.ptr(blob), N.ptr(off), len(tokens), N.ptr(sp), capcode, charset, norm_flag, level, 1 if with_unk else 0, int(device), C.byref(h)))
        v = cls.__new__(cls)
        v._image, v._h = b"", h
        return v

    def image(self):
        """the bytes of the .vocab file of this vocabulary (tm_vocab_image)"""
        p, n = C.c_void_p(), C.c_size_t()
        N.check(N.lib.tm_vocab_image(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value)

    def close(self):
        if getattr(self, "_h", None):
            N.lib.tm_vocab_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- metadata (python/tokenmonster.py:Vocab properties; go/tokenmonster.go:2366-2597) ----
    def __len__(self):
        return N.lib.tm_vocab_size(self._h)

    @property
    def handle(self):
        return self._h

    def max_token_length(self):
        return N.lib.tm_vocab_max_token_length(self._h)

    def capcode(self):
        return N.lib.tm_vocab_capcode(self._h)

    def charset(self):
        return N.lib.tm_vocab_charset(self._h)

    def normalization_code(self):
        return N.lib.tm_vocab_normalization(self._h)

    def n_info(self):
        return N.lib.tm_vocab_n_info(self._h)

    def n_ids(self):
        return N.lib.tm_vocab_n_ids(self._h)

    def tune(self, normalized_sample):
        """tm_vocab_tune: the tables laid out by use on a sample of NORMALIZED text (results unchanged; worth it for large vocabularies)"""
        data = N.as_u8(normalized_sample)
        N.check(N.lib.tm_vocab_tune(self._h, N.ptr(data), data.size))

    def unk_token_id(self):
        u = N.lib.tm_vocab_unk(self._h)
        return None if u == N.TM_NONE else u

    def delete_token_id(self):
        u = N.lib.tm_vocab_delete_token(self._h)
        return None if u == N.TM_NONE else u

    # ---- normalization pre-step (go/tokenmonster.go:953 Normalize) ----
    def normalize(self, data):
        return _synth.normalize(data, self.capcode(), self.normalization_code())

    def normalize_origins(self, data):
        """one raw document -> (normalized bytes - Vocab.normalize's -, own u32[n]): own[k] is the offset in `data` of the first byte of the
        character (unit) that normalized byte k came from (tm_normalize_origins)"""
        data = N.as_u8(data)
        out, own, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        N.check(N.lib.tm_normalize_origins(N.ptr(data), data.size, self.capcode(), self.normalization_code(), C.byref(out), C.byref(n), C.byref(own)))
        try:
            o = np.frombuffer(C.string_at(own.value, 4 * n.value), dtype=np.uint32).copy() if n.value else np.zeros(0, dtype=np.uint32)
        finally:
            N.lib.tm_free(own)
        return N.take(out, n.value), o

    def normalize_packed_device(self, raw_text, raw_offsets):
        """norm.Normalize + capcode.Encode of packed raw documents ON THE GPU (tm_batch_normalize; documents with
        other non-ASCII content fall back to the host normalizer inside the library)
        -> (normalized text u8, offsets u64[D+1], number of host-fallback documents)"""
        raw_text = N.as_u8(raw_text)
        raw_offsets = np.ascontiguousarray(raw_offsets, dtype=np.uint64)
        nd = raw_offsets.size - 1
        cap = int(raw_text.size * 4 + 16 * nd + 1024)
        b = C.c_void_p()
        N.check(N.lib.tm_batch_create(self._h, cap, max(nd, 1), C.byref(b)))
        try:
            N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw_text), N.ptr(raw_offsets), nd))
            N.check(N.lib.tm_batch_normalize(b, None))
            n = int(N.lib.tm_batch_normalized_bytes(b))
            text = np.empty(max(n, 1), dtype=np.uint8)
            offs = np.zeros(nd + 1, dtype=np.uint64)
            N.check(N.lib.tm_batch_download_text(b, N.ptr(text), n, N.ptr(offs)))
            return text[:n], offs, int(N.lib.tm_batch_host_fallback_docs(b))
        finally:
            N.lib.tm_batch_free(b)

    # ---- tokenize ----
    def tokenize_packed(self, text, offsets):
        """normalized packed documents -> (ids u32[T], tok_offsets u64[D+1], missing u32[D])"""
        text = N.as_u8(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nd = offsets.size - 1
        tok_off = np.zeros(nd + 1, dtype=np.uint64)
        missing = np.zeros(max(nd, 1), dtype=np.uint32)
        cap = int(text.size // 2 + 2 * nd + 64)
        while True:
            out = np.empty(cap, dtype=np.uint32)
            rc = N.lib.tm_tokenize_batch(self._h, N.ptr(text), N.ptr(offsets), nd, N.ptr(out), cap, N.ptr(tok_off), N.ptr(missing))
            if rc == N.TM_E_NOSPACE:
                cap = int(tok_off[nd])
                continue
            N.check(rc)
            return out[: int(tok_off[nd])], tok_off, missing[:nd]

    def tokenize_spans_packed(self, text, offsets, unit="bytes"):
        """normalized packed documents -> (ids u32[T], tok_offsets u64[D+1], spans u32[T, 2], missing u32[D]): spans[k] = (begin, end) of the
        bytes id k came from, counted from its document's start (tm_tokenize_batch_spans_in, TM_TEXT_NORMALIZED).  unit: "bytes", or "chars"
        (code points) / "utf16" (UTF-16 units) by the rule of include/tokenmonster_hip.h"""
        unit = span_unit(unit)
        text = N.as_u8(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nd = offsets.size - 1
        tok_off = np.zeros(nd + 1, dtype=np.uint64)
        missing = np.zeros(max(nd, 1), dtype=np.uint32)
        cap = int(text.size // 2 + 2 * nd + 64)
        while True:
            out = np.empty(cap, dtype=np.uint32)
            spans = np.empty((cap, 2), dtype=np.uint32)
            rc = N.lib.tm_tokenize_batch_spans_in(self._h, N.ptr(text), N.ptr(offsets), nd, N.TM_TEXT_NORMALIZED, unit, N.ptr(out), cap, N.ptr(tok_off), N.ptr(spans),
                                                  N.ptr(missing))
            if rc == N.TM_E_NOSPACE:
                cap = int(tok_off[nd])
                continue
            N.check(rc)
            n = int(tok_off[nd])
            return out[:n], tok_off, spans[:n], missing[:nd]

    def tokenize_raw_spans_packed(self, raw_text, raw_offsets, unit="bytes"):
        """RAW packed documents -> (ids u32[T], tok_offsets u64[D+1], spans u32[T, 2], number of documents mapped on the host): spans[k] =
        (begin, end) of the bytes id k came from, counted from its document's start in the raw text (tm_batch_upload_raw,
        tm_batch_normalize, tm_batch_run, tm_batch_spans_in with TM_TEXT_RAW - the batch calls, which report the host's documents).  unit:
        "bytes", or "chars" (code points: the index into the decoded str) / "utf16" (UTF-16 units) by the rule of include/tokenmonster_hip.h"""
        unit = span_unit(unit)
        raw_text = N.as_u8(raw_text)
        raw_offsets = np.ascontiguousarray(raw_offsets, dtype=np.uint64)
        nd = raw_offsets.size - 1
        b = C.c_void_p()
        N.check(N.lib.tm_batch_create(self._h, int(raw_text.size * 4 + 16 * nd + 1024), max(nd, 1), C.byref(b)))
        try:
            N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw_text), N.ptr(raw_offsets), nd))
            N.check(N.lib.tm_batch_normalize(b, None))
            N.check(N.lib.tm_batch_run(b, None))
            n = C.c_uint64()
            N.check(N.lib.tm_batch_totals(b, C.byref(n), None))
            n = int(n.value)
            ids = np.zeros(max(n, 1), dtype=np.uint32)
            tok_off = np.zeros(nd + 1, dtype=np.uint64)
            N.check(N.lib.tm_batch_download(b, N.ptr(ids), n, N.ptr(tok_off), None))
            spans = PinnedBuffer(8 * max(n, 1))
            host_docs = C.c_uint32()
            N.check(N.lib.tm_batch_spans_in(b, None, N.TM_TEXT_RAW, unit, spans.array.ctypes.data, n, C.byref(host_docs), None))
            N.check(N.lib.tm_batch_totals(b, None, None))                     # (waits for the NULL stream)
            return ids[:n], tok_off, spans.array[:8 * n].view(np.uint32).reshape(n, 2).copy(), int(host_docs.value)
        finally:
            N.lib.tm_batch_free(b)

    def tokenize_normalized(self, docs):
        """list of already-normalized documents -> list of uint32 arrays (Vocab.tokenize, go :1017)"""
        single = isinstance(docs, (bytes, bytearray, np.ndarray))
        text, offsets = pack_documents([docs] if single else docs)
        ids, off, missing = self.tokenize_packed(text, offsets)
        res = [ids[int(off[d]): int(off[d + 1])] for d in range(offsets.size - 1)]
        return (res[0], int(missing[0])) if single else (res, missing)

    def tokenize(self, docs):
        """raw text -> ids (go :959 Tokenize = normalize + tokenize; python/tokenmonster.py:410).  The normalization
        pre-step runs on the device too (tm_batch_upload_raw + tm_batch_normalize)."""
        single = isinstance(docs, (bytes, bytearray, str))
        lst = [docs] if single else list(docs)
        lst = [d.encode("utf-8") if isinstance(d, str) else d for d in lst]
        text, offsets = pack_documents(lst)
        nd = offsets.size - 1
        b = C.c_void_p()
        N.check(N.lib.tm_batch_create(self._h, int(text.size * 4 + 16 * nd + 1024), max(nd, 1), C.byref(b)))
        try:
            N.check(N.lib.tm_batch_upload_raw(b, N.ptr(text), N.ptr(offsets), nd))
            N.check(N.lib.tm_batch_normalize(b, None))
            N.check(N.lib.tm_batch_run(b, None))
            ntok = C.c_uint64()
            N.check(N.lib.tm_batch_totals(b, C.byref(ntok), None))
            ids = np.empty(max(int(ntok.value), 1), dtype=np.uint32)
            off = np.zeros(nd + 1, dtype=np.uint64)
            N.check(N.lib.tm_batch_download(b, N.ptr(ids), int(ntok.value), N.ptr(off), None))
        finally:
            N.lib.tm_batch_free(b)
        res = [ids[int(off[d]): int(off[d + 1])] for d in range(nd)]
        return res[0] if single else res

    def decode_packed(self, ids, tok_offsets, raw=False):
        """Decode (go/tokenmonster.go:445) of packed id streams -> (bytes u8, offsets u64[D+1]); raw=True: decode_raw"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        tok_offsets = np.ascontiguousarray(tok_offsets, dtype=np.uint64)
        nd = tok_offsets.size - 1
        ooff = np.zeros(nd + 1, dtype=np.uint64)
        cap = int(ids.size * 8 + 64)
        while True:
            out = np.empty(cap, dtype=np.uint8)
            rc = N.lib.tm_decode_batch(self._h, N.ptr(ids), N.ptr(tok_offsets), nd, 1 if raw else 0, N.ptr(out), cap, N.ptr(ooff))
            if rc == N.TM_E_NOSPACE:
                cap = int(ooff[nd])
                continue
            N.check(rc)
            return out[: int(ooff[nd])], ooff

    def roundtrip_resident(self, raw_text, raw_offsets, raw=False):
        """raw documents -> ids -> text without the ids leaving the device: tm_batch_upload_raw + tm_batch_normalize + tm_batch_run, then
        tm_batch_decode on the ids the batch holds -> (decoded text u8, offsets u64[D+1], documents the device left to the host decoder)"""
        raw_text = N.as_u8(raw_text)
        raw_offsets = np.ascontiguousarray(raw_offsets, dtype=np.uint64)
        nd = raw_offsets.size - 1
        b = C.c_void_p()
        N.check(N.lib.tm_batch_create(self._h, int(raw_text.size * 4 + 16 * nd + 1024), max(nd, 1), C.byref(b)))
        try:
            N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw_text), N.ptr(raw_offsets), nd))
            N.check(N.lib.tm_batch_normalize(b, None))
            N.check(N.lib.tm_batch_run(b, None))
            nbytes, host_docs = C.c_uint64(), C.c_uint32()
            N.check(N.lib.tm_batch_decode(b, 1 if raw else 0, None, C.byref(nbytes), C.byref(host_docs)))
            ooff = np.zeros(nd + 1, dtype=np.uint64)
            cap = int(raw_text.size * 2 + 64)
            while True:
                out = np.empty(cap, dtype=np.uint8)
                rc = N.lib.tm_batch_decoded_download(b, N.ptr(out), cap, N.ptr(ooff))
                if rc == N.TM_E_NOSPACE:
                    cap = int(ooff[nd])
                    continue
                N.check(rc)
                return out[: int(ooff[nd])], ooff, int(host_docs.value)
        finally:
            N.lib.tm_batch_free(b)

    def decode(self, ids):
        """one id sequence -> bytes (python/tokenmonster.py:341 decode)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out, _ = self.decode_packed(ids, np.array([0, ids.size], dtype=np.uint64))
        return out.tobytes()

    def decoder(self):
        return Decoder(self)

    def encoder(self, max_piece_bytes=0):
        """streaming encoder (tm_encoder_new): ONE document of normalized text fed piece by piece, ids exactly those of tokenizing it whole"""
        return Encoder(self, max_piece_bytes)

    def tokenize_normalized_stream(self, pieces, max_piece_bytes=0):
        """an iterable of pieces of ONE already-normalized document -> (ids u32, missing): tokenize_normalized of their concatenation,
        with device memory that depends on max_piece_bytes (0 = 32 MiB) only"""
        enc = self.encoder(max_piece_bytes)
        try:
            parts = [enc.feed(p) for p in pieces]
            last, missing = enc.finish()
        finally:
            enc.close()
        parts = [p for p in parts if p.size] + [last]
        return (np.concatenate(parts) if len(parts) > 1 else last), missing

    def encoder_raw_supported(self):
        """whether Encoder.feed_raw takes this vocabulary's raw text (capcode 0 or 2, none of the flags quotemarks, trim, leadingspace)"""
        return bool(N.lib.tm_encoder_raw_supported(self._h))

    def tokenize_raw_stream(self, pieces, max_piece_bytes=0):
        """an iterable of pieces of ONE raw document, cut anywhere -> (ids u32, missing): tokenize of the whole text normalized at once,
        with device memory that depends on max_piece_bytes (0 = 32 MiB) only"""
        enc = self.encoder(max_piece_bytes)
        try:
            parts = [enc.feed_raw(p) for p in pieces]
            last, missing = enc.finish()
        finally:
            enc.close()
        parts = [p for p in parts if p.size] + [last]
        return (np.concatenate(parts) if len(parts) > 1 else last), missing

    def count_packed(self, text, offsets):
        """Count (go :971 / :1281): b-branches count once (quirk Q2) -> (counts u64[D], missing u32[D])"""
        text = N.as_u8(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nd = offsets.size - 1
        counts = np.zeros(max(nd, 1), dtype=np.uint64)
        missing = np.zeros(max(nd, 1), dtype=np.uint32)
        N.check(N.lib.tm_count_batch(self._h, N.ptr(text), N.ptr(offsets), nd, N.ptr(counts), N.ptr(missing)))
        return counts[:nd], missing[:nd]

    def tokenize_count(self, docs):
        single = isinstance(docs, (bytes, bytearray, str))
        lst = [docs] if single else list(docs)
        lst = [d.encode("utf-8") if isinstance(d, str) else d for d in lst]
        text, offsets = pack_documents(lst)
        ntext, noff = _synth.normalize_batch(text, offsets, self.capcode(), self.normalization_code())
        counts, _ = self.count_packed(ntext, noff)
        return int(counts[0]) if single else counts

    def tokenize_serialized_packed(self, text, offsets, encoding_length=0):
        """TokenizeToSerialized (go :986) on normalized packed documents -> (bytes u8, byte_offsets, missing, enc)"""
        text = N.as_u8(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nd = offsets.size - 1
        boff = np.zeros(nd + 1, dtype=np.uint64)
        missing = np.zeros(max(nd, 1), dtype=np.uint32)
        enc = C.c_uint32()
        cap = int(text.size * 2 + 8 * nd + 64)
        while True:
            out = np.empty(cap, dtype=np.uint8)
            rc = N.lib.tm_tokenize_batch_serialized(self._h, N.ptr(text), N.ptr(offsets), nd, encoding_length, N.ptr(out), cap,
                                                    N.ptr(boff), N.ptr(missing), C.byref(enc))
            if rc == N.TM_E_NOSPACE:
                cap = int(boff[nd])
                continue
            N.check(rc)
            return out[: int(boff[nd])], boff, missing[:nd], enc.value


    def tokenize_pipeline(self, text, offsets, raw=True, encoding_length=0, chunk_bytes=0, lanes=0, out=None):
        """host-to-host tokenization of a large packed corpus (tm_tokenize_pipeline): chunks of documents run
        H2D | normalize + tokenize + serialize | D2H on several lanes at once.  -> (serialized ids u8, byte_offsets u64[D+1],
        missing u32[D], encoding length, stats dict).  `text` / `out` may be pinned arrays from pinned_empty()."""
        text = N.as_u8(text)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nd = offsets.size - 1
        boff = np.zeros(nd + 1, dtype=np.uint64)
        missing = np.zeros(max(nd, 1), dtype=np.uint32)
        enc = C.c_uint32()
        stats = PipelineStats()
        if out is None:
            out = np.empty(int(text.size) + 8 * nd + 64, dtype=np.uint8)
        while True:
            rc = N.lib.tm_tokenize_pipeline(self._h, N.ptr(text), N.ptr(offsets), nd, 1 if raw else 0, encoding_length, chunk_bytes, lanes,
                                            N.ptr(out), out.size, N.ptr(boff), N.ptr(missing), C.byref(enc), C.byref(stats))
            if rc == N.TM_E_NOSPACE:
                out = np.empty(int(boff[nd]), dtype=np.uint8)
                continue
            N.check(rc)
            st = {k: getattr(stats, k) for k, _ in PipelineStats._fields_}
            return out[: int(boff[nd])], boff, missing[:nd], enc.value, st

    def tokenize_document(self, data, raw=True, encoding_length=0, piece_bytes=0, slots=0, out=None):
        """ONE large document host to host (tm_tokenize_document): its pieces of piece_bytes (0 = 32 MiB) run through `slots` (0 = 3) device
        workspaces at once, upload | match | resolve + emit | download overlapped.  -> (ids, missing, stats dict): the ids of tokenize /
        tokenize_normalized of the whole text as uint16 (encoding_length 2), uint32 (3 and 4; 0 = by the size of the vocabulary).
        `data`: bytes, a numpy uint8 array or a PinnedBuffer; `out` (numpy uint8 or PinnedBuffer) receives the serialized ids."""
        if isinstance(data, PinnedBuffer):
            data = data.array
        if isinstance(out, PinnedBuffer):
            out = out.array
        if isinstance(data, str):
            data = data.encode("utf-8")
        text = N.as_u8(data)
        need, miss, enc = C.c_uint64(), C.c_uint32(), C.c_uint32()
        stats = DocumentStats()
        if out is None:
            out = np.empty(int(text.size) + 64, dtype=np.uint8)
        while True:
            rc = N.lib.tm_tokenize_document(self._h, N.ptr(text) if text.size else None, text.size, 1 if raw else 0, encoding_length, piece_bytes, slots,
                                            N.ptr(out), out.size, C.byref(need), C.byref(miss), C.byref(enc), C.byref(stats))
            if rc == N.TM_E_NOSPACE:
                out = np.empty(int(need.value), dtype=np.uint8)
                continue
            N.check(rc)
            break
        st = {k: getattr(stats, k) for k, _ in DocumentStats._fields_}
        st["encoding_length"] = enc.value
        packed = out[: int(need.value)]
        if enc.value == 2:
            ids = packed.view("<u2")
        elif enc.value == 4:
            ids = packed.view("<u4")
        else:
            t = packed.reshape(-1, 3).astype(np.uint32)
            ids = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        return ids, int(miss.value), st


class Decoder:
    """streaming decoder (go/tokenmonster.go:552-700 NewDecoder; python/tokenmonster.py Decoder): feed ids a few at a time, get the
    text that is complete so far; partial UTF-8 sequences and the capcode state carry over to the next call"""

    def __init__(self, vocab):
        self._vocab = vocab
        self._h = C.c_void_p()
        N.check(N.lib.tm_decoder_new(vocab.handle, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            N.lib.tm_decoder_free(self._h)
            self._h = None

    def _call(self, fn, *args):
        n = C.c_uint64()
        out = np.empty(4096, dtype=np.uint8)
        rc = fn(self._h, *args, N.ptr(out), out.size, C.byref(n))
        if rc == N.TM_E_NOSPACE:         # the ids were consumed; fetch the text with a buffer of the reported size
            out = np.empty(int(n.value), dtype=np.uint8)
            rc = N.lib.tm_decoder_decode(self._h, None, 0, N.ptr(out), out.size, C.byref(n))
        N.check(rc)
        return out[: int(n.value)].tobytes()

    def decode(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        return self._call(N.lib.tm_decoder_decode, N.ptr(ids), ids.size)

    def decode_serialized(self, data, encoding_length=0):
        d = N.as_u8(data)
        return self._call(N.lib.tm_decoder_decode_serialized, N.ptr(d), d.size, encoding_length)

    def flush(self):
        n = C.c_uint64()
        out = np.empty(64, dtype=np.uint8)
        rc = N.lib.tm_decoder_flush(self._h, N.ptr(out), out.size, C.byref(n))
        if rc == N.TM_E_NOSPACE:         # the remainder (a run of continuation bytes can be long) has been kept: fetch it with a buffer of the reported size
            out = np.empty(int(n.value), dtype=np.uint8)
            rc = N.lib.tm_decoder_decode(self._h, None, 0, N.ptr(out), out.size, C.byref(n))
        N.check(rc)
        return out[: int(n.value)].tobytes()


class Encoder:
    """streaming encoder (tm_encoder_*): feed() the normalized text of ONE document in pieces of any size and get the ids that are final
    so far; finish() says the text ends and returns (remaining ids, missing) - all ids together are those of the whole document tokenized
    at once, however it was cut.  feed_raw() takes the document's RAW text instead (one document goes through one of the two): the library
    cuts it behind line feeds, where the normalizer has no state, and keeps what lies behind the last one (raw_held) until more text or
    finish() comes.  Vocabularies with the flags quotemarks, trim or leadingspace, or capcode 1, are normalized whole (Vocab.encoder_raw_supported)."""

    def __init__(self, vocab, max_piece_bytes=0):
        self._vocab = vocab
        self._h = C.c_void_p()
        N.check(N.lib.tm_encoder_new(vocab.handle, int(max_piece_bytes), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            N.lib.tm_encoder_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ids(self, call, guess):
        n = C.c_uint64()
        out = np.empty(max(int(guess), 64), dtype=np.uint32)
        rc = call(N.ptr(out), out.size, C.byref(n))
        if rc == N.TM_E_NOSPACE:         # the text was consumed and the ids are kept: fetch them with a buffer of the reported size
            out = np.empty(int(n.value), dtype=np.uint32)
            rc = N.lib.tm_encoder_feed(self._h, None, 0, N.ptr(out), out.size, C.byref(n))
        N.check(rc)
        return out[: int(n.value)]

    def feed(self, data):
        d = N.as_u8(data)
        return self._ids(lambda out, cap, n: N.lib.tm_encoder_feed(self._h, N.ptr(d), d.size, out, cap, n), d.size // 2 + 256)

    def feed_raw(self, data):
        d = N.as_u8(data)
        return self._ids(lambda out, cap, n: N.lib.tm_encoder_feed_raw(self._h, N.ptr(d), d.size, out, cap, n), d.size // 2 + 256)

    @property
    def raw_held(self):
        """raw bytes kept on the host behind the last safe cut"""
        return int(N.lib.tm_encoder_raw_held(self._h))

    @property
    def host_pieces(self):
        """raw pieces of the current (after finish: the last) document that the host normalizer took"""
        return int(N.lib.tm_encoder_host_pieces(self._h))

    def finish(self):
        missing = C.c_uint32()
        ids = self._ids(lambda out, cap, n: N.lib.tm_encoder_finish(self._h, out, cap, n, C.byref(missing)), 512)
        return ids, int(missing.value)

    def reset(self):
        N.check(N.lib.tm_encoder_reset(self._h))

    @property
    def state(self):
        """the entry state (0..79: 2 * offset of the next token start + pending forward delete) the next pass will start in"""
        return int(N.lib.tm_encoder_state(self._h))

    def device_bytes(self):
        return int(N.lib.tm_encoder_device_bytes(self._h))


class PipelineStats(C.Structure):
    _fields_ = [("chunks", C.c_uint32), ("lanes", C.c_uint32), ("input_pinned", C.c_int), ("output_pinned", C.c_int),
                ("normalized_bytes", C.c_uint64), ("host_fallback_docs", C.c_uint32), ("ring", C.c_uint32), ("ring_exact_chunks", C.c_uint32)]


class DocumentStats(C.Structure):
    _fields_ = [("pieces", C.c_uint32), ("slots", C.c_uint32), ("input_pinned", C.c_int), ("output_pinned", C.c_int), ("normalized_bytes", C.c_uint64),
                ("host_pieces", C.c_uint32), ("host_normalized", C.c_uint32), ("device_bytes", C.c_uint64)]


class PinnedBuffer:
    """page-locked host memory (tm_host_alloc) viewed as a numpy uint8 array; freed with the object"""

    def __init__(self, nbytes):
        self._p = N.lib.tm_host_alloc(max(int(nbytes), 16))
        if not self._p:
            raise MemoryError("tm_host_alloc(%d) failed" % nbytes)
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(int(nbytes), 16)).from_address(self._p))[: int(nbytes)]

    def __del__(self):
        if getattr(self, "_p", None):
            self.array = None
            N.lib.tm_host_free(self._p)
            self._p = None


def load(path_or_bytes):
    """load a .vocab file (go/tokenmonster.go:2656 Load; python/tokenmonster.py load) onto the current GPU"""
    if isinstance(path_or_bytes, (bytes, bytearray)):
        return Vocab(path_or_bytes)
    with open(path_or_bytes, "rb") as f:
        return Vocab(f.read())
