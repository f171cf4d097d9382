"""-m gpu: tokenmonster_amd.torch_api.encode_pairs and encode_pair_windows on CUDA tensors, on a torch stream of the caller's, against what the
C ABI (tm_batch_pair, tm_batch_pair_windows and their span forms, tested in tests/test_gpu_pairs.py) writes for the same documents uploaded as one
batch, first sides then second sides.  Needs a real device and torch: on the emulated leg, and wherever torch has no device, it is skipped.

As in tests/test_gpu_windows_torch.py the cases run in ONE child process that imports torch first - this file as a script - and every test
below asserts on what the child recorded for its case."""
import ctypes as C
import json
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
TRUNCATION = {"longest_first": 0, "only_first": 1, "only_second": 2}
UNITS = {"bytes": 0, "chars": 1, "utf16": 2}


def make_env():
    import torch
    import tokenmonster_amd as tm
    from tokenmonster_amd import _native as N
    from tokenmonster_amd import synth, torch_api
    from test_gpu_pairs import LETTERS, vocab_tokens
    rng = np.random.default_rng(88201)
    v = tm.Vocab(synth.build_vocab(vocab_tokens(), capcode=2, charset=1, norm_flag=1, with_unk=True))

    def letters(n):
        return bytes(LETTERS[int(x)] for x in rng.integers(0, len(LETTERS), size=n))

    first = [letters(int(n)) for n in rng.integers(0, 30, size=30)] + [b"", b"a", "Hello WORLD zzé Éa".encode(), b"", letters(90), "ab😀cd é".encode(), b""]
    second = [letters(int(n)) for n in rng.integers(0, 60, size=30)] + [b"", b"", letters(200), letters(7), "É zu 😀 Zzu".encode() + letters(40), letters(3), b"abc"]
    assert len(first) == len(second)
    docs = first + second
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, 1 << 16, 128, C.byref(b)))
    n = v.n_ids()
    env = dict(torch=torch, api=torch_api, v=v, N=N, tm=tm, first=first, second=second, b=b, n=len(first), pad=n + 1, bos=n + 2, sep=n + 3, eos=n + 4,
               stream=torch.cuda.Stream())
    load(env, docs, raw=True)
    return env


def load(env, docs, raw):
    """the C ABI's batch holds `docs`: uploaded raw and normalized on the device, or as they are"""
    N, b = env["N"], env["b"]
    text, offs = env["tm"].pack_documents(docs)
    if raw:
        N.check(N.lib.tm_batch_upload_raw(b, N.ptr(text), N.ptr(offs), len(docs)))
        N.check(N.lib.tm_batch_normalize(b, None))
    else:
        N.check(N.lib.tm_batch_upload(b, N.ptr(text), N.ptr(offs), len(docs)))
    N.check(N.lib.tm_batch_run(b, None))


def host(torch, t):
    """a CUDA tensor -> numpy with its bits unsigned"""
    a = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()]).cpu().numpy()
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64, 1: np.uint8}[t.element_size()])


def abi(env, L, id_bytes, bos, sep, nsep, eos, truncation, pad_left, windows=None, offsets=None):
    """what the C ABI writes for the pairs of the batch -> dict of numpy arrays under the keys of the torch result (windows: (overlap, max_first);
    offsets: (text, unit))"""
    from fixed_shape import Out, DT, NONE, PAD_LEFT
    from test_gpu_pairs import Pair
    N, b, n = env["N"], env["b"], env["n"]

    def s(x):
        return NONE if x is None else x

    how = Pair(0, n, n, L, id_bytes, env["pad"], s(bos), s(sep), s(eos), nsep if sep is not None else 0, TRUNCATION[truncation], PAD_LEFT if pad_left else 0)
    if windows is None:
        rows = n
        o = [Out(rows * L, id_bytes), Out(rows * L, 1), Out(rows * L, 1), Out(2 * rows, 4)]
        N.check(N.lib.tm_batch_pair(b, C.byref(how), None, *[x.ptr for x in o]))
    else:
        need = C.c_uint64()
        N.check(N.lib.tm_batch_pair_window_rows(b, C.byref(how), windows[0], windows[1], C.byref(need)))
        rows = int(need.value)
        o = [Out(rows * L, id_bytes), Out(rows * L, 1), Out(rows * L, 1), Out(2 * rows, 4), Out(rows, 4), Out(rows, 4)]
        N.check(N.lib.tm_batch_pair_windows(b, C.byref(how), windows[0], windows[1], None, rows, *[x.ptr for x in o]))
    so = None
    if offsets is not None:
        so = Out(rows * L * 2, 8)
        if windows is None:
            N.check(N.lib.tm_batch_pair_spans_in(b, C.byref(how), None, offsets[0], offsets[1], so.ptr, 8))
        else:
            N.check(N.lib.tm_batch_pair_windows_spans_in(b, C.byref(how), windows[0], windows[1], None, rows, offsets[0], offsets[1], so.ptr, 8))
    N.check(N.lib.tm_batch_totals(b, None, None))          # (the NULL stream: waits for all of it)
    assert all(x.sentinels_intact() for x in o + ([so] if so else []))
    res = {"input_ids": o[0].view(DT[id_bytes]).reshape(rows, L).copy(), "attention_mask": o[1].view(np.uint8).reshape(rows, L).copy(),
           "token_type_ids": o[2].view(np.uint8).reshape(rows, L).copy(), "kept": o[3].view(np.uint32).reshape(rows, 2).copy()}
    if windows is not None:
        res["overflow_to_sample_mapping"] = o[4].view(np.uint32).copy()
        res["window_start"] = o[5].view(np.uint32).copy()
    if so is not None:
        res["offset_mapping"] = so.view(np.uint64).reshape(rows, L, 2).copy()
    return res


def check(env, out, exp, dtype):
    """the torch result against the C ABI's: the same keys, shapes, dtypes as documented, and bits"""
    torch = env["torch"]
    assert set(out) == set(exp), (sorted(out), sorted(exp))
    want = {"input_ids": dtype, "attention_mask": torch.bool, "token_type_ids": torch.uint8, "kept": torch.int32, "overflow_to_sample_mapping": torch.int32,
            "window_start": torch.int32, "offset_mapping": torch.int64}
    for k, e in exp.items():
        assert out[k].is_cuda and out[k].dtype == want[k] and tuple(out[k].shape) == e.shape, (k, out[k].dtype, tuple(out[k].shape), e.shape)
        assert (host(torch, out[k]) == e).all(), k
    return exp["input_ids"].shape[0]


def sides(env, kind):
    if kind == "bytes":
        return env["first"], env["second"]
    return [d.decode("utf-8") for d in env["first"]], [d.decode("utf-8") for d in env["second"]]


def case_encode_pairs(env, dtype, kind, pad_left, truncation, nsep):
    """bytes and str documents; rows of 24 with every special"""
    torch, api, L = env["torch"], env["api"], 24
    first, second = sides(env, kind)
    dt = getattr(torch, dtype)
    with torch.cuda.stream(env["stream"]):
        out = api.encode_pairs(env["v"], first, second, L, pad_id=env["pad"], bos_id=env["bos"], sep_id=env["sep"], sep_count=nsep, eos_id=env["eos"], truncation=truncation,
                               pad_left=pad_left, dtype=dt)
        exp = abi(env, L, out["input_ids"].element_size(), env["bos"], env["sep"], nsep, env["eos"], truncation, pad_left)
        assert check(env, out, exp, dt) == env["n"]
    kept = exp["kept"].astype(np.int64)
    assert (kept.sum(axis=1) == L - 2 - nsep).any() and (kept.sum(axis=1) < L - 2 - nsep).any() and (kept.sum(axis=1) == 0).any()      # cut, padded and empty rows


def case_no_specials_default_truncation(env):
    torch, api = env["torch"], env["api"]
    with torch.cuda.stream(env["stream"]):
        out = api.encode_pairs(env["v"], env["first"], env["second"], 31, pad_id=env["pad"])
        check(env, out, abi(env, 31, 8, None, None, 0, None, "longest_first", False), torch.int64)
        out = api.encode_pairs(env["v"], env["first"], env["second"], 9, pad_id=env["pad"], sep_id=env["sep"], sep_count=2, dtype=torch.int32)
        check(env, out, abi(env, 9, 4, None, env["sep"], 2, None, "longest_first", False), torch.int32)


def case_offsets(env, form, unit, windows):
    torch, api, L = env["torch"], env["api"], 20
    kw = dict(pad_id=env["pad"], bos_id=env["bos"], sep_id=env["sep"], eos_id=env["eos"], offset_unit=unit)
    args = (L,) + ((3, 5) if windows else ())
    fn = api.encode_pair_windows if windows else api.encode_pairs
    trunc = "only_second" if windows else "longest_first"
    w = (3, 5) if windows else None
    with torch.cuda.stream(env["stream"]):
        if form == "raw":
            out = fn(env["v"], env["first"], env["second"], *args, return_offsets="raw", **kw)
            exp = abi(env, L, 8, env["bos"], env["sep"], 1, env["eos"], trunc, False, w, (1, UNITS[unit]))
        elif form == "normalized":
            out = fn(env["v"], env["first"], env["second"], *args, return_offsets=True, pad_left=True, **kw)
            exp = abi(env, L, 8, env["bos"], env["sep"], 1, env["eos"], trunc, True, w, (0, UNITS[unit]))
        else:                                        # documents passed in normalized
            norm = [env["v"].normalize(d) for d in env["first"] + env["second"]]
            load(env, norm, raw=False)
            try:
                out = fn(env["v"], norm[:env["n"]], norm[env["n"]:], *args, return_offsets=True, raw=False, **kw)
                exp = abi(env, L, 8, env["bos"], env["sep"], 1, env["eos"], trunc, False, w, (0, UNITS[unit]))
            finally:
                load(env, env["first"] + env["second"], raw=True)
        rows = check(env, out, exp, torch.int64)
    assert exp["offset_mapping"].any() and (rows > env["n"]) == bool(windows)


def case_encode_pair_windows(env, dtype, kind, pad_left, overlap, max_first):
    torch, api, L = env["torch"], env["api"], 24
    first, second = sides(env, kind)
    dt = getattr(torch, dtype)
    with torch.cuda.stream(env["stream"]):
        out = api.encode_pair_windows(env["v"], first, second, L, overlap, max_first, pad_id=env["pad"], bos_id=env["bos"], sep_id=env["sep"], eos_id=env["eos"], pad_left=pad_left,
                                      dtype=dt)
        exp = abi(env, L, out["input_ids"].element_size(), env["bos"], env["sep"], 1, env["eos"], "only_second", pad_left, (overlap, max_first))
        rows = check(env, out, exp, dt)
    assert rows > env["n"] + 10 and set(exp["overflow_to_sample_mapping"].tolist()) == set(range(env["n"])) and exp["window_start"].any()
    assert exp["kept"][:, 0].max() == max_first


def case_str_slices(env):
    """str documents, return_offsets="raw", offset_unit="chars": the pair of a content column slices its side's string to the text of the id - the
    bytes the raw byte span of that id covers (tm_batch_spans_in of the batch, TM_TEXT_RAW / TM_UNIT_BYTES)"""
    from fixed_shape import Out
    torch, api, N, b, n, L = env["torch"], env["api"], env["N"], env["b"], env["n"], 40
    first, second = sides(env, "str")
    total, m = C.c_uint64(), C.c_uint64()
    N.check(N.lib.tm_batch_totals(b, C.byref(total), C.byref(m)))
    total = int(total.value)
    ids = np.zeros(max(total, 1), dtype=np.uint32)
    toff = np.zeros(2 * n + 1, dtype=np.uint64)
    miss = np.zeros(2 * n, dtype=np.uint32)
    N.check(N.lib.tm_batch_download(b, N.ptr(ids), total, N.ptr(toff), N.ptr(miss)))
    sp = Out(2 * total, 4)
    N.check(N.lib.tm_batch_spans_in(b, None, 1, 0, sp.ptr, total, None, None))
    N.check(N.lib.tm_batch_totals(b, None, None))
    byte = sp.view(np.uint32).reshape(total, 2)
    with torch.cuda.stream(env["stream"]):
        out = api.encode_pairs(env["v"], first, second, L, pad_id=env["pad"], bos_id=env["bos"], sep_id=env["sep"], sep_count=2, eos_id=env["eos"], return_offsets="raw",
                               offset_unit="chars")
        got, rows, kept, types = [out[k].cpu().numpy() for k in ("offset_mapping", "input_ids", "kept", "token_type_ids")]      # (on the stream of the call)
    seen = 0
    for p in range(n):
        for side, (strs, raws, d, col0) in enumerate(((first, env["first"], p, 1), (second, env["second"], n + p, 1 + kept[p, 0] + 2))):
            if "\U0001F600" in strs[p]:          # (a character without a token is an unk id per byte: spans inside a character round outward)
                continue
            for j in range(int(kept[p, side])):
                t = int(toff[d]) + j
                c = col0 + j
                assert rows[p, c] == ids[t] and types[p, c] == side
                assert strs[p][got[p, c, 0]:got[p, c, 1]].encode("utf-8") == raws[p][byte[t, 0]:byte[t, 1]], (p, side, j)
                seen += 1
    assert seen > 200 and any(len(s.encode("utf-8")) != len(s) for s in first + second)


def case_refusals(env):
    torch, api, v = env["torch"], env["api"], env["v"]
    held = api.device_bytes(v)
    ok = dict(pad_id=env["pad"], bos_id=env["bos"], sep_id=env["sep"], eos_id=env["eos"])
    one = ([b"abc"], [b"de"])
    for fn, docs, args, kw in ((api.encode_pairs, ([b"abc"], [b"d", b"e"]), (8,), ok),                       # lists of unequal length
                               (api.encode_pairs, one, (8,), dict(ok, dtype=torch.float16)),
                               (api.encode_pairs, one, (2,), ok),                                             # no row beside the specials
                               (api.encode_pairs, one, (3,), dict(ok, sep_count=2)),
                               (api.encode_pairs, one, (0,), dict(pad_id=0)),
                               (api.encode_pairs, one, (8,), dict(ok, sep_count=3)),
                               (api.encode_pairs, one, (8,), dict(ok, sep_count=0)),
                               (api.encode_pairs, one, (8,), dict(ok, truncation="do_not_truncate")),
                               (api.encode_pairs, one, (8,), dict(ok, raw=False, return_offsets="raw")),
                               (api.encode_pairs, one, (8,), dict(ok, return_offsets="normalized")),
                               (api.encode_pairs, one, (8,), dict(ok, return_offsets=True, offset_unit="graphemes")),
                               (api.encode_pair_windows, ([b"abc"], []), (8, 1, 2), ok),
                               (api.encode_pair_windows, one, (8, 1, 2), dict(ok, truncation="longest_first")),
                               (api.encode_pair_windows, one, (8, 1, 2), dict(ok, truncation="only_first")),
                               (api.encode_pair_windows, one, (8, 0, 6), ok),                                 # max_first > room
                               (api.encode_pair_windows, one, (8, 3, 2), ok),                                 # room - max_first <= overlap
                               (api.encode_pair_windows, one, (8, -1, 2), ok),
                               (api.encode_pair_windows, one, (8, 1, -1), ok),
                               (api.encode_pair_windows, one, (3, 0, 0), ok),                                 # room 0 holds no window
                               (api.encode_pair_windows, one, (8, 1, 2), dict(ok, raw=False, return_offsets="raw")),
                               (api.encode_pair_windows, one, (8, 1, 2), dict(ok, return_offsets=True, offset_unit="graphemes"))):
        try:
            fn(v, docs[0], docs[1], *args, **kw)
        except ValueError:
            continue
        raise AssertionError("accepted %r %r %r" % (docs, args, kw))
    assert api.device_bytes(v) == held                               # every check ran before any device call
    # a row of specials only is a row
    out = api.encode_pairs(v, one[0], one[1], 3, **ok)
    assert host(torch, out["input_ids"]).tolist() == [[env["bos"], env["sep"], env["eos"]]] and not out["kept"].any()


CASES = {}
for _dtype, _kind, _left, _trunc, _nsep in (("int64", "bytes", False, "longest_first", 1), ("int32", "str", True, "only_second", 2), ("uint16", "bytes", True, "only_first", 1),
                                            ("int16", "str", False, "longest_first", 2)):
    CASES["encode_pairs[%s-%s-%s-%s-%d]" % (_dtype, _kind, "left" if _left else "right", _trunc, _nsep)] = (case_encode_pairs, (_dtype, _kind, _left, _trunc, _nsep))
for _dtype, _kind, _left, _overlap, _max_first in (("int64", "str", False, 0, 4), ("int32", "bytes", True, 3, 6), ("int16", "bytes", False, 16, 3)):
    CASES["encode_pair_windows[%s-%s-%s-%d-%d]" % (_dtype, _kind, "left" if _left else "right", _overlap, _max_first)] = (case_encode_pair_windows,
                                                                                                                          (_dtype, _kind, _left, _overlap, _max_first))
for _form, _unit, _win in (("raw", "bytes", False), ("normalized", "utf16", False), ("normalized_input", "chars", False), ("raw", "chars", True), ("normalized", "bytes", True),
                           ("normalized_input", "utf16", True)):
    CASES["offset_mapping[%s-%s-%s]" % (_form, _unit, "windows" if _win else "pairs")] = (case_offsets, (_form, _unit, _win))
CASES["no_specials_default_truncation"] = (case_no_specials_default_truncation, ())
CASES["str_slices"] = (case_str_slices, ())
CASES["argument_checks"] = (case_refusals, ())


def child_main(out_path):
    import torch                                     # first: its HIP runtime is the one the library then shares
    results = {}
    if not torch.cuda.is_available():
        results["__skip__"] = "torch has no device"
    else:
        torch.cuda.init()
        sys.path.insert(0, os.path.dirname(HERE))
        sys.path.insert(0, HERE)
        try:
            env = make_env()
        except Exception:      # noqa: BLE001
            results["__env__"] = traceback.format_exc()
            env = None
        for name, (fn, args) in CASES.items():
            if env is None:
                break
            try:
                fn(env, *args)
                results[name] = "ok"
            except Exception:      # noqa: BLE001
                results[name] = traceback.format_exc()
    with open(out_path, "w") as f:
        json.dump(results, f)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pairs_torch") / "results.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and os.path.exists(out), r.stdout.decode(errors="replace")[-4000:]
    res = json.load(open(out))
    if "__skip__" in res:
        pytest.skip(res["__skip__"])
    assert "__env__" not in res, res["__env__"]
    return res


@pytest.mark.parametrize("case", sorted(CASES))
def test_encode_pairs(results, case):
    assert results.get(case) == "ok", results.get(case)


if __name__ == "__main__":
    child_main(sys.argv[1])
