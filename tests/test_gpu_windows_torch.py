"""-m gpu: tokenmonster_amd.torch_api.encode_windows on CUDA tensors, on a torch stream of the caller's, against the numpy statement of the
window rule (tests/test_gpu_windows.py: np_windows) applied to Vocab's own ragged ids and spans.  Needs a real device and torch: not part of
the emulated leg; skipped when torch has no device.

As in tests/test_gpu_torch_api.py the cases run in ONE child process that imports torch first - this file as a script - and every test
below asserts on what the child recorded for its case."""
import json
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


def make_env():
    import torch
    import tokenmonster_amd as tm
    from tokenmonster_amd import synth, torch_api
    from test_gpu_windows import LETTERS, vocab_tokens
    rng = np.random.default_rng(88101)
    v = tm.Vocab(synth.build_vocab(vocab_tokens(), capcode=2, charset=1, norm_flag=1, with_unk=True))

    def letters(n):
        return bytes(LETTERS[int(x)] for x in rng.integers(0, len(LETTERS), size=n))

    docs = [letters(int(n)) for n in rng.integers(0, 120, size=40)] + [b"", b"a", "Hello WORLD zzé Éa".encode(), letters(1000), b"", b""]
    raw, offs = tm.pack_documents(docs)
    ids, toff, rsp, hd = v.tokenize_raw_spans_packed(raw, offs)
    norm = [v.normalize(d) for d in docs]
    nids, ntoff, nsp, _ = v.tokenize_spans_packed(*tm.pack_documents(norm))
    assert hd == 0 and np.array_equal(ids, nids) and np.array_equal(toff, ntoff) and not np.array_equal(rsp, nsp)

    def cut(a):
        return [a[int(toff[d]):int(toff[d + 1])] for d in range(len(docs))]

    n = v.n_ids()
    env = dict(torch=torch, api=torch_api, v=v, docs=docs, norm=norm, ids=cut(ids), raw_spans=cut(rsp.astype(np.int64)), spans=cut(nsp.astype(np.int64)),
               pad=n + 1, bos=n + 2, eos=n + 3, stream=torch.cuda.Stream())
    assert min(len(x) for x in env["ids"]) == 0 and max(len(x) for x in env["ids"]) >= 1000
    return env


def host(torch, t):
    """a CUDA tensor -> numpy with its bits unsigned"""
    a = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()]).cpu().numpy()
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64, 1: np.uint8}[t.element_size()])


def check(env, out, L, overlap, bos, eos, pad_left, spans=None):
    torch = env["torch"]
    got = {k: host(torch, t) for k, t in out.items()}
    e_ids, e_mask, e_lens, e_doc, e_start, e_sp = np_windows(env["ids"], L, env["pad"], bos, eos, overlap, pad_left, spans)
    assert got["input_ids"].shape == e_ids.shape and (got["input_ids"] == e_ids.astype(got["input_ids"].dtype)).all()
    assert out["attention_mask"].dtype == torch.bool and (got["attention_mask"] == e_mask).all()
    for k, e in (("lengths", e_lens), ("overflow_to_sample_mapping", e_doc), ("window_start", e_start)):
        assert out[k].dtype == torch.int32 and out[k].is_cuda and (got[k] == e).all(), k
    if spans is not None:
        assert out["offset_mapping"].dtype == torch.int64 and (got["offset_mapping"].astype(np.int64) == e_sp).all()
    else:
        assert "offset_mapping" not in out
    return e_ids.shape[0]


def case_encode_windows(env, dtype, kind, pad_left):
    """bytes and str documents; rows of 33 with both specials, overlap 7"""
    torch, api, L, overlap = env["torch"], env["api"], 33, 7
    docs = env["docs"] if kind == "bytes" else [d.decode("utf-8") for d in env["docs"]]
    with torch.cuda.stream(env["stream"]):
        out = api.encode_windows(env["v"], docs, L, overlap, pad_id=env["pad"], bos_id=env["bos"], eos_id=env["eos"], pad_left=pad_left, dtype=getattr(torch, dtype))
        assert out["input_ids"].dtype == getattr(torch, dtype) and out["input_ids"].is_cuda
        rows = check(env, out, L, overlap, env["bos"], env["eos"], pad_left)
    assert rows > len(docs) + 30


def case_offsets(env, form):
    torch, api, L, overlap = env["torch"], env["api"], 16, 14          # (room 15: every row but a document's last brings one new id)
    with torch.cuda.stream(env["stream"]):
        if form == "raw":
            out = api.encode_windows(env["v"], env["docs"], L, overlap, pad_id=env["pad"], eos_id=env["eos"], return_offsets="raw")
            check(env, out, L, overlap, None, env["eos"], False, env["raw_spans"])
        elif form == "normalized":
            out = api.encode_windows(env["v"], env["docs"], L, overlap, pad_id=env["pad"], eos_id=env["eos"], pad_left=True, return_offsets=True)
            check(env, out, L, overlap, None, env["eos"], True, env["spans"])
        else:                                        # documents passed in normalized
            out = api.encode_windows(env["v"], env["norm"], L, 0, pad_id=env["pad"], bos_id=env["bos"], raw=False, return_offsets=True)
            check(env, out, L, 0, env["bos"], None, False, env["spans"])


def case_short_documents_are_encode_batch(env):
    """overlap 0 and no document longer than a row: encode_batch of the same arguments, tensor for tensor"""
    torch, api = env["torch"], env["api"]
    docs = [d for d, x in zip(env["docs"], env["ids"]) if len(x) <= 62]
    assert len(docs) > 10 and any(len(x) == 0 for x in env["ids"])
    for pad_left in (False, True):
        kw = dict(pad_id=env["pad"], bos_id=env["bos"], eos_id=env["eos"], pad_left=pad_left, dtype=torch.int32, return_offsets="raw")
        with torch.cuda.stream(env["stream"]):
            w = api.encode_windows(env["v"], docs, 64, 0, **kw)
            e = api.encode_batch(env["v"], docs, 64, **kw)
            for k, t in e.items():
                assert torch.equal(w[k], t), k
            assert torch.equal(w["overflow_to_sample_mapping"], torch.arange(len(docs), dtype=torch.int32, device="cuda")) and not w["window_start"].any()


def case_refusals(env):
    torch, api, v = env["torch"], env["api"], env["v"]
    held = api.device_bytes(v)
    ok = dict(pad_id=env["pad"], bos_id=env["bos"], eos_id=env["eos"])
    for args, kw in (((8, 0), dict(ok, dtype=torch.float16)),
                     ((2, 0), ok),                                   # no room beside the specials
                     ((1, 0), dict(pad_id=0, bos_id=1)),
                     ((0, 0), dict(pad_id=0)),
                     ((8, 6), ok),                                   # overlap == room
                     ((8, 7), dict(pad_id=0, bos_id=1)),
                     ((8, -1), ok),
                     ((8, 2), dict(ok, raw=False, return_offsets="raw")),
                     ((8, 2), dict(ok, return_offsets="normalized"))):
        try:
            api.encode_windows(v, [b"abc"], *args, **kw)
        except ValueError:
            continue
        raise AssertionError("accepted %r %r" % (args, kw))
    assert api.device_bytes(v) == held                               # every check ran before any device call


CASES = {}
for _dtype, _kind, _left in (("int64", "bytes", False), ("int32", "str", True), ("uint16", "bytes", True), ("int16", "str", False)):
    CASES["encode_windows[%s-%s-%s]" % (_dtype, _kind, "left" if _left else "right")] = (case_encode_windows, (_dtype, _kind, _left))
for _form in ("raw", "normalized", "normalized_input"):
    CASES["offset_mapping[%s]" % _form] = (case_offsets, (_form,))
CASES["short_documents_are_encode_batch"] = (case_short_documents_are_encode_batch, ())
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
        global np_windows
        from test_gpu_windows import np_windows
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
    out = str(tmp_path_factory.mktemp("windows_torch") / "results.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and os.path.exists(out), r.stdout.decode(errors="replace")[-4000:]
    res = json.load(open(out))
    if "__skip__" in res:
        pytest.skip(res["__skip__"])
    assert "__env__" not in res, res["__env__"]
    return res


@pytest.mark.parametrize("case", sorted(CASES))
def test_encode_windows(results, case):
    assert results.get(case) == "ok", results.get(case)


if __name__ == "__main__":
    child_main(sys.argv[1])
