"""-m gpu: tokenmonster_amd.torch_api - encode_batch / pack_batch / decode_batch on CUDA tensors, on a torch stream of the caller's, against
numpy collation (the rules as tests/test_gpu_collate.py states them) of Vocab.tokenize.  Needs a real device and torch: not part of the
emulated leg.

torch brings a HIP runtime of its own, and a process can drive the device through ONE: whichever of torch and libtokenmonster_hip.so is
loaded first brings the runtime both then share, and only torch's serves both.  The pytest process has loaded the library long before this
module is imported (conftest builds and imports the package), so the cases run in ONE child process that imports torch first - this file
as a script - and every test below asserts on what the child recorded for its case."""
import contextlib
import json
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def raises_value_error():
    try:
        yield
    except ValueError:
        return
    raise AssertionError("no ValueError")


def make_env():
    import torch
    import tokenmonster_amd as tm
    from tokenmonster_amd import synth, torch_api
    from conftest import fuzz_text, fuzz_vocab_tokens
    rng = np.random.default_rng(78001)
    v = tm.Vocab(synth.build_vocab(fuzz_vocab_tokens(rng, 2, 200), capcode=2, charset=1, with_unk=True))
    docs = [fuzz_text(rng, 2, int(n)).replace(b"\x00", b"q").replace(b"\xff", b"Q") for n in list(rng.integers(0, 400, size=61)) + [0, 1, 5000]]
    ids = [np.asarray(x, dtype=np.uint32) for x in v.tokenize(docs)]
    assert min(len(x) for x in ids) == 0 and max(len(x) for x in ids) > 1000
    n = v.n_ids()
    return dict(torch=torch, api=torch_api, v=v, docs=docs, ids=ids, pad=n + 1, bos=n + 2, eos=n + 3, stream=torch.cuda.Stream())


def host(torch, t):
    """a CUDA tensor -> numpy with its bits unsigned"""
    a = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()]).cpu().numpy()
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64, 1: np.uint8}[t.element_size()])


def case_encode_batch(env, dtype, pad_left):
    torch, api, L = env["torch"], env["api"], 48
    with torch.cuda.stream(env["stream"]):
        out = api.encode_batch(env["v"], env["docs"], L, pad_id=env["pad"], bos_id=env["bos"], eos_id=env["eos"], pad_left=pad_left, keep_tail=pad_left,
                               dtype=getattr(torch, dtype))
        got = {k: host(torch, t) for k, t in out.items()}            # (.cpu() on the stream waits for it)
    flags = (PAD_LEFT | KEEP_TAIL) if pad_left else 0
    e_ids, e_mask, e_lens = np_collate(env["ids"], L, env["pad"], env["bos"], env["eos"], flags, got["input_ids"].dtype)
    assert out["input_ids"].dtype == getattr(torch, dtype) and out["input_ids"].is_cuda and out["attention_mask"].dtype == torch.bool
    assert got["input_ids"].shape == e_ids.shape and (got["input_ids"] == e_ids).all()
    assert (got["attention_mask"] == e_mask).all() and (got["lengths"] == e_lens).all()


def case_pack_batch(env, dtype):
    torch, api = env["torch"], env["api"]
    for eos in (env["eos"], None):
        n = sum(len(x) + (eos is not None) for x in env["ids"])
        L = next(k for k in (96, 97, 98, 99) if n % k)              # (a last row with padding in it)
        with torch.cuda.stream(env["stream"]):
            out = api.pack_batch(env["v"], env["docs"], L, eos_id=eos, pad_id=env["pad"], dtype=getattr(torch, dtype))
            got = {k: host(torch, t) for k, t in out.items()}
        e_ids, e_di, e_po, _ = np_pack(env["ids"], L, env["pad"], eos, got["input_ids"].dtype)
        assert got["input_ids"].shape == e_ids.shape and (got["input_ids"] == e_ids).all()
        assert (got["doc_index"] == e_di).all() and (got["position"] == e_po).all()
        assert (e_di == 0xFFFFFFFF).any() and int(out["doc_index"].min()) == -1 and int(out["doc_index"][-1, -1]) == -1      # padding reads -1 as int32


def case_decode_of_encode(env, pad_left, with_lengths):
    torch, api, L, v = env["torch"], env["api"], 40, env["v"]
    with torch.cuda.stream(env["stream"]):
        out = api.encode_batch(v, env["docs"], L, pad_id=env["pad"], bos_id=env["bos"], eos_id=env["eos"], pad_left=pad_left, dtype=torch.int32)
        texts = api.decode_batch(v, out["input_ids"], lengths=out["lengths"] if with_lengths else None, pad_id=env["pad"], bos_id=env["bos"], eos_id=env["eos"])
    exp = [v.decode(truncated(x, L, env["bos"], env["eos"], 0)) for x in env["ids"]]
    assert texts == exp and sum(len(t) for t in texts) > 1000


def case_refusals(env):
    torch, api, v = env["torch"], env["api"], env["v"]
    good = torch.zeros((4, 8), dtype=torch.int64, device="cuda")
    for bad in (good.cpu(), good[:, ::2], good.to(torch.float32), good.to(torch.uint8), good[0], np.zeros((4, 8), dtype=np.int64)):
        with raises_value_error():
            api.decode_batch(v, bad)
    if torch.cuda.device_count() > 1:
        with raises_value_error():
            api.decode_batch(v, good.to("cuda:1"))
    with raises_value_error():
        api.decode_batch(v, good, lengths=torch.zeros(4, dtype=torch.int32))          # lengths on the host
    with raises_value_error():
        api.encode_batch(v, [b"a"], 8, pad_id=0, dtype=torch.float16)
    with raises_value_error():
        api.encode_batch(v, [b"a"], 1, pad_id=0, bos_id=1, eos_id=2)
    assert api.decode_batch(v, good, pad_id=0) == [b""] * 4


def case_second_call_allocates_nothing(env):
    torch, api, v = env["torch"], env["api"], env["v"]
    first = api.encode_batch(v, env["docs"], 64, pad_id=env["pad"])
    api.pack_batch(v, env["docs"], 64, eos_id=env["eos"], pad_id=env["pad"])
    api.decode_batch(v, first["input_ids"], lengths=first["lengths"], pad_id=env["pad"])
    held = api.device_bytes(v)
    assert held > 0
    again = api.encode_batch(v, env["docs"], 64, pad_id=env["pad"])
    api.pack_batch(v, env["docs"], 64, eos_id=env["eos"], pad_id=env["pad"])
    api.decode_batch(v, again["input_ids"], lengths=again["lengths"], pad_id=env["pad"])
    assert api.device_bytes(v) == held and torch.equal(first["input_ids"], again["input_ids"])


CASES = {}
for _dtype in ("int64", "int32", "uint16"):
    for _left in (False, True):
        CASES["encode_batch[%s-%s]" % (_dtype, "left" if _left else "right")] = (case_encode_batch, (_dtype, _left))
for _dtype in ("int64", "uint16"):
    CASES["pack_batch[%s]" % _dtype] = (case_pack_batch, (_dtype,))
for _left, _lens in ((False, True), (True, False), (False, False)):
    CASES["decode_of_encode[%s-%s]" % ("left" if _left else "right", "lengths" if _lens else "nolengths")] = (case_decode_of_encode, (_left, _lens))
CASES["decode_batch_refuses"] = (case_refusals, ())
CASES["second_call_allocates_nothing"] = (case_second_call_allocates_nothing, ())


def child_main(out_path):
    import torch                                     # first: its HIP runtime is the one the library then shares
    torch.cuda.init()
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    global KEEP_TAIL, PAD_LEFT, np_collate, np_pack, truncated
    from test_gpu_collate import KEEP_TAIL, PAD_LEFT, np_collate, np_pack, truncated
    results = {}
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
    out = str(tmp_path_factory.mktemp("torch_api") / "results.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and os.path.exists(out), r.stdout.decode(errors="replace")[-4000:]
    res = json.load(open(out))
    assert "__env__" not in res, res["__env__"]
    return res


@pytest.mark.parametrize("case", sorted(CASES))
def test_torch_api(results, case):
    assert results.get(case) == "ok", results.get(case)


if __name__ == "__main__":
    child_main(sys.argv[1])
