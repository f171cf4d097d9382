"""-m gpu: torch_api.tokenize_resident on CUDA tensors - length_order against torch.sort(stable=True) of counts(), collate(indices) against
encode_batch of the same documents re-listed in that order, a bad index counted.  As in tests/test_gpu_torch_api.py the work runs in a child
process that imports torch first: this file as a script."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


def child_main():
    import torch                                     # first: its HIP runtime is the one the library then shares
    if not torch.cuda.is_available():
        return print("SKIP torch has no device")
    sys.path[:0] = [HERE, os.path.dirname(HERE)]
    import tokenmonster_amd as tm
    from tokenmonster_amd import synth, torch_api
    v = tm.Vocab(synth.build_vocab(sorted(bytes([c]) for c in b"abcdefgh"), capcode=0, charset=1, norm_flag=0, with_unk=True))
    docs = [b"abc", b"", b"defgh", b"abcdefgha", b"h", b"", b"abc", b"gfedcbagfedcbagfe", b"ab", b"abcdefg", b"abcdefgh", b"c"]
    kw = dict(pad_id=60001, bos_id=60002, eos_id=60003, dtype=torch.int32)
    res = torch_api.tokenize_resident(v, docs)
    counts = res.counts()
    assert res.ndocs == len(docs) and counts.is_cuda and counts.dtype == torch.int64 and counts.tolist() == [len(d) for d in docs]      # (one id per byte)
    for desc in (False, True):
        order = res.length_order(descending=desc)
        assert order.is_cuda and order.dtype == torch.int64 and torch.equal(order, torch.sort(counts, stable=True, descending=desc).indices)
    for idx, flags in (([3, 3, 0, 11], {}), (torch.tensor([7, 1, 7], dtype=torch.int32), dict(pad_left=True)), (order, dict(keep_tail=True))):
        got = res.collate(idx, 8, **kw, **flags)
        exp = torch_api.encode_batch(v, [docs[int(i)] for i in idx], 8, **kw, **flags)
        assert int(got["bad_indices"]) == 0 and all(got[k].is_cuda and got[k].dtype == exp[k].dtype and torch.equal(got[k], exp[k]) for k in exp), (idx, flags)
    got = res.collate([2, len(docs), -1, 5], 8, **kw)
    assert int(got["bad_indices"]) == 2 and got["lengths"].tolist() == [7, 0, 0, 2] and (got["input_ids"][1:3] == 60001).all() and not got["attention_mask"][1:3].any()
    assert res.collate([], 8, **kw)["input_ids"].shape == (0, 8)
    res.close()
    print("OK")


def test_tokenize_resident():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    if "SKIP" in out:
        pytest.skip(out.strip())
    assert r.returncode == 0 and out.strip().endswith("OK"), out[-4000:]


if __name__ == "__main__":
    child_main()
