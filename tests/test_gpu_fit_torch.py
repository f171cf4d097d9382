"""-m gpu: torch_api.pack_batch(..., whole=True) on CUDA tensors against tests/test_gpu_fit.py's np_fit over Vocab's own ragged ids, and whole=False
against the stream cut into rows, as before.  As in tests/test_gpu_torch_api.py the work runs in a child process that imports torch first: this file as a script."""
import os
import subprocess
import sys

import numpy as np
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
    from test_gpu_fit import np_fit, PAD, EOS
    v = tm.Vocab(synth.build_vocab(sorted(bytes([c]) for c in b"abcdefgh"), capcode=0, charset=1, norm_flag=0, with_unk=True))
    L, docs = 8, [b"abc", b"", b"defgh", b"abcdefgha", b"h", b"", b"", b"gfedcbagfedcbagfe", b"ab", b"abcdefg", b"abcdefgh", b"c"]
    ids, toff = v.tokenize_packed(*tm.pack_documents(docs))[:2]
    ragged = [ids[int(toff[d]):int(toff[d + 1])] for d in range(len(docs))]
    for eos in (EOS, None):
        out = torch_api.pack_batch(v, docs, L, eos_id=eos, pad_id=PAD, dtype=torch.int32, whole=True)
        for k, exp in zip(("input_ids", "doc_index", "position", "lengths", "row_doc", "row_start"), np_fit(ragged, L, eos)):
            assert out[k].is_cuda and out[k].dtype == torch.int32 and (out[k].cpu().numpy().view(np.uint32) == exp.reshape(out[k].shape)).all(), (eos, k)
        # whole=False: the stream cut wherever it crosses a row end
        stream = np.array([x for doc in ragged for x in list(doc) + ([] if eos is None else [eos])], dtype=np.int64)
        old = torch_api.pack_batch(v, docs, L, eos_id=eos, pad_id=PAD)
        flat = old["input_ids"].cpu().numpy().reshape(-1)
        assert sorted(old) == ["doc_index", "input_ids", "position"] and flat.size == -(-stream.size // L) * L and (flat[:stream.size] == stream).all() and (flat[stream.size:] == PAD).all()
    print("OK")


def test_pack_batch_whole():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    if "SKIP" in out:
        pytest.skip(out.strip())
    assert r.returncode == 0 and out.strip().endswith("OK"), out[-4000:]


if __name__ == "__main__":
    child_main()
