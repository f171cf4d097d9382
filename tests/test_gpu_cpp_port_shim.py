"""-m gpu: the reference C++ port's OWN programs on the HIP library.  examples/cpp_port_shim re-declares the port's public header
(tokenmonster-cpp/include/tokenmonster/tokenmonster.hpp:52-115) over the C ABI; tokenmonster-cpp/tests/unit.cpp (the reference's only
known-answer test, :87-119) and tests/bench.cpp (its micro-benchmark) are compiled UNMODIFIED from /root/reference against it
(examples/cpp_port_shim/Makefile; the binaries travel to the GPU box prebuilt, like oracle/_ref).  unit must exit 0 with its asserts
compiled in; bench's token count, decoded bytes and checksums must equal what the reference runtime's own build of the same program
prints for the same vocabulary (oracle/_ref/bench)."""
import os
import subprocess

import pytest

from conftest import example_env
from tokenmonster_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "examples", "cpp_port_shim")
UNIT = os.path.join(ROOT, "oracle", "_ref", "cpp_port_shim", "unit")
BENCH = os.path.join(ROOT, "oracle", "_ref", "cpp_port_shim", "bench")
REF_BENCH = os.path.join(ROOT, "oracle", "_ref", "bench")


def _build():
    r = subprocess.run(["make", "-C", SHIM], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    if not os.path.exists(UNIT):
        pytest.skip("oracle/_ref/cpp_port_shim is not there (built where the reference sources are present)")


def test_the_ports_unit_test_passes_on_the_hip_library(tmp_path):
    _build()
    r = subprocess.run([UNIT], env=dict(example_env(), TMPDIR=str(tmp_path)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]


def _facts(out):
    rows = [l.split("\t") for l in out.splitlines()]
    head = {r[0]: r[1] for r in rows if len(r) == 2}
    bench = {r[0]: r for r in rows if len(r) == 6 and r[0] != "bench"}
    return head, bench


@pytest.mark.parametrize("shape", ["englishcode", "code-nocapcode"])
def test_the_ports_bench_prints_the_reference_runtimes_numbers(tmp_path, shape):
    _build()
    if shape == "englishcode":
        img = synth.synth_vocab(synth.ENGLISHCODE, 8000, capcode=2, norm_flag=1, level=3, seed=0x42454E43)
    else:
        img = synth.synth_vocab(synth.CODE, 4096, capcode=0, norm_flag=0, level=1, seed=0x42454E44)
    path = tmp_path / "v.vocab"
    path.write_bytes(img)
    nbytes = "200000"
    mine = subprocess.run([BENCH, str(path), "0.2", nbytes], env=example_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert mine.returncode == 0, mine.stderr.decode(errors="replace")[-2000:]
    head, bench = _facts(mine.stdout.decode())
    assert set(bench) == {"normalize", "tokenize_normalized", "encode_tokenize", "decode_tokens"} and int(head["tokens"]) > 0
    if not os.path.exists(REF_BENCH):
        pytest.skip("oracle/_ref/bench is not there")
    ref = subprocess.run([REF_BENCH, str(path), "0.2", nbytes], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert ref.returncode == 0, ref.stderr.decode(errors="replace")[-2000:]
    rhead, rbench = _facts(ref.stdout.decode())
    for k in ("vocab_size", "corpus_bytes", "corpus_fnv1a", "tokens", "missing", "decoded_bytes", "decoded_fnv1a"):
        assert head[k] == rhead[k], (k, head[k], rhead[k])
    # the checksum column is (5 warm-up + the timed iterations) x one call's checksum, summed modulo 2^64: cross-multiplied, the two programs' columns agree
    M = 1 << 64
    for name in bench:
        n_mine, n_ref = int(bench[name][1]) + 5, int(rbench[name][1]) + 5
        assert (int(bench[name][5]) * n_ref) % M == (int(rbench[name][5]) * n_mine) % M, (name, bench[name], rbench[name])
