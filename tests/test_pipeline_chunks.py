"""CPU: how tm_tokenize_pipeline cuts a batch into chunks (tokenmonster_amd/csrc/tm_chunks.h) in a stand-alone program of its own
(tools/chunks_check.cpp), built with the address and undefined-behaviour sanitizers and run here on synthetic offset arrays: the chunks tile
the documents, a chunk of several documents keeps within the limit in force for it and is a maximal run, and every layout equals the one
recorded in tests/golden/pipeline_chunks.txt - printed from the loop as it stood inside tokenize_pipeline_on, moved into the header word for
word, before anything else changed.  The GPU tests do not see chunk boundaries: this is the guard on them."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_layout_under_sanitizers(tmp_path):
    cxx = next(c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c))
    exe = str(tmp_path / "chunks_check")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tokenmonster_amd", "csrc"),
                        os.path.join(ROOT, "tools", "chunks_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "pipeline_chunks.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and b"chunks ok" in r.stdout, r.stdout.decode(errors="replace")
