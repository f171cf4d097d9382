"""-m gpu: step C of k_match_branch (the segment's exit map for its 80 entry states) on text built to stress it, bit-exact against the
oracle: chains that never merge, forward-delete states, documents that end just before or behind a segment boundary, documents of more
than 512 segments (the group resolve), byte ranges of one walk whose short last segment is followed by more text (entered in plain and in
forward-delete states), the wide form of the map (test hook 5) and the UTF-16 self-successor state.  test_exit_maps_on_the_emulated_device runs the same file on the emulated device (tools/emu), without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import synth
from conftest import fuzz_text, fuzz_vocab_tokens
from oracle_bind import Oracle, oracle_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
# lengths within 40 bytes of a segment boundary (the look-ahead of an entry state), either side
NEAR = [n for k in (1, 2, 3) for n in (256 * k - 40, 256 * k - 39, 256 * k - 17, 256 * k - 1, 256 * k, 256 * k + 1, 256 * k + 39, 256 * k + 40)]


def check_docs(vocab, orc, docs, what):
    text, offs = tm.pack_documents(docs)
    ids, toff, missing = vocab.tokenize_packed(text, offs)
    assert toff[0] == 0 and toff[-1] == ids.size
    for d, doc in enumerate(docs):
        exp, miss = orc.tokenize(doc)
        got = ids[int(toff[d]):int(toff[d + 1])]
        assert got.size == exp.size and (got == exp).all(), "%s doc %d (len %d): ids differ" % (what, d, len(doc))
        assert int(missing[d]) == miss, "%s doc %d: missing %d != %d" % (what, d, int(missing[d]), miss)


@pytest.mark.gpu
def test_digit_runs_and_base64_chains_that_never_merge():
    rng = np.random.default_rng(8101)
    toks = [bytes([c]) for c in B64] + [bytes(rng.choice(list(B64), size=int(rng.integers(2, 7))).tolist()) for _ in range(300)]
    toks += [b"%d" % n for n in range(0, 1000, 7)] + [b" ", b"=", b"\n"]
    img = synth.build_vocab(list(dict.fromkeys(toks)), capcode=0, charset=1, with_unk=True)
    v, orc = tm.Vocab(img), Oracle(img)
    docs = []
    for n in NEAR + [700, 1500]:
        docs.append(bytes(rng.choice(list(b"0123456789"), size=n).tolist()))
        docs.append(bytes(rng.choice(list(B64), size=n).tolist()))
        docs.append(bytes(rng.choice(list(B64), size=n).tolist()) + b"==")
    check_docs(v, orc, docs, "digits / base64")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_text_dense_in_forward_delete_states(seed):
    rng = np.random.default_rng(8200 + seed)
    toks = fuzz_vocab_tokens(rng, 2, 160)
    toks = list(dict.fromkeys(toks + [b"D " + bytes([c]) for c in b"abcde"] + [b" " + bytes([c]) for c in b"abcde"] + [b"D", b" "]))
    img = synth.build_vocab(toks, capcode=2, charset=1, with_unk=True)
    v, orc = tm.Vocab(img), Oracle(img)
    markers = [b"D a", b"D b", b"Da", b"D ab", b"C a", b"W b", b" a", b"a", b"D", b" "]
    docs = []
    for n in NEAR + [1000, 3000]:
        docs.append(b"".join(bytes(rng.choice(markers)) for _ in range(n))[:n])
        docs.append(fuzz_text(rng, 2, n)[:n])
    oracle_stats(reset=True)
    check_docs(v, orc, docs, "forward-delete dense")
    st = oracle_stats()
    assert st["s1b"] + st["s2b"] + st["s3b"] > 0, st          # the walks took forward-delete branches: (p,1) states were entered


@pytest.mark.gpu
def test_documents_of_more_than_512_segments():
    rng = np.random.default_rng(8301)
    img = synth.build_vocab(fuzz_vocab_tokens(rng, 2, 200), capcode=2, charset=1, with_unk=True)
    v, orc = tm.Vocab(img), Oracle(img)
    docs = [fuzz_text(rng, 2, 513 * 256 + 17)[:513 * 256 + 17], fuzz_text(rng, 2, 300)[:300], fuzz_text(rng, 2, 600 * 256)[:600 * 256 - 3]]
    check_docs(v, orc, docs, "group resolve")


@pytest.mark.gpu
def test_byte_ranges_whose_last_segment_is_followed_by_more_text():
    """tm_score_begin / tm_score_finish over byte ranges of one walk (tokenmonster_amd/dist.py): a range whose length is no multiple of the
    segment size ends in a short segment behind which its halo goes on - the exit map passes a token of the range through it."""
    import ctypes as C
    from tokenmonster_amd import _native as N
    from tokenmonster_amd import dist as tmdist
    rng = np.random.default_rng(8401)
    img = synth.build_vocab(fuzz_vocab_tokens(rng, 2, 150), capcode=2, charset=1)
    data = np.frombuffer(fuzz_text(rng, 2, 40_000)[:40_000], dtype=np.uint8)
    cuts = [0, 100, 300, 557, 5_250, 9_999, 23_456, 40_000]        # ranges of 257, 4 693, ... bytes: short last segments
    v, orc = tm.Vocab(img), Oracle(img)
    exp_s, exp_t, exp_m = orc.score(data)
    all_exits, hists, handles, checked = [], [], [], set()
    try:
        for a, b in zip(cuts, cuts[1:]):
            own = np.ascontiguousarray(data[a:min(b + tmdist.HALO, data.size)])
            ds = C.c_void_p()
            N.check(N.lib.tm_dataset_upload(N.ptr(own), own.size, C.byref(ds)))
            handles.append(ds)
            eng = tmdist.HipRange(v, ds, b - a, continues=b < data.size, text_ends_in_halo=data.size - b < tmdist.HALO)
            ex = eng.begin()
            for e in (0, 1, 2, 3, 4, 5, 20, 21, 40, 41, 78, 79):          # (odd: entered in a forward-delete state)
                if ex[e] != tmdist.UNREACHABLE and e // 2 < b - a:
                    assert int(ex[e]) == orc.score_range(data, a, b, e)[3], (a, b, e)
                    checked.add(e & 1)
            all_exits.append(ex)
            eng.finish(tmdist.resolve_entry(all_exits, len(all_exits) - 1))
            s_ = np.zeros(v.n_ids(), dtype=np.uint32)
            t_ = C.c_uint64()
            m_ = np.zeros(32, dtype=np.uint8)
            N.check(N.lib.tm_score_read(v.handle, ds, N.ptr(s_), C.byref(t_), N.ptr(m_)))
            hists.append((s_, t_.value, m_))
    finally:
        for ds in handles:
            N.lib.tm_dataset_free(ds)
    assert checked == {0, 1}, checked
    got_s = sum(h[0].astype(np.uint64) for h in hists)
    assert (got_s == exp_s).all() and sum(h[1] for h in hists) == exp_t
    assert (np.bitwise_or.reduce(np.stack([h[2] for h in hists])) == exp_m).all()


def _utf16(bs):
    return b"".join(bytes([c, 0]) for c in bs)


@pytest.mark.gpu
def test_utf16_self_successor_is_a_dead_end():
    """A (p,1) state that is its own successor (UTF-16 vocabulary with one-byte keys beside the delete token, text cut in half a
    character: the reference does not terminate on it) has no exit: the call reports TM_E_INPUT instead of looping, and the same text
    in whole characters tokenizes.  Every cut document is tried on its own; at least one of them must meet the dead end."""
    from tokenmonster_amd import _native as N
    rng = np.random.default_rng(913)
    toks8 = fuzz_vocab_tokens(rng, 2, 100)
    toks = sorted(set(_utf16(t) for t in toks8 if len(t) <= 20) | {b"D", b" ", b"a"})
    img = synth.build_vocab(toks, capcode=2, charset=2)
    v = tm.Vocab(img)
    dead = 0
    for n in (300, 700, 1100, 1487, 1500, 1800):
        whole = _utf16(fuzz_text(rng, 2, n)[:n])
        try:
            v.tokenize_packed(*tm.pack_documents([whole[:-1]]))
        except N.TokenMonsterHipError as e:
            assert e.code == N.TM_E_INPUT
            dead += 1
        ids, toff, _ = v.tokenize_packed(*tm.pack_documents([whole, whole[:-2]]))
        assert ids.size > 0 and (np.diff(toff.astype(np.int64)) > 0).all()
    assert dead > 0


@pytest.mark.gpu
def test_wide_exit_map_for_every_segment():
    """The wide exit map (a count of 511 in the 16-bit entry, the whole entry in the 32-bit array) is what a segment with more than 510
    ids from one entry state gets.  No UTF-8 text built for these tests reaches that (DESIGN, step C), so test hook 5 sends every
    segment's map that way: tokenize, the group resolve of long documents and the exit maps of byte ranges must stay exact."""
    from tokenmonster_amd import _native as N
    old = N.lib.tm_debug_flags(32)
    try:
        assert N.lib.tm_debug_flags(-1) == 32, "test hooks not armed"
        test_text_dense_in_forward_delete_states(1)
        test_documents_of_more_than_512_segments()
        test_byte_ranges_whose_last_segment_is_followed_by_more_text()
    finally:
        N.lib.tm_debug_flags(old)


def test_exit_maps_on_the_emulated_device():
    """the -m gpu tests above on the emulated device (tools/emu: the kernel sources compiled for the host, tests/conftest.py TM_EMU=1)"""
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_exit_maps.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert " passed" in out and " failed" not in out, out[-2000:]
