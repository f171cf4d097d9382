#!/usr/bin/env python3
"""bench.py — throughput of the HIP ungreedy-tokenization path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`)

Workload (BASELINE.json configs[1]): englishcode-32000-consistent vocabulary shape, 1 GiB of synthetic mixed
prose/code/log documents per GPU (weak scaling: every rank tokenizes its own shard, no data-path collective).
A "step" is ONE pass of the whole device pipeline over the resident batch: normalize (NFD + capcode on the GPU,
tm_batch_normalize; documents with other non-ASCII content go through the host normalizer inside that call), then
segments, match_branch(+link), resolve, scan, emit.  The timed region starts with the RAW UTF-8 documents in HBM and
ends with dense uint32 ids + offsets in HBM.  `value` = raw UTF-8 bytes of all ranks x K / max-over-ranks wall time.
(--hot-path-only times the tokenize kernels alone on host-normalized input, as rounds before the GPU normalizer did.)

A plain run sets up, warms up, times the K steps and prints the line.  --full adds everything beside the headline: the
checks against the oracle and the reference runtime, per-kernel times and rooflines (with their rocprofv3 counter passes),
the CPU baselines, the host-to-host pipeline and the tables laid out by use.  --dump-outputs DIR writes what the last timed
step computed as DIR/<name>.npy (see dump_outputs).

Prints ONE JSON line on rank 0 (see README / DESIGN.md for the roofline and cpu_baseline objects).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

# The HIP runtime spreads a process's streams over GPU_MAX_HW_QUEUES hardware queues (4 by default); the host-to-host ring wants its four streams
# on queues of their own (tm_host.hip: 27 ms per GiB with eight queues, 35 with four).  The library asks for eight when it is loaded - but this
# process initializes the runtime through torch BEFORE the library is loaded, so the variable is set here, as a server's environment would set it.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec, /opt/skills/guides/MI355X_MICROARCH.md
# vector-instruction issue: 256 CUs x 4 SIMD-32 x 2.4 GHz, a wave64 instruction issues over 2 cycles (same guide, "Wave scheduling")
VALU_PEAK_GINSTS = 256 * 4 * 2.4 / 2.0
H2H_WARM = 6                       # warm-up passes of the host-to-host measurement (see host_to_host)
L2_PEAK_GREQS = 128 * 2.1          # 128 L2 channels, one request each per clock (MI355X_MICROARCH.md: 34.5 TB/s = 128 channels x 128 B x 2.1 GHz)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mbytes", type=int, default=1024, help="MiB of raw text per GPU (default 1024 = BASELINE configs[1])")
    ap.add_argument("--config", default=None, help="vocabulary shape (default: englishcode-32000-consistent; score: candidates-65536)")
    ap.add_argument("--tune-mib", type=float, default=0.0, help="tm_vocab_tune the vocabulary on this many MiB of OTHER synthetic text of the same kind before anything is "
                                                                "timed (off by default: the lines of record are untuned); recorded in config.tables_tuned_on")
    ap.add_argument("--workload", default="tokenize", choices=["tokenize", "score", "decode"],
                    help="tokenize = BASELINE configs[1] (default); score = trainvocab candidate-scoring pass, configs[4]; decode = Decode of the ids of "
                         "the same corpus, device-resident (SURVEY 8(f) #2: ids in HBM -> text in HBM)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--hot-path-only", action="store_true", help="input = host-normalized bytes; time only the tokenize pipeline")
    ap.add_argument("--cpu-sample-mb", type=float, default=64.0)
    ap.add_argument("--verify", type=int, default=-1, help="documents re-checked after timing (rank 0): -1 = ALL of them against the reference runtime on every host core "
                                                           "(a bounded sample where the host has few cores), n > 0 = a random sample of n against the oracle, 0 = none")
    ap.add_argument("--also-flags", default="", help="development aid: comma separated tm_debug_flags values; the same step is timed again under each "
                                                      "(kernel variants) and reported on stderr, its ids compared with the default's")
    ap.add_argument("--no-host-to-host", action="store_true", help="skip the host-to-host pipeline and small-batch latency figures")
    ap.add_argument("--no-tuned-leg", action="store_true", help="skip the figure beside the line of record: the same step with the tables laid out by use "
                                                                "(tm_vocab_load_sample on 16 MiB of OTHER synthetic text)")
    ap.add_argument("--h2h-lanes", type=int, default=4, help="lanes of the host-to-host pipeline (ONE stated setting, timed over --steps)")
    ap.add_argument("--h2h-chunk-mib", type=int, default=0, help="chunk size of the host-to-host pipeline in MiB (0: the library's default - 48 on the ring, 32 with lanes)")
    ap.add_argument("--h2h-sweep", action="store_true", help="development aid: also time other (lanes, chunk) settings, reported on stderr only")
    ap.add_argument("--in-process", action="store_true",
                    help="N GPUs from ONE process through the library's own multi-device driver (tm_devices / tm_vocab_load_all / tm_score_multi, RCCL inside "
                         "the library; include/tokenmonster_hip.h) - the path a Go host uses - instead of one torch.distributed rank per GPU")
    ap.add_argument("--no-measure-traffic", dest="measure_traffic", action="store_false",
                    help="do not measure roofline.traffic / roofline_valu in this run (default: three rocprofv3 --pmc passes - instruction counts, FETCH_SIZE, "
                         "WRITE_SIZE - over tools/k1_time.py in a child process, about a minute; without them the figures of profiles/traffic_latest.json are "
                         "reported and labelled as static)")
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beside the headline figure (verification, per-kernel times and rooflines, counter passes, CPU "
                         "baselines, host-to-host pipeline, tables laid out by use); off: set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rank 0's shard, device 0's with --in-process) as DIR/<name>.npy, "
                         "float32 / float64, at most 64 MB")
    return ap.parse_args()


def config_image(synth, name):
    """the .vocab image of a named shape: from the cache beside the package, or made again (it is deterministic in its seed) where the
    checkout is read-only and the cache cannot be written"""
    try:
        return synth.config_vocab(name)
    except OSError:
        return synth.config_vocab(name, cache=False)


DUMP_LIMIT = 64 << 20
DUMP_SEED = 0x44554D50
DUMP_SAMPLE_DOCS = 8192


def dump_outputs(dirname, arrays, log):
    """--dump-outputs: every array as DIR/<name>.npy; the inputs are seeded, so two builds compare output for output"""
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT:
        raise SystemExit("bench.py: --dump-outputs would write %d bytes, more than %d" % (total, DUMP_LIMIT))
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(dirname, name + ".npy"), a)
    log("outputs of the last timed step: %s in %s (%.1f MB)" % (", ".join(sorted(arrays)), dirname, total / 1e6))


def score_outputs(res):
    """a scoring pass's histogram (scores u32[n_ids], tokens_in_text, missing_set u8[32]) as --dump-outputs writes it"""
    scores, tokens, missing = res
    return {"scores": np.asarray(scores).astype(np.float64), "tokens_in_text": np.array([tokens], dtype=np.float64),
            "missing_set": np.asarray(missing).astype(np.float64)}


def stream_outputs(prefix, data, offs, per_doc=None):
    """a batch's packed output (token ids, or decoded bytes, with the offsets of its documents) as --dump-outputs writes it: every
    document's offset (and `per_doc` value), the sums of the values over 65536 equal slices of the whole stream, and the values
    themselves of a fixed, seeded sample of documents.  Past 1M documents the per-document arrays hold the sample's documents only."""
    nd = offs.size - 1
    offs = offs[: nd + 1].astype(np.int64)
    pick = np.sort(np.random.default_rng(DUMP_SEED).choice(nd, size=min(nd, DUMP_SAMPLE_DOCS), replace=False))
    n = int(offs[-1])
    cut = np.unique(np.linspace(0, n, 65537).astype(np.int64))[:-1]
    out = {prefix + "_sample_docs": pick.astype(np.float64),
           prefix + "_sample": np.concatenate([data[offs[d]:offs[d + 1]] for d in pick] + [data[:0]])[: 6 << 20].astype(np.float32),
           prefix + "_slice_sums": (np.add.reduceat(data[:n], cut, dtype=np.uint64) if n else np.zeros(0)).astype(np.float64)}
    docs = slice(None) if nd <= (1 << 20) else pick
    out[prefix + "_offsets"] = np.stack([offs[:-1][docs], offs[1:][docs]]).astype(np.float64)
    if per_doc is not None:
        out[prefix + "_" + per_doc[0]] = np.asarray(per_doc[1][:nd])[docs].astype(np.float64)
    return out


def cpu_baseline(img, text, offs, sample_mb, log, raw_mode=False, check=None):
    """the reference's own C++ runtime (oracle/_ref, kind 'reference') — or our C port when it is absent — timed
    single-threaded on a bounded sample of the SAME normalized documents, the way benchmark/tokenmonster_bench.go
    :41-55 times Go: wall clock around tokenize calls."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_bind as ob
    kind = "reference" if ob.have_ref() else "port"
    eng = ob.Reference(img) if kind == "reference" else ob.Oracle(img)
    # raw_mode: `text` is RAW UTF-8 and the reference's full Tokenize (normalize + capcode + walk) is timed
    fn = (eng.tokenize if raw_mode else eng.tokenize_normalized) if kind == "reference" else eng.tokenize
    budget = int(sample_mb * (1 << 20)) if kind == "reference" else int(sample_mb * (1 << 20) / 8)
    nd = offs.size - 1
    done = 0
    d = 0
    t0 = time.perf_counter()
    ntok = 0
    while d < nd and done < budget and time.perf_counter() - t0 < 40.0:
        a, b = int(offs[d]), int(offs[d + 1])
        ids, _ = fn(text[a:b])
        ntok += ids.size
        done += b - a
        d += 1
    dt = time.perf_counter() - t0
    res = {"value": round(done / dt / 1e9, 6), "unit": "GB/s", "cores": 1, "kind": kind,
           "sample": "first %d documents (%.1f MB %s) of the same corpus, 1 thread, %.1f s" % (
               d, done / 1e6, "raw, Tokenize = normalize + capcode + walk" if raw_mode else "normalized, tokenize_normalized", dt),
           "host_cores": os.cpu_count()}
    if kind == "reference":
        # all host cores, one document per call like the server's goroutines (training/tokenmonsterserver.go:363-378); the sample
        # grows with the core count so that every thread has about a second of work
        ncores = os.cpu_count() or 1
        want = min(int(offs[nd]), int(16e6 * ncores))
        d2 = int(np.searchsorted(offs, want, side="right")) - 1
        d2 = max(1, min(nd, d2))
        t0 = time.perf_counter()
        if check is None:
            eng.tokenize_docs_mt(text[: int(offs[d2])], offs[: d2 + 1], raw_mode, ncores)
        else:
            # the same fan-out as the CHECKER of the device's ids: every document's id stream and `missing` compared (memcmp) with what the
            # reference produced for it; the comparison is negligible beside the tokenization it rides on
            ids, toff, miss = check
            bad, first_bad, _ = eng.verify_docs_mt(text[: int(offs[d2])], offs[: d2 + 1], raw_mode, ncores, ids, toff[: d2 + 1], miss)
            if bad:
                raise SystemExit("bench.py: HIP ids differ from the reference runtime's in %d of %d documents (first: document %d) - number is INVALID" % (bad, d2, first_bad))
            res["verified_docs_vs_reference"] = d2
        dt2 = time.perf_counter() - t0
        res["all_cores"] = {"value": round(int(offs[d2]) / dt2 / 1e9, 6), "unit": "GB/s", "cores": ncores,
                            "sample": "first %d documents (%.1f MB) of the same corpus, %d threads, %.1f s%s" % (
                                d2, int(offs[d2]) / 1e6, ncores, dt2, "" if check is None else "; every document's ids compared with the device's")}
        # fewer threads than hardware threads: the reference runtime's per-call vectors and its 25 MB index per vocabulary make it scale badly past
        # the physical cores of a socket (round 4: 256 threads = 11 x one thread) - the peak and where it lies, so that "all cores" is not read as
        # the best this host can do
        sweep = {}
        for th in sorted({t for t in (ncores // 8, ncores // 4, ncores // 2) if t >= 2}):
            dq = max(1, min(nd, int(np.searchsorted(offs, min(int(offs[nd]), int(6e6 * th)), side="right")) - 1))
            tq = time.perf_counter()
            eng.tokenize_docs_mt(text[: int(offs[dq])], offs[: dq + 1], raw_mode, th)
            sweep[str(th)] = round(int(offs[dq]) / (time.perf_counter() - tq) / 1e9, 6)
        sweep[str(ncores)] = res["all_cores"]["value"]
        best = max(sweep, key=lambda k: sweep[k])
        res["thread_sweep_GBps"] = sweep
        res["peak"] = {"value": sweep[best], "unit": "GB/s", "threads": int(best)}
        # the reference's own micro-benchmark on its own 1 MiB micro-corpus (tokenmonster-cpp/tests/bench.cpp:39-55), 1 thread
        if os.path.exists(ob.REF_BENCH):
            import subprocess
            import tempfile
            with tempfile.NamedTemporaryFile(suffix=".vocab", delete=False) as f:
                f.write(bytes(img))
            try:
                r = subprocess.run([ob.REF_BENCH, f.name, "1.0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
                rows = {ln.split("\t")[0]: ln.split("\t") for ln in r.stdout.decode(errors="replace").splitlines() if "\t" in ln}
                res["reference_micro_corpus"] = {k: {"MB_per_s": float(rows[k][4])} for k in ("normalize", "tokenize_normalized", "encode_tokenize", "decode_tokens")
                                                 if k in rows and len(rows[k]) > 4}
                res["reference_micro_corpus"]["note"] = "tokenmonster-cpp/tests/bench.cpp run as is: 1 MiB micro-corpus, 1 thread, this vocabulary"
            except Exception as ex:     # noqa: BLE001
                res["reference_micro_corpus"] = {"error": str(ex)}
            finally:
                os.unlink(f.name)
    log("cpu_baseline: %s" % res)
    return res


def host_to_host(vocab, raw, roffs, text, offs, ids_expected, log, tm, steps=3, lanes=4, chunk=32 << 20, sweep=False):
    """RAW UTF-8 in (pinned) host memory -> 2-byte serialized ids in (pinned) host memory, through tm_tokenize_pipeline:
    chunks run H2D | normalize + tokenize + serialize | D2H on several lanes.  This is SURVEY 8(d)'s 'first H2D to last D2H'
    figure; `value` stays the HBM-resident rate.  Also the latency of a small batch (64 documents of 2 KiB, already normalized)
    through tm_tokenize_batch on a warm lane: the job-1 case of the server."""
    import ctypes as C
    from tokenmonster_amd import _native as N
    pin_in = tm.PinnedBuffer(raw.size)
    pin_in.array[:] = raw
    pin_out = tm.PinnedBuffer(4 * ids_expected + 4096)
    res = {}

    def pages_on_nodes(arr):
        """where the pages of a buffer lie: {node: pages of the mapping it is part of} from /proc/self/maps + numa_maps (None if the kernel does not say)"""
        try:
            addr, start = arr.ctypes.data, None
            for line in open("/proc/self/maps"):
                a, b = line.split()[0].split("-")
                if int(a, 16) <= addr < int(b, 16):
                    start = a
                    break
            for line in open("/proc/self/numa_maps"):
                f = line.split()
                if f and f[0] == start:
                    return {x.split("=")[0]: int(x.split("=")[1]) for x in f[1:] if x[0] == "N" and x[1:].split("=")[0].isdigit()} or None
        except Exception:      # noqa: BLE001
            pass
        return None
    # NUMA: the node of the GPU's PCIe root, where the page-locked buffers ended up (hipHostMalloc: the node nearest to the device), and the
    # library's workers run on that node's CPUs for the length of a call (tm_host.hip: NearDevice; TM_NUMA=0 switches it off)
    res["numa"] = {"gpu_node": int(N.lib.tm_device_numa_node(0)), "pinned_input_pages": pages_on_nodes(pin_in.array), "pinned_output_pages": pages_on_nodes(pin_out.array),
                   "worker_threads": "bound to the GPU's node by the library" if os.environ.get("TM_NUMA", "1") != "0" else "left where the scheduler puts them (TM_NUMA=0)"}
    # what the host link of THIS box gives a plain copy of the same page-locked buffers (the ring cannot be faster than its upload: boxes differ)
    try:
        import torch
        dev_buf = torch.empty(int(raw.size), dtype=torch.uint8, device="cuda")
        link = {}
        for name, dst_p, src_p in (("h2d", dev_buf.data_ptr(), pin_in.array.ctypes.data), ("d2h", pin_in.array.ctypes.data, dev_buf.data_ptr())):
            best = None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                N.check(N.lib.tm_device_copy(C.c_void_p(dst_p), C.c_void_p(src_p), int(raw.size)))
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None or dt < best else best
            link[name + "_GBps"] = round(raw.size / best / 1e9, 2)
        link["note"] = "hipMemcpy of the %d MiB page-locked input buffer, best of 3: the floor of a host-to-host pass on this box is raw bytes / h2d" % (raw.size >> 20)
        res["link"] = link
        pin_in.array[:] = raw
        del dev_buf
    except Exception as ex:      # noqa: BLE001
        log("link probe failed (%s)" % ex)
    for label, src, dst in (("pinned", pin_in.array, pin_out.array), ("pageable", raw, np.empty(4 * ids_expected + 4096, dtype=np.uint8))):
        # ONE stated setting, `steps` passes after H2H_WARM warm-up passes (benchmark/tokenmonster_bench.go:41-55 times around the whole call).
        # Several, not one: in a fresh process the first five or so calls with four lanes' commands in flight take ~40 ms instead of ~32, each
        # with one ~8.6 ms stall below this library while no buffer of ours grows (profiles/r04_h2h_lanes.txt, (c)); a server is past that after
        # its first second, and what is quoted here is its steady state.  Every pass is listed in `ms_each`.
        settings = [(lanes, chunk)] + ([(6, 32 << 20), (6, 16 << 20), (8, 16 << 20), (4, 64 << 20), (3, 64 << 20), (4, 32 << 20)] if sweep else [])
        for k, (ln, ch) in enumerate(settings):
            for _ in range(H2H_WARM if (k == 0 and label == "pinned") else 1):
                vocab.tokenize_pipeline(src, roffs, raw=True, chunk_bytes=ch, lanes=ln, out=dst)      # warm the lanes
            each = []
            for _ in range(steps):
                t0 = time.perf_counter()
                blob, boff, _, enc, st = vocab.tokenize_pipeline(src, roffs, raw=True, chunk_bytes=ch, lanes=ln, out=dst)
                each.append(time.perf_counter() - t0)
            # (the MEDIAN pass: on the shared boxes this runs on, a call now and then starts 1.5 - 10 ms late - before its first chunk, gpurun_out/r06_probe25 -;
            # every pass is listed in ms_each and the mean beside it)
            dt = float(np.median(each))
            ntok = int(boff[-1]) // enc
            if k == 0:
                res[label] = {"value": round(raw.size / dt / 1e9, 4), "unit": "GB/s raw UTF-8, host to host", "ms": round(dt * 1e3, 3), "ms_is": "median of the passes",
                              "ms_mean": round(sum(each) / steps * 1e3, 3), "lanes": ln,
                              "chunk_MiB": (ch >> 20) or ("library default (48 ring / 32 lanes)"), "id_bytes": enc, "tokens": ntok, "steps": steps, "warmup_passes": H2H_WARM if label == "pinned" else 1,
                              "form": "ring (no host round trip inside a chunk)" if st.get("ring") else "lanes", "chunks": st["chunks"], "ring_exact_chunks": st.get("ring_exact_chunks", 0),
                              "ms_each": [round(x * 1e3, 2) for x in each]}
                if label == "pinned":
                    res["_ids"] = (blob.copy(), boff.copy(), enc)
            else:
                log("host_to_host sweep (%s): %d lanes x %d MiB: %.3f ms = %.2f GB/s" % (label, ln, ch >> 20, dt * 1e3, raw.size / dt / 1e9))
            if ntok != ids_expected:
                raise SystemExit("bench.py: host-to-host pipeline produced %d tokens, the resident pass %d - number is INVALID" % (ntok, ids_expected))
    # small batch latency
    nd = 64
    small_off = np.zeros(nd + 1, dtype=np.uint64)
    pos, k = 0, 0
    chunks = []
    while k < nd:
        a = int(offs[k % (offs.size - 1)])
        chunks.append(text[a:a + 2048])
        pos += chunks[-1].size
        k += 1
        small_off[k] = pos
    small = np.ascontiguousarray(np.concatenate(chunks))
    lat = []
    for it in range(220):
        t0 = time.perf_counter()
        vocab.tokenize_packed(small, small_off)
        lat.append(time.perf_counter() - t0)
    lat = np.sort(np.array(lat[20:]))
    res["small_batch_latency"] = {"docs": nd, "bytes": int(small.size), "p50_ms": round(float(lat[lat.size // 2]) * 1e3, 3),
                                  "p99_ms": round(float(lat[int(lat.size * 0.99)]) * 1e3, 3), "api": "tm_tokenize_batch (host buffers, warm lane)"}
    log("host_to_host: %s" % {k: v for k, v in res.items() if k != "_ids"})
    return res


def bench_score(args, rank, local_rank, world, vocab, img, kind, capcode, norm_flag, log):
    """trainvocab candidate-scoring pass (BASELINE configs[4], training/trainvocab.go:925-1176): ONE normalized dataset
    of --mbytes MiB in total (strong scaling: every rank owns 1/N of it, uploaded once), a 65536-id candidate
    vocabulary; a step = score the rank's range + ONE RCCL all-reduce(sum) of the (n_ids + 260)-word histogram."""
    import torch
    import torch.distributed as dist
    import tokenmonster_amd as tm
    from tokenmonster_amd import _native as N, synth, dist as tmdist
    total_raw = args.mbytes << 20
    t0 = time.time()
    raw, roffs = synth.synth_corpus(kind, total_raw // world, seed=0x434F5250 + 5 + 1000 * rank)
    raw_bytes = int(raw.size)
    text, _ = synth.normalize_batch(raw, roffs, capcode, norm_flag)   # documents concatenated = the dataset range of this rank
    del raw
    log("dataset range of rank 0: %.1f MB raw -> %.1f MB normalized (%.1fs host)" % (raw_bytes / 1e6, text.size / 1e6, time.time() - t0))
    # ONE whole-buffer walk (training/trainvocab.go:909-922) cut into a byte range per rank: every rank uploads its range followed by
    # the first bytes of the next rank's (the halo a token that straddles the boundary needs), and a pass is: match kernel -> 80 exit
    # states per rank, all-gathered -> finish from the true entry state -> ONE all-reduce of the histogram (tokenmonster_amd/dist.py)
    own_len = int(text.size)
    if world > 1:
        halo = tmdist.exchange_halo(text, rank, world, backend_device="cuda")
        text = np.concatenate([text, halo])
    ds = C.c_void_p()
    N.check(N.lib.tm_dataset_upload(N.ptr(np.ascontiguousarray(text)), int(text.size), C.byref(ds)))
    text = text[:own_len]
    n_ids = vocab.n_ids()
    words = n_ids + 4 + 256
    hist = torch.zeros(words, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    engine = tmdist.HipRange(vocab, ds, own_len, continues=rank + 1 < world, stream=stream, dst=hist.data_ptr(), dst_words=words)

    def step():
        tmdist.score_ranges_exact(engine, rank, world, backend_device="cuda")
        if world > 1:
            tmdist.allreduce_histogram(hist)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    tot = torch.tensor([float(raw_bytes), float(text.size)], dtype=torch.float64, device="cuda")
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
    all_raw, all_norm = float(tot[0].item()), float(tot[1].item())
    scores, tokens, missing = tmdist.decode_histogram(hist.cpu().numpy(), n_ids)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, score_outputs((scores, tokens, missing)), log)
    verified = None
    if rank == 0 and world == 1 and args.verify != 0:
        # bit-exact check against the oracle's scoring mode (outside the timed region): the whole buffer where the host has the cores for it
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from oracle_bind import Oracle
        orc = Oracle(img)
        verified = verify_score(orc, text, lambda n: score_prefix(N, vocab, ds, n_ids, n), (scores, tokens, missing), args, log)
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # the CPU leg walks strips of 1 MiB as the trainvocab workers do before "midway" (training/trainvocab.go:1668-1695): one unit of
        # work per strip, so that the all-cores figure really uses the cores (one whole-buffer document is one unit of work)
        strip = 1 << 20
        cut = np.arange(0, int(text.size) + 1, strip, dtype=np.uint64)
        offs = cut if int(cut[-1]) == int(text.size) else np.concatenate([cut, np.array([text.size], dtype=np.uint64)])
        cpu = cpu_baseline(img, text, offs, args.cpu_sample_mb, log)
        cpu["sample"] += " (strips of 1 MiB; the reference runtime has no scoring mode: this times the identical walk, tokenize_normalized)"
    traffic, traffic_source = None, None
    under_profiler = any(k.startswith("ROCPROF") for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", "")
    if args.measure_traffic and rank == 0 and world == 1 and not under_profiler:
        # HBM traffic of the match kernel of the same pass (it is 85 % of it): separate --pmc passes over tools/k1_time.py --score in a child process
        import subprocess
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pmc_profile.py"), "--fast", "--mbytes", str(args.mbytes), "--groups", "4,5",
                                "--kernel", "k_match_branch", "--out", os.path.join("/tmp", "tm_bench_traffic"), "--extra=--config %s --score" % args.config],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, start_new_session=True)
            k = list(json.loads(r.stdout.decode()).values())[0]
            traffic = int(k["FETCH_SIZE"] * 1024 * 2 + k["WRITE_SIZE"] * 1024)
            traffic_source = "k_match_branch of the same pass, measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes; FETCH_SIZE x 2 on gfx950)"
        except Exception as ex:     # noqa: BLE001
            log("counter passes failed (%s)" % ex)
    if rank == 0:
        value = all_raw * args.steps / elapsed / 1e9
        alg = float(text.size)                       # scoring pass B_alg = N per rank
        out = {
            "metric": "GB/s raw UTF-8 scored, trainvocab candidate-scoring pass, 65536-id candidate vocabulary", "value": round(value, 4),
            "unit": "GB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": "%s vocabulary shape (synthetic, %d ids / %d index records); ONE %d MiB synthetic mixed dataset in total, "
                                   "normalized on the host and resident in HBM (1/N per rank); step = score + all-reduce(sum) of %d uint32" % (
                                       args.config, n_ids, vocab.n_info(), args.mbytes, words),
                       "raw_bytes_total": int(all_raw), "normalized_bytes_total": int(all_norm), "tokens_in_text": int(tokens),
                       "normalized_GBps": round(all_norm * args.steps / elapsed / 1e9, 4),
                       "parallelism": "one whole-buffer walk cut into a byte range per rank (halo + all-gather of 80 exit states per rank), RCCL all-reduce of the score histogram",
                       "rccl_ranks": dist.get_world_size() if world > 1 else 0,
                       "verified_bytes_vs_oracle": ("all (%d)" % verified) if verified == int(text.size) else verified},
            "roofline": {"bound": "hbm", "kernel": "whole scoring pass of one rank", "achieved": round(alg / (elapsed / args.steps) / 1e9, 3),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(alg / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 6),
                         "traffic": traffic, "traffic_source": traffic_source, "traffic_note": TRAFFIC_NOTE, "algorithmic_bytes_per_launch": alg},
            "cpu_baseline": cpu,
        }
        print(json.dumps(out), flush=True)
    N.lib.tm_dataset_free(ds)
    if world > 1:
        dist.destroy_process_group()


def bench_decode(args, rank, local_rank, world, vocab, img, kind, capcode, norm_flag, log):
    """--workload decode: Decode (go/tokenmonster.go:445-550; tokenmonster.cpp:1404-1425) of the ids of the tokenize workload's corpus, device-resident:
    the timed region starts with the uint32 ids + offsets of the rank's shard in HBM (left there by the tokenizer) and ends with the decoded
    text in HBM (tm_batch_decode: lengths -> scan -> gather of the tokens' bytes -> capcode decoding).  `value` = decoded bytes of all ranks
    x K / max-over-ranks wall time.  Documents are sharded by rank, no collective."""
    import torch
    import torch.distributed as dist
    from tokenmonster_amd import _native as N, synth
    t0 = time.time()
    raw, roffs = synth.synth_corpus(kind, args.mbytes << 20, seed=0x434F5250 + 2 + 1000 * rank)
    ndocs = roffs.size - 1
    batch = C.c_void_p()
    N.check(N.lib.tm_batch_create(vocab.handle, int(raw.size) + int(raw.size) // 4 + (1 << 20), ndocs, C.byref(batch)))
    N.check(N.lib.tm_batch_upload_raw(batch, N.ptr(raw), N.ptr(roffs), ndocs))
    stream = torch.cuda.current_stream().cuda_stream
    N.check(N.lib.tm_batch_normalize(batch, C.c_void_p(stream)))
    N.check(N.lib.tm_batch_run(batch, C.c_void_p(stream)))
    ntok, nmiss = C.c_uint64(), C.c_uint64()
    N.check(N.lib.tm_batch_totals(batch, C.byref(ntok), C.byref(nmiss)))
    enc_bytes = int(N.lib.tm_batch_normalized_bytes(batch))
    log("corpus: %d docs, %.1f MB raw -> %d ids resident in HBM (%.1fs)" % (ndocs, raw.size / 1e6, ntok.value, time.time() - t0))
    nbytes, host_docs = C.c_uint64(), C.c_uint32()

    def step():
        N.check(N.lib.tm_batch_decode(batch, 0, C.c_void_p(stream), C.byref(nbytes), C.byref(host_docs)))

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    out_bytes = float(nbytes.value)
    tot = torch.tensor([out_bytes, float(ntok.value)], dtype=torch.float64, device="cuda")
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
    all_out = float(tot[0].item())

    def decoded():
        ooff = np.zeros(ndocs + 1, dtype=np.uint64)
        out = np.empty(int(raw.size) + int(raw.size) // 2 + 64, dtype=np.uint8)
        N.check(N.lib.tm_batch_decoded_download(batch, N.ptr(out), out.size, N.ptr(ooff)))
        return out, ooff
    if args.dump_outputs and rank == 0:
        out, ooff = decoded()
        dump_outputs(args.dump_outputs, stream_outputs("text", out, ooff), log)
        del out, ooff
    T, n_enc = float(ntok.value), float(enc_bytes)
    stage_ms, roofline = None, None
    if args.full:
        # the stages of one pass by HIP events on the launch stream
        ms = (C.c_float * 3)()
        acc = np.zeros(3)
        for _ in range(3):
            N.check(N.lib.tm_batch_decode_timed(batch, 0, C.c_void_p(stream), C.byref(nbytes), C.byref(host_docs), ms))
            acc += np.array(list(ms))
        acc /= 3
        stage_ms = {"tile_lengths_scan": round(float(acc[0]), 4), "k_dec_gather": round(float(acc[1]), 4), "k_dec_capcode": round(float(acc[2]), 4)}
        # algorithmic bytes of each stage: the byte counts of the tiles read the ids once (4T; the key lengths come out of a table of n_ids + 1 words that
        # stays in the caches, and what is written is one word per 2048 ids); the gather reads them once more and writes the encoded text once (the keys
        # come out of a 0.3 MB table); the capcode decoder reads the encoded text once and writes the decoded text once
        alg = {"tile_lengths_scan": 4 * T, "k_dec_gather": 4 * T + n_enc, "k_dec_capcode": n_enc + out_bytes}
        dom = max(stage_ms, key=lambda k: stage_ms[k])
        achieved = alg[dom] / (stage_ms[dom] * 1e-3) / 1e9 if stage_ms[dom] > 0 else 0.0
        e2e_alg = 4 * T + 2 * out_bytes
        roofline = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6),
                    "traffic": None, "algorithmic_bytes_per_launch": alg[dom],
                    "algorithmic_bytes_note": "tile_lengths_scan: 4T ids read; k_dec_gather: 4T ids read, encoded text written once; k_dec_capcode: encoded text read, decoded text written",
                    "whole_pass": {"algorithmic_bytes": e2e_alg, "achieved": round(e2e_alg / (elapsed / args.steps) / 1e9, 3),
                                   "frac": round(e2e_alg / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 6), "note": "4T + 2 N_out over the whole step"}}
    verified, verified_ref = None, None
    cpu = None
    if rank == 0 and args.full:
        # every document of the timed pass: the decoded text must be the NFD form of the raw text (no capcode, nothing missing) ...
        out, ooff = decoded()
        if int(nmiss.value) == 0 and args.verify != 0:
            plain, poff = synth.normalize_batch(raw, roffs, 0, norm_flag)
            if int(ooff[-1]) != plain.size or not (ooff == poff).all() or not (out[: plain.size] == plain).all():
                raise SystemExit("bench.py: the decoded text is not the (NFD) text that was tokenized - number is INVALID")
            verified = ndocs
        # ... and, document by document on a sample, what the reference runtime's decode makes of the same ids (also the CPU baseline)
        if not args.no_cpu_baseline:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from oracle_bind import Reference, have_ref
            if have_ref():
                ids = np.empty(max(int(ntok.value), 1), dtype=np.uint32)
                toff = np.empty(ndocs + 1, dtype=np.uint64)
                N.check(N.lib.tm_batch_download(batch, N.ptr(ids), int(ntok.value), N.ptr(toff), None))
                ref = Reference(img)
                budget, done, nb = 15.0, 0, 0
                t1 = time.perf_counter()
                while done < ndocs and time.perf_counter() - t1 < budget:
                    for d in range(done, min(done + 512, ndocs)):
                        txt = ref.decode(ids[int(toff[d]):int(toff[d + 1])])
                        if txt != out[int(ooff[d]):int(ooff[d + 1])].tobytes():
                            raise SystemExit("bench.py: document %d decodes differently in the reference runtime - number is INVALID" % d)
                        nb += len(txt)
                    done = min(done + 512, ndocs)
                dt = time.perf_counter() - t1
                verified_ref = done
                cpu = {"value": round(nb / dt / 1e9, 5), "unit": "GB/s", "cores": 1, "kind": "reference",
                       "sample": "decode of the first %d documents (%.1f MB of text) of the same id streams by the reference runtime (oracle/_ref, tokenmonster.cpp:1404-1425), "
                                 "1 thread, %.1f s incl. the Python loop around it; every document compared with the device's text" % (done, nb / 1e6, dt)}
    if rank == 0:
        value = all_out * args.steps / elapsed / 1e9
        line = {
            "metric": "GB/s of decoded UTF-8 text, Decode of englishcode-32000 id streams, device-resident", "value": round(value, 4), "unit": "GB/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": "%s vocabulary shape (synthetic, %d ids); the uint32 ids of %d MiB of raw synthetic mixed text per GPU (%d documents, %d ids) resident in HBM "
                                   "-> decoded text in HBM (tm_batch_decode: byte counts of the tiles of ids, scan, gather through LDS, capcode decoding)" % (args.config, vocab.n_ids(), args.mbytes, ndocs, int(T)),
                       "ids_per_gpu": int(T), "encoded_bytes_per_gpu": int(n_enc), "decoded_bytes_per_gpu": int(out_bytes), "host_decoded_docs": int(host_docs.value),
                       "parallelism": "documents sharded by rank, no collective", "rccl_ranks": dist.get_world_size() if world > 1 else 0,
                       "verified_docs_round_trip": verified, "verified_docs_vs_reference": verified_ref},
            "stage_ms": stage_ms,
            "roofline": roofline,
            "cpu_baseline": cpu,
        }
        print(json.dumps(line), flush=True)
    N.lib.tm_batch_free(batch)
    if world > 1:
        dist.destroy_process_group()


def score_prefix(N, vocab, ds, n_ids, n):
    """tm_score over the first n bytes of the resident dataset as one strip -> (scores, tokens_in_text, missing_set)"""
    so, sl = np.array([0], dtype=np.uint64), np.array([n], dtype=np.uint64)
    got = np.zeros(n_ids, dtype=np.uint32)
    tit = C.c_uint64()
    ms8 = np.zeros(32, dtype=np.uint8)
    N.check(N.lib.tm_score(vocab.handle, ds, N.ptr(so), N.ptr(sl), 1, N.ptr(got), C.byref(tit), N.ptr(ms8)))
    return got, tit.value, ms8


def verify_score(orc, text, device_prefix, whole, args, log):
    """the scoring pass against the oracle's scoring mode (training/trainvocab.go:1105-1174 restated; the reference runtime has none), outside
    the timed region.  With the cores for it (-1 = default): the WHOLE buffer as ONE strip, the oracle's serial walk run on every host core
    by tmo_score_strips_mt (exact: strips chained through their entry states) against the histogram of the timed pass itself (`whole`).
    Otherwise a prefix, against tm_score of the same prefix (`device_prefix`).  Returns the number of bytes verified."""
    ncores = os.cpu_count() or 1
    t0 = time.perf_counter()
    if args.verify == -1 and ncores >= 32 and whole is not None:
        exp_s, exp_t, exp_m, redone = orc.score_mt(text, ncores)
        got_s, got_t, got_m = whole
        n = int(text.size)
        what = "whole buffer, %d threads (%d strips redone)" % (ncores, redone)
    else:
        n = min(int(text.size), (2 << 20) * max(1, min(ncores, 16)))
        exp_s, exp_t, exp_m, _ = orc.score_mt(text[:n], ncores)
        got_s, got_t, got_m = device_prefix(n)
        what = "prefix, %d threads" % ncores
    if not ((np.asarray(got_s) == exp_s).all() and int(got_t) == int(exp_t) and (np.asarray(got_m) == exp_m).all()):
        raise SystemExit("bench.py: HIP score histogram differs from the oracle (%s) - number is INVALID" % what)
    log("scoring pass verified against the oracle: %d bytes (%s), %.1f s" % (n, what, time.perf_counter() - t0))
    return n


def bench_in_process(args, img, kind, capcode, norm_flag, log):
    """--in-process: N GPUs driven by ONE process through the library's own multi-device entry points (include/tokenmonster_hip.h "several
    devices", tm_multi.hip) - what a Go host (go/tokenmonster_hip.go: OpenHipDevices / LoadHipAll / ScoreCandidateAll) runs; no torch, no
    ranks.  tokenize: every device owns a resident batch of --mbytes MiB (weak scaling), one host thread per device steps it, all threads
    start together and the clock stops when the last one is through.  score: ONE dataset of --mbytes MiB in total over all devices (strong
    scaling), a step = tm_score_multi = ranges + exit-map chain + the RCCL all-reduce inside the library + the copy of the histogram to the host."""
    import threading
    import tokenmonster_amd as tm
    from tokenmonster_amd import _native as N, synth, multi
    ndev = args.gpus
    have = N.lib.tm_device_count()
    virt = os.environ.get("TM_VIRTUAL_DEVICES")
    if ndev > have and not virt:
        raise SystemExit("--gpus %d but only %d device(s) visible (TM_VIRTUAL_DEVICES=N puts N members on device 0: a code-path check, not a measurement)" % (ndev, have))
    g = multi.Devices([0] * ndev) if virt else multi.Devices(list(range(ndev)))
    vs = multi.VocabSet(g, img)
    n_ids = vs.n_ids()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_bind import Oracle
    base = {"n_gpus": ndev, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "unit": "GB/s"}
    if args.workload == "score":
        raw, roffs = synth.synth_corpus(kind, args.mbytes << 20, seed=0x434F5250 + 5)
        raw_bytes = int(raw.size)
        text, _ = synth.normalize_batch(raw, roffs, capcode, norm_flag)
        del raw
        ds = multi.DatasetSet(g, text)
        for _ in range(args.warmup):
            res = ds.score(vs)
        ranks, why = g.rccl_ranks()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = ds.score(vs)
        elapsed = time.perf_counter() - t0
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, score_outputs(res), log)
        verified = None
        if args.verify != 0:
            one = tm.Vocab(img)
            dsh = C.c_void_p()
            N.check(N.lib.tm_dataset_upload(N.ptr(np.ascontiguousarray(text)), int(text.size), C.byref(dsh)))
            verified = verify_score(Oracle(img), text, lambda n: score_prefix(N, one, dsh, n_ids, n), res, args, log)
            # ... and the multi-device histogram must be the single-device one, word for word
            s1, t1, m1 = score_prefix(N, one, dsh, n_ids, int(text.size))
            if not ((s1 == res[0]).all() and t1 == res[1] and (m1 == res[2]).all()):
                raise SystemExit("bench.py: tm_score_multi differs from tm_score on one device - number is INVALID")
            N.lib.tm_dataset_free(dsh)
        out = dict(base, metric="GB/s raw UTF-8 scored, trainvocab candidate-scoring pass, 65536-id candidate vocabulary", value=round(raw_bytes * args.steps / elapsed / 1e9, 4),
                   ms_per_step=round(elapsed / args.steps * 1e3, 3), scaling="strong",
                   config={"workload": "%s vocabulary shape (synthetic, %d ids); ONE %d MiB synthetic mixed dataset in total, normalized on the host, resident in HBM "
                                       "(1/N per device); step = tm_score_multi: ranges + halos, 80-state exit maps chained on the host, all-reduce(sum) of %d uint32, histogram to the host" % (
                                           args.config, n_ids, args.mbytes, n_ids + 260),
                           "raw_bytes_total": raw_bytes, "normalized_bytes_total": int(text.size), "tokens_in_text": int(res[1]),
                           "parallelism": "in-process: one host thread per device inside libtokenmonster_hip.so, RCCL all-reduce inside tm_score_multi",
                           "rccl_ranks": ranks, "rccl_note": why, "ranges": ds.ranges(), "virtual_devices": bool(virt), "verified_bytes_vs_oracle": verified},
                   roofline={"bound": "hbm", "kernel": "whole scoring pass", "achieved": round(float(text.size) / (elapsed / args.steps) / 1e9, 3), "peak": HBM_PEAK_GBS * ndev,
                             "unit": "GB/s", "frac": round(float(text.size) / (elapsed / args.steps) / 1e9 / (HBM_PEAK_GBS * ndev), 6), "traffic": None,
                             "algorithmic_bytes_per_launch": float(text.size)}, cpu_baseline=None)
        print(json.dumps(out), flush=True)
        ds.close(); vs.close(); g.close()
        return
    # tokenize: a resident batch per device
    shards = []
    for i in range(ndev):
        raw, roffs = synth.synth_corpus(kind, args.mbytes << 20, seed=0x434F5250 + 2 + 1000 * i)
        b = C.c_void_p()
        N.check(N.lib.tm_batch_create(vs.member(i), int(raw.size) + int(raw.size) // 8 + (2 << 20), roffs.size - 1, C.byref(b)))
        N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw), N.ptr(roffs), roffs.size - 1))
        shards.append((raw, roffs, b))
    start = threading.Barrier(ndev + 1)
    done = [0.0] * ndev
    errs = []

    def worker(i):
        try:
            b = shards[i][2]
            for k in range(args.warmup + args.steps):
                if k == args.warmup:
                    N.check(N.lib.tm_batch_totals(b, None, None))      # (synchronizes the batch's stream)
                    start.wait()
                N.check(N.lib.tm_batch_normalize(b, None))
                N.check(N.lib.tm_batch_run(b, None))
            N.check(N.lib.tm_batch_totals(b, None, None))
            done[i] = time.perf_counter()
        except Exception as ex:     # noqa: BLE001
            errs.append(ex)
            start.abort()
    th = [threading.Thread(target=worker, args=(i,)) for i in range(ndev)]
    for t in th:
        t.start()
    start.wait()
    t0 = time.perf_counter()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    elapsed = max(done) - t0
    all_raw = float(sum(int(r.size) for r, _, _ in shards))
    if args.dump_outputs:
        # (device 0's batch)
        b, nd = shards[0][2], shards[0][1].size - 1
        nt = C.c_uint64()
        N.check(N.lib.tm_batch_totals(b, C.byref(nt), None))
        ids, toff, miss = np.empty(max(int(nt.value), 1), dtype=np.uint32), np.empty(nd + 1, dtype=np.uint64), np.empty(max(nd, 1), dtype=np.uint32)
        N.check(N.lib.tm_batch_download(b, N.ptr(ids), int(nt.value), N.ptr(toff), N.ptr(miss)))
        dump_outputs(args.dump_outputs, stream_outputs("ids", ids, toff, ("missing", miss)), log)
        del ids, toff, miss
    # every document of every device against the reference runtime (RAW text through its Tokenize)
    verified = 0
    ntok_all = 0
    from oracle_bind import Reference, have_ref
    ref = Reference(img) if have_ref() and args.verify != 0 else None
    for i, (raw, roffs, b) in enumerate(shards):
        nt = C.c_uint64()
        N.check(N.lib.tm_batch_totals(b, C.byref(nt), None))
        ntok_all += int(nt.value)
        if ref is not None:
            nd = roffs.size - 1
            ids = np.empty(max(int(nt.value), 1), dtype=np.uint32)
            toff = np.empty(nd + 1, dtype=np.uint64)
            miss = np.empty(max(nd, 1), dtype=np.uint32)
            N.check(N.lib.tm_batch_download(b, N.ptr(ids), int(nt.value), N.ptr(toff), N.ptr(miss)))
            ncores = os.cpu_count() or 1
            d2 = nd if ncores >= 32 else max(1, min(nd, int(np.searchsorted(roffs, int(4e6 * ncores), side="right")) - 1))
            bad, first_bad, _ = ref.verify_docs_mt(raw[: int(roffs[d2])], roffs[: d2 + 1], True, ncores, ids, toff[: d2 + 1], miss)
            if bad:
                raise SystemExit("bench.py: device %d: HIP ids differ from the reference runtime's in %d documents (first: %d) - number is INVALID" % (i, bad, first_bad))
            verified += d2
        N.lib.tm_batch_free(b)
    out = dict(base, metric="GB/s raw UTF-8 tokenized, %s vocab" % args.config.split("-consistent")[0].split("-clean")[0].split("-balanced")[0],
               value=round(all_raw * args.steps / elapsed / 1e9, 4), ms_per_step=round(elapsed / args.steps * 1e3, 3), scaling="weak",
               config={"workload": "%s vocabulary shape (synthetic, %d ids), %d MiB raw synthetic mixed text per GPU; end to end: RAW UTF-8 resident in HBM -> normalize + "
                                   "tokenize on the GPU -> uint32 ids in HBM" % (args.config, n_ids, args.mbytes),
                       "parallelism": "in-process: one vocabulary replica (tm_vocab_load_all) and one resident batch per device, one host thread per device, no collective",
                       "raw_bytes_total": int(all_raw), "tokens_total": ntok_all, "virtual_devices": bool(virt), "verified_docs_vs_reference": verified},
               roofline=None, cpu_baseline=None)
    print(json.dumps(out), flush=True)
    vs.close(); g.close()


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU, rendezvous on
    127.0.0.1 (the container hostname may not resolve).  The children see WORLD_SIZE and take the normal path."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


TRAFFIC_NOTE = ("FETCH_SIZE / WRITE_SIZE count the requests on the memory side of the L2, hits in the 256 MB Infinity Cache included: what a vocabulary's tables "
                "(5 - 13 MB) miss in the 4 MB L2 of an XCD is served from there, not from HBM")


def main():
    args = parse()
    if not args.full:
        # a plain run: set up, warm up, time the steps, print the line (every other leg belongs to --full)
        args.verify, args.no_cpu_baseline, args.no_host_to_host, args.no_tuned_leg, args.measure_traffic = 0, True, True, True, False
    if args.also_flags:
        os.environ.setdefault("TM_TEST_HOOKS", "1")      # (the kernel-variant switches are inert unless the process is started this way)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.in_process:
        if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:
            raise SystemExit("--in-process is ONE process driving all GPUs: run it without a launcher")

        def log0(msg):
            print("[bench] " + msg, file=sys.stderr, flush=True)
        import __graft_entry__ as g0
        g0.build()
        from tokenmonster_amd import synth as synth0
        if args.config is None:
            args.config = "englishcode-32000-consistent" if args.workload == "tokenize" else "candidates-65536"
        kind0, _, capcode0, norm0, _, _ = synth0.CONFIGS[args.config]
        return bench_in_process(args, config_image(synth0, args.config), kind0, capcode0, norm0, log0)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:      # never print a line whose n_gpus differs from what was asked for
        raise SystemExit("WORLD_SIZE %d != --gpus %d (launch with --nproc-per-node equal to --gpus, or without a launcher)" % (world, args.gpus))

    def log(msg):
        if rank == 0:
            print("[bench] " + msg, file=sys.stderr, flush=True)

    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the tokenizer has no CPU fallback")
    if args.gpus > torch.cuda.device_count():
        raise SystemExit("--gpus %d but only %d device(s) visible" % (args.gpus, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    import __graft_entry__ as g
    if rank == 0:
        g.build()
    if world > 1:
        dist.barrier()
    import tokenmonster_amd as tm
    from tokenmonster_amd import _native as N, synth
    N.check(N.lib.tm_set_device(local_rank))

    if args.config is None:
        args.config = "candidates-65536" if args.workload == "score" else "englishcode-32000-consistent"
    kind, vsize, capcode, norm_flag, level, vseed = synth.CONFIGS[args.config]
    t0 = time.time()
    if rank == 0:
        img = config_image(synth, args.config)
    if world > 1:
        dist.barrier()
    img = config_image(synth, args.config)
    vocab = tm.Vocab(img)
    if args.tune_mib > 0:
        sraw, sroffs = synth.synth_corpus(kind, int(args.tune_mib * (1 << 20)), seed=0x434F5250 + 77)        # (not the corpus that is timed: another seed)
        stext, _ = synth.normalize_batch(sraw, sroffs, capcode, norm_flag)
        tt = time.time()
        vocab.tune(stext)
        log("tm_vocab_tune on %.3g MiB of other text: %.2f s" % (args.tune_mib, time.time() - tt))
    log("vocab %s: %d ids, %d index records, max token %d, tables %.1f MB (%.1fs)" % (
        args.config, vocab.n_ids(), vocab.n_info(), vocab.max_token_length(), N.lib.tm_vocab_device_bytes(vocab.handle) / 1e6, time.time() - t0))

    if args.workload == "score":
        return bench_score(args, rank, local_rank, world, vocab, img, kind, capcode, norm_flag, log)
    if args.workload == "decode":
        return bench_decode(args, rank, local_rank, world, vocab, img, kind, capcode, norm_flag, log)

    # ---- synthetic corpus shard of this rank ------------------------------------------------------------
    t0 = time.time()
    raw, roffs = synth.synth_corpus(kind, args.mbytes << 20, seed=0x434F5250 + 2 + 1000 * rank)
    raw_bytes = int(raw.size)
    text, offs = synth.normalize_batch(raw, roffs, capcode, norm_flag)   # host normalizer: reference input for verification
    ndocs = offs.size - 1
    log("corpus: %d docs, %.1f MB raw -> %.1f MB normalized (%.1fs host)" % (ndocs, raw_bytes / 1e6, text.size / 1e6, time.time() - t0))

    batch = C.c_void_p()
    N.check(N.lib.tm_batch_create(vocab.handle, int(text.size) + (1 << 20), ndocs, C.byref(batch)))
    t0 = time.time()
    if args.hot_path_only:
        N.check(N.lib.tm_batch_upload(batch, N.ptr(text), N.ptr(offs), ndocs))
    else:
        N.check(N.lib.tm_batch_upload_raw(batch, N.ptr(raw), N.ptr(roffs), ndocs))
    h2d_s = time.time() - t0
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        if not args.hot_path_only:
            N.check(N.lib.tm_batch_normalize(batch, C.c_void_p(stream)))
        N.check(N.lib.tm_batch_run(batch, C.c_void_p(stream)))

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        tot = torch.tensor([float(raw_bytes), float(text.size)], dtype=torch.float64, device="cuda")
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        all_raw, all_norm = float(tot[0].item()), float(tot[1].item())
    else:
        all_raw, all_norm = float(raw_bytes), float(text.size)

    ntok = C.c_uint64()
    nmiss = C.c_uint64()
    N.check(N.lib.tm_batch_totals(batch, C.byref(ntok), C.byref(nmiss)))
    if args.dump_outputs and rank == 0:
        ids = np.empty(max(int(ntok.value), 1), dtype=np.uint32)
        toff = np.empty(ndocs + 1, dtype=np.uint64)
        miss = np.empty(max(ndocs, 1), dtype=np.uint32)
        N.check(N.lib.tm_batch_download(batch, N.ptr(ids), int(ntok.value), N.ptr(toff), N.ptr(miss)))
        dump_outputs(args.dump_outputs, stream_outputs("ids", ids, toff, ("missing", miss)), log)
        del ids, toff, miss

    normalize_ms = None
    fallback_docs = 0 if args.hot_path_only else int(N.lib.tm_batch_host_fallback_docs(batch))
    if args.full and not args.hot_path_only:
        tn = time.perf_counter()
        for _ in range(3):
            N.check(N.lib.tm_batch_normalize(batch, C.c_void_p(stream)))
        torch.cuda.synchronize()
        normalize_ms = (time.perf_counter() - tn) / 3 * 1e3
        # the device-normalized bytes must equal the host normalizer's
        nb = int(N.lib.tm_batch_normalized_bytes(batch))
        if rank == 0:
            dtext = np.empty(max(nb, 1), dtype=np.uint8)
            doffs = np.empty(ndocs + 1, dtype=np.uint64)
            N.check(N.lib.tm_batch_download_text(batch, N.ptr(dtext), nb, N.ptr(doffs)))
            if nb != text.size or not (doffs == offs).all() or not (dtext[:nb] == text).all():
                raise SystemExit("bench.py: device-normalized text differs from the host normalizer - number is INVALID")

    ms = (C.c_float * N.TM_NUM_KERNELS)()
    names = [N.lib.tm_kernel_name(k).decode() for k in range(N.TM_NUM_KERNELS)]
    under_profiler = any(k.startswith("ROCPROF") for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", "")     # (no profiler inside a profiler)
    roofline = roofline_valu = roofline_l2 = None
    # ---- per-kernel time, HIP events on the launch stream (after the timed loop, a few extra passes) --------
    if args.full:
        acc = np.zeros(N.TM_NUM_KERNELS)
        reps = 3
        for _ in range(reps):
            N.check(N.lib.tm_batch_run_timed(batch, C.c_void_p(stream), ms))
            acc += np.array(list(ms))
        acc /= reps
        kernel_ms = {n: round(float(v), 4) for n, v in zip(names, acc)}
        dom = int(np.argmax(acc))
        alg_bytes = float(text.size) + 4.0 * float(ntok.value)     # B_alg = N + 4T per pass
        achieved = alg_bytes / (acc[dom] * 1e-3) / 1e9
        # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process, so the figure is the one
        # tools/pmc_profile.py measured under rocprofv3 for the same configuration and size (FETCH_SIZE x2 + WRITE_SIZE, separate passes,
        # as the MI355X microarchitecture guide prescribes) and wrote to profiles/traffic_latest.json; null when that file is for
        # another configuration.  `traffic_source` says so in the line itself.
        traffic, traffic_source = None, None
        valu_per_wave, salu_per_wave, waves_per_launch, insts_source = None, None, None, None
        l2_reqs = None            # requests of the vector L1s to the L2 per launch of the match kernel (reads + writes)
        tpath = os.path.join(ROOT, "profiles", "traffic_latest.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if tj.get("config") == args.config and tj.get("mbytes") == args.mbytes:
                    traffic = tj.get("hbm_bytes_per_launch")
                    traffic_source = "static: profiles/traffic_latest.json (%s), not measured in this run" % tj.get("measured", "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE")
                    if tj.get("valu_per_wave"):
                        valu_per_wave, salu_per_wave, waves_per_launch = tj["valu_per_wave"], tj.get("salu_per_wave"), tj.get("waves_per_launch")
                        insts_source = "static: profiles/traffic_latest.json, not measured in this run"
                    l2_reqs = tj.get("l2_requests_per_launch")
            except Exception:
                traffic = None
        if args.measure_traffic and rank == 0 and world == 1 and not args.hot_path_only and not under_profiler:
            # separate --pmc passes as the MI355X microarchitecture guide prescribes, the kernels driven without torch (tools/k1_time.py);
            # FETCH_SIZE / WRITE_SIZE are in KB, gfx950 tallies 128-byte fetches at 64 bytes (x2)
            import subprocess
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pmc_profile.py"), "--fast", "--mbytes", str(args.mbytes), "--groups", "0,3,4,5",
                                    "--kernel", "k_match_branch", "--out", os.path.join("/tmp", "tm_bench_traffic")] + (["--extra=--config " + args.config] if args.config else []),
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, start_new_session=True)
                k = list(json.loads(r.stdout.decode()).values())[0]
                if "FETCH_SIZE" in k and "WRITE_SIZE" in k:
                    traffic = int(k["FETCH_SIZE"] * 1024 * 2 + k["WRITE_SIZE"] * 1024)
                    traffic_source = "measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes; FETCH_SIZE x 2 on gfx950) over the same kernel, configuration and size"
                if k.get("SQ_WAVES"):
                    valu_per_wave, salu_per_wave, waves_per_launch = k["SQ_INSTS_VALU"] / k["SQ_WAVES"], k["SQ_INSTS_SALU"] / k["SQ_WAVES"], k["SQ_WAVES"]
                    insts_source = "measured in this run: rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES over the same kernel, configuration and size"
                if k.get("TCP_TCC_READ_REQ_sum"):
                    l2_reqs = k["TCP_TCC_READ_REQ_sum"] + k.get("TCP_TCC_WRITE_REQ_sum", 0.0)
            except Exception as ex:     # noqa: BLE001
                log("counter passes failed (%s): the static figures stay" % ex)
        roofline = {"bound": "hbm", "kernel": names[dom], "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": traffic, "traffic_source": traffic_source, "traffic_note": TRAFFIC_NOTE,
                    "algorithmic_bytes_per_launch": alg_bytes, "kernel_ms": kernel_ms}
        # the same kernel against the port it actually occupies: vector instructions issued per second (one wavefront = one 256-byte segment)
        if valu_per_wave:
            gi = valu_per_wave * waves_per_launch / (acc[dom] * 1e-3) / 1e9
            roofline_valu = {"bound": "valu_issue", "kernel": names[dom], "achieved": round(gi, 2), "peak": round(VALU_PEAK_GINSTS, 1), "unit": "G wave64 instructions/s",
                             "frac": round(gi / VALU_PEAK_GINSTS, 4), "vector_instructions_per_segment": round(valu_per_wave, 1),
                             "scalar_instructions_per_segment": None if salu_per_wave is None else round(salu_per_wave, 1),
                             "vector_instructions_per_input_byte": round(valu_per_wave * waves_per_launch / float(text.size), 3), "source": insts_source}

        # ... and against what its divergent gathers load most: the request rate of the L2 (16 channels per XCD x 8 XCDs, one request per channel
        # and clock of the 2.1 GHz the guide's 34.5 TB/s of L2 bandwidth are 128-byte lines at)
        if l2_reqs:
            gr = l2_reqs / (acc[dom] * 1e-3) / 1e9
            roofline_l2 = {"bound": "l2_requests", "kernel": names[dom], "achieved": round(gr, 1), "peak": L2_PEAK_GREQS, "unit": "G requests/s",
                           "frac": round(gr / L2_PEAK_GREQS, 4), "requests_per_segment": round(l2_reqs / waves_per_launch, 1) if waves_per_launch else None,
                           "source": "rocprofv3 --pmc TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum over the same kernel, configuration and size"}

    # ---- verification of a sample against the oracle (rank 0; outside the timed region) -------------------
    verified = None
    dev_ids = None            # (ids, tok_offsets, missing) of the timed pass, on the host: what every check below compares with
    if args.verify != 0 and world > 1:
        # the checker's library is built once (it normally travels prebuilt), not by every rank at the same moment
        if rank == 0:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import oracle_bind
            if not os.path.exists(oracle_bind.ORACLE_SO):
                oracle_bind.build_oracles()
        dist.barrier()
    if args.verify != 0 and (rank == 0 or world > 1):         # (with several ranks every rank checks a sample of its own shard)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from oracle_bind import Oracle
        orc = Oracle(img)
        cap = int(ntok.value)
        ids = np.empty(max(cap, 1), dtype=np.uint32)
        toff = np.empty(ndocs + 1, dtype=np.uint64)
        miss = np.empty(max(ndocs, 1), dtype=np.uint32)
        N.check(N.lib.tm_batch_download(batch, N.ptr(ids), cap, N.ptr(toff), N.ptr(miss)))
        dev_ids = (ids, toff, miss)
        rng = np.random.default_rng(1)
        verified = 0
        # a random sample against the oracle (our C restatement) in any case; ALL documents against the reference runtime below (cpu_baseline)
        for d in rng.choice(ndocs, size=min(args.verify if args.verify > 0 else 256, ndocs), replace=False):
            exp, m = orc.tokenize(text[int(offs[d]):int(offs[d + 1])])
            got = ids[int(toff[d]):int(toff[d + 1])]
            if got.size != exp.size or (got != exp).any() or m != int(miss[d]):
                raise SystemExit("bench.py: HIP ids differ from the oracle in document %d - number is INVALID" % d)
            verified += 1
    if world > 1 and args.verify != 0:
        tv = torch.tensor([float(verified or 0)], dtype=torch.float64, device="cuda")
        dist.all_reduce(tv, op=dist.ReduceOp.SUM)
        verified = int(tv.item())                        # documents checked against the oracle over all ranks

    if args.also_flags and rank == 0:
        cap = int(ntok.value)
        ref_ids = np.empty(max(cap, 1), dtype=np.uint32)
        ref_toff = np.empty(ndocs + 1, dtype=np.uint64)
        N.check(N.lib.tm_batch_download(batch, N.ptr(ref_ids), cap, N.ptr(ref_toff), None))
        for f in [int(x) for x in args.also_flags.split(",") if x.strip()]:
            old = N.lib.tm_debug_flags(f)
            try:
                step()
                torch.cuda.synchronize()
                tv = time.perf_counter()
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize()
                dtv = (time.perf_counter() - tv) / args.steps
                N.check(N.lib.tm_batch_run_timed(batch, C.c_void_p(stream), ms))
                ids2 = np.empty(max(cap, 1), dtype=np.uint32)
                toff2 = np.empty(ndocs + 1, dtype=np.uint64)
                nt2 = C.c_uint64()
                N.check(N.lib.tm_batch_totals(batch, C.byref(nt2), None))
                same = nt2.value == ntok.value
                if same:
                    N.check(N.lib.tm_batch_download(batch, N.ptr(ids2), cap, N.ptr(toff2), None))
                    same = bool((toff2 == ref_toff).all() and (ids2[:cap] == ref_ids[:cap]).all())
                log("variant flags=%d: %.3f ms/step = %.2f GB/s raw, kernels %s, ids %s the default's" % (
                    f, dtv * 1e3, raw_bytes / dtv / 1e9, {n: round(float(v), 3) for n, v in zip(names, list(ms))}, "EQUAL" if same else "DIFFER FROM"))
            finally:
                N.lib.tm_debug_flags(old)

    # host to host before the CPU baseline: its 256 threads leave this process's threads (and the pinned buffers it allocates next)
    # wherever the scheduler put them last, and pinned memory on the far socket halves the PCIe rate
    h2h = None
    if rank == 0 and world == 1 and not args.hot_path_only and not args.no_host_to_host:
        h2h = host_to_host(vocab, raw, roffs, text, offs, int(ntok.value), log, tm, steps=max(args.steps, 1), lanes=args.h2h_lanes, chunk=args.h2h_chunk_mib << 20,
                           sweep=args.h2h_sweep)
        blob, boff, enc = h2h.pop("_ids")
        if dev_ids is not None and enc == 2:
            # the host-to-host call must have produced the very ids of the resident pass, all of them
            same = np.array_equal(np.frombuffer(blob, dtype=np.uint16), dev_ids[0][: int(ntok.value)].astype(np.uint16)) and np.array_equal(boff, dev_ids[1] * 2)
            if not same:
                raise SystemExit("bench.py: the host-to-host pipeline's ids differ from the resident pass's - number is INVALID")
            h2h["ids_equal_resident_pass"] = True
        del blob, boff

    cpu = None
    verified_ref = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        chk = dev_ids if args.verify == -1 else None
        if args.hot_path_only or not __import__("oracle_bind").have_ref():
            cpu = cpu_baseline(img, text, offs, args.cpu_sample_mb, log, check=chk)
        else:
            cpu = cpu_baseline(img, raw, roffs, args.cpu_sample_mb, log, raw_mode=True, check=chk)
        verified_ref = cpu.pop("verified_docs_vs_reference", None)

    # ---- beside the line of record (whose tables are as tm_vocab_load lays them out): the same step with the tables laid out by use ----
    # (the last leg of the run: its 6 GB of allocations and their release must not sit in front of the host-to-host passes)
    tuned_leg = None
    if rank == 0 and world == 1 and not args.hot_path_only and not args.no_tuned_leg and args.tune_mib == 0 and not under_profiler:
        try:
            tt = time.time()
            sraw, sroffs = synth.synth_corpus(kind, 16 << 20, seed=0x434F5250 + 77)        # (not the corpus that is timed: another seed)
            stext, _ = synth.normalize_batch(sraw, sroffs, capcode, norm_flag)
            tl = time.time()
            vt = tm.Vocab(img, sample=stext)
            load_s = time.time() - tl
            bt = C.c_void_p()
            N.check(N.lib.tm_batch_create(vt.handle, int(text.size) + (1 << 20), ndocs, C.byref(bt)))
            N.check(N.lib.tm_batch_upload_raw(bt, N.ptr(raw), N.ptr(roffs), ndocs))

            def tstep():
                N.check(N.lib.tm_batch_normalize(bt, C.c_void_p(stream)))
                N.check(N.lib.tm_batch_run(bt, C.c_void_p(stream)))
            for _ in range(2):
                tstep()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                tstep()
            torch.cuda.synchronize()
            t_step = (time.perf_counter() - t1) / args.steps
            tacc = np.zeros(N.TM_NUM_KERNELS)
            for _ in range(reps):
                N.check(N.lib.tm_batch_run_timed(bt, C.c_void_p(stream), ms))
                tacc += np.array(list(ms))
            tacc /= reps
            nt2, nm2 = C.c_uint64(), C.c_uint64()
            N.check(N.lib.tm_batch_totals(bt, C.byref(nt2), C.byref(nm2)))
            ids_a = np.empty(max(int(ntok.value), 1), dtype=np.uint32); ids_b = np.empty(max(int(nt2.value), 1), dtype=np.uint32)
            toff_a = np.empty(ndocs + 1, dtype=np.uint64); toff_b = np.empty(ndocs + 1, dtype=np.uint64)
            N.check(N.lib.tm_batch_download(batch, N.ptr(ids_a), int(ntok.value), N.ptr(toff_a), None))
            N.check(N.lib.tm_batch_download(bt, N.ptr(ids_b), int(nt2.value), N.ptr(toff_b), None))
            same = int(nt2.value) == int(ntok.value) and bool((ids_a == ids_b).all()) and bool((toff_a == toff_b).all())
            if not same:
                raise SystemExit("bench.py: the ids under the tables laid out by use differ from the line of record's - number is INVALID")
            tuned_leg = {"tables": "tm_vocab_load_sample on 16 MiB of OTHER synthetic text of the same kind (%.2f s for the load)" % load_s,
                         "ms_per_step": round(t_step * 1e3, 3), "value": round(raw_bytes / t_step / 1e9, 4), "unit": "GB/s",
                         "match_branch_ms": round(float(tacc[dom]), 4), "roofline_frac": round(alg_bytes / (tacc[dom] * 1e-3) / 1e9 / HBM_PEAK_GBS, 6),
                         "ids_equal_line_of_record": same}
            N.lib.tm_batch_free(bt)
            del vt
            log("tables laid out by use: %s (%.1fs)" % (tuned_leg, time.time() - tt))
        except SystemExit:
            raise
        except Exception as ex:     # noqa: BLE001
            log("tuned leg failed (%s)" % ex)
    if rank == 0:
        value = all_raw * args.steps / elapsed / 1e9
        out = {
            "metric": "GB/s raw UTF-8 tokenized, %s vocab" % args.config.split("-consistent")[0].split("-clean")[0].split("-balanced")[0], "value": round(value, 4), "unit": "GB/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": "%s vocabulary shape (synthetic, %d ids / %d index records), %d MiB raw synthetic mixed "
                                   "text per GPU in %d documents; %s, output = uint32 ids + offsets in HBM" % (
                                       args.config, vocab.n_ids(), vocab.n_info(), args.mbytes, ndocs,
                                       "hot path only: input = host-normalized (NFD+capcode) bytes resident in HBM" if args.hot_path_only else
                                       "end to end: input = RAW UTF-8 resident in HBM, normalized (NFD+capcode) on the GPU inside the timed step"),
                       "normalize_ms_per_step": None if normalize_ms is None else round(normalize_ms, 3), "host_fallback_docs": fallback_docs,
                       "raw_bytes_per_gpu": raw_bytes, "normalized_bytes_per_gpu": int(text.size), "tokens_per_gpu": int(ntok.value),
                       "missing": int(nmiss.value), "normalized_GBps": round(all_norm * args.steps / elapsed / 1e9, 4),
                       "h2d_seconds": round(h2d_s, 3), "parallelism": "documents sharded by rank, no collective",
                       "rccl_ranks": dist.get_world_size() if world > 1 else 0,
                       "tables_tuned_on": ("%.3g MiB of other synthetic text (tm_vocab_tune)" % args.tune_mib) if args.tune_mib > 0 else None,
                       "verified_docs_vs_oracle": verified,
                       # every document of the timed pass against the REFERENCE runtime (oracle/_ref: RAW text through its Tokenize, ids and `missing`
                       # compared one by one): "all" when the host had the cores to do the whole corpus in the all-cores leg, else the count
                       "verified_docs_vs_reference": ("all (%d)" % ndocs) if verified_ref == ndocs else verified_ref},
            "roofline": roofline,
            "roofline_valu": roofline_valu,
            "roofline_l2": roofline_l2,
            "tables_by_use": tuned_leg,
            "cpu_baseline": cpu,
            # `value` is the HBM-resident rate (the timed region starts with the raw text in HBM and ends with the ids in HBM); the rate of
            # SURVEY 8(d)'s "first H2D to last D2H" harness (tm_tokenize_pipeline: raw UTF-8 in pinned host memory -> ids in pinned host memory,
            # benchmark/tokenmonster_bench.go:41-55 times around the whole call) is the key below
            "value_definition": "HBM-resident: raw UTF-8 in HBM -> uint32 ids in HBM (normalize + tokenize)",
            # (why `value` is not the host-to-host rate: the measurement contract of this build - task statement, section 4 "Measurement" - reads
            # "`value` is whole-job throughput with inputs already resident in HBM when the timed region starts (if the boundary hands over host
            # buffers, note the PCIe-inclusive rate in DESIGN.md - it is never `value`)"; SURVEY 8(d)'s H2D -> D2H figure is `value_host_to_host`)
            "value_contract": "task statement section 4: value = inputs resident in HBM when the timed region starts; the PCIe-inclusive rate is never `value` -> value_host_to_host",
            "value_resident": round(value, 4),
            "value_host_to_host": None if h2h is None else h2h["pinned"]["value"],
            "host_to_host": h2h,
        }
        print(json.dumps(out), flush=True)
    N.lib.tm_batch_free(batch)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
