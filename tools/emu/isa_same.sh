#!/bin/bash
# tools/emu/isa_same.sh <git-rev>: is the gfx950 code of the kernel units at <git-rev> the same as in the working tree?  Kernel by kernel.
# A change that is meant to be source-only — macro wrapping for tools/emu, comments, host code — must leave every instruction where it was
# (the __hip_cuid_* symbol, a hash of the source text, lies outside the kernels and is not looked at).  A refactor of device code may move
# some: for every kernel that differs both sides are printed, `rev | tree` — vgpr_count, sgpr_count, group_segment_fixed_size (LDS),
# private_segment_fixed_size (scratch), instructions (all, VALU, SALU) and the length, loop label to back branch, of every innermost loop that
# reads and writes LDS: the straight-line loop of a chain walk (K4, the scoring and span walks) is one, and K4's time follows it
# (profiles/r05_issue_model.txt).  Exit status 1 if any kernel differs.
set -e
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
REV=${1:-HEAD}
OLD=$(mktemp -d) ; NEW=$(mktemp -d)
trap 'rm -rf "$OLD" "$NEW"' EXIT
git -C "$ROOT" archive "$REV" tokenmonster_amd/csrc include | tar -x -C "$OLD"
UNITS="tm_kernels tm_norm tm_decode tm_spans tm_collate tm_windows tm_pairs tm_units"
for f in $UNITS; do
  ( cd "$OLD/tokenmonster_amd/csrc" && /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -I ../../include -I . -x hip $f.hip --cuda-device-only -S -o "$OLD/$f.s" 2>/dev/null ) &
  ( cd "$ROOT/tokenmonster_amd/csrc" && /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -I ../../include -I . -x hip $f.hip --cuda-device-only -S -o "$NEW/$f.s" 2>/dev/null ) &
done
wait
python3 - "$OLD" "$NEW" $UNITS <<'EOF'
import os, re, subprocess, sys

def kernels(path):
    """{symbol: (instructions, {metadata field: value})} of one assembly file (none at all: the unit does not exist on that side)"""
    if not os.path.exists(path): return {}
    lines = open(path).read().split("\n")
    out, meta, i = {}, {}, 0
    cur = {}
    for ln in lines[lines.index("amdhsa.kernels:") + 1 if "amdhsa.kernels:" in lines else len(lines):]:      # the metadata at the end: one map per kernel
        m = re.match(r"  (- |  )\.(\w+):\s+(\S+)\s*$", ln)
        if not m: continue
        if m.group(1) == "- ": cur = {}
        cur[m.group(2)] = m.group(3)
        if m.group(2) == "name": meta[m.group(3)] = cur
    while i < len(lines):
        m = re.match(r"\s+\.type\s+(\S+),@function", lines[i])
        if m:
            sym, body = m.group(1), []
            while not lines[i].startswith(sym + ":"): i += 1
            i += 1
            while not lines[i].startswith(".Lfunc_end"):
                t = re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", lines[i].split(";")[0].strip())      # (labels carry the function's number in the unit)
                if t and not t.startswith("."): body.append(t)
                elif re.match(r"\.L\w+:", t): body.append(t)
                i += 1
            out[sym] = (body, meta.get(sym, {}))
        i += 1
    return out

def counts(body):
    ins = [t for t in body if not t.endswith(":")]
    return len(ins), sum(t.startswith("v_") for t in ins), sum(t.startswith("s_") for t in ins)

def lds_loops(body):
    """instruction counts, loop label to back branch, of the innermost loops that read AND write LDS (a walk's straight-line loop is one)"""
    at = {t[:-1]: k for k, t in enumerate(body) if t.endswith(":")}
    spans = []
    for k, t in enumerate(body):
        m = re.match(r"s_c?branch\w*\s+(\S+)", t)
        if m and at.get(m.group(1), k) < k: spans.append((at[m.group(1)], k))
    res = []
    for s, k in spans:
        if any(s2 >= s and k2 <= k and (s2, k2) != (s, k) for s2, k2 in spans): continue
        blk = [x for x in body[s + 1:k + 1] if not x.endswith(":")]
        if any(x.startswith("ds_write") for x in blk) and any(x.startswith("ds_read") for x in blk): res.append(len(blk))
    return res

def by_name(ks):
    """the kernels of a unit by demangled name without the arguments (a kernel whose signature changed is still the same kernel);
    by symbol where that name is not unique"""
    syms = list(ks)
    try: names = [n.split("(")[0].replace("void ", "") for n in subprocess.run(["c++filt"] + syms, stdout=subprocess.PIPE, text=True).stdout.split("\n")[:len(syms)]]
    except OSError: names = syms
    return {(n if names.count(n) == 1 else s): ks[s] for s, n in zip(syms, names)}

old_dir, new_dir, units = sys.argv[1], sys.argv[2], sys.argv[3:]
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
rc = 0
for u in units:
    a, b = by_name(kernels("%s/%s.s" % (old_dir, u))), by_name(kernels("%s/%s.s" % (new_dir, u)))
    same = [s for s in a if s in b and a[s][0] == b[s][0]]
    print("%s: %d kernels, %d identical" % (u, len(set(a) | set(b)), len(same)))
    for s in sorted(set(a) | set(b)):
        if s in same: continue
        rc = 1
        if s not in a or s not in b: print("  %s: only in %s" % (s, "rev" if s in a else "tree")); continue
        (ba, ma), (bb, mb) = a[s], b[s]
        ca, cb = counts(ba), counts(bb)
        print("  %s: DIFFERS" % s)
        print("    " + "  ".join("%s %s | %s" % (f, ma.get(f, "?"), mb.get(f, "?")) for f in FIELDS))
        print("    instructions %d | %d  VALU %d | %d  SALU %d | %d  innermost LDS loops %s | %s" % (ca[0], cb[0], ca[1], cb[1], ca[2], cb[2], lds_loops(ba), lds_loops(bb)))
sys.exit(rc)
EOF
