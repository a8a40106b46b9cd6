"""What a kernel's gfx950 code is made of: instruction counts by class, spills, FLAT accesses and the waits inside its loops; a report
to read, without a GPU.  A sibling of tools/isa_waits.py (same compile, same way of finding the kernels).

For every kernel of the unit whose demangled name contains the given text it prints
    COUNTS   static instruction counts: VALU, of which v_cndmask / v_cmp*; SALU; LDS (ds_*); global, FLAT and scratch accesses; s_waitcnt;
             s_barrier;
    SPILLS   SGPR spills (v_writelane_b32 / v_readlane_b32 pairs) and the compiler's own figures from the kernel's metadata
             (.sgpr_spill_count, .vgpr_spill_count, .sgpr_count, .vgpr_count, LDS bytes);
    LOOP     every loop (a label some later branch jumps back to) with, in program order, its LDS atomics, its stores and every
             s_waitcnt that names lgkmcnt or vmcnt.
usage: python tools/isa_counts.py hsr_sort.hip tile_sort_pair_kernel [--no-loops] [SOURCE-FILE-OR-FLAGS...] > profiles/<name>.txt
An argument that ends in .hip and exists replaces the unit's source (the unit name still selects the flags): that is how a parent
revision's file, checked out elsewhere, is read with the tree's headers.  Counts are static: an instruction in a loop counts once."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_waits as W   # noqa: E402

NO_CONTRACT = {"hsr_preprocess.hip"}   # csrc/Makefile, HSR_FILE_FLAGS, for the units this report is used on

INSTR = re.compile(r"^\s+([a-z_0-9]+)\b(.*)$")
WAITANY = re.compile(r"^\s+s_waitcnt\s+(.*)$")


def assembly(unit, source, extra):
    flags = W.BASE_FLAGS + W.FILE_FLAGS.get(unit, []) + (["-ffp-contract=off"] if unit in NO_CONTRACT else [])
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "unit.s")
        subprocess.check_call([W.HIPCC] + flags + ["-I", W.CSRC] + list(extra) + ["-g1", "-S", "--cuda-device-only", source, "-o", out],
                              cwd=W.CSRC)
        with open(out) as f:
            return f.read().splitlines()


def klass(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("flat_"):
        return "FLAT"
    if op.startswith("global_") or op.startswith("buffer_"):
        return "global"
    if op.startswith("scratch_"):
        return "scratch"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op == "s_barrier":
        return "s_barrier"
    if op.startswith("s_"):
        return "SALU"
    return None


def kernel_metadata(lines, mangled):
    """metadata entries are lists of '.key: value' lines between '  - .args:' markers; pick the block that names this kernel"""
    blocks, cur = [], []
    in_md = False
    for l in lines:
        if ".amdgpu_metadata" in l:
            in_md = True
            continue
        if ".end_amdgpu_metadata" in l:
            break
        if not in_md:
            continue
        if re.match(r"^  - ", l) and cur:
            blocks.append(cur)
            cur = []
        cur.append(l)
    if cur:
        blocks.append(cur)
    for b in blocks:
        if any(re.match(r"^\s+\.name:\s+" + re.escape(mangled) + r"\s*$", l) for l in b):
            out = {}
            for l in b:
                m = re.match(r"^\s+\.(sgpr_spill_count|vgpr_spill_count|sgpr_count|vgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\S+)", l)
                if m:
                    out[m.group(1)] = m.group(2)
            return out
    return {}


def report(lines, first, last, mangled, loops=True):
    body = lines[first:last]
    files = {m.group(1): os.path.basename(m.group(2)) for l in lines for m in [W.FILE.match(l)] if m}
    counts, ops = {}, {}
    for l in body:
        m = INSTR.match(l)
        if not m or l.lstrip().startswith(".") or l.lstrip().startswith(";"):
            continue
        k = klass(m.group(1))
        if k:
            counts[k] = counts.get(k, 0) + 1
            ops[m.group(1)] = ops.get(m.group(1), 0) + 1
    cnd = sum(n for o, n in ops.items() if o.startswith("v_cndmask"))
    cmp64 = sum(n for o, n in ops.items() if o.startswith("v_cmp") and ("_u64" in o or "_i64" in o))
    cmpall = sum(n for o, n in ops.items() if o.startswith("v_cmp"))
    print("  COUNTS  VALU %d (v_cndmask %d, v_cmp* %d of which 64-bit %d)  SALU %d  LDS %d  global %d  FLAT %d  scratch %d  s_waitcnt %d  s_barrier %d"
          % (counts.get("VALU", 0), cnd, cmpall, cmp64, counts.get("SALU", 0), counts.get("LDS", 0), counts.get("global", 0),
             counts.get("FLAT", 0), counts.get("scratch", 0), counts.get("s_waitcnt", 0), counts.get("s_barrier", 0)))
    mem = sorted((o, n) for o, n in ops.items() if klass(o) in ("LDS", "global", "FLAT", "scratch"))
    print("  MEMORY  " + ", ".join("%d x %s" % (n, o) for o, n in mem))
    md = kernel_metadata(lines, mangled)
    print("  SPILLS  v_writelane_b32 %d, v_readlane_b32 %d;  metadata: %s"
          % (ops.get("v_writelane_b32", 0), ops.get("v_readlane_b32", 0), ", ".join("%s %s" % kv for kv in sorted(md.items())) or "none found"))
    if not loops:
        return
    label_at = {m.group(1): i for i, l in enumerate(body) for m in [W.LABEL.match(l)] if m}
    headers = {}
    for i, l in enumerate(body):
        m = W.BRANCH.match(l)
        if m and m.group(2) in label_at and label_at[m.group(2)] <= i:
            headers[m.group(2)] = i
    for lab, end in sorted(headers.items(), key=lambda kv: label_at[kv[0]]):
        beg = label_at[lab]
        src, events = "?", []
        for i in range(beg, end + 1):
            l = body[i]
            m = W.LOC.match(l)
            if m:
                if int(m.group(2)):
                    src = "%s:%s" % (files.get(m.group(1), "file" + m.group(1)), m.group(2))
                continue
            m = INSTR.match(l)
            if not m:
                continue
            op = m.group(1)
            w = WAITANY.match(l)
            if w:
                events.append("%d %s: s_waitcnt %s" % (first + i + 1, src, w.group(1).strip()))
            elif (op.startswith("ds_") and "rtn" in op) or "_store_" in op or "_atomic_" in op:
                events.append("%d %s: %s" % (first + i + 1, src, op))
        if events:
            print("  LOOP    %s, lines %d-%d:" % (lab, first + beg + 1, first + end + 1))
            for e in events:
                print("            " + e)


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    unit, want = os.path.basename(argv[1]), argv[2].replace(" ", "")
    source = os.path.join(W.CSRC, unit)
    extra, loops = [], True
    for a in argv[3:]:
        if a == "--no-loops":
            loops = False
        elif a.endswith(".hip") and os.path.exists(a):
            source = os.path.abspath(a)
        else:
            extra.append(a)
    lines = assembly(unit, source, extra)
    funcs = W.functions(lines)
    names = W.demangle([f[0] for f in funcs]) if funcs else []
    hit = False
    for (mangled, first, last), name in zip(funcs, names):
        if want in name.replace(" ", ""):
            hit = True
            print("== %s  (%s; %d lines of assembly)" % (re.sub(r"\(.*$", "", name), os.path.basename(source), last - first))
            report(lines, first, last, mangled, loops)
    if not hit:
        sys.exit("no kernel of %s matches %r" % (unit, argv[2]))


if __name__ == "__main__":
    main(sys.argv)
