"""Where a kernel's global loads are issued and where it waits for them: a report to read, without a GPU.

Compiles one unit of hier-slam_amd/csrc to gfx950 assembly with the unit's own flags from csrc/Makefile and prints, in program order, for
every kernel whose demangled name contains the given text:
    LOADS    a run of vector-memory loads (global_load_* / flat_load_* / buffer_load_*) with nothing but other instructions between them
             that are no waits, labels or branches; the opcodes and how many
    WAIT     every s_waitcnt that names vmcnt, with its count
    LOOP     every label some later branch jumps back to (a loop header), and the branch that closes it
Each line carries the line number of the .s file, and the source file and line of the last .loc in front of it.
usage: python tools/isa_waits.py hsr_render_bwd_q.hip "render_bwd_q_kernel<26, 224" [-DHSR_TRACE] > profiles/<name>.txt
It looks for nothing else; whether a wait is exposed is for the reader to judge from what stands between it and the loads."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hier-slam_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT") or shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
BASE_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=" + os.environ.get("ARCH", "gfx950"), "-Wall", "-Wno-unused-function"]
FILE_FLAGS = {"hsr_render_bwd_q.hip": ["-fno-slp-vectorize"]}   # csrc/Makefile, HSR_FILE_FLAGS (the -ffp-contract=off units have no tile kernel)

LOAD = re.compile(r"^\s+((?:global|flat|buffer|scratch)_load_\w+)\s")
WAIT = re.compile(r"^\s+s_waitcnt\s+(.*vmcnt\((\d+)\).*)$")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+(s_c?branch\w*)\s+(\.LBB\d+_\d+)")
LOC = re.compile(r"^\s+\.loc\s+(\d+)\s+(\d+)\s")
FILE = re.compile(r'^\s+\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"')


def assembly(unit, extra):
    src = unit if os.path.isabs(unit) else os.path.join(CSRC, unit)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "unit.s")
        subprocess.check_call([HIPCC] + BASE_FLAGS + FILE_FLAGS.get(os.path.basename(src), []) + list(extra) +
                              ["-g1", "-S", "--cuda-device-only", src, "-o", out], cwd=CSRC)
        with open(out) as f:
            return f.read().splitlines()


def functions(lines):
    """[(mangled name, first line, last line)] of the .text functions"""
    out, cur = [], None
    for i, line in enumerate(lines):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = (m.group(1), i)
        elif cur and re.match(r"^\s+\.size\s+" + re.escape(cur[0]) + ",", line):
            out.append((cur[0], cur[1], i))
            cur = None
    return out


def demangle(names):
    if not CXXFILT:   # no demangler: the text to look for has to be a piece of the mangled name then
        return list(names)
    res = subprocess.check_output([CXXFILT] + names, text=True).splitlines()
    return [r.replace("(anonymous namespace)::", "") for r in res]


def report(lines, first, last):
    files = {m.group(1): os.path.basename(m.group(2)) for l in lines for m in [FILE.match(l)] if m}
    body = lines[first:last]
    label_at = {m.group(1): i for i, l in enumerate(body) for m in [LABEL.match(l)] if m}
    headers = {}   # label -> line of the last branch back to it
    for i, l in enumerate(body):
        m = BRANCH.match(l)
        if m and m.group(2) in label_at and label_at[m.group(2)] <= i:
            headers[m.group(2)] = i
    closes = {v: k for k, v in headers.items()}
    src, run, run_at, run_src = "?", [], 0, "?"

    def flush_run():
        if run:
            kinds = {}
            for op in run:
                kinds[op] = kinds.get(op, 0) + 1
            print("%6d  %-26s LOADS  %2d: %s" % (first + run_at + 1, run_src, len(run), ", ".join("%d x %s" % (n, op) for op, n in kinds.items())))
            run.clear()

    for i, l in enumerate(body):
        m = LOC.match(l)
        if m:
            if int(m.group(2)):
                src = "%s:%s" % (files.get(m.group(1), "file" + m.group(1)), m.group(2))
            continue
        m = LOAD.match(l)
        if m:
            if not run:
                run_at, run_src = i, src
            run.append(m.group(1))
            continue
        w, lab = WAIT.match(l), LABEL.match(l)
        if w or lab or i in closes or BRANCH.match(l):
            flush_run()
        if w:
            print("%6d  %-26s WAIT   vmcnt(%s)%s" % (first + i + 1, src, w.group(2), "" if w.group(1).strip() == "vmcnt(%s)" % w.group(2) else "   [" + w.group(1).strip() + "]"))
        if lab and lab.group(1) in headers:
            print("%6d  %-26s LOOP   %s:  (closed at %d)" % (first + i + 1, src, lab.group(1), first + headers[lab.group(1)] + 1))
        if i in closes:
            print("%6d  %-26s LOOP   end of %s" % (first + i + 1, src, closes[i]))
    flush_run()


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    unit, want, extra = argv[1], argv[2].replace(" ", ""), argv[3:]
    lines = assembly(unit, extra)
    funcs = functions(lines)
    names = demangle([f[0] for f in funcs]) if funcs else []
    hit = False
    for (mangled, first, last), name in zip(funcs, names):
        if want in name.replace(" ", ""):
            hit = True
            print("== %s  (%s%s; %d lines of assembly)" % (re.sub(r"\(.*$", "", name), os.path.basename(unit), " " + " ".join(extra) if extra else "", last - first))
            report(lines, first, last)
    if not hit:
        sys.exit("no kernel of %s matches %r; it has: %s" % (unit, argv[2], ", ".join(sorted(set(re.sub(r"\(.*$", "", n) for n in names)))))


if __name__ == "__main__":
    main(sys.argv)
