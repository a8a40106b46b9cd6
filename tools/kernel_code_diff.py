"""Compare the gfx950 code of every kernel in two builds of the same units, without a GPU.

Each argument pair is a directory of device-only objects, one per unit, made with the unit's own flags from csrc/Makefile:
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 [-ffp-contract=off] --cuda-device-only --no-gpu-bundle-output -c X.hip -o DIR/X.o
usage: python tools/kernel_code_diff.py PARENT_DIR TREE_DIR > profiles/<name>.txt
One line per kernel: unit, kernel, bytes at the parent, bytes at the tree, "identical" or the number of differing disassembly lines
(addresses and encodings stripped; a unified diff's +/- lines), and whether the two sides hold the same multiset of opcodes."""
import difflib
import os
import re
import subprocess
import sys

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")


def short(name):
    name = re.sub(r"^void ", "", name)
    name = name.replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*$", "", name)             # drop the parameter list, keep template arguments


def kernels(obj):
    """{demangled name: (size, [instruction lines])} of the functions in a device object; none for a unit that side does not have"""
    if not os.path.exists(obj):
        return {}
    sizes = {}
    for line in subprocess.check_output([OBJDUMP, "-t", "-C", obj], text=True).splitlines():
        m = re.match(r"^[0-9a-f]+ [gl ].{6} \.text\s+([0-9a-f]+) (?:\.protected |\.hidden )?(.+)$", line)
        if m and " F " in line[:26]:
            sizes[short(m.group(2))] = int(m.group(1), 16)
    dis = subprocess.check_output([OBJDUMP, "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", obj], text=True)
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
        if m:
            cur = short(m.group(1))
            code[cur] = []
        elif cur and line.strip():
            code[cur].append(line.split("//")[0].strip())
    return {n: (sz, code.get(n, [])) for n, sz in sizes.items()}


def main(parent_dir, tree_dir):
    print("%-18s %-46s %8s %8s  %s" % ("unit", "kernel", "parent B", "tree B", "code"))
    for obj in sorted(os.listdir(tree_dir)):
        if not obj.endswith(".o"):
            continue
        a, b = kernels(os.path.join(parent_dir, obj)), kernels(os.path.join(tree_dir, obj))
        for name in sorted(set(a) | set(b)):
            sa, ca = a.get(name, (0, []))
            sb, cb = b.get(name, (0, []))
            if ca == cb and sa == sb:
                verdict = "identical"
            else:
                n = sum(1 for d in difflib.unified_diff(ca, cb, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
                same_ops = sorted(l.split()[0] for l in ca) == sorted(l.split()[0] for l in cb)
                verdict = "%d lines differ%s" % (n, " (same opcodes, other order or registers)" if same_ops else
                                                 "; %d -> %d instructions" % (len(ca), len(cb)))
            print("%-18s %-46s %8d %8d  %s" % (obj[:-2], name, sa, sb, verdict))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
