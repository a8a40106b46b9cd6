"""Records tests/golden/tree_labels_parent.npz on an MI355X: the labels the built library gives on the inputs of
tests/test_gpu_tree_labels_pin.py, with the sha256 of every input.  Run it on the commit whose labels are to be pinned, never on a tree
the pin is meant to check: the file in the repository was written by commit 348d066, the parent of the one that added csrc/hsr_tree.h.
Run: python tests/golden/make_tree_labels_pin.py [OUT.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "hier-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_gpu_tree_labels_pin as pin  # noqa: E402


def main(path):
    inp = pin.inputs()
    out = pin.labels_of(inp)
    out.update(pin.digests(inp))
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %s" % (path, os.path.getsize(path), ", ".join("%s%s" % (k, v.shape) for k, v in sorted(out.items()))))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tree_labels_parent.npz"))
