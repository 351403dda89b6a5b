"""The set of kernels in the built library's gfx950 code object (no GPU needed) equals tests/golden/kernel_names.txt, the sorted
mangled names, one per line.

device.hip names every render-kernel instance in its tables (kernels() and the small arrays beside it), and naming an instance
compiles it: a row too many costs seconds of build time and code-object bytes, a row too few is a launch that fails at run time.  A change
that adds or drops an instance edits the list in the open.  Skipped when the library or the LLVM tools are missing."""
import os

import pytest

from test_kernel_resources import LIB, TOOLS, _kernel_metadata

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_names.txt")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libliverrt.so is not built")
@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS.values()), reason="LLVM offload tools missing")
def test_kernel_names_equal_the_pinned_list(tmp_path):
    built = set(_kernel_metadata(tmp_path))
    with open(GOLDEN) as f:
        pinned = [l.strip() for l in f if l.strip()]
    assert pinned == sorted(set(pinned)), "kernel_names.txt must be sorted and free of duplicates"
    added, missing = sorted(built - set(pinned)), sorted(set(pinned) - built)
    assert not added and not missing, "kernels added: %s\nkernels missing: %s" % ("\n  ".join([""] + added) or " none", "\n  ".join([""] + missing) or " none")
