"""The 64-byte-record volpath kernels (record_layout.h, RecordLayout::Closed) compile only what closed_records() in device.hip leaves reachable (DESIGN.md section
6d): read from the built library's gfx950 code object, no GPU needed.

Both instances must hold every value of the trip in registers (no scratch, no spilled VGPR) at 4 waves per SIMD (at most 128 VGPRs), and
their code must stay near the size of this build: a branch that the proof makes dead and that comes back shows up here as code bytes
before it shows up as time.  Skipped when the library or the LLVM tools are missing."""
import os
import subprocess

import pytest

from test_kernel_resources import LIB, TOOLS, _kernel_metadata

KB = 1024
# mangled name prefix -> largest code size in bytes: this build's size rounded up to the next KB
CLOSED_INSTANCES = {
    "_ZN3lrt8k_renderILi103ELi1024ELb1ELb0ELb1ELb0EE": 38 * KB,    # independent sampler (the C3 kernel): 38 828 B; 78 424 B before the dead branches left
    "_ZN3lrt8k_renderILi103ELi1024ELb1ELb1ELb1ELb0EE": 42 * KB,    # ld sampler: 42 112 B; 82 480 B before
}


def _function_sizes(code_object):
    out = subprocess.run([TOOLS["llvm-readelf"], "-s", "-W", code_object], check=True, capture_output=True, text=True).stdout
    sizes = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            sizes[f[7]] = int(f[2])
    return sizes


@pytest.mark.skipif(not os.path.exists(LIB), reason="libliverrt.so is not built")
@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS.values()), reason="LLVM offload tools missing")
def test_closed_record_kernels_hold_the_trip_in_registers_and_stay_small(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    sizes = _function_sizes(str(tmp_path / "gfx950.co"))          # (the code object _kernel_metadata extracted)
    for prefix, max_bytes in CLOSED_INSTANCES.items():
        names = [n for n in kernels if n.startswith(prefix)]
        assert len(names) == 1, (prefix, names)
        md = kernels[names[0]]
        print(names[0], md, "code bytes", sizes.get(names[0]))
        assert md["private_segment_fixed_size"] == 0, (names[0], md)
        assert md["vgpr_spill_count"] == 0, (names[0], md)
        assert md["vgpr_count"] <= 128, (names[0], md)
        assert 0 < sizes[names[0]] <= max_bytes, (names[0], sizes[names[0]], max_bytes)
