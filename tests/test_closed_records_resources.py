"""Register budget of the 64-byte-record C3 kernels (record_layout.h, RecordLayout::Closed), read from the built library's gfx950 code object (no GPU needed).

k_render<LRT_INTEGRATOR_VOLPATH_CLOSED, 1024, LDS BVH, {independent, ld} sampler, compact> must keep 4 waves per SIMD (at most 128 VGPRs)
and the scratch area the smaller record leaves (the 80-byte C3 kernel needs 80 B): spills that come back show up
here before they show up as time.  Skipped when the library or the LLVM tools are missing."""
import os

import pytest

from test_kernel_resources import LIB, TOOLS, _kernel_metadata

# mangled name prefix -> (max VGPRs, max private segment bytes per lane)
CLOSED_INSTANCES = {
    "_ZN3lrt8k_renderILi103ELi1024ELb1ELb0ELb1ELb0EE": (128, 68),    # independent sampler (the C3 kernel)
    "_ZN3lrt8k_renderILi103ELi1024ELb1ELb1ELb1ELb0EE": (128, 76),    # ld sampler (the 80-byte instance: 96)
}


@pytest.mark.skipif(not os.path.exists(LIB), reason="libliverrt.so is not built")
@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS.values()), reason="LLVM offload tools missing")
def test_closed_record_kernels_keep_four_waves_and_their_scratch_budget(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    for prefix, (max_vgpr, max_scratch) in CLOSED_INSTANCES.items():
        names = [n for n in kernels if n.startswith(prefix)]
        assert len(names) == 1, (prefix, names)
        md = kernels[names[0]]
        assert md["vgpr_count"] <= max_vgpr, (names[0], md)
        assert md["private_segment_fixed_size"] <= max_scratch, (names[0], md)
