"""Register budget of the C3 render kernels, read from the built library's gfx950 code object (no GPU needed).

k_render<volpath, 1024, LDS BVH, independent sampler, {wide, compact} records> must keep 4 waves per SIMD (at most 128 VGPRs)
and its scratch area at or below what the trip's current live ranges need: a change that puts the spills
back shows up here before it shows up as time.  Skipped when the library or the LLVM tools are missing."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "liverrenderer_amd", "libliverrt.so")
LLVM = "/opt/rocm/llvm/bin"
TOOLS = {k: os.path.join(LLVM, k) for k in ("clang-offload-bundler", "llvm-objcopy", "llvm-readelf")}
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

# mangled name prefix -> (max VGPRs, max private segment bytes per lane)
C3_INSTANCES = {
    "_ZN3lrt8k_renderILi1ELi1024ELb1ELb0ELb1ELb0EE": (128, 80),    # compact records (the C3 kernel)
    "_ZN3lrt8k_renderILi1ELi1024ELb1ELb0ELb0ELb0EE": (128, 80),    # wide records
}


def _kernel_metadata(tmp_path):
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([TOOLS["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fat, LIB, str(tmp_path / "stripped.so")], check=True, capture_output=True)
    subprocess.run([TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co], check=True, capture_output=True)
    notes = subprocess.run([TOOLS["llvm-readelf"], "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for entry in re.split(r"\n  - ", notes):                 # one amdhsa.kernels entry each (deeper lists are indented further)
        m = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if not m:
            continue
        kernels[m.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", entry, re.M)}
    return kernels


@pytest.mark.skipif(not os.path.exists(LIB), reason="libliverrt.so is not built")
@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS.values()), reason="LLVM offload tools missing")
def test_c3_kernels_keep_four_waves_and_their_scratch_budget(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    for prefix, (max_vgpr, max_scratch) in C3_INSTANCES.items():
        names = [n for n in kernels if n.startswith(prefix)]
        assert len(names) == 1, (prefix, names)
        md = kernels[names[0]]
        assert md["vgpr_count"] <= max_vgpr, (names[0], md)
        assert md["private_segment_fixed_size"] <= max_scratch, (names[0], md)
