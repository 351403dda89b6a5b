"""The path-record layout table (liverrenderer_amd/csrc/record_layout.h) without a GPU: tests/host/record_layout_main.cpp is compiled
under AddressSanitizer and UBSan the way tests/test_scene_prep.py compiles its program, run once, and its JSON lines are compared with
the numbers written out here (include/liverrt.h, CELLS of tests/test_launch_matrix_gpu.py).  Only that program is
sanitized; nothing of it is loaded into Python."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "liverrenderer_amd", "csrc")

BASE = [["o_maxt", 16], ["d_eta", 16], ["tp_pdf", 16]]
WIDE_TAIL = [["res_flags", 16], ["lp_lane", 16], ["rng", 8]]
WS = [["res_flags", 16], ["lp_lane", 16], ["rng", 16], ["tdepth", 8]]
W14 = [["w1", 16], ["w2", 16], ["w3", 16], ["w4", 16]]
# form -> (layout, compact, bytes per record, streams in table order)
FORMS = {
    "wide":        ("wide", 0, 88, BASE + WIDE_TAIL),
    "compact":     ("wide", 1, 80, BASE + [["res_flags", 16], ["rng", 16]]),
    "bio":         ("bio", 0, 96, BASE + WIDE_TAIL + [["tdepth", 8]]),
    "bio compact": ("bio", 1, 88, BASE + [["res_flags", 16], ["rng", 16], ["tdepth", 8]]),
    "het":         ("het", 0, 104, BASE + WIDE_TAIL + [["hit", 16]]),
    "mis":         ("mis", 0, 168, BASE + WIDE_TAIL + [["hit", 16]] + W14),
    "closed":      ("closed", 1, 64, BASE + [["rng", 16]]),
}
PRB = {"wide": (104, BASE + WIDE_TAIL + [["delta_L", 16]]), "het": (120, BASE + WIDE_TAIL + [["hit", 16], ["delta_L", 16]])}
# (has_het, mis) -> bytes allocated per record and queue, streams
WORKSPACE = {(0, 0): (104, BASE + WS), (1, 0): (120, BASE + WS + [["hit", 16]]), (0, 1): (184, BASE + WS + [["hit", 16]] + W14)}
# kernel selector -> (value, layout): include/liverrt.h and device_types.h; the layouts are what CELLS implies (path / volpath 88 | 80, biovolpath* 96 | 88,
# volpath-het 104, volpathmis[-plain] 168, the closed volpath instance 64; prbvolpath queues the wide record beside its delta_L stream)
SELECTORS = {
    "LRT_INTEGRATOR_PATH": (0, "wide"), "LRT_INTEGRATOR_VOLPATH": (1, "wide"), "LRT_INTEGRATOR_PRBVOLPATH": (2, "wide"),
    "LRT_INTEGRATOR_BIOVOLPATH": (3, "bio"), "LRT_INTEGRATOR_BIOVOLPATH06": (4, "bio"), "LRT_INTEGRATOR_VOLPATHMIS": (5, "mis"),
    "LRT_INTEGRATOR_VOLPATH_HET": (101, "het"), "LRT_INTEGRATOR_VOLPATHMIS_PLAIN": (102, "mis"), "LRT_INTEGRATOR_VOLPATH_CLOSED": (103, "closed"),
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("record_layout") / "record_layout_main")
    cc = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                         "-I", CSRC, "-w", os.path.join(ROOT, "tests", "host", "record_layout_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    return [json.loads(l) for l in run.stdout.splitlines()]


def test_forms_that_exist_and_their_bytes(lines):
    forms = {l["name"]: (l["layout"], l["compact"], l["bytes"], l["streams"]) for l in lines if l["case"] == "form"}
    assert forms == FORMS
    for name, (_, _, nbytes, streams) in forms.items():
        assert nbytes == sum(b for _, b in streams), name


def test_compact_het_and_compact_mis_do_not_exist(lines):
    combos = [(l["layout"], l["compact"]) for l in lines if l["case"] == "form"]
    assert len(combos) == len(set(combos)) == 7
    assert ("het", 1) not in combos and ("mis", 1) not in combos and ("closed", 0) not in combos


def test_prb_records(lines):
    assert {l["layout"]: (l["bytes"], l["streams"]) for l in lines if l["case"] == "prb"} == PRB


def test_workspace_bytes_per_record_and_queue(lines):
    ws = {(l["has_het"], l["mis"]): (l["bytes"], l["streams"]) for l in lines if l["case"] == "workspace"}
    assert ws == WORKSPACE
    for key, (nbytes, streams) in ws.items():
        assert nbytes == sum(b for _, b in streams), key


def test_selector_to_layout(lines):
    assert {l["name"]: (l["value"], l["layout"]) for l in lines if l["case"] == "selector"} == SELECTORS
