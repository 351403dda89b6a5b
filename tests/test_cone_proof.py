"""The per-face cone table (liverrenderer_amd/csrc/scene_prep.cpp: build_cone_table) without a GPU:
tests/host/cone_proof_main.cpp is compiled with the preparation unit under AddressSanitizer and UBSan, run once, and its JSON lines are
checked here.  Only that program is sanitized; nothing of it is loaded into Python.

Soundness: on the liver and on small adversarial meshes (a strip folded by 20, 45 and 80 degrees towards the tested side, two sheets 0.01
apart, nested boxes with and without flipped normals, degenerate triangles, a single triangle) no segment of a row's full length, spawned
as the device spawns it, may meet a triangle: at least 200 segments per non-zero row, float64 Moller-Trumbore with inclusive comparisons.
Usefulness: an all-zero table is sound too, so on 40 000 segments refracted into the liver the table (with the two-ball cover for the
rest) must prove at least half of what a sampled, unsound estimate of the free lengths proves, for sigma_t = 0.5, 1 and 2."""
import json
import os
import subprocess

import pytest

from conftest import LIVER_XML, ROOT

CSRC = os.path.join(ROOT, "liverrenderer_amd", "csrc")
MESHES = ("fold20", "fold45", "fold80", "thin_shell", "nested_boxes", "nested_boxes_flipped", "zero_area", "single_triangle", "liver")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cone_proof")
    exe = str(tmp / "cone_proof_main")
    flags = ["-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-w"]
    # the program and the unit under test are optimised (millions of segments); the loader behind them is not, which keeps the compile short
    units = (("bvh.cpp", "-O0"), ("loader.cpp", "-O0"), ("xml.cpp", "-O0"), ("image_io.cpp", "-O0"), ("scene_prep.cpp", "-O2"))
    objs = [str(tmp / (f + ".o")) for f, _ in units]
    procs = [subprocess.Popen(["g++", *flags, opt, "-c", os.path.join(CSRC, f), "-o", o], stderr=subprocess.PIPE, text=True) for (f, opt), o in zip(units, objs)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-4000:]
    cc = subprocess.run(["g++", *flags, "-O2", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "host", "cone_proof_main.cpp"), *objs, "-lz", "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, os.path.dirname(LIVER_XML)], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    out = [json.loads(l) for l in run.stdout.splitlines()]
    for l in out:
        print(l)
    return out


def one(lines, case, **kw):
    out = [l for l in lines if l["case"] == case and all(l.get(k) == v for k, v in kw.items())]
    assert len(out) == 1, (case, kw)
    return out[0]


@pytest.mark.parametrize("mesh", MESHES)
def test_no_segment_of_a_rows_length_meets_a_triangle(lines, mesh):
    l = one(lines, "soundness", mesh=mesh)
    assert l["rows"] == 8 * l["faces"] and l["table_bytes"] == 16 * l["faces"]
    assert l["hits"] == 0, l
    if l["nonzero_rows"]:
        assert l["min_segments_per_row"] >= 200 and l["segments"] >= 200 * l["nonzero_rows"]


def test_the_adversarial_meshes_get_the_rows_their_geometry_allows(lines):
    """the construction's decisions, where they can be read off the mesh"""
    s = {m: one(lines, "soundness", mesh=m) for m in MESHES}
    assert s["zero_area"]["nonzero_rows"] == 0                      # every face is degenerate or touches a degenerate one
    assert s["single_triangle"]["nonzero_rows"] == 8                # nothing to meet: every row at the cap, an eighth of the extent (1 / 8)
    assert s["single_triangle"]["r_max"] == 0.125
    # two sheets 0.01 apart: no row of a face under the other sheet may pass it (the sheets overlap only partly, so some rows are longer)
    assert s["thin_shell"]["nonzero_rows"] > 0
    # a fold of 20 degrees stays outside every cone (70 degrees from the normal against at most 60): only rows cut by the 1e-3 widening may go;
    # at 80 degrees the wall stands inside every cone of the faces next to it (10 degrees from the normal)
    assert s["fold20"]["nonzero_rows"] > s["fold45"]["nonzero_rows"] > s["fold80"]["nonzero_rows"] > 0
    # inside a box every face borders a wall at 90 degrees: no inward row; the outward rows of the outer box are free, flipped normals swap the sides only
    assert s["nested_boxes"]["nonzero_rows"] == s["nested_boxes_flipped"]["nonzero_rows"] == 96
    assert s["liver"]["faces"] == 2400 and s["liver"]["table_bytes"] == 38400 and s["liver"]["nonzero_rows"] > 2400


@pytest.mark.parametrize("sigma_t", [0.5, 1.0, 2.0])
def test_the_table_proves_at_least_half_of_what_a_sampled_estimate_does(lines, sigma_t):
    l = one(lines, "usefulness", sigma_t=sigma_t)
    assert l["segments"] == 40000 and l["wrong_claims_conservative"] == 0
    assert l["conservative_with_balls"] >= 0.5 * l["sampled_with_balls"], l
    assert l["conservative_with_balls"] >= 0.5 * l["sampled_alone"], l
    assert l["conservative_alone"] >= 0.5 * l["sampled_alone"], l   # and the table alone against the estimate alone
