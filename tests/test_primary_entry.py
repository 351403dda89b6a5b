"""The per-pixel primary entry (liverrenderer_amd/csrc/scene_prep.cpp: build_primary_entry) without a GPU:
tests/host/primary_entry_main.cpp is compiled with the preparation unit under AddressSanitizer and UBSan, run once, and its JSON lines are
checked here.  Only that program is sanitized; nothing of it is loaded into Python.

Soundness: 25 camera rays per pixel (the four corners, the four edge midpoints, the centre, jitter 0, the largest float below 1, 14 random
positions), generated in float32 as camera_ray generates them and tested with test_tri_lds's arithmetic and tie rule: the closest hit over all
triangles must equal the closest hit over the triangles under the pixel's entry, face and bits of t, u, v; zero differences.  Scenes: the liver
with the C3 camera at 160 x 90, the liver at 1920 x 1080 through a 64 x 64 crop window on the silhouette, folded strips, nested boxes, a thin
shell, a degenerate mesh, a single triangle, a mesh that crosses the near plane, a camera inside a closed box.  A seeded mistake (no dilation,
the depth margin reversed) has to show up.
Usefulness: an all-root table is sound too, so on the liver at 1920 x 1080 the table must remove at least half of the node steps of a camera
ray's traversal and mark at least 45 % of the pixels "none" (52.8 % of them are background)."""
import json
import os
import subprocess

import pytest

from conftest import LIVER_XML, ROOT

CSRC = os.path.join(ROOT, "liverrenderer_amd", "csrc")
SCENES = ("liver_160x90", "liver_1080p_crop", "folded_strips", "nested_boxes", "thin_shell", "degenerate", "single_triangle", "near_plane", "inside_box")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("primary_entry")
    exe = str(tmp / "primary_entry_main")
    flags = ["-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-w"]
    # the program and the unit under test are optimised (a million rays); the loader behind them is not, which keeps the compile short
    units = (("bvh.cpp", "-O0"), ("loader.cpp", "-O0"), ("xml.cpp", "-O0"), ("image_io.cpp", "-O0"), ("scene_prep.cpp", "-O2"))
    objs = [str(tmp / (f + ".o")) for f, _ in units]
    procs = [subprocess.Popen(["g++", *flags, opt, "-c", os.path.join(CSRC, f), "-o", o], stderr=subprocess.PIPE, text=True) for (f, opt), o in zip(units, objs)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-4000:]
    cc = subprocess.run(["g++", *flags, "-O2", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "host", "primary_entry_main.cpp"), *objs, "-lz", "-o", exe], capture_output=True, text=True)
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


@pytest.mark.parametrize("scene", SCENES)
def test_the_closest_hit_under_the_entry_is_the_closest_hit_of_the_scene(lines, scene):
    l = one(lines, "soundness", scene=scene)
    assert l["valid"] and l["rays"] == 25 * l["width"] * l["height"] and l["hits"] > 0
    assert l["none"] + l["leaf"] + l["node"] + l["root"] == l["width"] * l["height"]
    assert l["differences"] == 0, l


def test_the_scenes_get_the_entries_their_geometry_allows(lines):
    """the construction's decisions, where they can be read off the scene"""
    s = {m: one(lines, "soundness", scene=m) for m in SCENES}
    assert not s["single_triangle"]["table"] and s["single_triangle"]["root"] == 48 * 48      # a root leaf: no table, every ray starts where it always did
    for m in SCENES:
        if m != "single_triangle":
            assert s[m]["table"], m
    # a mesh with triangles in front of the near plane, or around the camera: those are candidates of every pixel, so nothing is "none" or a single leaf
    for m in ("near_plane", "inside_box"):
        assert s[m]["none"] == 0 and s[m]["leaf"] == 0, s[m]
    assert s["inside_box"]["node"] == 0                                  # the twelve faces of the outer box lie in both halves of the tree
    # seen from outside: background pixels are "none", and most covered pixels see one leaf
    for m in ("folded_strips", "nested_boxes", "thin_shell", "degenerate"):
        assert s[m]["none"] > 0 and s[m]["leaf"] > s[m]["node"] + s[m]["root"], s[m]
    # at 160 x 90 a pixel of the liver is larger than a triangle: most covered pixels see several leaves
    assert s["liver_160x90"]["none"] > 0 and s["liver_160x90"]["node"] > s["liver_160x90"]["leaf"] > 0, s["liver_160x90"]
    c = s["liver_1080p_crop"]
    assert (c["crop_x"], c["crop_y"], c["width"], c["height"]) == (1168, 90, 64, 64)
    assert c["none"] > 400 and c["leaf"] > 400 and 0 < c["hits"] < c["rays"]       # the window lies on the silhouette
    assert s["liver_160x90"]["faces"] == 2400


def test_a_seeded_mistake_is_found(lines):
    seeded = [l for l in lines if l["case"] == "seeded"]
    assert len(seeded) == 2 and all(l["valid"] for l in seeded)
    assert sum(l["differences"] for l in seeded) > 0, seeded


def test_the_table_removes_most_of_a_camera_rays_traversal(lines):
    l = one(lines, "usefulness")
    print(l)
    assert l["rays"] == 4 * 480 * 270 and l["differences"] == 0 and l["table_bytes"] == 2 * 1920 * 1080
    assert l["nodes"] == 1009 and l["depth"] == 14
    assert l["node_steps_entry"] <= 0.5 * l["node_steps_root"], l          # the gate of DESIGN.md section 6f
    assert l["none"] >= 0.45, l
    assert abs(l["none"] + l["leaf"] + l["node"] + l["root"] - 1.0) < 1e-5
