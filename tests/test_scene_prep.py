"""The host-only scene preparation (liverrenderer_amd/csrc/scene_prep.cpp) without a GPU: tests/host/scene_prep_main.cpp is compiled
with the preparation unit and the host sources it needs under AddressSanitizer and UBSan, run once, and its JSON lines are checked
here.  A sanitizer report fails the run (halt_on_error, a non-zero exit status).  Only that program is sanitized; nothing of it is
loaded into Python.

The leaf-size search: a 64-triangle quad grid never gets leaves of 3 from the builder (its SAH cuts fall between quads, so the
subtrees hold 64, 32, ... 2 triangles and the trees for leaf sizes 2 and 3 are the same tree).  "2 does not fit, 3 does" is
therefore checked on a row of 96 separate triangles (96, 48, ... 6, 3), and the grid checks the same property where its sizes do
differ (2 and 3 do not fit, 4 does)."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "liverrenderer_amd", "csrc")
LEAVES = (2, 3, 4, 6, 8, 12, 16)
RAY_EPS = np.float32(2.0 ** -24) * np.float32(1500)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_prep") / "scene_prep_main")
    src = [os.path.join(ROOT, "tests", "host", "scene_prep_main.cpp")] + [os.path.join(CSRC, f) for f in ("scene_prep.cpp", "bvh.cpp", "loader.cpp", "xml.cpp", "image_io.cpp")]
    cc = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                         "-I", CSRC, "-w", *src, "-lz", "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    return [json.loads(l) for l in run.stdout.splitlines()]


def sel(lines, case, **kw):
    out = [l for l in lines if l["case"] == case and all(l.get(k) == v for k, v in kw.items())]
    assert out, (case, kw)
    return out


def one(lines, case, **kw):
    out = sel(lines, case, **kw)
    assert len(out) == 1, (case, kw)
    return out[0]


def f32(x):
    with np.errstate(over="ignore"):                     # 1e39 stands for inf in the program's JSON
        return np.asarray(x, np.float64).astype(np.float32)


# ---- the LDS image
def decode_image(l):
    """Checks the layout of one LDS image and returns (faces per slot, last-slot bits)."""
    blob = np.frombuffer(bytes.fromhex(l["blob"]), np.uint8)
    n_nodes, n_slots = l["n_nodes"], l["n_slots"]
    assert len(blob) == l["blob_bytes"] == l["stack_off"] and l["nodes_off"] == 0 and l["verts_off"] == 64 * n_nodes
    assert l["tris_off"] % 16 == 0 and l["blob_bytes"] % 16 == 0 and l["blob_bytes"] - l["tris_off"] == (8 * n_slots + 15) // 16 * 16
    assert l["total_bytes"] == l["image_bytes"] > l["blob_bytes"] and (l["total_bytes"] - l["blob_bytes"]) % 2048 == 0      # 16-bit stacks of 1024 lanes
    slots = blob[l["tris_off"]:l["tris_off"] + 8 * n_slots].view(np.uint16).reshape(n_slots, 4)
    face, last = slots[:, 3] >> 1, slots[:, 3] & 1
    assert sorted(face.tolist()) == list(range(l["n_faces"]))                                # every face in exactly one slot
    nodes = blob[:64 * n_nodes].reshape(n_nodes, 64)
    refs = nodes[:, 48:56].copy().view(np.uint32).reshape(n_nodes, 2); counts = nodes[:, 56:64].copy().view(np.int32).reshape(n_nodes, 2)
    leaf_last = np.zeros(n_slots, np.int64); covered = np.zeros(n_slots, np.int64); seen_inner = np.zeros(n_nodes, np.int64)
    if l["root_is_leaf"]:
        first, count = l["root_leaf_first"], l["root_leaf_count"]
        covered[first:first + count] += 1; leaf_last[first + count - 1] = 1
    else:
        for n in range(n_nodes):
            for c in range(2):
                r, k = int(refs[n, c]), int(counts[n, c])
                if r & 0x8000:                                                               # a leaf: 0x8000 | its first slot
                    first = r & 0x7fff
                    assert r < 0x10000 and k > 0 and first + k <= n_slots
                    covered[first:first + k] += 1; leaf_last[first + k - 1] += 1
                else:                                                                        # an inner node, never the root, named once
                    assert 0 < r < n_nodes and k == 0
                    seen_inner[r] += 1
        assert (seen_inner[1:] == 1).all() and seen_inner[0] == 0
    assert (covered == 1).all()                                                              # the leaves partition the slots
    assert (last == leaf_last).all()                                                         # bit 0 on every leaf's last slot and on no other
    return face, last


def test_one_triangle(lines):
    l = one(lines, "triangle")
    assert l["root_is_leaf"] == 1 and l["root_leaf_first"] == 0 and l["root_leaf_count"] == 1 and l["use_lds"] == 1 and l["n_slots"] == 1
    face, last = decode_image(l)
    slots = np.frombuffer(bytes.fromhex(l["blob"]), np.uint8)[l["tris_off"]:l["tris_off"] + 8].view(np.uint16)
    assert slots.tolist() == [0, 1, 2, 0 << 1 | 1]


@pytest.mark.parametrize("mesh,faces", [("grid", 64), ("row", 96)])
def test_leaf_size_search(lines, mesh, faces):
    size = one(lines, "grid_sizes", mesh=mesh, faces=faces)["bytes"]
    runs = {l["run"]: l for l in sel(lines, "grid", mesh=mesh, faces=faces)}
    if mesh == "row":                        # leaf size 2 does not fit and 3 does: 3 must be chosen
        assert size[3] < size[2] and runs["limit_of_leaf3"]["limit"] == size[3]
        assert runs["limit_of_leaf3"]["bvh_leaf"] == 3 and runs["limit_of_leaf3"]["use_lds"] == 1
    else:                                    # the grid's trees for 2 and 3 are one tree (module docstring): neither fits, 4 does
        assert size[2] == size[3] > size[4] and runs["limit_of_leaf4"]["bvh_leaf"] == 4 and runs["limit_of_leaf4"]["use_lds"] == 1
    n_search = 0
    for name, l in runs.items():
        if l["forced"] or l["switch"]:
            continue
        fitting = [leaf for leaf in LEAVES if size[leaf] <= l["limit"]]
        assert l["bvh_leaf"] == (fitting[0] if fitting else 4) and l["use_lds"] == (1 if fitting else 0), name
        n_search += 1
    assert n_search >= 4
    assert runs["nothing"]["bvh_leaf"] == 4 and runs["nothing"]["use_lds"] == 0               # nothing fits: leaf size 4 in global memory
    assert runs["forced8"]["bvh_leaf"] == 8 and runs["forced8"]["use_lds"] == 1 and runs["forced8"]["total_bytes"] == size[8]   # LRT_BVH_LEAF through PrepOptions
    assert runs["forced2_small"]["bvh_leaf"] == 2 and runs["forced2_small"]["use_lds"] == 0   # a forced size is not searched around
    assert runs["switch"]["use_lds"] == 0 and runs["switch"]["bvh_leaf"] == 4                 # LRT_NO_LDS_BVH
    images = [l for l in runs.values() if l["use_lds"]]
    assert len(images) >= 5
    for l in images:
        assert l["total_bytes"] == size[l["bvh_leaf"]] <= l["limit"]
        decode_image(l)


def test_sixteen_bit_limits(lines):
    got = {(l["n_faces"], l["n_vertices"]): l["use_lds"] for l in sel(lines, "limits16")}
    assert got == {(32767, 16641): 1, (32768, 16641): 0, (64, 65535): 1, (64, 65536): 0}


def test_sphere_record(lines):
    l = one(lines, "sphere")
    M = f32(l["to_world"]).astype(np.float64).reshape(4, 4)
    assert (f32(l["center"]) == f32(M[:3, 3])).all() and (f32(l["lin"]) == f32(M[:3, :3].ravel())).all() and l["n_spheres"] == 1 and l["shape"] == 0 and l["ext"] == 1
    # the radius comes from the first column: three products and two additions and a root in float32
    r = np.sqrt((M[:3, 0] ** 2).sum())
    assert abs(l["radius"] - r) <= 4 * 2.0 ** -24 * r and abs(r - 0.37) < 1e-6
    # to_object * to_world = identity: each entry of the float64 inverse was rounded once (2^-24 relative)
    inv = np.asarray(l["to_object"], np.float64).reshape(3, 4)
    prod = np.hstack([inv[:, :3] @ M[:3, :3], (inv[:, :3] @ M[:3, 3] + inv[:, 3])[:, None]])
    bound = 2.0 ** -24 * np.hstack([np.abs(inv[:, :3]) @ np.abs(M[:3, :3]), (np.abs(inv[:, :3]) @ np.abs(M[:3, 3]) + np.abs(inv[:, 3]))[:, None]]) + 1e-15
    assert (np.abs(prod - np.eye(3, 4)) <= bound).all(), np.abs(prod - np.eye(3, 4)).max()
    assert one(lines, "sphere_zero")["error"] == "sphere with a zero or invalid radius"


def test_bounds(lines):
    empty, cube, far = (one(lines, "bounds", run=r) for r in ("empty", "cube", "cube_far_vertex"))
    assert np.float32(empty["bsphere_r"]) == RAY_EPS and empty["bsphere_c"] == [0, 0, 0] and empty["grid_enabled"] == 0
    # unit cube: centre (.5, .5, .5), radius sqrt(3) / 2 widened by (1 + ray_eps); 0.75 is exact in float32, the root and the product round once each
    assert cube["bsphere_c"] == [0.5, 0.5, 0.5]
    assert np.float32(cube["bsphere_r"]) == np.sqrt(np.float32(0.75)) * (np.float32(1) + RAY_EPS)
    # one far vertex that no face references: the bounding sphere follows it, the distance field's box does not
    assert far["bsphere_c"] == [5.0, 0.5, 0.5] and far["bsphere_r"] > 5.0
    for k in ("grid_enabled", "grid_lo", "grid_cell", "grid_n", "abs_margin"):
        assert far[k] == cube[k], k
    assert cube["grid_enabled"] == 1 and cube["grid_lo"] == [0, 0, 0] and cube["grid_n"] == [192, 192, 192] and np.float32(cube["grid_cell"]) == np.float32(1) / np.float32(192)


# ---- the environment map
def swizzle(x, y, width):
    return ((x & 1) | (((x & ~1) | (y & 1)) << 1)) + ((y & ~1) * width)


@pytest.mark.parametrize("run", ["2x3", "2x3_zero_interior", "2x3_zero_border", "5x4"])
def test_envmap_table_and_hierarchy(lines, run):
    from envmap_ref import EnvmapRef
    l = one(lines, "envmap", run=run)
    W, h = l["w"], l["h"]; w = W - 1                                                         # (w + 1) x h storage
    tex = f32(l["texels"]).reshape(h, w, 3)
    data = f32(l["env_data"]).reshape(h, W, 4)
    assert (data[:, :w, :3] == tex).all() and (data[:, w, :3] == tex[:, 0]).all() and (data[..., 3] == 0).all()      # the wrapped column
    ref = EnvmapRef(tex)
    hier = np.asarray(l["hier"], np.float64); off, width = l["level_offset"], l["level_width"]
    n_patches = w * (h - 1)
    assert l["n_levels"] == ref.n_levels + 2 and off[0] == 0 and width[0] == W and all(o % 4 == 0 for o in off[:l["n_levels"]])
    assert l["max_patch"] == [w - 1, h - 2] and np.float32(l["patch_size"][0]) == np.float32(1) / np.float32(w)
    # float32 against float64: a node is 5 operations, sin and its argument (the luminance, sin(theta), the scale), level k adds 3 additions per level
    tol = lambda k: (16 + 3 * k) * 2.0 ** -24
    # level 0: the nodes, luminance * sin(theta) rows, normalised (envmap_ref's D)
    l0 = hier[:W * h].reshape(h, W)
    assert np.abs(l0 - ref.D).max() <= tol(0) * ref.D.max()
    sin_rows = np.sin(np.pi * np.arange(h) / (h - 1))
    assert (l0[0] == 0).all() and np.abs(l0[-1]).max() <= 2.0 ** -22 * ref.lum_n.max()      # sin(0) = 0; sin(float32 pi) is not
    assert np.abs(l0[1:-1] - ref.lum_n[1:-1] * sin_rows[1:-1, None]).max() <= tol(0) * ref.D.max()
    # level 1 and above: the probabilities of the patches and of their dyadic blocks, times the number of patches
    for k in range(1, l["n_levels"]):
        c = 1 << (k - 1)
        nx, ny = -(-w // c), -(-(h - 1) // c)
        for y in range(ny):
            for x in range(nx):
                want = ref._block(x * c, (x + 1) * c, y * c, (y + 1) * c) * n_patches
                got = hier[off[k] + swizzle(x, y, width[k])]
                assert abs(got - want) <= tol(k) * max(want, ref.P.max() * n_patches), (k, x, y)
    top = hier[off[l["n_levels"] - 1]:off[l["n_levels"] - 1] + 4].sum()
    assert abs(top - n_patches) <= tol(l["n_levels"]) * n_patches
    interior = bool((tex[1:-1].astype(np.float64) @ np.array([0.212671, 0.715160, 0.072169]) > 0).all())
    assert l["interior_positive"] == int(interior) == (0 if run == "2x3_zero_interior" else 1)
    assert l["nee_fast_reject"] == int(interior)


def test_nee_fast_reject_conditions(lines):
    got = {l["run"]: l["value"] for l in sel(lines, "nee_fast_reject")}
    assert got == {"base_envmap": 1, "base_constant": 1, "two_emitters": 0, "null_bsdf": 0, "het_medium": 0, "switch": 0, "interior_not_positive": 0, "point_only": 0}


def test_nee_vmin_never_below_what_it_rounds(lines):
    import math
    n_two = n_margin = 0
    for l in sel(lines, "nee_vmin"):
        assert l["sizes"] == [len(l["sigma_t"])] * 3
        st, vmin = f32(l["sigma_t"]), f32(l["nee_vmin"])
        assert (st == f32(l["medium_sigma_t"])).all()                                         # DMedium::sigma_t is the helper's product
        bound = np.float32(np.float32(2) * np.float32(l["bsphere_r"])) * np.float32(0.998) - np.float32(1e-3)
        for s, v in zip(st, vmin):
            x = float(s) * float(bound)
            if x > 0.05 and math.isfinite(x):
                want = math.exp(-x * (1.0 - 1e-4)) * (1.0 + 1e-4)
                assert float(v) >= want and float(np.nextafter(v, np.float32(-1))) < want     # the float32 at or just above it
                n_margin += 1
            else:
                assert v == 2                                                                # sigma_t * bound <= 0.05 (or not finite): never rejects
                n_two += 1
    assert n_two >= 20 and n_margin >= 20


def test_resolve(lines):
    r = {l["run"]: l for l in sel(lines, "resolve")}
    assert [r[k]["spp"] for k in ("ld1", "ld5", "ld17")] == [4, 16, 64] and all(r[k]["n_passes"] == 1 for k in ("ld1", "ld5", "ld17"))
    assert r["not_a_multiple"]["error"] == "sample_count (10) must be a multiple of spp_per_pass (4)."
    assert (r["three_passes"]["spp"], r["three_passes"]["n_passes"], r["three_passes"]["spp_total"]) == (4, 3, 12)
    # 65536 x 32768 pixels at 4 spp: one pass of 4 would be 2^33 lanes; passes of one sample are 2^31 lanes each
    wf = r["wavefront_2e33"]
    assert (wf["spp"], wf["n_passes"], wf["spp_total"]) == (1, 4, 4) and 65536 * 32768 * wf["spp"] <= 2 ** 32 - 1
    assert r["film_2e32"]["error"] == "film too large: a single sample per pixel exceeds 2^32 lanes"
    assert r["depth-1"]["max_depth"] == r["depth70000"]["max_depth"] == r["depth65535"]["max_depth"] == r["opts_depth-1"]["max_depth"] == 65535 and r["depth12"]["max_depth"] == 12
    assert (r["prb"]["integrator"], r["prb"]["spp"], r["prb"]["n_passes"], r["prb"]["spp_total"]) == (2, 12, 1, 12)      # prbvolpath: a single pass, whatever samples_per_pass says
    assert r["rank_out_of_range"]["error"] == "tile_rank must be smaller than tile_count"
    assert (r["rank1of2"]["tile_rank"], r["rank1of2"]["tile_count"]) == (1, 2)


def owner_map(w, h, count):
    y, x = np.mgrid[0:h, 0:w]
    return ((y // 32) * ((w + 31) // 32) + x // 32) % count


@pytest.mark.parametrize("w,h,count", [(33, 5, 2), (9, 5, 2), (70, 37, 3)])
def test_tile_lists(lines, w, h, count):
    ranks = sorted(sel(lines, "tiles", w=w, h=h, count=count), key=lambda l: l["rank"])
    assert [l["rank"] for l in ranks] == list(range(count))
    owner = owner_map(w, h, count)
    assert sorted(p for l in ranks for p in l["list"]) == list(range(w * h))                  # the lists partition the film
    for l in ranks:
        own = owner.ravel() == l["rank"]
        assert sorted(l["list"]) == np.flatnonzero(own).tolist() and len(l["slot"]) == w * h
        assert all(l["slot"][p] == k for k, p in enumerate(l["list"]))                       # the inverse
        assert all(s == 0 for p, s in enumerate(l["slot"]) if not own[p])
        # tile order, rows inside a tile
        key = [((p // w) // 32 * ((w + 31) // 32) + (p % w) // 32, p) for p in l["list"]]
        assert key == sorted(key)
        for halo in (0, 2, 40):                                                              # brute-force dilation by a (2 halo + 1)^2 box
            m = own.reshape(h, w); big = np.zeros((h + 2 * halo, w + 2 * halo), bool)
            ys, xs = np.nonzero(m)
            for y, x in zip(ys, xs):
                big[y:y + 2 * halo + 1, x:x + 2 * halo + 1] = True
            want = np.flatnonzero(big[halo:halo + h, halo:halo + w].ravel()).tolist()
            assert l["halo%d" % halo] == want, halo
    if (w, h) == (9, 5):
        assert ranks[1]["list"] == [] and ranks[1]["halo40"] == []                            # one tile, two ranks: rank 1 owns nothing


def test_closed_records_predicate(lines):
    got = {l["run"]: l["value"] for l in sel(lines, "closed_records")}
    assert got.pop("base") == 1 and got.pop("base_envmap") == 1
    assert sorted(got) == sorted(["a_heterogeneous", "a_sigma_t_zero", "a_sigma_t_times_scale_small", "a_sigma_t_infinite", "a_sensor_in_medium", "a_exterior_medium",
                                  "b_diffuse", "b_null", "b_no_bsdf", "b_bumpmap_over_diffuse", "b_bumpmap_nested_out_of_range",
                                  "c_area_emitter", "c_point_emitter", "c_two_emitters", "c_no_emitter"])
    assert all(v == 0 for v in got.values()), got


def test_prep_options_from_env(lines):
    """the five switches, read once: LRT_BVH_LEAF is at least 1 once set, LRT_DIST_GRID_RES is held to 8 .. 256, the three flags count as set whatever their value"""
    got = {l["run"]: (l["bvh_leaf"], l["no_lds_bvh"], l["no_dist_grid"], l["dist_grid_res"], l["no_nee_reject"]) for l in sel(lines, "from_env")}
    assert got == {"unset": (0, 0, 0, 0, 0), "leaf6_res100": (6, 0, 0, 100, 0), "leaf0_res4": (1, 0, 0, 8, 0), "leaf_negative_res1000": (1, 0, 0, 256, 0),
                   "leaf_text_res_text": (1, 0, 0, 8, 0), "flags": (0, 1, 1, 0, 1), "flags_zero_and_empty": (0, 1, 1, 0, 1)}
    assert all(l["lds_limit"] == 0 and l["n_cus"] == 256 for l in sel(lines, "from_env"))      # the device's figures are the upload side's to set
