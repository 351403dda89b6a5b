"""The conductor, plastic and twosided BSDFs on the host: what the loader and lrt_scene_from_desc read and
refuse, the description's new fields, the dictionary route, the host constants and the routing of the scene preparation (through the
stand-alone program tests/host/smooth_main.cpp, compiled under AddressSanitizer and UBSan; nothing of it is loaded into Python), and
the float64 reference of tests/smooth_ref.py held against itself: the K of every tolerance, the share of lanes left out, the
identities of the followed renderer's test_twosided.py, and seeded mistakes that the checks of test_smooth_gpu.py must catch."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import smooth_cases as sc
import smooth_ref as sr
from conftest import ROOT

CONDUCTOR, PLASTIC, TWOSIDED = 5, 6, 7
CSRC = os.path.join(ROOT, "liverrenderer_amd", "csrc")


def scene(mi, bsdf, integrator='<integrator type="path"/>'):
    return mi.load_string(sc.HEAD.format(integrator=integrator) + f'<shape type="rectangle">{bsdf}</shape></scene>')


def of_type(s, t):
    d = s.desc
    return [d.bsdfs[i] for i in range(d.n_bsdfs) if d.bsdfs[i].type == t]


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_version_and_struct_sizes(mi):
    from liverrenderer_amd import _lib
    assert _lib.lib().lrt_version() >= 119
    names = [f for f, _ in _lib.BsdfDesc._fields_]
    assert names[-9:] == ["eta_r", "eta_g", "eta_b", "k_r", "k_g", "k_b", "diffuse_reflectance", "nonlinear", "nested_back"]      # grown at its end only (eta_rgb[3], k_rgb[3])
    assert names[:12] == ["type", "reflectance", "eta", "nested", "texture", "scale", "alpha_u", "alpha_v", "distribution", "sample_visible", "specular_reflectance", "specular_transmittance"]
    assert C.sizeof(_lib.BsdfDesc) == 48 + 24 + 12 and _lib.BsdfDesc.eta_r.offset == 48 and _lib.BsdfDesc.k_r.offset == 60 and _lib.BsdfDesc.nested_back.offset == 80
    for t in ("conductor", "plastic", "twosided"):
        assert mi._TAGS[t] == "bsdf"
    with open(os.path.join(ROOT, "include", "liverrt.h")) as f:
        h = f.read()
    assert "LRT_BSDF_CONDUCTOR = 5, LRT_BSDF_PLASTIC = 6, LRT_BSDF_TWOSIDED = 7" in h and "float   eta_rgb[3], k_rgb[3];" in h


# ------------------------------------------------------------------------------------------------------------- the loader
def test_conductor_defaults_and_properties(mi):
    (B,) = of_type(scene(mi, '<bsdf type="conductor"/>'), CONDUCTOR)
    assert list(B.eta_rgb) == [0, 0, 0] and list(B.k_rgb) == [1, 1, 1]                                         # material = none: a mirror
    s = scene(mi, '<bsdf type="conductor"><string name="material" value="none"/><float name="eta" value="1.5"/><rgb name="k" value="3, 2, 1"/>'
                  '<texture name="specular_reflectance" type="checkerboard"/></bsdf>')
    (B,) = of_type(s, CONDUCTOR)
    assert list(B.eta_rgb) == [1.5] * 3 and list(B.k_rgb) == [3, 2, 1] and s.desc.textures[B.specular_reflectance].type == 1


def test_plastic_defaults_and_properties(mi):
    s = scene(mi, '<bsdf type="plastic"/>')
    (B,) = of_type(s, PLASTIC)
    assert B.eta == np.float32(1.49) / np.float32(1.000277) and B.nonlinear == 0 and B.specular_reflectance == -1          # polypropylene / air
    assert list(s.desc.textures[B.diffuse_reflectance].color0) == [0.5] * 3
    s = scene(mi, '<bsdf type="plastic"><string name="int_ior" value="water"/><float name="ext_ior" value="1.1"/><boolean name="nonlinear" value="true"/>'
                  '<rgb name="diffuse_reflectance" value="0.1, 0.2, 0.3"/><rgb name="specular_reflectance" value="0.5"/></bsdf>')
    (B,) = of_type(s, PLASTIC)
    assert B.eta == np.float32(1.3330) / np.float32(1.1) and B.nonlinear == 1
    assert np.allclose(list(s.desc.textures[B.diffuse_reflectance].color0), [0.1, 0.2, 0.3]) and list(s.desc.textures[B.specular_reflectance].color0) == [0.5] * 3


def test_twosided_children(mi):
    s = scene(mi, '<bsdf type="twosided"><bsdf type="diffuse"/></bsdf>')
    (B,) = of_type(s, TWOSIDED)
    assert s.desc.bsdfs[B.nested].type == 0 and B.nested_back == B.nested and s.desc.bsdfs[s.desc.shapes[0].bsdf].type == TWOSIDED
    s = scene(mi, '<bsdf type="twosided"><bsdf type="plastic"/><bsdf type="conductor"/></bsdf>')
    (B,) = of_type(s, TWOSIDED)
    assert s.desc.bsdfs[B.nested].type == PLASTIC and s.desc.bsdfs[B.nested_back].type == CONDUCTOR
    # the same object twice is one child (twosided.cpp:124 compares the pointers)
    s = mi.load_string(sc.HEAD.format(integrator='<integrator type="path"/>') + '<bsdf type="diffuse" id="d"/><shape type="rectangle"><bsdf type="twosided"><ref id="d"/><ref id="d"/></bsdf></shape></scene>')
    (B,) = of_type(s, TWOSIDED)
    assert B.nested_back == B.nested


BUMP = '<bsdf type="bumpmap"><texture name="arbitrary" type="checkerboard"/>{}</bsdf>'
LOADER_ERRORS = [            # body, message, status (1: LRT_ERR_INVALID, 4: LRT_ERR_UNSUPPORTED)
    ('<bsdf type="conductor"><string name="material" value="Cu"/></bsdf>', 'unsupported: conductor material "Cu"', 4),
    ('<bsdf type="conductor"><string name="material" value="Au"/><float name="eta" value="1.5"/></bsdf>', r"Should specify either \(eta, k\) or material, not both\.", 1),
    ('<bsdf type="conductor"><texture name="eta" type="checkerboard"/></bsdf>', 'unsupported: a texture as conductor "eta"', 4),
    ('<bsdf type="conductor"><texture name="k" type="checkerboard"/></bsdf>', 'unsupported: a texture as conductor "k"', 4),
    ('<bsdf type="conductor"><rgb name="eta" value="0.2, 0, 0.3"/><rgb name="k" value="1, 0, 2"/></bsdf>', "conductor with eta = k = 0 in a channel", 1),
    ('<bsdf type="plastic"><float name="int_ior" value="-1.5"/></bsdf>', "The interior and exterior indices of refraction must be positive!", 1),
    ('<bsdf type="plastic"><string name="int_ior" value="kryptonite"/></bsdf>', "unknown material", 1),
    ('<bsdf type="twosided"><bsdf type="dielectric"/></bsdf>', "Only materials without a transmission component can be nested!", 1),
    ('<bsdf type="twosided"><bsdf type="diffuse"/><bsdf type="roughdielectric"/></bsdf>', "Only materials without a transmission component can be nested!", 1),
    ('<bsdf type="twosided"><bsdf type="null"/></bsdf>', "Only materials without a transmission component can be nested!", 1),
    ('<bsdf type="twosided"><boolean name="allow_transmission" value="true"/><bsdf type="dielectric"/></bsdf>', "unsupported: twosided with allow_transmission = true", 4),
    ('<bsdf type="twosided">' + BUMP.format('<bsdf type="diffuse"/>') + '</bsdf>', "unsupported: a bumpmap nested in a twosided BSDF", 4),
    ('<bsdf type="twosided"><bsdf type="twosided"><bsdf type="diffuse"/></bsdf></bsdf>', "unsupported: a twosided nested in a twosided BSDF", 4),
    (BUMP.format('<bsdf type="twosided"><bsdf type="diffuse"/></bsdf>'), "unsupported: a twosided BSDF nested in a bumpmap", 4),
    ('<bsdf type="twosided"><bsdf type="diffuse"/><bsdf type="diffuse"/><bsdf type="diffuse"/></bsdf>', "At most two nested BSDFs can be specified!", 1),
    ('<bsdf type="twosided"/>', "A nested one-sided material is required!", 1),
    ('<bsdf type="roughconductor"/>', 'unsupported bsdf type "roughconductor"', 4),
    ('<bsdf type="roughplastic"/>', 'unsupported bsdf type "roughplastic"', 4),
]


@pytest.mark.parametrize("body, message, status", LOADER_ERRORS, ids=[str(i) for i in range(len(LOADER_ERRORS))])
def test_loader_errors(mi, body, message, status):
    with pytest.raises(RuntimeError, match=message):
        scene(mi, body)
    L = mi._lib.lib(); h = C.c_void_p()
    xml = (sc.HEAD.format(integrator='<integrator type="path"/>') + f'<shape type="rectangle">{body}</shape></scene>').encode()
    assert L.lrt_scene_load_xml_string(xml, b".", None, 0, C.byref(h)) == status


def test_bitmaps_stay_refused(mi, tmp_path):
    png = str(tmp_path / "flat.png"); sc.write_flat_png(png)
    tex = lambda name: f'<texture name="{name}" type="bitmap"><string name="filename" value="{png}"/></texture>'
    for plugin, name in (("conductor", "specular_reflectance"), ("plastic", "diffuse_reflectance"), ("plastic", "specular_reflectance")):
        with pytest.raises(RuntimeError, match=f"unsupported: a bitmap texture as {plugin}"):
            scene(mi, f'<bsdf type="{plugin}">{tex(name)}</bsdf>')


def test_prbvolpath_is_refused(mi):
    message = r"unsupported: prbvolpath on a scene with a conductor / plastic / twosided BSDF \(no adjoint is built for them\)"
    for bsdf in ('<bsdf type="conductor"/>', '<bsdf type="plastic"/>', '<bsdf type="twosided"><bsdf type="diffuse"/></bsdf>', BUMP.format('<bsdf type="plastic"/>')):
        with pytest.raises(RuntimeError, match=message):
            scene(mi, bsdf, integrator='<integrator type="prbvolpath"/>')
    # an unreferenced one changes nothing
    xml = sc.HEAD.format(integrator='<integrator type="prbvolpath"/>') + '<bsdf type="plastic" id="spare"/><shape type="rectangle"><bsdf type="diffuse"/></shape></scene>'
    assert len(of_type(mi.load_string(xml), PLASTIC)) == 1


def test_load_dict_and_xml_give_equal_descriptions(mi):
    T = mi.ScalarTransform4f
    d = {"type": "scene", "integrator": {"type": "volpath", "max_depth": 4},
         "sensor": {"type": "perspective", "fov": 30.0, "to_world": T().look_at([0, 0, 5], [0, 0, 0], [0, 1, 0]), "film": {"type": "hdrfilm", "width": 8, "height": 8}},
         "tool": {"type": "rectangle", "bsdf": {"type": "conductor", "eta": [0.2, 0.9, 1.1], "k": 3.5, "specular_reflectance": {"type": "rgb", "value": [0.9, 0.8, 0.7]}}},
         "drape": {"type": "rectangle", "to_world": T().translate([0.0, 0.0, -1.0]),
                   "bsdf": {"type": "twosided",
                            "front": {"type": "plastic", "int_ior": "water", "ext_ior": 1.0, "nonlinear": True,
                                      "diffuse_reflectance": {"type": "checkerboard", "color0": [0.25, 0.25, 0.25], "color1": [1.0, 0.5, 0.0]}, "specular_reflectance": 0.75},
                            "back": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.1, 0.2, 0.3]}}}},
         "light": {"type": "constant", "radiance": {"type": "rgb", "value": 1.0}}}
    xml = mi.dict_to_xml(d)
    assert '<bsdf type="conductor">' in xml and '<bsdf type="plastic" name="front">' in xml
    a, b = mi.load_dict(d), mi.load_string(xml)
    assert a.desc.n_bsdfs == b.desc.n_bsdfs == 4
    for i in range(a.desc.n_bsdfs):
        for f, t in mi._lib.BsdfDesc._fields_:
            assert getattr(a.desc.bsdfs[i], f) == getattr(b.desc.bsdfs[i], f), (i, f)
    (cd,) = of_type(a, CONDUCTOR); (pl,) = of_type(a, PLASTIC); (ts,) = of_type(a, TWOSIDED)
    assert np.allclose(list(cd.eta_rgb), [0.2, 0.9, 1.1]) and list(cd.k_rgb) == [3.5] * 3
    assert pl.eta == np.float32(1.3330) and pl.nonlinear == 1 and a.desc.textures[pl.diffuse_reflectance].type == 1 and list(a.desc.textures[pl.specular_reflectance].color0) == [0.75] * 3
    assert a.desc.bsdfs[ts.nested].type == PLASTIC and a.desc.bsdfs[ts.nested_back].type == 0


def test_scene_from_desc_validation(mi):
    from liverrenderer_amd import _lib
    base = scene(mi, '<bsdf type="twosided"><bsdf type="plastic"><rgb name="specular_reflectance" value="0.5"/></bsdf><bsdf type="conductor"/></bsdf>')
    extra = scene(mi, '<bsdf type="dielectric"/>')
    L = _lib.lib()
    n = base.desc.n_bsdfs
    assert [base.desc.bsdfs[i].type for i in range(n)] == [PLASTIC, CONDUCTOR, TWOSIDED]

    def attempt(mutate):
        d = _lib.SceneDesc.from_buffer_copy(base.desc)
        bs = (_lib.BsdfDesc * (n + 2))(*[d.bsdfs[i] for i in range(n)], extra.desc.bsdfs[0], d.bsdfs[2])      # [3]: a dielectric, [4]: a second twosided; no shape uses them
        d.bsdfs = C.cast(bs, C.POINTER(_lib.BsdfDesc)); d.n_bsdfs = n + 2
        mutate(bs)
        h = C.c_void_p()
        st = L.lrt_scene_from_desc(C.byref(d), C.byref(h))
        if st == 0:
            L.lrt_scene_free(h)
        return st, L.lrt_last_error().decode()

    assert attempt(lambda b: None)[0] == 0
    assert attempt(lambda b: setattr(b[2], "nested_back", -1))[0] == 0                     # one child serves both sides
    cases = {
        "plastic texture": (lambda b: setattr(b[0], "diffuse_reflectance", 9), 1, "invalid texture"),
        "plastic texture low": (lambda b: setattr(b[0], "specular_reflectance", -2), 1, "invalid texture"),
        "plastic eta": (lambda b: setattr(b[0], "eta", -1.0), 1, "must be positive"),
        "conductor texture": (lambda b: setattr(b[1], "specular_reflectance", -1), 1, "invalid texture"),
        "conductor zero index": (lambda b: (setattr(b[1], "eta_b", 0.0), setattr(b[1], "k_b", 0.0)), 1, "eta = k = 0"),
        "conductor nan": (lambda b: setattr(b[1], "eta_g", float("nan")), 1, "not finite"),
        "no child": (lambda b: setattr(b[2], "nested", -1), 1, "A nested one-sided material is required!"),
        "child index": (lambda b: setattr(b[2], "nested_back", 17), 1, "invalid nested bsdf"),
        "transmissive child": (lambda b: setattr(b[2], "nested_back", 3), 1, "Only materials without a transmission component can be nested!"),
        "twosided child": (lambda b: setattr(b[2], "nested", 4), 4, "unsupported: a twosided nested in a twosided"),
        "type": (lambda b: setattr(b[1], "type", 8), 1, "invalid bsdf type"),
    }
    for name, (fn, status, text) in cases.items():
        st, msg = attempt(fn)
        assert st == status and text in msg, (name, st, msg)


# ------------------------------------------------------------------------------------------------------------- the preparation
HOST_SCENES = {
    "mirror": '<shape type="rectangle"><bsdf type="conductor"/></shape>',
    "metal": '<shape type="rectangle"><bsdf type="conductor"><rgb name="eta" value="0.143, 0.375, 1.442"/><rgb name="k" value="3.983, 2.386, 1.603"/></bsdf></shape>',
    "plastic": '<shape type="rectangle"><bsdf type="plastic"/></shape>',
    "plastic2": ('<shape type="rectangle"><bsdf type="plastic"><float name="int_ior" value="1.9"/><string name="ext_ior" value="water"/><rgb name="diffuse_reflectance" value="0.8, 0.4, 0.1"/>'
                 '<texture name="specular_reflectance" type="checkerboard"><rgb name="color0" value="0.9, 0.6, 0.3"/><rgb name="color1" value="0.2, 0.3, 0.7"/></texture></bsdf></shape>'),
    "plastic_dense": '<shape type="rectangle"><bsdf type="plastic"><float name="int_ior" value="1.0"/><float name="ext_ior" value="1.5"/></bsdf></shape>',
    "twosided": '<shape type="rectangle"><bsdf type="twosided"><bsdf type="diffuse"/><bsdf type="plastic"/></bsdf></shape>',
    "twosided_mirror": '<shape type="rectangle"><bsdf type="twosided"><bsdf type="conductor"/></bsdf></shape>',
    "bump": '<shape type="rectangle">' + BUMP.format('<bsdf type="plastic"/>') + '</shape>',
    "unused": '<bsdf type="plastic" id="a"/><bsdf type="twosided" id="b"><bsdf type="conductor"/></bsdf><shape type="rectangle"><bsdf type="diffuse"/></shape>',
}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("smooth_host")
    exe = str(tmp / "smooth_main")
    src = [os.path.join(ROOT, "tests", "host", "smooth_main.cpp")] + [os.path.join(CSRC, f) for f in ("scene_prep.cpp", "bvh.cpp", "loader.cpp", "xml.cpp", "image_io.cpp")]
    cc = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                         "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-w", *src, "-lz", "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    files = []
    for name, body in HOST_SCENES.items():
        files.append(str(tmp / (name + ".xml")))
        with open(files[-1], "w") as f:
            f.write(sc.HEAD.format(integrator='<integrator type="path"/>') + body + "</scene>")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, *files], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    out = dict(zip(HOST_SCENES, (json.loads(l) for l in run.stdout.splitlines())))
    assert len(out) == len(HOST_SCENES) and not any("error" in v for v in out.values()), out
    return out


def test_rows_flags_and_routing(host):
    assert all(v["row_bytes"] == 64 for v in host.values())                       # rows of four 16-byte words
    for name in HOST_SCENES:
        assert (host[name]["ext"], host[name]["smooth"]) == ((0, 0) if name == "unused" else (1, 1)), name
    assert [b["flags"] for b in host["unused"]["bsdfs"]] == [3, 1, 1, 2] and len(host["unused"]["rows"]) == 4
    assert host["mirror"]["bsdfs"][0]["flags"] == sr.F_DELTA and host["mirror"]["rows"][0]["eta"] == [0, 0, 0] and host["mirror"]["rows"][0]["k"] == [1, 1, 1]
    assert np.allclose(host["metal"]["rows"][0]["eta"], [0.143, 0.375, 1.442], rtol=1e-7) and np.allclose(host["metal"]["rows"][0]["k"], [3.983, 2.386, 1.603], rtol=1e-7)
    assert host["plastic"]["bsdfs"][0]["flags"] == (sr.F_DELTA | sr.F_SMOOTH)                        # delta and smooth together
    t = host["twosided"]
    assert [b["type"] for b in t["bsdfs"]] == [0, PLASTIC, TWOSIDED] and t["bsdfs"][2]["flags"] == 3 and t["bsdfs"][2]["nested"] == 0 and t["rows"][2]["back"] == 1
    m = host["twosided_mirror"]
    assert m["bsdfs"][1]["flags"] == sr.F_DELTA and m["bsdfs"][1]["nested"] == 0 and m["rows"][1]["back"] == 0      # the union of the children's flags
    assert host["bump"]["bsdfs"][1]["flags"] == 3


def test_host_constants_against_float64(host):
    """plastic.cpp:192-207 as the host computes it in float32 against smooth_ref.py in float64, from the float32 eta both start from.
    Bounds from the formats: a quotient or a product of two rounded values 4 x 2^-24 relative; the two polynomial fits 4 x 2^-24 of the sum
    of their terms' sizes (six fused steps, each rounding a partial sum no larger than that), which for eta = 1.49 is 5e-6 absolute
    on values of 0.1 .. 0.6."""
    u = 2.0 ** -24
    cases = {"plastic": sr.Plastic(), "plastic2": sr.Plastic(int_ior=1.9, ext_ior="water", diffuse_reflectance=[0.8, 0.4, 0.1], specular_reflectance=sc.BOARD),
             "plastic_dense": sr.Plastic(int_ior=1.0, ext_ior=1.5)}
    for name, p in cases.items():
        B, X = host[name]["bsdfs"][0], host[name]["rows"][0]
        k = p.constants(np.float64)
        assert np.float32(B["eta"]) == p.eta32
        assert abs(X["inv_eta_2"] - k["inv_eta_2"]) <= 4 * u * k["inv_eta_2"]
        assert abs(X["spec_weight"] - k["specular_sampling_weight"]) <= 8 * u * k["specular_sampling_weight"]
        for key, e in (("fdr_int", 1 / k["eta"]), ("fdr_ext", k["eta"])):
            size = (sum(abs(c) / e ** i for i, c in enumerate(sr.FDR_2)) if e >= 1 else abs(sr.FDR_1[0]) / e + abs(sr.FDR_1[1]) + abs(sr.FDR_1[2]) * e + abs(sr.FDR_1[3]) * e * e)
            print(f"[smooth host] {name} {key}: host {X[key]!r} float64 {float(k[key])!r} bound {4 * u * size:.2e}")
            assert abs(X[key] - k[key]) <= 4 * u * size, (name, key)
        assert X["nonlinear"] == 0 and X["specular_reflectance"] == (-1 if p.spec is None else 1)
    # the two fits against each other: 1 - F(1 / eta) = (1 - F(eta)) / eta^2 holds for the exact diffuse Fresnel reflectance, and each fit is within 0.1 % at 1.5 (fresnel.h:335-350)
    assert abs((1 - sr.fresnel_diffuse_reflectance(1 / 1.5)) - (1 - sr.fresnel_diffuse_reflectance(1.5)) / 2.25) < 2e-3
    assert sr.Tex([0.3, 0.6, 0.9]).mean() == pytest.approx(0.6) and sc.BOARD.mean() == pytest.approx(0.5 * (0.6 + 0.4))


# ------------------------------------------------------------------------------------------------------------- the reference against itself
@pytest.fixture(scope="module")
def rows():
    out = []
    for name, bsdf, shape, bump in sc.CASES:
        o, d, smp, woq, wi, uv = sc.make_inputs(bsdf, shape)
        ref = sc.reference(bsdf, wi, smp, woq, uv)
        out.append((name, bsdf, (wi, smp, woq, uv), ref))
    return out


def test_k_table(rows):
    """the float32 run against the float64 run reproduces the committed K: 4 x the worst ratio, rounded up to a power of two"""
    worst = {k: 0.0 for k in sc.FIELDS}
    for name, bsdf, inp, ref in rows:
        w = sc.worst_ratios(ref, sc.run32(bsdf, *inp))
        print(f"[smooth K] {name:22s} " + "  ".join(f"{k} {v[0]:5.2f}" for k, v in w.items()))
        for k, (r, _) in w.items():
            worst[k] = max(worst[k], r)
    print("[smooth K] worst: " + "  ".join(f"{k} {v:.2f} (K = {sc.K[k]:g})" for k, v in worst.items()))
    for k, v in worst.items():
        assert sc.K[k] == max(1.0, 2.0 ** np.ceil(np.log2(max(4 * v, 1e-30)))), (k, v, sc.K[k])


def test_left_out_share(rows):
    """the float64 reference alone leaves at most 1 % of a batch out, in every case; both lobes and both sides are met"""
    for name, bsdf, inp, ref in rows:
        left = max((~ref["sample_ok"]).sum(), (~ref["eval_ok"]).sum())
        print(f"[smooth left out] {name:22s} sample {(~ref['sample_ok']).sum()} eval {(~ref['eval_ok']).sum()} of {sc.N_LANES}")
        assert left <= sc.MAX_LEFT_OUT * sc.N_LANES, (name, left)
        wi = inp[0]
        assert (wi[:, 2] > 0).sum() == (wi[:, 2] < 0).sum() == sc.N_LANES // 2 and (np.abs(wi[:, 2]) == 1).sum() >= 64 and (np.abs(wi[:, 2]) < 0.05).sum() >= 128
        for bit in (sr.F_DELTA, sr.F_SMOOTH):
            if bsdf.flags & bit:
                assert ((ref["type"] & bit) != 0).sum() >= 256, (name, bit)
        assert set(np.unique(ref["type"])) <= {0, sr.F_DELTA, sr.F_SMOOTH}                # a sample's type is one of the two


def test_twosided_identities():
    """test02 and test03 of the followed renderer's src/bsdfs/tests/test_twosided.py, on smooth_ref.py"""
    one = sr.TwoSided(sr.Diffuse(0.5)); uv = np.zeros((1, 2))
    up = np.array([[0.0, 0.0, 1.0]])
    assert np.allclose(one.eval_pdf(up, up, uv)[1], 1 / np.pi) and np.allclose(one.eval_pdf(up, -up, uv)[1], 0.0)          # test02
    two = sr.TwoSided(sr.Diffuse(0.1), sr.Diffuse(0.9)); n = 5; met = 0                                                      # test03
    for u in range(n):
        for v in range(n):
            z = 1 - 2 * v / (n - 1); r = np.sqrt(max(0.0, 1 - z * z)); ph = 2 * np.pi * u / (n - 1)
            wi = np.array([[r * np.cos(ph), r * np.sin(ph), z]])
            for x in range(n):
                for y in range(n):
                    s = two.sample(wi, np.array([0.5]), np.array([[x / (n - 1), y / (n - 1)]]), uv)
                    if (s["weight"] > 0).any():
                        val = s["weight"] * s["wo"][:, 2:3] / np.pi * (1 if z > 0 else -1)
                        ev, p, _ = two.eval_pdf(wi, s["wo"], uv)
                        assert np.allclose(val, ev, atol=1e-2) and np.allclose(s["pdf"], p) and np.isfinite(ev).all() and np.isfinite(val).all()
                        assert np.allclose(ev, 0.1 / np.pi * abs(s["wo"][0, 2]) if z > 0 else 0.9 / np.pi * abs(s["wo"][0, 2]))
                        met += 1
    assert met >= 150


MISTAKES = [            # case, the keyword smooth_ref.py takes, the fields that must leave their tolerance
    ("plastic", "f_o_at_wi", ("weight",)),
    ("plastic_nonlinear", "no_inv_eta_2", ("weight", "eval")),
    ("twosided_plastic", "no_mulsign", ("wo", "eval", "eval_pdf")),
    ("twosided_two", "wrong_child", ("weight", "pdf")),
    ("conductor_rgb", "swap", ("weight",)),
]


@pytest.mark.parametrize("case, mistake, fields", MISTAKES, ids=[m[1] for m in MISTAKES])
def test_seeded_mistakes_fail(rows, case, mistake, fields):
    """each mistake, made in the float64 reference, leaves the tolerance the device is held to by orders of magnitude"""
    (name, bsdf, inp, ref), = [r for r in rows if r[0] == case]
    w = sc.worst_ratios(ref, sc.run32(bsdf, *inp, **{mistake: True}))
    print(f"[smooth mistake] {mistake} on {case}: " + "  ".join(f"{k} {v[0]:.3g}/{sc.K[k]:g}" for k, v in w.items()))
    for k in fields:
        assert w[k][0] > 1000 * sc.K[k], (mistake, k, w[k][0])
