"""Surface scattering of the CPU oracle against float64 references (tests/surface_ref.py) and the reference's own BSDF test vectors
(tests/golden/bsdf_known_answers.json), through orc_bsdf_probe: checks a - d and the plate of f of DESIGN.md section 13.  The device
runs the same checks in tests/test_surface_gpu.py and is held to the oracle bit for bit there."""
import ctypes as C

import numpy as np
import pytest

import envmap_cases as ec
import surface_cases as sc


def _orc_fresnel(orc):
    def f(c, eta):
        out = (C.c_float * 4)()
        orc.lib().orc_fresnel(C.c_float(float(c)), C.c_float(float(eta)), out)
        return np.array(out[:], np.float32)
    return f


def test_known_answers_of_the_reference(mi, orc, tmp_path):
    """a: every assertion of test_dielectric.py test02 / 03 / 05, test_diffuse.py test02 and test_fresnel.py test01 / 04"""
    scene, _ = sc.build(mi, tmp_path, sc.known_items())
    n = sc.check_known_answers(sc.Prober(orc.OrcScene(scene).bsdf_probe), _orc_fresnel(orc), "oracle")
    assert n == len(sc.known_answers())


def test_dielectric_sweep(mi, orc, tmp_path):
    """b: six indices on the tilted rectangle, both sides, and the cube from outside and inside"""
    names = list(sc.ETAS)
    scene, surf = sc.build(mi, tmp_path, [("rectangle", ("dielectric", k)) for k in names] + [("cube", ("dielectric", "1.5"))])
    for k, name in enumerate(names):
        assert scene.desc.bsdfs[scene.desc.shapes[k].bsdf].eta == np.float32(sc.eta_of(name))
    prober = sc.Prober(orc.OrcScene(scene).bsdf_probe)
    for k, name in enumerate(names):
        sc.check_dielectric(prober, surf[k], k, sc.eta_of(name), f"oracle rectangle eta {name}", seed=10 + k)
    sc.check_dielectric(prober, surf[len(names)], len(names), 1.5, "oracle cube eta 1.5", seed=30)


def test_dielectric_sweep_on_the_sphere(mi, orc, tmp_path):
    """b on the sphere, from outside and inside (sphere.cpp's far root): the oracle's sphere interaction against float64"""
    scene, surf = sc.build(mi, tmp_path, [("sphere", ("dielectric", "1.5"))])
    sc.check_dielectric(sc.Prober(orc.OrcScene(scene).bsdf_probe), surf[0], 0, 1.5, "oracle sphere eta 1.5", seed=31)


def test_checkerboard_on_the_sphere(mi, orc, tmp_path):
    """c on the sphere: its uv (dir_to_sph of the local point) picks the checkerboard's colour"""
    scene, surf = sc.build(mi, tmp_path, [("sphere", ("checker",))])
    sc.check_diffuse(sc.Prober(orc.OrcScene(scene).bsdf_probe), surf[0], 0, "oracle sphere checker", True, seed=44)


def test_diffuse_and_checkerboard(mi, orc, tmp_path):
    """c"""
    items = [("rectangle", ("diffuse",)), ("rectangle", ("checker",)), ("quad", ("checker",))]
    scene, surf = sc.build(mi, tmp_path, items + [("rectangle_plain", ("checker_plain",))])
    prober = sc.Prober(orc.OrcScene(scene).bsdf_probe)
    for k, (kind, spec) in enumerate(items):
        sc.check_diffuse(prober, surf[k], k, f"oracle {kind} {spec[0]}", spec[0] == "checker", seed=40 + k)
    sc.check_checker_on_the_edge(prober, len(items), "oracle checkerboard edges")


BUMP_CASES = [("rectangle", "ramp_u", "id"), ("rectangle", "ramp_v", "id"), ("rectangle", "field", "scaled"), ("rectangle", "field", "affine"),
              ("rectangle", "rgb", "id"), ("quad", "field", "scaled"), ("quad", "ramp_u", "id")]
BUMP_SCALE = 0.4


def run_bump_case(mi, tmp_path, shape, name, to_uv, make_prober, label):
    import surface_ref as sr
    path, tex = sc.write_map(mi, tmp_path, name)
    scale = BUMP_SCALE * (4 if shape == "sphere" else 1)           # the sphere's tangents are 2.6 to 5 times as long as the rectangle's: the same order of tilt
    items = [(shape, ("bump", path, scale, to_uv, ("diffuse",))), (shape, ("bump", path, scale, to_uv, ("dielectric", "1.5")))]
    scene, surf = sc.build(mi, tmp_path, items)
    prober = make_prober(scene)
    hm = sr.HeightMap(tex, sc.to_uv_matrix(to_uv))
    ramp = (0, tex) if name == "ramp_u" else (1, tex) if name == "ramp_v" else None
    sc.check_bump_diffuse(prober, surf[0], 0, hm, scale, f"{label} {shape} {name} diffuse", ramp=ramp)
    sc.check_bump_dielectric(prober, surf[1], 1, hm, scale, sc.eta_of("1.5"), f"{label} {shape} {name} dielectric")
    return prober


@pytest.mark.parametrize("shape,name,to_uv", BUMP_CASES)
def test_bump_map(mi, orc, tmp_path, shape, name, to_uv):
    """d"""
    run_bump_case(mi, tmp_path, shape, name, to_uv, lambda scene: sc.Prober(orc.OrcScene(scene).bsdf_probe), "oracle")


@pytest.mark.parametrize("shape,name,to_uv", [("sphere", "field", "scaled"), ("sphere", "ramp_v", "id")])
def test_bump_map_on_the_sphere(mi, orc, tmp_path, shape, name, to_uv):
    """d on the sphere: the bump map perturbs the frame built from the sphere's dp_du / dp_dv"""
    run_bump_case(mi, tmp_path, shape, name, to_uv, lambda scene: sc.Prober(orc.OrcScene(scene).bsdf_probe), "oracle")


@pytest.mark.parametrize("integrator", ["path", "volpath"])
def test_plate_transport(mi, orc, tmp_path, integrator):
    """f, scene 1: a tilted glass plate in front of a smooth environment map, per pixel R_tot L(mirror d) + T_tot L(d)"""
    scene = sc.transport_scene(mi, tmp_path, "plate", integrator)
    o = orc.OrcScene(scene)
    sc.check_transport(lambda spp, seed: o.render(spp=spp, seed=seed), ec.reference_of(scene), "plate", f"oracle plate {integrator}", power=0.03)


@pytest.mark.parametrize("integrator", ["path", "volpath"])
def test_sphere_transport(mi, orc, tmp_path, integrator):
    """f, scene 2: a glass sphere in front of the same map, the series of its internal reflections: every bounce past the first starts
    inside the sphere, takes the far root, and carries the frame and wi of the hit before it"""
    scene = sc.transport_scene(mi, tmp_path, "sphere", integrator)
    o = orc.OrcScene(scene)
    sc.check_transport(lambda spp, seed: o.render(spp=spp, seed=seed), ec.reference_of(scene), "sphere", f"oracle sphere {integrator}", power=0.01)
