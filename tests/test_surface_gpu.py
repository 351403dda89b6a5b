"""Surface scattering on the device through lrt_bsdf_probe (k_bsdf_probe, csrc/kernels.h): the checks of tests/test_surface.py run on
the HIP kernel's output, every probe on triangle shapes compared with the oracle's bit for bit (check e), the sphere held to the float64
reference here (its probes are compared with the oracle's bit for bit in tests/test_sphere_parity_gpu.py), and the two transport closed forms of check f through the render kernels."""
import numpy as np
import pytest

import envmap_cases as ec
import surface_cases as sc
import test_surface as ts

pytestmark = pytest.mark.gpu


def _prober(orc, scene):
    return sc.Prober(scene.bsdf_probe, orc.OrcScene(scene).bsdf_probe)


def test_abi_and_probe_arguments(mi, tmp_path):
    L = mi._lib.lib()
    assert L.lrt_version() >= 113 and "lrt_bsdf_probe" in mi._lib.EXPORTED_SYMBOLS
    scene, _ = sc.build(mi, tmp_path, [("rectangle_plain", ("diffuse",))])
    z = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError):
        scene.bsdf_probe(z, z, z, z[:2])
    miss = scene.bsdf_probe([[0, 0, 5]], [[0, 0, 1]], [[0, 0, 0]], [[0, 0, 1]])          # away from the rectangle
    assert miss["shape"][0] == -1 and (miss["raw"][0, 1:] == 0).all()
    assert len(scene.bsdf_probe(z[:0], z[:0], z[:0], z[:0])["t"]) == 0
    # more than one block, and a count that is no multiple of the block
    n = 1000
    o = np.tile(np.float32([[0.1, 0.2, 3.0]]), (n, 1)); d = np.tile(np.float32([[0, 0, -1]]), (n, 1))
    pr = scene.bsdf_probe(o, d, np.full((n, 3), 0.5, np.float32), np.tile(np.float32([[0, 0, 1]]), (n, 1)))
    assert (pr["shape"] == 0).all() and (pr["raw"] == pr["raw"][0]).all() and pr["t"][0] == 3.0


def test_known_answers_of_the_reference(mi, orc, tmp_path):
    """a on the device (the fresnel(cos, eta) entries are the oracle's: the device is reached through the probe), e"""
    scene, _ = sc.build(mi, tmp_path, sc.known_items())
    prober = _prober(orc, scene)
    n = sc.check_known_answers(prober, None, "device")
    assert n == sum(e["via"] == "probe" for e in sc.known_answers()) and prober.n_compared > 0


def test_dielectric_sweep(mi, orc, tmp_path):
    """b and e"""
    names = list(sc.ETAS)
    items = [("rectangle", ("dielectric", k)) for k in names] + [("cube", ("dielectric", "1.5"))]
    scene, surf = sc.build(mi, tmp_path, items)
    prober = _prober(orc, scene)
    for k, name in enumerate(names):
        sc.check_dielectric(prober, surf[k], k, sc.eta_of(name), f"device rectangle eta {name}", seed=10 + k)
    sc.check_dielectric(prober, surf[len(names)], len(names), 1.5, "device cube eta 1.5", seed=30)
    assert prober.n_compared == prober.n_rays * mi._lib.BSDF_PROBE_FLOATS
    print(f"[surface e] dielectric sweep: {prober.n_compared} floats of {prober.n_rays} probes compared bit for bit")


def test_dielectric_sweep_on_the_sphere(mi, tmp_path):
    """b on the sphere, from outside and inside: the device against float64 (the oracle runs the same check in tests/test_surface.py)"""
    scene, surf = sc.build(mi, tmp_path, [("sphere", ("dielectric", "1.5"))])
    sc.check_dielectric(sc.Prober(scene.bsdf_probe), surf[0], 0, 1.5, "device sphere eta 1.5", seed=31)


def test_diffuse_and_checkerboard(mi, orc, tmp_path):
    """c and e"""
    items = [("rectangle", ("diffuse",)), ("rectangle", ("checker",)), ("quad", ("checker",))]
    scene, surf = sc.build(mi, tmp_path, items + [("rectangle_plain", ("checker_plain",))])
    prober = _prober(orc, scene)
    for k, (kind, spec) in enumerate(items):
        sc.check_diffuse(prober, surf[k], k, f"device {kind} {spec[0]}", spec[0] == "checker", seed=40 + k)
    sc.check_checker_on_the_edge(prober, len(items), "device checkerboard edges")
    assert prober.n_compared == prober.n_rays * mi._lib.BSDF_PROBE_FLOATS


def test_checkerboard_on_the_sphere(mi, tmp_path):
    """c on the sphere: the device against float64"""
    scene, surf = sc.build(mi, tmp_path, [("sphere", ("checker",))])
    sc.check_diffuse(sc.Prober(scene.bsdf_probe), surf[0], 0, "device sphere checker", True, seed=44)


@pytest.mark.parametrize("shape,name,to_uv", ts.BUMP_CASES + [("sphere", "field", "scaled"), ("sphere", "ramp_v", "id")])
def test_bump_map(mi, orc, tmp_path, shape, name, to_uv):
    """d and e"""
    prober = ts.run_bump_case(mi, tmp_path, shape, name, to_uv, lambda scene: _prober(orc, scene), "device")
    assert (prober.n_compared > 0) == (shape != "sphere")


@pytest.mark.parametrize("integrator", ["path", "volpath"])
@pytest.mark.parametrize("what", ["plate", "sphere"])
def test_transport(mi, tmp_path, what, integrator):
    """f: the glass plate (R_tot L(mirror d) + T_tot L(d)) and the glass sphere (the series of internal reflections) under a smooth map"""
    scene = sc.transport_scene(mi, tmp_path, what, integrator)
    sc.check_transport(lambda spp, seed: scene.render(spp=spp, seed=seed), ec.reference_of(scene), what, f"device {what} {integrator}", power=0.01)
