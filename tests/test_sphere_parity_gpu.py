"""Lane parity of the sphere and point-emitter kernels (the `EXT` instances of `k_render`, `k_trace[_lds]` and the probe kernel) with the
CPU oracle, which restates src/shapes/sphere.cpp and src/emitters/point.cpp on its own (oracle/orc_scene.cpp, orc_render.cpp; pinned on
the CPU by tests/test_sphere_oracle.py and tests/test_surface.py).  Every case compares `render_samples` lanes bit for bit
(`view(np.uint32)`), the loop-trip and shadow-ray counts, and the raw film under `film_close` (float atomics in any order)."""
import os

import numpy as np
import pytest

import sphere_ref as sr
from sphere_ref import FLOOR, SPHERES, sphere_xml, scene_xml
from test_parity_gpu import assert_lanes_equal, bits, film_close
from test_sphere_gpu import CHECKER_FLOOR, FORWARD, PARENCHYMA, sphere_liver

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "assets")


def parity(sc, o, **kw):
    """every lane of the film, the counts, the film"""
    h, w, _ = sc.film_shape()
    g = assert_lanes_equal(sc, o, 0, h * w * sc.spp, **kw)
    raw = sc.render(return_raw=True, **kw)[1]
    st = sc.stats()
    oraw = o.render(return_raw=True, **kw)[1]
    assert st["n_iter"] == o.last_stats["n_iter"] and st["n_shadow"] == o.last_stats["n_shadow_needed"]
    assert film_close(raw, oraw).all()
    return g


# ------------------------------------------------------------------ ray queries and the surface interaction
@pytest.mark.parametrize("lds", [True, False])
def test_ray_queries_bit_exact(mi, orc, monkeypatch, lds):
    """t, u, v and the primitive of 20000 + 5 rays equal to the oracle's brute-force search bit for bit, spheres beside the floor and alone:
    the random rays of the query tests, and the exact ties of tests/test_sphere_oracle.py::test_traversal_order (the tangent point on the
    floor, two equal spheres)."""
    if not lds:
        monkeypatch.setenv("LRT_NO_LDS_BVH", "1")
    o, d = sr.random_rays(20000, 3)
    tmax = np.full(len(o), np.finfo(np.float32).max, np.float32)
    tmax[::5] = np.random.default_rng(4).uniform(0.5, 6, size=len(tmax[::5])).astype(np.float32)
    ties = (np.float32([[0, 0, 0], [0, 0, 0], [0, 8, 0], [0, 2, 0], [0, 2, 0]]), np.float32([[0, -1, 0], [0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 1, 0]]),
            np.float32([tmax[1]] * 4 + [1.0]))
    spheres = "".join(sphere_xml(c, r) for c, r in SPHERES)
    tangent = sphere_xml((0, 0, 0), 1.0) + sphere_xml((0, 0, 0), 1.0) + sphere_xml((0, 4, 0), 0.5)
    for shapes, rays in ((FLOOR + spheres, (o, d, tmax)), (spheres, (o, d, tmax)), (FLOOR + tangent, ties)):
        sc = mi.load_string(scene_xml(shapes)); oc = orc.OrcScene(sc)
        g, c = sc.trace(*rays), oc.trace(*rays, brute_force=True)
        for x, y in zip(g, c):
            assert (bits(x) == bits(y)).all() if x.dtype == np.float32 else (x == y).all()
        assert (g[3] != sr.NONE).sum() > 2
        assert ((sc.trace(*rays, any_hit=True)[0] == 0) == (oc.trace(*rays, any_hit=True)[0] == 0)).all()
    assert g[3][0] < 2 and g[3][1] == 2 and g[3][2] == 4


@pytest.mark.parametrize("flip", [False, True])
def test_surface_interaction_and_bsdf_bit_exact(mi, orc, flip):
    """lrt_bsdf_probe against orc_bsdf_probe on a glass sphere and a checkerboard sphere, from outside and inside, the poles included: every
    float of the probe (t, p, n, the frame's normal, uv, wi, the BSDF sample, eval and pdf) bit for bit"""
    extra = '<boolean name="flip_normals" value="true"/>' if flip else ""
    checker = '<bsdf type="diffuse"><texture name="reflectance" type="checkerboard"><transform name="to_uv"><scale x="8" y="8"/></transform></texture></bsdf>'
    sc = mi.load_string(scene_xml(sphere_xml((0.25, -0.5, 0.5), 1.5, extra + '<bsdf type="dielectric"/>') + sphere_xml((4, 0, 0), 1.0, extra + checker)))
    rng = np.random.default_rng(9)
    n = 6000
    unit = lambda: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(n, 3)))
    which = rng.random((n, 1)) < 0.5
    c = np.where(which, [[0.25, -0.5, 0.5]], [[4.0, 0.0, 0.0]]); r = np.where(which, 1.5, 1.0)
    tgt = c + unit() * r * 0.9 * rng.random((n, 1)) ** (1 / 3)
    org = c + unit() * r * np.where(rng.random((n, 1)) < 0.5, rng.uniform(1.5, 5, (n, 1)), rng.uniform(0, 0.7, (n, 1)))
    d = tgt - org; d /= np.linalg.norm(d, axis=1, keepdims=True)
    org = np.concatenate([org, [[4, 0, 3], [4, 0, -3]]]); d = np.concatenate([d, [[0, 0, -1], [0, 0, 1]]])     # the poles: rd == 0
    smp = rng.random((n + 2, 3)).astype(np.float32); wo = unit()[:1].repeat(n + 2, 0)
    g = sc.bsdf_probe(np.float32(org), np.float32(d), smp, np.float32(wo))
    c_ = orc.OrcScene(sc).bsdf_probe(np.float32(org), np.float32(d), smp, np.float32(wo))
    assert (g["shape"] >= 0).mean() > 0.9
    same = (bits(g["raw"]) == bits(c_["raw"])).all(axis=1)
    assert same.all(), (int((~same).sum()), g["raw"][np.argmin(same)], c_["raw"][np.argmin(same)])


# ------------------------------------------------------------------ the SphereLiver layout
@pytest.mark.parametrize("light", ["point", "constant", "envmap"])
@pytest.mark.parametrize("integrator", FORWARD)
def test_sphere_liver_layout(mi, orc, light, integrator):
    """ld sampler, tent film, a unit glass sphere full of parenchyma tangent to the floor (the equal-t tie), 96 x 54 x 8 spp"""
    sc = sphere_liver(mi, light, integrator)
    g = parity(sc, orc.OrcScene(sc), seed=4)
    assert np.isfinite(g).all()
    # biovolpath.cpp:297-300 zeroes `result` wherever mei.transmittance == 0: with a point light alone both sides give the reference's black image
    assert (g[:, :3] > 0).any() != (integrator.startswith("bio") and light == "point")


# ------------------------------------------------------------------ further sphere scenes
FOG = ('<medium type="homogeneous" name="interior"><rgb name="sigma_t" value="1.5, 0.7, 2.0"/><rgb name="albedo" value="0.9, 0.95, 0.6"/>'
       '<phase type="hg"><float name="g" value="0.5"/></phase></medium>')
HAZE = ('<medium type="homogeneous" name="interior"><rgb name="sigma_t" value="0.4, 0.9, 0.3"/><rgb name="albedo" value="0.7, 0.8, 0.95"/></medium>')
GLASS = '<bsdf type="dielectric"/>'
ENV = '<emitter type="constant"><rgb name="radiance" value="0.8, 0.9, 1.0"/></emitter>'
POINT = '<emitter type="point"><point name="position" x="2" y="3" z="0"/><rgb name="intensity" value="5"/></emitter>'
ENVMAP = '<emitter type="envmap"><string name="filename" value="cavidade_latitude.exr"/></emitter>'


def small_scene(what, integrator):
    kw = dict(integrator=f'<integrator type="{integrator}"><integer name="max_depth" value="8"/></integrator>', size=(24, 16), spp=8, emitters=ENV)
    if what == "spheres-only":                      # n_faces == 0: no BVH at all
        shapes = sphere_xml((0, 0, 0), 1.0, GLASS + FOG) + sphere_xml((2.5, 0.5, 1.0), 0.6)
    elif what == "nested":                          # the medium stack at sphere boundaries: haze inside the outer sphere, fog inside the inner one
        outer = sphere_xml((0, 0, 0), 1.6, GLASS + HAZE)
        inner = sphere_xml((0.2, 0, 0), 0.7, GLASS + FOG + HAZE.replace('name="interior"', 'name="exterior"'))
        shapes = CHECKER_FLOOR.replace('y="-1"', 'y="-1.7"') + outer + inner
    elif what == "overlapping":
        shapes = CHECKER_FLOOR + sphere_xml((-0.5, 0, 0), 1.0, GLASS + FOG) + sphere_xml((0.5, 0.2, 0), 1.0, '<bsdf type="null"/>' + HAZE)
    elif what == "flip_normals":
        shapes = CHECKER_FLOOR + sphere_xml((0, 0, 0), 1.0, '<boolean name="flip_normals" value="true"/>' + GLASS + FOG) + sphere_xml((2.2, 0, 0.5), 0.8, '<boolean name="flip_normals" value="true"/>')
    elif what == "camera-inside":                   # rays start inside the sphere: the far root, a camera medium, a finite first maxt
        med = '<medium type="homogeneous" id="haze"><rgb name="sigma_t" value="0.3, 0.5, 0.2"/><rgb name="albedo" value="0.8"/></medium>'
        shapes = CHECKER_FLOOR.replace('y="-1"', 'y="-3.2"') + sphere_xml((0, 3, -8), 3.0, GLASS + '<ref name="interior" id="haze"/>') + sphere_xml((0, 0, 0), 1.0)
        kw["integrator"] = med + kw["integrator"]             # (declared before the sensor that names it)
        kw["sensor_extra"] = '<ref id="haze"/>'
    elif what == "point-beside-envmap":             # tests/test_sphere_gpu.py::test_volpath_point_light_beside_an_envmap's scene
        shapes = FLOOR + sphere_xml((0, 0, 0), 1.0, '<bsdf type="dielectric"/><medium type="homogeneous" name="interior"><rgb name="sigma_t" value="1"/></medium>')
        kw["emitters"] = POINT + ENVMAP
    return scene_xml(shapes, **kw)


@pytest.mark.parametrize("integrator", ["volpath", "volpathmis"])
@pytest.mark.parametrize("what", ["spheres-only", "spheres-only-global-bvh", "nested", "overlapping", "flip_normals", "camera-inside", "point-beside-envmap"])
def test_small_sphere_scenes(mi, orc, monkeypatch, what, integrator):
    if what.endswith("-global-bvh"):
        monkeypatch.setenv("LRT_NO_LDS_BVH", "1"); what = what[:-len("-global-bvh")]
    sc = mi.load_string(small_scene(what, integrator), ASSETS)
    assert (sc.desc.n_faces == 0) == (what == "spheres-only")
    if what == "camera-inside":
        assert sc.desc.sensor.medium >= 0
    g = parity(sc, orc.OrcScene(sc), seed=2)
    assert np.isfinite(g).all() and (g[:, :3] > 0).any()


def test_point_light_alone_under_biovolpath_is_black_on_both_sides(mi, orc):
    shapes = CHECKER_FLOOR + sphere_xml((0, 0, 0), 1.0, GLASS + PARENCHYMA)
    for integrator in ("biovolpath", "biovolpath06"):
        sc = mi.load_string(scene_xml(shapes, emitters=POINT, integrator=f'<integrator type="{integrator}"><integer name="max_depth" value="8"/></integrator>',
                                      size=(24, 16), spp=8))
        g = parity(sc, orc.OrcScene(sc), seed=2)
        assert (g[:, :3] == 0).all()


# ------------------------------------------------------------------ the fork's three scene files
@pytest.mark.parametrize("integrator", ["volpath", "biovolpath"])
@pytest.mark.parametrize("scene", sr.SPHERE_SCENES)
def test_sphere_liver_scene_files(mi, orc, scene, integrator):
    """tests/golden/scenes/SphereLiver*/scene.xml with RGB coefficients (sphere_ref.rgb_variant), at a small film by load-time overrides"""
    d = os.path.join(sr.GOLDEN_SCENES, scene)
    sc = mi.load_string(sr.rgb_variant(os.path.join(d, "scene.xml")), d, integrator=integrator, spp=4, res_width=48, res_height=27, max_depth=12)
    assert sc.film_shape()[:2] == (27, 48)
    g = parity(sc, orc.OrcScene(sc), seed=1)
    assert np.isfinite(g).all()
