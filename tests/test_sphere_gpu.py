"""GPU tests of sphere shapes and point emitters: the ray queries (LDS and global tracers, closest and any hit) against the float32
numpy restatement, the first-hit surface interaction through the aov integrator, Beer-Lambert through an index-matched sphere with
and without the distance-field proofs, direct light from a point emitter against its closed form, and the fork's SphereLiver layout
(point, constant and envmap lighting) through every forward integrator and through the multi-device path."""
import os

import numpy as np
import pytest

import sphere_ref as sr

pytestmark = pytest.mark.gpu

from sphere_ref import NONE, SPHERES, FLOOR, sphere_xml, scene_xml        # (shared with the oracle's tests: tests/test_sphere_oracle.py)


def _check_queries(sc, n_faces, with_floor):
    sr.check_queries(sc.trace, n_faces, with_floor)


@pytest.mark.parametrize("lds", [True, False])
def test_ray_queries_spheres_and_floor(mi, monkeypatch, lds):
    if not lds:
        monkeypatch.setenv("LRT_NO_LDS_BVH", "1")
    sc = mi.load_string(scene_xml(FLOOR + "".join(sphere_xml(c, r) for c, r in SPHERES)))
    _check_queries(sc, 2, True)


def test_ray_queries_spheres_only(mi):
    sc = mi.load_string(scene_xml("".join(sphere_xml(c, r) for c, r in SPHERES)))
    assert sc.desc.n_faces == 0
    _check_queries(sc, 0, False)


def test_aov_first_hit_on_a_sphere(mi):
    c, r = (0.25, -0.5, 0.5), 1.5
    floor = ('<shape type="rectangle"><transform name="to_world"><rotate x="1" angle="-90"/><scale x="25" y="1" z="25"/>'
             '<translate x="0" y="-3" z="0"/></transform></shape>')                  # (below the sphere: triangles make the LDS image)
    xml = scene_xml(floor + sphere_xml(c, r), integrator='<integrator type="aov"><string name="aovs" value="pp:position,nn:sh_normal,uv:uv,gg:geo_normal,du:dp_du,dv:dp_dv"/></integrator>',
                    size=(24, 24), fov=30)
    sc = mi.load_string(xml)
    n = 24 * 24 * 4
    a = sc.render_aov_samples(0, n)
    p, nn, uv, gn, dpu, dpv = a[:, 0:3], a[:, 3:6], a[:, 6:8], a[:, 8:11], a[:, 11:14], a[:, 14:17]
    hit = np.abs(np.linalg.norm(p.astype(np.float64) - c, axis=1) - r) < 1e-3           # lanes on the sphere (the others see the floor)
    floor_hit = np.abs(p[:, 1] + 3) < 1e-4
    assert 0.2 < hit.mean() < 0.9 and floor_hit.sum() > 50 and (hit | floor_hit | (np.abs(p).sum(1) == 0)).all()
    P = p[hit].astype(np.float64)
    dist = np.linalg.norm(P - c, axis=1)
    assert np.abs(dist - r).max() < 1e-5 * (r + np.abs(c).max() + 10)       # p = ray(t) lies on the sphere to float32 accuracy
    ref_n = (P - c) / dist[:, None]
    assert np.abs(nn[hit] - ref_n).max() < 2e-6 and np.abs(gn[hit] - ref_n).max() < 2e-6
    local = (P - c) / r
    theta = np.arccos(np.clip(local[:, 2] / np.linalg.norm(local, axis=1), -1, 1))
    phi = np.arctan2(local[:, 1], local[:, 0]); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    du = np.abs(uv[hit, 0] - phi / (2 * np.pi)); du = np.minimum(du, 1 - du)          # (phi wraps at 2 pi)
    assert du.max() < 2e-5 and np.abs(uv[hit, 1] - theta / np.pi).max() < 2e-5
    # the numpy surface interaction from the device's own t
    cam_o = np.array([0, 3, -8], np.float32)
    t = np.linalg.norm(P - cam_o, axis=1).astype(np.float32)
    dirs = ((P - cam_o) / t[:, None]).astype(np.float32)
    p2, n2, uv2, du2, dv2 = sr.surface_f32(np.repeat(cam_o[None], hit.sum(), 0), dirs, t, c, r)
    assert np.abs(p2 - P).max() < 1e-4 and np.abs(n2 - nn[hit]).max() < 1e-4
    # dp_du = to_world (-y, x, 0) 2 pi, dp_dv = to_world (z cos phi, z sin phi, -rd) pi of the local point (sphere.cpp:693-716)
    assert np.abs(dpu[hit] - du2).max() < 1e-3 * r * 2 * np.pi and np.abs(dpv[hit] - dv2).max() < 1e-3 * r * np.pi


def test_beer_lambert_through_an_index_matched_sphere(mi, monkeypatch):
    """Index-matched glass around a purely absorbing medium under a constant emitter: exp(-sigma_t * chord) per camera ray.  The
    distance-field proofs must not change any lane (a proof that ignored the sphere would walk medium trips through the glass)."""
    size = sr.BEER["size"]
    xml = sr.beer_lambert_xml()
    sc = mi.load_string(xml)
    img = sc.render(seed=11)
    lanes = sc.render_samples(0, size * size * 64, seed=11, spp=64)
    monkeypatch.setenv("LRT_NO_DIST_GRID", "1")
    sc2 = mi.load_string(xml)
    lanes2 = sc2.render_samples(0, size * size * 64, seed=11, spp=64)
    assert (lanes.view(np.uint32) == lanes2.view(np.uint32)).all()
    sr.check_beer_lambert(img)


def test_point_light_direct_closed_form(mi):
    """path, max_depth = 2: a diffuse unit sphere on a diffuse floor (y = -1), a point light on the axis above them, the camera
    looking straight down that axis: (a / pi) I max(0, cos) / d^2 per sample, the floor shadowed where the segment to the light
    meets the sphere."""
    sr.check_point_light(mi.load_string(sr.point_light_xml()).render(seed=2))


def test_volpath_point_light_beside_an_envmap(mi):
    xml = scene_xml(FLOOR + sphere_xml((0, 0, 0), 1.0, '<bsdf type="dielectric"/><medium type="homogeneous" name="interior"><rgb name="sigma_t" value="1"/></medium>'),
                    emitters='<emitter type="point"><point name="position" x="2" y="3" z="0"/><rgb name="intensity" value="5"/></emitter>'
                             '<emitter type="envmap"><string name="filename" value="cavidade_latitude.exr"/></emitter>',
                    integrator='<integrator type="volpath"><integer name="max_depth" value="8"/></integrator>', size=(32, 24), spp=16)
    assets = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "assets")
    sc = mi.load_string(xml, assets)
    a = sc.render(seed=1)
    assert np.isfinite(a).all() and (a[..., :3] >= 0).all() and a[..., :3].mean() > 0
    la = sc.render_samples(0, 4096, seed=1); lb = sc.render_samples(0, 4096, seed=1)
    assert (la.view(np.uint32) == lb.view(np.uint32)).all()
    # the point light adds light: the same scene without it is darker on the floor
    sc2 = mi.load_string(xml.replace('<emitter type="point"><point name="position" x="2" y="3" z="0"/><rgb name="intensity" value="5"/></emitter>', ""),
                         assets)
    assert sc2.render(seed=1)[..., :3].mean() < a[..., :3].mean()


FORWARD = ("path", "volpath", "volpathmis", "biovolpath", "biovolpath06")
PARENCHYMA = ('<medium type="parenchyma" name="interior"><rgb name="sigma_blood" value="0.2464, 0.15, 0.01"/><rgb name="sigma_bile" value="0.02, 0.01, 0.003"/>'
              '<rgb name="sigma_lipid_water" value="0.001"/><float name="sigma_hepatocity" value="2.0"/></medium>')
CHECKER_FLOOR = ('<shape type="rectangle"><transform name="to_world"><rotate x="1" angle="-90"/><scale x="25" y="1" z="25"/><translate x="0" y="-1" z="0"/></transform>'
                 '<bsdf type="diffuse"><texture name="reflectance" type="checkerboard"><rgb name="color0" value="0.325, 0.31, 0.25"/>'
                 '<rgb name="color1" value="0.725, 0.71, 0.68"/><transform name="to_uv"><scale x="10" y="10"/></transform></texture></bsdf></shape>')
LIGHTS = {"point": '<emitter type="point"><transform name="to_world"><translate x="2.5" y="0.25" z="0"/></transform><rgb name="intensity" value="10"/></emitter>',
          "constant": '<emitter type="constant"/>',
          "envmap": '<emitter type="envmap"><string name="filename" value="cavidade_latitude.exr"/><float name="scale" value="2.5"/></emitter>'}


def sphere_liver(mi, light, integrator):
    """The fork's SphereLiver layout (unit dielectric sphere with a parenchyma interior on a checkerboard floor, camera at (0, 5, -10)),
    with RGB medium coefficients, under a point light, a constant emitter or the cavity envmap."""
    xml = scene_xml(CHECKER_FLOOR + sphere_xml((0, 0, 0), 1.0, '<bsdf type="Dielectric"/>' + PARENCHYMA), emitters=LIGHTS[light],
                    integrator=f'<integrator type="{integrator}"><integer name="max_depth" value="12"/></integrator>',
                    cam=((0, 5, -10), (0, 0, 0), (0, 1, 0)), fov=35, size=(96, 54), spp=8, rfilter="tent", sampler="ldsampler")
    return mi.load_string(xml, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "assets"))


@pytest.mark.parametrize("light", ["point", "constant", "envmap"])
@pytest.mark.parametrize("integrator", FORWARD)
def test_sphere_scenes_every_forward_integrator(mi, light, integrator):
    sc = sphere_liver(mi, light, integrator)
    a = sc.render(seed=4); b = sc.render(seed=4)
    assert np.isfinite(a).all() and (a[..., :3] >= 0).all()
    assert np.allclose(a, b, rtol=1e-5, atol=1e-6)          # (the tent filter's film atomics add in any order)
    # biovolpath.cpp:297-300 zeroes `result` wherever mei.transmittance == 0, lanes outside any medium included: surface NEE is erased on
    # the next trip, so with a point light as the only emitter (never hit) the reference's image is black too
    if not (integrator.startswith("bio") and light == "point"):
        assert a[..., :3].mean() > 1e-3
    la = sc.render_samples(0, 4096, seed=4); lb = sc.render_samples(0, 4096, seed=4)
    assert (la.view(np.uint32) == lb.view(np.uint32)).all() and np.isfinite(la).all()


@pytest.mark.parametrize("light", ["point", "constant", "envmap"])
def test_sphere_scenes_multi_device_matches_single(mi, light):
    sc = sphere_liver(mi, light, "volpath")
    img, raw = sc.render(seed=6, return_raw=True)
    imgn, rawn = sc.render_multi([0, 0], seed=6, return_raw=True)
    assert np.allclose(rawn, raw, rtol=1e-5, atol=1e-6) and np.allclose(imgn, img, rtol=2e-4, atol=1e-6)


def test_prbvolpath_override_is_rejected(mi):
    sc = sphere_liver(mi, "constant", "volpath")
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath"):
        sc.render(integrator="prbvolpath")
