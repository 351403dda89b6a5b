"""GPU tests of sphere shapes and point emitters: the ray queries (LDS and global tracers, closest and any hit) against the float32
numpy restatement, the first-hit surface interaction through the aov integrator, Beer-Lambert through an index-matched sphere with
and without the distance-field proofs, direct light from a point emitter against its closed form, and the fork's SphereLiver layout
(point, constant and envmap lighting) through every forward integrator and through the multi-device path."""
import os

import numpy as np
import pytest

import sphere_ref as sr

pytestmark = pytest.mark.gpu

NONE = 0xffffffff

SPHERES = [((0.0, 0.0, 0.0), 1.0), ((2.5, 0.5, 1.0), 0.6)]


def sphere_xml(c, r, extra=""):
    return (f'<shape type="sphere"><point name="center" x="{c[0]}" y="{c[1]}" z="{c[2]}"/><float name="radius" value="{r}"/>'
            f'{extra}</shape>')


def scene_xml(shapes, emitters='<emitter type="constant"/>', integrator='<integrator type="path"/>', cam=((0, 3, -8), (0, 0, 0), (0, 1, 0)),
              fov=40, size=(32, 32), spp=4, rfilter="box", sampler="independent"):
    (o, t, u) = cam
    return f"""<scene version="3.0.0">{integrator}
  <sensor type="perspective"><float name="fov" value="{fov}"/>
    <transform name="to_world"><lookat origin="{o[0]}, {o[1]}, {o[2]}" target="{t[0]}, {t[1]}, {t[2]}" up="{u[0]}, {u[1]}, {u[2]}"/></transform>
    <sampler type="{sampler}"><integer name="sample_count" value="{spp}"/></sampler>
    <film type="hdrfilm"><integer name="width" value="{size[0]}"/><integer name="height" value="{size[1]}"/><rfilter type="{rfilter}"/></film></sensor>
  {shapes}
  {emitters}
</scene>"""


FLOOR = ('<shape type="rectangle"><transform name="to_world"><rotate x="1" angle="-90"/><scale x="25" y="1" z="25"/>'
         '<translate x="0" y="-1" z="0"/></transform></shape>')


def _random_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-4, 4, size=(n, 3)).astype(np.float32); o[:, 1] = np.abs(o[:, 1]) + 0.5
    tgt = np.array([s[0] for s in SPHERES])[rng.integers(0, len(SPHERES), n)] + rng.normal(size=(n, 3)) * 0.8
    d = (tgt - o); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def _check_queries(sc, n_faces, with_floor):
    o, d = _random_rays(20000, 3)
    tmax = np.full(len(o), np.finfo(np.float32).max, np.float32)
    tmax[::5] = np.random.default_rng(4).uniform(0.5, 6, size=len(tmax[::5])).astype(np.float32)     # maxt-clipped rays
    t, u, v, prim = sc.trace(o, d, tmax)
    ts, ps = sr.closest_f32(o, d, tmax, SPHERES, n_faces)
    if with_floor:                                      # floor plane y = -1 (|x|, |z| < 25), float64: rays whose floor hit comes first
        with np.errstate(all="ignore"):
            tf = (-1.0 - o[:, 1].astype(np.float64)) / d[:, 1]
        tf = np.where((tf > 0) & (tf <= tmax), tf, np.inf)
        floor_first = tf < ts.astype(np.float64) * (1 - 1e-5)
        with np.errstate(invalid="ignore"):
            near_tie = np.abs(tf - ts) <= 1e-5 * np.maximum(ts, 1)
        assert (prim[floor_first & ~near_tie] < n_faces).all()
        keep = ~floor_first & ~near_tie
    else:
        keep = np.ones(len(o), bool)
    assert keep.sum() > 10000
    assert (prim[keep] == ps[keep]).all()
    hit = keep & (ps != NONE)
    assert hit.sum() > 3000 and (u[hit] == 0).all() and (v[hit] == 0).all()
    ulp = np.abs(t[hit].view(np.int32).astype(np.int64) - ts[hit].view(np.int32).astype(np.int64))
    assert ulp.max() <= 2, ulp.max()
    assert np.isinf(t[keep & (ps == NONE)]).all()
    # any hit: the spheres' ray_test, or a floor hit
    ta, _, _, _ = sc.trace(o, d, tmax, any_hit=True)
    occ = np.zeros(len(o), bool)
    for c, r in SPHERES:
        occ |= sr.occluded_f32(o, d, tmax, c, r)
    if with_floor:
        occ_keep = keep & ~np.isfinite(tf)
        assert ((ta[occ_keep] == 0) == occ[occ_keep]).all()
        assert (ta[np.isfinite(tf) & ~near_tie] == 0).all()
    else:
        assert ((ta == 0) == occ).all()


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


def _camera_dirs(size, fov_deg, spp, seed):
    """Directions of a square perspective camera looking down +z in camera space, samples spread uniformly over every pixel
    (the box filter gives each pixel the mean over its own area).  Radially symmetric uses only: flips do not matter."""
    rng = np.random.default_rng(seed)
    tn = np.tan(np.radians(fov_deg) / 2)
    iy, ix = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    jx = rng.random((size, size, spp)); jy = rng.random((size, size, spp))
    x = ((ix[..., None] + jx) / size * 2 - 1) * tn
    y = ((iy[..., None] + jy) / size * 2 - 1) * tn
    d = np.stack([x, y, np.ones_like(x)], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def test_beer_lambert_through_an_index_matched_sphere(mi, monkeypatch):
    """Index-matched glass around a purely absorbing medium under a constant emitter: exp(-sigma_t * chord) per camera ray.  The
    distance-field proofs must not change any lane (a proof that ignored the sphere would walk medium trips through the glass)."""
    s, r, D, size, fov, spp = 0.8, 1.0, 20.0, 16, 7.0, 4096
    xml = scene_xml(sphere_xml((0, 0, 0), r, '<bsdf type="dielectric"><float name="int_ior" value="1.33"/><float name="ext_ior" value="1.33"/></bsdf>'
                               f'<medium type="homogeneous" name="interior"><rgb name="sigma_t" value="{s}"/><rgb name="albedo" value="0"/></medium>'),
                    emitters='<emitter type="constant"><rgb name="radiance" value="1"/></emitter>', integrator='<integrator type="volpath"/>',
                    cam=((0, 0, -D), (0, 0, 0), (0, 1, 0)), fov=fov, size=(size, size), spp=spp)
    sc = mi.load_string(xml)
    img = sc.render(seed=11)[..., :3].astype(np.float64)
    lanes = sc.render_samples(0, size * size * 64, seed=11, spp=64)
    monkeypatch.setenv("LRT_NO_DIST_GRID", "1")
    sc2 = mi.load_string(xml)
    lanes2 = sc2.render_samples(0, size * size * 64, seed=11, spp=64)
    assert (lanes.view(np.uint32) == lanes2.view(np.uint32)).all()
    dirs = _camera_dirs(size, fov, 256, 1)
    o = np.array([0, 0, -D])
    b2 = np.maximum((np.cross(np.broadcast_to(o, dirs.shape), dirs) ** 2).sum(-1), 0)          # squared distance of the line from the centre
    chord = 2 * np.sqrt(np.maximum(r * r - b2, 0))
    ref = np.exp(-s * chord).mean(-1)
    se = np.sqrt(np.maximum(ref * (1 - ref), 1e-12) / spp)
    assert se.max() <= 0.01
    inside = (chord > 0).all(-1)                  # pixels wholly inside the silhouette (the edge pixels depend on the film mapping's details)
    assert inside.sum() > 50
    for ch in range(3):
        z = np.abs(img[..., ch] - ref) / np.maximum(se, 1e-4)
        assert (z[inside] < 4).all(), z[inside].max()
    assert np.abs(img[(chord == 0).all(-1)] - 1).max() < 2e-3


def test_point_light_direct_closed_form(mi):
    """path, max_depth = 2: a diffuse unit sphere on a diffuse floor (y = -1), a point light on the axis above them, the camera
    looking straight down that axis: (a / pi) I max(0, cos) / d^2 per sample, the floor shadowed where the segment to the light
    meets the sphere."""
    I, a, H, size, fov, spp = 10.0, 0.5, 9.0, 64, 50.0, 64
    L = np.array([0.0, 3.0, 0.0])
    xml = scene_xml(FLOOR + sphere_xml((0, 0, 0), 1.0), emitters=f'<emitter type="point"><point name="position" x="0" y="3" z="0"/><rgb name="intensity" value="{I}"/></emitter>',
                    integrator='<integrator type="path"><integer name="max_depth" value="2"/></integrator>',
                    cam=((0, H, 0), (0, 0, 0), (0, 0, 1)), fov=fov, size=(size, size), spp=spp)
    sc = mi.load_string(xml)
    img = sc.render(seed=2)[..., :3].astype(np.float64)
    dc = _camera_dirs(size, fov, 256, 5)
    d = np.stack([dc[..., 0], -dc[..., 2], dc[..., 1]], -1)          # camera +z -> world -y
    o = np.array([0.0, H, 0.0])
    oc = o; bq = (d * oc).sum(-1); cq = (oc * oc).sum() - 1.0
    disc = bq * bq - cq
    ts = np.where(disc >= 0, -bq - np.sqrt(np.maximum(disc, 0)), np.inf)
    tf = (-1.0 - H) / d[..., 1]
    t = np.minimum(ts, tf)
    p = o + d * t[..., None]
    on_sphere = ts < tf
    n = np.where(on_sphere[..., None], p, np.array([0.0, 1.0, 0.0]))
    lv = L - p; dist = np.linalg.norm(lv, axis=-1); l = lv / dist[..., None]
    cos = np.maximum((n * l).sum(-1), 0)
    # shadow: the segment p -> L meets the unit sphere (floor points only; the sphere's lit side sees the light directly)
    bb = (l * p).sum(-1); cc = (p * p).sum(-1) - 1.0; dd = bb * bb - cc
    tn = -bb - np.sqrt(np.maximum(dd, 0))
    shadow = ~on_sphere & (dd > 0) & (tn > 0) & (tn < dist)
    val = np.where(shadow, 0.0, a / np.pi * I * cos / dist ** 2)
    ref = val.mean(-1)
    se = val.std(-1) / np.sqrt(spp) + 1e-4 * ref + 1e-6
    smooth = (on_sphere.all(-1) | (~on_sphere).all(-1)) & (shadow.all(-1) | (~shadow).all(-1))   # no silhouette or shadow edge inside the pixel
    assert smooth.sum() > 300
    z = (np.abs(img - ref[..., None]) / se[..., None])[smooth]
    # the z-scores of ~500 pixels: their mean square near 1 (the SE model holds, no bias), none beyond 5 (false alarm ~3e-4 per run)
    assert (z ** 2).mean() < 1.5 and z.max() < 5, ((z ** 2).mean(), z.max())
    assert ref.max() > 0.05 and (ref[smooth] == 0).any()                  # whole pixels in the shadow ring around the sphere


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
