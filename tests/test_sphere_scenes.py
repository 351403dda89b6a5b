"""CPU tests of sphere shapes and point emitters (src/shapes/sphere.cpp, src/emitters/point.cpp): the description the loader builds,
its case rule for plugin names and its handling of an unnamed shape medium, the errors it keeps, and the float32 restatement of the
sphere ray query against a float64 closed form."""
import numpy as np
import pytest

import sphere_ref as sr

SHAPE_SPHERE, EMITTER_POINT, EMITTER_ENVMAP, EMITTER_CONSTANT = 2, 3, 1, 2
BSDF_DIELECTRIC = 1


def _xform(m, p):
    m = np.array(list(m), np.float64).reshape(4, 4)
    return m[:3, :3] @ np.asarray(p, np.float64) + m[:3, 3]


SMALL = """<scene version="3.0.0">
  <integrator type="{integrator}"/>
  <sensor type="perspective"><float name="fov" value="40"/>
    <transform name="to_world"><lookat origin="0, 0, -5" target="0, 0, 0" up="0, 1, 0"/></transform>
    <film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="16"/></film></sensor>
  <shape type="sphere"><point name="center" x="0.5" y="-0.25" z="1"/><float name="radius" value="0.75"/>{child}</shape>
  {emitters}
</scene>"""


def small(mi, integrator="path", child="", emitters='<emitter type="point"><point name="position" x="1" y="2" z="3"/><rgb name="intensity" value="4"/></emitter>'):
    return mi.load_string(SMALL.format(integrator=integrator, child=child, emitters=emitters))


def test_plugin_type_case_is_ignored(mi):
    """SphereLiverPoint (the fork) says type="Dielectric": the reference finds plugins by file name, on a case-insensitive file system."""
    sc = mi.load_string(SMALL.replace('type="sphere"', 'type="Sphere"').format(
        integrator="Path", child='<bsdf type="Dielectric"/>', emitters='<emitter type="Point"/><emitter type="CONSTANT"/>'))
    d = sc.desc
    assert d.shapes[0].kind == SHAPE_SPHERE and d.shapes[0].n_faces == 0
    b = d.bsdfs[d.shapes[0].bsdf]
    assert b.type == BSDF_DIELECTRIC and b.eta == pytest.approx(np.float32(1.5046) / np.float32(1.000277), rel=1e-6)   # bk7 over air
    assert sorted(d.emitters[i].type for i in range(d.n_emitters)) == [EMITTER_CONSTANT, EMITTER_POINT]


def test_center_radius_and_point_position(mi):
    sc = small(mi)
    d = sc.desc
    s = d.shapes[0]
    assert np.allclose(_xform(s.to_world, (0, 0, 0)), (0.5, -0.25, 1.0))
    assert np.linalg.norm(_xform(s.to_world, (1, 0, 0)) - _xform(s.to_world, (0, 0, 0))) == pytest.approx(0.75)
    e = d.emitters[0]
    assert e.type == EMITTER_POINT and np.allclose(_xform(e.to_world, (0, 0, 0)), (1, 2, 3)) and list(e.radiance) == [4.0] * 3


def test_point_light_beside_an_environment_emitter_loads(mi):
    sc = small(mi, emitters='<emitter type="point"><point name="position" x="1" y="2" z="3"/></emitter><emitter type="constant"/>')
    d = sc.desc
    assert sorted(d.emitters[i].type for i in range(d.n_emitters)) == [EMITTER_CONSTANT, EMITTER_POINT]
    with pytest.raises(RuntimeError, match="Only one environment emitter"):
        small(mi, emitters='<emitter type="constant"/><emitter type="point"/><emitter type="constant"/>')


def test_area_light_on_a_sphere_is_unsupported(mi):
    with pytest.raises(RuntimeError, match="unsupported: an area emitter on a sphere"):
        small(mi, child='<emitter type="area"><rgb name="radiance" value="1"/></emitter>')


def test_prbvolpath_on_spheres_or_point_lights_is_unsupported(mi):
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath"):
        small(mi, integrator="prbvolpath")
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath"):
        small(mi, integrator="prbvolpath", emitters='<emitter type="constant"/>')


def test_unnamed_shape_medium_is_ignored(mi):
    """src/render/shape.cpp:40-49 binds `interior` / `exterior` and ignores any other medium (the fork's SphereLiverCavityEnv has an unnamed one)"""
    sc = small(mi, child='<medium type="homogeneous" name="sideways"/><medium type="homogeneous" name="interior"/>')
    d = sc.desc
    assert d.n_media == 1 and d.shapes[0].interior_medium == 0 and d.shapes[0].exterior_medium == -1


# ------------------------------------------------------------------------------------ the float32 ray query
def _rays(rng, n, center, radius):
    c = np.asarray(center)
    o = (rng.normal(size=(n, 3)) * 3 * radius + c).astype(np.float32)
    tgt = c + rng.normal(size=(n, 3)) * radius * 0.8
    d = (tgt - o).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


@pytest.mark.parametrize("center,radius", [((0.0, 0.0, 0.0), 1.0), ((3.5, -1.25, 10.0), 0.3), ((-20.0, 5.0, 2.0), 7.0)])
def test_sphere_intersection_f32_matches_f64(center, radius):
    rng = np.random.default_rng(7)
    n = 4000
    o, d = _rays(rng, n, center, radius)
    maxt = np.full(n, np.inf, np.float32)
    # inside rays: origins within the sphere (far root)
    oi = (np.asarray(center) + rng.uniform(-0.5, 0.5, size=(n // 4, 3)) * radius).astype(np.float32)
    di = rng.normal(size=(n // 4, 3)); di = (di / np.linalg.norm(di, axis=1, keepdims=True)).astype(np.float32)
    # tangent rays: offset by exactly the radius from the centre, perpendicular to the direction (hit or miss, t near the tangent point)
    dt = rng.normal(size=(n // 4, 3)); dt /= np.linalg.norm(dt, axis=1, keepdims=True)
    perp = np.cross(dt, rng.normal(size=(n // 4, 3))); perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    ot = (np.asarray(center) + perp * radius * (1 + 1e-3) - dt * 4 * radius).astype(np.float32)
    # maxt-clipped rays: the first hit lies beyond maxt (miss), or maxt lies between the two roots (hit)
    oc, dc = o[: n // 4], d[: n // 4]
    t64 = sr.intersect_f64(oc, dc, np.full(n // 4, np.inf), center, radius)
    clip = np.where(np.isfinite(t64), t64 * np.where(np.arange(n // 4) % 2 == 0, 0.5, 1.5), 1.0).astype(np.float32)
    O = np.concatenate([o, oi, ot, oc]); D = np.concatenate([d, di, dt.astype(np.float32), dc]); M = np.concatenate([maxt, maxt[: n // 4], maxt[: n // 4], clip])
    t32 = sr.intersect_f32(O, D, M, center, radius)
    t64 = sr.intersect_f64(O, D, M.astype(np.float64), center, radius)
    # tangent-grazing rays may flip between hit and miss in float32: exclude the 1e-4-wide band around the discriminant's zero
    oc64 = O.astype(np.float64) - np.asarray(center)
    b = (oc64 * D).sum(1); disc = b * b - ((oc64 * oc64).sum(1) - radius ** 2)
    clear = np.abs(disc) > 1e-4 * radius ** 2
    # ... and the maxt-clipped ones whose root sits on maxt itself
    with np.errstate(invalid="ignore"):
        clear &= ~(np.isfinite(M) & (np.abs(t64 - M) < 1e-5 * np.maximum(M, 1)))
    assert clear.mean() > 0.95
    hit32, hit64 = np.isfinite(t32), np.isfinite(t64)
    assert (hit32 == hit64)[clear].all()
    both = clear & hit32 & hit64
    assert both.sum() > 1000
    scale = np.abs(O.astype(np.float64)).max(1) + np.abs(np.asarray(center)).max() + radius + np.where(np.isfinite(t64), t64, 0)   # float32 error grows with the coordinates' magnitude
    err = np.abs(t32[both].astype(np.float64) - t64[both]) / scale[both]
    assert err.max() < 2e-6, err.max()
    # the any-hit test agrees with the closest-hit query
    occ = sr.occluded_f32(O, D, M, center, radius)
    assert (occ == hit64)[clear].all()
    # inside rays always hit (the far root), at a positive distance
    k = slice(n, n + n // 4)
    assert np.isfinite(t32[k]).all() and (t32[k] > 0).all()


# ------------------------------------------------------------------ the fork's three sphere scenes (tests/golden/scenes/, unchanged copies)
import os


@pytest.mark.parametrize("scene", sr.SPHERE_SCENES)
def test_sphere_scene_files_fail_as_in_the_reference(mi, scene):
    """scene.xml: one-entry spectra ("360:0.2464") fail Properties::Spectrum (src/core/properties.cpp:795); scene_temp.xml: parenchyma
    reads sigma_hepatocity with props.get<ScalarFloat> (parenchyma.cpp:145), a wavelength:value spectrum is a type error there
    (include/mitsuba/core/properties.h:832-856)."""
    d = os.path.join(sr.GOLDEN_SCENES, scene)
    with pytest.raises(RuntimeError, match="Spectrum must have at least two entries"):
        mi.load_file(os.path.join(d, "scene.xml"))
    with pytest.raises(RuntimeError, match=r'"sigma_hepatocity" has the wrong type \(expected float, got spectrum\)'):
        mi.load_file(os.path.join(d, "scene_temp.xml"))


@pytest.mark.parametrize("scene", sr.SPHERE_SCENES)
@pytest.mark.parametrize("fname", ["scene.xml", "scene_temp.xml"])
def test_sphere_scene_files_with_rgb_coefficients(mi, scene, fname):
    d = os.path.join(sr.GOLDEN_SCENES, scene)
    sc = mi.load_string(sr.rgb_variant(os.path.join(d, fname)), d)
    desc = sc.desc
    sph = [desc.shapes[i] for i in range(desc.n_shapes) if desc.shapes[i].kind == SHAPE_SPHERE]
    assert len(sph) == 1 and desc.n_faces == 2
    s = sph[0]
    assert np.allclose(_xform(s.to_world, (0, 0, 0)), 0.0)
    assert np.linalg.norm(_xform(s.to_world, (1, 0, 0))) == pytest.approx(1.0)
    b = desc.bsdfs[s.bsdf]                      # SphereLiverPoint's "Dielectric": the defaults, bk7 over air; the others set 1.5 / 1
    eta = np.float32(1.5046) / np.float32(1.000277) if scene == "SphereLiverPoint" else 1.5
    assert b.type == BSDF_DIELECTRIC and b.eta == pytest.approx(eta, rel=1e-6)
    types = sorted(desc.emitters[i].type for i in range(desc.n_emitters))
    if scene == "SphereLiverPoint":
        e = desc.emitters[0]
        assert types == [EMITTER_POINT] and np.allclose(_xform(e.to_world, (0, 0, 0)), (2.5, 0.25, 0.0)) and list(e.radiance) == [10.0] * 3
    else:
        assert types == [EMITTER_CONSTANT if scene == "SphereLiverConstEnv" else EMITTER_ENVMAP]
    if scene == "SphereLiverCavityEnv":         # `<ref id="parenchymaMedium"/>` without a name: ignored (shape.cpp:40-49), hollow glass
        assert s.interior_medium == -1
    else:
        assert desc.media[s.interior_medium].id.decode() == "parenchymaMedium"
