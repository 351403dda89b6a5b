"""Pins of the CPU oracle's sphere shapes and point emitters (oracle/orc_scene.cpp, orc_render.cpp), on the CPU.  The oracle is the
twin the device is compared with lane for lane (tests/test_sphere_parity_gpu.py), so it is held here to things that are not the device:
the float32 numpy restatement of sphere.cpp's ray queries and a float64 closed form of them, the traversal order written out as
single rays, float64 geometry of the surface interaction, the point emitter's sample against point.cpp's formulas in float64, and the two
closed-form renders the device's tests use (Beer-Lambert through an index-matched sphere, direct light from a point emitter) with the
same seeds and bounds.  DESIGN.md section 14 lists which of these tests catches which deliberate edit of the oracle."""
import numpy as np
import pytest

import sphere_ref as sr
from sphere_ref import SPHERES, FLOOR, NONE, sphere_xml, scene_xml

FMAX = np.finfo(np.float32).max


def _trace(o, brute):
    return lambda org, d, tmax, any_hit=False: o.trace(org, d, tmax, any_hit=any_hit, brute_force=brute)


# ------------------------------------------------------------------ ray queries
@pytest.mark.parametrize("brute", [True, False], ids=["brute-force", "bvh"])
@pytest.mark.parametrize("with_floor", [False, True], ids=["spheres-only", "spheres-and-floor"])
def test_ray_queries_against_the_numpy_restatement(mi, orc, with_floor, brute):
    """the ray sets and the assertions of tests/test_sphere_gpu.py's query tests, on orc_trace in both of its modes"""
    sc = mi.load_string(scene_xml((FLOOR if with_floor else "") + "".join(sphere_xml(c, r) for c, r in SPHERES)))
    assert sc.desc.n_faces == (2 if with_floor else 0)
    sr.check_queries(_trace(orc.OrcScene(sc), brute), sc.desc.n_faces, with_floor)


def test_closest_hit_from_far_origins(mi, orc):
    """What the plane shift of ray_intersect_preliminary_impl is for: origins 2000 radii away, where C = |o - c|^2 - r^2 of the unshifted
    quadratic cannot hold r^2 (ulp(4e6) = 0.25 .. 0.5).  Against the float64 closed form: rays with an impact parameter below 0.9 r hit,
    and t is within 8 ulp(t): the shifted quadratic's roots are of order r and exact to a few 1e-7, so t inherits the error of plane_t,
    a three-term fma dot product and one division (at most 4 ulp), and of one addition (half an ulp); 8 is twice that."""
    rng = np.random.default_rng(7)
    n = 4000
    c, r = SPHERES[0]
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    side = np.cross(d, rng.normal(size=(n, 3))); side /= np.linalg.norm(side, axis=1, keepdims=True)
    o = (np.asarray(c) - 2000.0 * d + side * rng.uniform(0, 0.9 * r, (n, 1))).astype(np.float32)
    d = d.astype(np.float32)
    tmax = np.full(n, FMAX, np.float32)
    sc = mi.load_string(scene_xml(sphere_xml(c, r)))
    t, _, _, prim = orc.OrcScene(sc).trace(o, d, tmax)
    t64 = sr.intersect_f64(o, d, tmax, c, r)
    b = np.linalg.norm(np.cross(o.astype(np.float64) - c, d.astype(np.float64)), axis=1) / np.linalg.norm(d.astype(np.float64), axis=1)
    assert (b < 0.95 * r).all() and np.isfinite(t64).all()
    assert (prim == 0).all()
    err = np.abs(t.astype(np.float64) - t64) / np.spacing(t64.astype(np.float32)).astype(np.float64)
    assert err.max() <= 8, err.max()


def test_traversal_order(mi, orc):
    """Spheres before triangles, a triangle at equal t wins, the lower sphere index wins, a sphere hit is n_faces + k with u = v = 0:
    single rays whose distances are exact in float32."""
    # a unit sphere tangent to the floor y = -1 (the SphereLiver layout): from the centre straight down both are met at t = 1 exactly
    sc = mi.load_string(scene_xml(FLOOR + sphere_xml((0, 0, 0), 1.0) + sphere_xml((0, 0, 0), 1.0) + sphere_xml((0, 4, 0), 0.5)))
    assert sc.desc.n_faces == 2
    o = orc.OrcScene(sc)
    org = np.float32([[0, 0, 0], [0, 0, 0], [0, 8, 0], [0, 2, 0], [0, 2, 0]])
    d = np.float32([[0, -1, 0], [0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 1, 0]])
    tmax = np.float32([FMAX, FMAX, FMAX, FMAX, 1.0])
    for brute in (True, False):
        t, u, v, prim = o.trace(org, d, tmax, brute_force=brute)
        assert t[0] == 1.0 and prim[0] < 2                        # tangent point: the floor's triangle, not the sphere
        assert t[1] == 1.0 and prim[1] == 2                       # from inside, upwards: the far root, and of two equal spheres the first
        assert t[2] == 3.5 and prim[2] == 4                       # the third sphere (k = 2) in front of the others
        assert np.isinf(t[3]) and prim[3] == NONE                 # between the spheres, sideways: nothing
        assert np.isinf(t[4]) and prim[4] == NONE                 # maxt ends before the sphere above: out of bounds
        assert (u[[1, 2]] == 0).all() and (v[[1, 2]] == 0).all()
        occ = o.trace(org, d, tmax, any_hit=True, brute_force=brute)[0]
        assert (occ[:3] == 0).all() and np.isinf(occ[3:]).all()
    # a segment wholly inside a sphere meets nothing (in_bounds), in both queries
    inside = (np.float32([[0.1, 0, 0]]), np.float32([[1, 0, 0]]), np.float32([0.5]))
    assert o.trace(*inside)[3][0] == NONE and np.isinf(o.trace(*inside, any_hit=True)[0][0])


# ------------------------------------------------------------------ surface interaction
def _probe(o, org, d):
    n = len(org)
    z = np.zeros((n, 3), np.float32)
    return o.bsdf_probe(np.float32(org), np.float32(d), z + 0.5, np.tile(np.float32([[0, 0, 1]]), (n, 1)))


@pytest.mark.parametrize("flip", [False, True], ids=["outward", "flip_normals"])
def test_surface_interaction_float64(mi, orc, flip):
    """p on the sphere, n = +-(p - c) / r, uv = (phi / 2 pi, theta / pi) of the local point, wi = to_local(-d) in a frame whose s lies
    along dp_du = 2 pi r (-sin phi, cos phi, 0), from outside and from inside.  Tolerance: DESIGN.md 13.4, 64 * 2^-23 * (1 + 1 / cos theta_i),
    times the scale of the quantity (the coordinates' magnitude for p, 1 for the unit vectors and uv)."""
    c, r = (0.25, -0.5, 0.5), 1.5
    extra = '<boolean name="flip_normals" value="true"/>' if flip else ""
    sc = mi.load_string(scene_xml(sphere_xml(c, r, extra + '<bsdf type="diffuse"/>')))
    assert sc.desc.shapes[0].flip_normals == int(flip)
    o = orc.OrcScene(sc)
    rng = np.random.default_rng(5)
    n = 4000
    unit = lambda: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(n, 3)))
    tgt = np.asarray(c) + unit() * r * 0.8 * rng.random((n, 1)) ** (1 / 3)                             # a point of the ball: every ray meets the sphere
    org = np.asarray(c) + unit() * r * np.where(rng.random((n, 1)) < 0.5, rng.uniform(2, 5, (n, 1)), rng.uniform(0, 0.6, (n, 1)))   # half outside, half inside
    d = tgt - org; d /= np.linalg.norm(d, axis=1, keepdims=True)
    pr = _probe(o, org, d)
    assert (pr["shape"] == 0).all()
    org32, d32 = np.float32(org).astype(np.float64), np.float32(d).astype(np.float64)
    t64 = sr.intersect_f64(org32, d32, np.full(n, np.inf), c, r)
    P = org32 + d32 * t64[:, None]
    N = (P - c) / r
    cos_i = np.abs((N * d32).sum(1)) / np.linalg.norm(d32, axis=1)
    keep = cos_i > 0.05
    assert keep.sum() > 3000
    tol = 64 * 2.0 ** -23 * (1 + 1 / cos_i[keep])
    scale_p = 1 + np.abs(P).max() + np.abs(org32).max()
    assert (np.abs(pr["t"][keep] - t64[keep]) <= tol * scale_p).all()
    assert (np.abs(pr["p"][keep] - P[keep]).max(1) <= tol * scale_p).all()
    sign = -1.0 if flip else 1.0
    assert (np.abs(pr["n"][keep] - sign * N[keep]).max(1) <= tol).all() and (pr["n"] == pr["sh_n"]).all()
    theta = np.arccos(np.clip(N[:, 2], -1, 1)); phi = np.arctan2(N[:, 1], N[:, 0]); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    pole = np.sin(theta) > 0.05                                     # (phi is ill-conditioned next to the poles: by 1 / sin theta)
    du = np.abs(pr["uv"][:, 0] - phi / (2 * np.pi)); du = np.minimum(du, 1 - du)
    assert (du[keep & pole] <= tol[pole[keep]] / 0.05).all() and (np.abs(pr["uv"][:, 1] - theta / np.pi)[keep & pole] <= tol[pole[keep]] / 0.05).all()
    s = np.stack([-np.sin(phi), np.cos(phi), np.zeros(n)], 1)      # dp_du / |dp_du|, already perpendicular to n
    tt = np.cross(sign * N, s)
    wi = np.stack([-(d32 * s).sum(1), -(d32 * tt).sum(1), -(d32 * sign * N).sum(1)], 1)
    k2 = keep & pole
    assert (np.abs(pr["wi"][k2] - wi[k2]).max(1) <= tol[pole[keep]] / 0.05).all()
    outside = np.linalg.norm(org32 - c, axis=1) > r
    assert ((pr["wi"][keep, 2] > 0) == (outside[keep] != flip)).all()          # the side the ray arrives from, seen through the (flipped) normal


def test_surface_interaction_at_the_poles(mi, orc):
    """rd == 0 exactly: dp_du = 0 and dp_dv = (1, 0, 0) pi r, so the shading frame falls back to coordinate_system(n); everything stays finite"""
    sc = mi.load_string(scene_xml(sphere_xml((0, 0, 0), 1.0, '<bsdf type="diffuse"/>')))
    pr = _probe(orc.OrcScene(sc), [[0, 0, 3], [0, 0, -3]], [[0, 0, -1], [0, 0, 1]])
    assert (pr["t"] == 2.0).all() and np.isfinite(pr["raw"]).all()
    assert (pr["n"] == np.float32([[0, 0, 1], [0, 0, -1]])).all() and (pr["uv"][:, 1] == np.float32([0, 1])).all()
    assert (pr["wi"] == np.float32([[0, 0, 1], [0, 0, 1]])).all()


# ------------------------------------------------------------------ point emitter
def test_point_emitter_sample(mi, orc):
    """point.cpp:119-148 through Scene::sample_emitter_direction: d = (p - ref) / |p - ref|, pdf = 1 times the selection pmf 1 / n,
    weight = n I / |p - ref|^2 (float64, 1e-6 relative), whatever the second sample; next to a constant emitter the first half of the
    first sample's range selects it and the second half the other."""
    I, L = np.array([10.0, 4.0, 2.5]), np.array([0.5, 3.0, -1.0])
    point = (f'<emitter type="point"><point name="position" x="{L[0]}" y="{L[1]}" z="{L[2]}"/>'
             f'<rgb name="intensity" value="{I[0]}, {I[1]}, {I[2]}"/></emitter>')
    rng = np.random.default_rng(2)
    refs = rng.uniform(-3, 3, (200, 3))
    for emitters, ne in ((point, 1), (point + '<emitter type="constant"><rgb name="radiance" value="0.5"/></emitter>', 2)):
        sc = mi.load_string(scene_xml(FLOOR, emitters=emitters))
        assert sc.desc.n_emitters == ne and sc.desc.emitters[0].type == 3
        o = orc.OrcScene(sc)
        for ref in refs:
            ref32 = np.float32(ref).astype(np.float64)
            u1 = rng.random() / ne                                  # the point light's share of the first sample
            d, pdf, w = o.envmap_sample(u1, rng.random(), ref32)
            v = L - ref32; dist2 = (v * v).sum()
            assert np.allclose(d, v / np.sqrt(dist2), rtol=0, atol=1e-6)
            assert pdf == np.float32(1.0 / ne)
            assert np.allclose(w, ne * I / dist2, rtol=1e-6, atol=0)
        if ne == 2:
            d, pdf, w = o.envmap_sample(0.75, 0.3, refs[0])
            assert pdf == np.float32(0.5 / (4 * np.pi)) and np.allclose(w, 2 * 0.5 * 4 * np.pi, rtol=1e-6)


def test_point_light_is_never_hit_and_counts_as_no_environment(mi, orc):
    """Nothing hits a point light and it is no environment: camera rays that miss everything are invalid (alpha 0) and black, with
    hide_emitters or without; the floor below is lit."""
    point = '<emitter type="point"><point name="position" x="0" y="3" z="0"/><rgb name="intensity" value="10"/></emitter>'
    sc = mi.load_string(scene_xml(FLOOR, emitters=point, cam=((0, 1, -20), (0, 1, 0), (0, 1, 0)), size=(16, 16), spp=4))
    o = orc.OrcScene(sc)
    for hide in (False, True):
        lanes = o.render_samples(0, 16 * 16 * 4, hide_emitters=hide)
        sky = lanes[:16 * 4]                                        # the top row looks above the horizon
        assert (sky == 0).all()
        assert (lanes[-16 * 4:, :3] > 0).all() and (lanes[-16 * 4:, 3] == 1).all()


# ------------------------------------------------------------------ closed forms
def test_beer_lambert_through_an_index_matched_sphere(mi, orc):
    """the device's test of the same name (tests/test_sphere_gpu.py) on the oracle: same scene, seed, sample count and bounds"""
    o = orc.OrcScene(mi.load_string(sr.beer_lambert_xml()))
    sr.check_beer_lambert(o.render(seed=11))


def test_point_light_direct_closed_form(mi, orc):
    """the device's test of the same name on the oracle: same scene, seed and bounds"""
    o = orc.OrcScene(mi.load_string(sr.point_light_xml()))
    sr.check_point_light(o.render(seed=2))


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
def test_point_light_beside_a_constant_emitter_closed_form(mi, orc, integrator):
    """max_depth = 2 on a diffuse floor alone, a point light above it and a constant emitter around it: per pixel
    (a / pi) I cos / d^2 + a E.  The point light's term carries the selection pmf (1 / 2 in the pdf, 2 in the weight) and no MIS weight;
    the constant emitter's term is split between emitter sampling and BSDF sampling by MIS and adds up to a E whatever the split.
    64 x 64 pixels at 64 spp; per pixel the standard error of the mean from the float64 model of the sample values is not available in
    closed form for the MIS part, so the bound is on the image mean: each sample lies in [0, 2 (a / pi) I / h^2 + 4 a E] (one emitter is
    chosen per sample, its term doubled; MIS weights are at most 1; the cosine-weighted and the uniform estimator of a E are at most 4 a E
    and 2 a E), so the standard error of the mean of 262144 samples is below that range / 2 / 512; the assertion allows 5 of them, which
    is 2.3 % of the mean: the point light's term is 27 % of it, so half or twice that term (the pmf left out on either side) or I / d (d
    is 3 to 11 here) is far outside."""
    I, a, E, h, size, spp = 10.0, 0.5, 0.25, 3.0, 64, 64
    emitters = (f'<emitter type="point"><point name="position" x="0" y="{h - 1}" z="0"/><rgb name="intensity" value="{I}"/></emitter>'
                f'<emitter type="constant"><rgb name="radiance" value="{E}"/></emitter>')
    xml = scene_xml(FLOOR, emitters=emitters, integrator=f'<integrator type="{integrator}"><integer name="max_depth" value="2"/></integrator>',
                    cam=((0, 9.0, 0), (0, 0, 0), (0, 0, 1)), fov=50.0, size=(size, size), spp=spp)
    img = orc.OrcScene(mi.load_string(xml)).render(seed=3)[..., :3].astype(np.float64)
    dc = sr.camera_dirs(size, 50.0, 64, 5)
    d = np.stack([dc[..., 0], -dc[..., 2], dc[..., 1]], -1)
    p = np.array([0.0, 9.0, 0.0]) + d * ((-1.0 - 9.0) / d[..., 1])[..., None]
    lv = np.array([0.0, h - 1, 0.0]) - p; dist = np.linalg.norm(lv, axis=-1)
    ref = (a / np.pi * I * (lv[..., 1] / dist) / dist ** 2).mean(-1) + a * E
    bound = 5 * (2 * a / np.pi * I / h ** 2 + 4 * a * E) / 2 / 512
    assert bound < 0.025 * ref.mean() and (ref - a * E).mean() > 0.25 * ref.mean()
    for ch in range(3):
        assert abs(img[..., ch].mean() - ref.mean()) <= bound, (img[..., ch].mean(), ref.mean(), bound)


# ------------------------------------------------------------------ what the oracle refuses
def test_render_backward_and_mesh_emitters_are_refused(mi, orc):
    sc = mi.load_string(scene_xml(FLOOR + sphere_xml((0, 0, 0), 1.0)))
    o = orc.OrcScene(sc)
    h, w, c = sc.film_shape()
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath"):
        o.render_backward(np.ones((h, w, c), np.float32))
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath"):
        o.render_samples(0, 16, integrator="prbvolpath")
    mesh_light = '<shape type="cube"><emitter type="area"><rgb name="radiance" value="1"/></emitter></shape>'
    o = orc.OrcScene(mi.load_string(scene_xml(FLOOR + mesh_light, emitters="")))
    with pytest.raises(RuntimeError, match="area emitter on a triangle mesh"):
        o.render(spp=1)
    with pytest.raises(RuntimeError, match="area emitter on a triangle mesh"):
        o.render_samples(0, 16)


# ------------------------------------------------------------------ the random sphere scenes of tests/test_fuzz_gpu.py
def test_sphere_fuzz_seeds_render_on_the_oracle(mi, orc):
    """every seed of the sphere family's list loads, and the oracle renders it to a finite film that is not black; most of them hold a
    sphere or a point light"""
    from conftest import ROOT
    from scene_gen import sphere_fuzz_xml
    from test_fuzz_gpu import SPHERE_SEEDS
    import os
    ext = 0
    for seed in SPHERE_SEEDS:
        xml, _ = sphere_fuzz_xml(seed, os.path.join(ROOT, "scenes", "assets"))
        sc = mi.load_string(xml)
        img, raw = orc.OrcScene(sc).render(return_raw=True, seed=seed)
        assert np.isfinite(raw).all() and (img[..., :3] > 0).any(), seed
        ext += any(sc.desc.shapes[i].kind == 2 for i in range(sc.desc.n_shapes)) or any(sc.desc.emitters[i].type == 3 for i in range(sc.desc.n_emitters))
    assert len(SPHERE_SEEDS) == 24 and ext >= 20


# ------------------------------------------------------------------ the hidden sphere of tests/test_ext_instances_gpu.py, on the oracle
def test_hidden_sphere_on_the_oracle(mi, orc):
    """A sphere inside the closed vault changes no lane, trip or shadow-ray count of the oracle (its own maxt tightening and any-hit order);
    the same sphere outside the vault, in view, changes lanes: the comparison of tests/test_ext_instances_gpu.py can see a difference."""
    import test_ext_instances_gpu as T
    xml, base, defines, cam, (c, half, r) = T.case_scene(mi, "volpath-fog", "independent", None)
    xml_a = T.with_shapes(xml, T.vault_xml(c, half))
    n = T.W * T.H * T.SPP
    oa = orc.OrcScene(mi.load_string(xml_a, base, **defines))
    a = oa.render_samples(0, n, seed=3); sa = dict(oa.last_stats)
    ob = orc.OrcScene(mi.load_string(T.with_shapes(xml_a, T.sphere_xml(c, r)), base, **defines))
    b = ob.render_samples(0, n, seed=3)
    assert (a.view(np.uint32) == b.view(np.uint32)).all() and ob.last_stats == sa
    oc = orc.OrcScene(mi.load_string(T.with_shapes(xml_a, T.sphere_xml((c[0] + 0.6, c[1], c[2] + 0.6), r)), base, **defines))
    differ = (oc.render_samples(0, n, seed=3).view(np.uint32) != a.view(np.uint32)).any(axis=1)
    assert differ.sum() > 10
