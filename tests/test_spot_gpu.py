"""GPU tests of the spot and directional emitters: the device's emitter sampling (lrt_emitter_probe) against the
float64 restatement of spot_ref.py within the K of spot_cases.py; a tilted spot over a diffuse floor against Lambert's closed form; a
wide spot against a point light through five integrators; a directional light over a floor, with a shadow, and through a slab in single
scattering; and the EXT routing, the aov / moment integrators and the multi-device path."""
import numpy as np
import pytest

import spot_cases as sc_
import spot_ref as sr
pytestmark = pytest.mark.gpu

CASES = sc_.configs()


# ------------------------------------------------------------------------------------------------------- the probe against float64
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.label)
def test_probe_against_float64(mi, case):
    sc = mi.load_string(sc_.scene_xml(case))
    ref_p, smp = sc_.make_inputs(case)
    want = sc_.reference(case, ref_p, smp)
    got = sc.emitter_probe(ref_p, smp)
    ne = len(case.emitters)
    dev = {"p": got["p"], "d": got["d"], "dist": got["dist"], "pdf": got["pdf"], "weight": got["weight"]}
    for k, v in dev.items():                                           # every lane, the ones left out below included
        assert np.isfinite(v).all(), k
    assert (got["weight"] >= 0).all()
    assert np.array_equal(got["emitter"], want["index"])
    worst = sc_.worst_ratios(want, dev)
    print(f"[spot probe] {case.label:14s} " + "  ".join(f"{k} {v:6.2f}" for k, v in worst.items()) + f"  left out {int((~want['ok']).sum())}")
    for k in sc_.QUANTITIES:
        assert worst[k] <= sc_.K[k], (k, worst[k])
    # what holds exactly
    light = want["index"] == 0
    assert (got["pdf"][light] == np.float32(1.0) / np.float32(ne)).all()                      # a delta emitter's pdf is 1 (times the selection's 1 / n)
    if ne == 1:                                                        # no ray hits the light: the hit's emitter pdf and emission are 0
        assert (got["hit_pdf"] == 0).all() and (got["hit_le"] == 0).all()
    e = case.light
    if e.kind == "directional":
        host = np.array(sc.desc.emitters[0].to_world, np.float32).reshape(4, 4)[:3, 2]
        assert np.array_equal(host, e.d)
        assert (got["weight"].view(np.uint32) == e.irradiance.view(np.uint32)[None]).all()
        assert (got["d"].view(np.uint32) == (-host).view(np.uint32)[None]).all() and (got["n"].view(np.uint32) == host.view(np.uint32)[None]).all()
    else:
        assert (got["n"][light] == 0).all() and (got["p"][light] == e.pos[None]).all()
        own = e.sample_direction(ref_p)                                  # the lanes well beyond the cutoff are exactly dark
        dark = light & (own["cos"] < float(e.cos_cutoff) - 1e-6)
        assert dark.sum() >= (0.2 if ne == 1 else 0.1) * len(light) and (got["weight"][dark] == 0).all()


# ------------------------------------------------------------------------------------------------- a spot over a floor, closed form
FLOOR_RHO = np.array([0.6, 0.4, 0.2])
CAM_Z, FOV = 5.0, 40.0


def floor_xml(integrator, emitter, size, spp, extra="", max_depth=2, moment=False, floor_scale=10.0):
    integ = f'<integrator type="{integrator}"><integer name="max_depth" value="{max_depth}"/></integrator>'
    if moment:
        integ = f'<integrator type="moment">{integ}</integrator>'
    return (f'<scene version="3.0.0">{integ}<sensor type="perspective"><float name="fov" value="{FOV}"/>'
            f'<transform name="to_world"><lookat origin="0, 0, {CAM_Z}" target="0, 0, 0" up="0, 1, 0"/></transform>'
            f'<sampler type="independent"><integer name="sample_count" value="{spp}"/></sampler>'
            f'<film type="hdrfilm"><integer name="width" value="{size}"/><integer name="height" value="{size}"/><rfilter type="box"/></film></sensor>'
            f'<shape type="rectangle"><transform name="to_world"><scale value="{floor_scale}"/></transform><bsdf type="diffuse">'
            f'<rgb name="reflectance" value="{", ".join(str(x) for x in FLOOR_RHO)}"/></bsdf></shape>{extra}{emitter}</scene>')


def floor_points(size, sub):
    """the floor points (z = 0) the camera sees at sub x sub midpoints of every pixel: (size, size, sub * sub, 3); the camera looks down -z
    from (0, 0, CAM_Z) with up = +y: film x runs along world +x, film y along world -y (perspective.cpp, transform.h look_at)"""
    t = np.tan(np.radians(FOV) / 2) * CAM_Z
    s = (np.arange(size * sub) + 0.5) / (size * sub)
    x, y = (2 * s - 1) * t, (1 - 2 * s) * t
    X, Y = np.meshgrid(x, y)
    P = np.stack([X, Y, np.zeros_like(X)], -1).reshape(size, sub, size, sub, 3).transpose(0, 2, 1, 3, 4)
    return P.reshape(size, size, sub * sub, 3)


SPOT_ORIGIN, SPOT_TARGET = np.array([1.0, 0.5, 3.0]), np.array([-0.26, 0.23, 0.0])      # (chosen with the lattice check of spot_floor_truth in view)
SPOT_I = 3.0


def tilted_spot():
    z = (SPOT_TARGET - SPOT_ORIGIN) / np.linalg.norm(SPOT_TARGET - SPOT_ORIGIN)
    left = np.cross([0.0, 1.0, 0.0], z); left /= np.linalg.norm(left)
    m = np.eye(4); m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, np.cross(z, left), z, SPOT_ORIGIN
    return sr.Spot("tilted", (SPOT_I,) * 3, 20.0, 10.0, m.astype(np.float32))


def lambert_under(light, P):
    """rho / pi * value * cos at floor points P (..., 3) with normal +z, per channel: (..., 3), and the light's falloff (spots)"""
    flat = P.reshape(-1, 3)
    s = light.sample_direction(flat)
    cos = np.maximum(s["d"][:, 2], 0.0)
    L = (FLOOR_RHO / np.pi)[None] * s["weight"] * cos[:, None]
    return L.reshape(P.shape), s.get("falloff", np.ones(len(flat))).reshape(P.shape[:-1])


@pytest.fixture(scope="module")
def spot_floor_truth():
    size, spp = 32, 256
    light = tilted_spot()
    L, falloff = lambert_under(light, floor_points(size, 16))
    mean, var = L.mean(2), L.var(2)
    kinds = {"core": (falloff == 1).all(2), "dark": (falloff == 0).all(2), "ring": ((falloff > 0) & (falloff < 1)).all(2)}
    assert all(k.sum() >= 4 for k in kinds.values()), {n: int(k.sum()) for n, k in kinds.items()}     # the frame holds core, ring and dark pixels
    # A pixel that the 256 midpoints call dark (mean 0, standard error 0) must be dark all over: the spot is placed so that the cone's rim clips
    # no such pixel's corner.  Checked on a 65 x 65 lattice that includes the pixel's border.
    t = np.tan(np.radians(FOV) / 2) * CAM_Z
    g = (np.arange(size)[:, None] + np.linspace(0, 1, 65)[None]).reshape(-1) / size
    X, Y = np.meshgrid((2 * g - 1) * t, (1 - 2 * g) * t)
    lat = light.sample_direction(np.stack([X, Y, np.zeros_like(X)], -1).reshape(-1, 3))["falloff"].reshape(size, 65, size, 65)
    assert not (kinds["dark"] & (lat > 0).any((1, 3))).any()
    return size, spp, light, mean, np.sqrt(var / spp), kinds


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
def test_spot_over_a_floor(mi, spot_floor_truth, integrator):
    """per pixel L = rho / pi * I * falloff * cos / r^2, averaged in float64 by a 16 x 16 midpoint rule; accepted within 5 standard errors
    of the jitter (the closed form's variance over those 256 points / spp) plus 1e-4 relative for float32; dark pixels are exactly 0"""
    size, spp, light, mean, se, kinds = spot_floor_truth
    sc = mi.load_string(floor_xml(integrator, sc_.emitter_xml(light), size, spp))
    img = sc.render(seed=11).astype(np.float64)[..., :3]
    err = np.abs(img - mean)
    tol = 5 * se + 1e-4 * mean
    worst = (err / np.maximum(tol, 1e-300))[mean > 0].max()
    print(f"[spot floor] {integrator:10s} worst |err| / tol {worst:.3f}  core {int(kinds['core'].sum())} ring {int(kinds['ring'].sum())} dark {int(kinds['dark'].sum())} pixels")
    assert (img[kinds["dark"]] == 0).all()
    assert (err <= tol).all()


# ------------------------------------------------------------------------------------------------- a wide spot equals a point light
WIDE_DEPTH = 6


def wide_xml(integrator, light):
    medium = "liver" if integrator.startswith("bio") else "homogeneous"
    return (f'<scene version="3.0.0"><integrator type="{integrator}"><integer name="max_depth" value="{WIDE_DEPTH}"/><integer name="rr_depth" value="{WIDE_DEPTH + 1}"/></integrator>'
            '<sensor type="perspective"><float name="fov" value="45"/><transform name="to_world"><lookat origin="5, -6, 4" target="0, 0, 1" up="0, 0, 1"/></transform>'
            '<sampler type="independent"><integer name="sample_count" value="16"/></sampler>'
            '<film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="16"/><rfilter type="box"/></film></sensor>'
            '<shape type="rectangle"><transform name="to_world"><scale value="2"/></transform><bsdf type="diffuse"/></shape>'
            f'<shape type="cube"><transform name="to_world"><translate z="1"/></transform><bsdf type="null"/><medium name="interior" type="{medium}">'
            '<rgb name="sigma_t" value="1"/><rgb name="albedo" value="0.8"/></medium></shape>' + light + '</scene>')


WIDE_SPOT = ('<emitter type="spot"><rgb name="intensity" value="400"/><float name="cutoff_angle" value="85"/><float name="beam_width" value="30"/>'
             '<transform name="to_world"><lookat origin="0, 0, 20" target="0, 0, 0" up="0, 1, 0"/></transform></emitter>')
WIDE_POINT = '<emitter type="point"><rgb name="intensity" value="400"/><point name="position" x="0" y="0" z="20"/></emitter>'


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis", "biovolpath", "biovolpath06"])
def test_wide_spot_equals_point_light(mi, integrator):
    """every point a path can reach (the 4 x 4 floor, the 2 x 2 x 2 cube on it) lies within 10 degrees of the axis of a spot whose beam is 30
    wide: falloff == 1.f, and the spot is the point light up to rcp(norm) against rsqrt and a product with 1.  Same seed, no roulette."""
    corners = np.array([[x, y, z] for x in (-2, 2) for y in (-2, 2) for z in (0, 2)], np.float64)
    angle = np.degrees(np.arccos((20.0 - corners[:, 2]) / np.linalg.norm(np.array([0, 0, 20.0]) - corners, axis=1)))
    assert angle.max() < 10.0
    a = mi.load_string(wide_xml(integrator, WIDE_SPOT)).render(seed=7).astype(np.float64)[..., :3]
    b = mi.load_string(wide_xml(integrator, WIDE_POINT)).render(seed=7).astype(np.float64)[..., :3]
    assert np.isfinite(a).all()
    if integrator == "biovolpath06":        # biovolpath06.cpp samples no emitter (its sample_emitter is never called): a delta light adds nothing, here as there
        assert (a == 0).all() and (b == 0).all()
    else:
        assert (b > 0).any()
    rel = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    print(f"[spot = point] {integrator:12s} worst relative difference {rel.max():.3e}  (bound {WIDE_DEPTH * 2.0 ** -20:.3e})  lit pixels {int((b.sum(2) > 0).sum())}")
    assert (rel <= WIDE_DEPTH * 2.0 ** -20).all()


# ------------------------------------------------------------------------------------------------- a directional light over a floor
SUN_DIR, SUN_E = (0.6, 0.0, -0.8), 2.0
SUN = f'<emitter type="directional"><vector name="direction" value="{", ".join(str(x) for x in SUN_DIR)}"/><rgb name="irradiance" value="{SUN_E}"/></emitter>'


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
def test_directional_over_a_floor(mi, integrator):
    """every pixel equals rho / pi * E * cos within 2^-20 relative; under a small opaque rectangle the pixels whose footprint lies wholly in
    the geometric shadow are exactly 0, the ones wholly outside keep the value"""
    size = 32
    sc = mi.load_string(floor_xml(integrator, SUN, size, 4))
    d = np.array(sc.desc.emitters[0].to_world, np.float32).reshape(4, 4)[:3, 2].astype(np.float64)
    want = FLOOR_RHO / np.pi * SUN_E * -d[2]
    img = sc.render(seed=2).astype(np.float64)[..., :3]
    rel = np.abs(img - want) / want
    print(f"[sun floor] {integrator:10s} worst relative error {rel.max():.3e}")
    assert (rel <= 2.0 ** -20).all()
    # the occluder: half-size 0.25 at height 1; its shadow is displaced by d.xy / |d.z|, the camera sees it over the floor points scaled by CAM_Z / (CAM_Z - 1)
    occ = '<shape type="rectangle"><transform name="to_world"><scale value="0.25"/><translate z="1"/></transform><bsdf type="diffuse"/></shape>'
    shadowed = mi.load_string(floor_xml(integrator, SUN, size, 4, extra=occ)).render(seed=2).astype(np.float64)[..., :3]
    P = floor_points(size, 2)                                           # midpoints of 2 x 2 cells; the pixel's own extent is half a cell wider
    half_px = np.tan(np.radians(FOV) / 2) * CAM_Z / size
    shift = d[:2] / -d[2]

    def inside(Q, grow):                                                # per pixel: all (grow < 0) or any (grow > 0) of the footprint within the square
        h = 0.25 + grow * (half_px + 1e-3)
        return (np.abs(Q[..., 0]) <= h) & (np.abs(Q[..., 1]) <= h)
    in_shadow = inside(P[..., :2] - shift, -1).all(2); off_shadow = ~inside(P[..., :2] - shift, +1).any(2)
    hidden = inside(P[..., :2] * ((CAM_Z - 1) / CAM_Z), +1).any(2)      # the occluder itself is in front of these pixels
    assert in_shadow.sum() >= 4 and not (in_shadow & hidden).any()
    assert (shadowed[in_shadow] == 0).all()
    keep = off_shadow & ~hidden
    assert keep.sum() > size * size * 0.8 and (np.abs(shadowed[keep] - want) / want <= 2.0 ** -20).all()


# ------------------------------------------------------------------------------------- a directional light through a slab, single scattering
def test_directional_through_a_slab(mi):
    """a null-BSDF box of isotropic medium, optical thickness 1, albedo 0.8, lit at mu0 and seen at mu, one scattering event (max_depth 2):
    L = albedo E / (4 pi) * mu0 / (mu0 + mu) * (1 - exp(-tau (1 / mu + 1 / mu0))); held by mi.z_test with the moment integrator's variance,
    alpha 0.01 Sidak-corrected, at least 99.75 % of the pixels (DESIGN.md 16.4's acceptance)"""
    size, spp, tau, albedo, E = 16, 256, 1.0, 0.8, 3.0
    sun = f'<emitter type="directional"><vector name="direction" value="0.5, 0.2, -1"/><rgb name="irradiance" value="{E}"/></emitter>'
    xml = (f'<scene version="3.0.0"><integrator type="moment"><integrator type="volpath"><integer name="max_depth" value="2"/></integrator></integrator>'
           '<sensor type="perspective"><float name="fov" value="30"/><transform name="to_world"><lookat origin="0, 0, 6" target="0, 0, 0" up="0, 1, 0"/></transform>'
           f'<sampler type="independent"><integer name="sample_count" value="{spp}"/></sampler>'
           f'<film type="hdrfilm"><integer name="width" value="{size}"/><integer name="height" value="{size}"/><rfilter type="box"/></film></sensor>'
           '<shape type="cube"><transform name="to_world"><scale x="200" y="200" z="0.5"/></transform><bsdf type="null"/>'
           f'<medium name="interior" type="homogeneous"><rgb name="sigma_t" value="{tau}"/><rgb name="albedo" value="{albedo}"/></medium></shape>{sun}</scene>')
    sc = mi.load_string(xml)
    d = np.array(sc.desc.emitters[0].to_world, np.float32).reshape(4, 4)[:3, 2].astype(np.float64)
    mu0 = -d[2]
    # mu per pixel: the cosine of the camera ray to the slab's normal, averaged over 4 x 4 midpoints of the pixel
    t = np.tan(np.radians(30.0) / 2)
    s = (np.arange(size * 4) + 0.5) / (size * 4)
    X, Y = np.meshgrid((2 * s - 1) * t, (1 - 2 * s) * t)
    mu = 1.0 / np.sqrt(1 + X * X + Y * Y)
    L = albedo * E / (4 * np.pi) * mu0 / (mu0 + mu) * (1 - np.exp(-tau * (1 / mu + 1 / mu0)))
    want = L.reshape(size, 4, size, 4).mean((1, 3))
    img = sc.render(seed=4)
    assert np.isfinite(img).all()
    var, mean = mi.moment_variance(img, sc, spp)
    pvals, frac = mi.z_test(mean[..., 1], var[..., 1], want, np.zeros_like(want))         # (grey light and medium: Y = L)
    print(f"[sun slab] pass {frac:.4f}  min p {pvals.min():.3g}  mean of Y {mean[..., 1].mean():.6f}  closed form {want.mean():.6f}")
    assert frac >= 0.9975


# --------------------------------------------------------------------------------------------------------------------- plumbing
def test_spot_scene_runs_on_the_ext_instances(mi):
    light = sc_.emitter_xml(tilted_spot())
    plain = mi.load_string(floor_xml("path", '<emitter type="constant"/>', 8, 4))
    spot = mi.load_string(floor_xml("path", light, 8, 4))
    plain.render(integrator="prbvolpath", spp=1)                      # `ext` seen from outside: prbvolpath has no EXT instances and refuses the scene that selects them
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath on a scene with .*point / spot / directional emitters"):
        spot.render(integrator="prbvolpath", spp=1)
    single = spot.render(seed=5)
    assert single[..., :3].max() > 0
    multi = spot.render_multi([0, 0], seed=5)                         # a repeated device: the rehearsal of lrt_render_multi
    assert np.allclose(multi, single, rtol=1e-6, atol=0)
    aov = mi.load_string(floor_xml("path", light, 8, 4).replace('<integrator type="path">', '<integrator type="aov"><string name="aovs" value="dd.y:depth"/><integrator type="path">')
                         .replace('</integrator><sensor', '</integrator></integrator><sensor'))
    img = aov.render(seed=5)
    assert np.allclose(img[..., :3], single[..., :3], rtol=1e-6, atol=0) and (img[..., -1] >= CAM_Z).all() and (img[..., -1] <= CAM_Z * 1.13).all()
    mom = mi.load_string(floor_xml("path", light, 8, 4, moment=True))
    img = mom.render(seed=5)
    assert np.allclose(img[..., :3], single[..., :3], rtol=1e-6, atol=0) and np.isfinite(img).all()
