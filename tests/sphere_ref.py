"""Numpy restatements of the sphere shape (src/shapes/sphere.cpp) for the tests: the float32 ray query of the device
(ray_intersect_preliminary_impl / ray_test_impl in the `is_diff_v` branch that llvm_ad_rgb takes, solve_quadratic of
include/mitsuba/core/math.h:360-400), the IsDiff surface interaction, and a float64 analytic solution to check them against.
fma is emulated through float64 (the product of two float32 values is exact there), so the float32 chain matches the device's
operation order to within an ulp of double rounding."""
import numpy as np

f32 = np.float32


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def dot(a, b):
    """dmath.h dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(f32)))


def solve_quadratic(a, b, c):
    with np.errstate(all="ignore"):
        linear = a == 0
        valid_linear = linear & (b != 0)
        x_lin = (-c / b).astype(f32)
        discrim = fma(b, b, -((f32(4) * a).astype(f32) * c).astype(f32))
        valid_quad = ~linear & (discrim >= 0)
        sd = np.sqrt(discrim).astype(f32)
        temp = (f32(-0.5) * (b + np.copysign(sd, b)).astype(f32)).astype(f32)
        x0p, x1p = (temp / a).astype(f32), (c / temp).astype(f32)
        x0 = np.where(linear, x_lin, np.fmin(x0p, x1p)).astype(f32)
        x1 = np.where(linear, x_lin, np.fmax(x0p, x1p)).astype(f32)
    return valid_linear | valid_quad, x0, x1


def intersect_f32(o, d, maxt, center, radius):
    """ray_intersect_preliminary_impl: t of the hit (inf: none).  o, d: (n, 3) float32; maxt: (n,)."""
    o, d, maxt = o.astype(f32), d.astype(f32), maxt.astype(f32)
    c = np.asarray(center, f32); r = f32(radius)
    with np.errstate(all="ignore"):
        l = (o - c).astype(f32)
        plane_t = (dot(-l, d) / np.sqrt(dot(d, d)).astype(f32)).astype(f32)
        pp = np.stack([fma(d[:, k], plane_t, o[:, k]) for k in range(3)], 1)
        oo = (pp - c).astype(f32)
        A = dot(d, d); B = (f32(2) * dot(oo, d)).astype(f32); C = (dot(oo, oo) - (r * r).astype(f32)).astype(f32)
        found, near_t, far_t = solve_quadratic(A, B, C)
        near_t = (near_t + plane_t).astype(f32); far_t = (far_t + plane_t).astype(f32)
        out_bounds = ~((near_t <= maxt) & (far_t >= 0))
        in_bounds = (near_t < 0) & (far_t > maxt)
        t = np.where(near_t < 0, far_t, near_t).astype(f32)
    return np.where(found & ~out_bounds & ~in_bounds, t, f32(np.inf)).astype(f32)


def occluded_f32(o, d, maxt, center, radius):
    """ray_test_impl (no plane shift): hit or not."""
    o, d, maxt = o.astype(f32), d.astype(f32), maxt.astype(f32)
    c = np.asarray(center, f32); r = f32(radius)
    with np.errstate(all="ignore"):
        oo = (o - c).astype(f32)
        A = dot(d, d); B = (f32(2) * dot(oo, d)).astype(f32); C = (dot(oo, oo) - (r * r).astype(f32)).astype(f32)
        found, near_t, far_t = solve_quadratic(A, B, C)
        out_bounds = ~((near_t <= maxt) & (far_t >= 0))
        in_bounds = (near_t < 0) & (far_t > maxt)
    return found & ~out_bounds & ~in_bounds


def intersect_f64(o, d, maxt, center, radius):
    """Closed form in float64: the first root in [0, maxt], inf when there is none."""
    o, d, maxt = o.astype(np.float64), d.astype(np.float64), maxt.astype(np.float64)
    oc = o - np.asarray(center, np.float64)
    a = (d * d).sum(1); b = 2 * (oc * d).sum(1); c = (oc * oc).sum(1) - float(radius) ** 2
    disc = b * b - 4 * a * c
    with np.errstate(all="ignore"):
        s = np.sqrt(np.maximum(disc, 0))
        t0 = (-b - s) / (2 * a); t1 = (-b + s) / (2 * a)
    t = np.where(t0 >= 0, t0, t1)
    ok = (disc >= 0) & (t >= 0) & (t <= maxt)
    return np.where(ok, t, np.inf)


def closest_f32(o, d, maxt, spheres, n_faces=0):
    """Closest hit over several spheres (ties: the lower index) -> (t, prim); prim = n_faces + k, 0xffffffff on a miss."""
    t = np.full(len(o), np.inf, f32); prim = np.full(len(o), 0xffffffff, np.uint32)
    for k, (c, r) in enumerate(spheres):
        tk = intersect_f32(o, d, maxt, c, r)
        better = tk < t
        t = np.where(better, tk, t); prim = np.where(better, np.uint32(n_faces + k), prim)
    return t, prim


def surface_f32(o, d, t, center, radius, flip=False):
    """compute_surface_interaction, IsDiff and !follow_shape (sphere.cpp:626-740) for a sphere whose to_world is
    translate(center) * scale(radius): p = ray(t) without re-projection, n = normalize(p - c), uv from dir_to_sph(local),
    the shading frame as for meshes.  Returns p, n (geometric = shading normal), uv, dp_du, dp_dv."""
    o, d, t = o.astype(f32), d.astype(f32), t.astype(f32)
    c = np.asarray(center, f32); r = f32(radius)
    p = np.stack([fma(d[:, k], t, o[:, k]) for k in range(3)], 1)
    pc = (p - c).astype(f32)
    n = (pc * (f32(1) / np.sqrt(dot(pc, pc))).astype(f32)[:, None]).astype(f32)
    inv_r = f32(1.0 / float(r))
    local = np.stack([fma(inv_r, p[:, k], f32(-float(c[k]) / float(r))) for k in range(3)], 1)   # to_object * p (rows: diag 1/r, translation -c/r)
    lx, ly, lz = local[:, 0].astype(np.float64), local[:, 1].astype(np.float64), local[:, 2].astype(np.float64)
    theta = np.arccos(np.clip(lz / np.sqrt(lx * lx + ly * ly + lz * lz), -1, 1))
    phi = np.arctan2(ly, lx); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    uv = np.stack([phi / (2 * np.pi), theta / np.pi], 1)
    rd = np.sqrt(lx * lx + ly * ly)
    with np.errstate(all="ignore"):
        dp_du = np.stack([-ly, lx, np.zeros_like(lx)], 1) * float(r) * 2 * np.pi
        dp_dv = np.stack([lz * lx / rd, lz * ly / rd, -rd], 1) * float(r) * np.pi
    dp_dv = np.where((rd == 0)[:, None], np.array([1.0, 0, 0]) * float(r) * np.pi, dp_dv)
    if flip:
        n = -n
    return p, n, uv, dp_du, dp_dv


# ------------------------------------------------------------------ scenes and ray sets shared by the device's and the oracle's tests
NONE = 0xffffffff
SPHERES = [((0.0, 0.0, 0.0), 1.0), ((2.5, 0.5, 1.0), 0.6)]
FLOOR = ('<shape type="rectangle"><transform name="to_world"><rotate x="1" angle="-90"/><scale x="25" y="1" z="25"/>'
         '<translate x="0" y="-1" z="0"/></transform></shape>')


def sphere_xml(c, r, extra=""):
    return (f'<shape type="sphere"><point name="center" x="{c[0]}" y="{c[1]}" z="{c[2]}"/><float name="radius" value="{r}"/>'
            f'{extra}</shape>')


def scene_xml(shapes, emitters='<emitter type="constant"/>', integrator='<integrator type="path"/>', cam=((0, 3, -8), (0, 0, 0), (0, 1, 0)),
              fov=40, size=(32, 32), spp=4, rfilter="box", sampler="independent", sensor_extra=""):
    (o, t, u) = cam
    return f"""<scene version="3.0.0">{integrator}
  <sensor type="perspective"><float name="fov" value="{fov}"/>
    <transform name="to_world"><lookat origin="{o[0]}, {o[1]}, {o[2]}" target="{t[0]}, {t[1]}, {t[2]}" up="{u[0]}, {u[1]}, {u[2]}"/></transform>
    <sampler type="{sampler}"><integer name="sample_count" value="{spp}"/></sampler>
    <film type="hdrfilm"><integer name="width" value="{size[0]}"/><integer name="height" value="{size[1]}"/><rfilter type="{rfilter}"/></film>{sensor_extra}</sensor>
  {shapes}
  {emitters}
</scene>"""


def random_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-4, 4, size=(n, 3)).astype(np.float32); o[:, 1] = np.abs(o[:, 1]) + 0.5
    tgt = np.array([s[0] for s in SPHERES])[rng.integers(0, len(SPHERES), n)] + rng.normal(size=(n, 3)) * 0.8
    d = (tgt - o); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def check_queries(trace, n_faces, with_floor):
    """`trace(o, d, tmax, any_hit=False)` -> (t, u, v, prim) of a scene holding SPHERES (and FLOOR when with_floor, n_faces = 2) against the
    float32 numpy restatement: primitives equal, t within 2 ulp (fma is emulated through float64 here: double rounding), misses inf, and
    the any-hit query against ray_test_impl."""
    o, d = random_rays(20000, 3)
    tmax = np.full(len(o), np.finfo(np.float32).max, np.float32)
    tmax[::5] = np.random.default_rng(4).uniform(0.5, 6, size=len(tmax[::5])).astype(np.float32)     # maxt-clipped rays
    t, u, v, prim = trace(o, d, tmax)
    ts, ps = closest_f32(o, d, tmax, SPHERES, n_faces)
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
    ta, _, _, _ = trace(o, d, tmax, any_hit=True)
    occ = np.zeros(len(o), bool)
    for c, r in SPHERES:
        occ |= occluded_f32(o, d, tmax, c, r)
    if with_floor:
        occ_keep = keep & ~np.isfinite(tf)
        assert ((ta[occ_keep] == 0) == occ[occ_keep]).all()
        assert (ta[np.isfinite(tf) & ~near_tie] == 0).all()
    else:
        assert ((ta == 0) == occ).all()


# ------------------------------------------------------------------ float64 closed forms of two sphere scenes
def camera_dirs(size, fov_deg, spp, seed):
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


BEER = dict(s=0.8, r=1.0, D=20.0, size=16, fov=7.0, spp=4096)


def beer_lambert_xml(size=None, spp=None):
    """Index-matched glass around a purely absorbing medium under a constant emitter, the camera on the axis"""
    B = BEER
    return scene_xml(sphere_xml((0, 0, 0), B["r"], '<bsdf type="dielectric"><float name="int_ior" value="1.33"/><float name="ext_ior" value="1.33"/></bsdf>'
                                f'<medium type="homogeneous" name="interior"><rgb name="sigma_t" value="{B["s"]}"/><rgb name="albedo" value="0"/></medium>'),
                     emitters='<emitter type="constant"><rgb name="radiance" value="1"/></emitter>', integrator='<integrator type="volpath"/>',
                     cam=((0, 0, -B["D"]), (0, 0, 0), (0, 1, 0)), fov=B["fov"], size=(size or B["size"],) * 2, spp=spp or B["spp"])


def check_beer_lambert(img, spp=None):
    """exp(-sigma_t * chord) per camera ray; every pixel wholly inside the silhouette within 4 standard errors of the per-sample Bernoulli
    model (a sample is 1 or 0: it leaves the absorber or not), the pixels wholly outside equal to the emitter"""
    B = BEER; spp = spp or B["spp"]; size = img.shape[0]
    img = img[..., :3].astype(np.float64)
    dirs = camera_dirs(size, B["fov"], 256, 1)
    o = np.array([0, 0, -B["D"]])
    b2 = np.maximum((np.cross(np.broadcast_to(o, dirs.shape), dirs) ** 2).sum(-1), 0)          # squared distance of the line from the centre
    chord = 2 * np.sqrt(np.maximum(B["r"] ** 2 - b2, 0))
    ref = np.exp(-B["s"] * chord).mean(-1)
    se = np.sqrt(np.maximum(ref * (1 - ref), 1e-12) / spp)
    assert se.max() <= 0.01
    inside = (chord > 0).all(-1)                  # pixels wholly inside the silhouette (the edge pixels depend on the film mapping's details)
    assert inside.sum() > 50
    for ch in range(3):
        z = np.abs(img[..., ch] - ref) / np.maximum(se, 1e-4)
        assert (z[inside] < 4).all(), z[inside].max()
    assert np.abs(img[(chord == 0).all(-1)] - 1).max() < 2e-3


POINT = dict(I=10.0, a=0.5, H=9.0, size=64, fov=50.0, spp=64, L=(0.0, 3.0, 0.0))


def point_light_xml():
    """path, max_depth = 2: a diffuse unit sphere on a diffuse floor (y = -1), a point light on the axis above them, the camera
    looking straight down that axis"""
    P = POINT
    return scene_xml(FLOOR + sphere_xml((0, 0, 0), 1.0), emitters=f'<emitter type="point"><point name="position" x="{P["L"][0]:g}" y="{P["L"][1]:g}" z="{P["L"][2]:g}"/><rgb name="intensity" value="{P["I"]}"/></emitter>',
                     integrator='<integrator type="path"><integer name="max_depth" value="2"/></integrator>',
                     cam=((0, P["H"], 0), (0, 0, 0), (0, 0, 1)), fov=P["fov"], size=(P["size"],) * 2, spp=P["spp"])


def check_point_light(img):
    """(a / pi) I max(0, cos) / d^2 per sample, the floor shadowed where the segment to the light meets the sphere"""
    P = POINT; I, a, H, size, fov, spp = P["I"], P["a"], P["H"], P["size"], P["fov"], P["spp"]
    L = np.array(P["L"])
    img = img[..., :3].astype(np.float64)
    dc = camera_dirs(size, fov, 256, 5)
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


# ------------------------------------------------------------------ the fork's sphere scene files
GOLDEN_SCENES = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "scenes")
SPHERE_SCENES = ("SphereLiverPoint", "SphereLiverConstEnv", "SphereLiverCavityEnv")


def rgb_variant(path):
    """The text of a SphereLiver scene file with its parenchyma's wavelength:value spectra replaced by the plugin's defaults (1.0).
    Neither file loads in the reference (sigma_hepatocity is read as a float, src/media/parenchyma.cpp:145; scene.xml's
    one-entry spectra fail Properties::Spectrum).  The replaced properties feed only the bio integrators' element competition:
    path / volpath / volpathmis see parenchyma's constant sigma_t (parenchyma.cpp:163-165), so their renders do not depend on them."""
    import re
    xml = open(path).read()
    xml = re.sub(r'<spectrum name="sigma_hepatocity" value="[^"]*"\s*/>', '<float name="sigma_hepatocity" value="1"/>', xml)
    return re.sub(r'<spectrum name="(\w+)" value="[^"]*"\s*/>', r'<rgb name="\1" value="1"/>', xml)
