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
