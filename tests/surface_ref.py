"""Float64 reference of surface scattering, numpy only, written from optics and from the plugins' documented behaviour, not from
csrc/dshade.h or the oracle: Fresnel's equations and Snell's law in world-space vectors, the Lambertian lobe on the concentric-disk
map, the checkerboard, the bump-mapped normal as the normal of the displaced surface, the bump-terminator shadowing term of
Estevez et al. (Ray Tracing Gems 2019, ch. 12), the plane-parallel plate and the glass sphere.

Conventions: `d` is the direction a ray travels (towards the surface), `n` the geometric normal of the surface (pointing to the
exterior side of a dielectric), `eta` = interior / exterior index.  The direction "towards the viewer" is wi = -d.  Everything is
in world space; the only local quantity is a cosine against a normal."""
import struct
import zlib

import numpy as np

EPS = 2.0 ** -23            # spacing of float32 at 1
F_DELTA, F_SMOOTH = 1, 2    # the probe's sampled_type values


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def dot(a, b):
    return np.sum(np.asarray(a, np.float64) * np.asarray(b, np.float64), axis=-1)


# ------------------------------------------------------------------------------------------------------------------ Fresnel
def fresnel(cos_i, n_i, n_t):
    """Unpolarized reflectance of a plane interface for light arriving at cos_i >= 0 in index n_i, leaving into n_t:
    R = (r_s^2 + r_p^2) / 2 with r_s = (n_i cos_i - n_t cos_t) / (n_i cos_i + n_t cos_t), r_p = (n_t cos_i - n_i cos_t) / (n_t cos_i + n_i cos_t)
    (Born & Wolf 1.5.2), cos_t from Snell's law n_i sin_i = n_t sin_t; total internal reflection (R = 1, cos_t = 0) when sin_t >= 1.
    Returns (R, cos_t >= 0)."""
    cos_i = np.asarray(cos_i, np.float64); n_i = np.asarray(n_i, np.float64) + 0 * cos_i; n_t = np.asarray(n_t, np.float64) + 0 * cos_i
    sin_t2 = (n_i / n_t) ** 2 * (1 - cos_i ** 2)
    tir = sin_t2 >= 1
    cos_t = np.sqrt(np.where(tir, 0, 1 - sin_t2))
    with np.errstate(invalid="ignore", divide="ignore"):
        r_s = (n_i * cos_i - n_t * cos_t) / (n_i * cos_i + n_t * cos_t)
        r_p = (n_t * cos_i - n_i * cos_t) / (n_t * cos_i + n_i * cos_t)
    R = np.where(tir | (cos_i == 0), 1.0, 0.5 * (r_s ** 2 + r_p ** 2))
    R = np.where(n_i == n_t, 0.0, R)
    return R, cos_t


def reflect(d, n):
    """mirror direction of a ray travelling along d at a surface of normal n (either orientation)"""
    d = np.asarray(d, np.float64); n = np.asarray(n, np.float64)
    return d - 2 * dot(d, n)[..., None] * n


def refract(d, n, n_i, n_t):
    """Snell's law in vector form: the transmitted direction of a ray travelling along d (unit) from index n_i into n_t through a
    surface of unit normal n (either orientation).  t = r d + (r c - cos_t) m with r = n_i / n_t, m the normal against d, c = -d.m.
    Rows under total internal reflection come back as NaN."""
    d = np.asarray(d, np.float64); n = np.asarray(n, np.float64)
    m = np.where((dot(d, n) > 0)[..., None], -n, n)
    c = -dot(d, m)
    r = np.asarray(n_i, np.float64) / np.asarray(n_t, np.float64)
    k = 1 - r * r * (1 - c * c)
    with np.errstate(invalid="ignore"):
        cos_t = np.sqrt(np.where(k > 0, k, np.nan))
    return (r * np.ones_like(c))[..., None] * d + (r * c - cos_t)[..., None] * m


def dielectric_sample(d, n, eta, reflect_it):
    """A smooth dielectric (interior / exterior index eta, n towards the exterior) hit by a camera-side ray travelling along d, in
    radiance transport.  reflect_it: per ray, take the reflected (True) or the refracted (False) lobe; under total internal reflection
    only the reflected one exists and is taken whatever reflect_it says.
    Returns a dict: wo (world), R, pdf (R or 1 - R), eta (n_t / n_i for a refraction, 1 for a reflection), weight ((n_i / n_t)^2 for a
    refraction: radiance along a ray scales with the square of the index, L / n^2 is invariant; 1 for a reflection), cos_t, tir,
    reflected."""
    d = unit(d); n = np.asarray(n, np.float64) + 0 * d
    outside = -dot(d, n) >= 0                      # the viewer side is the exterior
    n_i = np.where(outside, 1.0, eta); n_t = np.where(outside, eta, 1.0)
    cos_i = np.abs(dot(d, n))
    R, cos_t = fresnel(cos_i, n_i, n_t)
    tir = R >= 1
    refl = np.asarray(reflect_it, bool) | tir
    with np.errstate(invalid="ignore"):
        wo = np.where(refl[..., None], reflect(d, n), refract(d, n, n_i, n_t))
    return {"wo": wo, "R": R, "pdf": np.where(refl, R, 1 - R), "eta": np.where(refl, 1.0, n_t / n_i), "weight": np.where(refl, 1.0, (n_i / n_t) ** 2),
            "cos_t": cos_t, "tir": tir, "reflected": refl, "cond": 1 + 1 / np.maximum(cos_t, 1e-300) * (~tir)}


# ------------------------------------------------------------------------------------------------------------------ diffuse
def concentric_disk(u1, u2):
    """Shirley & Chiu, "A low distortion map between disk and square" (1997): (u1, u2) in [0, 1)^2 -> the unit disk"""
    x = 2 * np.asarray(u1, np.float64) - 1; y = 2 * np.asarray(u2, np.float64) - 1
    first = np.abs(x) >= np.abs(y)                 # the wedges around the x axis: radius x, angle (pi / 4) y / x
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(first, x, y)
        phi = np.where(first, (np.pi / 4) * y / x, np.pi / 2 - (np.pi / 4) * x / y)
    phi = np.where((x == 0) & (y == 0), 0.0, phi)
    return r * np.cos(phi), r * np.sin(phi)


def cosine_hemisphere(u1, u2):
    """Malley's method on the concentric map: local direction (x, y, z), density z / pi"""
    x, y = concentric_disk(u1, u2)
    return np.stack([x, y, np.sqrt(np.maximum(1 - x * x - y * y, 0))], -1)


def diffuse_eval(rho, cos_i, cos_o):
    """Lambert: f cos_o = rho cos_o / pi on the front side (both cosines positive), zero elsewhere.  rho: (..., 3).  Returns (value, pdf)."""
    on = (np.asarray(cos_i) > 0) & (np.asarray(cos_o) > 0)
    pdf = np.where(on, np.asarray(cos_o, np.float64) / np.pi, 0.0)
    return np.asarray(rho, np.float64) * pdf[..., None], pdf


def checkerboard(uv, to_uv, color0, color1, edge=1e-4):
    """The checkerboard texture: (s, t) = to_uv (u, v, 1); cells of half a unit, color0 where the two cell parities agree.  to_uv is the
    2 x 3 (or 3 x 3) affine map.  Returns (colour (n, 3), near: within `edge` of a cell border in s or t)."""
    uv = np.asarray(uv, np.float64); M = np.asarray(to_uv, np.float64)
    st = uv @ M[:2, :2].T + M[:2, 2]
    f = st - np.floor(st)
    upper = f > 0.5
    same = upper[:, 0] == upper[:, 1]
    near = (np.minimum(np.minimum(f, 1 - f), np.abs(f - 0.5)) < edge).any(1)
    return np.where(same[:, None], np.asarray(color0, np.float64), np.asarray(color1, np.float64)), near


# ----------------------------------------------------------------------------------------------------------------- textures
def read_png8(path):
    """the 8-bit samples of a non-interlaced PNG (colour types 0, 2, 4, 6), as (h, w, channels) uint8 (PNG specification, 2nd ed.)"""
    b = open(path, "rb").read()
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(b):
        n, tag = struct.unpack(">I4s", b[pos:pos + 8]); body = b[pos + 8:pos + 8 + n]; pos += 12 + n
        if tag == b"IHDR": hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT": idat += body
    w, h, depth, ctype, _, _, interlace = hdr
    assert depth == 8 and interlace == 0 and ctype in (0, 2, 4, 6)
    c = {0: 1, 2: 3, 4: 2, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * c)
    out = np.zeros((h, w * c), np.int64)
    for y in range(h):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(w * c, np.int64)
        for x in range(w * c):
            a = out[y, x - c] if x >= c else 0
            ul = up[x - c] if x >= c else 0
            if ft == 0: p = 0
            elif ft == 1: p = a
            elif ft == 2: p = up[x]
            elif ft == 3: p = (a + up[x]) // 2
            else:
                q = a + up[x] - ul; pa, pb, pc = abs(q - a), abs(q - up[x]), abs(q - ul)
                p = a if (pa <= pb and pa <= pc) else (up[x] if pb <= pc else ul)
            out[y, x] = (line[x] + p) & 255
    return out.reshape(h, w, c).astype(np.uint8)


def srgb_to_linear(v):
    """IEC 61966-2-1: the electro-optical transfer function of sRGB, v in [0, 1]"""
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def srgb_from_linear(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.0031308, v * 12.92, 1.055 * np.maximum(v, 0) ** (1 / 2.4) - 0.055)


def height_texels(png8):
    """What a bitmap texture holds of an 8-bit sRGB file: per channel linear light, stored as half floats; the height of an RGB file is
    its Rec. 709 luminance.  Returns (h, w) float64."""
    lin = srgb_to_linear(png8[..., :3 if png8.shape[2] >= 3 else 1].astype(np.float64) / 255).astype(np.float16).astype(np.float64)
    if lin.shape[2] == 1:
        return lin[..., 0]
    # (the luminance is formed in float32 from the stored halves: one more rounding, 2^-24 relative, which the tolerance of the normal carries)
    return lin @ np.array([0.212671, 0.715160, 0.072169])


class HeightMap:
    """h(u, v): bilinear, repeat-wrapped reconstruction of texels (rows = v) with centres at ((i + .5) / w, (j + .5) / h), under to_uv"""

    def __init__(self, texels, to_uv=None):
        self.t = np.asarray(texels, np.float64); self.h, self.w = self.t.shape
        self.to_uv = np.array([[1, 0, 0], [0, 1, 0]], np.float64) if to_uv is None else np.asarray(to_uv, np.float64)[:2]

    def st(self, uv):
        return np.asarray(uv, np.float64) @ self.to_uv[:, :2].T + self.to_uv[:, 2]

    def tex(self, st):
        """the interpolant at texture coordinates (s, t)"""
        x = st[:, 0] * self.w - 0.5; y = st[:, 1] * self.h - 0.5
        ix = np.floor(x).astype(np.int64); iy = np.floor(y).astype(np.int64)
        fx = x - ix; fy = y - iy
        g = lambda j, i: self.t[np.mod(j, self.h), np.mod(i, self.w)]
        return (1 - fy) * ((1 - fx) * g(iy, ix) + fx * g(iy, ix + 1)) + fy * ((1 - fx) * g(iy + 1, ix) + fx * g(iy + 1, ix + 1))

    def __call__(self, uv):
        return self.tex(self.st(uv))

    def cell_margin(self, uv):
        """distance, in texels, of each point from the nearest line through texel centres (where the gradient jumps)"""
        st = self.st(uv)
        x = st[:, 0] * self.w - 0.5; y = st[:, 1] * self.h - 0.5
        fx = x - np.floor(x); fy = y - np.floor(y)
        return np.minimum(np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy))

    def gradient(self, uv, margin, renderer_chain_rule=False):
        """(h_u, h_v) by central differences of the interpolant with a step that stays inside the bilinear cell of each point: the
        interpolant is linear along s and along t inside a cell, and (s, t) is affine in (u, v), so the difference quotient is the exact
        derivative there.  `margin` = cell_margin(uv) (points with margin 0 have no gradient).

        renderer_chain_rule: the reference renderer's bitmap texture does not form this derivative when the map is not square AND
        to_uv mixes u and v.  It takes the differences per texel step (f_x, f_y), applies to_uv's transpose to them, and only then
        scales by the resolution: h_u = w (M00 f_x + M10 f_y), h_v = h (M01 f_x + M11 f_y), where calculus has
        h_u = M00 w f_x + M10 h f_y, h_v = M01 w f_x + M11 h f_y.  The two agree when w = h or M01 = M10 = 0.  With the flag set, the
        same central differences (taken along s and t) are combined the renderer's way."""
        uv = np.asarray(uv, np.float64)
        if renderer_chain_rule:
            st = self.st(uv); M = self.to_uv
            es = 0.5 * margin / self.w; et = 0.5 * margin / self.h
            zs = np.zeros_like(st); zs[:, 0] = es
            zt = np.zeros_like(st); zt[:, 1] = et
            f_x = (self.tex(st + zs) - self.tex(st - zs)) / (2 * es) / self.w          # per texel step
            f_y = (self.tex(st + zt) - self.tex(st - zt)) / (2 * et) / self.h
            return self.w * (M[0, 0] * f_x + M[1, 0] * f_y), self.h * (M[0, 1] * f_x + M[1, 1] * f_y)
        # a step of e in u moves (s, t) by to_uv[:, 0] e: keep |ds| w and |dt| h below half the margin
        out = []
        for k in range(2):
            reach = np.abs(self.to_uv[0, k]) * self.w + np.abs(self.to_uv[1, k]) * self.h
            e = 0.5 * margin / max(reach, 1e-300)
            step = np.zeros_like(uv); step[:, k] = e
            out.append((self(uv + step) - self(uv - step)) / (2 * e))
        return out[0], out[1]


# ----------------------------------------------------------------------------------------------------------------- bump map
def bump_normal(n, dp_du, dp_dv, scale, h_u, h_v, wi):
    """The shading normal of a bump-mapped surface: the normal of the displaced surface p(u, v) + scale h(u, v) n, whose tangents are
    dp_du + n scale h_u and dp_dv + n scale h_v (the derivative of n is dropped, as bump mapping does: Blinn 1978); oriented to the
    geometric normal n; and, when it faces away from the viewer direction wi while n faces it (or the other way round), mirrored
    about n (its tangential part reversed), so that wi sees the perturbed surface from the side it sees the real one.
    Returns (normal, mirrored)."""
    n = np.asarray(n, np.float64)
    a = np.asarray(dp_du, np.float64) + n * (scale * np.asarray(h_u))[..., None]
    b = np.asarray(dp_dv, np.float64) + n * (scale * np.asarray(h_v))[..., None]
    m = unit(np.cross(a, b))
    m = np.where((dot(m, n) < 0)[..., None], -m, m)
    mirrored = dot(wi, n) * dot(wi, m) <= 0
    m = np.where(mirrored[..., None], 2 * dot(m, n)[..., None] * n - m, m)
    return m, mirrored


def tan2(c):
    c = np.asarray(c, np.float64)
    with np.errstate(divide="ignore"):
        return np.maximum(1 - c * c, 0) / (c * c)


def shadow_terminator(cos_nn, cos_wo):
    """Estevez, Lecocq, Kulla, "A microfacet-based shadowing function to solve the bump terminator problem" (RTG 2019): GGX
    shadowing G1(wo) = 2 / (1 + sqrt(1 + alpha^2 tan^2(theta_o))) with alpha^2 = min(tan^2(theta_d) / 8, 1), theta_d the angle
    between the perturbed and the true shading normal, theta_o that of wo to the true one.  Arguments: the two cosines."""
    a2 = np.minimum(tan2(cos_nn) / 8, 1)
    return 2 / (1 + np.sqrt(1 + a2 * tan2(cos_wo)))


def bumped_diffuse_eval(rho, n, m, wi, wo):
    """diffuse nested in a bump map: Lambert about the perturbed normal m, times the terminator, and zero where wo lies on different
    sides of the true and the perturbed surface.  Returns (value, pdf, cond): cond = 1 + tan^2(theta_o) (the terminator's sensitivity)."""
    val, pdf = diffuse_eval(rho, dot(wi, m), dot(wo, m))
    ok = dot(wo, n) * dot(wo, m) > 0
    g = shadow_terminator(dot(m, n), dot(wo, n))
    return val * (g * ok)[..., None], pdf * ok, 1 + np.minimum(tan2(dot(wo, n)), 1e30)


def bumped_dielectric_sample(d, n, m, eta, reflect_it):
    """dielectric nested in a bump map: reflection / refraction about the perturbed normal m; the weight carries the terminator and is
    exactly zero when the outgoing direction is not on the same side of the true surface as of the perturbed one"""
    r = dielectric_sample(d, m, eta, reflect_it)
    wo = r["wo"]
    side = dot(wo, m) * dot(wo, n)
    r["masked"] = ~(side > 0)
    r["side"] = side
    r["weight"] = np.where(r["masked"], 0.0, r["weight"] * shadow_terminator(dot(m, n), dot(wo, n)))
    r["tcond"] = 1 + np.minimum(tan2(dot(wo, n)), 1e30)
    return r


# ----------------------------------------------------------------------------------------------------------- closed forms
def plate(R):
    """A plane-parallel plate of single-interface reflectance R (the same at both faces, by reversibility), all orders of internal
    reflection summed incoherently: T_tot = (1 - R)^2 / (1 - R^2) = (1 - R) / (1 + R), R_tot = R + (1 - R)^2 R / (1 - R^2) = 2 R / (1 + R)."""
    R = np.asarray(R, np.float64)
    return (1 - R) / (1 + R), 2 * R / (1 + R)


def glass_sphere(o, d, center, radius, eta, orders):
    """A ray (o, d) that meets a glass sphere.  Returns (hit, d_reflect, R, [d_k], [w_k]) for k = 0 .. orders - 1: the directly reflected
    direction with weight R, and the exit directions after refracting in, k internal reflections and refracting out, with weights
    (1 - R)^2 R^k (the angle of incidence repeats at every internal hit, and R is the same from either side).  Radiance is unchanged
    by the two refractions together: (1 / eta)^2 eta^2 = 1."""
    o = np.asarray(o, np.float64); d = unit(d); c = np.asarray(center, np.float64)
    oc = o - c
    b = dot(oc, d); disc = b * b - (dot(oc, oc) - radius * radius)
    hit = disc > 0
    t = -b - np.sqrt(np.where(hit, disc, 0))
    p = o + t[..., None] * d
    n = (p - c) / radius
    R, _ = fresnel(np.abs(dot(d, n)), 1.0, eta)
    d_r = reflect(d, n)
    with np.errstate(invalid="ignore"):
        din = refract(d, n, 1.0, eta)
    dirs, ws = [], []
    for k in range(orders):
        # the chord to the next hit
        p = p + (-2 * dot(din, n))[..., None] * radius * din
        n = unit(p - c); p = c + radius * n                              # (back onto the sphere: the rounding of a chord does not feed the next one)
        with np.errstate(invalid="ignore"):
            dirs.append(refract(din, n, eta, 1.0)); ws.append((1 - R) ** 2 * R ** k)
        din = unit(reflect(din, n))
    return hit, d_r, R, dirs, ws
