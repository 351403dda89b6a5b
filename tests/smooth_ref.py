"""Float64 numpy restatement of the smooth conductor, the smooth plastic and the two-sided adapter, by source
line of the renderer this project follows: src/bsdfs/conductor.cpp:226-330, plastic.cpp:160-365, twosided.cpp:74-307,
include/mitsuba/render/fresnel.h:35-71 (fresnel), :92-117 (fresnel_conductor), :327-355 (fresnel_diffuse_reflectance), and the host
constants of plastic.cpp:192-207.  Every function takes the working type T (np.float64, or np.float32 for the run that K is made
from: smooth_cases.py), like rough_ref.py and spot_ref.py.  Directions are (n, 3) arrays in the local shading frame, uv is (n, 2).

A BSDF here is an object with
    sample(wi, s1, s2, uv, T) -> dict(wo, pdf, eta, type, weight, wi_margin, lobe_margin, tex_margin)
    eval_pdf(wi, wo, uv, T)   -> (eval (n, 3), pdf (n,), margin (n,))
    albedo(wi, uv, T)         -> (n, 3)        BSDF::eval_diffuse_reflectance
    flags                     -> F_DELTA | F_SMOOTH bits
The margins are distances to the nearest branch of the formulas (cos theta against 0, s1 against the lobe threshold, uv against a
checkerboard edge): a lane closer to one than the stated margin may legitimately take the other branch in float32."""
import numpy as np

EPS = 2.0 ** -23
F_DELTA, F_SMOOTH, F_NULL = 1, 2, 4
INF = np.inf

IOR = {"vacuum": 1.0, "air": 1.000277, "water": 1.3330, "polypropylene": 1.49, "bk7": 1.5046, "acrylic glass": 1.49, "diamond": 2.419}


def _f(T, x):
    return np.asarray(x, T)


# --------------------------------------------------------------------------------------------------------------- fresnel.h
def fresnel(cos_theta_i, eta, T=np.float64):
    """fresnel.h:35-71: the reflection coefficient F of a dielectric boundary (cos_theta_t, eta_it, eta_ti are not needed here)"""
    c = _f(T, cos_theta_i); eta = T(eta)
    outside = c >= 0
    rcp_eta = T(1) / eta
    eta_it = np.where(outside, eta, rcp_eta); eta_ti = np.where(outside, rcp_eta, eta)
    cos_theta_t_sqr = T(1) - (T(1) - c * c) * (eta_ti * eta_ti)
    ci = np.abs(c); ct = np.sqrt(np.maximum(cos_theta_t_sqr, T(0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        a_s = (ci - eta_it * ct) / (ci + eta_it * ct)
        a_p = (ct - eta_it * ci) / (ct + eta_it * ci)
    r = T(0.5) * (a_s * a_s + a_p * a_p)
    special = (eta == 1) | (ci == 0)
    return np.where(special, T(0) if eta == 1 else T(1), r).astype(T)


def fresnel_conductor(cos_theta_i, eta_r, eta_i, T=np.float64):
    """fresnel.h:92-117, eta = eta_r + i eta_i"""
    c = _f(T, cos_theta_i); eta_r = _f(T, eta_r); eta_i = _f(T, eta_i)
    c2 = c * c; s2 = T(1) - c2; s4 = s2 * s2
    temp_1 = eta_r * eta_r - eta_i * eta_i - s2
    a_2_pb_2 = np.sqrt(np.maximum(temp_1 * temp_1 + T(4) * eta_i * eta_i * eta_r * eta_r, T(0)))
    a = np.sqrt(np.maximum(T(0.5) * (a_2_pb_2 + temp_1), T(0)))
    term_1 = a_2_pb_2 + c2; term_2 = T(2) * c * a
    r_s = (term_1 - term_2) / (term_1 + term_2)
    term_3 = a_2_pb_2 * c2 + s4; term_4 = term_2 * s2
    r_p = r_s * (term_3 - term_4) / (term_3 + term_4)
    return (T(0.5) * (r_s + r_p)).astype(T)


FDR_1 = (0.0636, 0.6681, 0.7099, -1.4399)                                     # approx_1 = 0.0636 / eta + 0.6681 + eta (0.7099 - 1.4399 eta)
FDR_2 = (0.919317, -3.4793, 6.75335, -7.80989, 4.98554, -1.36881)            # approx_2 = horner(1 / eta, ...)


def fresnel_diffuse_reflectance(eta, T=np.float64):
    """fresnel.h:327-355"""
    eta = T(eta); inv_eta = T(1) / eta
    approx_1 = T(FDR_1[0]) * inv_eta + (eta * (eta * T(FDR_1[3]) + T(FDR_1[2])) + T(FDR_1[1]))
    approx_2 = T(FDR_2[5])
    for c in FDR_2[4::-1]:
        approx_2 = approx_2 * inv_eta + T(c)
    return T(approx_1 if eta < 1 else approx_2)


# --------------------------------------------------------------------------------------------------------------- textures
class Tex:
    """an RGB value, or a checkerboard of two RGB values with to_uv = scale (src/textures/checkerboard.cpp:70-88)"""

    def __init__(self, color0, color1=None, scale=1.0):
        c = lambda v: np.broadcast_to(np.asarray(v, np.float32), (3,)).astype(np.float32)      # the loader stores float32
        self.color0 = c(color0); self.color1 = None if color1 is None else c(color1); self.scale = float(scale)

    def mean(self, T=np.float64):
        """Texture::mean(): srgb.cpp:117-122 (the mean of the three channels), checkerboard.cpp:112-114"""
        m = lambda v: (T(v[0]) + T(v[1]) + T(v[2])) * (T(1) / T(3))
        return m(self.color0) if self.color1 is None else T(0.5) * (m(self.color0) + m(self.color1))

    def eval(self, uv, T=np.float64):
        n = len(uv)
        if self.color1 is None:
            return np.broadcast_to(self.color0.astype(T), (n, 3)).copy()
        u = _f(T, uv[:, 0]) * T(self.scale); v = _f(T, uv[:, 1]) * T(self.scale)
        mx = u - np.floor(u) > T(0.5); my = v - np.floor(v) > T(0.5)
        return np.where((mx == my)[:, None], self.color0.astype(T)[None], self.color1.astype(T)[None])

    def margin(self, uv):
        """distance of uv from the nearest edge of the board, in uv units (inf for a plain value)"""
        if self.color1 is None:
            return np.full(len(uv), INF)
        f = (np.asarray(uv, np.float64) * self.scale * 2.0) % 1.0                 # edges sit at the multiples of 1 / 2 of the scaled coordinate
        return (np.minimum(f, 1.0 - f).min(1)) / (2.0 * self.scale)

    def xml(self, name):
        rgb = lambda n, v: f'<rgb name="{n}" value="{float(v[0])!r}, {float(v[1])!r}, {float(v[2])!r}"/>'
        if self.color1 is None:
            return rgb(name, self.color0)
        return (f'<texture name="{name}" type="checkerboard">{rgb("color0", self.color0)}{rgb("color1", self.color1)}'
                f'<transform name="to_uv"><scale value="{self.scale!r}"/></transform></texture>')


def _zeros(n, T):
    return {"wo": np.zeros((n, 3), T), "pdf": np.zeros(n, T), "eta": np.zeros(n, T), "type": np.zeros(n, np.int32), "weight": np.zeros((n, 3), T),
            "lobe_margin": np.full(n, INF), "tex_margin": np.full(n, INF)}


def _mask(out, active):
    """dr::zeros<BSDFSample3f> and a zero weight where the lane is not active"""
    for k in ("wo", "pdf", "eta", "type", "weight"):
        a = active if out[k].ndim == 1 else active[:, None]
        out[k] = np.where(a, out[k], 0).astype(out[k].dtype)
    return out


def reflect(wi):
    return wi * np.asarray([-1, -1, 1], wi.dtype)


def square_to_cosine_hemisphere(s2, T):
    """warp.h:54-92, :412-420"""
    s2 = _f(T, s2)
    x = T(2) * s2[:, 0] - T(1); y = T(2) * s2[:, 1] - T(1)
    q13 = np.abs(x) < np.abs(y)
    r = np.where(q13, y, x); rp = np.where(q13, x, y)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = T(0.25 * np.pi) * rp / r
    phi = np.where(q13, T(0.5 * np.pi) - phi, phi)
    phi = np.where((x == 0) & (y == 0), T(0), phi).astype(T)
    px = r * np.cos(phi); py = r * np.sin(phi)
    z = np.sqrt(np.maximum(T(1) - (px * px + py * py), T(0)))
    return np.stack([px, py, z], 1).astype(T)


# --------------------------------------------------------------------------------------------------------------- the plugins
class Diffuse:
    """src/bsdfs/diffuse.cpp (a twosided's child here; the device's own diffuse is held elsewhere)"""
    flags = F_SMOOTH

    def __init__(self, reflectance=0.5):
        self.reflectance = reflectance if isinstance(reflectance, Tex) else Tex(reflectance)

    def xml(self):
        return f'<bsdf type="diffuse">{self.reflectance.xml("reflectance")}</bsdf>'

    def sample(self, wi, s1, s2, uv, T=np.float64, **kw):
        wi = _f(T, wi); n = len(wi); out = _zeros(n, T)
        out["wo"] = square_to_cosine_hemisphere(s2, T)
        out["pdf"] = (T(1 / np.pi) * out["wo"][:, 2]).astype(T); out["eta"][:] = 1; out["type"][:] = F_SMOOTH
        out["weight"] = self.reflectance.eval(uv, T)
        out["tex_margin"] = self.reflectance.margin(uv)
        return _mask(out, (wi[:, 2] > 0) & (out["pdf"] > 0))

    def eval_pdf(self, wi, wo, uv, T=np.float64, **kw):
        wi = _f(T, wi); wo = _f(T, wo)
        active = (wi[:, 2] > 0) & (wo[:, 2] > 0)
        p = T(1 / np.pi) * wo[:, 2]
        ev = self.reflectance.eval(uv, T) * T(1 / np.pi) * wo[:, 2:3]
        return np.where(active[:, None], ev, 0).astype(T), np.where(active, p, 0).astype(T), np.minimum(np.minimum(np.abs(wi[:, 2]), np.abs(wo[:, 2])), self.reflectance.margin(uv))

    def albedo(self, wi, uv, T=np.float64):
        return self.reflectance.eval(uv, T)


class Conductor:
    """conductor.cpp:226-330; the defaults (eta 0, k 1: material = none) are a perfect mirror"""
    flags = F_DELTA

    def __init__(self, eta=0.0, k=1.0, specular_reflectance=1.0):
        c = lambda v: np.broadcast_to(np.asarray(v, np.float32), (3,)).astype(np.float32)
        self.eta = c(eta); self.k = c(k)
        self.spec = specular_reflectance if isinstance(specular_reflectance, Tex) else Tex(specular_reflectance)

    def xml(self):
        rgb = lambda n, v: f'<rgb name="{n}" value="{float(v[0])!r}, {float(v[1])!r}, {float(v[2])!r}"/>'
        return f'<bsdf type="conductor">{rgb("eta", self.eta)}{rgb("k", self.k)}{self.spec.xml("specular_reflectance")}</bsdf>'

    def sample(self, wi, s1, s2, uv, T=np.float64, swap=False, **kw):
        wi = _f(T, wi); n = len(wi); out = _zeros(n, T)
        c = wi[:, 2]
        out["wo"] = reflect(wi); out["pdf"][:] = 1; out["eta"][:] = 1; out["type"][:] = F_DELTA
        er, ei = (self.k, self.eta) if swap else (self.eta, self.k)                  # swap: a seeded mistake (test_smooth.py)
        with np.errstate(invalid="ignore", divide="ignore"):
            F = np.stack([fresnel_conductor(c, er[j], ei[j], T) for j in range(3)], 1)
        out["weight"] = (self.spec.eval(uv, T) * F).astype(T)
        out["tex_margin"] = self.spec.margin(uv)
        return _mask(out, c > 0)

    def eval_pdf(self, wi, wo, uv, T=np.float64, **kw):
        n = len(wi)
        return np.zeros((n, 3), T), np.zeros(n, T), np.full(n, INF)

    def albedo(self, wi, uv, T=np.float64):
        return np.zeros((len(wi), 3), T)                                            # bsdf.cpp:38-43: eval(wo = +z) * pi


class Plastic:
    """plastic.cpp:160-365"""
    flags = F_DELTA | F_SMOOTH

    def __init__(self, int_ior="polypropylene", ext_ior="air", diffuse_reflectance=0.5, specular_reflectance=None, nonlinear=False):
        self.int_ior, self.ext_ior = int_ior, ext_ior
        self.diff = diffuse_reflectance if isinstance(diffuse_reflectance, Tex) else Tex(diffuse_reflectance)
        self.spec = specular_reflectance if (specular_reflectance is None or isinstance(specular_reflectance, Tex)) else Tex(specular_reflectance)
        self.nonlinear = bool(nonlinear)
        ior = lambda v: np.float32(IOR[v] if isinstance(v, str) else v)
        self.eta32 = np.float32(ior(int_ior) / ior(ext_ior))                          # plastic.cpp:168 in float32, as the loader forms it

    def xml(self):
        ior = lambda n, v: f'<string name="{n}" value="{v}"/>' if isinstance(v, str) else f'<float name="{n}" value="{float(v)!r}"/>'
        return (f'<bsdf type="plastic">{ior("int_ior", self.int_ior)}{ior("ext_ior", self.ext_ior)}{self.diff.xml("diffuse_reflectance")}'
                f'{self.spec.xml("specular_reflectance") if self.spec else ""}<boolean name="nonlinear" value="{"true" if self.nonlinear else "false"}"/></bsdf>')

    def constants(self, T=np.float64):
        """plastic.cpp:192-207 from the float32 eta: eta, inv_eta_2, fdr_int, fdr_ext, specular_sampling_weight"""
        eta = T(self.eta32)
        d_mean = self.diff.mean(T); s_mean = self.spec.mean(T) if self.spec else T(1)
        return {"eta": eta, "inv_eta_2": T(1) / (eta * eta), "fdr_int": fresnel_diffuse_reflectance(T(1) / eta, T), "fdr_ext": fresnel_diffuse_reflectance(eta, T),
                "specular_sampling_weight": T(s_mean / (d_mean + s_mean))}

    def _base(self, uv, k, T, skip_inv_eta_2=False):
        """:264-266 / :290-294 without the Fresnel factors: diff / (1 - (nonlinear ? diff fdr_int : fdr_int))"""
        d = self.diff.eval(uv, T)
        return (d / (T(1) - (d * k["fdr_int"] if self.nonlinear else k["fdr_int"]))).astype(T)

    def sample(self, wi, s1, s2, uv, T=np.float64, f_o_at_wi=False, no_inv_eta_2=False, **kw):
        wi = _f(T, wi); s1 = _f(T, s1); n = len(wi); out = _zeros(n, T); k = self.constants(T)
        c = wi[:, 2]
        f_i = fresnel(c, k["eta"], T)
        w = k["specular_sampling_weight"]
        ps = f_i * w; pd = (T(1) - f_i) * (T(1) - w)
        with np.errstate(invalid="ignore", divide="ignore"):
            ps = ps / (ps + pd)
        pd = T(1) - ps
        spec = s1 < ps
        wo_d = square_to_cosine_hemisphere(s2, T)
        out["wo"] = np.where(spec[:, None], reflect(wi), wo_d).astype(T)
        out["pdf"] = np.where(spec, ps, pd * (T(1 / np.pi) * wo_d[:, 2])).astype(T)
        out["eta"][:] = 1; out["type"] = np.where(spec, F_DELTA, F_SMOOTH).astype(np.int32)
        with np.errstate(invalid="ignore", divide="ignore"):
            v_s = (f_i / ps)[:, None] * (self.spec.eval(uv, T) if self.spec else np.ones((n, 3), T))
            f_o = fresnel(c if f_o_at_wi else wo_d[:, 2], k["eta"], T)                        # f_o_at_wi, no_inv_eta_2: seeded mistakes (test_smooth.py)
            v_d = self._base(uv, k, T) * ((T(1) if no_inv_eta_2 else k["inv_eta_2"]) * (T(1) - f_i) * (T(1) - f_o) / pd)[:, None]
        out["weight"] = np.where(spec[:, None], v_s, v_d).astype(T)
        out["lobe_margin"] = np.abs(s1.astype(np.float64) - ps.astype(np.float64)); out["ps"] = ps
        out["tex_margin"] = np.where(spec, self.spec.margin(uv) if self.spec else INF, self.diff.margin(uv))
        return _mask(out, c > 0)

    def eval_pdf(self, wi, wo, uv, T=np.float64, no_inv_eta_2=False, **kw):
        wi = _f(T, wi); wo = _f(T, wo); k = self.constants(T)
        ci, co = wi[:, 2], wo[:, 2]
        active = (ci > 0) & (co > 0)
        f_i = fresnel(ci, k["eta"], T); f_o = fresnel(co, k["eta"], T)
        hemi = T(1 / np.pi) * co
        with np.errstate(invalid="ignore", divide="ignore"):
            ev = self._base(uv, k, T) * (hemi * (T(1) if no_inv_eta_2 else k["inv_eta_2"]) * (T(1) - f_i) * (T(1) - f_o))[:, None]
            w = k["specular_sampling_weight"]
            ps = f_i * w; pd = (T(1) - f_i) * (T(1) - w); pd = pd / (ps + pd)
            p = hemi * pd
        return (np.where(active[:, None], ev, 0).astype(T), np.where(active, p, 0).astype(T),
                np.minimum(np.minimum(np.abs(ci), np.abs(co)).astype(np.float64), self.diff.margin(uv)))

    def albedo(self, wi, uv, T=np.float64):
        return self.diff.eval(uv, T)                                                # plastic.cpp:362-365


class TwoSided:
    """twosided.cpp:74-307.  back = None: one child (the same-child branch, abs and mulsign); else the front_side / back_side masks"""

    def __init__(self, front, back=None):
        self.front, self.back = front, back
        self.flags = front.flags | (back.flags if back is not None else 0)

    def xml(self):
        return f'<bsdf type="twosided">{self.front.xml()}{self.back.xml() if self.back is not None else ""}</bsdf>'

    def _sides(self, wi):
        """per lane: which child (0 / 1 / -1 none), the child's wi, and the sign wo.z is multiplied with"""
        z = wi[:, 2]
        neg = np.signbit(z)
        wi_c = wi.copy(); wi_c[:, 2] = np.abs(z)
        sign = np.where(neg, -1, 1).astype(wi.dtype)
        if self.back is None:
            return np.zeros(len(wi), np.int32), wi_c, sign
        return np.where(z > 0, 0, np.where(z < 0, 1, -1)).astype(np.int32), wi_c, sign

    def sample(self, wi, s1, s2, uv, T=np.float64, no_mulsign=False, wrong_child=False, **kw):
        wi = _f(T, wi); which, wi_c, sign = self._sides(wi)
        if no_mulsign:
            sign = np.ones_like(sign)                                                # seeded mistakes (test_smooth.py)
        if wrong_child and self.back is not None:
            which = np.where(which >= 0, 0, which)
        outs = [self.front.sample(wi_c, s1, s2, uv, T, **kw)] + ([self.back.sample(wi_c, s1, s2, uv, T, **kw)] if self.back is not None else [])
        out = {}
        for k in outs[0]:
            if k == "ps":
                continue
            v = outs[0][k]
            for j in range(1, len(outs)):
                m = which == j
                v = np.where(m if v.ndim == 1 else m[:, None], outs[j][k], v)
            out[k] = v
        out = _mask(out, which >= 0)
        out["wo"] = out["wo"].copy(); out["wo"][:, 2] = out["wo"][:, 2] * sign
        return out

    def eval_pdf(self, wi, wo, uv, T=np.float64, no_mulsign=False, wrong_child=False, **kw):
        wi = _f(T, wi); wo = _f(T, wo); which, wi_c, sign = self._sides(wi)
        if no_mulsign:
            sign = np.ones_like(sign)
        if wrong_child and self.back is not None:
            which = np.where(which >= 0, 0, which)
        wo_c = wo.copy(); wo_c[:, 2] = wo[:, 2] * sign
        rs = [self.front.eval_pdf(wi_c, wo_c, uv, T, **kw)] + ([self.back.eval_pdf(wi_c, wo_c, uv, T, **kw)] if self.back is not None else [])
        ev, p, mg = rs[0]
        for j in range(1, len(rs)):
            m = which == j
            ev = np.where(m[:, None], rs[j][0], ev); p = np.where(m, rs[j][1], p); mg = np.where(m, rs[j][2], mg)
        none = which < 0
        return np.where(none[:, None], 0, ev).astype(T), np.where(none, 0, p).astype(T), mg

    def albedo(self, wi, uv, T=np.float64):
        wi = _f(T, wi); which, _, _ = self._sides(wi)
        a = self.front.albedo(wi, uv, T)
        if self.back is not None:
            a = np.where((which == 1)[:, None], self.back.albedo(wi, uv, T), a)
        return np.where((which < 0)[:, None], 0, a).astype(T)
