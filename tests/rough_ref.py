"""The rough dielectric BSDF in numpy, with the working precision as a parameter: Walter, Marschner, Li and Torrance, "Microfacet
models for refraction through rough surfaces" (EGSR 2007) with the Beckmann and GGX distributions, Smith's separable shadowing
(Beckmann through the rational fit of that paper), Heitz and d'Eon's sampling of the visible normals (EGSR 2014) with the Newton
inversion for Beckmann, and the conventions of the renderer this project follows: both lobes always enabled, radiance transport
(a transmitted value carries 1 / eta^2), the roughness scaled by 1.2 - 0.2 sqrt|cos theta_i| when all normals are sampled, D cut
to zero where D cos theta_m <= 1e-20, perfectly grazing wi inactive.

Everything is in the local frame of the surface (z = normal).  `dtype` is np.float64 (the reference the device is held to) or
np.float32 (the same formulas rounded as a float32 program rounds them: its distance from the float64 run is what float32 costs,
and sets the K of every tolerance).  erf and erfinv are math.erf and torch.special.erfinv in float64 in both runs, rounded to the
working precision."""
import math

import numpy as np

EPS = 2.0 ** -23
F_SMOOTH = 2
CUT = 1e-20


class Config:
    def __init__(self, alpha_u, alpha_v=None, ggx=False, visible=True, int_ior=1.5046, ext_ior=1.000277):
        self.alpha_u = float(alpha_u); self.alpha_v = float(alpha_u if alpha_v is None else alpha_v)
        self.ggx = bool(ggx); self.visible = bool(visible); self.int_ior = float(int_ior); self.ext_ior = float(ext_ior)

    def eta(self, T):
        """int_ior / ext_ior as the loader forms it: a float32 quotient of float32 values, whatever the working precision"""
        return T(np.float32(self.int_ior) / np.float32(self.ext_ior))

    def alphas(self, T):
        return T(max(np.float32(self.alpha_u), np.float32(1e-4))), T(max(np.float32(self.alpha_v), np.float32(1e-4)))

    def label(self):
        a = f"{self.alpha_u:g}" if self.alpha_u == self.alpha_v else f"({self.alpha_u:g},{self.alpha_v:g})"
        return f"{'ggx' if self.ggx else 'beckmann'}-{'vis' if self.visible else 'all'}-a{a}-{self.int_ior:g}/{self.ext_ior:g}"


def erf(x, T):
    x64 = np.asarray(x, np.float64)
    return np.vectorize(math.erf, otypes=[np.float64])(x64).astype(T)


def erfinv(x, T):
    import torch
    x64 = np.ascontiguousarray(np.asarray(x, np.float64))
    return torch.special.erfinv(torch.from_numpy(x64)).numpy().astype(T)


def _mulsign(a, s):
    return np.where(np.signbit(s), -a, a)


def fresnel(cos_i, eta, T):
    """unpolarized Fresnel reflectance at cos_i (its sign tells the side), relative index eta = interior / exterior.
    Returns (F, cos_t with the sign opposite to cos_i, eta_it, eta_ti)."""
    cos_i = np.asarray(cos_i, T)
    outside = cos_i >= 0
    rcp_eta = T(1) / eta
    eta_it = np.where(outside, eta, rcp_eta).astype(T); eta_ti = np.where(outside, rcp_eta, eta).astype(T)
    ctt2 = T(1) - (T(1) - cos_i * cos_i) * (eta_ti * eta_ti)
    cti = np.abs(cos_i); ctt = np.sqrt(np.maximum(ctt2, T(0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        a_s = (cti - eta_it * ctt) / (cti + eta_it * ctt)
        a_p = (ctt - eta_it * cti) / (ctt + eta_it * cti)
    F = T(0.5) * (a_s * a_s + a_p * a_p)
    F = np.where(cti == 0, T(1), F)
    if eta == 1:
        F = np.zeros_like(F)
    return F.astype(T), _mulsign(ctt, -cos_i).astype(T), eta_it, eta_ti


class Distribution:
    """normal distribution D, Smith G1, and the two ways to draw a normal"""

    def __init__(self, au, av, ggx, visible, T, iso=None):
        self.au, self.av, self.ggx, self.visible, self.T = au, av, ggx, visible, T
        self.iso = bool(au == av) if iso is None else iso

    def scaled(self, f):
        return Distribution(self.au * f, self.av * f, self.ggx, self.visible, self.T, self.iso)

    def eval(self, m, with_margin=False):
        T = self.T
        mx, my, mz = m[..., 0], m[..., 1], m[..., 2]
        alpha_uv = self.au * self.av
        c2 = mz * mz
        e = (mx / self.au) ** 2 + (my / self.av) ** 2
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            if not self.ggx:
                r = np.exp(-e / c2) / (T(np.pi) * alpha_uv * c2 * c2)
            else:
                r = T(1) / (T(np.pi) * alpha_uv * (e + c2) ** 2)
            keep = r * mz > T(CUT)
            out = np.where(keep, r, T(0)).astype(T)
            if with_margin:
                return out, np.abs(np.asarray(r * mz, np.float64) / CUT - 1)
        return out

    def smith_g1(self, v, m):
        T = self.T
        xy = (self.au * v[..., 0]) ** 2 + (self.av * v[..., 1]) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            t2 = xy / (v[..., 2] * v[..., 2])
            if not self.ggx:
                a = T(1) / np.sqrt(t2); a2 = a * a
                r = np.where(a >= T(1.6), T(1), (T(3.535) * a + T(2.181) * a2) / (T(1) + T(2.276) * a + T(2.577) * a2))
            else:
                r = T(2) / (T(1) + np.sqrt(T(1) + t2))
        r = np.where(xy == 0, T(1), r)
        r = np.where(np.sum(v * m, -1) * v[..., 2] <= 0, T(0), r)
        return r.astype(T)

    def G(self, wi, wo, m):
        return self.smith_g1(wi, m) * self.smith_g1(wo, m)

    def pdf(self, wi, m):
        r = self.eval(m)
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.visible:
                return (r * self.smith_g1(wi, m) * np.abs(np.sum(wi * m, -1)) / wi[..., 2]).astype(self.T)
        return (r * m[..., 2]).astype(self.T)

    def sample_visible_11(self, cos_i, sin_i, sx, sy, dx=0.0):
        T = self.T
        if not self.ggx:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
                tan_i = sin_i / cos_i
                cot_i = T(1) / tan_i
                maxval = erf(cot_i, T)
                sx = np.maximum(np.minimum(sx, T(1) - T(1e-6)), T(1e-6)); sy = np.maximum(np.minimum(sy, T(1) - T(1e-6)), T(1e-6))
                x = maxval - (maxval + T(1)) * erf(np.sqrt(-np.log(sx)), T)
                isp = T(1 / math.sqrt(math.pi))
                sx = sx * (T(1) + maxval + isp * tan_i * np.exp(-(cot_i * cot_i)))
                for _ in range(3):
                    slope = erfinv(x, T)
                    value = T(1) + x + isp * tan_i * np.exp(-(slope * slope)) - sx
                    deriv = T(1) - slope * tan_i
                    x = (x - value / deriv).astype(T)
                if np.ndim(dx) or dx:            # (the tests' condition number: a perturbation of the residual of the last step, in the erf domain)
                    x = (x + T(dx) * (T(1) + T(1) / np.abs(deriv))).astype(T)
                return erfinv(x, T), erfinv(T(2) * sy - T(1), T)
        # GGX: a point of the disk, its ordinate squeezed towards the half disk the direction sees
        x = T(2) * sx - T(1); y = T(2) * sy - T(1)
        first = ~(np.abs(x) < np.abs(y))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(first, x, y); rp = np.where(first, y, x)
            phi = T(np.pi / 4) * rp / r
            phi = np.where(first, phi, T(np.pi / 2) - phi)
        phi = np.where((x == 0) & (y == 0), T(0), phi).astype(T)
        px = (r * np.cos(phi)).astype(T); py = (r * np.sin(phi)).astype(T)
        s = T(0.5) * (T(1) + cos_i)
        a = np.sqrt(np.maximum(T(1) - px * px, T(0)))
        py = (T(1) - s) * a + s * py
        pz = np.sqrt(np.maximum(T(1) - (px * px + py * py), T(0)))
        with np.errstate(divide="ignore", invalid="ignore"):
            nrm = T(1) / (sin_i * py + cos_i * pz)
            return ((cos_i * py - sin_i * pz) * nrm).astype(T), (px * nrm).astype(T)

    def sample(self, wi, sx, sy, dx=0.0):
        """(m, pdf, margin) for a viewer direction wi with wi.z > 0.  dx: a perturbation of the Newton residual of Beckmann's visible
        normals, for the tests' condition numbers.  Two sines are formed without cancellation, in either precision: sin theta_m =
        tan theta_m cos theta_m (not sqrt(1 - cos^2 theta_m), which loses a small alpha), and the sine of the stretched wi = sqrt(x^2 +
        y^2) (not sqrt(1 - z^2), which loses normal incidence)."""
        T = self.T
        if not self.visible:
            with np.errstate(divide="ignore", invalid="ignore"):
                if self.iso:
                    ang = T(2 * np.pi) * sy
                    sin_phi, cos_phi = np.sin(ang).astype(T), np.cos(ang).astype(T)
                    alpha_2 = self.au * self.au + 0 * sx
                else:
                    tmp = (self.av / self.au) * np.tan(T(2 * np.pi) * sy).astype(T)
                    cos_phi = T(1) / np.sqrt(tmp * tmp + T(1))
                    cos_phi = _mulsign(cos_phi, np.abs(sy - T(0.5)) - T(0.25))
                    sin_phi = cos_phi * tmp
                    alpha_2 = T(1) / ((cos_phi / self.au) ** 2 + (sin_phi / self.av) ** 2)
                if not self.ggx:
                    t2 = -alpha_2 * np.log(T(1) - sx)
                    cos_t = T(1) / np.sqrt(T(1) + t2)
                    c2 = cos_t * cos_t
                    c3 = np.maximum(c2 * cos_t, T(CUT))
                    pdf = (T(1) - sx) / (T(np.pi) * self.au * self.av * c3)
                else:
                    t2 = alpha_2 * sx / (T(1) - sx)
                    cos_t = T(1) / np.sqrt(T(1) + t2)
                    c2 = cos_t * cos_t
                    temp = T(1) + t2 / alpha_2
                    c3 = np.maximum(c2 * cos_t, T(CUT))
                    pdf = T(1) / (T(np.pi) * self.au * self.av * c3 * temp * temp)
                sin_t = np.sqrt(t2) * cos_t
            return np.stack([cos_phi * sin_t, sin_phi * sin_t, cos_t], -1).astype(T), pdf.astype(T), np.full(np.shape(sx), np.inf)
        wp = np.stack([self.au * wi[..., 0], self.av * wi[..., 1], wi[..., 2]], -1)
        wp = (wp / np.sqrt(np.sum(wp * wp, -1))[..., None]).astype(T)
        st2 = (wp[..., 0] * wp[..., 0] + wp[..., 1] * wp[..., 1]).astype(T)       # sin^2 of the stretched wi: serves the azimuth and sample_visible_11
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = T(1) / np.sqrt(st2)
            cos_phi = np.clip(wp[..., 0] * inv, T(-1), T(1)); sin_phi = np.clip(wp[..., 1] * inv, T(-1), T(1))
        flat = np.abs(st2) <= T(4 * 2.0 ** -24)              # (the float32 renderer's Epsilon in either precision: the branch is part of what is computed)
        fm = np.abs(np.asarray(st2, np.float64) / (4 * 2.0 ** -24) - 1)
        cos_phi = np.where(flat, T(1), cos_phi).astype(T); sin_phi = np.where(flat, T(0), sin_phi).astype(T)
        s1, s2 = self.sample_visible_11(wp[..., 2], np.sqrt(np.maximum(st2, T(0))), sx, sy, dx)
        slx = (cos_phi * s1 - sin_phi * s2) * self.au; sly = (sin_phi * s1 + cos_phi * s2) * self.av
        m = np.stack([-slx, -sly, np.ones_like(slx)], -1)
        m = (m / np.sqrt(np.sum(m * m, -1))[..., None]).astype(T)
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf = self.eval(m) * self.smith_g1(wi, m) * np.abs(np.sum(wi * m, -1)) / wi[..., 2]
        return m, pdf.astype(T), fm


def _setup(cfg, T):
    au, av = cfg.alphas(T)
    return Distribution(au, av, cfg.ggx, cfg.visible, T), cfg.eta(T)


def sample(cfg, wi, s1, s2, dtype=np.float64, dx=0.0):
    """BSDF sample: dict of wo (n, 3), pdf, eta, type, weight (scalar per lane: no reflectance textures), plus what the tests need of
    the inside: F, m, active, `lobe_margin` = |s1 - F|, and `margin`: the distance of the lane from the other discontinuities of the
    sample (cos theta_i against 0, D cos theta_m against the cut and the azimuth branch of the stretched wi in relative terms)."""
    T = dtype
    wi = np.asarray(wi, T); s1 = np.asarray(s1, T); s2 = np.asarray(s2, T)
    distr, m_eta = _setup(cfg, T)
    ci = wi[..., 2]
    active = ci != 0
    sd = distr if cfg.visible else distr.scaled((T(1.2) - T(0.2) * np.sqrt(np.abs(ci))).astype(T))
    wif = _mulsign(wi, ci[..., None]).astype(T)
    m, pdf, fm = sd.sample(wif, s2[..., 0], s2[..., 1], dx)
    active = active & (pdf != 0)
    wi_m = np.sum(wi * m, -1).astype(T)
    F, ctt, eta_it, eta_ti = fresnel(wi_m, m_eta, T)
    sel_r = (s1 <= F) & active
    pdf = pdf * np.where(sel_r, F, T(1) - F)
    eta = np.where(sel_r, T(1), eta_it).astype(T)
    wo_r = m * (T(2) * wi_m)[..., None] - wi
    wo_t = m * (wi_m * eta_ti + ctt)[..., None] - wi * eta_ti[..., None]
    wo = np.where(sel_r[..., None], wo_r, wo_t).astype(T)
    wo_m = np.sum(wo * m, -1).astype(T)
    with np.errstate(divide="ignore", invalid="ignore"):
        jac = np.where(sel_r, T(1) / (T(4) * wo_m), (eta * eta * wo_m) / (wi_m + eta * wo_m) ** 2)
        weight = np.where(sel_r, T(1), eta_ti * eta_ti)
        if cfg.visible:
            weight = weight * distr.smith_g1(wo, m)
        else:
            weight = weight * (distr.G(wi, wo, m) * wi_m / (ci * m[..., 2]))
        pdf = np.where(active, pdf * np.abs(jac), T(0)).astype(T)
    wo = np.where(active[..., None], wo, T(0)).astype(T)                  # (neither lobe selected: wo and the Jacobian stay 0)
    weight = np.where(active, weight, T(0)).astype(T)
    if cfg.visible:
        _, dm = distr.eval(m, with_margin=True)
    else:
        dm = np.full(ci.shape, np.inf)
    margin = np.minimum(np.minimum(np.abs(np.asarray(ci, np.float64)), dm), fm)
    return {"wo": wo, "pdf": pdf, "eta": eta, "type": np.full(ci.shape, F_SMOOTH), "weight": weight, "F": F, "m": m, "active": active,
            "reflected": sel_r, "margin": margin,
            "lobe_margin": np.abs(np.asarray(s1, np.float64) - np.asarray(F, np.float64))}


def eval_pdf(cfg, wi, wo, dtype=np.float64, need_pdf=True):
    """(value with the cosine, pdf, margin): margin is the distance from the nearest discontinuity of either (cos theta_i and cos
    theta_o against 0, the D cut in relative terms, and the side tests of wi and wo against the half vector)."""
    T = dtype
    wi = np.asarray(wi, T); wo = np.asarray(wo, T)
    distr, m_eta = _setup(cfg, T)
    ci, co = wi[..., 2], wo[..., 2]
    active = ci != 0
    refl = ci * co > 0
    inv_m_eta = T(1) / m_eta
    eta = np.where(ci > 0, m_eta, inv_m_eta).astype(T); inv_eta = np.where(ci > 0, inv_m_eta, m_eta).astype(T)
    h = wi + wo * np.where(refl, T(1), eta)[..., None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        m = (h / np.sqrt(np.sum(h * h, -1))[..., None]).astype(T)
        m = _mulsign(m, m[..., 2][..., None]).astype(T)
        wi_m = np.sum(wi * m, -1).astype(T); wo_m = np.sum(wo * m, -1).astype(T)
        D, dm = distr.eval(m, with_margin=True)
        F = fresnel(wi_m, m_eta, T)[0]
        G = distr.G(wi, wo, m)
        v_r = F * D * G / (T(4) * np.abs(ci))
        v_t = np.abs((inv_eta * inv_eta * (T(1) - F) * D * G * eta * eta * wi_m * wo_m) / (ci * (wi_m + eta * wo_m) ** 2))
        value = np.where(active, np.where(refl, v_r, v_t), T(0)).astype(T)
        if not need_pdf:
            return value, None, None
        ok = active & (wi_m * ci > 0) & (wo_m * co > 0)
        sd = distr if cfg.visible else distr.scaled((T(1.2) - T(0.2) * np.sqrt(np.abs(ci))).astype(T))
        p = sd.pdf(_mulsign(wi, ci[..., None]).astype(T), m) * np.where(refl, F, T(1) - F)
        jac = np.where(refl, T(1) / (T(4) * wo_m), (eta * eta * wo_m) / (wi_m + eta * wo_m) ** 2)
        pdf = np.where(ok, p * np.abs(jac), T(0)).astype(T)
    f64 = lambda a: np.abs(np.asarray(a, np.float64))
    margin = np.minimum.reduce([f64(ci), f64(co), dm, f64(wi_m), f64(wo_m)])
    return value, pdf, margin


# ---------------------------------------------------------------------------------------------------------------- quadrature
def sphere_grid(n_theta=2048, n_phi=512, half=False):
    """midpoint nodes in (cos theta, phi) over the whole sphere (half: phi in (0, pi) only, for integrands that are even in phi):
    directions (n, 3) and the solid angle of a cell"""
    ct = -1 + (np.arange(n_theta) + 0.5) * (2 / n_theta)
    span = np.pi if half else 2 * np.pi
    ph = (np.arange(n_phi) + 0.5) * (span / n_phi)
    C, P = np.meshgrid(ct, ph, indexing="ij")
    st = np.sqrt(1 - C * C)
    return np.stack([st * np.cos(P), st * np.sin(P), C], -1).reshape(-1, 3), (2 / n_theta) * (span / n_phi)


def lobe_integrals(cfg, wi, weight_t=None, n_theta=2048, n_phi=512, what="eval"):
    """(reflected, transmitted) integrals over the sphere of eval (or pdf) for one wi; weight_t(wo) multiplies the transmitted part.
    Midpoint rule in (cos theta, phi); for alpha >= 0.1 the default grid is within 2e-5 relative of grids four times as fine
    (test_rough.py holds two resolutions against each other).  An isotropic roughness seen from the xz plane is even in phi: half the
    nodes do."""
    wi = np.asarray(wi, np.float64)
    half = cfg.alpha_u == cfg.alpha_v and wi[1] == 0
    d, w = sphere_grid(n_theta, n_phi // 2 if half else n_phi, half)
    W = np.broadcast_to(wi, d.shape)
    v, p, _ = eval_pdf(cfg, W, d, need_pdf=what != "eval")
    f = v if what == "eval" else p
    same = d[:, 2] * wi[2] > 0
    wt = np.ones(len(d)) if weight_t is None else weight_t(d)
    k = 2.0 if half else 1.0
    return float(np.sum(f[same]) * w * k), float(np.sum((f * wt)[~same]) * w * k)


# --------------------------------------------------------------------------------------------------------------- chi-square
def chi2_test(wo, pdf_of, n_samples, res=(64, 128), sub=4, p_zero=None, mass_slack=0.0):
    """Pearson's test of directions wo (n, 3) against the density pdf_of(directions) over cells of (cos theta, phi).  p_zero marks the
    samples of zero density (pdf 0, or weight 0: a reflection that ends below the surface keeps the pdf of its normal and has no
    density as a direction).  Expected counts: composite Simpson of the density over each cell, 2 sub + 1 nodes a side.  Cells expecting
    fewer than 5 are pooled.  The samples without density make one more cell, expected n (1 - total mass).  That expectation is a small
    difference of large numbers, so what is known of the error of the total mass is taken off its deviation first: the quadrature's
    own error (the same nodes at half the density, Richardson) and mass_slack, the caller's bound on how far the density is from
    integrating to what the sampler does (Beckmann's visible normals: the rational fit of G1, below 0.35 % by its authors' statement).
    Returns (p value, statistic, degrees of freedom, total mass)."""
    import torch
    nt, nphi = res
    wo = np.asarray(wo, np.float64)
    zero = (np.abs(wo).sum(1) == 0) if p_zero is None else np.asarray(p_zero, bool)
    live = wo[~zero]
    live = live / np.linalg.norm(live, axis=1, keepdims=True)
    ict = np.clip(((live[:, 2] + 1) * 0.5 * nt).astype(np.int64), 0, nt - 1)
    phi = np.arctan2(live[:, 1], live[:, 0]); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    iph = np.clip((phi / (2 * np.pi) * nphi).astype(np.int64), 0, nphi - 1)
    obs = np.bincount(ict * nphi + iph, minlength=nt * nphi).astype(np.float64)
    # Simpson nodes shared between neighbouring cells
    kt, kp = 2 * sub * nt + 1, 2 * sub * nphi + 1
    ct = np.linspace(-1, 1, kt); ph = np.linspace(0, 2 * np.pi, kp)
    C, P = np.meshgrid(ct, ph, indexing="ij"); S = np.sqrt(np.maximum(1 - C * C, 0))
    f = pdf_of(np.stack([S * np.cos(P), S * np.sin(P), C], -1).reshape(-1, 3)).reshape(kt, kp)
    f = np.nan_to_num(np.asarray(f, np.float64), nan=0.0, posinf=0.0)

    def simpson(f, sub):
        w1 = np.ones(2 * sub + 1); w1[1:-1:2] = 4; w1[2:-1:2] = 2
        hct, hph = (2 / nt) / (2 * sub), (2 * np.pi / nphi) / (2 * sub)
        out = np.zeros((nt, nphi))
        for a in range(2 * sub + 1):
            for b in range(2 * sub + 1):
                out += w1[a] * w1[b] * f[a:a + 2 * sub * nt:2 * sub, b:b + 2 * sub * nphi:2 * sub][:nt, :nphi]
        return out.reshape(-1) * (hct / 3) * (hph / 3)
    exp = simpson(f, sub)
    mass = float(exp.sum())
    q_err = abs(mass - float(simpson(f[::2, ::2], sub // 2).sum())) if sub % 2 == 0 else 0.0
    exp = exp * n_samples
    order = np.argsort(exp)
    e, o = exp[order], obs[order]
    small = np.cumsum(e) < 5
    k = int(small.sum())
    if k and k < len(e):
        k += 1                                               # the pool reaches 5 with the next cell
    pe, po = (e[:k].sum(), o[:k].sum()) if k else (0.0, 0.0)
    e2, o2 = e[k:], o[k:]
    stat = float(np.sum((o2 - e2) ** 2 / e2)); cells = len(e2)
    if pe > 0:
        stat += (po - pe) ** 2 / pe; cells += 1
    elif po > 0:
        stat = np.inf
    ez = max(n_samples * (1 - mass), 0.0); oz = float(zero.sum())
    dev = max(abs(oz - ez) - n_samples * (q_err + mass_slack), 0.0)
    stat += dev * dev / max(ez, 5.0); cells += 1
    dof = cells - 1
    p = float(torch.special.gammaincc(torch.tensor(dof / 2.0, dtype=torch.float64), torch.tensor(stat / 2.0, dtype=torch.float64)))
    return p, stat, dof, mass
