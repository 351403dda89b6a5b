"""A numpy restatement of the tabulated, Rayleigh and blended phase functions and of the ContinuousDistribution behind the first
(the renderer this project follows: src/phase/tabphase.cpp, rayleigh.cpp, blendphase.cpp, include/mitsuba/core/distr_1d.h:320-597),
with isotropic and HG as a blend's children (src/phase/isotropic.cpp, hg.cpp).  The precision T is a parameter, in the manner of
rough_ref.py: float64 is the reference the device is held to, float32 the run whose distance from it sets the tolerances
(phase_cases.py).  A table's state (values, cdf, interval size, integral, normalisation) is what the reference's scalar constructor
stores, float32 numbers, and both precisions read the same ones.  cbrt is np.cbrt at either precision (the device's own, m_cbrt, is
held to float64 apart from this).

Conventions: wi points back along the incoming ray (mei.wi); hg / isotropic / rayleigh work with cos = dot(wo, wi), the table is laid
out in physics convention, cos(theta) = -dot(wo, wi) = 1 for forward scattering."""
import numpy as np

EPS = 2.0 ** -23

ISOTROPIC, HG, TABULATED, RAYLEIGH, BLEND = 0, 1, 2, 3, 4


def parse_values(s):
    """tabphase.cpp:45-57: tokens split at blanks and commas, each (float) stod"""
    out = []
    for tok in s.replace(",", " ").split():
        try:
            out.append(np.float32(float(tok)))
        except ValueError:
            raise ValueError(f"Could not parse floating point value '{tok}'")
    return np.array(out, np.float32)


class Table:
    """ContinuousDistribution(range = (-1, 1), values, n) as compute_cdf_scalar builds it (distr_1d.h:548-597)"""

    def __init__(self, values):
        v = parse_values(values) if isinstance(values, str) else np.asarray(values, np.float32)
        n = v.size
        if n < 2:
            raise ValueError("ContinuousDistribution: needs at least two entries!")
        interval = (float(np.float32(1.0)) - float(np.float32(-1.0))) / (n - 1)
        cdf = np.zeros(n - 1, np.float32)
        integral = 0.0
        vx = vy = -1
        for i in range(n - 1):
            y0, y1 = float(v[i]), float(v[i + 1])
            value = 0.5 * interval * (y0 + y1)
            integral += value
            cdf[i] = np.float32(integral)
            if y0 < 0 or y1 < 0:
                raise ValueError("ContinuousDistribution: entries must be non-negative!")
            elif value > 0:
                if vx < 0:
                    vx = i
                vy = i
        if vx < 0 or vy < 0:
            raise ValueError("ContinuousDistribution: no probability mass found!")
        self.values, self.cdf, self.n = v, cdf, n
        self.valid = (vx, vy)
        self.integral = cdf[vy]
        self.normalization = np.float32(1.0) / self.integral
        self.interval_size = np.float32(interval)
        self.inv_interval_size = np.float32(1.0) / self.interval_size

    def eval_pdf_normalized(self, x, T):
        """distr_1d.h:370-392"""
        x = np.asarray(x, T)
        active = (x >= -1) & (x <= 1)
        xs = (x - T(-1)) * T(self.inv_interval_size)
        index = np.clip(np.nan_to_num(xs, nan=0.0).astype(np.int64), 0, self.n - 2)
        y0, y1 = self.values[index].astype(T), self.values[index + 1].astype(T)
        w1 = xs - index.astype(T); w0 = T(1) - w1
        return np.where(active, (w0 * y0 + w1 * y1) * T(self.normalization), T(0))

    def search(self, s, T):
        """Dr.Jit's binary_search over [valid.x, valid.y] with the JIT predicate (distr_1d.h:434-446)"""
        cdf = self.cdf.astype(T); total = T(self.integral)
        start = np.full(s.shape, self.valid[0], np.int64); end = np.full(s.shape, self.valid[1], np.int64)
        d = self.valid[1] - self.valid[0]
        for _ in range(int(d).bit_length()):
            middle = (start + end) >> 1
            c = cdf[middle]
            pred = ((c < s) | (c == 0)) & (c != total)
            start = np.where(pred, np.minimum(middle + 1, end), start)
            end = np.where(pred, end, middle)
        return start

    def sample(self, u, T):
        """distr_1d.h:429-459 -> (position, index, t): t is the position within the chosen interval"""
        s = np.asarray(u, T) * T(self.integral)
        index = self.search(s, T)
        y0, y1 = self.values[index].astype(T), self.values[index + 1].astype(T)
        c0 = np.where(index > 0, self.cdf[np.maximum(index - 1, 0)].astype(T), T(0))
        s = (s - c0) * T(self.inv_interval_size)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_linear = (y0 - np.sqrt(np.maximum(y0 * y0 + T(2) * s * (y1 - y0), T(0)))) * (T(1) / (y0 - y1))
            t_const = s * (T(1) / y0)
        t = np.where(y0 == y1, t_const, t_linear)
        return (index.astype(T) + t) * T(self.interval_size) + T(-1), index, t


class Phase:
    """one phase function: kind, g (hg), table (tabphase), weight and children (blendphase)"""

    def __init__(self, kind, g=0.0, table=None, weight=0.0, children=None, label=None):
        self.kind, self.g, self.table, self.children = kind, np.float32(g), table, children
        self.weight = np.float32(min(max(np.float32(weight), np.float32(0)), np.float32(1)))          # blendphase.cpp:156-159
        self.label = label

    def to_dict(self):
        if self.kind == ISOTROPIC:
            return {"type": "isotropic"}
        if self.kind == HG:
            return {"type": "hg", "g": float(self.g)}
        if self.kind == RAYLEIGH:
            return {"type": "rayleigh"}
        if self.kind == TABULATED:
            return {"type": "tabphase", "values": ", ".join(repr(float(x)) for x in self.table.values)}
        return {"type": "blendphase", "weight": float(self.weight), "phase_0": self.children[0].to_dict(), "phase_1": self.children[1].to_dict()}


def isotropic():
    return Phase(ISOTROPIC, label="isotropic")


def hg(g):
    return Phase(HG, g=g, label=f"hg{g:g}")


def rayleigh():
    return Phase(RAYLEIGH, label="rayleigh")


def tabphase(values, label=None):
    t = Table(values)
    return Phase(TABULATED, table=t, label=label or f"tab{t.n}")


def blend(w, p0, p1):
    if p0.kind == BLEND or p1.kind == BLEND:
        raise ValueError("one blend level")
    return Phase(BLEND, weight=w, children=(p0, p1), label=f"blend{w:g}({p0.label},{p1.label})")


def hg_eval(g, cos_theta, T=np.float64):
    """hg.cpp:64-69"""
    g = T(g); c = np.asarray(cos_theta, T)
    temp = T(1) + g * g + T(2) * g * c
    return T(1 / (4 * np.pi)) * (T(1) - g * g) / (temp * np.sqrt(temp))


def hg_table(g, n):
    """HG tabulated at n nodes over cos(theta), physics convention: node value hg_eval(g, -cos) (float32, as a scene file holds it)"""
    c = np.linspace(-1.0, 1.0, n)
    return hg_eval(g, -c).astype(np.float32)


def _frame(n, T):
    """coordinate_system of include/mitsuba/core/vector.h (Duff et al.): (s, t) for unit n"""
    sign = np.where(np.signbit(n[:, 2]), T(-1), T(1)).astype(T)
    a = -T(1) / (sign + n[:, 2]); b = n[:, 0] * n[:, 1] * a
    s = np.stack([(n[:, 0] * n[:, 0] * a) * sign + T(1), b * sign, -sign * n[:, 0]], 1)
    t = np.stack([b, n[:, 1] * n[:, 1] * a + sign, -n[:, 1]], 1)
    return s, t


def _to_world(wi, v, T):
    s, t = _frame(wi, T)
    return s * v[:, 0:1] + t * v[:, 1:2] + wi * v[:, 2:3]


def leaf_eval(p, wi, wo, T):
    """eval_pdf of a leaf: (value, margin); eval = pdf in all four.  margin: the distance of |cos| from 1 where the table's range test
    is a branch (1 elsewhere)"""
    c = np.sum(wo * wi, 1)
    one = np.ones(len(c))
    if p.kind == ISOTROPIC:
        return np.full(len(c), T(1 / (4 * np.pi)), T), one
    if p.kind == HG:
        return hg_eval(p.g, c, T), one
    if p.kind == RAYLEIGH:
        return T(3 / 16) * T(1 / np.pi) * (T(1) + c * c), one                                  # rayleigh.cpp:50-52
    return p.table.eval_pdf_normalized(-c, T) * T(1 / (2 * np.pi)), 1 - np.abs(c).astype(np.float64)      # tabphase.cpp:105-118


def leaf_sample(p, wi, s2, T):
    """sample of a leaf -> wo, pdf, margin (the weight is 1).  margin: the least distance from a branch point: |cos| = 1 and, for a table,
    the ends of the chosen interval in the interval's own coordinate t."""
    sx, sy = s2[:, 0], s2[:, 1]
    phi = T(2 * np.pi) * sy
    sp, cp = np.sin(phi), np.cos(phi)
    if p.kind == TABULATED:                                                                  # tabphase.cpp:77-103
        c, _, t = p.table.sample(sx, T)
        st = np.sqrt(np.maximum(T(1) - c * c, T(0)))
        wo = -_to_world(wi, np.stack([st * cp, st * sp, c], 1), T)
        pdf = p.table.eval_pdf_normalized(c, T) * T(1 / (2 * np.pi))
        margin = np.minimum(1 - np.abs(c), np.minimum(t, 1 - t)).astype(np.float64)
        return wo, pdf, np.nan_to_num(margin, nan=0.0)
    if p.kind == RAYLEIGH:                                                                   # rayleigh.cpp:54-74
        z = T(2) * (T(2) * sx - T(1))
        tmp = np.sqrt(z * z + T(1))
        c = np.cbrt(z + tmp) + np.cbrt(z - tmp)
        st = np.sqrt(np.maximum(T(1) - c * c, T(0)))
        wo = _to_world(wi, np.stack([st * cp, st * sp, c], 1), T)
        return wo, T(3 / 16) * T(1 / np.pi) * (T(1) + c * c), (1 - np.abs(c)).astype(np.float64)
    if p.kind == HG:                                                                         # hg.cpp:71-99
        g = T(p.g)
        sqr_term = (T(1) - g * g) / (T(1) - g + T(2) * g * sx)
        c = (T(1) + g * g - sqr_term * sqr_term) / (T(2) * g) if abs(float(g)) >= 2.0 ** -24 else T(1) - T(2) * sx
        st = np.sqrt(np.maximum(T(1) - c * c, T(0)))
        wo = _to_world(wi, np.stack([st * cp, st * sp, -c], 1), T)
        return wo, hg_eval(g, -c, T), (1 - np.abs(c)).astype(np.float64)
    z = T(1) - T(2) * sy                                                                     # isotropic.cpp:39-47 + warp::square_to_uniform_sphere
    r = np.sqrt(np.maximum(T(1) - z * z, T(0)))                                              # (include/mitsuba/core/warp.h: z from sample.y, phi from sample.x)
    phi = T(2 * np.pi) * sx
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1), np.full(len(z), T(1 / (4 * np.pi)), T), (1 - np.abs(z)).astype(np.float64)


def sample(p, wi, smp, T=np.float64):
    """PhaseFunction::sample(ctx, mei, s1, (s2x, s2y)) -> dict wo (n, 3), weight, pdf, margin"""
    wi = np.asarray(wi, T); smp = np.asarray(smp, T)
    if p.kind != BLEND:
        wo, pdf, m = leaf_sample(p, wi, smp[:, 1:], T)
        return {"wo": wo, "weight": np.ones(len(pdf), T), "pdf": pdf, "margin": m}
    w = T(p.weight); s1 = smp[:, 0]                                                          # blendphase.cpp:122-153
    m0 = s1 > w
    wo0, pdf0s, mg0 = leaf_sample(p.children[0], wi, smp[:, 1:], T)
    wo1, pdf1s, mg1 = leaf_sample(p.children[1], wi, smp[:, 1:], T)
    wo = np.where(m0[:, None], wo0, wo1)
    e1, me1 = leaf_eval(p.children[1], wi, wo, T); e0, me0 = leaf_eval(p.children[0], wi, wo, T)
    pdf0 = np.where(m0, pdf0s, e0); pdf1 = np.where(m0, e1, pdf1s)
    pdf_w = w * pdf1 + (T(1) - w) * pdf0
    num = np.where(m0, w * e1 + (T(1) - w) * T(1) * pdf0s, w * T(1) * pdf1s + (T(1) - w) * e0)
    with np.errstate(divide="ignore", invalid="ignore"):
        weight = num * np.where(pdf_w > 0, T(1) / pdf_w, T(0))
    margin = np.minimum(np.where(m0, np.minimum(mg0, me1), np.minimum(mg1, me0)), np.abs(s1 - w).astype(np.float64))
    return {"wo": wo, "weight": weight, "pdf": pdf_w, "margin": margin}


def eval_pdf(p, wi, wo, T=np.float64):
    """PhaseFunction::eval_pdf -> (value, margin); the pdf equals the value in every family"""
    wi = np.asarray(wi, T); wo = np.asarray(wo, T)
    if p.kind != BLEND:
        return leaf_eval(p, wi, wo, T)
    v0, m0 = leaf_eval(p.children[0], wi, wo, T); v1, m1 = leaf_eval(p.children[1], wi, wo, T)
    w = T(p.weight)
    return v1 * w + (v0 - v0 * w), np.minimum(m0, m1)                                        # dr::lerp: fmadd(b, t, fnmadd(a, t, a))
