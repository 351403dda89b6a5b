"""The environment-map emitter as float64 mathematics (src/emitters/envmap.cpp, Hierarchical2D of include/mitsuba/core/distr_2d.h,
interval_to_linear of warp.h), for tests/test_envmap.py and tests/test_envmap_gpu.py.  No hierarchy is built: the density is a sum
of tensor-product hat functions, its integrals are sums of integrated hats, and the inverse of the warp reads the probability of a
dyadic block of patches from one summed-area table.  DESIGN.md ("Envmap sampling against float64") has the formulas.

Notation: the map has h rows and w columns; the node grid has h rows and w + 1 columns (column w repeats column 0), so there are
w x (h - 1) bilinear patches on the unit square (u, v).  u is the warp's coordinate: the direction's azimuth / 2 pi minus the
half-texel shift 0.5 / w, wrapped to [0, 1); v is the polar angle / pi."""
import numpy as np

F32_EPS = 2.0 ** -24            # one float32 rounding of a value in [0, 1] (half an ulp of 1)
EPSILON = 2.0 ** -24            # dr::Epsilon<float>: envmap.cpp clamps sin^2(theta) to its square before the rsqrt
ITL_SWITCH = 1e-4               # warp.h interval_to_linear: the linear case below this relative difference
ANGLE_ERR = 5e-7                # rad: the accuracy of atan2 and acos that test_oracle_pins.py pins
NODE_ANGLE_ERR = 2.0 ** -22     # rad: a node row's angle y * (pi / (h - 1)) in float32: two roundings of a value up to pi (half a float there is 2^-23)
LUMINANCE = np.array([0.212671, 0.715160, 0.072169])


def _hat_cdf(pos, n):
    """C[k, x] = integral over [0, pos[k]] of the hat function of node x on a grid of n intervals over [0, 1]"""
    t = np.asarray(pos, np.float64)[:, None] * n - np.arange(n + 1)[None, :]
    full = lambda t: np.where(t <= -1, 0.0, np.where(t <= 0, 0.5 * (t + 1) ** 2, np.where(t <= 1, 0.5 + t - 0.5 * t * t, 1.0)))
    return (full(t) - full(-np.arange(n + 1, dtype=np.float64)[None, :])) / n


class EnvmapRef:
    def __init__(self, texels, scale=1.0, to_world=None):
        """texels: (h, w, 3) as the loader read them back; to_world: the 3x3 linear part of the emitter's transform"""
        t = np.asarray(texels, np.float64)
        self.h, self.w = h, w = t.shape[0], t.shape[1]
        self.scale = float(scale)
        self.to_world = np.eye(3) if to_world is None else np.asarray(to_world, np.float64).reshape(3, 3)
        self.to_local = np.linalg.inv(self.to_world)
        self.rgb = np.concatenate([t, t[:, :1]], axis=1)                                  # the wrap column
        lum = np.maximum(self.rgb @ LUMINANCE, 0.0)
        L = lum * np.sin(np.pi * np.arange(h) / (h - 1))[:, None]                          # node density
        A = 0.25 * (L[:-1, :-1] + L[:-1, 1:] + L[1:, :-1] + L[1:, 1:])                     # patch averages
        self.D = L / A.mean()                                                            # normalised nodes: the interpolant integrates to 1
        self.lum_n = lum / A.mean()                                                      # the nodes without their sin(theta) factor
        self.P = A / A.sum()                                                             # probability of each patch, (h - 1, w)
        self.S = np.zeros((h, w + 1)); self.S[1:, 1:] = self.P.cumsum(0).cumsum(1)       # summed-area table
        n = max(w, h - 1)
        self.n_levels = int(np.ceil(np.log2(n))) if n > 1 else 0                          # binary choices per coordinate
        # the largest slopes of the density and of the radiance per unit u and per unit v (attained on patch edges)
        self.grad = (np.abs(np.diff(self.D, axis=1)).max() * w, np.abs(np.diff(self.D, axis=0)).max() * (h - 1))
        R = self.rgb * self.scale
        self.rad_grad = (np.abs(np.diff(R, axis=1)).max() * w, np.abs(np.diff(R, axis=0)).max() * (h - 1))

    # ---- directions and the unit square
    def dir_to_uv(self, d, wrap_v=True):
        """world direction -> (u, v, sin theta), as envmap.cpp writes it: u = atan2(x, -z) / 2 pi minus the half-texel shift,
        v = acos(y) / pi on the direction as given (unit to float32 precision, not re-normalised), both minus their floor.  So the
        exact south pole y = -1, v = 1, wraps to v = 0 and reads the north pole's row: in float32 that is every direction within
        2^-12.5 rad of the south pole.  sin theta = sqrt(x^2 + z^2).  wrap_v=False keeps v = 1 (where a sampled point is looked for).
        The reference's atan2 (Dr.Jit's) returns 0 where both arguments are zero, whatever their signs; IEEE's gives pi for (+0, -0)."""
        dl = np.asarray(d, np.float64) @ self.to_local.T
        u = np.where((dl[..., 0] == 0) & (dl[..., 2] == 0), 0.0, np.arctan2(dl[..., 0], -dl[..., 2])) / (2 * np.pi) - 0.5 / self.w
        v = np.arccos(np.clip(dl[..., 1], -1, 1)) / np.pi
        return u - np.floor(u), v - np.floor(v) if wrap_v else v, np.hypot(dl[..., 0], dl[..., 2])

    def uv_to_dir(self, u, v):
        phi, theta = 2 * np.pi * (np.asarray(u, np.float64) + 0.5 / self.w), np.pi * np.asarray(v, np.float64)
        dl = np.stack([np.sin(phi) * np.sin(theta), np.cos(theta), -np.cos(phi) * np.sin(theta)], -1)
        return dl @ self.to_world.T

    def _patch(self, u, v):
        x, y = np.asarray(u, np.float64) * self.w, np.asarray(v, np.float64) * (self.h - 1)
        i = np.clip(np.floor(x), 0, self.w - 1).astype(np.int64); j = np.clip(np.floor(y), 0, self.h - 2).astype(np.int64)
        return i, j, x - i, y - j

    @staticmethod
    def _bilinear(T, i, j, a, b):
        a = a[..., None] if T.ndim == 3 else a; b = b[..., None] if T.ndim == 3 else b
        return (T[j, i] * (1 - a) + T[j, i + 1] * a) * (1 - b) + (T[j + 1, i] * (1 - a) + T[j + 1, i + 1] * a) * b

    # ---- densities and radiance
    def density(self, u, v):
        """the target density on the unit square"""
        return self._bilinear(self.D, *self._patch(u, v))

    def pdf(self, d):
        """solid-angle density of a world direction, with envmap.cpp's clamp: density / (2 pi^2 max(sin theta, Epsilon))"""
        u, v, st = self.dir_to_uv(d)
        return self.density(u, v) / (2 * np.pi ** 2 * np.maximum(st, EPSILON))

    def radiance(self, d):
        u, v, _ = self.dir_to_uv(d)
        return self._bilinear(self.rgb, *self._patch(u, v)) * self.scale

    # ---- integration
    def box_masses(self, u_edges, v_edges):
        """exact integrals of the density over the boxes of a grid: (len(v_edges) - 1, len(u_edges) - 1)"""
        return np.diff(_hat_cdf(v_edges, self.h - 1), axis=0) @ self.D @ np.diff(_hat_cdf(u_edges, self.w), axis=0).T

    # ---- the inverse warp
    def _block(self, x0, x1, y0, y1):
        x0, x1 = np.clip(x0, 0, self.w), np.clip(x1, 0, self.w); y0, y1 = np.clip(y0, 0, self.h - 1), np.clip(y1, 0, self.h - 1)
        S = self.S
        return S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0]

    def invert_patch(self, i, j, a, b):
        """The sample (sx, sy) that the warp maps to the point (a, b) of patch (column i, row j), and the factors (qx, qy) by which
        the levels above the patch contract sx and sy: the products of the conditional probabilities of the column choices and of
        the row choices (qx qy is the patch's probability).
        In the patch: v is drawn from the linear density through the two row sums, then u from the linear density through the
        two columns at that v; each has the closed-form CDF t (2 f0 + (f1 - f0) t) / (f0 + f1).  Above it the warp spends one
        binary choice per level and coordinate, rows before columns, on the probabilities of the four children of the dyadic
        block that holds the patch: the choice maps [0, 1] affinely onto the chosen child's share of it."""
        D = self.D
        v00, v10, v01, v11 = D[j, i], D[j, i + 1], D[j + 1, i], D[j + 1, i + 1]
        lin = lambda f0, f1, t: t * (2 * f0 + (f1 - f0) * t) / (f0 + f1)
        with np.errstate(invalid="ignore", divide="ignore"):
            sy = lin(v00 + v10, v01 + v11, b)
            sx = lin(v00 * (1 - b) + v01 * b, v10 * (1 - b) + v11 * b, a)
            qx, qy = np.ones_like(sx), np.ones_like(sy)
            for m in range(self.n_levels):
                c = 1 << m
                bx, by = (i >> (m + 1)) << (m + 1), (j >> (m + 1)) << (m + 1)
                m00, m10 = self._block(bx, bx + c, by, by + c), self._block(bx + c, bx + 2 * c, by, by + c)
                m01, m11 = self._block(bx, bx + c, by + c, by + 2 * c), self._block(bx + c, bx + 2 * c, by + c, by + 2 * c)
                right, lower = ((i >> m) & 1) == 1, ((j >> m) & 1) == 1
                r0, r1 = m00 + m10, m01 + m11
                c0, c1 = np.where(lower, m01, m00), np.where(lower, m11, m10)
                sx = np.where(right, c0 + sx * c1, sx * c0) / (c0 + c1)
                sy = np.where(lower, r0 + sy * r1, sy * r0) / (r0 + r1)
                qx = qx * np.where(right, c1, c0) / (c0 + c1); qy = qy * np.where(lower, r1, r0) / (r0 + r1)
        return sx, sy, qx, qy

    def itl_error(self, i, j, a, b):
        """The patch-coordinate error that float32 interval_to_linear may make, for u and for v: N roundings of 2^-24 relative to
        f0 + f1 reach the numerator f0 - sqrt(lerp(f0^2, f1^2, s)) (the two squares and the lerp's two operations at half weight
        after the root, the root, and the two roundings in each of f0 and f1: N = 5), divided by |f0 - f1|; below the switch the
        identity stands in for a CDF that differs from it by at most |f0 - f1| / (4 (f0 + f1))."""
        D = self.D
        v00, v10, v01, v11 = D[j, i], D[j, i + 1], D[j + 1, i], D[j + 1, i + 1]
        def err(f0, f1):
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.abs(f0 - f1) / (f0 + f1)
                return np.where(rel > ITL_SWITCH, np.minimum(5 * F32_EPS / rel, 5 * F32_EPS / ITL_SWITCH), ITL_SWITCH / 4)
        return err(v00 * (1 - b) + v01 * b, v10 * (1 - b) + v11 * b), err(v00 + v10, v01 + v11)

    def level_error(self):
        """The sample-space error of the float32 descent.  A level multiplies, subtracts and divides the sample (3 roundings of a
        value in [0, 1]), forms one sum of two children and the sum of the two sums (2), and reads masses that float32 additions
        built: 3 additions per level below it plus the patch average's 4 operations (3 l + 1 at level l).  Summed over the levels."""
        K = self.n_levels
        return (6 * K + 1.5 * K * (K + 1)) * F32_EPS

    def uv_error(self, sin_theta, rounded=True):
        """(du, dv): how far the (u, v) of a float32 direction may lie from the (u, v) it was made from.  The angle accuracy of
        atan2 / acos, plus one float32 rounding of the direction's components: 2^-24 of a unit vector moves its polar angle and
        its azimuth by 2^-24 / sin theta each.  Both in (u, v) units, with a margin of 4 for the 3x3 transform.
        rounded=False: the map-frame direction is the very float32 vector that the float64 formulas are given (a direction handed
        to eval / pdf_direction of a map without a transform), so no component was rounded and the angle accuracy alone remains."""
        st = np.maximum(np.asarray(sin_theta, np.float64), EPSILON)
        r = F32_EPS / st if rounded else 0.0
        return 4 * (ANGLE_ERR + r) / (2 * np.pi), 4 * (ANGLE_ERR + r) / np.pi

    # ---- At the poles
    # envmap.cpp evaluates u = atan2(x, -z) / 2 pi, v = acos(y) / pi, uv -= floor(uv), and 1 / sin theta = rsqrt(max(x^2 + z^2,
    # Epsilon^2)).  Where the map-frame y is exactly +1, v = 0; where it is exactly -1, v = 1 and the floor sends it to 0 as well.
    # Node row 0 of the density is lum * sin(0) = 0 in every column, so the density is exactly 0 for every azimuth, and with the
    # clamp the pdf is 0 / max(sin theta, Epsilon) = 0: finite, exactly zero, never negative, whatever x and z hold (they are
    # below 2^-12 in a unit vector, or zero).  The radiance is texel row 0 interpolated at the azimuth's u, for y = -1 too; at
    # the exact poles x = z = 0, the reference's atan2 returns 0 (see dir_to_uv), and u = -0.5 / w wraps to 1 - 0.5 / w.  `pdf`, `density` and `radiance` above compute
    # just that.  The nearest float32 unit vectors off a pole have y = +-(1 - 2^-24), sin theta = 3.45e-4, where the pdf is back
    # to about (h - 1) D[1][u] / (2 pi^3): the pole itself is a removable zero of measure 1.9e-7 sr.
    @property
    def reads_direction_as_given(self):
        """no transform: the map-frame direction is the world direction, bit for bit"""
        return np.array_equal(self.to_world, np.eye(3))

    def at_pole(self, d):
        """where a float32 direction's map-frame y is exactly +-1 (for a map that reads the direction as given)"""
        return np.abs(np.asarray(d, np.float32)[..., 1]) == 1

    def round_trip(self, d, sx, sy):
        """Check a: invert the warp at returned directions d.  Returns (ratio, error, patch probability, located) per sample:
        ratio is the larger of |sx' - sx| / bound_x and |sy' - sy| / bound_y (ratio <= 1 is the assertion), error the larger of
        the two differences.  `located` is False where the direction's own (u, v) uncertainty exceeds a quarter of a patch (next
        to a pole a float32 direction has no azimuth left): nothing can be inverted there.  The warp is discontinuous across some patch edges, so a point within the
        uncertainty of an edge may belong to the neighbouring patch: the better of the patches it may lie in counts."""
        u, v, st = self.dir_to_uv(d, wrap_v=False)
        du, dv = self.uv_error(st)
        located = (du * self.w <= 0.25) & (dv * (self.h - 1) <= 0.25)
        lvl = self.level_error()
        best = None
        for ou in (-du, du):
            for ov in (-dv, dv):
                i, j, _, _ = self._patch(np.mod(u + ou, 1.0), np.clip(v + ov, 0, 1))
                c = 0.5 / self.w                                                                  # (the seam: u near 1 belongs next to column 0)
                a = np.clip(np.mod(u - i / self.w - c + 0.5, 1.0) - 0.5 + c, 0, 1 / self.w) * self.w
                b = np.clip(v * (self.h - 1) - j, 0, 1)
                ix, iy, qx, qy = self.invert_patch(i, j, a, b)
                p = self.P[j, i]
                ea, eb = self.itl_error(i, j, a, b)
                # a patch-coordinate error e moves sx by at most 2 e qx (the in-patch density is at most twice its mean), sy by 2 e qy
                # and an error e in b changes the ratio of the two column values that the draw of a reads by at most
                # 2 e / min(b, 1 - b) in the logarithm, which moves sx by at most an eighth of that (|d sx / d ln ratio| <= 1 / 8)
                db = dv * (self.h - 1)
                bx = lvl + 2 * qx * (ea + du * self.w) + qx * db / (4 * np.maximum(np.minimum(b, 1 - b), 1e-300))
                by = lvl + 2 * qy * (eb + db)
                with np.errstate(invalid="ignore"):
                    ratio = np.maximum(np.abs(ix - sx) / bx, np.abs(iy - sy) / by)
                    raw = np.maximum(np.abs(ix - sx), np.abs(iy - sy))
                cand = [np.where(np.isfinite(ratio), ratio, np.inf), np.where(np.isfinite(raw), raw, np.inf), p]
                if best is None:
                    best = cand
                else:
                    take = cand[0] < best[0]
                    best = [np.where(take, c, b_) for c, b_ in zip(cand, best)]
        return best[0], best[1], best[2], located

    # ---- tolerances of checks b and d
    #: float32 roundings between the node values and the returned pdf, each 2^-24 relative: the luminance (3), its product with
    #: sin theta (2), the normalisation (2), three lerps of two operations (6), sin^2 theta and its rsqrt (3 at half weight: 2),
    #: the two final products (2), and the weight's division where the weight is concerned (1): 18
    RTOL = 18 * F32_EPS

    def pdf_tolerance(self, pdf, sin_theta, rounded=True):
        du, dv = self.uv_error(sin_theta, rounded)
        return self.RTOL * pdf + (self.grad[0] * du + self.grad[1] * dv) / (2 * np.pi ** 2 * np.maximum(sin_theta, EPSILON))

    def local_slopes(self, T, u, v, du, dv):
        """the largest slopes per unit u and per unit v that the bilinear interpolant of the node table T (the density's D, or the
        texels) takes within (du, dv) of the point (u, v): the two partial derivatives, each linear in the other coordinate
        within a patch, at the point and at the four corners of the box (which reach every patch that the box touches)"""
        T = T.reshape(T.shape[0], T.shape[1], -1)
        su, sv = 0.0, 0.0
        for ou, ov in ((0, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)):
            i, j, a, b = self._patch(np.mod(u + ou * du, 1.0), np.clip(v + ov * dv, 0, 1))
            a, b = a[..., None], b[..., None]
            su = np.maximum(su, np.abs((1 - b) * (T[j, i + 1] - T[j, i]) + b * (T[j + 1, i + 1] - T[j + 1, i])).max(-1) * self.w)
            sv = np.maximum(sv, np.abs((1 - a) * (T[j + 1, i] - T[j, i]) + a * (T[j + 1, i + 1] - T[j, i + 1])).max(-1) * (self.h - 1))
        return su, sv

    def pole_tolerances(self, pdf, rad, u, v, sin_theta):
        """pdf_tolerance and radiance_tolerance of a direction that is read as given (rounded=False), with the slopes at the spot
        instead of the map's largest: next to a pole the density is b D[1][u] (rows 0 and 1) and the map's largest
        slope, taken somewhere on the equator of a map that spans three decades, says nothing about it.
        The pdf gets one more term, which the relative RTOL cannot hold next to the south pole: the float32 node table carries
        lum * sin(angle) with the angle NODE_ANGLE_ERR off, an absolute error of that times lum.  Row h - 1 is lum * sin(fl(pi))
        = -8.7e-8 lum in the reference and here, not 0, and one float off that pole the row above weighs (1 - b) = 1e-4 (h - 1)."""
        du, dv = self.uv_error(sin_theta, rounded=False)
        node = NODE_ANGLE_ERR * self._bilinear(self.lum_n, *self._patch(u, v))
        gu, gv = self.local_slopes(self.D, u, v, du, dv); ru, rv = self.local_slopes(self.rgb * self.scale, u, v, du, dv)
        return (self.RTOL * pdf + (node + gu * du + gv * dv) / (2 * np.pi ** 2 * np.maximum(sin_theta, EPSILON)),
                self.RTOL * np.abs(rad) + (ru * du + rv * dv)[..., None])

    def radiance_tolerance(self, rad, sin_theta, rounded=True):
        du, dv = self.uv_error(sin_theta, rounded)
        return self.RTOL * np.abs(rad) + (self.rad_grad[0] * du + self.rad_grad[1] * dv)[..., None]


def chi_square(counts, expected, min_expected=5.0):
    """Pearson's test with the cells of low expectation pooled into one (the reference's ChiSquareTest): (statistic, dof, p-value)"""
    from scipy.stats import chi2
    counts = np.asarray(counts, np.float64).ravel(); expected = np.asarray(expected, np.float64).ravel()
    low = expected < min_expected
    c, e = counts[~low], expected[~low]
    if low.any() and expected[low].sum() > 0:
        c, e = np.append(c, counts[low].sum()), np.append(e, expected[low].sum())
    elif low.any() and counts[low].sum() > 0:
        return np.inf, len(e) - 1, 0.0           # samples where the density is zero
    stat = float(((c - e) ** 2 / e).sum()); dof = len(e) - 1
    return stat, dof, float(chi2.sf(stat, dof))


def sidak(alpha, n_tests):
    return 1.0 - (1.0 - alpha) ** (1.0 / n_tests)
