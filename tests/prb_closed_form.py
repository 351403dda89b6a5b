"""Float64 closed forms for the PRB gradient tests (test_prb_closed_form.py, test_prb_closed_form_gpu.py).  numpy only.

Two references, both independent of the renderer's code:

* per-pixel chord lengths: camera rays of a perspective sensor (src/sensors/perspective.cpp: fov along x, aspect =
  width / height, look_at) built in float64 on a sub-pixel grid, intersected with an axis-aligned box by a slab test.  With a
  box filter a pixel is the mean over its footprint, so for a pure absorber in front of a constant emitter
  L_pk = mean_footprint(Le_k exp(-sigma_k l)) and dL_pk / dsigma_k = mean_footprint(-l Le_k exp(-sigma_k l)).
* the infinite slab in single scattering: thickness d, a ray along the normal, HG phase p_g(mu) with mu the cosine between the
  ray and the scattered direction, constant emitter Le on both sides:
      L = exp(-sigma d) Le + a sigma Le int_0^d exp(-sigma s) int_{-1}^{1} 2 pi p_g(mu) exp(-sigma l(s, mu)) dmu ds,
  l = (d - s) / mu for mu > 0 and s / (-mu) for mu < 0.  The s integral is done in closed form per mu (s + l is linear in s),
  which leaves a smooth integrand in mu: Gauss-Legendre on [-1, 0] and [0, 1] converges to round-off.  Derivatives:
      dL/dsigma = -d exp(-sigma d) Le + a Le int int 2 pi p_g (1 - sigma (s + l)) exp(-sigma (s + l))
      dL/da = single / a,   dL/dg = a sigma Le int int 2 pi (dp_g/dg) exp(-sigma (s + l)).
"""
import numpy as np


# ---------------------------------------------------------------------------------------------------------- camera + box
def look_at(origin, target, up):
    """Mitsuba's Transform4f.look_at: columns (left, up', dir), origin."""
    o, t, u = (np.asarray(v, np.float64) for v in (origin, target, up))
    d = (t - o) / np.linalg.norm(t - o)
    left = np.cross(u, d); left /= np.linalg.norm(left)
    return o, left, np.cross(d, left), d


def camera_directions(origin, target, up, fov_x, width, height, sub):
    """World-space unit directions of a sub x sub midpoint grid in every pixel of a width x height film: (H, W, sub*sub, 3).
    Film position (u, v) in [0, 1]^2 maps to the camera-space direction ((1 - 2u) tan(fov/2), (1 - 2v) tan(fov/2) / aspect, 1)."""
    o, left, upv, fwd = look_at(origin, target, up)
    th = np.tan(np.radians(fov_x) / 2.0); aspect = width / height
    j = (np.arange(sub) + 0.5) / sub
    jx, jy = np.meshgrid(j, j)                                            # (sub, sub): x along the last axis
    u = (np.arange(width)[None, :, None] + jx.reshape(-1)[None, None, :]) / width
    v = (np.arange(height)[:, None, None] + jy.reshape(-1)[None, None, :]) / height
    u, v = np.broadcast_arrays(u, v)
    x, y = (1.0 - 2.0 * u) * th, (1.0 - 2.0 * v) * th / aspect
    d = x[..., None] * left + y[..., None] * upv + fwd
    return o, d / np.linalg.norm(d, axis=-1, keepdims=True)


def box_span(o, d, lo, hi):
    """Slab test: entry and exit distance of rays o + t d through the box [lo, hi] (t0 > t1 where the ray misses)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        ta, tb = (lo - o) * inv, (hi - o) * inv
    t0 = np.max(np.minimum(ta, tb), axis=-1); t1 = np.min(np.maximum(ta, tb), axis=-1)
    return np.maximum(t0, 0.0), t1


def pixel_chords(origin, target, up, fov_x, width, height, lo, hi, sub=48):
    """Chord length l of every sub-pixel ray through the box: (H, W, sub*sub), 0 where the ray misses."""
    o, d = camera_directions(origin, target, up, fov_x, width, height, sub)
    t0, t1 = box_span(o, d, lo, hi)
    return np.maximum(t1 - t0, 0.0)


def absorber_pixels(chords, sigma, Le):
    """(value, d value / d sigma_k) of every pixel and channel of a pure absorber, box filter: (H, W, 3) each."""
    sigma, Le = np.asarray(sigma, np.float64), np.asarray(Le, np.float64)
    e = np.exp(-chords[..., None] * sigma) * Le                           # (H, W, n, 3)
    return e.mean(axis=2), (-chords[..., None] * e).mean(axis=2)


# ------------------------------------------------------------------------------------------ infinite slab, single scattering
def hg(g, mu):
    """HG phase value for the cosine mu between propagation directions (forward peak at mu = 1 for g > 0)."""
    return (1.0 - g * g) / (4.0 * np.pi * (1.0 + g * g - 2.0 * g * mu) ** 1.5)


def hg_dg(g, mu):
    t = 1.0 + g * g - 2.0 * g * mu
    return hg(g, mu) * (-2.0 * g / (1.0 - g * g) - 1.5 * (2.0 * g - 2.0 * mu) / t)


def _phi(x):
    """int_0^1 exp(-x t) dt"""
    x = np.asarray(x, np.float64)
    small = np.abs(x) < 1e-4
    xs = np.where(small, 1.0, x)
    return np.where(small, 1.0 - x / 2.0 + x * x / 6.0, -np.expm1(-xs) / xs)


def _psi(x):
    """int_0^1 t exp(-x t) dt"""
    x = np.asarray(x, np.float64)
    small = np.abs(x) < 1e-2
    xs = np.where(small, 1.0, x)
    series = 0.5 - x / 3.0 + x * x / 8.0 - x ** 3 / 30.0 + x ** 4 / 144.0
    return np.where(small, series, (1.0 - (1.0 + xs) * np.exp(-xs)) / (xs * xs))


def _mu_nodes(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return np.concatenate([(x - 1.0) / 2.0, (x + 1.0) / 2.0]), np.concatenate([w, w]) / 2.0   # [-1, 0] then [0, 1]


def _inner(sigma, d, mu):
    """A(mu) = int_0^d exp(-sigma (s + l)) ds and B(mu) = int_0^d (s + l) exp(-sigma (s + l)) ds."""
    fwd = mu > 0
    m = np.abs(mu)
    # mu > 0: s + l = d + u q with u = d - s, q = 1/mu - 1;   mu < 0: s + l = s c with c = 1 + 1/|mu|
    q = np.where(fwd, 1.0 / m - 1.0, 0.0); c = np.where(fwd, 1.0, 1.0 + 1.0 / m)
    ed = np.exp(-sigma * d)
    A = np.where(fwd, ed * d * _phi(sigma * q * d), d * _phi(sigma * c * d))
    B = np.where(fwd, d * A + q * ed * d * d * _psi(sigma * q * d), c * d * d * _psi(sigma * c * d))
    return A, B


def slab_single_scatter(sigma, albedo, g, d, Le, n=128):
    """Per-channel dict of the primal L (unscattered + single scattered), 'single' and dL/dsigma, dL/dalbedo, dL/dg (arrays of the
    channels' shape).  sigma > 0 in every channel."""
    sigma, albedo, Le = (np.atleast_1d(np.asarray(v, np.float64)) for v in (sigma, albedo, Le))
    mu, w = _mu_nodes(n)
    out = {k: np.zeros(np.broadcast(sigma, albedo, Le).shape) for k in ("L", "single", "d_sigma", "d_albedo", "d_g")}
    for i in range(out["L"].size):
        s, a, le = np.broadcast_to(sigma, out["L"].shape)[i], np.broadcast_to(albedo, out["L"].shape)[i], np.broadcast_to(Le, out["L"].shape)[i]
        A, B = _inner(s, d, mu)
        p, dp = 2.0 * np.pi * hg(g, mu), 2.0 * np.pi * hg_dg(g, mu)
        single = a * s * le * np.sum(w * p * A)
        ed = np.exp(-s * d) * le
        out["L"].flat[i] = ed + single
        out["single"].flat[i] = single
        out["d_sigma"].flat[i] = -d * ed + a * le * np.sum(w * p * (A - s * B))
        out["d_albedo"].flat[i] = single / a if a != 0 else s * le * np.sum(w * p * A)
        out["d_g"].flat[i] = a * s * le * np.sum(w * dp * A)
    return out
