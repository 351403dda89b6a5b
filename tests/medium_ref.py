"""Float64 restatement of medium sampling (test_medium.py, test_medium_gpu.py).  numpy only, written from the reference's sources and
independent of the renderer's and the oracle's code:

* src/volumes/grid.cpp: a one-channel grid is looked up trilinearly with clamp-to-edge texel fetches, texel centres at (i + 1/2) / res
  (interpolate_1, and :510-524 for the weights); the lookup point is m_to_local * p (:556).
* src/render/volume.cpp:15-17 + include/mitsuba/render/volume.h:99-109: m_to_local = to_world^-1, the world AABB is the bound of the eight
  corners of the unit cube under m_to_local^-1.  src/volumes/grid.cpp:296-300 + include/mitsuba/render/volumegrid.h:26-30: with
  use_grid_bbox, m_to_local = scale(1 / extents) * translate(-min) * to_world^-1 with the box of the file's header (volumegrid.cpp:60-64).
* include/mitsuba/core/bbox.h:303-340: the slab test (Williams et al.), its NaN-safe minimum / maximum.
* src/render/medium.cpp:40-82: mint = max(0, slab entry), maxt = min(ray.maxt, slab exit), sampled_t = mint - log(1 - sample) / majorant,
  valid = hit && sampled_t <= maxt, t = valid ? sampled_t : inf, p = o + sampled_t d.
* src/media/heterogeneous.cpp:163-200: majorant = scale * max(grid), sigma_t = scale * grid(p) (0 where not valid: the lookup is masked),
  sigma_s = sigma_t * albedo, sigma_n = majorant - sigma_t.
* src/media/homogeneous.cpp:121-126,153-181: sigma_t = value * scale per channel, the majorant is sigma_t, the sampling rate is its
  `channel` entry, sigma_n = 0, no bounding box (mint = 0, maxt = ray.maxt); sigma_t and sigma_s are 0 where not valid.

Every formula takes `dt`: float64 is the reference; float32 is the same formula in single precision and exists only to measure the
K table: how far single precision alone moves each output.  Arrays of grids are indexed (z, y, x).
"""
import numpy as np

import grid_grad_ref as gg

EPS32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- transforms
def translate(v):
    m = np.eye(4); m[:3, 3] = v
    return m


def scale(v):
    return np.diag(list(np.broadcast_to(np.asarray(v, np.float64), (3,))) + [1.0])


def rotate(axis, degrees):
    """Rotation about `axis` (normalised here) by `degrees`: Rodrigues' formula, counter-clockwise seen against the axis."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4); m[:3, :3] = c * np.eye(3) + s * k + (1 - c) * np.outer(a, a)
    return m


def compose(steps):
    """A <transform> element: its children apply in order, each on the left of what came before.  steps: ("scale", v), ("translate", v),
    ("rotate", axis, degrees)."""
    m = np.eye(4)
    for st in steps:
        m = {"scale": scale, "translate": translate, "rotate": rotate}[st[0]](*st[1:]) @ m
    return m


def volume_frame(to_world, header_box=None):
    """(to_local 3 x 4, aabb_min, aabb_max) of a volume: to_local = [bbox_transform *] to_world^-1; the AABB bounds the unit cube's corners
    under to_local^-1.  header_box = (min, max) of the file when use_grid_bbox is set."""
    tl = np.linalg.inv(np.asarray(to_world, np.float64))
    if header_box is not None:
        lo, hi = (np.asarray(v, np.float64) for v in header_box)
        tl = scale(1.0 / (hi - lo)) @ translate(-lo) @ tl
    tw = np.linalg.inv(tl)
    c = np.array([[x, y, z, 1.0] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    w = c @ tw.T
    return tl[:3], w[:, :3].min(0), w[:, :3].max(0)


# ------------------------------------------------------------------------------------------------------------- grid lookup
def trilinear(grid, p, dt=np.float64):
    """The clamped trilinear lookup at local points p (..., 3).  float64: grid_grad_ref.trilinear; float32: the same steps in single."""
    if dt == np.float64:
        return gg.trilinear(grid, p)
    g = np.asarray(grid, dt); p = np.asarray(p, dt)
    rz, ry, rx = g.shape

    def axis(v, n):
        f = v * dt(n) - dt(0.5)
        fl = np.floor(f)
        i = np.clip(fl, -4.0, n + 4.0).astype(np.int64)
        return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), f - fl
    x0, x1, tx = axis(p[..., 0], rx); y0, y1, ty = axis(p[..., 1], ry); z0, z1, tz = axis(p[..., 2], rz)
    lerp = lambda a, b, t: a + (b - a) * t
    c0 = lerp(lerp(g[z0, y0, x0], g[z0, y0, x1], tx), lerp(g[z0, y1, x0], g[z0, y1, x1], tx), ty)
    c1 = lerp(lerp(g[z1, y0, x0], g[z1, y0, x1], tx), lerp(g[z1, y1, x0], g[z1, y1, x1], tx), ty)
    return lerp(c0, c1, tz)


def corner_range(grid, p):
    """(max |corner|, max corner - min corner) over the eight texels of the lookup at p: what the lookup's error scales with"""
    idx, _ = gg.corners(np.asarray(p, np.float64), np.shape(grid))
    v = np.asarray(grid, np.float64).reshape(-1)[idx]
    return np.abs(v).max(-1), v.max(-1) - v.min(-1)


def to_local_point(to_local, p, dt=np.float64):
    A = np.asarray(to_local, dt).reshape(3, 4); p = np.asarray(p, dt)
    return p @ A[:, :3].T + A[:, 3]


# ---------------------------------------------------------------------------------------------------------------- slab test
def slab(o, d, lo, hi, dt=np.float64):
    """bbox.h ray_intersect for rays (n, 3): (hit, t_min, t_max, margin).  margin: the smallest relative gap of the two comparisons that decide
    `hit` (inf where a comparison involves a NaN or an infinity on both sides); a lane with a small margin is within rounding of a decision."""
    o, d, lo, hi = (np.asarray(v, dt) for v in (o, d, lo, hi))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rcp = dt(1.0) / d
        pos = rcp >= 0
        tmin = (np.where(pos, lo, hi) - o) * rcp
        tmax = (np.where(pos, hi, lo) - o) * rcp
        hit = (d != 0).any(-1)
        safe_max = lambda a, b: np.where((a > b) | ~np.isfinite(b), a, b)
        safe_min = lambda a, b: np.where((a < b) | ~np.isfinite(b), a, b)

        def gap(a, b):
            g = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), dt(1e-30))
            return np.where(np.isfinite(a) & np.isfinite(b), g, np.inf)
        hit = hit & ~((tmin[:, 0] > tmax[:, 1]) | (tmin[:, 1] > tmax[:, 0]))
        margin = np.minimum(gap(tmin[:, 0], tmax[:, 1]), gap(tmin[:, 1], tmax[:, 0]))
        t0 = safe_max(tmin[:, 0], tmin[:, 1]); t1 = safe_min(tmax[:, 0], tmax[:, 1])
        hit = hit & ~((t0 > tmax[:, 2]) | (tmin[:, 2] > t1))
        margin = np.minimum(margin, np.minimum(gap(t0, tmax[:, 2]), gap(tmin[:, 2], t1)))
        t0 = safe_max(t0, tmin[:, 2]); t1 = safe_min(t1, tmax[:, 2])
    return hit, t0, t1, margin


def on_face_with_zero_direction(o, d, lo, hi):
    """Lanes where a zero direction component meets an origin on that axis' box face: (face - o) * (1 / 0) = 0 * inf = NaN in the slab test"""
    o, d, lo, hi = (np.asarray(v, np.float64) for v in (o, d, lo, hi))
    return ((d == 0) & ((o == lo) | (o == hi))).any(-1)


# ------------------------------------------------------------------------------------------------------------------ sampling
def sample_heterogeneous(frame, grid, med_scale, albedo, o, d, maxt, u, dt=np.float64):
    """Medium::sample_interaction of a grid medium.  frame = (to_local 3 x 4, aabb_min, aabb_max); u: the float32 samples.  Returns a dict of
    arrays with the probe's fields plus `hit` (the slab test with its finiteness condition), `margin` (slab) and `t_margin`
    (|sampled_t - maxt| relative to sampled_t)."""
    to_local, lo, hi = frame
    o, d = np.asarray(o, dt).reshape(-1, 3), np.asarray(d, dt).reshape(-1, 3)
    maxt = np.asarray(maxt, dt).reshape(-1)
    one_minus = (np.float32(1.0) - np.asarray(u, np.float32).reshape(-1)).astype(dt)       # medium.cpp:71 forms 1 - sample in single
    hit, t0, t1, margin = slab(o, d, lo, hi, dt)
    hit = hit & (np.isfinite(t0) | np.isfinite(t1))
    t0 = np.where(hit, t0, dt(0.0)); t1 = np.where(hit, t1, dt(np.inf))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mint = np.maximum(dt(0.0), t0); end = np.minimum(maxt, t1)
        majorant = dt(med_scale) * dt(np.max(grid))
        sampled_t = mint + (-np.log(one_minus) / majorant)
        valid = hit & (sampled_t <= end)
        p = o + d * sampled_t[:, None]
        local = to_local_point(to_local, p, dt)
        finite = np.isfinite(local).all(-1)
        raw = np.where(finite, trilinear(grid, np.where(finite[:, None], local, 0.0).astype(dt), dt), np.nan)
        sigma_t = np.where(valid, dt(med_scale) * raw, dt(0.0))
        t_margin = np.abs(sampled_t - end) / np.maximum(np.abs(sampled_t), dt(1e-30))
    three = lambda a: np.repeat(np.asarray(a)[:, None], 3, 1)
    return {"valid": valid, "hit": hit, "t": np.where(valid, sampled_t, np.inf), "sampled_t": sampled_t, "p": p, "mint": mint,
            "sigma_t": three(sigma_t), "sigma_s": three(sigma_t) * np.asarray(albedo, dt), "sigma_n": three(majorant - sigma_t),
            "combined": np.full((len(o), 3), majorant), "local": local, "grid": raw, "margin": margin,
            "t_margin": np.where(np.isfinite(end), t_margin, np.inf)}


def sample_homogeneous(sigma_t_rgb, med_scale, albedo, o, d, maxt, u, channel, dt=np.float64):
    """Medium::sample_interaction of a homogeneous medium: the rate is channel `channel` of sigma_t * scale, no box."""
    o, d = np.asarray(o, dt).reshape(-1, 3), np.asarray(d, dt).reshape(-1, 3)
    maxt = np.asarray(maxt, dt).reshape(-1)
    one_minus = (np.float32(1.0) - np.asarray(u, np.float32).reshape(-1)).astype(dt)
    sig = np.asarray(sigma_t_rgb, dt) * dt(med_scale)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sampled_t = -np.log(one_minus) / sig[np.minimum(np.asarray(channel, np.int64), 2)]
        valid = sampled_t <= maxt
        p = o + d * sampled_t[:, None]
        t_margin = np.abs(sampled_t - maxt) / np.maximum(np.abs(sampled_t), dt(1e-30))
    st = np.where(valid[:, None], sig, dt(0.0))
    z = np.zeros((len(o), 3))
    return {"valid": valid, "hit": np.ones(len(o), bool), "t": np.where(valid, sampled_t, np.inf), "sampled_t": sampled_t, "p": p,
            "mint": np.zeros(len(o)), "sigma_t": st, "sigma_s": st * np.asarray(albedo, dt), "sigma_n": z, "combined": np.broadcast_to(sig, (len(o), 3)).copy(),
            "local": z, "grid": np.zeros(len(o)), "margin": np.full(len(o), np.inf), "t_margin": np.where(np.isfinite(maxt), t_margin, np.inf)}


# -------------------------------------------------------------------------------------------------------- density, optical depth
def density(frame, grid, p):
    """The density a ray meets at world points p (..., 3): 0 outside the volume's world AABB (free flights start at the slab entry and
    end at the slab exit, medium.cpp:53-60), else the clamped trilinear value at to_local(p).  Inside the AABB but outside the rotated unit
    cube the edge texels continue: that is the reference's behaviour (clamp wrap mode, grid.cpp), not a choice made here."""
    to_local, lo, hi = frame
    p = np.asarray(p, np.float64)
    inside = ((p >= lo) & (p <= hi)).all(-1)
    return np.where(inside, gg.trilinear(grid, to_local_point(to_local, p)), 0.0)


def optical_depth(frame, grid, o, d, t0, t1, n=256):
    """integral over [t0, t1] of density(o + t d) dt for rays (m, 3), midpoint rule with n steps on the part of [t0, t1] inside the AABB
    (the integral is split at the slab's entry and exit, so the jump there costs no accuracy; the integrand is piecewise polynomial)."""
    to_local, lo, hi = frame
    d = np.asarray(d, np.float64).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, np.float64), d.shape)
    hit, a, b, _ = slab(o, d, lo, hi)
    a = np.maximum(np.where(hit, a, np.inf), np.broadcast_to(np.asarray(t0, np.float64), a.shape))
    b = np.minimum(np.where(hit, b, -np.inf), np.broadcast_to(np.asarray(t1, np.float64), a.shape))
    length = np.where(b > a, b - a, 0.0)
    a = np.where(b > a, a, 0.0)
    out = np.zeros(len(d))
    for k in range(n):
        t = a + (k + 0.5) / n * length
        out += gg.trilinear(grid, to_local_point(to_local, o + d * t[:, None]))
    return out * length / n
