"""The perspective sensor, the reconstruction filters, a sample's film footprint and the film's develop step, restated in numpy from the
reference's sources.  float64 unless a dtype is passed: every formula takes `dt`, so that the same text evaluated
in float32 measures its own rounding (the K table of test_sensor.py); nothing here reads the oracle or the device.

Sources: src/render/sensor.cpp:142-196 (parse_fov), include/mitsuba/render/sensor.h:234-269 (perspective_projection),
include/mitsuba/core/transform.h:393-410 (Transform::perspective) and :177-205 (look_at), src/sensors/perspective.cpp:200-236 (sample_ray),
src/rfilters/box.cpp:41-43, tent.cpp:48-55, gaussian.cpp:52-96, src/render/imageblock.cpp:438-456 (the footprint),
src/films/hdrfilm.cpp:401-402 (develop)."""
import numpy as np

BOX, GAUSSIAN, TENT = 0, 1, 2            # lrt_film_desc::rfilter


# ---------------------------------------------------------------------------------------------------------- parse_fov
def parse_fov(aspect, fov=None, fov_axis="x", focal_length=None):
    """sensor.cpp:142-196 in double: the horizontal field of view in degrees"""
    if fov is not None and focal_length is not None:
        raise ValueError("Please specify either a focal length ('focal_length') or a field of view ('fov')!")
    if fov is not None:                                                                      # :150-158
        fov = float(fov); axis = fov_axis.lower()
        if axis == "smaller":
            axis = "y" if aspect > 1 else "x"
        elif axis == "larger":
            axis = "x" if aspect > 1 else "y"
    else:                                                                                    # :159-175: the 36 x 24 mm diagonal
        f = "50mm" if focal_length is None else str(focal_length)
        value = float(f[:-2] if f.endswith("mm") else f)
        fov = 2.0 * np.degrees(np.arctan(np.sqrt(float(36 * 36 + 24 * 24)) / (2.0 * value))); axis = "diagonal"
    if axis == "x":                                                                          # :178-190
        result = fov
    elif axis == "y":
        result = np.degrees(2.0 * np.arctan(np.tan(0.5 * np.radians(fov)) * aspect))
    elif axis == "diagonal":
        diagonal = 2.0 * np.tan(0.5 * np.radians(fov))
        width = diagonal / np.sqrt(1.0 + 1.0 / (aspect * aspect))
        result = np.degrees(2.0 * np.arctan(width * 0.5))
    else:
        raise ValueError("The 'fov_axis' parameter must be set to one of 'smaller', 'larger', 'diagonal', 'x', or 'y'!")
    if result <= 0.0 or result >= 180.0:
        raise ValueError("The horizontal field of view must be in the range [0, 180]!")
    return float(result)


# ------------------------------------------------------------------------------------------------------------- camera
def look_at(origin, target, up):
    """Transform::look_at (transform.h:177-205): columns left, up, dir, origin"""
    o, t, u = (np.asarray(v, np.float64) for v in (origin, target, up))
    d = (t - o) / np.linalg.norm(t - o)
    left = np.cross(u, d); left /= np.linalg.norm(left)
    m = np.eye(4); m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, np.cross(d, left), d, o
    return m


class Camera:
    """What PerspectiveCamera holds: to_world (4 x 4), x_fov in degrees, the clip planes, the principal-point offset, the film's size, crop
    size and crop offset.  Values as the plugin stores them (float32 numbers held in float64)."""

    def __init__(self, to_world, fov_x, near, far, film, crop=None, offset=(0, 0), ppo=(0.0, 0.0)):
        self.to_world = np.asarray(to_world, np.float64).reshape(4, 4)
        self.fov_x, self.near, self.far = float(fov_x), float(near), float(far)
        self.film = tuple(int(v) for v in film); self.crop = self.film if crop is None else tuple(int(v) for v in crop)
        self.offset = tuple(int(v) for v in offset); self.ppo = (float(ppo[0]), float(ppo[1]))

    @classmethod
    def from_desc(cls, desc):
        """the inputs as a loaded description holds them"""
        S, F = desc.sensor, desc.film
        return cls(np.array(S.to_world[:], np.float64).reshape(4, 4), S.fov_x, S.near_clip, S.far_clip, (F.width, F.height),
                   (F.crop_width, F.crop_height), (F.crop_offset_x, F.crop_offset_y), (S.principal_point_offset_x, S.principal_point_offset_y))


def _scale(v, dt):
    return np.diag(np.array([v[0], v[1], v[2], 1], dt))


def _translate(v, dt):
    m = np.eye(4, dtype=dt); m[:3, 3] = v
    return m


def perspective(fov, near, far, dt=np.float64):
    """Transform::perspective, the forward matrix (transform.h:393-403)"""
    fov, near, far = dt(fov), dt(near), dt(far)
    recip = dt(1) / (far - near)
    cot = dt(1) / np.tan(np.radians(fov * dt(0.5)))
    m = np.diag(np.array([cot, cot, far * recip, 0], dt))
    m[2, 3] = -near * far * recip; m[3, 2] = 1
    return m


def perspective_projection(c, dt=np.float64):
    """sensor.h:234-269: the forward product of the five matrices, camera space -> crop-relative sample space"""
    fw, fh = dt(c.film[0]), dt(c.film[1])
    rsx, rsy = dt(c.crop[0]) / fw, dt(c.crop[1]) / fh
    rox, roy = dt(c.offset[0]) / fw, dt(c.offset[1]) / fh
    aspect = fw / fh
    return (_scale((dt(1) / rsx, dt(1) / rsy, 1), dt) @ _translate((-rox, -roy, 0), dt) @ _scale((dt(-0.5), dt(-0.5) * aspect, 1), dt)
            @ _translate((-1, dt(-1) / aspect, 0), dt) @ perspective(c.fov_x, c.near, c.far, dt))


def sample_to_camera(c, dt=np.float64):
    """perspective.cpp:175-177: the inverse, here by numpy.linalg.inv of the forward product (not by composed analytic inverses)"""
    return np.linalg.inv(perspective_projection(c, dt)).astype(dt)


def sample_ray(c, ax, ay, dt=np.float64):
    """perspective.cpp:200-236 at the adjusted position samples (ax, ay): origins (n, 3), directions (n, 3), maxt (n)"""
    ax, ay = np.asarray(ax, dt), np.asarray(ay, dt)
    ppx = dt(c.film[0]) * dt(c.ppo[0]) / dt(c.crop[0]); ppy = dt(c.film[1]) * dt(c.ppo[1]) / dt(c.crop[1])       # :214-215
    M = sample_to_camera(c, dt)
    p = np.stack([ax + ppx, ay + ppy, np.zeros_like(ax), np.ones_like(ax)], axis=-1)                                  # :218-221
    r = p @ M.T
    near_p = r[..., :3] / r[..., 3:4]
    d = near_p / np.sqrt(np.sum(near_p * near_p, axis=-1, keepdims=True))                                            # :224
    tw = c.to_world.astype(dt)
    dw = d @ tw[:3, :3].T                                                                                             # :227
    inv_z = dt(1) / d[..., 2]                                                                                         # :229
    near_t, far_t = dt(c.near) * inv_z, dt(c.far) * inv_z
    o = tw[:3, 3] + dw * near_t[..., None]                                                                            # :226,232
    return o, dw, far_t - near_t                                                                                      # :233


def geometric_direction(c, ax, ay):
    """The second statement: the film position (u, v) in [0, 1]^2 of the FULL film, u = (crop_offset + a * crop_size) / film_size + the
    principal-point offset, looks along ((1 - 2u) tan(fov/2), (1 - 2v) tan(fov/2) / aspect, 1) in camera space (x = left, y = up)."""
    ax, ay = np.asarray(ax, np.float64), np.asarray(ay, np.float64)
    u = (c.offset[0] + ax * c.crop[0]) / c.film[0] + c.ppo[0]
    v = (c.offset[1] + ay * c.crop[1]) / c.film[1] + c.ppo[1]
    th = np.tan(np.radians(c.fov_x) / 2.0); aspect = c.film[0] / c.film[1]
    d = np.stack([(1.0 - 2.0 * u) * th, (1.0 - 2.0 * v) * th / aspect, np.ones_like(u)], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d, d @ c.to_world[:3, :3].T


def film_to_sample(c, spx, spy, dt=np.float64):
    """integrator.cpp:462-466: scale = 1 / crop_size, offset = -crop_offset * scale, adjusted = fmadd(pos, scale, offset)"""
    sx, sy = dt(1) / dt(c.crop[0]), dt(1) / dt(c.crop[1])
    return np.asarray(spx, dt) * sx + (-dt(c.offset[0]) * sx), np.asarray(spy, dt) * sy + (-dt(c.offset[1]) * sy)


# ------------------------------------------------------------------------------------------------------------ filters
REMEZ = (9.992604880e-1, -4.977025247e-1, 1.222248550e-1, -1.932406282e-2, 2.136713061e-3, -1.679873860e-4, 9.202145248e-6,
         -3.329417433e-7, 7.128382794e-9, -6.821193280e-11)              # gaussian.cpp:69-73: the fit to exp(-x / 2) on [0, 16], minus its value at 16


def radius(kind, param):
    """box.cpp:37, gaussian.cpp:53 (4 stddev), tent.cpp:48; the float32 value the plugin stores"""
    return float(np.float32(0.5) if kind == BOX else np.float32(4) * np.float32(param) if kind == GAUSSIAN else np.float32(param))


def gaussian_coeffs(stddev, dt=np.float64, correct=True):
    """gaussian.cpp:77-85: coeff[i] * stddev^(-2 i), the scale kept in double, each product rounded to float32; then (:85) the value at
    radius^2 taken off coeff[0], evaluated in dt"""
    s = float(np.float32(stddev)); scale = 1.0; c = np.zeros(10, dt)
    for i in range(10):
        c[i] = np.float32(REMEZ[i] * scale); scale /= s * s
    if correct:
        r2 = dt(radius(GAUSSIAN, stddev)) ** 2
        acc = c[9]
        for i in range(8, -1, -1):
            acc = acc * r2 + c[i]
        c[0] -= acc
    return c


def gaussian_terms(x, stddev, dt=np.float64):
    """the polynomial's ten terms c_i x^(2 i) at x: (n, 10)"""
    x2 = np.square(np.asarray(x, dt))
    return gaussian_coeffs(stddev, dt) * x2[..., None] ** np.arange(10).astype(dt)


def rfilter(kind, param, x, dt=np.float64):
    """ReconstructionFilter::eval"""
    x = np.asarray(x, dt)
    if kind == BOX:                                                                          # box.cpp:42: half open
        return np.where((x >= dt(-0.5)) & (x < dt(0.5)), dt(1), dt(0))
    if kind == TENT:                                                                         # tent.cpp:49,54
        inv = dt(1) / dt(np.float32(param))
        return np.maximum(dt(0), dt(1) - np.abs(x * inv))
    c = gaussian_coeffs(param, dt); x2 = x * x                                        # gaussian.cpp:96 (Horner here, Estrin there)
    acc = np.full_like(x2, c[9])
    for i in range(8, -1, -1):
        acc = acc * x2 + c[i]
    return np.maximum(acc, dt(0))


def rfilter_integral(kind, param, t):
    """the antiderivative of ReconstructionFilter::eval from minus infinity to t, float64, in closed form (the Gaussian's polynomial is
    positive inside its radius, test_filter_integrals, so the clamp at zero acts only outside)"""
    t = np.asarray(t, np.float64); r = radius(kind, param)
    s = np.clip(t, -r, r)
    if kind == BOX:
        return s + 0.5
    if kind == TENT:
        return np.where(s <= 0, (s + r) ** 2 / (2 * r), r / 2 + s - s * s / (2 * r))
    c = gaussian_coeffs(param) / (2.0 * np.arange(10) + 1.0)
    P = lambda v: np.sum(c * v[..., None] ** (2 * np.arange(10) + 1), axis=-1)
    return P(s) - P(np.full_like(s, -r))


def gaussian_ideal(x, stddev):
    """what the polynomial fits: exp(-x^2 / 2 stddev^2) - exp(-8), zero outside the radius"""
    x = np.asarray(x, np.float64); s = float(np.float32(stddev))
    return np.where(np.abs(x) <= 4.0 * s, np.exp(-x * x / (2.0 * s * s)) - np.exp(-8.0), 0.0)


# ---------------------------------------------------------------------------------------------------------- footprint
def footprint(kind, param, spx, spy, dt=np.float64):
    """imageblock.cpp:438-456 for samples at the film positions (spx, spy): n, count, origin (n, 2) int, rel (n, 2).  The filter is
    evaluated at rel + k for cell k = 0 .. count - 1 of each axis."""
    n = int(np.ceil(np.float32(radius(kind, param)) - np.float32(0.5)))                     # :439 (float32 as stored)
    pos = np.stack([np.asarray(spx, dt), np.asarray(spy, dt)], axis=-1)
    pos_i = np.floor(pos).astype(np.int64) - n                                               # :445
    rel = pos_i.astype(dt) + dt(0.5) - pos                                                   # :456
    return n, 2 * n + 1, pos_i, rel


def footprint_weights(kind, param, spx, spy):
    """the separable weights of every cell: wx, wy (n, count)"""
    _, count, _, rel = footprint(kind, param, spx, spy)
    k = np.arange(count, dtype=np.float64)
    return rfilter(kind, param, rel[:, 0:1] + k), rfilter(kind, param, rel[:, 1:2] + k)


def accumulate(kind, param, crop, offset, spx, spy, rec, wx=None, wy=None):
    """ImageBlock::put of records rec (n, C) at (spx, spy) into the crop window's film, float64: (crop_h, crop_w, C).  wx, wy: other
    per-cell factors in place of the filter's weights (n, count), for error bounds."""
    _, count, org, _ = footprint(kind, param, spx, spy)
    fx, fy = footprint_weights(kind, param, spx, spy)
    wx, wy = fx if wx is None else wx, fy if wy is None else wy
    film = np.zeros((crop[1], crop[0], rec.shape[1]))
    for ys in range(count):
        for xs in range(count):
            x, y = org[:, 0] + xs - offset[0], org[:, 1] + ys - offset[1]
            ok = (x >= 0) & (x < crop[0]) & (y >= 0) & (y < crop[1])
            np.add.at(film, (y[ok], x[ok]), rec[ok].astype(np.float64) * (wy[ok, ys] * wx[ok, xs])[:, None])
    return film


# ------------------------------------------------------------------------------------------------------------ develop
def develop(film):
    """hdrfilm.cpp:401-402 in float32: values / select(weight == 0, 1, weight); film (..., C) with the weight last"""
    film = np.asarray(film, np.float32)
    w = film[..., -1:]
    with np.errstate(all="ignore"):
        return film[..., :-1] / np.where(w == 0, np.float32(1), w)
