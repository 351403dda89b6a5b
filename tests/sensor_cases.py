"""Cases of the sensor / film pin: the sensors, filters and probe inputs, the scene with one rectangle emitter, and
its per-pixel closed form.  numpy and sensor_ref only; the scenes are dictionaries for mi.load_dict."""
import numpy as np

import sensor_ref as sr

PPO = (0.125, -0.0625)
# name: film (w, h), crop (w, h, x, y) or None, the sensor's fov keys, look_at, clip planes (None: the plugin's defaults 1e-2, 1e4), offset
SENSORS = {
    "a": dict(film=(12, 8), fov=dict(fov=40.0, fov_axis="x"), look=([0.3, -0.2, -4.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]), clip=(0.1, 100.0)),
    "b": dict(film=(9, 5), fov=dict(fov=35.0, fov_axis="y"), look=([2.0, -0.3, -4.0], [0.0, 0.1, 0.0], [0.0, 1.0, 0.0]), clip=(1.0, 5.0), ppo=PPO),
    "c": dict(film=(16, 10), crop=(5, 3, 2, 1), fov=dict(fov=50.0, fov_axis="x"), look=([2.0, 1.2, -3.1], [0.1, -0.2, 0.3], [0.1, 1.0, 0.2]),
              clip=(0.5, 6.0), ppo=PPO),
    "d": dict(film=(5, 9), fov=dict(focal_length="25mm", fov_axis="smaller"), look=([-1.0, 0.4, 3.0], [0.2, 0.0, 0.0], [0.0, 0.0, 1.0]), clip=(0.25, 50.0)),
    "e170": dict(film=(7, 4), fov=dict(fov=170.0, fov_axis="x"), look=([0.0, 0.5, -2.0], [0.3, 0.0, 1.0], [0.0, 1.0, 0.0]), clip=None),
    "e1": dict(film=(7, 4), fov=dict(fov=1.0, fov_axis="x"), look=([0.0, 0.5, -2.0], [0.3, 0.0, 1.0], [0.0, 1.0, 0.0]), clip=None),
}
FILTERS = {"box": (sr.BOX, 0.5), "tent1": (sr.TENT, 1.0), "tent2.5": (sr.TENT, 2.5), "gaussian0.5": (sr.GAUSSIAN, 0.5),
           "gaussian1": (sr.GAUSSIAN, 1.0), "gaussian2": (sr.GAUSSIAN, 2.0)}
WIDE = {"gaussian3": (sr.GAUSSIAN, 3.0)}            # beyond the probe's list: the oracle's film at 25 cells per side
RADIANCE = (1.0, 0.5, 0.25)


def sensor_spec(sensor):
    return SENSORS[sensor] if isinstance(sensor, str) else sensor


def filter_spec(rfilter):
    return FILTERS[rfilter] if rfilter in FILTERS else WIDE[rfilter]


def rfilter_dict(name):
    kind, param = filter_spec(name)
    return {"type": "box"} if kind == sr.BOX else {"type": "tent", "radius": param} if kind == sr.TENT else {"type": "gaussian", "stddev": param}


def expected_camera(name):
    """The sensor of a case as sensor_ref states it from the case's own parameters: parse_fov and look_at in float64, every value then
    rounded to float32 as the plugin stores it"""
    s = sensor_spec(name); w, h = s["film"]
    crop = s.get("crop") or (w, h, 0, 0)
    near, far = s["clip"] or (1e-2, 1e4)
    f32 = lambda v: float(np.float32(v))
    return sr.Camera(sr.look_at(*s["look"]).astype(np.float32), f32(sr.parse_fov(w / h, **s["fov"])), f32(near), f32(far), (w, h), crop[:2], crop[2:],
                     tuple(f32(v) for v in s.get("ppo", (0.0, 0.0))))


def rectangle_to_world(mi, sensor="b"):
    """The emitter of the closed-form scene, one placement per sensor that sees it, each running from in front of the sensor's near plane
    to beyond its far plane with its emitting side towards the sensor.  (b), and every probe scene: the [-1, 1]^2 rectangle stretched to
    8 x 1, turned 78 degrees about y and 12 about z.  (c): built in the sensor's own frame, along the line of sight through its crop
    window, RECT_C below."""
    if sensor != "c":
        return mi.ScalarTransform4f().translate([0.2, 0.0, 0.2]).rotate([0, 0, 1], 12.0).rotate([0, 1, 0], 78.0).scale([4.0, 0.5, 1.0])
    cam = expected_camera("c"); R, t = cam.to_world[:3, :3], cam.to_world[:3, 3]
    u = (cam.offset[0] + 0.5 * cam.crop[0]) / cam.film[0] + cam.ppo[0]; v = (cam.offset[1] + 0.5 * cam.crop[1]) / cam.film[1] + cam.ppo[1]
    th = np.tan(np.radians(cam.fov_x) / 2.0)
    los = np.array([(1 - 2 * u) * th, (1 - 2 * v) * th * cam.film[1] / cam.film[0], 1.0])           # the window centre's line of sight
    eu = los + np.array(RECT_C["skew"]); eu *= RECT_C["half_length"] / np.linalg.norm(eu)
    ev = np.cross(eu, np.array(RECT_C["across"])); ev *= RECT_C["half_width"] / np.linalg.norm(ev)
    axis = eu / eu[2]                                                                               # per unit of depth
    centre = RECT_C["cross"] * los + (RECT_C["depth"] - RECT_C["cross"]) * axis                    # the long axis meets the line of sight at depth `cross`
    n = np.cross(eu, ev)
    if centre @ n > 0:                                                                              # the camera, at 0, must be on the normal's side
        ev, n = -ev, -n
    m = np.eye(4); m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = R @ eu, R @ ev, R @ (n / np.linalg.norm(n)), t + R @ centre
    return mi.ScalarTransform4f(m)


RECT_C = dict(skew=(0.12, -0.03, 0.0), across=(0.0, 0.0, 1.0), half_length=3.6, half_width=0.2, depth=3.8, cross=0.7)


def scene_dict(mi, sensor, rfilter, integrator="path", fmt="rgba", spp=4):
    s = sensor_spec(sensor); w, h = s["film"]
    film = {"type": "hdrfilm", "width": w, "height": h, "pixel_format": fmt, "rfilter": rfilter_dict(rfilter)}
    if s.get("crop"):
        film.update(crop_width=s["crop"][0], crop_height=s["crop"][1], crop_offset_x=s["crop"][2], crop_offset_y=s["crop"][3])
    sensor_d = {"type": "perspective", **s["fov"], "to_world": mi.ScalarTransform4f().look_at(*s["look"]),
                "sampler": {"type": "independent", "sample_count": spp}, "film": film}
    if s["clip"]:
        sensor_d.update(near_clip=s["clip"][0], far_clip=s["clip"][1])
    if "ppo" in s:
        sensor_d.update(principal_point_offset_x=s["ppo"][0], principal_point_offset_y=s["ppo"][1])
    return {"type": "scene", "integrator": {"type": integrator, "max_depth": 2}, "sensor": sensor_d,
            "black": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.0, 0.0, 0.0]}},
            "light": {"type": "rectangle", "to_world": rectangle_to_world(mi, sensor if isinstance(sensor, str) else "b"), "bsdf": {"type": "ref", "id": "black"},
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": list(RADIANCE)}}}}


# ------------------------------------------------------------------------------------------------------- probe inputs
def ulp(x, k):
    """the float32 k ulps from x"""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def probe_inputs(sensor, rfilter, seed=0):
    """(n, 5) float32: position samples, film positions and filter arguments, cycled to the longest list"""
    rng = np.random.default_rng([seed, sorted(SENSORS).index(sensor), sorted(FILTERS).index(rfilter)])
    s = SENSORS[sensor]; w, h = s["film"]
    cw, ch, cx, cy = s.get("crop") or (w, h, 0, 0)
    g = np.linspace(0.0, 1.0, 9)
    pos = np.concatenate([np.stack(np.meshgrid(g, g), -1).reshape(-1, 2), rng.random((200, 2))])
    xs, ys = np.arange(cx, cx + cw + 1), np.arange(cy, cy + ch + 1)
    film = [np.stack(np.meshgrid(xs[:-1] + 0.5, ys[:-1] + 0.5), -1).reshape(-1, 2),                       # pixel centres
            np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2),                                                # pixel edges (the window's too)
            np.array([[ulp(x + 0.5, a), ulp(y + 0.5, b)] for x in (cx, cx + cw - 1) for y in (cy, cy + ch - 1) for a in (-1, 0, 1) for b in (-1, 0, 1)]),      # 1/2 +- 1 ulp
            np.array([[x + 0.3, y + 0.7] for x in (cx, cx + cw - 1) for y in ys[:-1]] + [[x + 0.7, y + 0.3] for y in (cy, cy + ch - 1) for x in xs[:-1]]),
            np.array([cx, cy]) + rng.random((200, 2)) * np.array([cw, ch])]
    film = np.concatenate(film)
    r = np.float32(sr.radius(*FILTERS[rfilter]))
    arg = np.concatenate([np.array([0.0, 0.2, -0.2, 0.49, 0.51, -0.49, -0.51, 1.0, -1.0, r, ulp(r, -1), ulp(r, 1), -r, -ulp(r, -1), -ulp(r, 1), 1.5 * r, -1.5 * r]),
                          (rng.random(200) * 2.4 - 1.2) * r])
    n = max(len(pos), len(film), len(arg))
    idx = np.arange(n)
    return np.concatenate([pos[idx % len(pos)], film[idx % len(film)], arg[idx % len(arg), None]], axis=1).astype(np.float32)


# -------------------------------------------------------------------------------------------------------- closed form
SUB = 192                               # midpoint samples per pixel and axis


def coverage(mi, sensor, rfilter, sub=SUB, clipped=False):
    """Per pixel of the crop window: (T_front, T_hit) = sum f hit front / sum f and sum f hit / sum f, f the filter at pixel centre minus
    sample position, over a sub x sub midpoint grid in every pixel of the crop window (where the render's samples fall).  hit: the ray of
    sensor_ref.sample_ray meets the rectangle within maxt, that is at a camera-space depth in [near, far]; front: on its emitting side.
    With clipped=True also the numbers of samples that meet the rectangle before the near plane and beyond the far plane."""
    c = expected_camera(sensor); kind, param = filter_spec(rfilter)
    (cw, ch), (cx, cy) = c.crop, c.offset
    sx = cx + (np.arange(cw * sub) + 0.5) / sub; sy = cy + (np.arange(ch * sub) + 0.5) / sub
    A = rectangle_to_world(mi, sensor).matrix
    p0, eu, ev = A[:3, 3], A[:3, 0], A[:3, 1]
    nrm = np.cross(eu, ev)
    hit = np.zeros((len(sy), len(sx)), bool); front = np.zeros_like(hit); n_near = n_far = 0
    ax = sr.film_to_sample(c, sx, 0.0)[0]
    for j, y in enumerate(sy):                                                                    # a row at a time
        o, d, maxt = sr.sample_ray(c, ax, np.full_like(ax, sr.film_to_sample(c, 0.0, y)[1]))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((p0 - o) @ nrm) / (d @ nrm)
        q = o + d * t[:, None] - p0
        u, v = q @ eu / (eu @ eu), q @ ev / (ev @ ev)
        inside = (np.abs(u) <= 1) & (np.abs(v) <= 1)
        hit[j] = (t > 0) & (t <= maxt) & inside
        front[j] = hit[j] & (d @ nrm < 0)
        n_near += int(np.sum(inside & (t <= 0))); n_far += int(np.sum(inside & (t > maxt)))
    # weights: pixel centre minus sample position, per axis
    wx = sr.rfilter(kind, param, (cx + np.arange(cw) + 0.5)[:, None] - sx[None, :])
    wy = sr.rfilter(kind, param, (cy + np.arange(ch) + 0.5)[:, None] - sy[None, :])
    den = wy.sum(1)[:, None] * wx.sum(1)[None, :]
    out = (wy @ front.astype(np.float64) @ wx.T) / den, (wy @ hit.astype(np.float64) @ wx.T) / den
    return out + (n_near, n_far) if clipped else out


def clip_polygon(poly, axis, bound, keep_above):
    """Sutherland-Hodgman against one plane: the part of the convex polygon poly (n, 3) with poly[:, axis] >= bound (or <=)"""
    out = []; sgn = 1.0 if keep_above else -1.0
    for a, b in zip(poly, np.roll(poly, -1, axis=0)):
        da, db = sgn * (a[axis] - bound), sgn * (b[axis] - bound)
        if da >= 0:
            out.append(a)
        if (da >= 0) != (db >= 0):
            out.append(a + (b - a) * (da / (da - db)))
    return np.array(out).reshape(-1, 3)


def image_polygon(mi, sensor):
    """The rectangle's visible part as a convex polygon in film pixels: the rectangle in the sensor's frame, cut at the camera-space depths
    near and far, projected by sensor_ref.geometric_direction's statement (u = (1 - x / (z tan)) / 2, v likewise with the aspect), and
    film position = (u - principal-point offset) * film size."""
    c = expected_camera(sensor); A = rectangle_to_world(mi, sensor).matrix
    p0, eu, ev = A[:3, 3], A[:3, 0], A[:3, 1]
    corners = np.array([p0 - eu - ev, p0 + eu - ev, p0 + eu + ev, p0 - eu + ev])
    cam = (corners - c.to_world[:3, 3]) @ np.linalg.inv(c.to_world[:3, :3]).T
    poly = clip_polygon(clip_polygon(cam, 2, c.near, True), 2, c.far, False)
    th = np.tan(np.radians(c.fov_x) / 2.0); aspect = c.film[0] / c.film[1]
    u = (1.0 - poly[:, 0] / (poly[:, 2] * th)) / 2.0; v = (1.0 - poly[:, 1] * aspect / (poly[:, 2] * th)) / 2.0
    return np.stack([(u - c.ppo[0]) * c.film[0], (v - c.ppo[1]) * c.film[1]], axis=-1)


ROWS = 2048                             # scanlines per pixel of coverage_exact


def coverage_exact(mi, sensor, rfilter, rows=ROWS):
    """sum f hit / sum f per pixel of the crop window with the filter integrated in closed form along x: on every scanline the polygon of
    image_polygon covers one interval [xl, xr], whose weight for the pixel column centred at cx is G(cx - xl) - G(cx - xr), G =
    sensor_ref.rfilter_integral; along y the midpoint rule over `rows` scanlines per pixel, whose integrand is continuous and piecewise
    smooth, so its error falls with rows^-2.  The denominator is the filter's integral over the crop window, in closed form on both axes."""
    c = expected_camera(sensor); kind, param = filter_spec(rfilter)
    (cw, ch), (cx, cy) = c.crop, c.offset
    poly = image_polygon(mi, sensor)
    y = cy + (np.arange(ch * rows) + 0.5) / rows
    xl = np.full(len(y), np.inf); xr = np.full(len(y), -np.inf)
    for a, b in zip(poly, np.roll(poly, -1, axis=0)):
        if a[1] == b[1]:
            continue
        s = (y - a[1]) / (b[1] - a[1]); on = (s >= 0) & (s <= 1)
        x = a[0] + s * (b[0] - a[0])
        xl = np.where(on, np.minimum(xl, x), xl); xr = np.where(on, np.maximum(xr, x), xr)
    xl, xr = np.clip(xl, cx, cx + cw), np.clip(xr, cx, cx + cw)
    xl, xr = np.where(xr > xl, xl, 0.0), np.where(xr > xl, xr, 0.0)                                # scanlines that miss: an empty interval
    pcx, pcy = cx + np.arange(cw) + 0.5, cy + np.arange(ch) + 0.5
    wx = sr.rfilter_integral(kind, param, pcx[None, :] - xl[:, None]) - sr.rfilter_integral(kind, param, pcx[None, :] - xr[:, None])     # (rows, cw)
    wy = sr.rfilter(kind, param, pcy[:, None] - y[None, :]) / rows                                                                           # (ch, rows)
    den_x = sr.rfilter_integral(kind, param, pcx - cx) - sr.rfilter_integral(kind, param, pcx - (cx + cw))
    den_y = sr.rfilter_integral(kind, param, pcy - cy) - sr.rfilter_integral(kind, param, pcy - (cy + ch))
    return (wy @ wx) / (den_y[:, None] * den_x[None, :])


def closed_form(mi, sensor, rfilter):
    """the developed rgba image: (crop_h, crop_w, 4).  Both sensors see the rectangle's emitting side wherever they see it
    (test_closed_form_reference_alone), so the colour is the radiance times the coverage."""
    t = coverage_exact(mi, sensor, rfilter)
    return np.concatenate([t[..., None] * np.array(RADIANCE), t[..., None]], axis=-1)


CLOSED_SENSORS, CLOSED_FILTERS, CLOSED_INTEGRATORS = ("b", "c"), ("box", "tent1", "gaussian0.5"), ("path", "volpath")
SEEDS = tuple(range(20, 28))
# The noise cap, from the reference alone: a pixel's estimate is Bernoulli, variance T (1 - T) / N with N = 8 seeds x spp and T <= 1/2 at
# worst, so the standard error of the 8-seed mean stays below SE_CAP (a share of the emitter's radiance) from spp >= 0.25 / (8 SE_CAP^2)
# = 3473 on; the tests take at least twice that.
SE_CAP, SPP = 0.003, 8192
assert SPP >= 2 * 0.25 / (8 * SE_CAP ** 2)
