"""The scenes, probes and checks that tests/test_surface.py (oracle, CPU) and tests/test_surface_gpu.py (device) share (DESIGN.md
section 13).  A "prober" is a callable (o, d, sample, wo_query) -> the dict of arrays that Scene.bsdf_probe and OrcScene.bsdf_probe
return; every check takes one, builds its rays itself and compares what comes back with tests/surface_ref.py in float64.

Tolerances are K * 2^-23 * cond: cond is computed by the reference in float64 from the geometry of each probe, K per check is at
least twice the worst ratio measured on the oracle (K below; the measurements are in DESIGN.md 13.4).  The device is held to the
oracle bit for bit (check e), so it needs no measurement of its own."""
import json
import os

import numpy as np

import surface_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = os.path.join(ROOT, "tests", "golden", "bsdf_known_answers.json")
EPS = sr.EPS

#: check -> K (DESIGN.md 13.4 lists the measured worst ratio beside each)
K = {"geom": 64, "b.wo": 8, "b.pdf": 32, "b.eta": 4, "b.weight": 4, "b.reverse": 8, "c.wo": 4, "c.pdf": 4, "c.weight": 4, "c.eval": 4,
     "d.normal_pdf": 4, "d.normal_mirror": 4, "d.ramp": 4, "d.eval": 4, "d.pdf": 32, "d.wo": 64, "d.weight": 4}
EDGE_CHECKER = 1e-4             # probes this close (in texture units) to a checkerboard cell edge are left out ...
EDGE_TEXEL = 1e-3               # ... and probes this close (in texels) to a line through texel centres, where the bump gradient jumps
EDGE_SIDE = 1e-5                # ... and probes whose side tests (which side of the perturbed surface) are this close to zero
CAP = 0.01                      # at most this share of a batch may be left out

ETAS = {"default": (1.5046, 1.000277), "1.5": (1.5, 1.0), "1/1.5": (1.0, 1.5), "diamond": (2.419, 1.0), "1.0003": (1.0003, 1.0), "one": (1.0, 1.0)}


def eta_of(name):
    """int_ior / ext_ior as the float32 quotient of the two float32 values a scene file states"""
    i, e = ETAS[name]
    return float(np.float32(i) / np.float32(e))


# ------------------------------------------------------------------------------------------------------------------ surfaces
def xform(ops):
    """the 4 x 4 matrix of a <transform>: each operation is multiplied from the left.  ops: ("scale", x, y, z) | ("rotate", axis, degrees)
    | ("translate", x, y, z)"""
    M = np.eye(4)
    for op in ops:
        T = np.eye(4)
        if op[0] == "scale": T[0, 0], T[1, 1], T[2, 2] = op[1:]
        elif op[0] == "translate": T[:3, 3] = op[1:]
        else:
            a = sr.unit(op[1]); t = np.radians(op[2])
            Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            T[:3, :3] = np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)                      # Rodrigues
        M = T @ M
    return M


def xform_xml(ops, name="to_world"):
    out = []
    for op in ops:
        if op[0] == "rotate": out.append(f'<rotate x="{op[1][0]!r}" y="{op[1][1]!r}" z="{op[1][2]!r}" angle="{op[2]!r}"/>')
        else: out.append(f'<{op[0]} x="{op[1]!r}" y="{op[2]!r}" z="{op[3]!r}"/>')
    return f'<transform name="{name}">' + "".join(out) + "</transform>"


class Plane:
    """a parallelogram p = P0 + a ea + b eb, (a, b) in [0, 1]^2, with texture coordinates uv = A (a, b) + c"""
    kind = "plane"

    def __init__(self, P0, ea, eb, A=None, c=None):
        self.P0, self.ea, self.eb = (np.asarray(v, np.float64) for v in (P0, ea, eb))
        self.A = np.eye(2) if A is None else np.asarray(A, np.float64); self.c = np.zeros(2) if c is None else np.asarray(c, np.float64)
        self.n = sr.unit(np.cross(self.ea, self.eb))
        J = np.stack([self.ea, self.eb], 1) @ np.linalg.inv(self.A)                                   # dp / d(u, v)
        self.dp_du, self.dp_dv = J[:, 0], J[:, 1]

    def point(self, ab):
        return self.P0 + ab[:, :1] * self.ea + ab[:, 1:] * self.eb

    def sample_points(self, rng, n):
        ab = rng.uniform(0.03, 0.97, (n, 2))
        return self.point(ab), np.broadcast_to(self.n, (n, 3))

    def hit(self, o, d):
        t = sr.dot(self.P0 - o, self.n) / sr.dot(d, self.n)
        p = o + t[:, None] * d
        ab = np.linalg.lstsq(np.stack([self.ea, self.eb], 1), (p - self.P0).T, rcond=None)[0].T
        z = np.zeros_like(p)
        return {"t": t, "p": p, "n": self.n + z, "uv": ab @ self.A.T + self.c, "dp_du": self.dp_du + z, "dp_dv": self.dp_dv + z,
                "valid": (t > 0) & (ab > 0).all(1) & (ab < 1).all(1)}


def rectangle(M):
    """the rectangle shape under to_world M: (x, y) in [-1, 1]^2 at z = 0, uv = ((x + 1) / 2, (y + 1) / 2)"""
    return Plane(M[:3, :3] @ [-1, -1, 0] + M[:3, 3], 2 * M[:3, 0], 2 * M[:3, 1])


class Sphere:
    """centre c, radius r, axes along the world's: p = c + r (sin th cos ph, sin th sin ph, cos th), uv = (ph / 2 pi, th / pi)"""
    kind = "sphere"

    def __init__(self, c, r):
        self.c = np.asarray(c, np.float64); self.r = float(r)

    def sample_points(self, rng, n, pole=np.radians(8)):
        th = np.arccos(rng.uniform(np.cos(np.pi - pole), np.cos(pole), n)); ph = rng.uniform(0, 2 * np.pi, n)
        nn = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
        return self.c + self.r * nn, nn

    def hit(self, o, d):
        oc = o - self.c; a = sr.dot(d, d); b = sr.dot(oc, d); disc = b * b - a * (sr.dot(oc, oc) - self.r ** 2)
        sq = np.sqrt(np.maximum(disc, 0)); t0, t1 = (-b - sq) / a, (-b + sq) / a
        t = np.where(t0 > 1e-9, t0, t1)
        p = o + t[:, None] * d; n = (p - self.c) / self.r
        th = np.arccos(np.clip(n[:, 2], -1, 1)); ph = np.mod(np.arctan2(n[:, 1], n[:, 0]), 2 * np.pi)
        st, ct = np.sin(th), np.cos(th)
        dp_du = 2 * np.pi * self.r * np.stack([-st * np.sin(ph), st * np.cos(ph), 0 * ph], 1)
        dp_dv = np.pi * self.r * np.stack([ct * np.cos(ph), ct * np.sin(ph), -st], 1)
        return {"t": t, "p": p, "n": n, "uv": np.stack([ph / (2 * np.pi), th / np.pi], 1), "dp_du": dp_du, "dp_dv": dp_dv,
                "valid": (disc > 0) & (t > 0), "pole": np.degrees(np.minimum(th, np.pi - th))}


class Cube:
    """the cube shape [-1, 1]^3 under to_world M (no texture coordinates are compared on it)"""
    kind = "cube"

    def __init__(self, M):
        self.M = M; self.Mi = np.linalg.inv(M)

    def sample_points(self, rng, n):
        ax = rng.integers(0, 3, n); sg = rng.choice([-1.0, 1.0], n)
        q = rng.uniform(-0.85, 0.85, (n, 3)); q[np.arange(n), ax] = sg
        nl = np.zeros((n, 3)); nl[np.arange(n), ax] = sg
        return q @ self.M[:3, :3].T + self.M[:3, 3], sr.unit(nl @ self.Mi[:3, :3])

    def hit(self, o, d):
        ol = o @ self.Mi[:3, :3].T + self.Mi[:3, 3]; dl = d @ self.Mi[:3, :3].T
        with np.errstate(divide="ignore"):
            ta, tb = (-1 - ol) / dl, (1 - ol) / dl
        tn, tf = np.minimum(ta, tb), np.maximum(ta, tb)
        t_in, t_out = tn.max(1), tf.min(1)
        inside = t_in < 1e-9
        t = np.where(inside, t_out, t_in)
        ax = np.where(inside, tf.argmin(1), tn.argmax(1))
        pl = ol + t[:, None] * dl
        nl = np.zeros_like(pl); nl[np.arange(len(t)), ax] = np.sign(pl[np.arange(len(t)), ax])
        p = o + t[:, None] * d
        return {"t": t, "p": p, "n": sr.unit(nl @ self.Mi[:3, :3]), "uv": None, "valid": (t_in <= t_out) & (t > 0)}


def local_frame(n, dp_du):
    """the shading frame of a surface without interpolated normals: s along dp_du (made perpendicular to n), t = n x s"""
    s = sr.unit(dp_du - n * sr.dot(n, dp_du)[:, None])
    return s, np.cross(n, s)


def aim(points, normals, theta, phi, side, dist):
    """float32 rays that arrive at `points` at angle theta off the normal (azimuth phi about it), from the front (side = 1) or the
    back (-1) of the surface, starting dist before the point"""
    n = np.asarray(normals, np.float64)
    a = np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])
    s = sr.unit(np.cross(a, n)); t = np.cross(n, s)
    d = -(np.sin(theta) * np.cos(phi))[:, None] * s - (np.sin(theta) * np.sin(phi))[:, None] * t - (side * np.cos(theta))[:, None] * n
    o = points - np.asarray(dist, np.float64).reshape(-1, 1) * d
    return o.astype(np.float32), d.astype(np.float32)


def start_distance(surf, inside, cos):
    """how far before its target a probe ray starts: 3 in free space; inside a closed body a stretch that stays inside it"""
    if surf.kind == "sphere": return np.where(inside, 0.8 * surf.r * np.abs(cos), 3.0)
    if surf.kind == "cube": return np.where(inside, 0.05, 3.0)
    return np.full(len(cos), 3.0)


def f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


# -------------------------------------------------------------------------------------------------------------------- scenes
MAPS = {"ramp_u": (8, 5), "ramp_v": (4, 3), "field": (8, 5), "rgb": (4, 3)}


def map_bytes(name):
    """the 8-bit samples of a height map, (h, w) or (h, w, 3)"""
    w, h = MAPS[name]
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    if name == "ramp_u": return (20 + 30 * i).astype(np.uint8)
    if name == "ramp_v": return (40 + 80 * j).astype(np.uint8)
    rng = np.random.default_rng(w * 10 + h + (name == "rgb"))

    def field():
        f = sum(rng.uniform(0.3, 1) * np.sin(2 * np.pi * (rng.integers(1, 3) * i / w + rng.integers(0, 2) * j / h) + rng.uniform(0, 6.28)) for _ in range(3))
        return np.clip(np.round(128 + 38 * f), 0, 255).astype(np.uint8)
    return np.stack([field(), field(), field()], -1) if name == "rgb" else field()


def write_map(mi, tmp_path, name):
    """writes the map as an 8-bit sRGB PNG, reads the bytes back with the reference's own decoder and returns (path, height texels)"""
    path = os.path.join(str(tmp_path), name + ".png")
    b = map_bytes(name)
    mi.write_png(path, sr.srgb_to_linear(b / 255.0).astype(np.float32))
    back = sr.read_png8(path)
    assert back.shape[:2] == b.shape[:2] and (back[..., :b.shape[2] if b.ndim == 3 else 1].reshape(b.shape) == b).all(), name
    return path, sr.height_texels(back)


TO_UV = {"id": [], "scaled": [("scale", 1.3, 0.7, 1.0), ("translate", 0.11, 0.23, 0.0)], "affine": [("scale", 1.3, 0.7, 1.0), ("rotate", (0, 0, 1), 20.0), ("translate", 0.11, 0.23, 0.0)],
         "checker": [("scale", 3.2, 2.4, 1.0), ("rotate", (0, 0, 1), 25.0), ("translate", 0.13, 0.27, 0.0)]}


def to_uv_matrix(name):
    M = xform(TO_UV[name])
    return np.array([[M[0, 0], M[0, 1], M[0, 3]], [M[1, 0], M[1, 1], M[1, 3]]])


RHO = (0.2, 0.5, 0.8)
CHECK0, CHECK1 = (0.7, 0.3, 0.1), (0.05, 0.4, 0.9)


def bsdf_xml(spec):
    kind = spec[0]
    if kind == "dielectric":
        if spec[1] == "default": return '<bsdf type="dielectric"/>'
        i, e = ETAS[spec[1]]
        return f'<bsdf type="dielectric"><float name="int_ior" value="{i!r}"/><float name="ext_ior" value="{e!r}"/></bsdf>'
    if kind == "diffuse":
        return '<bsdf type="diffuse"><rgb name="reflectance" value="%r, %r, %r"/></bsdf>' % RHO
    if kind == "diffuse_default":
        return '<bsdf type="diffuse"/>'
    if kind == "checker":
        return ('<bsdf type="diffuse"><texture type="checkerboard" name="reflectance"><rgb name="color0" value="%r, %r, %r"/>'
                '<rgb name="color1" value="%r, %r, %r"/>' % (CHECK0 + CHECK1) + xform_xml(TO_UV["checker"], "to_uv") + "</texture></bsdf>")
    if kind == "checker_plain":                                       # no to_uv: (s, t) = (u, v) without arithmetic
        return ('<bsdf type="diffuse"><texture type="checkerboard" name="reflectance"><rgb name="color0" value="%r, %r, %r"/>'
                '<rgb name="color1" value="%r, %r, %r"/></texture></bsdf>' % (CHECK0 + CHECK1))
    if kind == "bump":                                                # ("bump", png path, scale, to_uv name, nested spec)
        return (f'<bsdf type="bumpmap"><float name="scale" value="{spec[2]!r}"/><texture type="bitmap" name="texture"><string name="filename" value="{spec[1]}"/>'
                + xform_xml(TO_UV[spec[3]], "to_uv") + "</texture>" + bsdf_xml(spec[4]) + "</bsdf>")
    raise ValueError(kind)


RECT_OPS = [("scale", 1.5, 0.75, 1.0), ("rotate", (1.0, 0.0, 0.0), 30.0), ("rotate", (0.0, 0.0, 1.0), 40.0), ("translate", 0.2, -0.1, 0.3)]
CUBE_OPS = [("scale", 0.8, 1.1, 0.6), ("rotate", (0.0, 1.0, 0.0), 25.0), ("rotate", (1.0, 0.0, 0.0), -35.0), ("translate", 0.1, 0.2, -0.3)]
QUAD = dict(P0=(-1.2, -0.8, 0.1), ea=(2.2, 0.3, 0.5), eb=(-0.2, 1.7, 0.4), A=((0.9, 0.35), (0.2, -0.8)), c=(0.05, 0.9))      # det A < 0: uv mirrored and sheared
SPACING = 10.0


def shape_xml(kind, k, bsdf, tmp_path):
    """item k of a scene, moved SPACING * k along x: (xml, float64 surface)"""
    off = np.array([SPACING * k, 0, 0])
    move = [("translate", float(off[0]), 0.0, 0.0)]
    if kind == "rectangle":
        return f'<shape type="rectangle">{xform_xml(RECT_OPS + move)}{bsdf}</shape>', rectangle(xform(RECT_OPS + move))
    if kind == "rectangle_plain":                                     # to_world = identity (+ the move): local frame = world axes
        return f'<shape type="rectangle">{xform_xml(move)}{bsdf}</shape>', rectangle(xform(move))
    if kind == "cube":
        return f'<shape type="cube">{xform_xml(CUBE_OPS + move)}{bsdf}</shape>', Cube(xform(CUBE_OPS + move))
    if kind == "sphere":
        c = np.array([0.3, -0.2, 0.1]) + off
        c = [float(np.float32(x)) for x in c]
        return (f'<shape type="sphere"><point name="center" x="{c[0]!r}" y="{c[1]!r}" z="{c[2]!r}"/><float name="radius" value="1.25"/>{bsdf}</shape>',
                Sphere(f64(c), 1.25))
    if kind == "quad":
        q = Plane(np.array(QUAD["P0"]) + off, QUAD["ea"], QUAD["eb"], QUAD["A"], QUAD["c"])
        ab = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
        P = q.point(ab).astype(np.float32); T = (ab @ q.A.T + q.c).astype(np.float32)
        path = os.path.join(str(tmp_path), f"quad{k}.obj")
        with open(path, "w") as f:
            for p in P: f.write("v %.9g %.9g %.9g\n" % tuple(p))
            for t in T: f.write("vt %.9g %.9g\n" % (t[0], 1.0 - float(t[1])))          # (OBJ files keep v upside down: the loader flips it back)
            f.write("f 1/1 2/2 3/3\nf 1/1 3/3 4/4\n")
        P, T = P.astype(np.float64), T.astype(np.float64)
        T[:, 1] = 1.0 - f64(1.0 - T[:, 1])                                              # what the loader ends up with
        A = np.stack([T[1] - T[0], T[3] - T[0]], 1)
        return f'<shape type="obj"><string name="filename" value="{path}"/>{bsdf}</shape>', Plane(P[0], P[1] - P[0], P[3] - P[0], A, T[0])
    raise ValueError(kind)


def build(mi, tmp_path, items):
    """items: [(shape kind, bsdf spec)] -> (scene, [surface])"""
    parts, surfaces = [], []
    for k, (kind, spec) in enumerate(items):
        x, s = shape_xml(kind, k, bsdf_xml(spec), tmp_path)
        parts.append(x); surfaces.append(s)
    xml = f"""<scene version="3.0.0"><integrator type="path"/>
      <sensor type="perspective"><transform name="to_world"><lookat origin="0, 0, 50" target="0, 0, 0" up="0, 1, 0"/></transform>
        <sampler type="independent"><integer name="sample_count" value="1"/></sampler>
        <film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="6"/><rfilter type="box"/></film></sensor>
      {''.join(parts)}<emitter type="constant"><rgb name="radiance" value="1"/></emitter></scene>"""
    return mi.load_string(xml), surfaces


# -------------------------------------------------------------------------------------------------------------------- probing
class Prober:
    """Runs probes on `primary` (Scene.bsdf_probe or OrcScene.bsdf_probe).  With a `twin` (check e: the device beside the oracle),
    every batch is run on both and every float of it compared bit for bit."""

    def __init__(self, primary, twin=None):
        self.primary, self.twin, self.n_rays, self.n_compared = primary, twin, 0, 0

    def __call__(self, o, d, smp, woq, twin=True):
        pr = self.primary(o, d, smp, woq)
        assert np.isfinite(pr["raw"]).all()
        self.n_rays += len(pr["t"])
        if self.twin is not None and twin:
            tw = self.twin(o, d, smp, woq)
            same = (pr["raw"].view(np.uint32) == tw["raw"].view(np.uint32))
            bad = np.argwhere(~same)
            assert same.all(), (f"device and oracle differ in {len(bad)} of {same.size} floats; first at probe {bad[0][0]} float {bad[0][1]}: "
                                f"{pr['raw'][tuple(bad[0])]!r} against {tw['raw'][tuple(bad[0])]!r}")
            self.n_compared += same.size
        return pr


def ratio(got, want, cond, relative=True):
    """|got - want| / (2^-23 cond max(1, |want|)), the worst component of each row"""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    e = np.abs(got - want) / (np.maximum(1, np.abs(want)) if relative else 1)
    if e.ndim == 2: e = e.max(1)
    return e / (EPS * np.asarray(cond, np.float64))


class Report:
    """collects the worst ratio of each named check and asserts it against K"""

    def __init__(self, label):
        self.label, self.worst = label, {}

    def hold(self, name, r, key=None, where=None):
        r = np.asarray(r, np.float64)
        if where is not None: r = r[where]
        assert np.isfinite(r).all(), (self.label, name)
        w = float(r.max()) if r.size else 0.0
        self.worst[name] = max(self.worst.get(name, 0.0), w)
        k = K[key or name]
        print(f"[surface] {self.label}: {name}: n={r.size} worst error / (2^-23 cond) = {w:.3f} (K = {k})")
        assert w <= k, (self.label, name, w, k, int(np.argmax(r)) if r.size else -1)


def normal_cond(surf, cos_i):
    """A flat surface has one normal wherever the ray lands.  On a sphere the normal is (p - c) / r, and p = o + t d carries the error of
    t, 2^-24 r / cos(theta_i) along a ray that is almost tangent there: the normal, and everything formed with it, inherits 1 + 1 / cos(theta_i)."""
    return 1 + 1 / cos_i if surf.kind == "sphere" else np.ones_like(cos_i)


def side_edge(surf, cos_i):
    """How close to zero a side test (wo.n, wo.n', their product) may be before float32 and float64 can disagree about its sign: EDGE_SIDE
    on flat surfaces.  On a sphere the normal itself is turned by up to 2 * 2^-23 * (1 / cos(theta_i)) (twice the largest measured ratio of
    geom.n, 0.81); the perturbed normal turns with it, a mirrored wo by twice that, so each of the two cosines moves by at most three such
    angles and their product by at most six: 12 * 2^-23 / cos(theta_i) more."""
    return EDGE_SIDE + 12 * EPS * (normal_cond(surf, cos_i) - 1)


def check_geometry(rep, surf, pr, o, d, item):
    """a6-a7: hit distance, position, normals, uv and the local wi of the surface interaction against the float64 surface"""
    o, d = f64(o), f64(d)
    g = surf.hit(o, d)
    assert g["valid"].all() and (pr["shape"] == item).all(), (rep.label, g["valid"].mean(), np.unique(pr["shape"]))
    du = sr.unit(d)
    cos_i = np.abs(sr.dot(du, g["n"]))
    cond = 1 + 1 / cos_i                                              # t = (P0 - o).n / d.n: the denominator's rounding over its size
    g["ncond"] = normal_cond(surf, cos_i)
    rep.hold("geom.t", ratio(pr["t"], g["t"], cond), "geom")
    rep.hold("geom.p", ratio(pr["p"] - o, g["p"] - o, cond), "geom")
    rep.hold("geom.n", ratio(pr["n"], g["n"], g["ncond"]), "geom")
    rep.hold("geom.sh_n", ratio(pr["sh_n"], g["n"], g["ncond"]), "geom")
    rep.hold("geom.wi_z", ratio(pr["wi"][:, 2], -sr.dot(du, g["n"]), g["ncond"]), "geom")
    if g["uv"] is not None:
        span = np.linalg.norm(g["dp_du"], axis=1) ** -1 + np.linalg.norm(g["dp_dv"], axis=1) ** -1          # uv per unit of p
        rep.hold("geom.uv", ratio(pr["uv"], g["uv"], cond * (1 + span * np.abs(g["p"] - o).max(1)), relative=False), "geom")
        s, t = local_frame(g["n"], g["dp_du"])
        rep.hold("geom.wi_xy", ratio(pr["wi"][:, :2], np.stack([-sr.dot(du, s), -sr.dot(du, t)], 1), g["ncond"]), "geom")
    g["d"] = du
    return g


# ------------------------------------------------------------------------------------------------------- b: dielectric sweep
def sweep_rays(surf, eta, rng):
    """incidence 0 .. 89.9 degrees in 37 steps, the neighbourhood of the critical angle, three azimuths, both sides, both lobes"""
    th = np.radians(np.concatenate([np.linspace(0, 89.9, 37), [1e-3, 0.05, 89.0, 89.5]]))
    ratio_ = max(eta, 1 / eta)
    if ratio_ > 1.0000001:
        crit = np.arcsin(1 / ratio_)
        th = np.concatenate([th, crit + np.array([-1e-2, -1e-3, -1e-4, 1e-4, 1e-3, 1e-2])])
    th = th[(th >= 0) & (th < np.radians(89.95))]
    T, PH, SD, S1 = (x.reshape(-1) for x in np.meshgrid(th, np.radians([10.0, 130.0, 250.0]), [1.0, -1.0], [0.0, 1.0], indexing="ij"))
    p, n = surf.sample_points(rng, len(T))
    o, d = aim(p, n, T, PH, SD, start_distance(surf, SD < 0, np.cos(T)))
    return o, d, S1.astype(np.float32)


def check_dielectric(prober, surf, item, eta, label, seed=1):
    rng = np.random.default_rng(seed)
    rep = Report(label)
    o, d, s1 = sweep_rays(surf, eta, rng)
    n = len(s1)
    smp = np.stack([s1, rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)], 1)
    woq = sr.unit(rng.normal(size=(n, 3))).astype(np.float32)
    pr = prober(o, d, smp, woq, twin=surf.kind != "sphere")
    g = check_geometry(rep, surf, pr, o, d, item)
    want = sr.dielectric_sample(g["d"], g["n"], eta, s1 == 0)
    nc = g["ncond"]
    cond = np.where(want["tir"], 1.0, want["cond"]) * nc
    refl = want["reflected"]
    # which lobe: s1 = 0 reflects (0 <= R), s1 = 1 refracts unless R = 1
    got_refl = pr["eta"] == 1.0 if eta != 1.0 else np.sign(pr["wo_z"]) == np.sign(pr["wi"][:, 2])
    near_crit = (~want["tir"]) & (want["cos_t"] < 1e-3)                    # (float32 may already see total reflection here: compared only where it chose the same lobe)
    assert (got_refl == refl)[~near_crit].all(), (label, np.argwhere(got_refl != refl)[:5])
    both = got_refl == refl
    rep.hold("b.wo", ratio(pr["wo"], want["wo"], np.where(refl, nc, cond)), where=both)
    rep.hold("b.wo_z", ratio(pr["wo_z"], sr.dot(want["wo"], g["n"]), np.where(refl, nc, cond)), "b.wo", where=both)
    rep.hold("b.pdf", ratio(pr["pdf"], want["pdf"], cond), where=both)
    rep.hold("b.eta", ratio(pr["eta"], want["eta"], 1), where=both)
    rep.hold("b.weight", ratio(pr["weight"], want["weight"][:, None] + np.zeros(3), 1), where=both)
    assert (pr["type"] == sr.F_DELTA).all()
    assert (pr["eval"] == 0).all() and (pr["eval_pdf"] == 0).all(), "a delta BSDF evaluates to exactly 0"
    tir = want["tir"] & ~near_crit
    if eta != 1.0:
        assert tir.sum() >= 12, (label, tir.sum())
    assert (pr["pdf"][tir] == 1).all() and (pr["eta"][tir] == 1).all() and (pr["weight"][tir] == 1).all(), "total internal reflection: the mirror lobe with pdf 1"
    # the selection boundary: s1 = the returned float32 R reflects, the next float above it refracts
    sel = (s1 == 0) & ~want["tir"] & ~near_crit
    r_i = pr["pdf"][sel]
    for s_edge, want_refl in ((r_i, True), (np.nextafter(r_i, np.float32(2)), False)):
        e = smp[sel].copy(); e[:, 0] = s_edge
        pe = prober(o[sel], d[sel], e, woq[sel], twin=surf.kind != "sphere")
        is_refl = (pe["pdf"] == r_i)
        if eta == 1.0:
            is_refl = np.sign(pe["wo_z"]) == np.sign(pe["wi"][:, 2])
        assert (is_refl == want_refl).all(), (label, "s1 = R must reflect, the next float must refract", want_refl, float(is_refl.mean()))
        if not want_refl:
            assert (pe["pdf"] == np.float32(1) - r_i).all()
    # reversibility: the refracted ray sent back refracts into the first ray reversed, and the two radiance weights multiply to 1
    fw = (~refl) & both
    cwo = sr.dot(f64(pr["wo"][fw]), g["n"][fw])
    ob = (f64(pr["p"][fw]) + start_distance(surf, cwo < 0, cwo)[:, None] * f64(pr["wo"][fw])).astype(np.float32)
    db = (-f64(pr["wo"][fw])).astype(np.float32)
    sb = smp[fw].copy(); sb[:, 0] = 1
    pb = prober(ob, db, sb, woq[fw], twin=surf.kind != "sphere")
    back = pb["eta"] != 1.0 if eta != 1.0 else np.ones(fw.sum(), bool)
    cb = cond[fw] * (1 + 1 / np.maximum(np.abs(sr.dot(g["d"][fw], g["n"][fw])), 1e-3))
    assert back[want["cos_t"][fw] > 1e-2].all(), label
    rep.hold("b.reverse.wo", ratio(pb["wo"], -g["d"][fw], cb), "b.reverse", where=back)
    rep.hold("b.reverse.weights", ratio(pb["weight"][:, 0].astype(np.float64) * pr["weight"][fw][:, 0], 1.0, 1), "b.reverse", where=back)
    rep.hold("b.reverse.etas", ratio(pb["eta"].astype(np.float64) * pr["eta"][fw], 1.0, 1), "b.reverse", where=back)
    return rep.worst


# ------------------------------------------------------------------------------------------- c: diffuse and the checkerboard
def check_diffuse(prober, surf, item, label, checker, seed=2, n=1500):
    rng = np.random.default_rng(seed)
    rep = Report(label)
    p, nn = surf.sample_points(rng, n)
    side = np.where(rng.random(n) < 0.7, 1.0, -1.0)
    th = np.arccos(rng.uniform(0.02, 1, n)); th[:8] = np.radians(89.9)
    o, d = aim(p, nn, th, rng.uniform(0, 2 * np.pi, n), side, start_distance(surf, side < 0, np.cos(th)))
    smp = rng.random((n, 3), dtype=np.float32)
    smp[8:16, 1:] = [[0, 0], [0.5, 0.5], [1 - 2.0 ** -24, 0.5], [0.5, 0], [0.25, 0.75], [0.75, 0.25], [2.0 ** -24, 2.0 ** -24], [0.5, 1 - 2.0 ** -24]]
    wq = sr.unit(rng.normal(size=(n, 3)))
    woq = wq.astype(np.float32)
    pr = prober(o, d, smp, woq, twin=surf.kind != "sphere")
    g = check_geometry(rep, surf, pr, o, d, item)
    s, t = local_frame(g["n"], g["dp_du"])
    front = -sr.dot(g["d"], g["n"]) > 0
    assert (pr["wi"][:, 2] > 0).sum() == front.sum() and front.sum() > 0.5 * n and (~front).sum() > 0.1 * n
    if checker:
        rho, near = sr.checkerboard(g["uv"], to_uv_matrix("checker"), CHECK0, CHECK1, EDGE_CHECKER)
        assert near.mean() <= CAP, (label, near.mean())
        assert len(np.unique(rho[:, 0])) == 2
        print(f"[surface] {label}: {near.sum()} of {n} probes within {EDGE_CHECKER} of a cell edge left out ({near.mean():.4%}, cap {CAP:.0%})")
    else:
        rho, near = np.broadcast_to(f64(RHO), (n, 3)), np.zeros(n, bool)
    # the sample
    loc = sr.cosine_hemisphere(f64(smp[:, 1]), f64(smp[:, 2]))
    wo = loc[:, :1] * s + loc[:, 1:2] * t + loc[:, 2:] * g["n"]
    live = front & (loc[:, 2] > 0)
    cz = g["ncond"] * (1 + 1 / np.maximum(loc[:, 2], 1e-30))                              # z = sqrt(1 - x^2 - y^2): a small root of a difference
    rep.hold("c.wo", ratio(pr["wo"], wo, cz), where=live & (loc[:, 2] > 1e-3))
    rep.hold("c.pdf", ratio(pr["pdf"], loc[:, 2] / np.pi, cz), where=live & (loc[:, 2] > 1e-3))
    rep.hold("c.weight", ratio(pr["weight"], rho, 1), where=live & ~near & (pr["pdf"] > 0))
    assert (pr["type"][front] == sr.F_SMOOTH).all() and (pr["eta"][front] == 1).all()
    back = ~front
    assert (pr["pdf"][back] == 0).all() and (pr["weight"][back] == 0).all() and (pr["eval"][back] == 0).all() and (pr["eval_pdf"][back] == 0).all(), \
        "hit from behind: every value is exactly 0"
    # eval / pdf at the query direction
    wqu = sr.unit(f64(woq))
    val, pdf = sr.diffuse_eval(rho, -sr.dot(g["d"], g["n"]), sr.dot(wqu, g["n"]))
    below = sr.dot(wqu, g["n"]) <= 0
    knife = np.abs(sr.dot(wqu, g["n"])) < side_edge(surf, np.abs(sr.dot(g["d"], g["n"])))
    assert knife.mean() <= CAP
    assert below.sum() > 0.3 * n and (pr["eval"][below & ~knife] == 0).all() and (pr["eval_pdf"][below & ~knife] == 0).all(), "wo below the surface: exactly 0"
    rep.hold("c.eval", ratio(pr["eval"], val, g["ncond"]), where=~near & ~knife)
    rep.hold("c.eval_pdf", ratio(pr["eval_pdf"], pdf, g["ncond"]), "c.pdf", where=~knife)
    return rep.worst


def check_checker_on_the_edge(prober, item, label):
    """The cell edge itself, which the random probes leave out: an axis-aligned rectangle (`rectangle_plain`) with a checkerboard
    without to_uv, hit straight down on a grid of dyadic points, so that u or v comes out as exactly 0.5 in float32.  The reference
    takes the uv the probe reports (no arithmetic lies between it and the cell test): a fraction of exactly 0.5 belongs to the
    lower cell (the texture's test is `> 0.5`)."""
    k = np.arange(-7, 8) / 8.0
    x, y = (a.reshape(-1) for a in np.meshgrid(k, k))
    o = np.stack([x + SPACING * item, y, np.full(len(x), 2.0)], 1).astype(np.float32)
    d = np.tile(np.float32([[0, 0, -1]]), (len(x), 1))
    pr = prober(o, d, np.full((len(x), 3), 0.5, np.float32), np.tile(np.float32([[0, 0, 1]]), (len(x), 1)))
    uv = f64(pr["uv"])
    assert (pr["shape"] == item).all() and np.abs(uv - np.stack([(x + 1) / 2, (y + 1) / 2], 1)).max() < 1e-6
    on_edge = ((uv - np.floor(uv)) == 0.5).any(1)
    assert on_edge.sum() >= 20, (label, on_edge.sum())
    rho, _ = sr.checkerboard(uv, [[1, 0, 0], [0, 1, 0]], CHECK0, CHECK1)
    assert np.abs(f64(pr["weight"]) - f64(rho)).max() == 0, (label, "cell colours, the edges included", np.argwhere(f64(pr["weight"]) != f64(rho))[:4])
    print(f"[surface] {label}: {len(x)} probes, {on_edge.sum()} with u or v of exactly 0.5: colours as `> 0.5` decides")


# ---------------------------------------------------------------------------------------------------------------- d: bump map
def bump_amplification(surf_hit, hm, scale):
    """how far one rounding of a texel or of a lerp weight is stretched on its way into the tilt: scale * (slope per texel step)
    over the length of dp_du / dp_dv"""
    lu = np.linalg.norm(surf_hit["dp_du"], axis=1); lv = np.linalg.norm(surf_hit["dp_dv"], axis=1)
    reach = np.abs(hm.to_uv[:, :2]).sum() * max(hm.w, hm.h)
    return 1 + scale * reach * (1 / lu + 1 / lv) * (1 + np.abs(hm.t).max())


def bump_setup(surf, hm, scale, o, d):
    """the float64 side of a bump-map batch.  A map that is not square under a to_uv that mixes u and v is held to the reference
    renderer's own chain rule (surface_ref.HeightMap.gradient), every other one to the derivative of the interpolant: the two agree there."""
    g = surf.hit(f64(o), f64(d))
    g["d"] = sr.unit(f64(d))
    margin = hm.cell_margin(g["uv"])
    g["near"] = margin < EDGE_TEXEL
    quirk = hm.w != hm.h and (hm.to_uv[0, 1] != 0 or hm.to_uv[1, 0] != 0)
    hu, hv = hm.gradient(g["uv"], np.maximum(margin, 1e-9), renderer_chain_rule=quirk)
    ou, ov = hm.gradient(g["uv"], np.maximum(margin, 1e-9))
    g["chain_rule_gap"] = float(np.abs(np.stack([hu - ou, hv - ov])).max())
    assert quirk or g["chain_rule_gap"] < 1e-9
    wi = -g["d"]
    m0, _ = sr.bump_normal(g["n"], g["dp_du"], g["dp_dv"], scale, hu, hv, g["n"] * np.sign(sr.dot(wi, g["n"]))[:, None])    # before any mirroring
    g["m"], g["mirrored"] = sr.bump_normal(g["n"], g["dp_du"], g["dp_dv"], scale, hu, hv, wi)
    g["near"] |= np.abs(sr.dot(wi, m0)) < EDGE_SIDE
    g["amp"] = bump_amplification(g, hm, scale) * normal_cond(surf, np.abs(sr.dot(g["d"], g["n"])))
    g["hu"], g["hv"] = hu, hv
    return g


def bump_rays(surf, rng, n):
    p, nn = surf.sample_points(rng, n)
    side = np.where(rng.random(n) < 0.75, 1.0, -1.0) if surf.kind != "sphere" else np.ones(n)
    th = np.arccos(rng.uniform(0.0, 1, n)); th = np.minimum(th, np.radians(89.5))
    th[: n // 4] = np.radians(rng.uniform(70, 89.5, n // 4))                 # a quarter at grazing incidence: these meet normals that face away
    o, d = aim(p, nn, th, rng.uniform(0, 2 * np.pi, n), side, np.full(n, 3.0))
    return o, d


def check_bump_diffuse(prober, surf, item, hm, scale, label, seed=3, n=900, ramp=None):
    """nested diffuse: the perturbed normal solved from the probe's pdf at three directions (pdf = n'.wo / pi: linear in n'); eval
    and pdf at arbitrary wo with the shadow terminator; exact zeros"""
    rng = np.random.default_rng(seed)
    rep = Report(label)
    o, d = bump_rays(surf, rng, n)
    g = bump_setup(surf, hm, scale, o, d)
    assert g["valid"].all()
    if surf.kind == "sphere": assert (g["pole"] > 5).all()
    print(f"[surface] {label}: {g['near'].sum()} of {n} probes within {EDGE_TEXEL} texel of a texel-centre line (or on the mirror's edge) left out "
          f"({g['near'].mean():.4%}, cap {CAP:.0%}); {g['mirrored'].sum()} meet a normal that faces away and is mirrored")
    assert g["near"].mean() <= CAP
    front = -sr.dot(g["d"], g["n"]) > 0
    assert (g["mirrored"] & front).sum() >= 10, (label, "no grazing probe triggered the invalid-normal mirror")
    s, t = local_frame(g["n"], g["dp_du"])
    # three query directions around the true normal, on the viewer's side
    sg = np.sign(-sr.dot(g["d"], g["n"]))[:, None]
    W = [sr.unit(sg * g["n"] + 0.35 * s), sr.unit(sg * g["n"] + 0.35 * t), sr.unit(sg * g["n"] - 0.25 * (s + t))]
    smp = rng.random((n, 3), dtype=np.float32)
    prs = [prober(o, d, smp, w.astype(np.float32), twin=surf.kind != "sphere") for w in W]
    W = [sr.unit(f64(w.astype(np.float32))) for w in W]
    pdfs = np.stack([f64(p["eval_pdf"]) for p in prs], 1)
    usable = front & (pdfs > 0).all(1) & ~g["near"]
    assert usable.sum() > 0.5 * front.sum(), (label, usable.sum(), front.sum())
    Wm = np.stack(W, 1)                                                      # (n, 3, 3)
    solved = np.linalg.solve(Wm[usable], (np.pi * pdfs[usable])[:, :, None])[:, :, 0]
    cW = np.linalg.cond(Wm[usable])
    rep.hold("d.normal_pdf", ratio(solved, g["m"][usable], g["amp"][usable] * cW))
    assert np.abs(np.linalg.norm(solved, axis=1) - 1).max() < 1e-4
    if ramp is not None:
        # a ramp's cells each have one slope, so each cell is a plane tilted about the other tangent: tan(tilt) = scale * slope / |e|,
        # towards -e, with e the part of dp_du (dp_dv for the ramp along v) perpendicular to the other tangent (dp_du itself on a rectangle)
        axis, tex = ramp
        st = hm.st(g["uv"][usable])
        if axis == 0:
            i = np.floor(st[:, 0] * hm.w - 0.5).astype(int); slope = (tex[0, np.mod(i + 1, hm.w)] - tex[0, np.mod(i, hm.w)]) * hm.w * hm.to_uv[0, 0]
            e, other = g["dp_du"][usable], sr.unit(g["dp_dv"][usable])
        else:
            j = np.floor(st[:, 1] * hm.h - 0.5).astype(int); slope = (tex[np.mod(j + 1, hm.h), 0] - tex[np.mod(j, hm.h), 0]) * hm.h * hm.to_uv[1, 1]
            e, other = g["dp_dv"][usable], sr.unit(g["dp_du"][usable])
        e = e - other * sr.dot(e, other)[:, None]
        le = np.linalg.norm(e, axis=1)
        closed = sr.unit(g["n"][usable] - (scale * slope / le)[:, None] * (e / le[:, None]))
        flipped = g["mirrored"][usable]                                    # (a mirrored normal tilts the other way)
        closed = np.where(flipped[:, None], 2 * sr.dot(closed, g["n"][usable])[:, None] * g["n"][usable] - closed, closed)
        rep.hold("d.ramp", ratio(solved, closed, g["amp"][usable] * cW))
        tan_got = np.linalg.norm(np.cross(solved, g["n"][usable]), axis=1) / np.abs(sr.dot(solved, g["n"][usable]))
        assert np.unique(np.round(scale * np.abs(slope) / le, 9)).size >= 2        # (the wrap cell's slope is another one)
        rep.hold("d.ramp.tan", ratio(tan_got, scale * np.abs(slope) / le, g["amp"][usable] * cW * (1 + tan_got ** 2)), "d.ramp")
    # eval and pdf at arbitrary directions
    woq = sr.unit(rng.normal(size=(n, 3))).astype(np.float32)
    pr = prober(o, d, smp, woq, twin=surf.kind != "sphere")
    check_geometry(rep, surf, pr, o, d, item)
    wq = sr.unit(f64(woq))
    val, pdf, tcond = sr.bumped_diffuse_eval(f64(RHO), g["n"], g["m"], -g["d"], wq)
    edge = side_edge(surf, np.abs(sr.dot(g["d"], g["n"])))
    knife = (np.abs(sr.dot(wq, g["n"])) < edge) | (np.abs(sr.dot(wq, g["m"])) < edge) | g["near"]
    assert knife.mean() <= 2 * CAP
    zero = (pdf == 0) & ~knife
    assert zero.sum() > 0.3 * n and (pr["eval"][zero] == 0).all() and (pr["eval_pdf"][zero] == 0).all(), (label, "exact zeros")
    assert ((pr["eval_pdf"] > 0) == (pdf > 0))[~knife].all()
    rep.hold("d.eval", ratio(pr["eval"], val, g["amp"] * np.minimum(tcond, 1e6)), where=~knife)
    rep.hold("d.pdf", ratio(pr["eval_pdf"], pdf, g["amp"]), where=~knife)
    return rep.worst


def check_bump_dielectric(prober, surf, item, hm, scale, eta, label, seed=4, n=900):
    """nested dielectric: n' from the mirror sample (n' along wi + wo), refraction about n', the weight's terminator and its exact
    zero where the sampled direction leaves on the wrong side of the true surface"""
    rng = np.random.default_rng(seed)
    rep = Report(label)
    o, d = bump_rays(surf, rng, n)
    g = bump_setup(surf, hm, scale, o, d)
    assert g["valid"].all() and g["near"].mean() <= CAP
    woq = sr.unit(rng.normal(size=(n, 3))).astype(np.float32)
    out = {}
    for s1 in (0.0, 1.0):
        smp = rng.random((n, 3), dtype=np.float32); smp[:, 0] = s1
        pr = prober(o, d, smp, woq, twin=surf.kind != "sphere")
        assert (pr["eval"] == 0).all() and (pr["eval_pdf"] == 0).all() and (pr["type"] == sr.F_DELTA).all()
        want = sr.bumped_dielectric_sample(g["d"], g["n"], g["m"], eta, np.full(n, s1 == 0))
        cond = g["amp"] * np.where(want["tir"], 1.0, want["cond"])
        near_crit = (~want["tir"]) & (want["cos_t"] < 1e-3)
        refl = want["reflected"]
        got_refl = pr["eta"] == 1.0
        ok = ~g["near"] & ~near_crit
        assert (got_refl == refl)[ok].all(), label
        if s1 == 0:
            wi = -g["d"]
            mirror_n = sr.unit(wi + f64(pr["wo"]))
            mirror_n = mirror_n * np.sign(sr.dot(mirror_n, g["m"]))[:, None]
            c = np.abs(sr.dot(wi, g["m"]))
            rep.hold("d.normal_mirror", ratio(mirror_n, g["m"], g["amp"] * (1 + 1 / c)), where=ok & (c > 1e-3))
        rep.hold(f"d.wo[s1={s1:g}]", ratio(pr["wo"], want["wo"], cond), "d.wo", where=ok)
        rep.hold(f"d.pdf[s1={s1:g}]", ratio(pr["pdf"], want["pdf"], cond), "d.pdf", where=ok)
        rep.hold(f"d.eta[s1={s1:g}]", ratio(pr["eta"], want["eta"], 1), "b.eta", where=ok)
        knife = np.abs(want["side"]) < side_edge(surf, np.abs(sr.dot(g["d"], g["n"])))
        print(f"[surface] {label}: s1={s1:g}: {knife.sum()} of {n} samples with a side test on its edge left out ({knife.mean():.4%}, cap {CAP:.0%})")
        assert knife.mean() <= CAP
        live = ok & ~knife
        masked = want["masked"]
        assert ((pr["weight"] == 0).all(1) == masked)[live].all(), (label, "the weight is 0 exactly where wo leaves on the wrong side of the true surface")
        rep.hold(f"d.weight[s1={s1:g}]", ratio(pr["weight"], want["weight"][:, None] + np.zeros(3), cond * np.minimum(want["tcond"], 1e6)), "d.weight", where=live & ~masked)
        out[s1] = (masked & live).sum()
    print(f"[surface] {label}: masked samples: {out[0.0]} reflected, {out[1.0]} refracted of {n}; {g['mirrored'].sum()} probes with a mirrored normal")
    assert out[0.0] >= 5, (label, "no reflected sample went below the true surface")
    assert g["mirrored"].sum() >= 10
    return rep.worst


# ------------------------------------------------------------------------------------------- a: the reference's own vectors
def known_answers():
    return json.load(open(KNOWN))["entries"]


def known_items():
    return [("rectangle_plain", ("dielectric", "1.5")), ("rectangle_plain", ("dielectric", "1/1.5")), ("rectangle_plain", ("diffuse_default",))]


def allclose(got, want, rtol=1e-5, atol=1e-8):
    """dr.allclose with its defaults: |a - b| <= |b| rtol + atol, every component"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= np.abs(want) * rtol + atol).all())


def check_known_answers(prober, fresnel=None, label=""):
    """every entry of tests/golden/bsdf_known_answers.json: the probe is aimed at an axis-aligned rectangle (local frame = world axes),
    so si.wi = -d and bs.wo comes back as stated.  `fresnel`: the oracle's orc_fresnel for the entries that name it."""
    entries = known_answers()
    item_of = {"dielectric_1.5": 0, "dielectric_1/1.5": 1, "diffuse": 2}
    results, n_checked = {}, 0
    for e in entries:
        if e["via"] == "fresnel":
            if fresnel is None: continue
            got = fresnel(np.float32(e["cos_theta_i"]), np.float32(e["eta"]))
            if e["field"] == "snell":
                val = np.sin(np.arccos(np.float32(e["cos_theta_i"]))) - np.float32(1.5) * np.sin(np.arccos(np.float32(abs(got[1]))))
            else:
                val = got[["F", "cos_theta_t", "eta_it", "eta_ti"].index(e["field"])]
        else:
            k = item_of[e["bsdf"]]
            wi = np.array(results[e["wi_from"]] if "wi_from" in e else e["wi"], np.float64)
            dd = (-wi).astype(np.float32)[None]
            oo = (np.array([[SPACING * k + 0.25, -0.35, 0.0]]) + 2.0 * wi).astype(np.float32)
            pr = prober(oo, dd, np.float32([e["sample"]]), np.float32([e.get("wo", [0, 0, 1])]))
            assert pr["shape"][0] == k
            assert allclose(pr["wi"][0], wi, atol=1e-7), (e["id"], pr["wi"][0], wi)        # the probe does see the stated si.wi
            if e["field"] == "snell":
                val = np.sin(np.arccos(np.float32(wi[2]))) - np.float32(1.5) * np.sin(np.arccos(np.float32(abs(pr["wo_z"][0]))))
            elif e["field"] == "wo":
                val = pr["wo"][0]; results[e["id"]] = [float(x) for x in val]
            elif e["field"] == "eval0":
                val = pr["eval"][0, 0]
            elif e["field"] == "type":
                val = pr["type"][0]
            else:
                val = {"pdf": pr["pdf"], "eta": pr["eta"], "weight": pr["weight"], "eval_pdf": pr["eval_pdf"], "cos_theta_t": pr["wo_z"]}[e["field"]][0]
        ok = allclose(val, e["expected"], e.get("rtol", 1e-5), e.get("atol", 1e-8))
        assert ok, (label, e["id"], e["source"], val, e["expected"])
        n_checked += 1
    print(f"[surface] {label}: {n_checked} of {len(entries)} known answers of the reference hold")
    return n_checked


# --------------------------------------------------------------------------------------------------- f: transport closed forms
ENV_W, ENV_H = 8, 4
CAM = dict(origin=(0.0, 0.0, 6.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=20.0, width=8, height=6)
SPHERE_FOV = 12.0               # the unit sphere fills this film from 6 away: impact parameters up to 0.79 of the radius

PLATE_TILT = 40.0
PLATE_ETA = 1.5
MAX_DEPTH = 24
SEEDS = 8


def env_texels():
    i, j = np.meshgrid(np.arange(ENV_W), np.arange(ENV_H))
    base = 1.0 + 0.6 * np.sin(2 * np.pi * i / ENV_W + 0.4) * np.sin(np.pi * (j + 0.5) / ENV_H) + 0.25 * np.cos(np.pi * j / (ENV_H - 1))
    return np.stack([base, 0.8 * base + 0.3, 1.6 - 0.5 * base], -1).astype(np.float32)


def transport_scene(mi, tmp_path, what, integrator):
    path = os.path.join(str(tmp_path), "surface_env.exr")
    mi.write_exr(path, env_texels())
    glass = f'<bsdf type="dielectric"><float name="int_ior" value="{PLATE_ETA!r}"/><float name="ext_ior" value="1.0"/></bsdf>'
    if what == "plate":
        shape = ('<shape type="cube"><transform name="to_world"><scale x="6" y="6" z="0.02"/>'
                 f'<rotate y="1" angle="{PLATE_TILT!r}"/></transform>{glass}</shape>')
    else:
        shape = f'<shape type="sphere"><point name="center" x="0" y="0" z="0"/><float name="radius" value="1.0"/>{glass}</shape>'
    c = dict(CAM, fov=SPHERE_FOV if what == "sphere" else CAM["fov"])
    xml = f"""<scene version="3.0.0"><integrator type="{integrator}"><integer name="max_depth" value="{MAX_DEPTH}"/><integer name="rr_depth" value="{MAX_DEPTH + 100}"/></integrator>
      <sensor type="perspective"><float name="fov" value="{c['fov']!r}"/>
        <transform name="to_world"><lookat origin="{c['origin'][0]}, {c['origin'][1]}, {c['origin'][2]}" target="0, 0, 0" up="0, 1, 0"/></transform>
        <sampler type="independent"><integer name="sample_count" value="1"/></sampler>
        <film type="hdrfilm"><integer name="width" value="{c['width']}"/><integer name="height" value="{c['height']}"/><rfilter type="box"/></film></sensor>
      {shape}<emitter type="envmap"><string name="filename" value="{path}"/></emitter></scene>"""
    return mi.load_string(xml)


def closed_form_image(env, what, sub=24):
    """per pixel, the mean over a sub x sub grid of its footprint of the closed form.  Returns (image (H, W, 3), largest relative tail):
    the part of the series that a path of MAX_DEPTH vertices cannot reach, over the pixel's value."""
    import prb_closed_form as cf
    c = dict(CAM, fov=SPHERE_FOV if what == "sphere" else CAM["fov"])
    o, d = cf.camera_directions(c["origin"], c["target"], c["up"], c["fov"], c["width"], c["height"], sub)
    D = d.reshape(-1, 3)
    L = lambda v: env.radiance(v)
    lmax = float(env.rgb.max() * env.scale)
    if what == "plate":
        t = np.radians(PLATE_TILT)
        n = np.array([np.sin(t), 0.0, np.cos(t)])                          # rotate y by the tilt: z -> (sin, 0, cos)
        R, _ = sr.fresnel(np.abs(D @ n), 1.0, PLATE_ETA)
        T_tot, R_tot = sr.plate(R)
        val = R_tot[:, None] * L(sr.reflect(D, n + 0 * D)) + T_tot[:, None] * L(D)
        # a path with k vertices on the plate has seen k - 1 interface events; what is left after MAX_DEPTH - 1 of them is below R^(MAX_DEPTH - 3)
        tail = R ** (MAX_DEPTH - 3) * lmax
    else:
        orders = MAX_DEPTH - 2                                            # vertices: in, k internal, out
        hit, d_r, R, dirs, ws = sr.glass_sphere(np.broadcast_to(o, D.shape), D, (0, 0, 0), 1.0, PLATE_ETA, orders)
        assert hit.all(), "the sphere fills the film"
        val = R[:, None] * L(d_r)
        for dk, wk in zip(dirs, ws):
            val = val + wk[:, None] * L(dk)
        tail = (1 - R) * R ** orders * lmax
    img = val.reshape(c["height"], c["width"], sub * sub, 3).mean(2)
    rel_tail = (tail.reshape(c["height"], c["width"], -1).mean(2) / img.min(2)).max()
    return img, float(rel_tail)


def check_transport(render, env, what, label, power, spp_from=1, spp_max=1 << 16):
    """|mean - closed form| <= 4 SE over SEEDS seeds, at the smallest power-of-two spp whose SE is at most
    `power` of every pixel value.  render(spp, seed) -> (H, W, 3+).  Returns (spp, worst |mean - closed| / SE, worst SE / pixel)."""
    want, rel_tail = closed_form_image(env, what)
    assert rel_tail < 1e-6, (label, rel_tail)
    spp = spp_from
    while True:
        imgs = np.stack([np.asarray(render(spp, seed), np.float64)[..., :3] for seed in range(1, SEEDS + 1)])
        mean = imgs.mean(0); se = imgs.std(0, ddof=1) / np.sqrt(SEEDS)
        rel = float((se / want).max())
        if rel <= power or spp >= spp_max: break
        spp *= 2
    z = np.abs(mean - want) / np.maximum(se, 1e-30)
    print(f"[surface f] {label}: spp {spp} x {SEEDS} seeds: worst SE / pixel {rel:.4f} (power condition {power}), worst |mean - closed form| / SE {z.max():.2f}, "
          f"worst relative difference {np.abs(mean / want - 1).max():.4f}, truncated tail / pixel <= {rel_tail:.1e}")
    assert rel <= power, (label, "the power condition is not met", spp, rel)
    assert (z <= 4).all(), (label, float(z.max()), np.unravel_index(np.argmax(z), z.shape))
    return spp, float(z.max()), rel
