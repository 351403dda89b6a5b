"""Cases of the medium tests (test_medium.py, test_medium_gpu.py): small non-cubic grids with one distinct value per voxel under five volume
transforms, a homogeneous medium, the probe's inputs, and the pure-absorber and emitter-march scenes.  numpy only."""
import os

import numpy as np

import medium_ref as mr


def grid_values(shape, seed):
    """One distinct value per voxel in [0.6, 1.4], shuffled: an index-order mistake moves every lookup.  (z, y, x)."""
    n = int(np.prod(shape))
    return (0.6 + 0.8 * np.random.default_rng(seed).permutation(n) / max(n - 1, 1)).reshape(shape).astype(np.float32)


GRID_A = grid_values((3, 2, 4), 1)
GRID_B = grid_values((2, 3, 1), 2)
AXIS = (2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0)                                  # a unit vector with rational entries
HEADER_BOX = ((-0.5, 0.25, 1.0), (1.5, 0.75, 4.0))
STEPS_B = [("scale", (1.5, 0.8, 2.5)), ("translate", (-0.6, -0.3, -1.1))]

# name -> grid, the volume's to_world steps, the file header's box (use_grid_bbox) or None, the shape: "volume" (the cube under the volume's
# own transform), or ("aabb", factor): the volume's world AABB scaled about its centre
VOLUMES = {
    "a": dict(grid=GRID_A, steps=[("scale", (2.0, 2.0, 2.0)), ("translate", (-1.0, -1.0, -1.0))], header=None, shape="volume"),
    "b": dict(grid=GRID_B, steps=STEPS_B, header=None, shape="volume"),
    "c": dict(grid=GRID_A, steps=[("rotate", AXIS, 35.0), ("scale", (1.2, 0.7, 1.9)), ("translate", (0.3, -0.2, 0.1))], header=None, shape=("aabb", 0.9)),
    "d": dict(grid=GRID_B, steps=[("scale", (0.8, 2.0, 0.5)), ("translate", (-0.4, -1.0, -1.2))], header=HEADER_BOX, shape="volume"),
    "e": dict(grid=GRID_B, steps=STEPS_B, header=None, shape=("aabb", 1.6)),
}
HOM = dict(sigma_t=(0.7, 1.3, 2.1), scale=1.7, albedo=(0.9, 0.5, 0.2))          # case (f)
ALBEDO = (0.9, 0.8, 0.6)
PROBE_SCALE = 2.5


def frame(name):
    v = VOLUMES[name]
    return mr.volume_frame(mr.compose(v["steps"]), v["header"])


def frame32(name):
    """The frame rounded to float32, as a description holds it (the loader's may differ from it in the last place)"""
    return tuple(np.asarray(a, np.float32).astype(np.float64) for a in frame(name))


def unit_cube_to_world(name):
    """4 x 4: the grid's unit cube -> world (the inverse of the volume's to_local)"""
    tl = np.vstack([frame(name)[0], [0, 0, 0, 1.0]])
    return np.linalg.inv(tl)


def shape_matrix(name):
    """4 x 4 to_world of the cube shape ([-1, 1]^3) that holds the medium"""
    v = VOLUMES[name]
    unit = mr.translate((0.5, 0.5, 0.5)) @ mr.scale(0.5)                  # [-1, 1]^3 -> [0, 1]^3
    if v["shape"] == "volume":
        return unit_cube_to_world(name) @ unit
    _, lo, hi = frame(name)
    return mr.translate((lo + hi) / 2) @ mr.scale((hi - lo) / 2 * v["shape"][1])


def _f(x):
    return repr(float(x))


def steps_xml(steps):
    out = []
    for st in steps:
        if st[0] == "rotate":
            out.append(f'<rotate x="{_f(st[1][0])}" y="{_f(st[1][1])}" z="{_f(st[1][2])}" angle="{_f(st[2])}"/>')
        else:
            out.append(f'<{st[0]} x="{_f(st[1][0])}" y="{_f(st[1][1])}" z="{_f(st[1][2])}"/>')
    return "".join(out)


def matrix_xml(m):
    return '<matrix value="' + " ".join(_f(x) for x in np.asarray(m).reshape(-1)) + '"/>'


def write_volume(mi, tmp_dir, name):
    v = VOLUMES[name]
    path = os.path.join(str(tmp_dir), f"medium_{name}.vol")
    if v["header"] is None:
        mi.write_volume_grid(path, v["grid"])
    else:
        mi.write_volume_grid(path, v["grid"], bbox_min=v["header"][0], bbox_max=v["header"][1])
    return path


def medium_xml(mi, tmp_dir, name, med_scale, albedo=ALBEDO, spectral=True, steps=None, use_grid_bbox=None):
    v = VOLUMES[name]
    ugb = (v["header"] is not None) if use_grid_bbox is None else use_grid_bbox
    return f"""<medium type="heterogeneous" id="smoke">
    <volume name="sigma_t" type="gridvolume"><string name="filename" value="{write_volume(mi, tmp_dir, name)}"/>
      {'<boolean name="use_grid_bbox" value="true"/>' if ugb else ''}
      <transform name="to_world">{steps_xml(v["steps"] if steps is None else steps)}</transform></volume>
    <rgb name="albedo" value="{', '.join(map(_f, albedo))}"/><float name="scale" value="{_f(med_scale)}"/>
    <boolean name="has_spectral_extinction" value="{'true' if spectral else 'false'}"/></medium>"""


def hom_medium_xml():
    h = HOM
    return (f'<medium type="homogeneous" id="smoke"><rgb name="sigma_t" value="{", ".join(map(_f, h["sigma_t"]))}"/>'
            f'<rgb name="albedo" value="{", ".join(map(_f, h["albedo"]))}"/><float name="scale" value="{_f(h["scale"])}"/></medium>')


def scene_xml(medium, shape_m, cam, integrator="volpath", integrator_extra="", max_depth=8, rr_depth=64, spp=4, rest=None, width=4, height=3):
    """One medium `smoke` inside a null-bounded cube under shape_m, a perspective camera, and `rest` (default: a constant environment of
    radiance 1).  rr_depth is out of reach: Russian roulette would put weights of 1 / 0.95 on the survivors, and the per-pixel standard errors
    of the absorber tests are sized for a plain Bernoulli estimate."""
    rest = '<emitter type="constant"><rgb name="radiance" value="1, 1, 1"/></emitter>' if rest is None else rest
    return f"""<scene version="3.0.0">
  <integrator type="{integrator}"><integer name="max_depth" value="{max_depth}"/><integer name="rr_depth" value="{rr_depth}"/>{integrator_extra}</integrator>
  {medium}
  <sensor type="perspective"><float name="fov" value="{_f(cam['fov'])}"/>
    <transform name="to_world"><lookat origin="{', '.join(map(_f, cam['origin']))}" target="{', '.join(map(_f, cam['target']))}" up="{', '.join(map(_f, cam['up']))}"/></transform>
    <sampler type="independent"><integer name="sample_count" value="{spp}"/></sampler>
    <film type="hdrfilm"><integer name="width" value="{width}"/><integer name="height" value="{height}"/><rfilter type="box"/></film>
  </sensor>
  <shape type="cube"><transform name="to_world">{matrix_xml(shape_m)}</transform><bsdf type="null"/><ref name="interior" id="smoke"/></shape>
  {rest}
</scene>"""


def camera(name, fov=3.0, dist=9.0, direction=(0.15, 0.1, 1.0)):
    """A narrow camera aimed at the centre of the volume's AABB: every pixel's rays cross the whole volume"""
    _, lo, hi = frame(name)
    c = (lo + hi) / 2
    d = np.asarray(direction, np.float64); d /= np.linalg.norm(d)
    return dict(origin=tuple(c - dist * d), target=tuple(c), up=(0.0, 1.0, 0.0), fov=fov)


def probe_scene_xml(mi, tmp_dir, name):
    if name == "f":
        return scene_xml(hom_medium_xml(), np.eye(4), dict(origin=(0, 0, -9), target=(0, 0, 0), up=(0, 1, 0), fov=3.0))
    return scene_xml(medium_xml(mi, tmp_dir, name, PROBE_SCALE), shape_matrix(name), camera(name))


# ------------------------------------------------------------------------------------------------------------- probe inputs
def local_points(shape):
    """Local points of the lookup-only mode: (points (n, 3) float32, exact (n,)): texel centres (exact: every coordinate times its
    resolution minus 1/2 is an integer in floating point, so the lookup must return the texel itself), texel faces, cube corners, and
    points up to one cube width outside on every side."""
    rz, ry, rx = shape
    res = np.array([rx, ry, rz], np.float64)
    pts = []
    for z in range(rz):
        for y in range(ry):
            for x in range(rx):
                pts.append(((x + 0.5) / rx, (y + 0.5) / ry, (z + 0.5) / rz))
    n_centres = len(pts)
    for z in range(rz + 1):
        for y in range(ry + 1):
            for x in range(rx + 1):
                pts.append((x / rx, y / ry, z / rz))                        # texel faces / corners, the cube's corners among them
    for a in range(3):
        for off in (-1.0, -0.37, -1e-3, 1.0 + 1e-3, 1.37, 2.0):
            p = [0.31, 0.62, 0.45]; p[a] = off
            pts.append(tuple(p))
    pts += [(-1.0, -1.0, -1.0), (2.0, 2.0, 2.0), (-0.5, 1.5, 0.5), (1.5, -0.5, 2.0)]
    r = np.random.default_rng(5)
    pts += [tuple(p) for p in r.uniform(-1.0, 2.0, (24, 3))]
    pts = np.asarray(pts, np.float32)
    f = pts.astype(np.float64) * res - 0.5
    exact = np.zeros(len(pts), bool)
    exact[:n_centres] = (f[:n_centres] == np.round(f[:n_centres])).all(-1)
    return pts, exact


def probe_rays(name, seed=11):
    """Rays for a grid volume, as float32 arrays o, d (n, 3), maxt, sample (n), channel (n, uint32), and kind (n, list of str).  Built in
    the AABB's own units so that no ray is within rounding of a decision, except the lanes whose kind says so ("face": on a box face with a
    zero direction component, "nan": NaN in o), which are compared device against oracle only."""
    _, lo, hi = frame32(name)
    ext = hi - lo
    r = np.random.default_rng(seed)
    o, d, mt, kind = [], [], [], []
    at = lambda u: lo + np.asarray(u) * ext

    def add(oo, dd, m, k):
        o.append(oo); d.append(dd); mt.append(m); kind.append(k)
    inside = [at(r.uniform(0.15, 0.85, 3)) for _ in range(12)]
    for i in range(12):                                                       # start outside, aimed at an interior point: clear hits
        start = at(r.uniform(-1.5, 2.5, 3)); start[i % 3] = at([-0.8 - 0.1 * i] * 3)[i % 3] if i % 2 else at([1.7 + 0.1 * i] * 3)[i % 3]
        dd = inside[i] - start
        L = np.linalg.norm(dd)
        add(start, dd / L, np.inf, "outside"); add(start, dd / L, 0.2 * np.min(np.abs(lo - start)[i % 3:i % 3 + 1]) , "outside-maxt-before")
        add(start, dd / L, L, "outside-maxt-inside")
    for i in range(10):                                                       # start inside
        dd = r.normal(size=3); dd /= np.linalg.norm(dd)
        add(inside[i], dd, np.inf, "inside"); add(inside[i], dd, 0.05 * ext.min(), "inside-maxt-inside")
    for i in range(8):                                                        # start beyond a face, moving away from the box, or past it
        a = i % 3
        start = at(r.uniform(0.2, 0.8, 3)); start[a] = at([2.0] * 3)[a]
        dd = r.normal(size=3); dd[a] = abs(dd[a]) + 0.5; dd /= np.linalg.norm(dd)
        add(start, dd, np.inf, "behind")                                      # (the slab test is a line test: it may report the box behind the ray)
        side = r.normal(size=3); side[a] = 0.0; side[(a + 1) % 3] = 1.0; side /= np.linalg.norm(side)
        add(start, side, np.inf, "miss")
    for a in range(3):                                                        # one and two zero direction components
        b, c = (a + 1) % 3, (a + 2) % 3
        e1 = np.zeros(3); e1[a] = 1.0
        e2 = np.zeros(3); e2[a] = 0.6; e2[b] = 0.8
        for dd in (e1, -e1, e2, -e2):
            inslab = at([0.37, 0.58, 0.44]); inslab[a] = at([-0.9] * 3)[a] if dd[a] > 0 else at([1.9] * 3)[a]
            if dd is e2 or (dd == -e2).all():
                inslab[b] = at([0.3] * 3)[b] - (at([0.5] * 3)[a] - inslab[a]) * dd[b] / dd[a]       # aimed at an interior point
            add(inslab, dd, np.inf, "axis-in-slab")
            outslab = inslab.copy(); outslab[c] = at([1.6] * 3)[c]
            add(outslab, dd, np.inf, "axis-out-of-slab")
            add(at([0.41, 0.52, 0.63]), dd, np.inf, "axis-inside")
        on = at([0.4, 0.6, 0.5]); on[b] = lo[b]                                # on a face, a zero component along that face's axis
        add(on, e1, np.inf, "face"); on2 = on.copy(); on2[b] = hi[b]; add(on2, -e1, np.inf, "face")
        onf = at([0.4, 0.6, 0.5]); onf[a] = lo[a]                              # on the box (entry face), moving in
        dd = np.array([0.3, 0.2, 0.1]); dd[a] = 1.0; dd /= np.linalg.norm(dd)
        add(onf, dd, np.inf, "on-box")
    add(np.array([np.nan, 0.1, 0.2]), np.array([0.0, 0.6, 0.8]), np.inf, "nan")
    o, d, mt = np.asarray(o, np.float32), np.asarray(d, np.float32), np.asarray(mt, np.float32)
    n = len(o)
    fixed = np.array([0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24], np.float32)
    reps = []
    for j in range(6):                                                        # every ray with the four fixed samples and two random ones
        u = np.full(n, fixed[j], np.float32) if j < 4 else r.random(n).astype(np.float32)
        reps.append(u)
    O = np.tile(o, (6, 1)); D = np.tile(d, (6, 1)); MT = np.tile(mt, 6); U = np.concatenate(reps)
    CH = (np.arange(len(U)) % 3).astype(np.uint32)
    return O, D, MT, U, CH, kind * 6


def hom_rays(seed=12):
    r = np.random.default_rng(seed)
    n = 96
    o = r.uniform(-2, 2, (n, 3)).astype(np.float32)
    d = r.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[0] = (0, 0, 1); d[1] = (0, 1, 0); d[2] = (0, 0.6, 0.8)
    mt = np.where(np.arange(n) % 3 == 0, np.inf, r.uniform(0.05, 0.8, n)).astype(np.float32)
    u = r.random(n).astype(np.float32)
    u[:8] = np.array([0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24] * 2, np.float32)
    ch = (np.arange(n) % 3).astype(np.uint32)
    o[n - 1, 0] = np.nan
    kind = ["hom"] * (n - 1) + ["nan"]
    return o, d, mt, u, ch, kind
