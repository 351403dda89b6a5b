"""What test_spot.py (CPU) and test_spot_gpu.py share: the spot and directional configurations of DESIGN.md section 17, their scenes and
reference points, the float64 reference with the condition number of every quantity, the ratio both files measure and the K table
both hold it to.

A quantity q of a lane is compared as |got - want| / (2^-23 cond max(1, |want|)) <= K[q] (the units of DESIGN.md 16.3), cond = 1 + the
summed |dq / dx_j| max(1, |x_j|) over the reference point's coordinates (central differences of the float64 reference) / max(1, |q|): a
float32 reference point carries a rounding of 2^-24 |x_j|, and the emitter's position is subtracted from it first.  K comes from the
float32 run of the same reference on the CPU (test_spot.py::test_k_table): 4 x the worst ratio, rounded up to a power of two; the device
is then held to the same K."""
import zlib

import numpy as np

import spot_ref as sr

EPS = sr.EPS
F = np.float32
MARGIN = 1e-5                 # lanes whose projected uv lies closer than this to a checkerboard tile edge are not compared per lane ...
MAX_LEFT_OUT = 0.01           # ... and at most this share of a batch may be
N_LANES = 4096
N_AXIS = 8                    # lanes on the optical axis
STEP_GAP = 1e-3               # beam_width == cutoff_angle makes the falloff a step: the reference points keep this angle (radians) from it
QUANTITIES = ("p", "d", "dist", "pdf", "weight")
# test_spot.py::test_k_table measures these and fails when the measurement asks for another value
K = {"p": 16.0, "d": 16.0, "dist": 4.0, "pdf": 1.0, "weight": 128.0}

# the probe scenes hold one cube [-1, 1]^3: the scene's bounding box, hence the sphere a directional light and a constant sky take
CUBE_LO, CUBE_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
BSPHERE = sr.bounding_sphere(CUBE_LO, CUBE_HI)


def rigid(axis_angle_deg, translate):
    """rotations about x, then y, then z (degrees), then a translation; rounded to float32"""
    ax, ay, az = np.radians(axis_angle_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    m = np.eye(4); m[:3, :3] = rz @ ry @ rx; m[:3, 3] = translate
    return m.astype(F)


class Case:
    def __init__(self, label, emitters, integrator="path"):
        self.label, self.emitters, self.integrator = label, emitters, integrator

    @property
    def light(self):
        return self.emitters[0]


def configs():
    posed = rigid((35.0, -20.0, 10.0), (0.5, 3.0, -1.5))
    return [
        Case("spot_default", [sr.Spot("spot_default", (1, 2, 3), to_world=rigid((0, 0, 0), (0, 0, 3)))]),
        Case("spot_narrow", [sr.Spot("spot_narrow", (10, 10, 10), 5.0, 4.0, rigid((0, 0, 0), (0, 0, 3)))]),
        Case("spot_wide", [sr.Spot("spot_wide", (1, 1, 1), 85.0, 30.0, rigid((0, 0, 0), (0, 0, 3)))]),
        Case("spot_step", [sr.Spot("spot_step", (2, 1, 0.5), 25.0, 25.0, rigid((0, 0, 0), (0, 0, 3)))]),
        Case("spot_posed", [sr.Spot("spot_posed", (3, 2, 1), 30.0, 12.0, posed)]),
        Case("spot_checker", [sr.Spot("spot_checker", (4, 4, 4), 40.0, 25.0, posed, sr.Checkerboard((1.0, 0.5, 0.25), (0.1, 0.2, 0.3), 4.0))]),
        Case("spot_and_sky", [sr.Spot("spot_and_sky", (5, 5, 5), 20.0, None, posed), sr.ConstantSky((0.25, 0.5, 0.75), BSPHERE)]),
        Case("dir_direction", [sr.Directional("dir_direction", (1, 2, 3), direction=(1.0, -2.0, 0.5), bsphere=BSPHERE)]),
        Case("dir_to_world", [sr.Directional("dir_to_world", (0.5, 0.25, 2), to_world=rigid((40.0, 25.0, 0.0), (0, 0, 0)), bsphere=BSPHERE)]),
    ]


def _matrix_xml(m):
    return '<transform name="to_world"><matrix value="' + " ".join(repr(float(x)) for x in np.asarray(m, F).reshape(-1)) + '"/></transform>'


def _rgb(name, v):
    return f'<rgb name="{name}" value="' + ", ".join(repr(float(x)) for x in v) + '"/>'


def emitter_xml(e):
    if e.kind == "spot":
        tex = ""
        if e.texture is not None:
            t = e.texture
            tex = (f'<texture type="checkerboard" name="texture">{_rgb("color0", t.color0)}{_rgb("color1", t.color1)}'
                   f'<transform name="to_uv"><scale x="{float(t.to_uv[0, 0])!r}" y="{float(t.to_uv[1, 1])!r}"/></transform></texture>')
        return (f'<emitter type="spot">{_rgb("intensity", e.intensity)}<float name="cutoff_angle" value="{float(e.cutoff_deg)!r}"/>'
                f'<float name="beam_width" value="{float(e.beam_deg)!r}"/>{_matrix_xml(e.to_world)}{tex}</emitter>')
    if e.kind == "directional":
        pose = (f'<vector name="direction" value="{", ".join(repr(float(x)) for x in e.direction)}"/>' if e.direction is not None else _matrix_xml(e.to_world))
        return f'<emitter type="directional">{_rgb("irradiance", e.irradiance)}{pose}</emitter>'
    return f'<emitter type="constant">{_rgb("radiance", e.radiance)}</emitter>'


def scene_xml(case, integrator=None):
    """the cube [-1, 1]^3 (diffuse) and the case's emitters"""
    return (f'<scene version="3.0.0"><integrator type="{integrator or case.integrator}"/><sensor type="perspective">'
            '<transform name="to_world"><lookat origin="0, 0, 6" target="0, 0, 0" up="0, 1, 0"/></transform>'
            '<film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/></film></sensor>'
            '<shape type="cube"/>' + "".join(emitter_xml(e) for e in case.emitters) + '</scene>')


def make_inputs(case, n=N_LANES):
    """(reference points (n x 3), samples (n x 2)), float32.  A spot: a third of the points each in the beam's core, the transition ring and
    the dark beyond the cutoff (halves when the ring is empty), by the angle to the optical axis; N_AXIS of them on the axis.  A directional
    light: half inside the scene's bounding sphere, half up to thirty radii outside."""
    rng = np.random.default_rng(zlib.crc32(case.label.encode()))
    e = case.light
    if e.kind == "spot":
        cutoff, beam = float(e.cutoff), float(e.beam)
        dark_hi = min(cutoff + np.radians(40.0), np.pi)
        u = rng.random(n)
        if beam == cutoff:
            theta = np.where(np.arange(n) % 2 == 0, u * (cutoff - STEP_GAP), cutoff + STEP_GAP + u * (dark_hi - cutoff - STEP_GAP))
        else:
            region = np.arange(n) % 3
            theta = np.where(region == 0, u * beam, np.where(region == 1, beam + u * (cutoff - beam), cutoff + u * (dark_hi - cutoff)))
        theta[:N_AXIS] = 0.0
        phi = rng.random(n) * 2 * np.pi
        r = 0.5 + 5.5 * rng.random(n)
        local = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], 1) * r[:, None]
        m = e.to_world.astype(np.float64)
        ref = local @ m[:3, :3].T + m[:3, 3]
    else:
        v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
        radius = float(e.radius)
        r = np.where(np.arange(n) % 2 == 0, rng.random(n) * 0.95 * radius, radius * (1.05 + 29 * rng.random(n)))
        ref = v * r[:, None] + e.center.astype(np.float64)
    return ref.astype(F), rng.random((n, 2)).astype(F)


def _fd(f, x, rel=1e-6):
    """sum over the columns of x of |d f / d x_j| max(1, |x_j|) by central differences; f returns (n,) or (n, k) (the worst component counts)"""
    tot = 0
    for j in range(x.shape[1]):
        h = rel * np.maximum(1.0, np.abs(x[:, j]))
        e = np.zeros_like(x); e[:, j] = h
        with np.errstate(invalid="ignore", divide="ignore"):
            dq = np.abs(f(x + e) - f(x - e))
        dq = np.nan_to_num(dq if dq.ndim == 1 else dq.max(1), nan=0.0, posinf=1e30) / (2 * h)
        tot = tot + dq * np.maximum(1.0, np.abs(x[:, j]))
    return tot


def reference(case, ref, smp):
    """the float64 reference at float32 inputs (taken as exact), with cond of every quantity and the mask of the compared lanes"""
    ref = np.asarray(ref, np.float64); smp = np.asarray(smp, np.float64)
    s = sr.sample_emitter_direction(case.emitters, ref, smp)
    big = lambda q: np.maximum(1.0, np.abs(q) if np.ndim(q) == 1 else np.abs(q).max(1))
    cond = {k: 1 + _fd(lambda x: sr.sample_emitter_direction(case.emitters, x, smp)[k], ref) / big(s[k]) for k in QUANTITIES}
    s["cond"] = cond
    s["ok"] = s["margin"] > MARGIN
    return s


def float32_run(case, ref, smp):
    return sr.sample_emitter_direction(case.emitters, np.asarray(ref, F), np.asarray(smp, F), F)


def ratio(got, want, cond):
    """|got - want| / (2^-23 cond max(1, |want|)) per lane (the worst component of a vector)"""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want)
    e = np.where(np.isnan(e), np.inf, e)
    if e.ndim == 2:
        e = e.max(1); big = np.maximum(1.0, np.abs(want).max(1))
    else:
        big = np.maximum(1.0, np.abs(want))
    return e / (EPS * np.asarray(cond, np.float64) * big)


def worst_ratios(ref, got):
    """per quantity: the worst ratio over the compared lanes"""
    ok = ref["ok"]
    return {k: float(ratio(got[k], ref[k], ref["cond"][k])[ok].max()) if ok.any() else 0.0 for k in QUANTITIES}


def k_from(worst):
    """4 x the worst ratio, rounded up to a power of two (at least 1)"""
    return float(2.0 ** max(0, int(np.ceil(np.log2(max(4 * worst, 1e-30))))))
