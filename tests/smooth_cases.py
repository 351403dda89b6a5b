"""Shared by test_smooth.py (CPU) and test_smooth_gpu.py: the probe scenes of the conductor, plastic and twosided BSDFs, the
configurations and inputs of the per-lane comparison, its condition numbers and its K.

Tolerances are K * 2^-23 * cond * max(1, |want|), as in rough_cases.py and surface_cases.py.
 * cond comes from the float64 reference alone: 1 + the sum over the inputs of a quantity (the components of wi, the two sample
   coordinates or the components of wo) of |d quantity / d input| / max(1, |quantity|), by central differences.
 * K is 4 times the worst ratio |float32 run - float64 run| / (2^-23 cond max(1, |want|)) of smooth_ref.py over every case below on
   these very inputs, rounded up to a power of two (test_smooth.py::test_k_table recomputes the ratios and holds 4 x them to K;
   DESIGN.md section 19 tabulates them).  Nothing in it comes from the device.
 * Lanes are left out only where a branch may flip: |wi.z| (for eval / pdf also |wo.z|) within MARGIN of 0, the 1-D sample within
   LOBE_MARGIN of plastic's lobe threshold, uv within TEX_MARGIN of a checkerboard edge.  At most 1 % of a batch."""
import os

import numpy as np

import smooth_ref as sr
from rough_cases import write_flat_png            # an 8-bit PNG of one value: a height map without slope

EPS = sr.EPS
N_LANES = 4096
MAX_LEFT_OUT = 0.01
MARGIN = 1e-5          # of cos theta_i / cos theta_o to 0: float32 inputs are exact, the device's dot products with an axis-aligned frame too
LOBE_MARGIN = 1e-4     # of s1 to prob_specular (a value below 1 formed by a dozen float32 operations: 1e-4 is a thousand ulp)
TEX_MARGIN = 1e-5      # of uv to a checkerboard edge, in uv units (uv of a hit point 3 away: a few 2^-24)

BOARD = sr.Tex([0.9, 0.6, 0.3], [0.2, 0.3, 0.7], scale=4.0)
GOLD = dict(eta=[0.143, 0.375, 1.442], k=[3.983, 2.386, 1.603])                  # per-channel eta and k (the order of magnitude of gold's)

# name, BSDF, shape ("planes": a rectangle and a small mesh; "sphere"), under a bumpmap
CASES = [
    ("mirror", sr.Conductor(), "planes", False),
    ("conductor_rgb", sr.Conductor(specular_reflectance=[0.9, 0.8, 0.7], **GOLD), "planes", False),
    ("conductor_board", sr.Conductor(specular_reflectance=BOARD, **GOLD), "planes", False),
    ("plastic", sr.Plastic(), "planes", False),
    ("plastic_nonlinear", sr.Plastic(int_ior=1.9, ext_ior="water", diffuse_reflectance=[0.8, 0.4, 0.1], specular_reflectance=[0.9, 0.9, 0.5], nonlinear=True), "planes", False),
    ("plastic_board", sr.Plastic(diffuse_reflectance=BOARD), "planes", False),
    ("twosided_diffuse", sr.TwoSided(sr.Diffuse([0.7, 0.5, 0.2])), "planes", False),
    ("twosided_plastic", sr.TwoSided(sr.Plastic(diffuse_reflectance=[0.3, 0.6, 0.8])), "planes", False),
    ("twosided_two", sr.TwoSided(sr.Plastic(nonlinear=True, diffuse_reflectance=BOARD), sr.Conductor(specular_reflectance=[0.9, 0.8, 0.7], **GOLD)), "planes", False),
    ("twosided_two_diffuse", sr.TwoSided(sr.Diffuse([0.7, 0.5, 0.2]), sr.Diffuse(BOARD)), "planes", False),
    ("twosided_sphere", sr.TwoSided(sr.Plastic(diffuse_reflectance=[0.3, 0.6, 0.8])), "sphere", False),
    ("bump_plastic", sr.Plastic(diffuse_reflectance=[0.3, 0.6, 0.8], specular_reflectance=[0.5, 0.7, 0.9]), "planes", True),
]

# K per output field: 4 x the worst float32-against-float64 ratio of smooth_ref.py over CASES with make_inputs(), rounded up to a power of
# two (test_smooth.py::test_k_table prints and holds them).  Measured worst ratios: wo 0.36, pdf 0.48, eta 0
# (it is 0 or 1), weight 5.15 (fresnel_conductor's term_1 - term_2 and term_3 - term_4 cancel for a metal, which the derivative against
# the inputs does not see), eval 0.43, eval_pdf 0.30.
K = {"wo": 2.0, "pdf": 2.0, "eta": 1.0, "weight": 32.0, "eval": 2.0, "eval_pdf": 2.0}
FIELDS = ("wo", "pdf", "eta", "weight", "eval", "eval_pdf")

MESH_X = 3.0      # the mesh is the rectangle's square moved by this along x


def write_mesh(path):
    """a 2 x 2 grid of quads (8 triangles, more than one leaf) over [-1, 1]^2 + (MESH_X, 0, 0) in the z = 0 plane, normal +z, uv = (x', y') / 2 + 1 / 2"""
    v = [(x, y) for y in (-1.0, 0.0, 1.0) for x in (-1.0, 0.0, 1.0)]
    lines = [f"v {x + MESH_X!r} {y!r} 0.0" for x, y in v] + [f"vt {(x + 1) / 2!r} {(y + 1) / 2!r}" for x, y in v]
    for j in range(2):
        for i in range(2):
            a, b, c, d = 3 * j + i + 1, 3 * j + i + 2, 3 * j + i + 5, 3 * j + i + 4
            lines += [f"f {a}/{a} {b}/{b} {c}/{c}", f"f {a}/{a} {c}/{c} {d}/{d}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def bsdf_xml(bsdf, bump, tmp_dir):
    x = bsdf.xml()
    if bump:
        png = os.path.join(tmp_dir, "flat.png"); write_flat_png(png)
        x = f'<bsdf type="bumpmap"><texture name="arbitrary" type="bitmap"><boolean name="raw" value="true"/><string name="filename" value="{png}"/></texture>{x}</bsdf>'
    return x.replace("<bsdf ", '<bsdf id="m" ', 1)


HEAD = """<scene version="3.0.0">{integrator}
<sensor type="perspective"><float name="fov" value="40"/><transform name="to_world"><lookat origin="0,0,5" target="0,0,0" up="0,1,0"/></transform>
<sampler type="independent"><integer name="sample_count" value="4"/></sampler>
<film type="hdrfilm"><integer name="width" value="4"/><integer name="height" value="4"/><rfilter type="box"/></film></sensor>
"""


def scene_xml(bsdf, shape, bump, tmp_dir, integrator='<integrator type="path"><integer name="max_depth" value="2"/></integrator>'):
    tmp_dir = str(tmp_dir)
    body = bsdf_xml(bsdf, bump, tmp_dir)
    if shape == "sphere":
        shapes = '<shape type="sphere"><float name="radius" value="1.0"/><ref id="m"/></shape>'
    else:
        obj = os.path.join(tmp_dir, "quad.obj"); write_mesh(obj)
        shapes = f'<shape type="rectangle"><ref id="m"/></shape><shape type="obj"><string name="filename" value="{obj}"/><ref id="m"/></shape>'
    return HEAD.format(integrator=integrator) + body + shapes + "</scene>"


def _dirs(rng, n):
    """unit directions towards the surface from both sides: cos theta uniform in 0.01 .. 1 with alternating sign, every 16th lane at
    grazing incidence (0.01 .. 0.05), every 32nd exactly at normal incidence"""
    k = np.arange(n)
    z = rng.uniform(0.01, 1.0, n)
    z = np.where(k % 16 == 5, rng.uniform(0.01, 0.05, n), z)
    z = np.where(k % 32 == 9, 1.0, z) * np.where(k % 2 == 0, 1.0, -1.0)
    ph = rng.uniform(0, 2 * np.pi, n)
    st = np.sqrt(1 - z * z)
    return np.stack([st * np.cos(ph), st * np.sin(ph), z], 1)


def _queries(rng, n):
    u = rng.normal(0, 1, (n, 3))
    u[np.arange(n) % 8 == 3] = np.array([0.0, 0.0, 1.0]) * np.where(rng.uniform(size=(n // 8 + 1, 1))[: (np.arange(n) % 8 == 3).sum()] < 0.5, -1.0, 1.0)
    return (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)


def make_inputs(bsdf, shape="planes", n=N_LANES, seed=11):
    """origins, directions, samples and query directions (all float32), and the nominal wi and uv of the hits for the CPU run.  planes:
    even pairs of lanes aim at the rectangle, odd pairs at the mesh.  sphere: half the rays start outside, half inside (they see its back)."""
    rng = np.random.default_rng(seed)
    if shape == "sphere":
        d = rng.normal(0, 1, (n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        inside = np.arange(n) % 2 == 1
        t = rng.uniform(-0.9, 0.9, (n, 3)); t -= (t * d).sum(1, keepdims=True) * d                 # a point of the plane through the centre, orthogonal to d
        t *= np.minimum(1.0, 0.95 / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-9))
        o = np.where(inside[:, None], t * 0.3, t - 3.0 * d)
        wi_nom = _dirs(rng, n)                                                   # (the CPU run's stand-in: odd lanes see the back, as the inside rays do)
        uv = rng.uniform(0.05, 0.95, (n, 2))
    else:
        wi_nom = _dirs(rng, n)
        d = -wi_nom
        p = np.concatenate([rng.uniform(-0.9, 0.9, (n, 2)), np.zeros((n, 1))], 1)
        uv = (p[:, :2] + 1) / 2
        p[:, 0] += np.where((np.arange(n) // 2) % 2 == 1, MESH_X, 0.0)
        o = p - 3.0 * d
    o = o.astype(np.float32); d = d.astype(np.float32)
    if shape != "sphere":
        wi_nom = -d.astype(np.float64)
    smp = rng.uniform(0.002, 0.998, (n, 3)).astype(np.float32)
    s = bsdf.sample(wi_nom, smp[:, 0].astype(np.float64), smp[:, 1:].astype(np.float64), uv)
    smp[:, 0] = np.where(s["lobe_margin"] < 0.02, np.mod(smp[:, 0] + 0.5, 1.0), smp[:, 0]).astype(np.float32)      # s1 stays away from the lobe threshold
    return o, d, smp, _queries(rng, n), wi_nom.astype(np.float32), uv.astype(np.float32)


def _fd(f, x, h=1e-6):
    """sum over the columns of x of |d f / d x_j| by central differences; f returns (n,) or (n, k) (the worst component counts)"""
    tot = 0
    for j in range(x.shape[1]):
        e = np.zeros_like(x); e[:, j] = h
        with np.errstate(invalid="ignore"):
            dq = np.abs(f(x + e) - f(x - e)) / (2 * h)
        dq = np.nan_to_num(dq, nan=0.0, posinf=1e30)
        tot = tot + (dq if dq.ndim == 1 else dq.max(1))
    return tot


def reference(bsdf, wi, smp, wo, uv):
    """the float64 reference at float32 inputs (taken as exact), the condition number of every field and the lanes that are compared"""
    wi = np.asarray(wi, np.float64); smp = np.asarray(smp, np.float64); wo = np.asarray(wo, np.float64); uv = np.asarray(uv, np.float64)
    s = bsdf.sample(wi, smp[:, 0], smp[:, 1:], uv)
    ev, pdf, em = bsdf.eval_pdf(wi, wo, uv)
    big = lambda q: np.maximum(1.0, np.abs(q) if np.ndim(q) == 1 else np.abs(q).max(1))
    xs = np.concatenate([wi, smp[:, 1:]], 1)
    sens = lambda key: _fd(lambda x: bsdf.sample(x[:, :3], smp[:, 0], x[:, 3:], uv)[key], xs)
    cond = {k: 1 + sens(k) / big(s[k]) for k in ("wo", "pdf", "weight")}
    cond["eta"] = np.ones(len(wi))
    xe = np.concatenate([wi, wo], 1)
    cond["eval"] = 1 + _fd(lambda x: bsdf.eval_pdf(x[:, :3], x[:, 3:], uv)[0], xe) / big(ev)
    cond["eval_pdf"] = 1 + _fd(lambda x: bsdf.eval_pdf(x[:, :3], x[:, 3:], uv)[1], xe) / big(pdf)
    sample_ok = (np.abs(wi[:, 2]) > MARGIN) & (s["lobe_margin"] > LOBE_MARGIN) & (s["tex_margin"] > TEX_MARGIN)
    return {"wo": s["wo"], "pdf": s["pdf"], "eta": s["eta"], "type": s["type"], "weight": s["weight"], "eval": ev, "eval_pdf": pdf, "cond": cond,
            "sample_ok": sample_ok, "eval_ok": (em > MARGIN) & (np.abs(wi[:, 2]) > MARGIN) & (bsdf_tex_margin(bsdf, uv) > TEX_MARGIN)}


def bsdf_tex_margin(bsdf, uv):
    """the smallest distance of uv to an edge of any checkerboard the BSDF holds"""
    m = np.full(len(uv), np.inf)
    for b in (bsdf.front, bsdf.back) if isinstance(bsdf, sr.TwoSided) else (bsdf,):
        for t in (getattr(b, a, None) for a in ("reflectance", "spec", "diff")):
            if t is not None:
                m = np.minimum(m, t.margin(uv))
    return m


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


def worst_ratios(ref, got, fields=FIELDS):
    """per field: the worst ratio over the lanes that are compared, and how many are left out"""
    out = {}
    for k in fields:
        ok = ref["eval_ok"] if k in ("eval", "eval_pdf") else ref["sample_ok"]
        want = ref["wo"][:, 2] if k == "wo_z" else ref[k]
        r = ratio(got[k], want, ref["cond"]["wo" if k == "wo_z" else k])
        out[k] = (float(r[ok].max()) if ok.any() else 0.0, int((~ok).sum()))
    return out


def run32(bsdf, wi, smp, wo, uv, **mistake):
    """smooth_ref.py in float32 (or, with a seeded mistake, in float64) in the shape worst_ratios() takes"""
    T = np.float64 if mistake else np.float32
    s = bsdf.sample(np.asarray(wi, T), np.asarray(smp[:, 0], T), np.asarray(smp[:, 1:], T), np.asarray(uv, T), T, **mistake)
    ev, p, _ = bsdf.eval_pdf(np.asarray(wi, T), np.asarray(wo, T), np.asarray(uv, T), T, **mistake)
    return {"wo": s["wo"], "pdf": s["pdf"], "eta": s["eta"], "weight": s["weight"], "eval": ev, "eval_pdf": p, "type": s["type"]}
