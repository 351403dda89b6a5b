"""Shared by test_rough.py (CPU) and test_rough_gpu.py: the probe scene of the rough dielectric, the configurations and inputs of the
per-lane comparison, its condition numbers and its K.

Tolerances are K * 2^-23 * cond * max(1, |want|), as in surface_cases.py.
 * cond comes from the float64 reference alone: 1 + the sum over the inputs of a quantity (the components of wi, the two sample
   coordinates or the components of wo) of |d quantity / d input| / max(1, |quantity|), by central differences.  A float32
   evaluation rounds its first intermediate results by about 2^-24 of the inputs' size, so the derivative against the inputs is
   the factor such an error reaches the result with.  One intermediate result counts like an input: the residual of the last Newton
   step of Beckmann's visible normals (reference()).  rough_ref.py forms its two small sines without cancellation in either precision,
   as the device does, so a roughness at the clamp (1e-4) gets the same kind of bound as any other.
 * K is 4 times the worst ratio |float32 run - float64 run| / (2^-23 cond max(1, |want|)) of rough_ref.py on these very inputs,
   rounded up (test_rough.py::test_k_table recomputes the ratios and holds them below K / 4; DESIGN.md section 15 tabulates them).
   Nothing here comes from the device.
 * Lanes within MARGIN of a discontinuity are left out (s1 against F, cos theta_i against 0, the cut of D; for eval / pdf at a given
   wo also cos theta_o against 0 and the side tests of wi and wo against the half vector, roughdielectric.cpp:467-468, which cut the
   pdf of the all-normals sampling where D G does not vanish), at most 1 % of a batch."""
import os
import struct
import zlib

import numpy as np

import rough_ref as rr

EPS = rr.EPS
MARGIN = 1e-5
N_LANES = 4096
MAX_LEFT_OUT = 0.01

IORS = [(1.5046, 1.000277), (1.0, 1.5)]                       # bk7 / air, and from the denser side
ALPHAS = [(1e-4, 1e-4), (0.05, 0.05), (0.1, 0.1), (0.5, 0.5), (0.5, 0.2)]


def configs():
    out = []
    for ggx in (False, True):
        for visible in (True, False):
            for au, av in ALPHAS:
                for ii, ei in IORS:
                    out.append(rr.Config(au, av, ggx, visible, ii, ei))
    return out


# K per quantity: 4 x the worst float32-against-float64 ratio of rough_ref.py over all configurations of configs() with the inputs
# of make_inputs() (measured on the CPU by test_rough.py::test_k_table, tabulated in DESIGN.md section 15), rounded up.
# The lobe is chosen by s1 <= F: a lane whose |s1 - F| lies within MARGIN, or within the tolerance F itself has by the rule above, is
# left out (F is no output of the probe; its K is that of the other sampled quantities).
K_F = 12.0
K = {"wo": 4.0, "pdf": 16.0, "eta": 4.0, "weight": 16.0, "eval": 8.0, "eval_pdf": 8.0}


def bsdf_xml(cfg, extra=""):
    a = (f'<float name="alpha" value="{cfg.alpha_u!r}"/>' if cfg.alpha_u == cfg.alpha_v else
         f'<float name="alpha_u" value="{cfg.alpha_u!r}"/><float name="alpha_v" value="{cfg.alpha_v!r}"/>')
    return (f'<bsdf type="roughdielectric">{a}<string name="distribution" value="{"ggx" if cfg.ggx else "beckmann"}"/>'
            f'<boolean name="sample_visible" value="{"true" if cfg.visible else "false"}"/>'
            f'<float name="int_ior" value="{cfg.int_ior!r}"/><float name="ext_ior" value="{cfg.ext_ior!r}"/>{extra}</bsdf>')


def scene_xml(bsdf, integrator='<integrator type="path"><integer name="max_depth" value="2"/></integrator>', scale=1.0, extra="", fov=1.0,
              origin=(0, 0, 5), spp=4, res=4, sensor_extra=""):
    """one rectangle in the z = 0 plane (normal +z, shading frame = the world axes) carrying `bsdf`"""
    ox, oy, oz = origin
    up = "0,1,0" if abs(ox) + abs(oz) > 0 else "0,0,1"
    return f"""<scene version="3.0.0">{integrator}
<sensor type="perspective"><float name="fov" value="{fov!r}"/><transform name="to_world"><lookat origin="{ox!r},{oy!r},{oz!r}" target="0,0,0" up="{up}"/></transform>
<sampler type="independent"><integer name="sample_count" value="{spp}"/></sampler>
<film type="hdrfilm"><integer name="width" value="{res}"/><integer name="height" value="{res}"/><rfilter type="box"/></film>{sensor_extra}</sensor>
<shape type="rectangle"><transform name="to_world"><scale value="{scale!r}"/></transform>{bsdf}{extra}</shape>
</scene>"""


def write_flat_png(path, value=128, size=4):
    """an 8-bit grey PNG of one value: a height map without slope"""
    raw = b"".join(b"\x00" + bytes([value]) * size for _ in range(size))
    chunk = lambda tag, body: struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", size, size, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def make_inputs(cfg, n=N_LANES, seed=7):
    """rays onto the rectangle whose wi covers both sides, samples, and query directions: half of them near the direction the float64
    reference samples for the nominal wi (where the lobes are), half uniform on the sphere.  All float32."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.03, 1.0, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    ph = rng.uniform(0, 2 * np.pi, n)
    st = np.sqrt(1 - z * z)
    wi = np.stack([st * np.cos(ph), st * np.sin(ph), z], 1)
    d = (-wi).astype(np.float32)
    p = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), np.zeros((n, 1))], 1)
    o = (p - 3.0 * d.astype(np.float64)).astype(np.float32)
    smp = rng.uniform(0.002, 0.998, (n, 3)).astype(np.float32)
    s = rr.sample(cfg, -d.astype(np.float64), smp[:, 0].astype(np.float64), smp[:, 1:].astype(np.float64))
    close = np.abs(smp[:, 0] - s["F"]) < 0.02                        # s1 is kept away from the lobe choice's threshold (the cap on lanes left out)
    smp[:, 0] = np.where(close, np.mod(s["F"] + 0.5, 1.0), smp[:, 0]).astype(np.float32)
    near = s["wo"] + rng.normal(0, 0.3 * max(cfg.alpha_u, cfg.alpha_v, 1e-3), (n, 3))
    u = rng.normal(0, 1, (n, 3))
    use_near = (np.arange(n) % 4 < 2) & np.isfinite(near).all(1) & (np.abs(near).sum(1) > 0)
    woq = np.where(use_near[:, None], near, u)
    woq = (woq / np.linalg.norm(woq, axis=1, keepdims=True)).astype(np.float32)
    return o, d, smp, woq


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


def reference(cfg, wi, smp, wo):
    """the float64 reference at float32 inputs (taken as exact), with the condition number and the margin of every quantity"""
    wi = np.asarray(wi, np.float64); smp = np.asarray(smp, np.float64); wo = np.asarray(wo, np.float64)
    s = rr.sample(cfg, wi, smp[:, 0], smp[:, 1:])
    ev, pdf, em = rr.eval_pdf(cfg, wi, wo)
    xs = np.concatenate([wi, smp[:, 1:]], 1)
    big = lambda q: np.maximum(1.0, np.abs(q) if np.ndim(q) == 1 else np.abs(q).max(1))
    # Beckmann's visible normals come out of a Newton iteration in the erf domain: the residual of its last step is rounded at 2^-24
    # of a sum of size 1 .. 2 and divided by the step's derivative, whatever the inputs were (rough_ref.py, sample_visible_11: dx).
    # Its derivative counts like those of the inputs.
    hooks = [("dx", 1e-7)] if (cfg.visible and not cfg.ggx) else []

    def sens(key):
        tot = _fd(lambda x: rr.sample(cfg, x[:, :3], smp[:, 0], x[:, 3:])[key], xs)
        for name, h in hooks:
            with np.errstate(invalid="ignore"):
                dq = np.abs(rr.sample(cfg, wi, smp[:, 0], smp[:, 1:], **{name: h})[key] - rr.sample(cfg, wi, smp[:, 0], smp[:, 1:], **{name: -h})[key]) / (2 * h)
            dq = np.nan_to_num(dq, nan=0.0, posinf=1e30)
            tot = tot + (dq if dq.ndim == 1 else dq.max(1))
        return tot
    cond = {k: 1 + sens(k) / big(s[k]) for k in ("wo", "pdf", "weight")}
    cond["eta"] = np.ones(len(wi))
    xe = np.concatenate([wi, wo], 1)
    cond["eval"] = 1 + _fd(lambda x: rr.eval_pdf(cfg, x[:, :3], x[:, 3:])[0], xe) / big(ev)
    cond["eval_pdf"] = 1 + _fd(lambda x: rr.eval_pdf(cfg, x[:, :3], x[:, 3:])[1], xe) / big(pdf)
    return {"wo": s["wo"], "pdf": s["pdf"], "eta": s["eta"], "type": s["type"], "weight": s["weight"], "eval": ev, "eval_pdf": pdf,
            "cond": cond, "sample_ok": (s["margin"] > MARGIN) & (s["lobe_margin"] > np.maximum(MARGIN, K_F * EPS * (1 + sens("F")))), "eval_ok": em > MARGIN, "active": s["active"]}


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
    """per quantity: the worst ratio over the lanes that are compared, and how many are left out.  got: dict with wo, pdf, eta, weight
    (scalar per lane), eval (scalar per lane), eval_pdf."""
    out = {}
    for k in ("wo", "pdf", "eta", "weight", "eval", "eval_pdf"):
        ok = ref["eval_ok"] if k in ("eval", "eval_pdf") else ref["sample_ok"]
        r = ratio(got[k], ref[k], ref["cond"][k])
        out[k] = (float(r[ok].max()) if ok.any() else 0.0, int((~ok).sum()))
    return out


def scaling_ratio(cfg, wi, m):
    """D(m) / D_scaled(m) m.z-free: what weight * pdf of a sample lacks against eval when all normals are sampled (1 otherwise)"""
    if cfg.visible:
        return np.ones(len(m))
    T = np.float64
    au, av = cfg.alphas(T)
    d = rr.Distribution(au, av, cfg.ggx, False, T)
    ds = d.scaled(1.2 - 0.2 * np.sqrt(np.abs(np.asarray(wi, T)[:, 2])))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.nan_to_num(d.eval(m) / ds.eval(m), nan=1.0, posinf=1.0)


# The sampling tests of the renderer this project follows (its test_rough_dielectric.py, test02 - test09): wi, roughness, distribution,
# sampling mode and indices as there.  test10 / test11 restrict a lobe and are not restated.
CHI2_CASES = [
    ("test02_rough_grazing", rr.Config(0.5), (0.8, 0.3, 0.05)),
    ("test03_beckmann_all", rr.Config(0.5, ggx=False, visible=False), (0.5, 0.0, 0.5)),
    ("test04_beckmann_visible", rr.Config(0.5, ggx=False, visible=True), (0.5, 0.0, 0.5)),
    ("test05_ggx_all", rr.Config(0.5, ggx=True, visible=False), (0.5, 0.0, 0.5)),
    ("test06_ggx_visible", rr.Config(0.5, ggx=True, visible=True), (0.5, 0.5, 0.001)),
    ("test07_from_inside", rr.Config(0.5), (0.2, -0.6, -0.5)),
    ("test08_from_inside_tir", rr.Config(0.5), (0.8, 0.3, -0.05)),
    ("test09_from_denser", rr.Config(0.5, int_ior=1.0, ext_ior=1.5), (0.2, -0.6, 0.5)),
]
CHI2_THRESHOLD = 1 - (1 - 0.01) ** (1 / len(CHI2_CASES))       # significance 0.01, Sidak-corrected over the eight cases


def chi2_slack(cfg):
    """how far the pdf may be from integrating to what the sampler does: Beckmann's visible normals are drawn from the exact
    distribution of visible normals while the pdf carries the rational fit of G1 (below 0.35 %, microfacet.h:348-352)"""
    return 0.0035 if (cfg.visible and not cfg.ggx) else 0.0
