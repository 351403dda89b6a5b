"""What test_phase.py (CPU) and test_phase_gpu.py share: the configurations of DESIGN.md section 16, their inputs, the float64 reference
with the condition number and branch margin of every quantity, the ratio both files measure and the K table both hold it to.

A quantity q of a lane is compared as |got - want| / (2^-23 cond max(1, |want|)) <= K[q] (the method of DESIGN.md 15.4), cond = 1 + the
summed |dq / dx| over the lane's continuous inputs (central differences of the float64 reference) / max(1, |q|).  K comes from the float32
run of the same reference on the CPU (test_phase.py::test_k_table): 4 x the worst ratio, rounded up to a power of two; the device is then
held to the same K."""
import zlib

import numpy as np

import phase_ref as pr

EPS = pr.EPS
MARGIN = 1e-5                 # lanes closer than this to a branch point are not compared per lane ...
MAX_LEFT_OUT = 0.01           # ... and at most this share of a batch may be
N_LANES = 4096
N_EDGE = 8                    # lanes with s2x = 0, and as many with s2x = 1 - 2^-24 (they sample |cos| = 1, a branch point: they count against the cap)
S1_GAP = 0.02                 # s1 stays this far from a blend's weight: that branch leaves no lane out
QUANTITIES = ("wo", "weight", "pdf", "eval", "eval_pdf")
# test_phase.py::test_k_table measures these and fails when the measurement asks for another value
K = {"wo": 128.0, "weight": 2.0, "pdf": 512.0, "eval": 2.0, "eval_pdf": 2.0}

TAB = {
    "tab2": lambda: pr.tabphase("1,1", "tab2"),
    "tab5": lambda: pr.tabphase("0,0,1,2,0", "tab5"),
    "tabflat": lambda: pr.tabphase("1,1,3,3,2", "tabflat"),
    "tab257": lambda: pr.tabphase(pr.hg_table(0.9, 257), "tab257"),
    "tab1801": lambda: pr.tabphase(pr.hg_table(0.9, 1801), "tab1801"),
}


def configs():
    out = [TAB[k]() for k in ("tab2", "tab5", "tabflat", "tab257", "tab1801")] + [pr.rayleigh()]
    for w in (0.0, 0.3, 1.0):
        out += [pr.blend(w, pr.rayleigh(), pr.hg(0.8)), pr.blend(w, pr.isotropic(), TAB["tab257"]()), pr.blend(w, TAB["tab5"](), TAB["tab257"]())]
    return out


def scene_dict(phase, integrator="volpath"):
    """the smallest scene that carries the phase function: a cube with a null BSDF around a homogeneous medium"""
    return {"type": "scene", "integrator": {"type": integrator},
            "sensor": {"type": "perspective", "film": {"type": "hdrfilm", "width": 4, "height": 4}},
            "box": {"type": "cube", "bsdf": {"type": "null"},
                    "interior": {"type": "homogeneous", "sigma_t": 1.0, "albedo": 0.8, "phase": phase.to_dict()}},
            "sky": {"type": "constant", "radiance": 1.0}}


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def make_inputs(p, n=N_LANES):
    """wi random on the sphere, uniform samples with the edge values of s2x, wo_query random on the sphere; all float32"""
    rng = np.random.default_rng(zlib.crc32(p.label.encode()))
    wi, woq = _unit(rng, n), _unit(rng, n)
    smp = rng.random((n, 3)).astype(np.float32)
    smp[:N_EDGE, 1] = 0.0; smp[N_EDGE:2 * N_EDGE, 1] = np.float32(1 - 2.0 ** -24)
    if p.kind == pr.BLEND:                                      # uniform over [0, 1) without the band around the weight
        w = float(p.weight); lo, hi = max(w - S1_GAP, 0.0), min(w + S1_GAP, 1.0)
        u = rng.random(n) * (1 - (hi - lo))
        s1 = np.where(u < lo, u, u + (hi - lo)).astype(np.float32)
        near = np.abs(s1.astype(np.float64) - w) < S1_GAP        # (the rounding to float32 at the band's edge)
        s1[near] = np.float32(hi + 1e-3 if hi < 0.9 else lo - 1e-3)
        smp[:, 0] = np.minimum(s1, np.float32(1 - 2.0 ** -24))
    return wi, smp, woq


def _fd(f, x, h=1e-6):
    """sum over the columns of x of |d f / d x_j| by central differences; f returns (n,) or (n, k) (the worst component counts)"""
    tot = 0
    for j in range(x.shape[1]):
        e = np.zeros_like(x); e[:, j] = h
        with np.errstate(invalid="ignore", divide="ignore"):
            dq = np.abs(f(x + e) - f(x - e)) / (2 * h)
        dq = np.nan_to_num(dq, nan=0.0, posinf=1e30)
        tot = tot + (dq if dq.ndim == 1 else dq.max(1))
    return tot


def reference(p, wi, smp, woq):
    """the float64 reference at float32 inputs (taken as exact), with cond and the compared-lane masks of every quantity"""
    wi = np.asarray(wi, np.float64); smp = np.asarray(smp, np.float64); woq = np.asarray(woq, np.float64)
    s = pr.sample(p, wi, smp)
    ev, em = pr.eval_pdf(p, wi, woq)
    big = lambda q: np.maximum(1.0, np.abs(q) if np.ndim(q) == 1 else np.abs(q).max(1))
    xs = np.concatenate([wi, smp[:, 1:]], 1)                    # (s1 only chooses the lobe)
    sens = lambda key: _fd(lambda x: pr.sample(p, x[:, :3], np.concatenate([smp[:, :1], x[:, 3:]], 1))[key], xs)
    cond = {k: 1 + sens(k) / big(s[k]) for k in ("wo", "weight", "pdf")}
    xe = np.concatenate([wi, woq], 1)
    cond["eval"] = cond["eval_pdf"] = 1 + _fd(lambda x: pr.eval_pdf(p, x[:, :3], x[:, 3:])[0], xe) / big(ev)
    return {"wo": s["wo"], "weight": s["weight"], "pdf": s["pdf"], "eval": ev, "eval_pdf": ev, "cond": cond,
            "sample_ok": s["margin"] > MARGIN, "eval_ok": em > MARGIN}


def float32_run(p, wi, smp, woq):
    T = np.float32
    s = pr.sample(p, np.asarray(wi, T), np.asarray(smp, T), T)
    ev, _ = pr.eval_pdf(p, np.asarray(wi, T), np.asarray(woq, T), T)
    return {"wo": s["wo"], "weight": s["weight"], "pdf": s["pdf"], "eval": ev, "eval_pdf": ev}


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
    """per quantity: the worst ratio over the compared lanes, and how many lanes are left out"""
    out = {}
    for k in QUANTITIES:
        ok = ref["eval_ok"] if k in ("eval", "eval_pdf") else ref["sample_ok"]
        r = ratio(got[k], ref[k], ref["cond"][k])
        out[k] = (float(r[ok].max()) if ok.any() else 0.0, int((~ok).sum()))
    return out


def k_from(worst):
    """4 x the worst ratio, rounded up to a power of two (at least 1)"""
    return float(2.0 ** max(0, int(np.ceil(np.log2(max(4 * worst, 1e-30))))))
