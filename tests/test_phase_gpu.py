"""Tabulated, Rayleigh and blended phase functions on the device, held to the float64 reference of
tests/phase_ref.py: (a) lrt_phase_probe per lane, (b) cbrt, (c) weight * pdf = eval on the device, (d) chi-square tests of the probe's
directions, (e) an unreferenced medium moves nothing, (f) furnace renders, (g) one integrand through two phase functions, (h) a blend of
weight 0 against its first child, (i) prbvolpath refused at render time.  Tolerances: phase_cases.py (the K table of test_phase.py::test_k_table)."""
import numpy as np
import pytest

import phase_cases as pc
import phase_ref as pr
import rough_ref as rr

pytestmark = pytest.mark.gpu

CONFIGS = pc.configs()
_cache = {}


def probe_case(mi, p):
    if p.label not in _cache:
        sc = mi.load_dict(pc.scene_dict(p))
        wi, smp, woq = pc.make_inputs(p)
        got = sc.phase_probe(0, wi, smp, woq)
        _cache[p.label] = (sc, got, pc.reference(p, wi, smp, woq), wi, smp, woq)
    return _cache[p.label]


# ---------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("p", CONFIGS, ids=lambda p: p.label)
def test_probe_against_float64(mi, p):
    _, got, ref, _, _, _ = probe_case(mi, p)
    w = pc.worst_ratios(ref, got)
    print(f"[phase a] {p.label:28s} " + "  ".join(f"{k} {v[0]:7.2f}/{pc.K[k]:g} (-{v[1]})" for k, v in w.items()))
    for k, (r, left) in w.items():
        assert left <= pc.MAX_LEFT_OUT * pc.N_LANES, (p.label, k, left)
        assert r <= pc.K[k], (p.label, k, r, pc.K[k])
    assert np.array_equal(got["eval"], got["eval_pdf"])
    # every lane, the ones left out above included (the edge samples s2x = 0 and 1 - 2^-24 land on |cos| = 1): finite, a unit direction, a density
    wo = got["wo"].astype(np.float64)
    assert np.isfinite(wo).all() and np.isfinite(got["pdf"]).all() and np.isfinite(got["weight"]).all() and np.isfinite(got["eval"]).all()
    # (the length of wi, the frame's two vectors, the local vector and the three fmas of to_world: a few roundings of 2^-24 each, 16 x 2^-23 in all)
    assert np.abs(np.linalg.norm(wo, axis=1) - 1).max() <= 16 * pc.EPS
    assert (got["pdf"] >= 0).all() and (got["eval"] >= 0).all() and ((got["weight"] == 0) | (np.abs(got["weight"] - 1) <= 2 * pc.EPS)).all()


# ---------------------------------------------------------------------------------------------------------------------- (b)
def test_cbrt(mi):
    """lrt_math_eval fn 11: exp(log|x| / 3) and one Newton step whose residual y^2 * y - |x| is one fma.  With y^2 rounded (2^-24
    relative) the step's own error is at most a third of an ulp, the division and the subtraction round once more each: 1 ulp
    (2^-23 relative) is the documented error; the bound here is that plus 2 ulp."""
    x = np.concatenate([np.geomspace(1e-30, 1e30, 24576), -np.geomspace(1e-30, 1e30, 24576), np.linspace(-4.25, 4.25, 16384)]).astype(np.float32)
    assert x.size == 65536
    got = mi.math_eval(11, x)[0].astype(np.float64)
    want = np.cbrt(x.astype(np.float64))
    err = np.abs(got - want); bound = 3 * pr.EPS * np.abs(want)
    nz = want != 0
    print(f"[phase b] cbrt: worst error {np.max(err[nz] / (pr.EPS * np.abs(want[nz]))):.3f} ulp (2^-23 relative)")
    assert (err <= bound).all()
    sp = mi.math_eval(11, np.array([0.0, -0.0, np.inf, -np.inf, 8.0, -27.0], np.float32))[0]
    assert sp.tolist() == [0.0, 0.0, np.inf, -np.inf, 2.0, -3.0] and np.signbit(sp[1])


# ---------------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("p", CONFIGS, ids=lambda p: p.label)
def test_device_identity(mi, p):
    """weight * pdf against eval at the sampled wo, all three from the device (a second probe asks for eval at the first one's wo).
    The bound, in units of 2^-23 cond max(1, eval) with cond eval's sensitivity to (wi, wo): the sampler's pdf is eval's own arithmetic
    at the sampled cosine and the second probe's eval the same arithmetic at the cosine it takes again from the float32 wo, each within
    K_eval of the float64 value at its cosine; the two cosines differ by the rounding of wo and of the dot product, 1 unit of cond;
    the weight is within K_weight of 1.  K_weight + 2 K_eval + 1 = 7."""
    sc, got, ref, wi, smp, _ = probe_case(mi, p)
    wo = np.ascontiguousarray(got["wo"], np.float32)
    again = sc.phase_probe(0, wi, smp, wo)
    assert np.array_equal(again["pdf"], got["pdf"]) and np.array_equal(again["weight"], got["weight"])
    wi64, wo64 = wi.astype(np.float64), wo.astype(np.float64)
    ev, em = pr.eval_pdf(p, wi64, wo64)
    d = pc._fd(lambda x: pr.eval_pdf(p, x[:, :3], x[:, 3:])[0], np.concatenate([wi64, wo64], 1))
    cond = 1 + d / np.maximum(1.0, ev)
    ok = ref["sample_ok"] & (em > pc.MARGIN)
    lhs = got["weight"].astype(np.float64) * got["pdf"].astype(np.float64)
    bound = pc.K["weight"] + 2 * pc.K["eval"] + 1
    r = pc.ratio(lhs, again["eval"], cond)[ok]
    print(f"[phase c] {p.label:28s} weight * pdf against eval: worst ratio {r.max():.3f} of {bound:g} over {ok.sum()} lanes")
    assert ok.mean() > 0.98 and r.max() <= bound


# ---------------------------------------------------------------------------------------------------------------------- (d)
CHI2 = [c for c in CONFIGS if c.label in ("tab257", "blend0.3(rayleigh,hg0.8)")]
CHI2_THRESHOLD = 1 - (1 - 0.01) ** (1 / len(CHI2))            # significance 0.01, Sidak-corrected over the cases


@pytest.mark.parametrize("p", CHI2, ids=lambda p: p.label)
def test_chi2_of_the_probe(mi, p):
    n = 200000
    rng = np.random.default_rng(11)
    wi = np.broadcast_to(np.array([0.36, -0.48, 0.8], np.float32), (n, 3)).copy()
    smp = rng.random((n, 3)).astype(np.float32)
    got = probe_case(mi, p)[0].phase_probe(0, wi, smp, wi)
    wi0 = wi[0].astype(np.float64)
    pv, stat, dof, mass = rr.chi2_test(got["wo"], lambda d: pr.eval_pdf(p, np.broadcast_to(wi0, d.shape), d)[0], n, res=(32, 64))
    print(f"[phase d] {p.label:28s} p = {pv:.4f}  chi2 = {stat:.1f}  dof = {dof}  mass = {mass:.6f}")
    assert pv > CHI2_THRESHOLD


# ------------------------------------------------------------------------------------------------------------------ renders
def cube_scene(mi, phase, integrator, *, albedo, size, spp, max_depth, rr_depth=None, light="sky", medium="homogeneous", moment=True, extra=None):
    """a cube of side 2 with a null BSDF around a medium of sigma_t = 1 (optical thickness 2), seen from outside"""
    T = mi.ScalarTransform4f
    integ = {"type": integrator, "max_depth": max_depth}
    if rr_depth is not None:
        integ["rr_depth"] = rr_depth
    d = {"type": "scene", "integrator": {"type": "moment", "img": integ} if moment else integ,
         "sensor": {"type": "perspective", "fov": 20.0, "to_world": T().look_at([0, 0, 6], [0, 0, 0], [0, 1, 0]),
                    "sampler": {"type": "independent", "sample_count": spp},
                    "film": {"type": "hdrfilm", "width": size, "height": size, "rfilter": {"type": "box"}}},
         "box": {"type": "cube", "bsdf": {"type": "null"},
                 "interior": {"type": medium, "sigma_t": 1.0, "albedo": albedo, "phase": phase if isinstance(phase, dict) else phase.to_dict()}}}
    if light in ("sky", "lamp+sky"):
        d["sky"] = {"type": "constant", "radiance": 1.0 if light == "sky" else 0.25}
    if light in ("lamp", "lamp+sky"):                           # a small area light above the cube, facing down
        d["lamp"] = {"type": "rectangle", "to_world": T().translate([0.0, 2.5, 0.0]).rotate([1, 0, 0], 90).scale(0.5),
                     "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": 0.0}}, "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 20.0}}}
    if extra:
        d.update(extra)
    return mi.load_dict(d)


def y_mean_var(mi, sc, spp, seed):
    img = sc.render(seed=seed)
    assert np.isfinite(img).all()
    var, mean = mi.moment_variance(img, sc, spp)
    return mean[..., 1], var[..., 1]


# ---------------------------------------------------------------------------------------------------------------------- (e)
def test_unreferenced_medium_changes_nothing(mi):
    spare = {"spare": {"type": "homogeneous", "phase": pc.TAB["tab257"]().to_dict()}}
    kw = dict(albedo=0.8, size=16, spp=16, max_depth=8, moment=False)
    a = cube_scene(mi, pr.hg(0.5), "volpath", **kw); b = cube_scene(mi, pr.hg(0.5), "volpath", extra=spare, **kw)
    assert b.desc.n_phases == 1 and b.desc.n_media == 2
    ia, ib = a.render(seed=3), b.render(seed=3)
    assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
    # (lrt_render_stats carries no kernel name: the record layout, the BVH's residence and the trip and record counts stand in for it; they
    #  differ between the plain and the EXT instances, as the last line shows)
    sa, sb = a.stats(), b.stats()
    assert (sa["record_bytes"], sa["lds_resident"], sa["n_iter"], sa["n_records"]) == (sb["record_bytes"], sb["lds_resident"], sb["n_iter"], sb["n_records"])
    # ... and a referenced one takes the EXT route's wide records
    c = cube_scene(mi, pc.TAB["tab257"](), "volpath", **kw)
    assert np.isfinite(c.render(seed=3)).all() and c.stats()["record_bytes"] >= 88


# ---------------------------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("integrator", ["volpath", "volpathmis"])
@pytest.mark.parametrize("which", ["tab257", "blend0.3(rayleigh,hg0.8)"])
def test_furnace(mi, integrator, which):
    """albedo 1 under a constant environment of radiance 1: every pixel's Y is 1 in expectation (paths that reach max_depth = 256 at
    optical thickness 2 carry less than 1e-30 of the energy).  mi.z_test of the Y mean against 1 (variance 0) at alpha 0.01,
    Sidak-corrected; at least 99.75 % of the pixels pass (the reference's acceptance, test_renders.py)."""
    p = [c for c in CONFIGS if c.label == which][0]
    spp = 256
    sc = cube_scene(mi, p, integrator, albedo=1.0, size=16, spp=spp, max_depth=256, rr_depth=257)
    mean, var = y_mean_var(mi, sc, spp, seed=5)
    pvals, frac = mi.z_test(mean, var, np.ones_like(mean), np.zeros_like(var))
    print(f"[phase f] {integrator:10s} {which:26s} pass {frac:.4f}  min p {pvals.min():.3g}  mean of Y {mean.mean():.6f}")
    assert frac >= 0.9975


# ---------------------------------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("integrator, medium", [("volpath", "homogeneous"), ("biovolpath", "liver")])
def test_tabulated_hg_renders_what_hg_renders(mi, integrator, medium):
    """the same integrand through two estimators: hg g = 0.5 on the plain instance, and the same lobe tabulated at n = 1025 on the EXT
    instance (interpolation error below 3e-5 of the lobe's peak, far below the noise), different seeds.  The bio integrator samples no
    emitter from inside its medium, so its scene adds a dim sky to the lamp: the paths that leave the cube find light."""
    spp = 1024
    kw = dict(albedo=0.8, size=32, spp=spp, max_depth=16, light="lamp" if medium == "homogeneous" else "lamp+sky", medium=medium)
    a = cube_scene(mi, pr.hg(0.5), integrator, **kw)
    b = cube_scene(mi, pr.tabphase(pr.hg_table(0.5, 1025)), integrator, **kw)
    ma, va = y_mean_var(mi, a, spp, seed=1); mb, vb = y_mean_var(mi, b, spp, seed=2)
    pvals, frac = mi.z_test(ma, va, mb, vb)
    print(f"[phase g] {integrator:10s} pass {frac:.4f}  min p {pvals.min():.3g}  mean of Y {ma.mean():.5f} / {mb.mean():.5f}  lit pixels {(ma > 0).mean():.2f}")
    assert (ma > 0).mean() > 0.2 and frac >= 0.9975
    assert a.stats()["record_bytes"] != 0 and b.desc.n_phases == 1


# ---------------------------------------------------------------------------------------------------------------------- (h)
def test_zero_weight_blend_is_its_first_child(mi):
    """blendphase(weight 0, hg g, rayleigh) against plain hg g, same seed: s1 > 0 takes child 0 with the lane's own (s2x, s2y), so the paths
    are the same and each scattering weight is pdf * rcp(pdf), 1 up to a rounding: every pixel agrees within max_depth * 2^-22 relative.
    The exception: a lane that draws s1 == 0 (probability 2^-32 per scattering event) takes the source's `s1 <= weight` branch and
    samples child 1; at most one pixel of the 256 may differ for it."""
    kw = dict(albedo=0.8, size=16, spp=16, max_depth=8, moment=False)
    a = cube_scene(mi, pr.hg(0.6), "volpath", **kw).render(seed=9)
    b = cube_scene(mi, pr.blend(0.0, pr.hg(0.6), pr.rayleigh()), "volpath", **kw).render(seed=9)
    rel = np.abs(a.astype(np.float64) - b) / np.maximum(np.abs(a), 1e-30)
    rel = np.where(a == b, 0.0, rel).max(-1)
    off = rel > 8 * 2.0 ** -22
    print(f"[phase h] worst relative difference {rel.max():.3g} (bound {8 * 2.0 ** -22:.3g}), pixels beyond it {off.sum()}")
    assert off.sum() <= 1


# ---------------------------------------------------------------------------------------------------------------------- (i)
def test_prbvolpath_override_is_refused_at_render_time(mi):
    sc = mi.load_dict(pc.scene_dict(pr.rayleigh()))
    for call in (lambda: sc.render(integrator="prbvolpath"), lambda: sc.render_backward(np.ones(sc.film_shape(), np.float32), integrator="prbvolpath")):
        with pytest.raises(RuntimeError, match="unsupported: prbvolpath on a scene with .*tabulated / Rayleigh / blended phase function"):
            call()
