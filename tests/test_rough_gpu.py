"""The roughdielectric BSDF on the device, held to the float64 reference of tests/rough_ref.py:
(a) lrt_bsdf_probe per lane, (b) erf / erfinv, (c) the sampling tests of the renderer this project follows as chi-square tests of the
probe, (d) weight * pdf = eval on the device, (e) reflection + transmission + MIS through `path`, (f) transmission into a medium
through volpath / volpathmis, (g) the albedo AOV, (h) nothing else moved.  Tolerances: rough_cases.py."""
import math

import numpy as np
import pytest

import rough_cases as rc
import rough_ref as rr

pytestmark = pytest.mark.gpu

CONFIGS = rc.configs()
_cache = {}


def probe_case(mi, cfg, tmp_path=None, bump=False):
    """the probe on the configuration's inputs, and the float64 reference at the device's own wi (float32, taken as exact)"""
    key = (cfg.label(), bump)
    if key not in _cache:
        bsdf = rc.bsdf_xml(cfg)
        if bump:
            png = str(tmp_path / "flat.png"); rc.write_flat_png(png)
            bsdf = f'<bsdf type="bumpmap"><texture name="arbitrary" type="bitmap"><boolean name="raw" value="true"/><string name="filename" value="{png}"/></texture>{bsdf}</bsdf>'
        sc = mi.load_string(rc.scene_xml(bsdf))
        o, d, smp, woq = rc.make_inputs(cfg)
        pr = sc.bsdf_probe(o, d, smp, woq)
        assert (pr["shape"] == 0).all()
        ref = rc.reference(cfg, pr["wi"], smp, woq)
        _cache[key] = (pr, ref, smp, woq)
    return _cache[key]


def as_got(pr):
    w, e = pr["weight"], pr["eval"]
    assert (w[:, 0] == w[:, 1]).all() and (w[:, 0] == w[:, 2]).all() and (e[:, 0] == e[:, 1]).all() and (e[:, 0] == e[:, 2]).all()      # no reflectance texture: grey
    return {"wo": pr["wo"], "pdf": pr["pdf"], "eta": pr["eta"], "weight": w[:, 0], "eval": e[:, 0], "eval_pdf": pr["eval_pdf"]}


def hold(label, pr, ref):
    w = rc.worst_ratios(ref, as_got(pr))
    print(f"[rough a] {label:46s} " + "  ".join(f"{k} {v[0]:6.2f}/{rc.K[k]:g} (-{v[1]})" for k, v in w.items()))
    for k, (r, left) in w.items():
        assert left <= rc.MAX_LEFT_OUT * rc.N_LANES, (label, k, left)
        assert r <= rc.K[k], (label, k, r, rc.K[k])
    ok = ref["sample_ok"]
    assert (pr["type"][ok] == rr.F_SMOOTH).all()
    assert np.allclose(pr["wo_z"][ok], pr["wo"][ok][:, 2], rtol=0, atol=1e-6)            # the shading frame is the world's


# ------------------------------------------------------------------------------------------------------------------ (a), (d)
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: c.label())
def test_probe_against_float64(mi, cfg):
    pr, ref, _, _ = probe_case(mi, cfg)
    hold(cfg.label(), pr, ref)


def test_probe_under_a_bumpmap(mi, tmp_path):
    """nested in a bumpmap whose height map has no slope: the perturbed frame is the shading frame and the terminator term is 1, so the
    nested BSDF's values come back unchanged (the dispatch through bsdf_sample / bsdf_eval / bsdf_pdf's nested branch)"""
    cfg = rr.Config(0.5, 0.2, ggx=True, visible=True)
    pr, ref, _, _ = probe_case(mi, cfg, tmp_path, bump=True)
    hold("bumpmap over " + cfg.label(), pr, ref)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: c.label())
def test_device_identity(mi, cfg):
    """weight * pdf against eval at the sampled wo, all three from the device (the second probe asks for eval at the first one's wo).
    With sample_visible = false the product carries D_scaled(m) / D(m) (test_rough.py::test_sampling_identity_f64), taken from the reference."""
    pr, ref, smp, _ = probe_case(mi, cfg)
    sc = mi.load_string(rc.scene_xml(rc.bsdf_xml(cfg)))
    o, d, _, _ = rc.make_inputs(cfg)
    wo = pr["wo"].astype(np.float32)
    pr2 = sc.bsdf_probe(o, d, smp, wo)
    assert np.array_equal(pr2["pdf"], pr["pdf"]) and np.array_equal(pr2["weight"], pr["weight"])
    s = rr.sample(cfg, pr["wi"].astype(np.float64), smp[:, 0].astype(np.float64), smp[:, 1:].astype(np.float64))
    ev, _, em = rr.eval_pdf(cfg, pr["wi"].astype(np.float64), wo.astype(np.float64))
    # eval is asked at the device's wo, which is itself off by what (a) allows: its derivative against wo counts cond(wo) times
    wi_d, wo_d = pr["wi"].astype(np.float64), wo.astype(np.float64)
    d_wi = rc._fd(lambda x: rr.eval_pdf(cfg, x, wo_d)[0], wi_d); d_wo = rc._fd(lambda x: rr.eval_pdf(cfg, wi_d, x)[0], wo_d)
    cond = ref["cond"]["weight"] + ref["cond"]["pdf"] + 1 + (d_wi + d_wo * ref["cond"]["wo"]) / np.maximum(1.0, ev)
    if not cfg.visible:
        # the factor is taken at the reference's m; the device's m is off by what the tolerance of wo allows, and the factor follows it
        with np.errstate(divide="ignore", invalid="ignore"):
            cond = cond + ref["cond"]["wo"] * np.nan_to_num(rc._fd(lambda m: np.log(rc.scaling_ratio(cfg, pr["wi"], m)), s["m"]), nan=0.0, posinf=1e30)
    valid = ref["sample_ok"] & (em > rc.MARGIN) & (s["weight"] > 0) & (pr["weight"][:, 0] > 0)
    # the factor at the device's own normal: the half vector of its wi and wo (at the clamp alpha float32 cannot tell the sampled
    # normal from the surface normal, roughdielectric's sqrt(1 - cos^2), and the reference's normal is another one)
    wi64, wo64 = pr["wi"].astype(np.float64), wo.astype(np.float64)
    eta = np.where(wi64[:, 2] > 0, float(cfg.eta(np.float64)), 1 / float(cfg.eta(np.float64)))
    h = wi64 + wo64 * np.where(wi64[:, 2] * wo64[:, 2] > 0, 1.0, eta)[:, None]
    m_dev = h / np.linalg.norm(h, axis=1, keepdims=True); m_dev *= np.sign(m_dev[:, 2:3])
    lhs = pr["weight"][:, 0].astype(np.float64) * pr["pdf"].astype(np.float64) * rc.scaling_ratio(cfg, pr["wi"], m_dev)
    r = rc.ratio(lhs, pr2["eval"][:, 0], cond)[valid]
    print(f"[rough d] {cfg.label():46s} weight * pdf against eval: worst ratio {r.max():.2f} over {valid.sum()} lanes")
    assert valid.mean() > 0.5 and r.max() <= max(rc.K["weight"], rc.K["pdf"], rc.K["eval"])       # (a)'s K over the summed cond of the three factors


# ---------------------------------------------------------------------------------------------------------------------- (b)
def test_erf(mi):
    """lrt_math_eval fn 9.  |x| < 1: the odd polynomial of Cephes' single-precision erff (its float64 evaluation is within 1.3e-9 of erf);
    beyond: Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 by the handbook.  Bound: 1.5e-7 + 2 ulp of the value."""
    x = np.concatenate([np.linspace(-4.5, 4.5, 49152), np.linspace(-1, 1, 8192), np.geomspace(1e-6, 1, 4096), -np.geomspace(1e-6, 1, 4096)]).astype(np.float32)
    assert x.size == 65536
    got = mi.math_eval(9, x)[0].astype(np.float64)
    want = np.vectorize(math.erf)(x.astype(np.float64))
    err = np.abs(got - want); bound = 1.5e-7 + 2 * rr.EPS * np.abs(want)
    print(f"[rough b] erf: worst error / bound {np.max(err / bound):.3f}, worst absolute {err.max():.3e}")
    assert (err <= bound).all()
    assert mi.math_eval(9, np.array([np.inf, -np.inf, 0.0], np.float32))[0].tolist() == [1.0, -1.0, 0.0]


def test_erfinv(mi):
    """lrt_math_eval fn 10.  Giles' single-precision polynomial pair ("Approximating the erfinv function", GPU Computing Gems Jade
    edition, 2012); evaluated in float64 its coefficients stay within 1.3e-7 relative of torch.special.erfinv (float64) over (-1, 1).
    Bound: 1.3e-7 + 2 ulp, relative."""
    import torch
    tail = 1 - np.geomspace(1e-7, 0.1, 8192)
    x = np.concatenate([np.linspace(-0.99999, 0.99999, 49152), tail, -tail]).astype(np.float32)
    assert x.size == 65536
    got = mi.math_eval(10, x)[0].astype(np.float64)
    want = torch.special.erfinv(torch.from_numpy(x.astype(np.float64))).numpy()
    err = np.abs(got - want); bound = (1.3e-7 + 2 * rr.EPS) * np.abs(want)
    nz = want != 0
    print(f"[rough b] erfinv: worst error / bound {np.max(err[nz] / bound[nz]):.3f}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------------- (c)
def _probe_dirs(sc, wi, smp, woq):
    """the probe for one wi: rays that arrive along -wi at points of the rectangle"""
    n = len(woq)
    wi32 = np.asarray(wi, np.float32)
    d = np.broadcast_to(-wi32, (n, 3)).copy()
    o = (np.float32([0.3, 0.2, 0.0]) + np.broadcast_to(3 * wi32, (n, 3))).astype(np.float32)     # (off the rectangle's diagonal)
    return sc.bsdf_probe(o, d, smp, woq.astype(np.float32))


@pytest.mark.parametrize("case", rc.CHI2_CASES, ids=lambda c: c[0])
def test_chi2(mi, case):
    """2^20 samples of the probe, three sample dimensions, 64 x 128 cells of (cos theta, phi), expected counts by Simpson quadrature of
    the probe's pdf; accepted at 0.01, Sidak-corrected over the eight cases (test_rough.py runs the same harness on the reference)"""
    name, cfg, wi = case
    sc = mi.load_string(rc.scene_xml(rc.bsdf_xml(cfg)))
    wi = np.asarray(wi, np.float64) / np.linalg.norm(wi)
    n = 1 << 20
    u = np.random.default_rng(2024).random((n, 3), dtype=np.float32)
    pr = _probe_dirs(sc, wi, u, np.broadcast_to(np.float32([0, 0, 1]), (n, 3)))
    assert (pr["shape"] == 0).all()
    zero = ~(pr["pdf"] > 0) | ~(pr["weight"][:, 0] > 0)

    def pdf_of(dirs):
        out = np.empty(len(dirs))
        for a in range(0, len(dirs), 1 << 19):
            blk = dirs[a:a + (1 << 19)]
            out[a:a + len(blk)] = _probe_dirs(sc, wi, np.full((len(blk), 3), 0.5, np.float32), blk)["eval_pdf"]
        return out
    p, stat, dof, mass = rr.chi2_test(pr["wo"], pdf_of, n, p_zero=zero, mass_slack=rc.chi2_slack(cfg))
    print(f"[rough c] {name}: p = {p:.4f}, chi2 = {stat:.1f}, dof = {dof}, mass = {mass:.5f}, zero-density samples {int(zero.sum())}")
    assert p > rc.CHI2_THRESHOLD, (name, p, stat, dof)


# ----------------------------------------------------------------------------------------------------------------- (e), (f)
ANGLES = [20.0, 60.0, 80.0]
SPP, RES = 4096, 4


def view_xml(cfg, angle, integrator, medium="", extra="", tail="", moment=True, spp=SPP):
    """the rectangle scaled by 1e3 under a constant emitter of radiance 1, seen through a 1 degree camera at `angle` from the normal"""
    t = math.radians(angle)
    xml = rc.scene_xml(rc.bsdf_xml(cfg), integrator=f'<integrator type="moment">{integrator}</integrator>' if moment else integrator,
                       scale=1e3, extra=extra, fov=1.0, origin=(5 * math.sin(t), 0.0, 5 * math.cos(t)), spp=spp, res=RES)
    xml = xml.replace("<sensor", medium + "<sensor", 1)
    return xml.replace("</scene>", tail + '<emitter type="constant"><rgb name="radiance" value="1"/></emitter></scene>')


def film_mean(mi, xml):
    sc = mi.load_string(xml)
    img = sc.render()
    var, mean = mi.moment_variance(img, sc, SPP)
    assert np.isfinite(img).all()
    # a grey scene under radiance 1: Y is the radiance.  The film's mean and the standard error of that mean
    return float(mean[..., 1].mean()), float(np.sqrt(var[..., 1].sum()) / (RES * RES))


def cone(angle):
    """the central wi and the four corner directions of the 1 degree field of view (the quadrature's change across the pixel cone)"""
    t = math.radians(angle); h = math.radians(0.5) * math.sqrt(2)
    return [np.array([math.sin(a), 0.0, math.cos(a)]) for a in (t, t - h, t + h)]


_expected = {}


def expected(cfg, angle, weight_t=None, tag=""):
    key = (cfg.label(), angle, tag)
    if key not in _expected:
        _expected[key] = _expected_uncached(cfg, angle, weight_t)
    return _expected[key]


def _expected_uncached(cfg, angle, weight_t=None):
    vals = []
    for wi in cone(angle):
        r, tr = rr.lobe_integrals(cfg, wi, weight_t=weight_t, n_theta=2048, n_phi=512)
        vals.append((r, tr))
    centre = sum(vals[0])
    spread = max(abs(sum(v) - centre) for v in vals[1:])
    return centre, spread, vals[0]


@pytest.mark.parametrize("ggx", [False, True], ids=["beckmann", "ggx"])
def test_path_reflection_transmission_mis(mi, ggx):
    """Under a constant environment of radiance 1 the pixel is the integral of eval over the whole sphere: the reflected and the
    transmitted lobe, each met by BSDF sampling and by emitter sampling through bsdf_eval / bsdf_pdf on either side, MIS-weighted"""
    cfg = rr.Config(0.1, ggx=ggx)
    for angle in ANGLES:
        want, spread, (r, t) = expected(cfg, angle)
        got, se = film_mean(mi, view_xml(cfg, angle, '<integrator type="path" name="img"><integer name="max_depth" value="2"/></integrator>'))
        print(f"[rough e] {cfg.label()} at {angle:g} deg: film {got:.5f} +- {se:.5f}, quadrature {want:.5f} (R {r:.5f}, T {t:.5f}), change across the cone {spread:.2e}")
        assert abs(got - want) <= 4.5 * se + spread, (angle, got, want, se, spread)
        assert se < 0.01 * want                                           # the interval is narrow enough to tell a lobe missing (T > 0.3 here)


SLAB = '<medium type="homogeneous" id="slab"><rgb name="albedo" value="0"/><rgb name="sigma_t" value="1"/></medium>'
INSIDE = '<ref name="interior" id="slab"/>'
NULL_PLANE = ('<shape type="rectangle"><transform name="to_world"><scale value="1e3"/><translate z="-1"/></transform><bsdf type="null"/>'
              '<ref name="exterior" id="slab"/></shape>')


@pytest.mark.parametrize("integrator", ["volpath", "volpathmis"])
@pytest.mark.parametrize("ggx", [False, True], ids=["beckmann", "ggx"])
def test_transmission_into_a_medium(mi, integrator, ggx):
    """An absorbing slab of optical thickness 1 below the rough interface, left through a null plane: R(wi) + the transmitted lobe
    attenuated by exp(-1 / |cos theta_o|).  A sampled smooth transmission must enter the medium (target_medium after a non-delta
    direction), and the emitter sample through the transmitted side must be weighted once."""
    cfg = rr.Config(0.1, ggx=ggx)
    att = lambda d: np.exp(-1.0 / np.maximum(np.abs(d[:, 2]), 1e-300))
    for angle in ANGLES:
        want, spread, (r, t) = expected(cfg, angle, weight_t=att, tag="slab")
        # what could leave through the rectangles' edges (half width 1e3 against a depth of 1): directions with |cos theta_o| < 2e-3
        leak = rr.lobe_integrals(cfg, cone(angle)[0], weight_t=lambda d: att(d) * (np.abs(d[:, 2]) < 2e-3), n_theta=2048, n_phi=512)[1]
        got, se = film_mean(mi, view_xml(cfg, angle, f'<integrator type="{integrator}" name="img"><integer name="max_depth" value="6"/></integrator>', medium=SLAB, extra=INSIDE, tail=NULL_PLANE))
        print(f"[rough f] {integrator} {cfg.label()} at {angle:g} deg: film {got:.5f} +- {se:.5f}, quadrature {want:.5f} (R {r:.5f}, attenuated T {t:.5f}), cone {spread:.2e}, edge leak < {leak:.1e}")
        assert leak < 0.01 * se
        assert abs(got - want) <= 4.5 * se + spread, (integrator, angle, got, want, se, spread)
        assert abs(got - expected(cfg, angle)[0]) > 9 * se or angle == 80.0   # ... and differs from the scene without the medium


# ---------------------------------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("ggx", [False, True], ids=["beckmann", "ggx"])
def test_aov_albedo(mi, ggx):
    """albedo = eval(si, wo = +z) pi of the BSDF base class, per lane: wi of a lane is rebuilt from its position AOV"""
    cfg = rr.Config(0.5, ggx=ggx)
    angle = 20.0
    xml = view_xml(cfg, angle, '<integrator type="aov"><string name="aovs" value="al:albedo,pp:position"/></integrator>', moment=False)
    sc = mi.load_string(xml)
    n = RES * RES * SPP
    lanes = sc.render_aov_samples(0, n).astype(np.float64)
    t = math.radians(angle); origin = np.array([5 * math.sin(t), 0.0, 5 * math.cos(t)])
    wi = origin - lanes[:, 3:6]; wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    up = np.broadcast_to(np.array([0.0, 0.0, 1.0]), wi.shape)
    want = math.pi * rr.eval_pdf(cfg, wi, up)[0]
    cond = 1 + rc._fd(lambda x: math.pi * rr.eval_pdf(cfg, x, up)[0], wi) / np.maximum(1.0, want)
    assert (lanes[:, 0] == lanes[:, 1]).all() and (lanes[:, 0] == lanes[:, 2]).all() and want.min() > 0.01
    hit = (lanes[:, 3:6] != 0).any(1)                      # (the camera looks at the rectangle's centre, on the diagonal its two triangles share: a ray may slip between them)
    assert (~hit).mean() < 1e-3 and (lanes[~hit, :3] == 0).all()
    # (a)'s tolerance, K 2^-23 cond, plus what rebuilding wi costs: the position is o + t d, two terms of size 5 each rounded at 2^-24 of
    # it, seen from 5 away: 2^-23 in each component of wi, times the derivative of the albedo against that component
    d_wi = rc._fd(lambda x: math.pi * rr.eval_pdf(cfg, x, up)[0], wi)
    allowed = rc.EPS * (rc.K["eval"] * cond * np.maximum(1.0, want) + d_wi)
    r = np.where(hit, np.abs(lanes[:, 0] - want) / allowed, 0.0)
    print(f"[rough g] {cfg.label()}: albedo per lane, worst error / allowed {r.max():.2f}; values {want.min():.4f} .. {want.max():.4f}")
    assert r.max() <= 1.0
    img = sc.render()
    assert np.allclose(img[..., :3].mean(), want[hit].mean(), rtol=2e-3)


# ---------------------------------------------------------------------------------------------------------------------- (h)
def test_unused_rough_bsdf_changes_nothing(mi):
    """A roughdielectric that no shape references leaves the scene on the kernels it ran before (scene_prep.cpp): bit-identical film"""
    base = mi.cornell_box()
    d = dict(base); d["spare"] = {"type": "roughdielectric", "alpha": 0.2}
    a = mi.load_dict(base); b = mi.load_dict(d)
    assert b.desc.n_bsdfs == a.desc.n_bsdfs + 1
    n = 256 * 256 * 4
    la, lb = a.render_samples(0, n, spp=4, seed=3), b.render_samples(0, n, spp=4, seed=3)          # (the film is summed by atomics: lanes are the bit-exact view)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)) and la[:, :3].max() > 0
    assert a.stats()["record_bytes"] == b.stats()["record_bytes"]


LIVER = ('<medium type="liver" id="slab">' + "".join(f'<float name="sigma_{k}{l}_{c}" value="{v:.4f}"/>' for k, base in (("collagen", 0.9), ("elastin", 0.5))
                                                      for l in range(1, 5) for c, v in zip("RGB", (base * l, base * l * 0.6 + 0.1, base * (5 - l) * 0.4)))
         + '<float name="layer1Limit" value="0.1"/><float name="layer2Limit" value="0.2"/><float name="layer3Limit" value="0.35"/><float name="layer4Limit" value="0.6"/>'
         '<rgb name="sigma_blood" value="0.3, 0.9, 1.1"/><rgb name="sigma_bile" value="0.02, 0.0, 0.3"/><rgb name="sigma_lipid_water" value="0.05, 0.01, 0.2"/>'
         '<float name="sigma_hepatocity" value="9.5"/><boolean name="has_spectral_extinction" value="false"/><rgb name="sigma_t" value="0.4, 0.2, 0.6"/>'
         '<phase type="hg"><float name="g" value="0.4"/></phase></medium>')


@pytest.mark.parametrize("integrator", ["biovolpath", "biovolpath06"])
def test_bio_integrators_render_the_rough_interface(mi, integrator):
    """the scene of (f) with a liver medium in the slab: the bio instances run the rough interface without error, finite output.
    (Without spectral extinction: with it an emitter sample's shadow ray divides the slab's transmittance by that of the path's channel,
    biovolpath.cpp's ratio estimator, which overflows over the hundreds of units a grazing ray stays inside a slab 1e3 wide, for a
    smooth dielectric interface too.  biovolpath06 collects emission along delta chains only: under an environment alone it renders
    a non-delta interface black, as the reference does.)"""
    cfg = rr.Config(0.1, ggx=True)
    xml = view_xml(cfg, 60.0, f'<integrator type="{integrator}"><integer name="max_depth" value="8"/></integrator>', medium=LIVER, extra=INSIDE, tail=NULL_PLANE,
                   moment=False, spp=64)
    sc = mi.load_string(xml)
    img = sc.render()
    assert img.shape[:2] == (RES, RES) and np.isfinite(img).all() and (img[..., :3] >= 0).all()


def test_prbvolpath_override_is_refused_at_render_time(mi):
    sc = mi.load_string(rc.scene_xml(rc.bsdf_xml(rr.Config(0.1))))
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath on a scene with .*roughdielectric"):
        sc.render(integrator="prbvolpath")
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath on a scene with .*roughdielectric"):
        sc.render_backward(np.ones(sc.film_shape(), np.float32), integrator="prbvolpath")
