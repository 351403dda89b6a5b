"""The roughdielectric BSDF on the host: what the loader reads and refuses, the description's new fields, the
dictionary route, and the float64 reference of tests/rough_ref.py held against itself, so that the device checks of
test_rough_gpu.py are known to be passable: the K of every tolerance (float32 against float64 on the CPU), the sampling identity, the
normalisation of the pdf and the chi-square harness fed with the reference's own sampler."""
import ctypes as C

import numpy as np
import pytest

import rough_cases as rc
import rough_ref as rr

BSDF_ROUGH = 4


def scene(mi, bsdf, **kw):
    return mi.load_string(rc.scene_xml(bsdf, **kw))


def rough_desc(sc):
    d = sc.desc
    return [d.bsdfs[i] for i in range(d.n_bsdfs) if d.bsdfs[i].type == BSDF_ROUGH]


def test_version_and_defaults(mi):
    assert mi._lib.lib().lrt_version() >= 114
    sc = scene(mi, '<bsdf type="roughdielectric"/>')
    (B,) = rough_desc(sc)
    assert B.alpha_u == np.float32(0.1) and B.alpha_v == np.float32(0.1) and B.distribution == 0 and B.sample_visible == 1
    assert B.specular_reflectance == -1 and B.specular_transmittance == -1
    assert B.eta == np.float32(1.5046) / np.float32(1.000277)                  # bk7 / air


def test_properties(mi):
    sc = scene(mi, '<bsdf type="roughdielectric"><float name="alpha_u" value="0.5"/><float name="alpha_v" value="0.2"/><string name="distribution" value="GGX"/>'
                   '<boolean name="sample_visible" value="false"/><string name="int_ior" value="water"/><float name="ext_ior" value="1.5"/>'
                   '<rgb name="specular_reflectance" value="0.5, 0.25, 1"/>'
                   '<texture name="specular_transmittance" type="checkerboard"><rgb name="color0" value="0.1"/><rgb name="color1" value="0.9"/></texture></bsdf>')
    (B,) = rough_desc(sc)
    assert (B.alpha_u, B.alpha_v, B.distribution, B.sample_visible) == (0.5, np.float32(0.2), 1, 0)
    assert B.eta == np.float32(1.3330) / np.float32(1.5)
    d = sc.desc
    tr, tt = d.textures[B.specular_reflectance], d.textures[B.specular_transmittance]
    assert list(tr.color0) == [0.5, 0.25, 1.0] and tt.type == 1 and tt.color0[0] == np.float32(0.1) and tt.color1[0] == np.float32(0.9)
    # an alpha below the clamp is kept in the description; the device table holds max(alpha, 1e-4) (scene_prep.cpp)
    (B,) = rough_desc(scene(mi, '<bsdf type="roughdielectric"><float name="alpha" value="1e-6"/></bsdf>'))
    assert B.alpha_u == np.float32(1e-6)


@pytest.mark.parametrize("body, message", [
    ('<float name="alpha" value="0.1"/><float name="alpha_u" value="0.1"/><float name="alpha_v" value="0.1"/>', "please specify"),
    ('<float name="alpha_u" value="0.1"/>', "both 'alpha_u' and 'alpha_v' must be specified"),
    ('<float name="alpha_v" value="0.1"/>', "both 'alpha_u' and 'alpha_v' must be specified"),
    ('<string name="distribution" value="phong"/>', 'Specified an invalid distribution "phong"'),
    ('<float name="int_ior" value="1.5"/><float name="ext_ior" value="1.5"/>', "must be positive and differ"),
    ('<string name="int_ior" value="kryptonite"/>', "unknown material"),
    ('<texture name="alpha" type="checkerboard"/>', 'unsupported: a texture as roughdielectric "alpha"'),
    ('<texture name="alpha_u" type="checkerboard"/><float name="alpha_v" value="0.1"/>', 'unsupported: a texture as roughdielectric "alpha_u"'),
])
def test_loader_errors(mi, body, message):
    with pytest.raises(RuntimeError, match=message):
        scene(mi, f'<bsdf type="roughdielectric">{body}</bsdf>')


def test_textured_alpha_is_unsupported_status(mi):
    L = mi._lib.lib()
    h = C.c_void_p()
    xml = rc.scene_xml('<bsdf type="roughdielectric"><texture name="alpha" type="checkerboard"/></bsdf>').encode()
    assert L.lrt_scene_load_xml_string(xml, b".", None, 0, C.byref(h)) == mi._lib.UNSUPPORTED
    assert b'"alpha"' in L.lrt_last_error()


def test_bitmap_reflectance_refused(mi, tmp_path):
    png = str(tmp_path / "flat.png"); rc.write_flat_png(png)
    for name in ("specular_reflectance", "specular_transmittance"):
        with pytest.raises(RuntimeError, match=f"bitmap texture as roughdielectric {name}"):
            scene(mi, f'<bsdf type="roughdielectric"><texture name="{name}" type="bitmap"><string name="filename" value="{png}"/></texture></bsdf>')


@pytest.mark.parametrize("plugin", ["roughconductor", "roughplastic"])
def test_other_rough_plugins_stay_unsupported(mi, plugin):
    with pytest.raises(RuntimeError, match=f'unsupported bsdf type "{plugin}"'):
        scene(mi, f'<bsdf type="{plugin}"/>')


def test_bumpmap_nesting(mi, tmp_path):
    png = str(tmp_path / "flat.png"); rc.write_flat_png(png)
    sc = scene(mi, f'<bsdf type="bumpmap"><texture name="arbitrary" type="bitmap"><boolean name="raw" value="true"/><string name="filename" value="{png}"/></texture>'
                   '<bsdf type="roughdielectric"><float name="alpha" value="0.3"/></bsdf></bsdf>')
    d = sc.desc
    (bump,) = [d.bsdfs[i] for i in range(d.n_bsdfs) if d.bsdfs[i].type == 2]
    assert d.bsdfs[bump.nested].type == BSDF_ROUGH and d.bsdfs[bump.nested].alpha_u == np.float32(0.3)
    assert d.bsdfs[d.shapes[0].bsdf].type == 2


def test_load_dict_round_trip(mi):
    T = mi.ScalarTransform4f
    d = {"type": "scene", "integrator": {"type": "volpath", "max_depth": 4},
         "sensor": {"type": "perspective", "fov": 30.0, "to_world": T().look_at([0, 0, 5], [0, 0, 0], [0, 1, 0]),
                    "film": {"type": "hdrfilm", "width": 8, "height": 8}},
         "wet": {"type": "rectangle",
                 "bsdf": {"type": "roughdielectric", "alpha_u": 0.25, "alpha_v": 0.125, "distribution": "ggx", "sample_visible": False,
                          "int_ior": "water", "ext_ior": 1.0, "specular_reflectance": {"type": "rgb", "value": [0.5, 0.75, 1.0]},
                          "specular_transmittance": {"type": "checkerboard", "color0": [0.25, 0.25, 0.25], "color1": [1.0, 1.0, 1.0]}},
                 "interior": {"type": "homogeneous", "albedo": {"type": "rgb", "value": 0.5}, "sigma_t": {"type": "rgb", "value": 1.0}}},
         "light": {"type": "constant", "radiance": {"type": "rgb", "value": 1.0}}}
    xml = mi.dict_to_xml(d)
    assert '<bsdf type="roughdielectric">' in xml and '<boolean name="sample_visible" value="false"/>' in xml
    assert '<texture type="checkerboard" name="specular_transmittance">' in xml
    sc = mi.load_dict(d)
    (B,) = rough_desc(sc)
    assert (B.alpha_u, B.alpha_v, B.distribution, B.sample_visible) == (0.25, 0.125, 1, 0) and B.eta == np.float32(1.3330)
    dd = sc.desc
    assert list(dd.textures[B.specular_reflectance].color0) == [0.5, 0.75, 1.0] and dd.textures[B.specular_transmittance].type == 1
    assert dd.shapes[0].interior_medium == 0 and dd.bsdfs[dd.shapes[0].bsdf].type == BSDF_ROUGH
    same = mi.load_string(xml)
    (B2,) = rough_desc(same)
    assert all(getattr(B, f) == getattr(B2, f) for f, _ in mi._lib.BsdfDesc._fields_)


def test_prbvolpath_is_refused(mi):
    bsdf = '<bsdf type="roughdielectric"/>'
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath on a scene with a roughdielectric"):
        scene(mi, bsdf, integrator='<integrator type="prbvolpath"/>')
    xml = rc.scene_xml(bsdf, integrator='<integrator type="$integrator"/>')
    assert mi.load_string(xml, integrator="volpath").desc.n_bsdfs == 1
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath on a scene with a roughdielectric"):
        mi.load_string(xml, integrator="prbvolpath")                       # ... and as an override of the file's parameter
    # an unreferenced roughdielectric changes nothing (scene_prep.cpp: only a shape's BSDF routes a scene to the EXT instances)
    spare = rc.scene_xml('<bsdf type="diffuse"/>', integrator='<integrator type="prbvolpath"/>').replace("<sensor", '<bsdf type="roughdielectric" id="spare"/><sensor', 1)
    assert len(rough_desc(mi.load_string(spare))) == 1


def test_scene_from_desc_validation(mi):
    from liverrenderer_amd import _lib
    base = scene(mi, '<bsdf type="roughdielectric"><rgb name="specular_reflectance" value="0.5"/></bsdf>')
    L = _lib.lib()

    def attempt(mutate):
        d = _lib.SceneDesc.from_buffer_copy(base.desc)
        bs = (_lib.BsdfDesc * d.n_bsdfs)(*[d.bsdfs[i] for i in range(d.n_bsdfs)])
        d.bsdfs = C.cast(bs, C.POINTER(_lib.BsdfDesc))
        mutate(bs[0])
        h = C.c_void_p()
        st = L.lrt_scene_from_desc(C.byref(d), C.byref(h))
        if st == 0:
            L.lrt_scene_free(h)
        return st, L.lrt_last_error().decode()

    assert attempt(lambda b: None)[0] == 0
    assert attempt(lambda b: setattr(b, "alpha_u", 0.0))[0] == 0               # raised to the clamp, not an error
    for name, fn in {"type": lambda b: setattr(b, "type", 5), "eta": lambda b: setattr(b, "eta", 1.0), "eta sign": lambda b: setattr(b, "eta", -1.5),
                     "alpha": lambda b: setattr(b, "alpha_u", -0.1), "alpha nan": lambda b: setattr(b, "alpha_v", float("nan")),
                     "distribution": lambda b: setattr(b, "distribution", 2), "texture": lambda b: setattr(b, "specular_reflectance", 7),
                     "texture low": lambda b: setattr(b, "specular_transmittance", -2)}.items():
        st, msg = attempt(fn)
        assert st != 0 and msg, name


# ------------------------------------------------------------------------------------------- the reference against itself
CONFIGS = rc.configs()


@pytest.fixture(scope="module")
def k_rows():
    """float32 run against float64 run of rough_ref.py per configuration: the table behind K"""
    rows = []
    for cfg in CONFIGS:
        o, d, smp, woq = rc.make_inputs(cfg)
        wi = -d
        ref = rc.reference(cfg, wi, smp, woq)
        s32 = rr.sample(cfg, wi, smp[:, 0], smp[:, 1:], np.float32)
        e32, p32, _ = rr.eval_pdf(cfg, wi, woq, np.float32)
        got = {"wo": s32["wo"], "pdf": s32["pdf"], "eta": s32["eta"], "weight": s32["weight"], "eval": e32, "eval_pdf": p32}
        rows.append((cfg, ref, rc.worst_ratios(ref, got)))
    return rows


def test_k_table(k_rows):
    """K is at least 4 times the worst float32-against-float64 ratio, and the lanes left out stay under the cap, in every configuration"""
    worst = {}
    for cfg, ref, w in k_rows:
        print(f"[rough K] {cfg.label():44s} " + "  ".join(f"{k} {v[0]:6.2f} (-{v[1]})" for k, v in w.items()))
        for k, (r, left) in w.items():
            worst[k] = max(worst.get(k, 0.0), r)
            assert left <= rc.MAX_LEFT_OUT * rc.N_LANES, (cfg.label(), k, left)
    print("[rough K] worst: " + "  ".join(f"{k} {v:.2f} (K = {rc.K[k]:g})" for k, v in worst.items()))
    for k, v in worst.items():
        assert 4 * v <= rc.K[k], (k, v, rc.K[k])


def test_sampling_identity_f64(k_rows):
    """weight * pdf = eval at the sampled wo for valid samples.  With sample_visible = false the weight is built on the unscaled
    distribution and the pdf on the scaled one (roughdielectric.cpp:269-276,349-355), so the product carries D_scaled(m) / D(m)."""
    for cfg, ref, _ in k_rows:
        o, d, smp, _ = rc.make_inputs(cfg)
        wi = (-d).astype(np.float64)
        s = rr.sample(cfg, wi, smp[:, 0].astype(np.float64), smp[:, 1:].astype(np.float64))
        ev, pdf, _ = rr.eval_pdf(cfg, wi, s["wo"])
        valid = (s["weight"] > 0) & (ev > 1e-280)
        assert valid.mean() > 0.5
        assert np.allclose(pdf[valid], s["pdf"][valid], rtol=1e-6, atol=0), cfg.label()
        assert np.allclose((s["weight"] * s["pdf"] * rc.scaling_ratio(cfg, wi, s["m"]))[valid], ev[valid], rtol=1e-6, atol=0), cfg.label()


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c.alpha_u >= 0.05 and c.int_ior > 1.2], ids=lambda c: c.label())
def test_pdf_integrates_to_at_most_one(cfg):
    for wi in ([0.3, 0.2, 0.93], [0.2, -0.6, -0.5]):
        wi = np.asarray(wi) / np.linalg.norm(wi)
        r, t = rr.lobe_integrals(cfg, wi, n_theta=1024, n_phi=256, what="pdf")
        assert 0.5 < r + t <= 1 + 2e-3, (cfg.label(), wi, r, t)


def test_quadrature_converges():
    cfg = rr.Config(0.1, ggx=True)
    wi = np.array([np.sin(np.radians(60)), 0, np.cos(np.radians(60))])
    a = rr.lobe_integrals(cfg, wi, n_theta=2048, n_phi=512); b = rr.lobe_integrals(cfg, wi, n_theta=4096, n_phi=1024)
    assert abs(a[0] - b[0]) < 1e-4 * b[0] and abs(a[1] - b[1]) < 1e-4 * b[1]


@pytest.mark.parametrize("case", rc.CHI2_CASES, ids=lambda c: c[0])
def test_chi2_harness_on_the_reference(case):
    name, cfg, wi = case
    n = 1 << 18
    rng = np.random.default_rng(11)
    u = rng.random((n, 3))
    wi = np.asarray(wi, np.float64) / np.linalg.norm(wi)
    W = np.broadcast_to(wi, (n, 3))
    s = rr.sample(cfg, W, u[:, 0], u[:, 1:])
    zero = ~(s["pdf"] > 0) | ~(s["weight"] > 0)
    p, stat, dof, mass = rr.chi2_test(s["wo"], lambda d: rr.eval_pdf(cfg, np.broadcast_to(wi, d.shape), d)[1], n, p_zero=zero, mass_slack=rc.chi2_slack(cfg))
    print(f"[rough chi2 ref] {name}: p = {p:.4f}, chi2 = {stat:.1f}, dof = {dof}, mass = {mass:.5f}, zero-density samples {int(zero.sum())}")
    assert p > rc.CHI2_THRESHOLD, (name, p, stat, dof)
    # ... and the harness can fail: the sampler of another roughness against this pdf
    other = rr.Config(cfg.alpha_u * 0.8, cfg.alpha_v * 0.8, cfg.ggx, cfg.visible, cfg.int_ior, cfg.ext_ior)
    s2 = rr.sample(other, W, u[:, 0], u[:, 1:])
    zero2 = ~(s2["pdf"] > 0) | ~(s2["weight"] > 0)
    p2 = rr.chi2_test(s2["wo"], lambda d: rr.eval_pdf(cfg, np.broadcast_to(wi, d.shape), d)[1], n, p_zero=zero2, mass_slack=rc.chi2_slack(cfg))[0]
    assert p2 < 1e-6, (name, p2)
