"""The conductor, plastic and twosided BSDFs on the device, held to the float64 reference of tests/smooth_ref.py:
(a) lrt_bsdf_probe per lane on every case of smooth_cases.py, (b) what holds exactly, (c) a mirror and a metal floor under a constant
environment, (d) a plastic floor under a directional light through four integrators, (e) a twosided rectangle seen from behind,
(f) routing: prbvolpath, an unused BSDF, the albedo AOV, moment and lrt_render_multi.  Tolerances: smooth_cases.py."""
import numpy as np
import pytest

import smooth_cases as sc
import smooth_ref as sr

pytestmark = pytest.mark.gpu

_cache = {}
CASE = {c[0]: c for c in sc.CASES}


def local_queries(pr, woq, shape):
    """the query directions in the shading frame: the planes' frame is the world's; on the sphere only wo.z = <wo, n> is known, and
    it is all these BSDFs read of wo"""
    if shape != "sphere":
        return np.asarray(woq, np.float64)
    z = np.clip((np.asarray(woq, np.float64) * pr["sh_n"].astype(np.float64)).sum(1), -1, 1)
    return np.stack([np.sqrt(1 - z * z), np.zeros_like(z), z], 1)


def probe_case(mi, name, tmp_path_factory):
    """the probe on the case's inputs, and the float64 reference at the device's own wi and uv (float32, taken as exact)"""
    if name not in _cache:
        _, bsdf, shape, bump = CASE[name]
        s = mi.load_string(sc.scene_xml(bsdf, shape, bump, tmp_path_factory.mktemp("smooth_" + name)))
        o, d, smp, woq, _, _ = sc.make_inputs(bsdf, shape)
        pr = s.bsdf_probe(o, d, smp, woq)
        assert (pr["shape"] >= 0).all()
        ref = sc.reference(bsdf, pr["wi"], smp, local_queries(pr, woq, shape), pr["uv"])
        _cache[name] = (s, pr, ref, (o, d, smp, woq))
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", [c[0] for c in sc.CASES])
def test_probe_against_float64(mi, name, tmp_path_factory):
    _, bsdf, shape, bump = CASE[name]
    s, pr, ref, _ = probe_case(mi, name, tmp_path_factory)
    assert np.isfinite(pr["raw"]).all()                                   # every lane, the left-out ones included
    if shape == "planes":
        assert set(np.unique(pr["shape"])) == {0, 1}                      # the rectangle and the mesh
        assert (pr["wi"][:, 2] > 0).sum() == (pr["wi"][:, 2] < 0).sum()
    else:
        assert (pr["wi"][:, 2] < 0).sum() > 1000 and (pr["wi"][:, 2] > 0).sum() > 1000
    got = {"wo": pr["wo"], "wo_z": pr["wo_z"], "pdf": pr["pdf"], "eta": pr["eta"], "weight": pr["weight"], "eval": pr["eval"], "eval_pdf": pr["eval_pdf"]}
    fields = tuple("wo_z" if (k == "wo" and shape == "sphere") else k for k in sc.FIELDS) + (("wo_z",) if shape != "sphere" else ())
    w = sc.worst_ratios(ref, got, fields)
    print(f"[smooth a] {name:22s} " + "  ".join(f"{k} {v[0]:5.2f}/{sc.K['wo' if k == 'wo_z' else k]:g} (-{v[1]})" for k, v in w.items()))
    for k, (r, left) in w.items():
        assert left <= sc.MAX_LEFT_OUT * sc.N_LANES, (name, k, left)
        assert r <= sc.K["wo" if k == "wo_z" else k], (name, k, r)
    ok = ref["sample_ok"]
    assert (pr["type"][ok] == ref["type"][ok]).all()
    assert set(np.unique(pr["type"])) <= {0, sr.F_DELTA, sr.F_SMOOTH}    # a sample's type is one of the two, never both


# ---------------------------------------------------------------------------------------------------------------------- (b)
def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["mirror", "conductor_rgb", "conductor_board"])
def test_conductor_exact(mi, name, tmp_path_factory):
    """wo is the reflection, pdf 1, type delta; eval and pdf are 0 everywhere, at the sampled wo too; a back-side hit is all zero"""
    s, pr, ref, (o, d, smp, woq) = probe_case(mi, name, tmp_path_factory)
    front = pr["wi"][:, 2] > 0
    wi = pr["wi"]
    assert np.array_equal(bits(pr["wo"][front]), bits(wi[front] * np.float32([-1, -1, 1])))
    assert (pr["pdf"][front] == 1).all() and (pr["eta"][front] == 1).all() and (pr["type"][front] == sr.F_DELTA).all()
    assert (pr["eval"] == 0).all() and (pr["eval_pdf"] == 0).all()
    at_wo = s.bsdf_probe(o, d, smp, np.where(front[:, None], pr["wo"], woq).astype(np.float32))
    assert (at_wo["eval"] == 0).all() and (at_wo["eval_pdf"] == 0).all()
    back = ~front
    for k in ("wo", "pdf", "eta", "type", "weight", "eval", "eval_pdf"):
        assert (pr[k][back] == 0).all(), k


def test_mirror_weight_is_the_reflectance_in_the_bits(mi, tmp_path_factory):
    """eta = 0, k = 1: fresnel_conductor is exactly 1 at every angle (dshade.h), so the weight is specular_reflectance"""
    colour = np.float32([0.9, 0.55, 0.3])
    bsdf = sr.Conductor(specular_reflectance=colour)
    s = mi.load_string(sc.scene_xml(bsdf, "planes", False, tmp_path_factory.mktemp("smooth_mirror_colour")))
    o, d, smp, woq, _, _ = sc.make_inputs(bsdf)
    pr = s.bsdf_probe(o, d, smp, woq)
    front = pr["wi"][:, 2] > 0
    assert front.sum() == sc.N_LANES // 2 and np.array_equal(bits(pr["weight"][front]), np.broadcast_to(bits(colour), (front.sum(), 3)))
    _, pr1, _, _ = probe_case(mi, "mirror", tmp_path_factory)
    assert (pr1["weight"][pr1["wi"][:, 2] > 0] == 1).all()


@pytest.mark.parametrize("name", ["plastic", "plastic_nonlinear", "plastic_board", "bump_plastic"])
def test_plastic_identity_and_sides(mi, name, tmp_path_factory):
    """A smooth sample: weight * pdf = eval at that wo, all three from the device (the second probe asks for eval at the first one's wo).
    Each factor carries its own tolerance of (a), so to first order |w p - e| <= 2^-23 (K_w c_w max(1, |w|) p + K_p c_p max(1, p) |w| +
    K_e c_e max(1, |e|)).  A delta sample adds nothing to eval and pdf: at the mirror direction they are the diffuse lobe's alone,
    the reference's value (plastic.cpp:273-323 never name the coat).  A back-side hit is all zero."""
    _, bsdf, shape, bump = CASE[name]
    s, pr, ref, (o, d, smp, woq) = probe_case(mi, name, tmp_path_factory)
    wo = pr["wo"].astype(np.float32)
    pr2 = s.bsdf_probe(o, d, smp, wo)
    assert np.array_equal(pr2["pdf"], pr["pdf"]) and np.array_equal(pr2["weight"], pr["weight"])
    ref2 = sc.reference(bsdf, pr["wi"], smp, wo, pr["uv"])
    smooth = ref["sample_ok"] & ref2["eval_ok"] & (pr["type"] == sr.F_SMOOTH)
    w, p, e = pr["weight"].astype(np.float64), pr["pdf"].astype(np.float64)[:, None], pr2["eval"].astype(np.float64)
    c = ref["cond"]
    tol = sc.EPS * (sc.K["weight"] * c["weight"][:, None] * np.maximum(1, np.abs(w).max(1))[:, None] * p + sc.K["pdf"] * c["pdf"][:, None] * np.maximum(1, p) * np.abs(w)
                    + sc.K["eval"] * ref2["cond"]["eval"][:, None] * np.maximum(1, np.abs(e).max(1))[:, None])
    r = (np.abs(w * p - e) / tol)[smooth]
    print(f"[smooth b] {name:18s} weight * pdf against eval: worst error / bound {r.max():.3f} over {smooth.sum()} smooth lanes")
    assert smooth.sum() > 1000 and r.max() <= 1.0
    delta = ref["sample_ok"] & ref2["eval_ok"] & (pr["type"] == sr.F_DELTA)
    assert delta.sum() > 200
    for k in ("eval", "eval_pdf"):
        rr = sc.ratio(pr2[k], ref2[k], ref2["cond"][k])[delta]
        assert rr.max() <= sc.K[k], (k, rr.max())
    assert (pr2["eval"][delta] > 0).all() and np.isfinite(pr2["eval"]).all()
    back = pr["wi"][:, 2] < 0
    for k in ("wo", "pdf", "eta", "type", "weight", "eval", "eval_pdf"):
        assert (pr[k][back] == 0).all(), k


@pytest.mark.parametrize("name", ["twosided_diffuse", "twosided_plastic"])
def test_twosided_back_is_the_mirrored_front(mi, name, tmp_path_factory):
    """one child: a back-side hit gives what the front side gives at the mirrored wi, with wo.z negated, in the bits (twosided.cpp:124-127)"""
    _, bsdf, shape, bump = CASE[name]
    s, _, _, (o, d, smp, woq) = probe_case(mi, name, tmp_path_factory)
    flip = np.float32([1, 1, -1])
    front = d[:, 2] < 0                                                  # rays going down meet the front
    o, d, smp, woq = o[front], d[front], smp[front], woq[front]
    a = s.bsdf_probe(o, d, smp, woq)
    b = s.bsdf_probe(o * flip, d * flip, smp, woq * flip)
    assert (a["wi"][:, 2] > 0).all() and np.array_equal(bits(b["wi"]), bits(a["wi"] * flip))
    for k in ("pdf", "eta", "type", "weight", "eval", "eval_pdf"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(bits(b["wo"]), bits(a["wo"] * flip)) and np.array_equal(bits(b["wo_z"]), bits(-a["wo_z"]))
    assert (a["weight"] > 0).all() and (a["eval"].max(1) > 0).sum() > 200


# ------------------------------------------------------------------------------------------------------------------ floors
SIZE, FOV = 32, 40.0
CAM_O, CAM_T, CAM_UP = np.array([0.0, -4.0, 3.0]), np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])


def floor_xml(integrator, bsdf, emitter, spp, moment=False, origin=CAM_O, up=CAM_UP, max_depth=3, extra=""):
    integ = f'<integrator type="{integrator}"><integer name="max_depth" value="{max_depth}"/></integrator>'
    if moment:
        integ = f'<integrator type="moment">{integ}</integrator>'
    v = lambda a: ", ".join(repr(float(x)) for x in a)
    return (f'<scene version="3.0.0">{integ}<sensor type="perspective"><float name="fov" value="{FOV}"/>'
            f'<transform name="to_world"><lookat origin="{v(origin)}" target="{v(CAM_T)}" up="{v(up)}"/></transform>'
            f'<sampler type="independent"><integer name="sample_count" value="{spp}"/></sampler>'
            f'<film type="hdrfilm"><integer name="width" value="{SIZE}"/><integer name="height" value="{SIZE}"/><rfilter type="box"/></film></sensor>'
            f'<shape type="rectangle"><transform name="to_world"><scale value="10"/></transform>{bsdf}</shape>{extra}{emitter}</scene>')


def pixel_dirs(origin=CAM_O, up=CAM_UP, sub=16):
    """unit directions of the camera rays through sub x sub midpoints of every pixel: (SIZE, SIZE, sub * sub, 3).  look_at (transform.h): dir,
    left = up x dir, new_up = dir x left; film x runs along -left and film y along -new_up (perspective.cpp; tests/test_spot_gpu.py floor_points)"""
    dr = (CAM_T - origin) / np.linalg.norm(CAM_T - origin)
    left = np.cross(up, dr); left /= np.linalg.norm(left)
    nup = np.cross(dr, left)
    t = np.tan(np.radians(FOV) / 2)
    s = (np.arange(SIZE * sub) + 0.5) / (SIZE * sub)
    X, Y = np.meshgrid((2 * s - 1) * t, (2 * s - 1) * t)
    D = dr[None, None] - X[..., None] * left[None, None] - Y[..., None] * nup[None, None]
    D /= np.linalg.norm(D, axis=-1, keepdims=True)
    return D.reshape(SIZE, sub, SIZE, sub, 3).transpose(0, 2, 1, 3, 4).reshape(SIZE, SIZE, sub * sub, 3)


def held(img, L, spp, label):
    """per pixel against the 16 x 16 midpoint mean of the closed form L (SIZE, SIZE, 256, 3): 5 standard errors of the jitter plus 1e-4 relative"""
    mean, se = L.mean(2), np.sqrt(L.var(2) / spp)
    err = np.abs(img.astype(np.float64)[..., :3] - mean)
    tol = 5 * se + 1e-4 * mean
    print(f"[smooth floor] {label}: worst |err| / tol {(err / np.maximum(tol, 1e-300))[mean > 0].max():.3f}; values {mean.min():.4f} .. {mean.max():.4f}")
    assert np.isfinite(img).all() and (mean > 0).all() and (err <= tol).all()


ENV_L = np.array([0.7, 1.1, 0.4])
ENV = f'<emitter type="constant"><rgb name="radiance" value="{", ".join(str(x) for x in ENV_L)}"/></emitter>'


def test_mirror_floor(mi):
    """every camera ray meets the floor and leaves into the environment: L * specular_reflectance in every pixel"""
    colour = np.array([0.9, 0.55, 0.3])
    s = mi.load_string(floor_xml("path", sr.Conductor(specular_reflectance=colour).xml(), ENV, 16))
    assert (-pixel_dirs()[..., 2] > 0.2).all()                          # every ray goes down onto the 20 x 20 floor
    held(s.render(seed=3), np.broadcast_to(ENV_L * np.float32(colour).astype(np.float64), (SIZE, SIZE, 256, 3)), 16, "mirror")


def test_metal_floor(mi):
    """L * F(cos theta) per channel, cos theta from the camera ray"""
    bsdf = sr.Conductor(**sc.GOLD)
    spp = 64
    s = mi.load_string(floor_xml("path", bsdf.xml(), ENV, spp))
    c = -pixel_dirs()[..., 2]
    F = np.stack([sr.fresnel_conductor(c, bsdf.eta[j], bsdf.k[j]) for j in range(3)], -1)
    assert F.min() > 0.3 and F.max() < 1 and np.ptp(F[..., 0]) > 0.005
    held(s.render(seed=3), ENV_L * F, spp, "metal")


SUN_DIR, SUN_E = np.array([0.5, 0.3, -0.8]), 2.5
SUN = f'<emitter type="directional"><vector name="direction" value="{", ".join(str(x) for x in SUN_DIR)}"/><rgb name="irradiance" value="{SUN_E}"/></emitter>'


def clear_liver():
    """a liver medium whose every coefficient is 0: transmittance 1, no collision, for the homogeneous reading (sigma_t) and the bio one alike"""
    return ('<medium type="liver" id="clear">' + "".join(f'<float name="sigma_{k}{l}_{c}" value="0"/>' for k in ("collagen", "elastin") for l in range(1, 5) for c in "RGB")
            + '<float name="layer1Limit" value="0.1"/><float name="layer2Limit" value="0.2"/><float name="layer3Limit" value="0.35"/><float name="layer4Limit" value="0.6"/>'
            '<rgb name="sigma_blood" value="0"/><rgb name="sigma_bile" value="0"/><rgb name="sigma_lipid_water" value="0"/>'
            '<float name="sigma_hepatocity" value="0"/><boolean name="has_spectral_extinction" value="false"/><rgb name="sigma_t" value="0"/></medium>')


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis", "biovolpath"])
def test_plastic_floor(mi, integrator):
    """a directional light, no environment, the camera off the mirror direction: the coat's reflection finds nothing, the emitter sample is taken
    because the BSDF is smooth too, and every pixel is E * eval(wi, wo = towards the light) (eval carries the cosine).
    The sensor sits in a liver medium whose coefficients are all 0 (the floor is no medium boundary, so the whole scene lies in it): biovolpath
    clears a path's radiance on every trip that is not inside a medium (biovolpath.cpp:297-300, kernels_bio.h), so without one it renders every
    surface black, a Lambertian one too.  A clear medium changes no value, and the four integrators render one scene."""
    bsdf = sr.Plastic(diffuse_reflectance=[0.7, 0.4, 0.15], specular_reflectance=[0.9, 0.9, 0.9], nonlinear=True)
    spp = 64
    xml = floor_xml(integrator, bsdf.xml(), SUN, spp).replace("<sensor", clear_liver() + "<sensor", 1).replace("</film></sensor>", '</film><ref id="clear"/></sensor>')
    s = mi.load_string(xml)
    assert s.desc.sensor.medium == 0
    wo = np.array(s.desc.emitters[0].to_world, np.float32).reshape(4, 4)[:3, 2].astype(np.float64) * -1
    assert np.allclose(wo, -SUN_DIR / np.linalg.norm(SUN_DIR), atol=1e-6)
    wi = -pixel_dirs().reshape(-1, 3)
    mirror = wi * np.array([-1, -1, 1])
    assert (mirror @ wo).max() < 0.9                                     # no pixel looks along the light's reflection
    ev = bsdf.eval_pdf(wi, np.broadcast_to(wo, wi.shape), np.zeros((len(wi), 2)))[0]
    held(s.render(seed=5), (SUN_E * ev).reshape(SIZE, SIZE, 256, 3), spp, f"plastic {integrator}")


# ---------------------------------------------------------------------------------------------------------------------- (e)
def test_twosided_seen_from_behind(mi):
    """a rectangle lit and seen from below (its back): Lambert's rho / pi E cos with the adapter, black without it, the back child's colour with two
    children.  Bound: 2^-20 relative, as for tests/test_spot_gpu.py's directional floor (a handful of float32 products, no jitter in the value)."""
    below = CAM_O * np.array([1, 1, -1]); sun = SUN.replace("-0.8", "0.8")
    rho, rho_back = np.array([0.7, 0.5, 0.2]), np.array([0.1, 0.8, 0.3])
    render = lambda b: mi.load_string(floor_xml("path", b.xml(), sun, 4, origin=below, max_depth=2)).render(seed=2).astype(np.float64)[..., :3]
    cos = 0.8 / np.linalg.norm(SUN_DIR)
    one = render(sr.TwoSided(sr.Diffuse(rho)))
    want = np.float32(rho).astype(np.float64) / np.pi * SUN_E * cos
    assert (np.abs(one - want) / want <= 2.0 ** -20).all()
    assert (render(sr.Diffuse(rho)) == 0).all()
    two = render(sr.TwoSided(sr.Diffuse(rho), sr.Diffuse(rho_back)))
    want = np.float32(rho_back).astype(np.float64) / np.pi * SUN_E * cos
    assert (np.abs(two - want) / want <= 2.0 ** -20).all()


# ---------------------------------------------------------------------------------------------------------------------- (f)
def test_prbvolpath_is_refused_at_render_time(mi):
    message = r"unsupported: prbvolpath on a scene with a conductor / plastic / twosided BSDF \(no adjoint is built for them\)"
    plain = mi.load_string(floor_xml("path", '<bsdf type="diffuse"/>', ENV, 1))
    plain.render(integrator="prbvolpath", spp=1)                        # the same scene without a new type has an adjoint
    for b in (sr.Conductor(), sr.Plastic(), sr.TwoSided(sr.Diffuse())):
        s = mi.load_string(floor_xml("path", b.xml(), ENV, 1))
        with pytest.raises(RuntimeError, match=message):
            s.render(integrator="prbvolpath", spp=1)
        with pytest.raises(RuntimeError, match=message):
            s.render_backward(np.ones(s.film_shape(), np.float32), integrator="prbvolpath")


def test_unused_smooth_bsdfs_change_nothing(mi):
    """BSDFs of the new types that no shape references leave the scene on the kernels it ran before (scene_prep.cpp): bit-identical lanes"""
    base = mi.cornell_box()
    d = dict(base)
    d["spare_c"] = {"type": "conductor"}; d["spare_p"] = {"type": "plastic"}; d["spare_t"] = {"type": "twosided", "a": {"type": "diffuse"}, "b": {"type": "plastic"}}
    a = mi.load_dict(base); b = mi.load_dict(d)
    assert b.desc.n_bsdfs == a.desc.n_bsdfs + 5
    n = 256 * 256 * 4
    la, lb = a.render_samples(0, n, spp=4, seed=3), b.render_samples(0, n, spp=4, seed=3)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)) and la[:, :3].max() > 0
    assert a.stats()["record_bytes"] == b.stats()["record_bytes"]
    b.render(integrator="prbvolpath", spp=1)                            # ... and keeps its adjoint


@pytest.mark.parametrize("name", ["conductor_board", "plastic_board", "twosided_two", "twosided_two_diffuse", "bump_plastic"])
def test_aov_albedo(mi, name, tmp_path_factory):
    """plastic: diffuse_reflectance (plastic.cpp:362-365); conductor: 0 (bsdf.cpp:38-43); twosided: the child of the side that was hit
    (twosided.cpp:284-307); a bumpmap hands on its child's.  The camera sees the front of the rectangle; per lane, at the lane's own uv."""
    _, bsdf, shape, bump = CASE[name]
    xml = sc.scene_xml(bsdf, shape, bump, tmp_path_factory.mktemp("smooth_aov_" + name), integrator='<integrator type="aov"><string name="aovs" value="al:albedo,tc:uv"/></integrator>')
    for origin, front in (("0,0,5", True), ("0,0,-5", False)):
        s = mi.load_string(xml.replace('origin="0,0,5"', f'origin="{origin}"').replace('<float name="fov" value="40"/>', '<float name="fov" value="15"/>'))      # the rectangle fills the frame
        lanes = s.render_aov_samples(0, 4 * 4 * 4)
        uv = lanes[:, 3:5]
        hit = (uv != 0).any(1)
        assert hit.sum() > 32 and (lanes[~hit, :3] == 0).all()
        wi = np.broadcast_to(np.array([0.0, 0.0, 1.0 if front else -1.0]), (len(lanes), 3))
        want = bsdf.albedo(wi, uv.astype(np.float64)).astype(np.float32)
        # (eval_diffuse_reflectance of a one-sided BSDF does not look at the side: smooth_ref.py's albedo() ignores wi there too)
        keep = hit & (sc.bsdf_tex_margin(bsdf, uv) > sc.TEX_MARGIN)
        assert keep.sum() > 32 and np.array_equal(lanes[keep, :3], want[keep]), (name, front)
        if name in ("plastic_board", "twosided_two_diffuse"):
            assert len(np.unique(lanes[keep, 0])) == (2 if (name == "plastic_board" or not front) else 1)


def test_moment_and_multi_agree_with_a_plain_render(mi):
    bsdf = sr.TwoSided(sr.Plastic(diffuse_reflectance=[0.7, 0.4, 0.15]), sr.Conductor(**sc.GOLD))
    both = ENV + SUN
    s = mi.load_string(floor_xml("path", bsdf.xml(), both, 4))
    single = s.render(seed=5)
    assert single[..., :3].min() > 0
    multi = s.render_multi([0, 0], seed=5)
    assert np.allclose(multi, single, rtol=1e-6, atol=0)
    mom = mi.load_string(floor_xml("path", bsdf.xml(), both, 4, moment=True)).render(seed=5)
    assert np.allclose(mom[..., :3], single[..., :3], rtol=1e-6, atol=0) and np.isfinite(mom).all()
    aov = mi.load_string(floor_xml("path", bsdf.xml(), both, 4).replace('<integrator type="path">', '<integrator type="aov"><string name="aovs" value="dd.y:depth"/><integrator type="path">')
                         .replace('</integrator><sensor', '</integrator></integrator><sensor')).render(seed=5)
    assert np.allclose(aov[..., :3], single[..., :3], rtol=1e-6, atol=0)
