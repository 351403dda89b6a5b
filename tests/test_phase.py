"""Tabulated, Rayleigh and blended phase functions on the host: what the loader reads and refuses, the phase
table of the description, the dictionary route, and the float64 reference of tests/phase_ref.py held against itself, so that the device
checks of test_phase_gpu.py are known to be passable: normalisation, the sampling identity, chi-square tests of the reference's own
sampler, the forward / backward convention against analytic HG, the details of the scalar constructor, the K table and the 1 % cap."""
import ctypes as C

import numpy as np
import pytest

import phase_cases as pc
import phase_ref as pr
import rough_ref as rr

CONFIGS = pc.configs()
TAB, RAYLEIGH, BLEND = 2, 3, 4


def scene(mi, phase_xml, integrator="volpath", extra=""):
    return mi.load_string(f'<scene version="3.0.0"><integrator type="{integrator}"/><sensor type="perspective"><film type="hdrfilm">'
                          f'<integer name="width" value="4"/><integer name="height" value="4"/></film></sensor>{extra}'
                          f'<shape type="cube"><bsdf type="null"/><medium name="interior" type="homogeneous">{phase_xml}</medium></shape>'
                          '<emitter type="constant"/></scene>')


def phases(sc):
    """copies of the table's entries (their `values` point into the scene: keep it alive while reading them)"""
    d = sc.desc
    return [type(d.phases[i]).from_buffer_copy(d.phases[i]) for i in range(d.n_phases)]


# ------------------------------------------------------------------------------------------------- loader, description, load_dict
def test_version_and_xml(mi):
    assert mi._lib.lib().lrt_version() >= 116 and "lrt_phase_probe" in mi._lib.EXPORTED_SYMBOLS
    sc = scene(mi, '<phase type="tabphase"><string name="values" value="0.5, 1 2,3.5"/></phase>')
    (P,) = phases(sc)
    assert P.type == TAB and P.n_values == 4 and [P.values[i] for i in range(4)] == [0.5, 1.0, 2.0, 3.5] and list(P.child) == [-1, -1]
    m = sc.desc.media[0]
    assert m.phase_index == 0 and m.phase == 0 and m.g == 0.0                  # `phase` / `g` keep today's meaning: isotropic when unused
    (P,) = phases(scene(mi, '<phase type="rayleigh"/>'))
    assert P.type == RAYLEIGH and P.n_values == 0
    sc = scene(mi, '<phase type="blendphase"><float name="weight" value="1.5"/><phase type="hg"><float name="g" value="0.25"/></phase>'
                   '<phase type="tabphase"><string name="values" value="1 2"/></phase></phase>')
    c0, c1, B = phases(sc)
    assert (c0.type, c0.g, c1.type, c1.n_values) == (1, 0.25, TAB, 2)             # the children in document order, then the blend
    assert B.type == BLEND and list(B.child) == [0, 1] and B.weight == 1.5 and sc.desc.media[0].phase_index == 2   # (clipped where it is used)
    # isotropic and hg media stay out of the table
    assert scene(mi, '<phase type="hg"><float name="g" value="0.5"/></phase>').desc.n_phases == 0


@pytest.mark.parametrize("phase_xml, message", [
    ('<phase type="tabphase"><string name="values" value="1"/></phase>', "needs at least two entries"),
    ('<phase type="tabphase"><string name="values" value=""/></phase>', "needs at least two entries"),
    ('<phase type="tabphase"><string name="values" value="1, -0.5, 1"/></phase>', "entries must be non-negative"),
    ('<phase type="tabphase"><string name="values" value="0 0 0"/></phase>', "no probability mass found"),
    ('<phase type="tabphase"><string name="values" value="1, abc"/></phase>', "Could not parse floating point value 'abc'"),
    ('<phase type="tabphase"><float name="values" value="1"/></phase>', "'values' must be a string"),
    ('<phase type="blendphase"><float name="weight" value="0.5"/><phase type="isotropic"/></phase>', "BlendPhase: Two child phase functions must be specified!"),
    ('<phase type="blendphase"><float name="weight" value="0.5"/><phase type="isotropic"/><phase type="rayleigh"/><phase type="hg"/></phase>',
     "BlendPhase: Cannot specify more than two child phase functions"),
    ('<phase type="blendphase"><volume name="weight" type="gridvolume"/><phase type="isotropic"/><phase type="rayleigh"/></phase>',
     "unsupported: a volume as the weight of a blendphase"),
    ('<phase type="blendphase"><float name="weight" value="0.5"/><phase type="isotropic"/><phase type="blendphase"><float name="weight" value="0.5"/>'
     '<phase type="isotropic"/><phase type="rayleigh"/></phase></phase>', "unsupported: a blendphase as the child of a blendphase"),
    ('<phase type="sggx"/>', 'unsupported phase function "sggx"'),
])
def test_loader_errors(mi, phase_xml, message):
    with pytest.raises(RuntimeError, match=message):
        scene(mi, phase_xml)


def test_unsupported_status(mi):
    L = mi._lib.lib()
    for body in ('<phase type="blendphase"><volume name="weight" type="gridvolume"/><phase type="isotropic"/><phase type="rayleigh"/></phase>',
                 '<phase type="blendphase"><float name="weight" value="0.5"/><phase type="isotropic"/><phase type="blendphase"/></phase>'):
        xml = (f'<scene version="3.0.0"><integrator type="volpath"/><sensor type="perspective"><film type="hdrfilm"/></sensor><shape type="cube"><bsdf type="null"/>'
               f'<medium name="interior" type="homogeneous">{body}</medium></shape></scene>').encode()
        h = C.c_void_p()
        assert L.lrt_scene_load_xml_string(xml, b".", None, 0, C.byref(h)) == mi._lib.UNSUPPORTED


def test_prbvolpath_is_refused(mi):
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath on a scene with a tabulated / Rayleigh / blended phase function"):
        scene(mi, '<phase type="rayleigh"/>', integrator="prbvolpath")
    # a medium that nothing references changes nothing
    spare = '<medium type="homogeneous" id="spare"><phase type="rayleigh"/></medium>'
    sc = scene(mi, '<phase type="isotropic"/>', integrator="prbvolpath", extra=spare)
    assert sc.desc.n_phases == 1 and sc.desc.n_media == 2


def test_load_dict_round_trip(mi):
    tab = [0.25, 1.0, 4.0]
    d = pc.scene_dict(pr.rayleigh())
    d["box"]["interior"]["phase"] = {"type": "blendphase", "weight": 0.25, "phase_0": {"type": "rayleigh"}, "phase_1": {"type": "tabphase", "values": tab}}
    xml = mi.dict_to_xml(d)
    assert '<phase type="blendphase">' in xml and '<string name="values" value="0.25, 1.0, 4.0"/>' in xml
    sc = mi.load_dict(d)
    c0, c1, B = phases(sc)
    assert (c0.type, c1.type, B.type, B.weight, list(B.child)) == (RAYLEIGH, TAB, BLEND, 0.25, [0, 1]) and [c1.values[i] for i in range(3)] == tab
    d["box"]["interior"]["phase"]["phase_1"]["values"] = "0.25 1 4"                     # a string, as the plugin reads it
    as_string = mi.load_dict(d)
    assert [phases(as_string)[1].values[i] for i in range(3)] == tab
    same = phases(mi.load_string(xml))
    assert [(p.type, p.weight, p.n_values) for p in same] == [(p.type, p.weight, p.n_values) for p in (c0, c1, B)]
    # the parameter keys of mi.traverse gain nothing
    mid = sc.medium_ids()[0]
    for key in (f"{mid}.phase_function.values", f"{mid}.phase_function.weight", f"{mid}.phase_function.g"):
        with pytest.raises(RuntimeError, match="unknown parameter"):
            sc.param_set(key, [0.5])


def test_scene_from_desc_validation(mi):
    from liverrenderer_amd import _lib
    base = mi.load_dict(pc.scene_dict(pr.blend(0.3, pr.tabphase("1,2,3"), pr.hg(0.5))))
    L = _lib.lib()

    def attempt(mutate):
        d = _lib.SceneDesc.from_buffer_copy(base.desc)
        ph = (_lib.PhaseDesc * d.n_phases)(*[d.phases[i] for i in range(d.n_phases)])
        md = (_lib.MediumDesc * d.n_media)(*[d.media[i] for i in range(d.n_media)])
        d.phases = C.cast(ph, C.POINTER(_lib.PhaseDesc)); d.media = C.cast(md, C.POINTER(_lib.MediumDesc))
        keep = mutate(ph, md, d)
        h = C.c_void_p()
        st = L.lrt_scene_from_desc(C.byref(d), C.byref(h))
        n = -1
        if st == 0:
            n = L.lrt_scene_desc_get(h).contents.n_phases
            L.lrt_scene_free(h)
        return st, L.lrt_last_error().decode(), n, keep

    assert attempt(lambda ph, md, d: None)[::2] == (0, 3)
    neg = (C.c_float * 3)(1.0, -2.0, 3.0); zero = (C.c_float * 3)(0.0, 0.0, 0.0)
    cases = {
        "type": (lambda ph, md, d: setattr(ph[0], "type", 9), "invalid phase function"),
        "g": (lambda ph, md, d: setattr(ph[1], "g", 1.0), "asymmetry parameter"),
        "one value": (lambda ph, md, d: setattr(ph[0], "n_values", 1), "needs at least two entries"),
        "negative": (lambda ph, md, d: (setattr(ph[0], "values", C.cast(neg, C.POINTER(C.c_float))), neg)[1], "entries must be non-negative"),
        "no mass": (lambda ph, md, d: (setattr(ph[0], "values", C.cast(zero, C.POINTER(C.c_float))), zero)[1], "no probability mass found"),
        "child": (lambda ph, md, d: ph[2].child.__setitem__(1, 3), "invalid child"),
        "nested": (lambda ph, md, d: ph[2].child.__setitem__(0, 2), "unsupported: a blendphase as the child of a blendphase"),
        "weight": (lambda ph, md, d: setattr(ph[2], "weight", float("nan")), "weight"),
        "medium index": (lambda ph, md, d: setattr(md[0], "phase_index", 3), "invalid entry"),
        "medium at a leaf": (lambda ph, md, d: setattr(md[0], "phase_index", 1), "isotropic / hg entry"),
    }
    for name, (fn, msg) in cases.items():
        st, err, _, _ = attempt(fn)
        assert st != 0 and msg in err, (name, st, err)
    assert attempt(cases["nested"][0])[0] == _lib.UNSUPPORTED
    # a description from before the table (n_phases = 0) means what it meant: the medium's index is not read
    st, _, n, _ = attempt(lambda ph, md, d: (setattr(d, "n_phases", 0), setattr(md[0], "phase_index", 0)))
    assert st == 0 and n == 0


# ------------------------------------------------------------------------------------------ the reference against itself, float64
FAMILIES = [c for c in CONFIGS if c.label in ("tab5", "tabflat", "tab257", "rayleigh", "blend0.3(rayleigh,hg0.8)", "blend0.3(tab5,tab257)")]


@pytest.mark.parametrize("p", FAMILIES, ids=lambda p: p.label)
def test_eval_integrates_to_one(p):
    """midpoint rule in (cos, phi) with the table's nodes on cell borders (4096 = 16 * 256 cells over cos): exact for the piecewise linear
    table up to rounding; Rayleigh / HG 0.8: smooth, error below 1e-5 at this resolution"""
    d, w = rr.sphere_grid(4096, 8)
    wi = np.broadcast_to(np.array([0.0, 0.0, 1.0]), d.shape)
    v, _ = pr.eval_pdf(p, wi, d)
    assert abs(float(v.sum() * w) - 1) < 1e-5


@pytest.mark.parametrize("p", CONFIGS, ids=lambda p: p.label)
def test_sampling_identity_f64(p):
    """weight * pdf = eval at the sampled direction (wi made a unit vector in float64: eval takes the cosine from dot(wo, wi))"""
    wi, smp, _ = pc.make_inputs(p)
    wi = wi.astype(np.float64); wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    s = pr.sample(p, wi, smp.astype(np.float64))
    ok = s["margin"] > pc.MARGIN
    ev, _ = pr.eval_pdf(p, wi, s["wo"])
    assert np.allclose((s["weight"] * s["pdf"])[ok], ev[ok], rtol=1e-7, atol=1e-9)
    assert np.allclose(np.linalg.norm(s["wo"][ok], axis=1), 1, atol=1e-12)


CHI2 = [c for c in CONFIGS if c.label in ("tab5", "tab257", "rayleigh", "blend0.3(rayleigh,hg0.8)")]
CHI2_THRESHOLD = 1 - (1 - 0.01) ** (1 / len(CHI2))            # significance 0.01, Sidak-corrected over the cases


def chi2_inputs(n, seed):
    rng = np.random.default_rng(seed)
    wi = np.array([0.36, -0.48, 0.8])
    return np.broadcast_to(wi, (n, 3)).copy(), rng.random((n, 3))


@pytest.mark.parametrize("p", CHI2, ids=lambda p: p.label)
def test_chi2_of_the_reference_sampler(p):
    n = 200000
    wi, smp = chi2_inputs(n, 7)
    s = pr.sample(p, wi, smp)
    pv, stat, dof, mass = rr.chi2_test(s["wo"], lambda d: pr.eval_pdf(p, np.broadcast_to(wi[0], d.shape), d)[0], n, res=(32, 64))
    print(f"[phase chi2 ref] {p.label:28s} p = {pv:.4f}  chi2 = {stat:.1f}  dof = {dof}  mass = {mass:.6f}")
    assert pv > CHI2_THRESHOLD


@pytest.mark.parametrize("g, n", [(0.5, 257), (0.9, 1801), (-0.3, 65)])
def test_table_of_hg_is_hg_in_physics_convention(g, n):
    """A table whose nodes are hg_eval in physics convention, F(x) = hg_eval(g, -x) at x = cos(theta) with x = 1 forward, evaluates to
    analytic HG (pinned to the oracle, test_oracle_pins.py) within the bound of linear interpolation, h^2 / 8 max|F''|.
    F''(x) = 15 g^2 (1 - g^2) / (4 pi) (1 + g^2 - 2 g x)^-3.5 is positive and monotone, so an interval's ends bound it.  The table's
    normalisation is the trapezoid sum of the nodes; its distance from the analytic 2 pi has the bound 2 h^2 / 12 max|F''| and is
    asserted on its own.  A table read the other way round would miss by the difference of the forward and the backward lobe."""
    tab = pr.tabphase(pr.hg_table(g, n))
    rng = np.random.default_rng(3)
    wi = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (4096, 3))
    c = rng.uniform(-1, 1, 4096); phi = rng.uniform(0, 2 * np.pi, 4096); st = np.sqrt(1 - c * c)
    wo = np.stack([st * np.cos(phi), st * np.sin(phi), c], 1)           # graphics convention: c = dot(wo, wi)
    got, _ = pr.eval_pdf(tab, wi, wo)
    want = pr.hg_eval(g, c)
    F2 = lambda x: 15 * g * g * (1 - g * g) / (4 * np.pi) * (1 + g * g - 2 * g * x) ** -3.5
    h = 2.0 / (n - 1)
    x = -c; xl = np.floor((x + 1) / h) * h - 1
    interp_bound = h * h / 8 * np.maximum(F2(xl), F2(xl + h))
    k = float(tab.table.normalization) / (2 * np.pi)                    # 1 for an exact normalisation
    err = np.abs(got - want)
    assert (err <= interp_bound * k + want * abs(k - 1) + 8 * pr.EPS * want).all()          # (8 eps: the nodes are float32)
    assert abs(1 / float(tab.table.normalization) - 1 / (2 * np.pi)) <= 2 * h * h / 12 * max(F2(-1.0), F2(1.0)) + 4 * pr.EPS / (2 * np.pi)
    assert np.abs(got - pr.hg_eval(g, -c)).max() > 10 * err.max()       # the other convention is far away


def test_scalar_constructor_details():
    t = pr.Table("0,0,1,2,0")                                           # leading zero interval: valid starts at 1
    assert t.valid == (1, 3) and t.cdf.tolist() == [0.0, 0.25, 1.0, 1.5] and t.integral == 1.5 and t.interval_size == 0.5 and t.inv_interval_size == 2.0
    t = pr.Table("0,0,1,2,0,0,0")                                       # ... and trailing ones: valid ends at the last interval with mass
    assert t.valid == (1, 3) and t.integral == t.cdf[3] and t.cdf[5] == t.cdf[3]
    c, idx, _ = t.sample(np.array([0.0, 1e-9, 0.5, 1 - 2.0 ** -24]), np.float64)
    assert idx.tolist()[0] == 1 and (idx >= 1).all() and (idx <= 3).all() and c[0] == float(t.interval_size) - 1 and c[-1] < 4 * float(t.interval_size) - 1 + 1e-6
    t = pr.Table("1,1")                                                 # n = 2: one interval, no search trip, y0 == y1 takes the constant inversion
    assert t.valid == (0, 0) and t.cdf.tolist() == [2.0] and t.normalization == 0.5
    c, idx, tt = t.sample(np.array([0.0, 0.25, 0.75]), np.float64)
    assert idx.tolist() == [0, 0, 0] and np.allclose(c, [-1.0, -0.5, 0.5], atol=1e-15)
    assert np.allclose(t.eval_pdf_normalized(np.array([-1.0, 0.3, 1.0, 1.0000001, -1.5]), np.float64), [0.5, 0.5, 0.5, 0, 0])
    t = pr.Table("1,1,3,3,2")                                           # flat segments beside sloped ones
    c, idx, tt = t.sample(np.array([0.1, 0.3, 0.6, 0.9]), np.float64)
    def mass_below(x):                                                  # the interpolant's integral over [-1, x], trapezoid rule on a fine grid
        g = np.linspace(-1, x, 20001); y = np.interp(g, np.linspace(-1, 1, 5), t.values)
        return float(np.sum((y[1:] + y[:-1]) * 0.5 * np.diff(g)))
    u_back = np.array([mass_below(x) for x in c]) / float(t.integral)
    assert np.allclose(u_back, [0.1, 0.3, 0.6, 0.9], atol=1e-7) and set(idx.tolist()) == {0, 1, 2, 3}
    for bad, msg in (("1", "needs at least two entries"), ("1,-1", "non-negative"), ("0,0", "no probability mass"), ("1,z", "Could not parse")):
        with pytest.raises(ValueError, match=msg):
            pr.Table(bad)


# ------------------------------------------------------------------------------------------------------ the K table and the cap
_measured = {}


def measured(p):
    if p.label not in _measured:
        wi, smp, woq = pc.make_inputs(p)
        ref = pc.reference(p, wi, smp, woq)
        _measured[p.label] = (ref, pc.worst_ratios(ref, pc.float32_run(p, wi, smp, woq)))
    return _measured[p.label]


def test_k_table():
    """float32 against float64, both from tests/phase_ref.py, over every configuration: K = 4 x the worst ratio, rounded up to a power of two
    (DESIGN.md 15.4's method).  Printed as DESIGN.md section 16 shows it; a measurement that asks for another K than phase_cases.K fails."""
    worst = {k: 0.0 for k in pc.QUANTITIES}
    for p in CONFIGS:
        w = measured(p)[1]
        print(f"[phase K] {p.label:28s} " + "  ".join(f"{k} {v[0]:6.2f}" for k, v in w.items()))
        for k, v in w.items():
            worst[k] = max(worst[k], v[0])
    print("[phase K] worst " + "  ".join(f"{k} {v:.2f} -> K {pc.k_from(v):g}" for k, v in worst.items()))
    assert {k: pc.k_from(v) for k, v in worst.items()} == pc.K


@pytest.mark.parametrize("p", CONFIGS, ids=lambda p: p.label)
def test_one_percent_cap(p):
    """from the reference alone: the lanes within 1e-5 of a branch point (a table interval's ends in the interval's own coordinate, |cos| = 1;
    s1 is drawn 0.02 away from a blend's weight, so that branch leaves none out) are at most 1 % of the batch"""
    wi, smp, _ = pc.make_inputs(p)
    if p.kind == pr.BLEND:
        assert (np.abs(smp[:, 0].astype(np.float64) - float(p.weight)) >= pc.S1_GAP * (1 - 1e-6)).all()
    ref = measured(p)[0]
    left = max(int((~ref["sample_ok"]).sum()), int((~ref["eval_ok"]).sum()))
    print(f"[phase cap] {p.label:28s} left out {left} of {pc.N_LANES}")
    assert left <= pc.MAX_LEFT_OUT * pc.N_LANES
