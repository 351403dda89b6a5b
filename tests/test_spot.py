"""Spot and directional emitters on the host: what the loader reads and refuses, the description's round trip with
the plugins' defaults, the dictionary route, lrt_scene_from_desc's validation, and the float64 reference of tests/spot_ref.py held
against itself, so that the device checks of test_spot_gpu.py are known to be passable: the falloff's shape, the projection's uv, the
directional sample's geometry, the K table and the 1 % cap."""
import ctypes as C

import numpy as np
import pytest

import spot_cases as sc_
import spot_ref as sr

CASES = sc_.configs()
SPOT, DIRECTIONAL = 4, 5
HEAD = ('<scene version="3.0.0"><integrator type="{integrator}"/><sensor type="perspective"><film type="hdrfilm">'
        '<integer name="width" value="4"/><integer name="height" value="4"/></film></sensor><shape type="cube"/>')


def scene(mi, emitters, integrator="path"):
    return mi.load_string(HEAD.format(integrator=integrator) + emitters + "</scene>")


def emitters(sc):
    d = sc.desc
    return [type(d.emitters[i]).from_buffer_copy(d.emitters[i]) for i in range(d.n_emitters)]


# ------------------------------------------------------------------------------------------------- loader, description, load_dict
def test_version_and_xml_defaults(mi):
    assert mi._lib.lib().lrt_version() >= 117
    (E,) = emitters(scene(mi, '<emitter type="spot"/>'))
    assert E.type == SPOT and list(E.radiance) == [1.0, 1.0, 1.0] and E.cutoff_angle == 20.0 and E.beam_width == 15.0 and E.texture == -1
    assert np.array_equal(np.array(E.to_world).reshape(4, 4), np.eye(4))
    (E,) = emitters(scene(mi, '<emitter type="spot"><float name="cutoff_angle" value="30"/><rgb name="intensity" value="1, 2, 3"/>'
                              '<transform name="to_world"><translate x="1" y="2" z="3"/></transform></emitter>'))
    assert E.cutoff_angle == 30.0 and E.beam_width == np.float32(30.0) * np.float32(3.0) / np.float32(4.0) and list(E.radiance) == [1.0, 2.0, 3.0]
    assert [E.to_world[3], E.to_world[7], E.to_world[11]] == [1.0, 2.0, 3.0]
    (E,) = emitters(scene(mi, '<emitter type="directional"/>'))
    assert E.type == DIRECTIONAL and list(E.radiance) == [1.0, 1.0, 1.0] and np.array_equal(np.array(E.to_world).reshape(4, 4), np.eye(4))
    (E,) = emitters(scene(mi, '<emitter type="directional"><vector name="direction" value="1, -2, 0.5"/><rgb name="irradiance" value="3"/></emitter>'))
    m = np.array(E.to_world, np.float32).reshape(4, 4)
    assert np.array_equal(m, sr.look_at_direction((1.0, -2.0, 0.5))) and list(E.radiance) == [3.0, 3.0, 3.0]
    want = np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])
    assert np.abs(m[:3, 2] - want).max() <= 2 * sr.EPS and np.abs(m[:3, :3].astype(np.float64).T @ m[:3, :3] - np.eye(3)).max() <= 4 * sr.EPS
    # a medium child is ignored, as the point emitter ignores it
    (E,) = emitters(scene(mi, '<emitter type="spot"><medium type="homogeneous"/></emitter>'))
    assert E.type == SPOT


def test_checkerboard_texture(mi):
    sc = scene(mi, '<emitter type="spot"><texture type="checkerboard" name="texture"><transform name="to_uv"><scale x="4" y="4"/></transform></texture></emitter>')
    (E,) = emitters(sc)
    T = sc.desc.textures[E.texture]
    assert E.texture >= 0 and T.type == 1 and T.to_uv[0] == 4.0 and T.to_uv[4] == 4.0


def test_environment_count(mi):
    """neither is an environment emitter: a scene may hold both beside one sky, and still refuses a second sky"""
    both = '<emitter type="spot"/><emitter type="directional"/>'
    assert [e.type for e in emitters(scene(mi, both))] == [SPOT, DIRECTIONAL]
    assert [e.type for e in emitters(scene(mi, both + '<emitter type="constant"/>'))] == [SPOT, DIRECTIONAL, 2]
    assert [e.type for e in emitters(scene(mi, '<emitter type="constant"/>' + both))] == [2, SPOT, DIRECTIONAL]
    with pytest.raises(RuntimeError, match="Only one environment emitter can be specified per scene."):
        scene(mi, both + '<emitter type="constant"/><emitter type="constant"/>')


@pytest.mark.parametrize("emitter_xml, message", [
    ('<emitter type="directional"><vector name="direction" value="0, 0, 1"/><transform name="to_world"><translate x="1"/></transform></emitter>',
     "Only one of the parameters 'direction' and 'to_world' can be specified at the same time!"),
    ('<emitter type="directional"><texture type="checkerboard" name="irradiance"/></emitter>', "Expected a non-spatially varying irradiance spectra!"),
    ('<emitter type="spot"><rgb name="texture" value="0.5"/></emitter>', r"The parameter 'texture' must be spatially varying \(e.g. bitmap type\)!"),
    ('<emitter type="spot"><texture type="rgb" name="texture"><rgb name="color" value="0.5"/></texture></emitter>',
     r"The parameter 'texture' must be spatially varying \(e.g. bitmap type\)!"),
    ('<emitter type="spot"><texture type="bitmap" name="texture"><string name="filename" value="none.png"/></texture></emitter>',
     "unsupported: a bitmap texture as the spot emitter's 'texture'"),
    ('<emitter type="spot"><texture type="checkerboard" name="intensity"/></emitter>', r"The parameter 'intensity' cannot be spatially varying \(e.g. bitmap type\)!"),
    ('<emitter type="spot"><float name="beam_width" value="25"/></emitter>', "0 < beam_width <= cutoff_angle <= 180"),
    ('<emitter type="spot"><float name="beam_width" value="0"/></emitter>', "0 < beam_width <= cutoff_angle <= 180"),
    ('<emitter type="spot"><float name="cutoff_angle" value="181"/></emitter>', "0 < beam_width <= cutoff_angle <= 180"),
    ('<emitter type="spot"><float name="cutoff_angle" value="-5"/></emitter>', "0 < beam_width <= cutoff_angle <= 180"),
    ('<emitter type="spot"><float name="cutoff_angle" value="90"/><texture type="checkerboard" name="texture"/></emitter>', "cutoff_angle must be below 90 degrees when a texture is given"),
    ('<emitter type="spot"><transform name="to_world"><scale x="0"/></transform></emitter>', "spot emitter: to_world must be finite and invertible"),
    ('<emitter type="directional"><transform name="to_world"><scale z="0"/></transform></emitter>', "directional emitter: to_world must be finite and invertible"),
    ('<emitter type="projector"/>', 'unsupported emitter type "projector"'),
])
def test_loader_errors(mi, emitter_xml, message):
    with pytest.raises(RuntimeError, match=message):
        scene(mi, emitter_xml)


def test_bitmap_texture_is_unsupported_status(mi):
    L = mi._lib.lib()
    xml = (HEAD.format(integrator="path") + '<emitter type="spot"><texture type="bitmap" name="texture"><string name="filename" value="none.png"/></texture></emitter></scene>').encode()
    h = C.c_void_p()
    assert L.lrt_scene_load_xml_string(xml, b".", None, 0, C.byref(h)) == mi._lib.UNSUPPORTED
    assert "'texture'" in L.lrt_last_error().decode()


@pytest.mark.parametrize("kind", ["spot", "directional"])
def test_prbvolpath_is_refused(mi, kind):
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath on a scene with a spot or directional emitter"):
        scene(mi, f'<emitter type="{kind}"/>', integrator="prbvolpath")


def test_load_dict_round_trip(mi):
    d = {"type": "scene", "integrator": {"type": "path"},
         "sensor": {"type": "perspective", "film": {"type": "hdrfilm", "width": 4, "height": 4}},
         "box": {"type": "cube"},
         "lamp": {"type": "spot", "intensity": [1.0, 2.0, 3.0], "cutoff_angle": 40.0,
                  "to_world": mi.ScalarTransform4f().translate([0.0, 0.0, 3.0]),
                  "texture": {"type": "checkerboard", "to_uv": mi.ScalarTransform4f().scale([4.0, 4.0, 1.0])}},
         "sun": {"type": "directional", "irradiance": 2.0, "direction": [0.0, -1.0, 0.25]}}
    xml = mi.dict_to_xml(d)
    assert '<emitter type="spot" id="lamp">' in xml and '<texture type="checkerboard" name="texture">' in xml and '<vector name="direction" value="0.0, -1.0, 0.25"/>' in xml
    lamp, sun = emitters(mi.load_dict(d))
    assert (lamp.type, lamp.cutoff_angle, lamp.beam_width, list(lamp.radiance), lamp.to_world[11]) == (SPOT, 40.0, 30.0, [1.0, 2.0, 3.0], 3.0) and lamp.texture >= 0
    assert sun.type == DIRECTIONAL and list(sun.radiance) == [2.0, 2.0, 2.0]
    assert np.array_equal(np.array(sun.to_world, np.float32).reshape(4, 4), sr.look_at_direction((0.0, -1.0, 0.25)))
    same = emitters(mi.load_string(xml))
    assert [(e.type, e.cutoff_angle, e.beam_width, e.texture) for e in same] == [(e.type, e.cutoff_angle, e.beam_width, e.texture) for e in (lamp, sun)]


def test_scene_from_desc_validation(mi):
    from liverrenderer_amd import _lib
    base = scene(mi, sc_.emitter_xml(CASES[5].light) + '<emitter type="directional"/>')            # a spot with a checkerboard, a directional light
    L = _lib.lib()
    n_tex = base.desc.n_textures

    def attempt(mutate):
        d = _lib.SceneDesc.from_buffer_copy(base.desc)
        em = (_lib.EmitterDesc * d.n_emitters)(*[d.emitters[i] for i in range(d.n_emitters)])
        tx = (_lib.TextureDesc * d.n_textures)(*[d.textures[i] for i in range(d.n_textures)])
        d.emitters = C.cast(em, C.POINTER(_lib.EmitterDesc)); d.textures = C.cast(tx, C.POINTER(_lib.TextureDesc))
        mutate(em, tx)
        h = C.c_void_p()
        st = L.lrt_scene_from_desc(C.byref(d), C.byref(h))
        if st == 0:
            L.lrt_scene_free(h)
        return st, L.lrt_last_error().decode()

    def setter(i, **kw):
        def f(em, tx):
            for k, v in kw.items():
                setattr(em[i], k, v)
        return f

    def world(i, k, v):
        def f(em, tx):
            em[i].to_world[k] = v
        return f

    texel = (C.c_float * 1)(0.5)

    def tex_type(t):
        def f(em, tx):
            T = tx[em[0].texture]
            T.type = t
            if t == 2:                                                                 # a valid 1 x 1 bitmap
                T.width = T.height = T.channels = 1; T.data = C.cast(texel, C.POINTER(C.c_float))
        return f

    assert attempt(lambda em, tx: None)[0] == 0
    assert attempt(setter(0, texture=-1, cutoff_angle=180.0, beam_width=180.0))[0] == 0
    INVALID, UNSUPPORTED = _lib.INVALID, _lib.UNSUPPORTED
    for mutate, status, text in [
            (setter(0, type=6), INVALID, "invalid emitter type"), (setter(0, type=-1), INVALID, "invalid emitter type"),
            (setter(0, beam_width=0.0), INVALID, "0 < beam_width <= cutoff_angle <= 180"),
            (setter(0, beam_width=41.0), INVALID, "0 < beam_width <= cutoff_angle <= 180"),
            (setter(0, cutoff_angle=float("nan")), INVALID, "0 < beam_width <= cutoff_angle <= 180"),
            (setter(0, cutoff_angle=200.0, beam_width=10.0, texture=-1), INVALID, "0 < beam_width <= cutoff_angle <= 180"),
            (setter(0, cutoff_angle=90.0), INVALID, "cutoff_angle must be below 90 degrees when a texture is given"),
            (setter(0, texture=n_tex), INVALID, "spot emitter references an invalid texture"),
            (setter(0, texture=-2), INVALID, "spot emitter references an invalid texture"),
            (tex_type(0), INVALID, "The parameter 'texture' must be spatially varying"),
            (tex_type(2), UNSUPPORTED, "unsupported: a bitmap texture as the spot emitter's 'texture'"),
            (world(0, 3, float("inf")), INVALID, "spot emitter: to_world must be finite and invertible"),
            (world(1, 10, 0.0), INVALID, "directional emitter: to_world must be finite and invertible")]:
        st, msg = attempt(mutate)
        assert st == status and text in msg, (st, msg, text)
    # a zero-filled tail, as a description from before the fields has it, means what it meant for the other types
    sky = scene(mi, '<emitter type="constant"/>')
    d = _lib.SceneDesc.from_buffer_copy(sky.desc)
    em = (_lib.EmitterDesc * 1)(d.emitters[0]); em[0].cutoff_angle = 0.0; em[0].beam_width = 0.0; em[0].texture = 0
    d.emitters = C.cast(em, C.POINTER(_lib.EmitterDesc))
    h = C.c_void_p()
    assert L.lrt_scene_from_desc(C.byref(d), C.byref(h)) == 0
    L.lrt_scene_free(h)


# ------------------------------------------------------------------------------------------------- the reference against itself
def test_falloff_shape():
    for case in CASES:
        e = case.light
        if e.kind != "spot":
            continue
        cutoff, beam = float(e.cutoff), float(e.beam)
        theta = np.concatenate([[0.0], np.linspace(0.0, min(cutoff + 0.5, np.pi), 20001)])
        d = np.stack([np.sin(theta), np.zeros_like(theta), np.cos(theta)], 1)
        f, _ = e.falloff_curve(d * 3.7, np.float64)                                  # (any length: the curve normalises)
        assert f[0] == 1.0 and (f[theta < beam - 1e-6] == 1.0).all() and (f[theta >= cutoff + 1e-6] == 0.0).all()
        assert (np.diff(f[1:]) <= 1e-12).all() and f.min() >= 0.0 and f.max() <= 1.0 + 1e-6             # monotone in the angle
        if beam < cutoff:                                                            # continuous: no step larger than the grid's slope allows
            step = (theta[2] - theta[1]) / (cutoff - beam)
            assert np.abs(np.diff(f[1:])).max() <= step * (1 + 1e-3) + 4 * sr.EPS * float(e.inv_transition)
            mid = np.array([[np.sin((beam + cutoff) / 2), 0.0, np.cos((beam + cutoff) / 2)]])
            assert abs(e.falloff_curve(mid, np.float64)[0][0] - 0.5) <= 1e-5
            at = np.array([[np.sqrt(1 - float(e.cos_cutoff) ** 2), 0.0, float(e.cos_cutoff)]])      # at the cutoff, as the host's float32 cosine places it
            assert e.falloff_curve(at, np.float64)[0][0] <= 1e-5
        beyond = np.array([[np.sin(cutoff + 4e-6), 0.0, np.cos(cutoff + 4e-6)]])                     # (the float32 cosine moves the edge by up to 1e-6 rad at 5 degrees)
        assert e.falloff_curve(beyond, np.float64)[0][0] == 0.0


def test_direction_to_uv_maps_the_rim_to_the_inscribed_circle():
    e = CASES[5].light
    phi = np.linspace(0, 2 * np.pi, 721)
    c = float(e.cutoff)
    rim = np.stack([np.sin(c) * np.cos(phi), np.sin(c) * np.sin(phi), np.full_like(phi, np.cos(c))], 1) * 2.5
    uv = e.direction_to_uv(rim, np.float64)
    assert np.abs(np.hypot(uv[:, 0] - 0.5, uv[:, 1] - 0.5) - 0.5).max() <= 4 * sr.EPS                  # (tan is the host's float32 one)
    assert np.allclose(e.direction_to_uv(np.array([[0.0, 0.0, 1.0]]), np.float64), [[0.5, 0.5]], atol=0)
    tex, _ = e.texture.eval(np.array([[0.05, 0.05], [0.2, 0.05], [0.2, 0.2], [0.55, 0.55]]), np.float64)       # to_uv scale 4: tiles of 1/8
    assert tex[:, 0].tolist() == [float(e.texture.color0[0]), float(e.texture.color1[0]), float(e.texture.color0[0]), float(e.texture.color0[0])]


def test_directional_sample_geometry():
    for case in CASES:
        e = case.light
        if e.kind != "directional":
            continue
        ref, _ = sc_.make_inputs(case)
        s = e.sample_direction(ref)
        d = e.d.astype(np.float64)
        assert abs(np.linalg.norm(d) - 1) <= 4 * sr.EPS
        radius = np.maximum(float(e.radius), np.linalg.norm(ref.astype(np.float64) - e.center, axis=1))
        assert np.array_equal(s["dist"], 2 * radius) and np.array_equal(s["d"], np.broadcast_to(-d, s["d"].shape)) and np.array_equal(s["n"], -s["d"])
        assert np.abs((ref - s["p"]) - d * (2 * radius)[:, None]).max() <= 1e-12 * s["dist"].max()    # p lies 2 radius from ref against d
        inside = np.linalg.norm(ref.astype(np.float64) - e.center, axis=1) < float(e.radius)
        assert 0.4 < inside.mean() < 0.6 and (s["dist"][inside] == 2 * float(e.radius)).all() and (s["weight"] == e.irradiance.astype(np.float64)).all()


@pytest.mark.parametrize("case", [c for c in CASES if c.light.kind == "spot"], ids=lambda c: c.label)
def test_inputs_cover_core_ring_and_dark(case):
    e = case.light
    ref, _ = sc_.make_inputs(case)
    s = e.sample_direction(ref)
    core, dark = (s["falloff"] == 1.0).mean(), (s["falloff"] == 0.0).mean()
    ring = 1 - core - dark
    on_axis = np.abs(s["cos"][:sc_.N_AXIS] - 1) <= 4 * sr.EPS
    print(f"[spot inputs] {case.label:14s} core {core:.3f} ring {ring:.3f} dark {dark:.3f}")
    assert on_axis.all() and len(ref) == sc_.N_LANES
    if float(e.beam) == float(e.cutoff):
        assert ring == 0 and core >= 0.45 and dark >= 0.45
        assert (np.abs(np.arccos(np.clip(s["cos"], -1, 1)) - float(e.cutoff)) >= sc_.STEP_GAP * 0.99)[sc_.N_AXIS:].all()
    else:
        assert core >= 0.25 and ring >= 0.25 and dark >= 0.25


# ------------------------------------------------------------------------------------------------------ the K table and the cap
_measured = {}


def measured(case):
    if case.label not in _measured:
        ref_p, smp = sc_.make_inputs(case)
        ref = sc_.reference(case, ref_p, smp)
        _measured[case.label] = (ref, sc_.worst_ratios(ref, sc_.float32_run(case, ref_p, smp)))
    return _measured[case.label]


def test_k_table():
    """float32 against float64, both from tests/spot_ref.py, over every configuration: K = 4 x the worst ratio, rounded up to a power of two
    (the project's margin).  Printed as DESIGN.md section 17 shows it; a measurement that asks for another K than
    spot_cases.K fails."""
    worst = {k: 0.0 for k in sc_.QUANTITIES}
    for case in CASES:
        w = measured(case)[1]
        print(f"[spot K] {case.label:14s} " + "  ".join(f"{k} {v:6.2f}" for k, v in w.items()))
        for k, v in w.items():
            worst[k] = max(worst[k], v)
    print("[spot K] worst " + "  ".join(f"{k} {v:.2f} -> K {sc_.k_from(v):g}" for k, v in worst.items()))
    assert {k: sc_.k_from(v) for k, v in worst.items()} == sc_.K


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.label)
def test_one_percent_cap(case):
    """from the reference alone: the lanes within 1e-5 (in uv) of a checkerboard tile edge are at most 1 % of the batch; the falloff is
    continuous and leaves none out, and the step of beam_width == cutoff_angle is kept clear of by the inputs"""
    ref = measured(case)[0]
    left = int((~ref["ok"]).sum())
    print(f"[spot cap] {case.label:14s} left out {left} of {sc_.N_LANES}")
    assert left <= sc_.MAX_LEFT_OUT * sc_.N_LANES
    if getattr(case.light, "texture", None) is None:
        assert left == 0
