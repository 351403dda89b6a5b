"""The perspective sensor and the film without a GPU: tests/sensor_ref.py against itself, the oracle's sensor probe
against it, the reference's own test vectors (tests/golden/sensor_film_known_answers.json) on sensor_ref, the loader and the oracle, the
oracle's develop and its film under wide Gaussians, and what the loader and lrt_scene_from_desc refuse.  test_sensor_gpu.py runs the
same checks on the device."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import sensor_cases as sc
import sensor_ref as sr

U = 2.0 ** -24
KNOWN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sensor_film_known_answers.json")))
# probe cases: every sensor with a filter of its own, and sensor (c), the crop window, with every filter
PROBE_CASES = [("a", "box"), ("b", "tent1"), ("d", "tent2.5"), ("e170", "gaussian1"), ("e1", "gaussian2")] + [("c", f) for f in sc.FILTERS]
RAY_FIELDS, FILM_FIELDS = ("d", "o", "maxt"), ("adjusted", "rel", "weight")


def allclose(a, b, rtol=KNOWN["allclose_default"]["rtol"], atol=KNOWN["allclose_default"]["atol"]):
    return bool(np.all(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) <= atol + rtol * np.abs(np.asarray(b, np.float64))))


def same_bits(a, b):
    """bit for bit, a NaN equal to a NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


@functools.lru_cache(maxsize=None)
def load(mi, sensor, rfilter, integrator="path", fmt="rgba", spp=4):
    return mi.load_dict(sc.scene_dict(mi, sensor, rfilter, integrator, fmt, spp))


# ------------------------------------------------------------------------------------- the restatement, in two precisions
def reference_record(cam, rfilter, inp, dt=np.float64):
    """sensor_ref's record for probe inputs inp (n, 5), with each field's conditioning: {field: (value, scale)}"""
    kind, param = sc.filter_spec(rfilter)
    ax, ay, spx, spy, x = (inp[:, k].astype(dt) for k in range(5))
    o, d, maxt = sr.sample_ray(cam, ax, ay, dt)
    o64, d64, maxt64 = (o, d, maxt) if dt is np.float64 else sr.sample_ray(cam, ax.astype(np.float64), ay.astype(np.float64))
    inv_z = 1.0 / (d64 @ cam.to_world[:3, :3])[:, 2]                                              # camera-space z of the unit direction
    n, count, org, rel = sr.footprint(kind, param, spx, spy, dt)
    w = sr.rfilter(kind, param, x, dt)
    wscale = np.abs(sr.gaussian_terms(x.astype(np.float64), param)).sum(-1) if kind == sr.GAUSSIAN else np.ones(len(x))
    return {"d": (d, np.ones((len(x), 1))), "o": (o, (np.abs(cam.to_world[:3, 3]).max() + cam.near * inv_z)[:, None]), "maxt": (maxt, cam.far * inv_z),
            "adjusted": (np.stack(sr.film_to_sample(cam, spx, spy, dt), -1), np.ones((len(x), 1))),
            "rel": (rel, np.abs(np.stack([spx, spy], -1).astype(np.float64)) + n + 0.5), "weight": (w, wscale),
            "origin": (org, None), "fcount": (np.full(len(x), count), None)}


@functools.lru_cache(maxsize=None)
def k_table():
    """K per field: the largest conditioned error of sensor_ref's own formulas in float32 against float64 over the probe
    cases, in units of 2^-24, at least 1/2.  The weight's K is kept per filter kind (the box filter has none: it must be equal)."""
    K = {}
    for sensor, rfilter in PROBE_CASES:
        cam = sc.expected_camera(sensor); inp = sc.probe_inputs(sensor, rfilter)
        r64, r32 = reference_record(cam, rfilter, inp), reference_record(cam, rfilter, inp, np.float32)
        for f in RAY_FIELDS + FILM_FIELDS:
            key = f if f != "weight" else ("weight", sc.filter_spec(rfilter)[0])
            err = np.max(np.abs(r32[f][0].astype(np.float64) - r64[f][0]) / r64[f][1]) / U
            K[key] = max(K.get(key, 0.5), float(err))
    K["weight", sr.BOX] = 0.0
    return K


def check_probe(got, sensor, rfilter, who, cam=None):
    """A probe's record `got` against sensor_ref: decisions equal on every lane, values within 4 K.  Returns the worst figure per field."""
    cam = cam or sc.expected_camera(sensor); inp = sc.probe_inputs(sensor, rfilter)
    ref = reference_record(cam, rfilter, inp); K = k_table(); worst = {}
    assert np.array_equal(got["origin"], ref["origin"][0]) and np.array_equal(got["fcount"], ref["fcount"][0]), (who, sensor, rfilter, "footprint")
    for f in RAY_FIELDS + FILM_FIELDS:
        k = K[f if f != "weight" else ("weight", sc.filter_spec(rfilter)[0])]
        e = np.abs(got[f].astype(np.float64) - ref[f][0]) / ref[f][1] / U
        worst[f] = float(np.max(e))
        print(f"{who} {sensor}/{rfilter} {f}: worst {worst[f]:.2f} x 2^-24 (K {k:.2f}, bound {4 * k:.2f})")
        assert worst[f] <= 4 * k, (who, sensor, rfilter, f, worst[f], 4 * k, int(np.argmax(e.reshape(len(inp), -1).max(-1))))
    return worst


# ---------------------------------------------------------------------------------------------------------------- API
def test_api(mi):
    assert mi._lib.lib().lrt_version() >= 120 and "lrt_sensor_probe" in mi._lib.EXPORTED_SYMBOLS
    assert mi._lib.SENSOR_PROBE_FLOATS == 16


# ------------------------------------------------------------------------------------------ sensor_ref against itself
@pytest.mark.parametrize("sensor", sorted(sc.SENSORS))
def test_reference_checks_itself(sensor):
    """sample_ray through the inverted matrix product against the geometric statement; the origin on the near plane, the end on the far one"""
    cam = sc.expected_camera(sensor); inp = sc.probe_inputs(sensor, "box").astype(np.float64)
    o, d, maxt = sr.sample_ray(cam, inp[:, 0], inp[:, 1])
    dc, dw = sr.geometric_direction(cam, inp[:, 0], inp[:, 1])
    err = np.abs(dw - d).max()
    print(f"{sensor}: |sample_ray.d - geometric| <= {err:.3g}")
    assert err <= 1e-12 and np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 4 * U                # (the frame is a float32 look_at)
    R, t = cam.to_world[:3, :3], cam.to_world[:3, 3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6                                                 # float32 look_at
    depth = lambda p: (p - t) @ R[:, 2] / (R[:, 2] @ R[:, 2])
    assert np.allclose(depth(o), cam.near, rtol=1e-6) and np.allclose(depth(o + d * maxt[:, None]), cam.far, rtol=1e-6)
    # the mirrors: the film's left edge looks to the camera's +x (left), its top to +y (up)
    assert dc[np.argmin(inp[:, 0]), 0] > dc[np.argmax(inp[:, 0]), 0] and dc[np.argmin(inp[:, 1]), 1] > dc[np.argmax(inp[:, 1]), 1]


def test_remez_fit_error():
    """The polynomial against exp(-x^2 / 2 stddev^2) - exp(-8) on [0, 4 stddev].  The bound is the fit's own error: a minimax fit to
    exp(-x / 2) shifted to vanish at 16 errs by 1 - exp(-8) - coeff[0] = 4.04e-4 at 0, and nowhere by more than 1.1 times that."""
    at0 = abs(1.0 - np.exp(-8.0) - sr.REMEZ[0])
    for stddev in (0.5, 1.0, 2.0):
        x = np.linspace(0.0, 4.0 * stddev, 20001)
        err = np.abs(sr.rfilter(sr.GAUSSIAN, stddev, x) - sr.gaussian_ideal(x, stddev)).max()
        print(f"stddev {stddev}: max |polynomial - ideal| on [0, 4 stddev] = {err:.3e} (error at 0: {at0:.3e})")
        assert 0.9 * at0 <= err <= 1.1 * at0
        assert sr.rfilter(sr.GAUSSIAN, stddev, np.array([4.0 * stddev]))[0] <= 1e-12 and np.all(sr.rfilter(sr.GAUSSIAN, stddev, np.array([4.001 * stddev, -5.0 * stddev])) == 0)
    print(f"f(0.2) at the default stddev: {sr.rfilter(sr.GAUSSIAN, 0.5, np.array([0.2]))[0]:.5f}")


def test_k_table_is_finite():
    K = k_table()
    for k, v in sorted(K.items(), key=str):
        print(f"K[{k}] = {v:.2f}")
    assert all(np.isfinite(v) for v in K.values()) and K["weight", sr.TENT] < 4 and K["d"] < 64 and K["adjusted"] < 4 and K["rel"] < 4


# ------------------------------------------------------------------------------------------------- the known answers
@pytest.mark.parametrize("case", KNOWN["parse_fov"]["cases"], ids=lambda c: "-".join(f"{v}" for v in c["props"].values()) + f"-{c['aspect']}")
def test_parse_fov_known_answers(mi, case):
    """test_sensor.py:5-45 on sensor_ref and, through a loaded sensor's fov_x, on the loader (XML and dictionary are one parser)"""
    p = case["props"]
    assert allclose(sr.parse_fov(case["aspect"], p.get("fov"), p.get("fov_axis", "x"), p.get("focal_length")), case["value"])
    w, h = {0.5: (8, 16), 1.0: (8, 8), 1.5: (12, 8)}[case["aspect"]]
    s = dict(sc.SENSORS["a"], film=(w, h), fov=dict(p))
    assert allclose(mi.load_dict(sc.scene_dict(mi, s, "box")).desc.sensor.fov_x, case["value"])


@pytest.mark.parametrize("sensor", sorted(sc.SENSORS))
def test_loader_sensor(mi, sensor):
    """What the loader stores against the case's own parameters through sensor_ref: fov_x to one float32 ulp, the rest equal"""
    got = sr.Camera.from_desc(load(mi, sensor, "gaussian1").desc); want = sc.expected_camera(sensor)
    assert abs(got.fov_x - want.fov_x) <= np.spacing(np.float32(want.fov_x)) and np.array_equal(got.to_world, want.to_world)
    assert (got.near, got.far, got.film, got.crop, got.offset, got.ppo) == (want.near, want.far, want.film, want.crop, want.offset, want.ppo)
    F = load(mi, sensor, "gaussian1").desc.film
    assert (F.rfilter, F.rfilter_param) == (sr.GAUSSIAN, 1.0)


KNOWN_FILTERS = {"box": "box", "gaussian": "gaussian0.5", "tent": "tent1"}           # the plugins' defaults


def check_known_filters(probe_of):
    """test_rfilter.py test01, 02, 06; probe_of(sensor, rfilter, inputs) -> record"""
    for c in KNOWN["rfilter"]["cases"]:
        kind, param = sc.FILTERS[KNOWN_FILTERS[c["filter"]]]
        inp = np.zeros((2, 5), np.float32); inp[:, 4] = c["x"], -c["x"]
        got = probe_of("a", KNOWN_FILTERS[c["filter"]], inp)["weight"]
        for v in (sr.rfilter(kind, param, np.float64(np.float32(c["x"]))), got[0], got[1]):
            assert abs(float(v) - c["value"]) <= c["atol"], (c, v)


def known_camera(origin, direction, fov, axis):
    P = KNOWN["perspective"]
    return dict(film=tuple(P["film"]), fov=dict(fov=fov, fov_axis=axis), look=(origin, [o + d for o, d in zip(origin, direction)], P["up"]),
                clip=(P["near_clip"], P["far_clip"]))


def check_known_perspective(probe_of):
    """test_perspective.py test02 and test04"""
    P = KNOWN["perspective"]; S = P["sample_ray"]
    for origin in P["origins"]:
        for direction in P["directions"]:
            s = known_camera(origin, direction, S["fov"], S["fov_axis"])
            inp = np.zeros((1 + len(S["position_samples"]), 5), np.float32); inp[0, :2] = S["centre"]; inp[1:, :2] = S["position_samples"]
            cam = sc.expected_camera(s)
            for rec in (dict(zip(("o", "d", "maxt"), sr.sample_ray(cam, inp[:, 0].astype(np.float64), inp[:, 1].astype(np.float64)))), probe_of(s, "box", inp)):
                assert allclose(rec["d"][0], direction, rtol=KNOWN["allclose_default"]["rtol"], atol=S["atol_d"])
                inv_z = 1.0 / (rec["d"].astype(np.float64) @ cam.to_world[:3, :3])[:, 2]          # (world_transform.inverse() @ ray.d).z
                assert allclose(rec["o"], np.asarray(origin) + P["near_clip"] * inv_z[:, None] * rec["d"], rtol=KNOWN["allclose_default"]["rtol"], atol=S["atol_o"])
    A = P["fov_axis"]
    for fov in A["fovs"]:
        for direction in P["directions"]:
            for e in A["extremities"]:
                for axis in e["axes"]:
                    s = known_camera(A["origin"], direction, fov, axis)
                    inp = np.zeros((len(e["samples"]), 5), np.float32); inp[:, :2] = e["samples"]
                    cam = sc.expected_camera(s)
                    for d in (sr.sample_ray(cam, inp[:, 0].astype(np.float64), inp[:, 1].astype(np.float64))[1], probe_of(s, "box", inp)["d"]):
                        assert allclose(np.degrees(np.arccos(d.astype(np.float64) @ np.asarray(direction))), fov / 2), (fov, axis, direction)


def check_known_imageblock(probe_of):
    """test_imageblock.py test03 on the probe's footprint and weights: one sample at (1.5, 1.5) into a 3 x 3 block"""
    B = KNOWN["imageblock"]
    for name in B["filters"]:
        rfilter = KNOWN_FILTERS[name]
        inp = np.zeros((1, 5), np.float32); inp[0, 2:4] = B["position"]
        fp = probe_of("a", rfilter, inp)
        count, (x0, y0) = int(fp["fcount"][0]), fp["origin"][0]
        lanes = np.zeros((2 * count + 2, 5), np.float32)
        lanes[:count, 4] = fp["rel"][0, 0] + np.arange(count, dtype=np.float32); lanes[count:2 * count, 4] = fp["rel"][0, 1] + np.arange(count, dtype=np.float32)
        lanes[2 * count:, 4] = 0.0, 1.0
        w = probe_of("a", rfilter, lanes)["weight"].astype(np.float64)
        wx, wy, (a, b) = w[:count], w[count:2 * count], w[2 * count:]
        block = np.array([[wy[y - y0] * wx[x - x0] if 0 <= y - y0 < count and 0 <= x - x0 < count else 0.0 for x in range(B["size"][0])] for y in range(B["size"][1])])
        c = b * b
        assert allclose(block, [[c, b, c], [b, a, b], [c, b, c]], rtol=KNOWN["allclose_default"]["rtol"], atol=B["atol"]), (name, block)
        assert a > 0.5 and (b > 0) == (name == "gaussian")


def oracle_probe_of(mi, orc):
    return lambda sensor, rfilter, inp: orc.OrcScene(mi.load_dict(sc.scene_dict(mi, sensor, rfilter))).sensor_probe(inp)


def test_known_filters_oracle(mi, orc):
    check_known_filters(oracle_probe_of(mi, orc))


def test_known_perspective_oracle(mi, orc):
    check_known_perspective(oracle_probe_of(mi, orc))


def test_known_imageblock_oracle(mi, orc):
    check_known_imageblock(oracle_probe_of(mi, orc))


# ------------------------------------------------------------------------------------- the oracle's probe and float64
@pytest.mark.parametrize("sensor,rfilter", PROBE_CASES)
def test_oracle_probe_matches_float64(mi, orc, sensor, rfilter):
    scene = load(mi, sensor, rfilter)
    check_probe(orc.OrcScene(scene).sensor_probe(sc.probe_inputs(sensor, rfilter)), sensor, rfilter, "oracle")


def test_inputs_cover_the_cases():
    for sensor, rfilter in PROBE_CASES:
        inp = sc.probe_inputs(sensor, rfilter); s = sc.SENSORS[sensor]; w, h = s["film"]
        cw, ch, cx, cy = s.get("crop") or (w, h, 0, 0); r = np.float32(sr.radius(*sc.FILTERS[rfilter]))
        assert {0.0, 0.5, 1.0} <= set(inp[:, 0].tolist()) and {0.0, 0.5, 1.0} <= set(inp[:, 1].tolist())
        assert np.any(inp[:, 2] == cx) and np.any(inp[:, 2] == cx + cw) and np.any(inp[:, 2] == np.float32(cx + 0.5)) and np.any(inp[:, 2] == np.nextafter(np.float32(cx + 0.5), np.float32(0)))
        assert np.any(np.floor(inp[:, 3]) == cy) and np.any(np.floor(inp[:, 3]) == cy + ch - 1)
        for v in (0.0, 0.2, -0.2, 0.49, 0.51, r, np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(9)), 1.5 * r):
            assert np.any(inp[:, 4] == np.float32(v)), (sensor, rfilter, v)


# ------------------------------------------------------------------------------------------------------------ develop
W_VALUES = [1.0, 3.5, 0.0, -0.0, 1.401298464324817e-45, -2.0, np.inf, np.nan, 7.0, 1e-30, 6e-39]
COLOURS = [0.25, 1.5, -3.0, np.inf, -np.inf, np.nan, 1.401298464324817e-45, 2e-39, 0.0, 1e30, 3.0, 1e-38, 0.1]


def crafted_film(h, w, channels):
    """A raw film whose weight takes every value of W_VALUES beside every residue of the colours' cycle (13 and 11 are coprime)"""
    film = np.empty((h, w, channels), np.float32); n = h * w
    film[..., -1] = np.resize(np.array(W_VALUES, np.float32), n).reshape(h, w)
    film[..., :-1] = np.resize(np.array(COLOURS, np.float32), n * (channels - 1)).reshape(h, w, channels - 1)
    return film


def check_develop(develop_of):
    """develop_of(sensor, fmt, film) -> image, against numpy's float32 film / where(W == 0, 1, W), bit for bit"""
    for sensor in ("b", "c", "d"):
        for fmt, channels in (("rgb", 4), ("rgba", 5)):
            crop = sc.expected_camera(sensor).crop
            film = crafted_film(crop[1], crop[0], channels)
            assert len(film.reshape(-1, channels)) >= len(W_VALUES)
            got, want = develop_of(sensor, fmt, film), sr.develop(film)
            bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
            assert got.shape == want.shape and not bad.any(), (sensor, fmt, [(film.reshape(-1, channels)[i // (channels - 1)], got.reshape(-1)[i], want.reshape(-1)[i])
                                                                               for i in np.flatnonzero(bad.reshape(-1))[:6]])


def test_develop_oracle(mi, orc):
    check_develop(lambda sensor, fmt, film: orc.OrcScene(load(mi, sensor, "box", "path", fmt)).develop(film))
    scene = load(mi, "c", "tent1", "path", "rgba", 4)
    img, raw = orc.OrcScene(scene).render(return_raw=True)
    assert same_bits(img, sr.develop(raw)) and raw[..., -1].min() > 0


# ------------------------------------------------------------------------------- the oracle's film under wide Gaussians
def lane_jitter(orc, scene, n, seed=0):
    d = scene.desc; L = orc.lib(); out = (C.c_float * 2)(); jit = np.empty((n, 2), np.float32)
    for lane in range(n):
        L.orc_lane_stream(d.sampler_seed, seed, lane, 2, out)
        jit[lane] = out[0], out[1]
    return jit


@pytest.mark.parametrize("rfilter,cells", [("gaussian2", 17), ("gaussian3", 25)])
def test_oracle_film_wide_gaussian(mi, orc, rfilter, cells):
    """ImageBlock::put with more than 16 cells per side: the oracle's 9 x 5 film against the float64 accumulation of its own lanes"""
    spp = 4
    scene = load(mi, "b", rfilter, "path", "rgba", spp); O = orc.OrcScene(scene); F = scene.desc.film
    kind, param = sc.filter_spec(rfilter)
    assert sr.footprint(kind, param, [0.0], [0.0])[1] == cells and (F.crop_width, F.crop_height) == (9, 5)
    _, raw = O.render(return_raw=True)
    n = 9 * 5 * spp; pix = np.arange(n) // spp; jit = lane_jitter(orc, scene, n)
    spx, spy = np.float32(pix % 9) + jit[:, 0], np.float32(pix // 9) + jit[:, 1]
    lanes = O.render_samples(0, n)
    rec = np.concatenate([lanes, np.ones((n, 1), np.float32)], axis=1)
    args = (kind, param, (9, 5), (0, 0), spx, spy)
    want = sr.accumulate(*args, rec); mag = sr.accumulate(*args, np.abs(rec))
    # n sequential float32 additions of products rounded twice: (n + 2) 2^-24 of the sum of magnitudes.  The weights are the oracle's: within
    # 4 K 2^-24 of float64 relative to the sum of the polynomial's absolute terms S (test_oracle_probe_matches_float64), which is far more
    # than the weight near the radius, so that part of the bound is accumulated cell by cell: |rec| (S_x w_y + w_x S_y) 4 K 2^-24.
    K = k_table()["weight", sr.GAUSSIAN]
    _, count, _, rel = sr.footprint(kind, param, spx, spy); k = np.arange(count, dtype=np.float64)
    S = [np.abs(sr.gaussian_terms(rel[:, a:a + 1] + k, param)).sum(-1) for a in (0, 1)]
    bound = (n + 2) * U * mag + 4 * K * U * (sr.accumulate(*args, np.abs(rec), wx=S[0]) + sr.accumulate(*args, np.abs(rec), wy=S[1])) + 1e-30
    err = np.abs(raw.astype(np.float64) - want)
    print(f"{rfilter}: max |film - float64| / bound = {np.max(err / bound):.3f}; W in [{raw[..., -1].min():.3f}, {raw[..., -1].max():.3f}]")
    assert lanes[:, :3].max() > 0 and np.all(err <= bound)


# ------------------------------------------------------------------------------------------------------- closed form
def test_filter_integrals():
    """sensor_ref.rfilter_integral against the midpoint sum of sensor_ref.rfilter; the Gaussian's polynomial is positive inside its radius"""
    for kind, param in sc.FILTERS.values():
        r = sr.radius(kind, param); n = 200000
        x = -1.2 * r + (np.arange(n) + 0.5) * (2.4 * r / n)
        F = np.cumsum(sr.rfilter(kind, param, x)) * (2.4 * r / n)
        G = sr.rfilter_integral(kind, param, x + 1.2 * r / n)
        I = lambda t: sr.rfilter_integral(kind, param, t)
        assert np.abs(F - G).max() <= 2e-5 * r and G[0] == 0 and np.abs(I(x) + I(-x) - I(10 * r)).max() <= 1e-12        # (the filters are even)
        if kind == sr.GAUSSIAN:
            inside = np.linspace(0.0, r, 100001)[:-1]
            assert np.polyval(sr.gaussian_coeffs(param)[::-1], inside ** 2).min() > 0


@pytest.mark.parametrize("sensor", sc.CLOSED_SENSORS)
def test_closed_form_reference_alone(mi, sensor):
    """The rectangle's image, by two routes: sensor_cases.coverage (sample_ray and a ray / rectangle test on a midpoint grid) and
    coverage_exact (the clipped polygon's image, the filter integrated in closed form).  Partly covered pixels in plenty, both clip planes
    at work, the emitting side seen, roughly a quadrant and off centre."""
    for rfilter in sc.CLOSED_FILTERS:
        tf, th, n_near, n_far = sc.coverage(mi, sensor, rfilter, clipped=True)
        exact = sc.coverage_exact(mi, sensor, rfilter)
        part = np.mean((exact > 0.05) & (exact < 0.95))
        fine = np.abs(exact - sc.coverage_exact(mi, sensor, rfilter, rows=sc.ROWS // 2)).max()
        print(f"{sensor}/{rfilter}: {part:.2f} of the pixels have 0.05 < T < 0.95; mean T {exact.mean():.3f}; samples cut by the near / far plane: "
              f"{n_near} / {n_far}; exact against the midpoint grid {np.abs(exact - th).max():.1e}; {sc.ROWS} against {sc.ROWS // 2} scanlines {fine:.1e}")
        assert part >= 0.25 and np.array_equal(tf, th) and n_far > 1000 and n_near > 1000
        assert 0.2 < exact.mean() < 0.45                                                                   # roughly a quadrant
        assert abs(exact[:, : exact.shape[1] // 2].mean() - exact[:, exact.shape[1] // 2 + 1:].mean()) > 0.2   # off centre
        # a midpoint grid of SUB^2 cells per pixel errs by about one cell row along the outline: a few times 1 / SUB^1.5
        assert np.abs(exact - th).max() <= 4.0 / sc.SUB ** 1.5
        assert fine <= 0.1 * FILM32                             # the scanline rule has converged: (1 / 4 of) what halving the step moves


@functools.lru_cache(maxsize=None)
def closed_form_reference(mi, sensor, rfilter):
    return sc.closed_form(mi, sensor, rfilter)


# What a float32 film costs a developed pixel: the colour sum and the weight sum are each held to 8e-5 of their size elsewhere
# (test_parity_gpu.film_close: sums of up to 25 spp = 2e5 terms), so their quotient to 1.6e-4.  A pixel that is all but covered or all but
# empty has a sampling error far below that (1e-6 and less), so there, and only there, this is the bound.
FILM32 = 2 * 8e-5


def check_closed_form(mi, sensor, rfilter, integrator, render, who):
    """A developed pixel is sum f L hit / sum f and its alpha sum f hit / sum f over the pixel's footprint (sensor_cases.closed_form, whose
    own error is below 0.1 FILM32, test_closed_form_reference_alone).  render(seed) -> the rgba image at sensor_cases.SPP samples.  Over
    sensor_cases.SEEDS, SE from the seeds: |mean - reference| <= 4 SE per pixel and channel wherever 4 SE exceeds FILM32 of the channel's
    radiance, and <= FILM32 of it elsewhere; |sum (mean - reference)| <= 4 sqrt(sum SE^2); the pooled SE below SE_CAP."""
    want = closed_form_reference(mi, sensor, rfilter)
    imgs = np.stack([render(s).astype(np.float64) for s in sc.SEEDS])
    assert imgs.shape[1:] == want.shape
    mean = imgs.mean(0); se = imgs.std(0, ddof=1) / np.sqrt(len(sc.SEEDS))
    level = np.array(sc.RADIANCE + (1.0,))
    dev = np.abs(mean - want); noisy = 4 * se > FILM32 * level
    z = dev / np.where(se > 0, se, 1.0)
    pooled_se = np.sqrt((se ** 2).mean(axis=(0, 1))) / level
    partial = int(np.sum((want[..., 3] > 0.05) & (want[..., 3] < 0.95)))
    root = np.sqrt((se ** 2).sum(axis=(0, 1)))
    pooled = np.abs((mean - want).sum(axis=(0, 1)))
    print(f"{who} {sensor}/{rfilter}/{integrator}: max |z| {np.max(z[noisy], initial=0):.2f} over {int(noisy.sum())} of {noisy.size} values; elsewhere the largest "
          f"deviation is {np.max((dev / level)[~noisy], initial=0):.2e} of the radiance (bound {FILM32:.1e}); pooled z {np.max(pooled / root):.2f}; "
          f"pooled SE {100 * pooled_se.max():.3f} % of the radiance (cap {100 * sc.SE_CAP:.1f} %)")
    assert np.all(pooled_se <= sc.SE_CAP) and partial >= 0.25 * want.shape[0] * want.shape[1]
    ok = np.where(noisy, dev <= 4 * se, dev <= FILM32 * level)
    assert np.all(ok), (np.argwhere(~ok)[:6], z[~ok][:6], dev[~ok][:6])
    assert np.all(pooled <= 4 * root), (pooled, 4 * root)


@pytest.mark.parametrize("integrator", sc.CLOSED_INTEGRATORS)
@pytest.mark.parametrize("rfilter", sc.CLOSED_FILTERS)
@pytest.mark.parametrize("sensor", sc.CLOSED_SENSORS)
def test_rectangle_closed_form_oracle(mi, orc, sensor, rfilter, integrator):
    O = orc.OrcScene(load(mi, sensor, rfilter, integrator, "rgba", 4))
    check_closed_form(mi, sensor, rfilter, integrator, lambda seed: O.render(spp=sc.SPP, seed=seed), "oracle")


# ----------------------------------------------------------------------------------------------------------- refusals
def test_scaled_camera_is_refused(mi):
    T = mi.ScalarTransform4f
    look = sc.SENSORS["c"]["look"]

    def load_with(tw):
        d = sc.scene_dict(mi, "c", "box"); d["sensor"]["to_world"] = tw
        return mi.load_dict(d)
    for bad in (T().look_at(*look).scale(2.0), T().look_at(*look).scale([1.0, 1.001, 1.0]), T().look_at(*look) @ T([[1, 0.01, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])):
        with pytest.raises(RuntimeError, match="Scale factors in the camera-to-world transformation are not allowed!"):
            load_with(bad)
    for good in (T().look_at(*look).scale([-1.0, 1.0, 1.0]), T().look_at(*look).scale(1.0004), T().look_at(*look).rotate([0, 0, 1], 33.0)):
        assert load_with(good).desc.sensor.fov_x == 50.0
    # lrt_scene_from_desc: the same test
    pos = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32); faces = np.array([[0, 1, 2]], np.uint32)
    assert mi.scene_from_buffers(pos, faces, sensor_to_world=T().scale([1.0, -1.0, 1.0])) is not None
    with pytest.raises(RuntimeError, match="Scale factors in the camera-to-world transformation are not allowed!"):
        mi.scene_from_buffers(pos, faces, sensor_to_world=T().scale(1.5))


def test_footprint_key_range_is_refused(mi):
    """FilmFootprint::key() packs (origin + 0x4000) into 16 bits per axis: wide-filter films beyond that are refused by name"""
    def film(width, rfilter, **kw):
        d = sc.scene_dict(mi, "a", "box"); d["sensor"]["film"].update(width=width, height=2, rfilter=dict(type=rfilter, **kw))
        return mi.load_dict(d)
    assert film(0xbfff, "tent").desc.film.width == 0xbfff and film(0xc000, "box").desc.film.width == 0xc000
    assert film(16, "gaussian", stddev=4096.0).desc.film.rfilter_param == 4096.0
    for w, f, kw in ((0xc000, "tent", {}), (16, "gaussian", dict(stddev=4097.0)), (16, "tent", dict(radius=16385.0))):
        with pytest.raises(RuntimeError, match="film footprint out of range"):
            film(w, f, **kw)
    # lrt_scene_from_desc
    good = film(16, "tent"); L = mi._lib.lib()
    d = mi._lib.SceneDesc.from_buffer_copy(good.desc); d.film.rfilter_param = 20000.0
    h = C.c_void_p()
    assert L.lrt_scene_from_desc(C.byref(d), C.byref(h)) == mi._lib.INVALID and b"film footprint out of range" in L.lrt_last_error()
    d.film.rfilter_param = 2.0
    assert L.lrt_scene_from_desc(C.byref(d), C.byref(h)) == mi._lib.OK
    L.lrt_scene_free(h)
