"""Heterogeneous media against float64 (medium_ref.py), on the CPU: the loader's volume frames, the oracle's medium probe field by field,
pure absorbers per pixel and the emitter march through a grid.  test_medium_gpu.py runs the same cases on the device.  DESIGN.md section 18."""
import functools

import numpy as np
import pytest

import medium_cases as mc
import medium_ref as mr
import prb_closed_form as cf

EPS = mr.EPS32
NEAR = 64 * EPS                       # a lane whose decision the float64 reference itself makes within this relative gap is not compared
FIELDS = ("t", "mint", "p", "local", "grid", "sigma_t", "sigma_s", "sigma_n", "combined")
# 8 fixed seeds.  (0 - 7 put one pixel of volume a at z = -5.48 through an SE estimate of 0.45 x its Bernoulli value, a false alarm of the
# 7-degrees-of-freedom test that 96 other seeds do not repeat; the next eight were taken once.  DESIGN.md section 18.5.)
SEEDS = tuple(range(8, 16))
W, H = 4, 3


# ------------------------------------------------------------------------------------------------- reference runs, conditioning, K
def ref_run(name, inputs, dt=np.float64, frame=None):
    o, d, mt, u, ch, _ = inputs
    if name == "f":
        h = mc.HOM
        return mr.sample_homogeneous(np.float32(h["sigma_t"]), np.float32(h["scale"]), np.float32(h["albedo"]), o, d, mt, u, ch, dt)
    v = mc.VOLUMES[name]
    fr = mc.frame32(name) if frame is None else frame
    return mr.sample_heterogeneous(fr, v["grid"], np.float32(mc.PROBE_SCALE), np.float32(mc.ALBEDO), o, d, mt, u, dt)


def conditioning(name, inputs, ref, frame=None):
    """What each field's rounding error scales with (the issue's choices; `local` and the coefficients follow from them):
    t relative to t; mint to mint; p to |o| + t; local to |A| |p| + |b|; grid to max |corner| + res * (max - min corner) * (local's scale);
    sigma_t / sigma_s to scale * that; sigma_n to the majorant plus sigma_t's; combined to the majorant."""
    o = np.asarray(inputs[0], np.float64)
    n = len(o)
    with np.errstate(invalid="ignore"):
        c = {"t": np.abs(ref["sampled_t"]), "mint": np.abs(ref["mint"]), "p": np.abs(o).max(-1) + np.abs(ref["sampled_t"]), "combined": ref["combined"][:, 0]}
        if name == "f":
            z = np.zeros(n)
            c.update(local=z, grid=z, sigma_t=ref["combined"].max(-1), sigma_s=ref["combined"].max(-1), sigma_n=z)
            return c
        v = mc.VOLUMES[name]
        A = np.asarray((mc.frame32(name) if frame is None else frame)[0], np.float64)
        cl = (np.abs(ref["p"]) @ np.abs(A[:, :3]).T + np.abs(A[:, 3])).max(-1)
        fin = np.isfinite(ref["local"]).all(-1)
        maxc, rng = mr.corner_range(v["grid"], np.where(fin[:, None], ref["local"], 0.0))
        cg = maxc + max(v["grid"].shape) * rng * np.maximum(cl, 1.0)
        s = float(mc.PROBE_SCALE)
        c.update(local=cl, grid=cg, sigma_t=s * cg, sigma_s=s * cg, sigma_n=ref["combined"][:, 0] + s * cg)
    return c


def comparable(ref, kind):
    """(lanes compared against float64, lanes the reference flags as within rounding of a decision)"""
    special = np.array([k in ("face", "nan") for k in kind])
    near = ~special & ((ref["margin"] < NEAR) | (ref["t_margin"] < NEAR))
    return ~special & ~near, near


def field_error(got, ref, cond, field, lanes):
    """max over `lanes` of |got - ref| / cond in units of 2^-24; t is compared on valid lanes (it is inf elsewhere)"""
    a, b = np.asarray(got[field], np.float64), np.asarray(ref[field], np.float64)
    sel = lanes & ref["valid"] if field == "t" else lanes
    if a.ndim == 2:
        sel = sel[:, None] & np.ones(a.shape, bool); c = np.repeat(cond[field][:, None], a.shape[1], 1)
    else:
        c = cond[field]
    with np.errstate(invalid="ignore"):
        err = np.abs(a - b)[sel]
    c = c[sel]
    assert np.isfinite(err).all(), field
    exact = err == 0
    assert (c[~exact] > 0).all(), field                          # a field with nothing to scale with must match exactly
    return float((err[~exact] / c[~exact]).max() / EPS) if (~exact).any() else 0.0


def all_inputs():
    return {name: (mc.hom_rays() if name == "f" else mc.probe_rays(name)) for name in list(mc.VOLUMES) + ["f"]}


@functools.lru_cache(maxsize=None)
def k_table():
    """K per field: the largest conditioned error of medium_ref's formulas evaluated in float32 against their float64 evaluation over every
    case, in units of 2^-24 (never below 1/2: storing a result as float32 costs that much).  The bound on a probe is 4 K."""
    K = {f: 0.5 for f in FIELDS}
    for name, inp in all_inputs().items():
        r64, r32 = ref_run(name, inp), ref_run(name, inp, np.float32)
        lanes, _ = comparable(r64, inp[5])
        lanes &= (r32["valid"] == r64["valid"])
        cond = conditioning(name, inp, r64)
        for f in FIELDS:
            K[f] = max(K[f], field_error(r32, r64, cond, f, lanes))
    return K


def check_probe(name, got, inputs, frame, label):
    """A probe's record against float64, field by field; returns a report line"""
    ref = ref_run(name, inputs, frame=frame)
    lanes, near = comparable(ref, inputs[5])
    share = near.sum() / len(near)
    assert share <= 0.02, (name, share)
    assert (got["valid"][lanes] == ref["valid"][lanes]).all(), (label, name, np.flatnonzero(lanes & (got["valid"] != ref["valid"])))
    miss = lanes & ~ref["hit"]
    assert not got["valid"][miss].any() and (got["mint"][miss] == 0).all()
    assert np.isinf(got["t"][lanes & ~ref["valid"]]).all()
    cond = conditioning(name, inputs, ref, frame)
    K = k_table()
    errs = {f: field_error(got, ref, cond, f, lanes) for f in FIELDS}
    line = f"{label} {name}: {int(lanes.sum())} lanes, {int(ref['valid'][lanes].sum())} valid, {int(miss.sum())} miss, excluded {share:.2%}; " + \
        ", ".join(f"{f} {errs[f]:.2f}/{4 * K[f]:.2f}" for f in FIELDS)
    print(line)
    for f in FIELDS:
        assert errs[f] <= 4 * K[f], line
    return line


def desc_frame(sc, m=0):
    M = sc.desc.media[m]
    return (np.array(M.grid_to_local[:], np.float64).reshape(3, 4), np.array(M.grid_bbox_min[:], np.float64), np.array(M.grid_bbox_max[:], np.float64))


def probe_inputs(inputs):
    return inputs[:5]


def check_lookups(name, probe, label):
    """The lookup-only mode at medium_cases.local_points: exact at exact texel centres, within 4 K elsewhere"""
    grid = mc.VOLUMES[name]["grid"]
    pts, exact = mc.local_points(grid.shape)
    n = len(pts)
    got = probe(pts, np.zeros((n, 3), np.float32), np.full(n, np.nan, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32))
    assert (got["raw"][:, :18] == 0).all() and (got["local"] == pts).all()
    ref = mr.trilinear(grid, pts.astype(np.float64))
    rz, ry, rx = grid.shape
    assert exact.sum() >= 2
    assert (got["grid"][exact] == grid.reshape(-1)[: rz * ry * rx][exact[: rz * ry * rx]]).all(), f"{label} {name}: a texel centre does not return its texel"
    maxc, rng = mr.corner_range(grid, pts)
    cond = maxc + max(grid.shape) * rng * np.maximum(np.abs(pts).max(-1), 1.0)
    err = (np.abs(got["grid"] - ref) / cond).max() / EPS
    print(f"{label} {name}: {n} lookups ({int(exact.sum())} exact centres, {int(((pts < 0) | (pts > 1)).any(-1).sum())} outside the cube): {err:.2f}/{4 * k_table()['grid']:.2f}")
    assert err <= 4 * k_table()["grid"]
    return got


@pytest.fixture(scope="module")
def probe_scenes(mi, tmp_path_factory):
    d = tmp_path_factory.mktemp("medium_probe")
    return {name: mi.load_string(mc.probe_scene_xml(mi, d, name)) for name in list(mc.VOLUMES) + ["f"]}


# ---------------------------------------------------------------------------------------------------------------------- API
def test_api_version_and_symbol(mi):
    assert mi._lib.lib().lrt_version() >= 118 and "lrt_medium_probe" in mi._lib.EXPORTED_SYMBOLS
    assert mi._lib.MEDIUM_PROBE_FLOATS == 22


# ------------------------------------------------------------------------------------------------------------------- loader
@pytest.mark.parametrize("name", sorted(mc.VOLUMES))
def test_loader_volume_frame(probe_scenes, name):
    """grid_to_local, grid_bbox_min / max, grid_res and grid_max of the description against the float64 frame.  The matrix is rounded once
    from a double computation (2 ulp of its row's largest entry); the box comes from single-precision corner transforms (8 ulp of the box)."""
    sc = probe_scenes[name]; M = sc.desc.media[0]; grid = mc.VOLUMES[name]["grid"]
    tl, lo, hi = mc.frame(name)
    got_tl, got_lo, got_hi = desc_frame(sc)
    assert tuple(M.grid_res[:]) == grid.shape[::-1]
    assert M.grid_max == grid.max() and abs(M.scale - mc.PROBE_SCALE) < 1e-7
    assert (np.abs(got_tl - tl) <= 2 * EPS * np.abs(tl).max(1, keepdims=True)).all(), (got_tl, tl)
    size = max(np.abs(lo).max(), np.abs(hi).max())
    assert np.abs(got_lo - lo).max() <= 8 * EPS * size and np.abs(got_hi - hi).max() <= 8 * EPS * size, (got_lo, lo, got_hi, hi)


def test_use_grid_bbox_changes_the_frame(mi, tmp_path):
    """Volume (d) with and without use_grid_bbox: the header's box decides where the volume lies"""
    with_box = mi.load_string(mc.probe_scene_xml(mi, tmp_path, "d"))
    xml = mc.scene_xml(mc.medium_xml(mi, tmp_path, "d", mc.PROBE_SCALE, use_grid_bbox=False), mc.shape_matrix("d"), mc.camera("d"))
    without = mi.load_string(xml)
    _, lo, hi = mr.volume_frame(mr.compose(mc.VOLUMES["d"]["steps"]))
    assert np.abs(desc_frame(without)[1] - lo).max() <= 1e-6 and np.abs(desc_frame(without)[2] - hi).max() <= 1e-6
    assert np.abs(desc_frame(with_box)[1] - mc.frame("d")[1]).max() <= 1e-6 and np.abs(desc_frame(with_box)[1] - lo).max() > 0.1


@pytest.mark.parametrize("steps", [[("scale", (2.0, 0.0, 2.0))], [("scale", (1.0, 2.0, 3.0)), ("rotate", (0.0, 0.0, 1.0), 30.0), ("scale", (1.0, 1.0, 0.0))]])
def test_singular_volume_transform_is_refused(mi, tmp_path, steps):
    xml = mc.scene_xml(mc.medium_xml(mi, tmp_path, "a", 1.0, steps=steps), np.eye(4), mc.camera("a"))
    with pytest.raises(RuntimeError, match="singular|not invertible"):
        mi.load_string(xml)


@pytest.mark.parametrize("box", [((0.0, 0.0, 0.0), (1.0, 0.0, 1.0)), ((0.0, 0.0, 2.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (float("nan"), 1.0, 1.0))])
def test_empty_header_box_is_refused(mi, tmp_path, box):
    """use_grid_bbox with max <= min on an axis (or a NaN) has no bbox_transform; the same file loads without use_grid_bbox"""
    vol = str(tmp_path / "empty.vol")
    mi.write_volume_grid(vol, mc.GRID_B, bbox_min=box[0], bbox_max=box[1])

    def xml(ugb):
        med = f"""<medium type="heterogeneous" id="smoke"><volume name="sigma_t" type="gridvolume"><string name="filename" value="{vol}"/>
          <boolean name="use_grid_bbox" value="{ugb}"/></volume></medium>"""
        return mc.scene_xml(med, np.eye(4), mc.camera("a"))
    with pytest.raises(RuntimeError, match="use_grid_bbox"):
        mi.load_string(xml("true"))
    assert mi.load_string(xml("false")).desc.media[0].grid_max == mc.GRID_B.max()


def test_scene_from_desc_refuses_a_broken_grid_frame(mi, probe_scenes):
    """lrt_scene_from_desc takes the frame ready-made: a non-finite matrix or an empty box is refused there too"""
    import ctypes as C
    L = mi._lib.lib()
    sc = probe_scenes["b"]
    M = sc.desc.media[0]
    keep_tl, keep_max = M.grid_to_local[0], M.grid_bbox_max[1]
    try:
        for breakage in ("matrix", "box"):
            if breakage == "matrix": M.grid_to_local[0] = float("inf")
            else: M.grid_bbox_max[1] = M.grid_bbox_min[1]
            h = C.c_void_p()
            assert L.lrt_scene_from_desc(C.byref(sc.desc), C.byref(h)) == mi._lib.INVALID, breakage
            M.grid_to_local[0], M.grid_bbox_max[1] = keep_tl, keep_max
        h = C.c_void_p()
        assert L.lrt_scene_from_desc(C.byref(sc.desc), C.byref(h)) == mi._lib.OK
        L.lrt_scene_free(h)
    finally:
        M.grid_to_local[0], M.grid_bbox_max[1] = keep_tl, keep_max


# ---------------------------------------------------------------------------------------------------------- reference checks
def test_reference_is_self_consistent():
    """medium_ref against itself: the float32 lookup is the float64 one in single, the frame maps the AABB's defining corners into the unit
    cube, the optical depth of a constant grid is the chord, and density is 0 outside the AABB"""
    r = np.random.default_rng(0)
    p = r.uniform(-1, 2, (200, 3))
    for g in (mc.GRID_A, mc.GRID_B):
        assert np.abs(mr.trilinear(g, p, np.float32) - mr.trilinear(g, p)).max() < 2e-5
    for name in mc.VOLUMES:
        tl, lo, hi = mc.frame(name)
        corners = mc.unit_cube_to_world(name) @ np.array([[x, y, z, 1.0] for x in (0, 1) for y in (0, 1) for z in (0, 1)]).T
        assert np.allclose(corners[:3].min(1), lo) and np.allclose(corners[:3].max(1), hi)
        const = np.full((2, 2, 2), 0.75, np.float32)
        o = np.array([[lo[0] - 1.0, (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2]]); d = np.array([[1.0, 0.0, 0.0]])
        assert abs(mr.optical_depth((tl, lo, hi), const, o, d, 0.0, np.inf)[0] - 0.75 * (hi[0] - lo[0])) < 1e-12
        assert mr.density((tl, lo, hi), const, hi + 1e-9) == 0 and mr.density((tl, lo, hi), const, (lo + hi) / 2) == 0.75
    assert np.abs(mc.frame("d")[1] - np.array([-0.8, -0.5, -0.7])).max() < 1e-12          # to_world * header box, by hand


def test_k_table_is_measured_from_the_reference_alone():
    K = k_table()
    print("K (units of 2^-24):", ", ".join(f"{f} {K[f]:.2f}" for f in FIELDS))
    assert all(0.5 <= K[f] < 64 for f in FIELDS), K


def test_inputs_cover_the_cases_and_stay_clear_of_decisions():
    for name, inp in all_inputs().items():
        ref = ref_run(name, inp)
        lanes, near = comparable(ref, inp[5])
        print(f"{name}: {len(near)} lanes, {int(near.sum())} within rounding of a decision ({near.mean():.2%}), {int(ref['valid'][lanes].sum())} valid, {int((~ref['hit'])[lanes].sum())} miss")
        assert near.mean() <= 0.02
        assert ref["valid"][lanes].sum() >= 20 and (~ref["valid"])[lanes].sum() >= 10
        if name != "f":
            kinds = set(inp[5])
            assert {"outside", "inside", "miss", "behind", "axis-in-slab", "axis-out-of-slab", "face", "on-box", "nan", "outside-maxt-before"} <= kinds
            assert (~ref["hit"])[lanes].sum() >= 20
            k = np.array(inp[5])
            assert ref["hit"][k == "axis-in-slab"].all() and not ref["hit"][k == "miss"].any() and not ref["valid"][k == "behind"].any()
            # bbox.h:320-337 as written: a ray along z that passes beside the box in x or y is a hit, since both of that axis' slab distances
            # are infinities of one sign, no comparison between infinities is true, and the NaN-safe minimum / maximum skip them.  The
            # probes must reproduce that; every other ray beside the box misses.
            along_z = (np.asarray(inp[1])[:, 0] == 0) & (np.asarray(inp[1])[:, 1] == 0)
            out = k == "axis-out-of-slab"
            assert not ref["hit"][out & ~along_z].any() and ref["hit"][out & along_z].all() and (out & along_z).sum() >= 2
            assert mr.on_face_with_zero_direction(inp[0], inp[1], *mc.frame32(name)[1:])[k == "face"].all()
            # points inside the AABB but outside the (rotated) unit cube are looked up too
            if name == "c":
                loc = ref["local"][lanes & ref["valid"]]
                assert ((loc < 0) | (loc > 1)).any(-1).sum() >= 5


# ------------------------------------------------------------------------------------------------------------ oracle probe
@pytest.mark.parametrize("name", sorted(mc.VOLUMES) + ["f"])
def test_oracle_probe_matches_float64(orc, probe_scenes, name):
    sc = probe_scenes[name]; o = orc.OrcScene(sc)
    inp = all_inputs()[name]
    got = o.medium_probe(0, *probe_inputs(inp))
    check_probe(name, got, inp, None if name == "f" else desc_frame(sc), "oracle")
    if name != "f":
        check_lookups(name, lambda *a: o.medium_probe(0, *a), "oracle")
    with pytest.raises(RuntimeError):
        o.medium_probe(1, *probe_inputs(inp))


# -------------------------------------------------------------------------------------------------------- absorbers per pixel
SUB = 12
ABSORBER_VARIANTS = [("volpath", True), ("volpath", False), ("volpathmis", True), ("volpathmis", False)]


def shape_span(name, o, d):
    """Entry and exit of rays through the medium's shape: the slab test in the cube's own frame (distances are affine invariants)"""
    inv = np.linalg.inv(mc.shape_matrix(name))
    ol = inv[:3, :3] @ np.asarray(o, np.float64) + inv[:3, 3]
    dl = np.asarray(d, np.float64) @ inv[:3, :3].T
    return cf.box_span(ol, dl, (-1, -1, -1), (1, 1, 1))


# The measured SE is itself an estimate: 8 seeds x 12 pixels give the pooled variance 84 degrees of freedom, a relative standard deviation of
# sqrt(2 / 84) = 15 % (8 % of the SE); a pixel's has 7 (27 % of its SE, and the largest of 12 is compared).  At the Bernoulli minimum the
# measured pooled SE would miss its cap every other time.  Twice the samples put the expected pooled SE at 0.3 % / sqrt(2) = 0.21 % and the
# expected per-pixel SE near 0.75 %: the caps lie 5 and 6 of those deviations above.  (The estimator is Bernoulli: over 96 seeds its per-pixel
# variance is 1.02 and 1.04 times T (1 - T) / spp at spp 256 and 2048.)
SE_MARGIN = 2.0


def spp_for(T, n_seeds=len(SEEDS)):
    """The smallest multiple of 64 samples per pixel and seed at which the Bernoulli standard error sqrt(T (1 - T) / N) keeps the pooled
    relative SE <= 0.3 % and every pixel's <= 2 %, times SE_MARGIN so that the SE measured from the seeds meets the same caps"""
    T = np.asarray(T, np.float64).reshape(-1)
    var = T * (1 - T)
    n_pixel = (var / (0.02 * T) ** 2).max()
    n_pool = var.sum() / (0.003 * T.sum()) ** 2
    return int(np.ceil(SE_MARGIN * max(n_pixel, n_pool) / n_seeds / 64.0)) * 64


@functools.lru_cache(maxsize=None)
def absorber_reference(name):
    """(medium scale, per-pixel reference (H, W), spp): scale puts the largest pixel optical depth at 1.8"""
    cam = mc.camera(name)
    o, d = cf.camera_directions(cam["origin"], cam["target"], cam["up"], cam["fov"], W, H, SUB)
    flat = d.reshape(-1, 3)
    t0, t1 = shape_span(name, o, flat)
    assert (t1 > t0).all()                                                   # every ray crosses the shape
    od = mr.optical_depth(mc.frame(name), mc.VOLUMES[name]["grid"], o, flat, t0, t1).reshape(H, W, -1)
    s = float(np.float32(1.8 / od.mean(-1).max()))
    tau = s * od.mean(-1)
    assert tau.min() >= 0.5 and tau.max() <= 2.0, tau
    T = np.exp(-s * od).mean(-1)
    return s, T, spp_for(T)


def seed_stats(render, spp):
    """render(spp=, seed=) -> (H, W, 3) over the fixed seeds: per-pixel mean and standard error of the channel mean"""
    runs = np.array([np.asarray(render(spp=spp, seed=s), np.float64)[..., :3].mean(-1) for s in SEEDS])
    assert np.isfinite(runs).all()
    return runs.mean(0), runs.std(0, ddof=1) / np.sqrt(len(SEEDS))


def assert_pixels(mean, se, ref, label):
    z = (mean - ref) / se
    pooled = (mean - ref).sum() / np.sqrt((se ** 2).sum())
    line = (f"{label}: max |z| {np.abs(z).max():.2f}, pooled z {pooled:.2f}, per-pixel SE <= {(se / ref).max():.3%}, "
            f"pooled SE {np.sqrt((se ** 2).sum()) / ref.sum():.3%}, ref {ref.min():.4f} .. {ref.max():.4f}")
    print(line)
    assert (se / ref).max() <= 0.02 and np.sqrt((se ** 2).sum()) / ref.sum() <= 0.003, line
    assert (np.abs(mean - ref) <= 4 * se).all(), line
    assert abs((mean - ref).sum()) <= 4 * np.sqrt((se ** 2).sum()), line
    return line


def absorber_xml(mi, tmp_dir, name, integrator, flag):
    s, _, spp = absorber_reference(name)
    extra = f'<boolean name="use_spectral_mis" value="{"true" if flag else "false"}"/>' if integrator == "volpathmis" else ""
    med = mc.medium_xml(mi, tmp_dir, name, s, albedo=(0.0, 0.0, 0.0), spectral=flag if integrator == "volpath" else True)
    return mc.scene_xml(med, mc.shape_matrix(name), mc.camera(name), integrator=integrator, integrator_extra=extra, spp=spp)


@pytest.mark.parametrize("integrator,flag", ABSORBER_VARIANTS)
@pytest.mark.parametrize("name", sorted(mc.VOLUMES))
def test_absorber_pixels_oracle(mi, orc, tmp_path, name, integrator, flag):
    """albedo 0 under a constant environment of radiance 1: pixel = footprint mean of exp(-scale * optical depth)"""
    s, T, spp = absorber_reference(name)
    o = orc.OrcScene(mi.load_string(absorber_xml(mi, tmp_path, name, integrator, flag)))
    mean, se = seed_stats(o.render, spp)
    assert_pixels(mean, se, T, f"oracle absorber {name} {integrator} {flag} scale {s:.4f} spp {spp}")


def test_absorber_spans_match_trace(mi, orc, tmp_path):
    """The float64 camera and shape span against the oracle's ray casts at pixel centres (as test_reference_chords_match_trace)"""
    for name in sorted(mc.VOLUMES):
        o = orc.OrcScene(mi.load_string(absorber_xml(mi, tmp_path, name, "volpath", True)))
        cam = mc.camera(name)
        org, d = cf.camera_directions(cam["origin"], cam["target"], cam["up"], cam["fov"], W, H, 1)
        d = d[:, :, 0].reshape(-1, 3)
        t0, t1 = shape_span(name, org, d)
        g0, _, _, prim = o.trace(np.broadcast_to(org, d.shape), d)
        assert (prim != 0xffffffff).all() and np.abs(g0 - t0).max() <= 1e-4
        g1, _, _, prim1 = o.trace(org + d * (g0[:, None] + 1e-3), d)
        assert (prim1 != 0xffffffff).all() and np.abs(g1 + g0 + 1e-3 - t1).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- emitter march
MARCH_VOLUMES = ("b", "c", "e")
MARCH_VARIANTS = [("volpath", True), ("volpath", False), ("volpathmis", True), ("volpathmis", False)]
RHO, INTENSITY, FLOOR_DROP, LIGHT_RISE = 0.7, 40.0, 2.6, 3.0


def march_geometry(name):
    _, lo, hi = mc.frame(name)
    c = (lo + hi) / 2
    floor_y = c[1] - FLOOR_DROP
    light = c + np.array([0.0, LIGHT_RISE, 0.0])
    cam = dict(origin=(c[0] + 5.0, floor_y + 0.9, c[2] + 0.4), target=(c[0], floor_y, c[2]), up=(0.0, 1.0, 0.0), fov=3.0)
    return floor_y, light, cam


@functools.lru_cache(maxsize=None)
def march_reference(name):
    """(medium scale, per-pixel reference, spp): a diffuse floor under a point light on the far side of the volume; the camera's rays do not
    cross the medium's shape.  pixel = footprint mean of (rho / pi) I cos(theta) / r^2 exp(-scale * optical depth(x -> light))."""
    floor_y, light, cam = march_geometry(name)
    o, d = cf.camera_directions(cam["origin"], cam["target"], cam["up"], cam["fov"], W, H, SUB)
    flat = d.reshape(-1, 3)
    t0, t1 = shape_span(name, o, flat)
    assert ((t0 > t1) | (t1 < 0)).all()                                     # no camera ray meets the shape
    tf = (floor_y - o[1]) / flat[:, 1]
    assert (tf > 0).all()
    x = o + flat * tf[:, None]
    to_light = light - x
    r = np.linalg.norm(to_light, axis=1)
    wl = to_light / r[:, None]
    s0, s1 = shape_span_many(name, x, wl)
    assert (s1 > s0).all() and (s1 < r).all()                                # every shadow ray crosses the whole shape below the light
    od = mr.optical_depth(mc.frame(name), mc.VOLUMES[name]["grid"], x, wl, s0, s1)
    s = float(np.float32(1.2 / od.mean()))
    T = np.exp(-s * od)
    assert 0.5 <= (s * od).min() and (s * od).max() <= 2.0
    geom = RHO / np.pi * INTENSITY * wl[:, 1] / r ** 2
    ref = (geom * T).reshape(H, W, -1).mean(-1)
    return s, ref, spp_for(T.reshape(H, W, -1).mean(-1))


def shape_span_many(name, o, d):
    inv = np.linalg.inv(mc.shape_matrix(name))
    ol = np.asarray(o, np.float64) @ inv[:3, :3].T + inv[:3, 3]
    dl = np.asarray(d, np.float64) @ inv[:3, :3].T
    return cf.box_span(ol, dl, (-1, -1, -1), (1, 1, 1))


def march_xml(mi, tmp_dir, name, integrator, flag):
    s, _, spp = march_reference(name)
    floor_y, light, cam = march_geometry(name)
    extra = f'<boolean name="use_spectral_mis" value="{"true" if flag else "false"}"/>' if integrator == "volpathmis" else ""
    rest = (f'<shape type="rectangle"><transform name="to_world"><scale value="20"/><rotate x="1" angle="-90"/><translate x="{mc._f(light[0])}" y="{mc._f(floor_y)}" z="{mc._f(light[2])}"/></transform>'
            f'<bsdf type="diffuse"><rgb name="reflectance" value="{RHO}, {RHO}, {RHO}"/></bsdf></shape>'
            f'<emitter type="point"><point name="position" x="{mc._f(light[0])}" y="{mc._f(light[1])}" z="{mc._f(light[2])}"/><rgb name="intensity" value="{INTENSITY}, {INTENSITY}, {INTENSITY}"/></emitter>')
    med = mc.medium_xml(mi, tmp_dir, name, s, albedo=(0.0, 0.0, 0.0), spectral=flag if integrator == "volpath" else True)
    return mc.scene_xml(med, mc.shape_matrix(name), cam, integrator=integrator, integrator_extra=extra, max_depth=2, spp=spp, rest=rest)


@pytest.mark.parametrize("integrator,flag", MARCH_VARIANTS)
@pytest.mark.parametrize("name", MARCH_VOLUMES)
def test_emitter_march_oracle(mi, orc, tmp_path, name, integrator, flag):
    s, ref, spp = march_reference(name)
    o = orc.OrcScene(mi.load_string(march_xml(mi, tmp_path, name, integrator, flag)))
    mean, se = seed_stats(o.render, spp)
    assert_pixels(mean, se, ref, f"oracle march {name} {integrator} {flag} scale {s:.4f} spp {spp}")
