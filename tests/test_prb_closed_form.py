"""PRB adjoint (lrt_render_backward, kernels_prb.h) against float64 closed forms (prb_closed_form.py): the oracle here, the device in
test_prb_closed_form_gpu.py, on the same cases.

Every estimate is split over K = 8 seeds; the test asserts |mean - closed form| <= 4 SE + a small floor AND that the SE itself is a
small fraction of the gradient (so that a case cannot pass on its noise).  The expected gradient of the loss sum(grad * image) is
sum over pixels and channels of grad * dL/dtheta, with grad a random positive image."""
import os

import numpy as np
import pytest

import prb_closed_form as cf

K = 8
LE = np.array([1.0, 0.8, 0.6])                       # the constant emitter of every case


# ------------------------------------------------------------------------------------------------------------------- scenes
ABS_CAM = dict(origin=(4.0, 2.5, -3.5), target=(0.3, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=38.0)
ABS_SIGMA = np.array([0.5, 0.9, 1.4])
ABS_W, ABS_H = 24, 10


def absorber_xml(pixel_format="rgb", crop=None):
    """A pure absorber (albedo 0, HG g = 0.5, spectrally varying sigma_t) in the null-BSDF cube [-1, 1]^3 seen obliquely on a 24 x 10
    film: chords from 0 (pixels that miss the cube) to about 3."""
    c = ABS_CAM
    cr = "" if crop is None else "".join(f'<integer name="{k}" value="{v}"/>' for k, v in zip(("crop_offset_x", "crop_offset_y", "crop_width", "crop_height"), crop))
    return f"""<scene version="3.0.0">
  <integrator type="prbvolpath"><integer name="max_depth" value="4"/></integrator>
  <sensor type="perspective"><float name="fov" value="{c['fov']}"/>
    <transform name="to_world"><lookat origin="{', '.join(map(str, c['origin']))}" target="{', '.join(map(str, c['target']))}" up="0, 1, 0"/></transform>
    <sampler type="independent"><integer name="sample_count" value="4"/></sampler>
    <film type="hdrfilm"><integer name="width" value="{ABS_W}"/><integer name="height" value="{ABS_H}"/><string name="pixel_format" value="{pixel_format}"/>{cr}<rfilter type="box"/></film>
  </sensor>
  <medium type="homogeneous" id="fog"><rgb name="sigma_t" value="{', '.join(map(str, ABS_SIGMA))}"/><rgb name="albedo" value="0, 0, 0"/>
    <phase type="hg"><float name="g" value="0.5"/></phase></medium>
  <shape type="cube"><bsdf type="null"/><ref name="interior" id="fog"/></shape>
  <emitter type="constant"><rgb name="radiance" value="{', '.join(map(str, LE))}"/></emitter>
</scene>"""


def absorber_chords(sub=48):
    c = ABS_CAM
    return cf.pixel_chords(c["origin"], c["target"], c["up"], c["fov"], ABS_W, ABS_H, (-1, -1, -1), (1, 1, 1), sub=sub)


AXIAL_CAM = dict(origin=(0.0, 0.0, -20.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
AXIAL_SIGMA = np.array([0.3, 0.8, 1.4])


def axial_absorber_xml(rfilter):
    """The narrow-fov axial slab of test_beer_lambert_transmittance (every pixel Le exp(-2 sigma)) on a 10 x 6 film."""
    return f"""<scene version="3.0.0">
  <integrator type="prbvolpath"><integer name="max_depth" value="4"/></integrator>
  <sensor type="perspective"><float name="fov" value="2"/>
    <transform name="to_world"><lookat origin="0, 0, -20" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="independent"><integer name="sample_count" value="4"/></sampler>
    <film type="hdrfilm"><integer name="width" value="10"/><integer name="height" value="6"/><rfilter type="{rfilter}"/></film>
  </sensor>
  <medium type="homogeneous" id="fog"><rgb name="sigma_t" value="{', '.join(map(str, AXIAL_SIGMA))}"/><rgb name="albedo" value="0, 0, 0"/></medium>
  <shape type="cube"><bsdf type="null"/><ref name="interior" id="fog"/></shape>
  <emitter type="constant"><rgb name="radiance" value="{', '.join(map(str, LE))}"/></emitter>
</scene>"""


# the wide slab: the cube scaled to [-40, 40] x [-40, 40] x [-1, 1] (>= 20 mean free paths sideways for sigma >= 0.5), a 0.5 degree
# camera on its axis: every camera ray runs along the normal through thickness 2 (chord error < 1e-4 relative)
SLAB_D = 2.0
SLAB_HALF = 40.0
SLAB_SIGMA = np.array([0.6, 0.9, 1.2])
SLAB_ALBEDO = np.array([0.5, 0.7, 0.8])


def _slab_common(medium, shape_medium_ref, sample_count=4):
    return f"""<scene version="3.0.0">
  <integrator type="prbvolpath"><integer name="max_depth" value="2"/></integrator>
  <sensor type="perspective"><float name="fov" value="0.5"/>
    <transform name="to_world"><lookat origin="0, 0, -20" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="independent"><integer name="sample_count" value="{sample_count}"/></sampler>
    <film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/><rfilter type="box"/></film>
  </sensor>
  {medium}
  <shape type="cube"><transform name="to_world"><scale x="{SLAB_HALF}" y="{SLAB_HALF}" z="1"/></transform><bsdf type="null"/><ref name="interior" id="{shape_medium_ref}"/></shape>
  <emitter type="constant"><rgb name="radiance" value="{', '.join(map(str, LE))}"/></emitter>
</scene>"""


def _v(a):
    return ", ".join(repr(float(x)) for x in a)


def slab_xml(sigma=SLAB_SIGMA, albedo=SLAB_ALBEDO, g=0.4, sample_emitters=True):
    med = (f'<medium type="homogeneous" id="fog"><rgb name="sigma_t" value="{_v(sigma)}"/><rgb name="albedo" value="{_v(albedo)}"/>'
           f'<boolean name="sample_emitters" value="{"true" if sample_emitters else "false"}"/><phase type="hg"><float name="g" value="{g}"/></phase></medium>')
    return _slab_common(med, "fog")


HET_SIGMA = 0.9                                      # grey: a grid medium's sigma_t comes from one grid channel


def het_slab_xml(mi, tmp_path, density, majorant, albedo=SLAB_ALBEDO, g=0.4):
    """The wide slab filled with a constant grid `density` (scale = HET_SIGMA / density); when majorant > density one corner texel holds
    `majorant`, far (> 25 mean free paths) from the camera rays and from where single scattering reaches: the medium is the
    homogeneous slab, with null collisions on both the path and the NEE march."""
    grid = np.full((6, 6, 6), density, np.float32)
    if majorant != density:
        grid[0, 0, 0] = majorant
    vol = os.path.join(str(tmp_path), f"slab_{density}_{majorant}.vol")
    mi.write_volume_grid(vol, grid)
    med = f"""<medium type="heterogeneous" id="smoke">
    <volume name="sigma_t" type="gridvolume"><string name="filename" value="{vol}"/>
      <transform name="to_world"><scale x="{2 * SLAB_HALF}" y="{2 * SLAB_HALF}" z="2"/><translate x="{-SLAB_HALF}" y="{-SLAB_HALF}" z="-1"/></transform></volume>
    <rgb name="albedo" value="{_v(albedo)}"/><float name="scale" value="{HET_SIGMA / density!r}"/>
    <phase type="hg"><float name="g" value="{g}"/></phase></medium>"""
    return _slab_common(med, "smoke")


# ------------------------------------------------------------------------------------------------------------ estimation
def grad_image(shape, seed=0):
    """A random positive grad image (sums to ~1 per channel)"""
    H, W, T = shape
    return ((0.5 + np.random.default_rng(seed).random((H, W, T))) / (H * W)).astype(np.float32)


def seed_split(backward, grad, spp, k=K):
    """backward(grad, spp=, seed=) over k seeds: dict key -> (mean, SE, all runs) in float64."""
    runs = [backward(grad, spp=spp, seed=s) for s in range(k)]
    out = {}
    for key in ("sigma_t", "albedo", "g"):
        r = np.array([np.atleast_1d(x[key]) for x in runs], np.float64)
        out[key] = (r.mean(0), r.std(0, ddof=1) / np.sqrt(k), r)
    return out


def expected_grads(grad, d_sigma, d_albedo, d_g):
    """sum_p grad_pk * dL_pk / dtheta for per-pixel (H, W, 3) or per-channel (3,) derivatives"""
    g = grad[..., :3].astype(np.float64)
    full = lambda a: np.broadcast_to(a, g.shape)
    return {"sigma_t": (g * full(d_sigma)).sum((0, 1)), "albedo": (g * full(d_albedo)).sum((0, 1)), "g": np.atleast_1d((g * full(d_g)).sum())}


def check(est, expect, se_frac, zero=None, floor=1e-6):
    """est: seed_split output; expect: key -> closed form, NaN entries not compared; zero: key -> boolean mask (or True) of entries whose
    every run must be exactly 0.  Every run of every entry must be finite.  Returns one report line per key."""
    lines = []
    for key in ("sigma_t", "albedo", "g"):
        m, se, runs = est[key]
        assert np.isfinite(runs).all(), (key, runs)
        z = np.broadcast_to(np.asarray((zero or {}).get(key, False)), m.shape)
        assert (runs[:, z] == 0).all(), (key, "not exactly 0", runs)
        e = np.broadcast_to(np.asarray(expect[key], np.float64), m.shape)
        mask = np.isfinite(e) & ~z
        err = np.abs(m - e)
        with np.errstate(divide="ignore", invalid="ignore"):
            lines.append(f"{key}: mean {m} closed form {e} SE/|cf| {se / np.abs(e)} |err|/SE {err / se}")
        assert (err[mask] <= 4 * se[mask] + floor).all(), lines[-1]
        assert (se[mask] <= se_frac * np.abs(e[mask])).all(), ("noise too large", lines[-1])
    return lines


# --------------------------------------------------------------------------------------------------------------- cases
def absorber_expect(grad, crop=None):
    _, dv = cf.absorber_pixels(absorber_chords(), ABS_SIGMA, LE)
    if crop is not None:
        x, y, w, h = crop
        dv = dv[y:y + h, x:x + w]
    z = np.zeros(3)
    return expected_grads(grad, dv, z, 0.0)


def axial_expect(grad):
    c = AXIAL_CAM
    ch = cf.pixel_chords(c["origin"], c["target"], c["up"], 2.0, 10, 6, (-1, -1, -1), (1, 1, 1), sub=8)
    _, dv = cf.absorber_pixels(ch, AXIAL_SIGMA, LE)
    return expected_grads(grad, dv, np.zeros(3), 0.0)


def slab_expect(grad, sigma=SLAB_SIGMA, albedo=SLAB_ALBEDO, g=0.4, rho=None):
    """closed form of the wide slab; rho: a grid medium of density rho, whose d_sigma_t[k] is channel k's share of d/d(scale)"""
    r = cf.slab_single_scatter(sigma, albedo, g, SLAB_D, LE)
    e = expected_grads(grad, r["d_sigma"], r["d_albedo"], r["d_g"])
    if rho is not None:
        e["sigma_t"] = e["sigma_t"] * rho
    return e, r


def image_estimate(render, spp, k=K):
    """per-channel image mean over k seeds: (mean, SE)"""
    r = np.array([render(spp=spp, seed=100 + s)[..., :3].astype(np.float64).mean((0, 1)) for s in range(k)])
    return r.mean(0), r.std(0, ddof=1) / np.sqrt(k)


# ----------------------------------------------------------------------------------------------- the reference itself
def test_reference_quadrature_derivatives():
    """The analytic slab derivatives equal float64 central differences of the quadrature (<= 1e-6 relative), and doubling the
    Gauss-Legendre nodes moves nothing by more than 1e-7."""
    sig, a = np.array([0.6, 0.9, 1.2, 0.05, 3.0]), np.array([0.5, 0.7, 0.8, 0.9, 0.3])
    le = np.array([1.0, 0.8, 0.6, 1.0, 2.0])
    for g in (0.4, -0.3, 0.0, 0.8):
        r = cf.slab_single_scatter(sig, a, g, SLAB_D, le)
        r2 = cf.slab_single_scatter(sig, a, g, SLAB_D, le, n=256)
        for key in r:
            assert np.abs(r[key] - r2[key]).max() <= 1e-7, key
        h = 1e-5
        L = lambda **kw: cf.slab_single_scatter(kw.get("s", sig), kw.get("a", a), kw.get("g", g), SLAB_D, le)["L"]
        fds = {"d_sigma": (L(s=sig + h) - L(s=sig - h)) / (2 * h), "d_albedo": (L(a=a + h) - L(a=a - h)) / (2 * h),
               "d_g": (L(g=g + h) - L(g=g - h)) / (2 * h)}
        for key, fd in fds.items():
            assert np.abs(fd - r[key]).max() <= 1e-6 * np.abs(r[key]).max(), (g, key, fd, r[key])
    # the chords' pixel-footprint mean converges as well
    a24, b48 = absorber_chords(sub=24).mean(-1), absorber_chords(sub=48).mean(-1)
    assert np.abs(a24 - b48).max() <= 2e-3


def test_reference_single_scatter_matches_monte_carlo():
    """The primal of the quadrature against the Monte-Carlo estimator of test_single_scattering_closed_form (exit distance through
    the box along uniformly drawn directions), run on the wide slab, to that test's tolerance."""
    sigma, a = 0.6, 0.9
    rng = np.random.default_rng(0)
    n = 400000
    s = rng.random(n) * SLAB_D
    z = rng.random(n) * 2 - 1; ph = rng.random(n) * 2 * np.pi
    w = np.stack([np.sqrt(1 - z * z) * np.cos(ph), np.sqrt(1 - z * z) * np.sin(ph), z], 1)
    p = np.stack([np.zeros(n), np.zeros(n), -1 + s], 1)
    half = np.array([SLAB_HALF, SLAB_HALF, 1.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(w > 0, (half - p) / w, (-half - p) / w)
    l = np.nanmin(np.where(np.isfinite(t), t, np.inf), axis=1)
    single = a * np.mean(2.0 * sigma * np.exp(-sigma * s) * np.exp(-sigma * l))
    expect = np.exp(-2 * sigma) + single
    assert cf.slab_single_scatter(sigma, a, 0.0, SLAB_D, 1.0)["L"][0] == pytest.approx(expect, rel=0.015)


def test_reference_chords_match_trace(mi, orc):
    """Chord lengths of the float64 camera at pixel centres against the oracle's ray casts: first hit and the exit behind it."""
    sc = mi.load_string(absorber_xml()); o = orc.OrcScene(sc)
    c = ABS_CAM
    org, d = cf.camera_directions(c["origin"], c["target"], c["up"], c["fov"], ABS_W, ABS_H, 1)
    d = d[:, :, 0].reshape(-1, 3)
    ch = cf.pixel_chords(c["origin"], c["target"], c["up"], c["fov"], ABS_W, ABS_H, (-1, -1, -1), (1, 1, 1), sub=1)[..., 0].reshape(-1)
    t0, _, _, prim = o.trace(np.broadcast_to(org, d.shape), d)
    hit = prim != 0xffffffff
    assert (hit == (ch > 0)).all()
    assert hit.sum() > 100 and (~hit).sum() > 30 and ch.max() > 2.8
    eps = 1e-3
    t1, _, _, prim1 = o.trace(org + d[hit] * (t0[hit, None] + eps), d[hit])
    assert (prim1 != 0xffffffff).all()
    assert np.abs(t1 + eps - ch[hit]).max() <= 1e-4


# ------------------------------------------------------------------------------------------- the cases (shared with the GPU module)
ORACLE_SE = 0.03
NAN3 = np.full(3, np.nan)


def case_absorber(variant):
    """(a) pure absorber per pixel: d_sigma_t[k] = sum_p grad_pk mean_footprint(-l Le_k exp(-sigma_k l)).  d_albedo and d_g are exactly
    0: PRB multiplies the local derivatives by Lo, the radiance still to be collected, which is 0 after any real collision at albedo 0
    (the reference's detached Lo cannot see in-scattering there either).  Variants: an rgba film whose grad is nonzero only in alpha
    (every gradient exactly 0), a crop window at odd offsets (crop_offset indexing of lane_delta_L), a grad image nonzero in one pixel.
    Returns (xml, grad, expect, zero)."""
    crop = (3, 1, 17, 7) if variant == "crop" else None
    xml = absorber_xml(pixel_format="rgba" if variant == "alpha" else "rgb", crop=crop)
    H, W = (crop[3], crop[2]) if crop else (ABS_H, ABS_W)
    grad = grad_image((H, W, 4 if variant == "alpha" else 3))
    if variant == "alpha":
        grad[..., :3] = 0.0
        return xml, grad, {k: np.zeros(3) for k in ("sigma_t", "albedo")} | {"g": 0.0}, {"sigma_t": True, "albedo": True, "g": True}
    if variant == "pixel":
        keep = grad[4, 7].copy(); grad[:] = 0.0; grad[4, 7] = keep          # chord ~1, its neighbours' differ by ~1/3
    return xml, grad, absorber_expect(grad, crop), {"albedo": True, "g": True}


def case_filter(rfilter):
    """(b) non-box filters on the axial slab (every pixel Le exp(-2 sigma), border pixels included): the weight-film path of the adjoint
    (lane_delta_L's footprint loop, the wfilm pass) must give the box-filter closed form."""
    xml = axial_absorber_xml(rfilter)
    grad = grad_image((6, 10, 3), seed=1)
    return xml, grad, axial_expect(grad), {"albedo": True, "g": True}


def case_slab(g, sample_emitters):
    """(c) single scattering in the wide slab, max_depth 2: d_sigma_t, d_albedo, d_g against the quadrature.  sample_emitters true: the g
    term comes from NEE at the scatter; false: from phase sampling."""
    xml = slab_xml(g=g, sample_emitters=sample_emitters)
    grad = grad_image((8, 8, 3), seed=2)
    return xml, grad, slab_expect(grad, g=g)[0], None


def case_het(mi, tmp_path, ratio):
    """(d) a constant grid of density rho with a loose majorant (ratio = majorant / rho): most collisions are null, ratio tracking runs on
    the NEE march.  d_sigma_t[k] is channel k's share of d/d(scale) = rho dL_k/dsigma; albedo and g as in (c)."""
    rho = 1.0 / ratio
    xml = het_slab_xml(mi, tmp_path, rho, 1.0)
    grad = grad_image((8, 8, 3), seed=3)
    return xml, grad, slab_expect(grad, sigma=HET_SIGMA, rho=rho)[0], None


def case_zero(mi, tmp_path, which):
    """(e) a zero channel (k = 1), wide slab, HG g = 0.4.
    albedo_k = 0: d_albedo[k] == 0 (PRB's Lo is 0 after a real collision in channel k) and d_sigma_t[k] = -d Le_k exp(-sigma_k d) sum grad_k,
      which here is also the true derivative; the other channels follow the (c) closed form.  'het': the grid medium with a loose
      majorant, d_sigma_t[k] channel k's share of d/d(scale) (the same forms times rho).
    sigma_k = 0: passing paths carry weight_k = 1 / pdf and the term -t * weight_k * Lo, whose expectation is -d Le_k; every real scatter
      has weight_k = sigma_k a_k (...) = 0 and nothing left to collect in channel k.  So d_sigma_t[k] = -d Le_k sum grad_k and
      d_albedo[k] == 0, the reference's PRB answer (the true derivative also holds the single-scattering slope).  The other channels are
      NOT the slab integral: with hero channel k the one-channel free-flight pdf never samples a collision, so their scattered light is
      missed in a third of the paths; they are only compared with the oracle (GPU module)."""
    grad = grad_image((8, 8, 3), seed=4)
    zero = {"albedo": np.array([False, True, False])}
    if which == "albedo":
        al = np.array([0.5, 0.0, 0.8])
        return slab_xml(albedo=al), grad, slab_expect(grad, albedo=al)[0], zero
    if which == "het":
        al = np.array([0.5, 0.0, 0.8]); rho = 0.4
        return het_slab_xml(mi, tmp_path, rho, 1.0, albedo=al), grad, slab_expect(grad, sigma=HET_SIGMA, albedo=al, rho=rho)[0], zero
    st = np.array([0.6, 0.0, 1.2])
    ds = NAN3.copy(); ds[1] = -SLAB_D * LE[1] * grad[..., 1].astype(np.float64).sum()
    return slab_xml(sigma=st), grad, {"sigma_t": ds, "albedo": NAN3, "g": np.nan}, zero


def _oracle_check(mi, orc, xml, grad, expect, zero, spp, k=K):
    o = orc.OrcScene(mi.load_string(xml))
    assert o.film_shape == grad.shape
    return check(seed_split(o.render_backward, grad, spp, k), expect, ORACLE_SE, zero)


@pytest.mark.parametrize("variant", ["plain", "alpha", "crop", "pixel", "spp8"])
def test_absorber_gradients(mi, orc, variant):
    """(a); 'spp8': 8 samples per pixel over 32 seeds, where the box filter's 1/spp normalisation of delta_L shows (1/(spp+1) is 11 % off)"""
    if variant == "spp8":
        _oracle_check(mi, orc, *case_absorber("plain"), spp=8, k=32)
    else:
        _oracle_check(mi, orc, *case_absorber(variant), spp=2048 if variant == "pixel" else 512)


@pytest.mark.parametrize("rfilter", ["tent", "gaussian"])
def test_filter_gradients(mi, orc, rfilter):
    _oracle_check(mi, orc, *case_filter(rfilter), spp=1024)


@pytest.mark.parametrize("g", [0.4, -0.3])
@pytest.mark.parametrize("sample_emitters", [True, False])
def test_single_scatter_gradients(mi, orc, g, sample_emitters):
    xml, grad, expect, zero = case_slab(g, sample_emitters)
    _oracle_check(mi, orc, xml, grad, expect, zero, spp=4096)
    o = orc.OrcScene(mi.load_string(xml))
    m, se = image_estimate(lambda spp, seed: o.render(spp=spp, seed=seed, integrator="prbvolpath"), 1024)
    L = cf.slab_single_scatter(SLAB_SIGMA, SLAB_ALBEDO, g, SLAB_D, LE)["L"]
    assert (np.abs(m - L) <= 4 * se + 1e-6).all() and (se <= 0.01 * L).all(), (m, L, se)


@pytest.mark.parametrize("ratio", [2.5, 1.25])
def test_heterogeneous_constant_grid_gradients(mi, orc, tmp_path, ratio):
    _oracle_check(mi, orc, *case_het(mi, tmp_path, ratio), spp=4096)


@pytest.mark.parametrize("which", ["albedo", "sigma_t", "het"])
def test_zero_channel_gradients(mi, orc, tmp_path, which):
    _oracle_check(mi, orc, *case_zero(mi, tmp_path, which), spp=4096)
