"""Every route into a film against the oracle's film, on shapes chosen for the corners of the film code (csrc/film.h): the Cornell box on
a 9 x 5 film at 3 samples per pixel (not a power of two; 135 lanes: two full waves and a partial one) and at 4.

Routes: colour (lrt_render: finish_paths_wave for the box filter, k_splat_lanes for wide ones), `moment` (k_moment_splat), `aov` with a
3-wide and a 1-wide AOV (k_aov), and the PRB adjoint, whose weight film (k_splat_lanes<true>) and footprint loop (lane_delta_L) show in
the gradients of test_prb_closed_form.case_filter's scene.
Filters: box, tent radius 1 (3 x 3 cells), the default Gaussian (5 x 5) and a Gaussian of stddev 1: 9 x 9 = 81 cells, two chunks of the
walk and wider than the film, so that every footprint is cut by the bounds test; and (colour, moment) a Gaussian of stddev 2: 17 x 17 = 289
cells, five chunks, far wider than the film.
Switches: pixel_format rgb / rgba, a 5 x 3 crop window at (2, 1), tile shards 0 / 2 and 1 / 2 summed, samples_per_pass = 1 (three
passes), 4 samples per pixel.  Each switch appears with each route that has it.

What the film is held to: colour, the oracle's film.  moment and aov, which the oracle does not render: the float64 accumulation of the
oracle's lanes (moment_ref.film_record; test_aov_gpu.reference_lanes) through the oracle's jitter and filter, as test_moment_gpu and
test_aov_gpu do.  PRB: the oracle's gradients for the same seed.  Bound: test_parity_gpu.film_close, 8e-5 of the pixel's largest raw
channel (of the largest gradient for PRB); W of a box film is exactly spp.

Combinations left out, and why:
  - tile shards at 9 x 5: tiles are 32 x 32 pixels, so rank 1 of 2 would own nothing and rank 0's pixel list would be the identity.  The
    tile cases use a 33 x 5 film instead: two tiles, 32 and 1 pixels wide, and a list that is not the identity.
  - aov x tile shards: lrt_render_aov rejects tile sharding.
  - PRB x samples_per_pass: the adjoint renders in one pass (as the reference's).
  - moment x samples_per_pass, the three second-moment channels: the oracle gives per-lane radiance of the first pass only, and m2 is
    not linear in it.  R, G, B, [A], W are the oracle's multi-pass film and X, Y, Z its image under srgb_to_xyz (linear).
  - aov x samples_per_pass, the AOV channels: the same (first-pass lanes only).  W is the oracle's multi-pass colour film's W, which
    depends on every lane's jitter in every pass."""
import numpy as np
import pytest

import moment_ref
from test_parity_gpu import film_close
from test_prb_closed_form import case_filter, grad_image

pytestmark = pytest.mark.gpu

W, H, W_TILES = 9, 5, 33
CROP = dict(crop_offset_x=2, crop_offset_y=1, crop_width=5, crop_height=3)
FILTERS = {"box": {"type": "box"}, "tent": {"type": "tent", "radius": 1.0}, "gaussian": {"type": "gaussian"},
           "gaussian1": {"type": "gaussian", "stddev": 1.0}, "gaussian2": {"type": "gaussian", "stddev": 2.0}}
FOOTPRINT = {"box": 1, "tent": 3, "gaussian": 5, "gaussian1": 9, "gaussian2": 17}
XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])


def footprint(F):
    """cells per side of a sample's footprint: 2 ceil(radius - 0.5) + 1 (imageblock.cpp:431-447)"""
    radius = {0: 0.5, 1: 4.0 * F.rfilter_param, 2: F.rfilter_param}[F.rfilter]
    return 2 * int(np.ceil(np.float32(radius) - np.float32(0.5))) + 1


def case(rfilter, fmt="rgb", spp=3, crop=False, tiles=False, spass=None):
    name = "-".join([rfilter, fmt] + (["spp4"] if spp == 4 else []) + (["crop"] if crop else []) + (["tiles"] if tiles else []) + (["passes"] if spass else []))
    return pytest.param(dict(rfilter=rfilter, fmt=fmt, spp=spp, crop=crop, tiles=tiles, spass=spass), id=name)


def cornell(mi, c, integrator=None):
    """The Cornell box of mi.cornell_box() under case c; integrator(inner) wraps the path integrator (moment, aov)."""
    d = mi.cornell_box()
    inner = dict(d["integrator"], **({"samples_per_pass": c["spass"]} if c["spass"] else {}))
    d["integrator"] = integrator(inner) if integrator else inner
    if integrator and c["spass"]:
        d["integrator"]["samples_per_pass"] = c["spass"]
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": c["spp"]}
    d["sensor"]["film"].update(width=W_TILES if c["tiles"] else W, height=H, rfilter=dict(FILTERS[c["rfilter"]]), pixel_format=c["fmt"])
    if c["crop"]:
        d["sensor"]["film"].update(CROP)
    sc = mi.load_dict(d)
    F = sc.desc.film
    assert footprint(F) == FOOTPRINT[c["rfilter"]] and (F.crop_width, F.crop_height) == ((5, 3) if c["crop"] else (W_TILES if c["tiles"] else W, H))
    return sc


def render_raw(sc, c, **kw):
    """The scene's raw film; tile cases: the sum of the two ranks' films (both own pixels)."""
    if not c["tiles"]:
        return sc.render(return_raw=True, **kw)[1]
    parts = [sc.render(return_raw=True, tile_rank=r, tile_count=2, **kw)[1] for r in range(2)]
    assert all(p.any() for p in parts)
    return parts[0] + parts[1]


def accumulate(O, F, spx, spy, rec):
    """float64 film of the records rec (n, C) of samples at (spx, spy) through the oracle's filter (ImageBlock::put, imageblock.cpp:431-500)."""
    count = footprint(F); rad = count // 2
    film = np.zeros((F.crop_height, F.crop_width, rec.shape[1]))
    for k in range(len(rec)):
        x0, y0 = int(np.floor(spx[k])) - rad, int(np.floor(spy[k])) - rad
        for ys in range(count):
            wy = O.rfilter_eval(np.float32(np.float32(y0) + np.float32(0.5) - spy[k]) + np.float32(ys))
            for xs in range(count):
                x, y = x0 + xs - F.crop_offset_x, y0 + ys - F.crop_offset_y
                if 0 <= x < F.crop_width and 0 <= y < F.crop_height:
                    wx = O.rfilter_eval(np.float32(np.float32(x0) + np.float32(0.5) - spx[k]) + np.float32(xs))
                    film[y, x] += rec[k].astype(np.float64) * (float(wy) * float(wx))
    return film


def assert_film(got, want, what):
    ok = film_close(got, want)
    scale = np.maximum(np.abs(want).max(axis=-1, keepdims=True), 1.0)
    print(f"{what}: max |film - reference| / largest channel of the pixel = {np.max(np.abs(got - want) / scale):.3g} (bound 8e-5)")
    assert ok.all(), (what, np.argwhere(~ok)[:5])


def assert_box_weight(raw, wi, c):
    if c["rfilter"] == "box":
        assert np.array_equal(raw[..., wi], np.full(raw.shape[:2], float(c["spp"]), np.float32))


# ------------------------------------------------------------------------------------------------------------ colour
@pytest.mark.parametrize("c", [case("box"), case("box", "rgba", tiles=True), case("tent", "rgba", crop=True), case("gaussian", tiles=True),
                               case("gaussian", spp=4), case("gaussian1", "rgba"), case("gaussian1", spass=1), case("gaussian2", "rgba")])
def test_colour_film(mi, orc, c):
    sc = cornell(mi, c)
    raw = render_raw(sc, c)
    _, oraw = orc.OrcScene(sc).render(return_raw=True)
    assert raw.shape[-1] == (5 if c["fmt"] == "rgba" else 4) and oraw[..., :3].max() > 0
    assert_film(raw, oraw, "colour")
    assert_box_weight(raw, -1, c)


# ------------------------------------------------------------------------------------------------------------ moment
@pytest.mark.parametrize("c", [case("box", "rgba", crop=True), case("tent", tiles=True), case("gaussian", "rgba", spp=4), case("gaussian1"),
                               case("gaussian1", "rgba", spass=1), case("gaussian2")])
def test_moment_film(mi, orc, c):
    from test_moment_gpu import oracle_jitter
    sc = cornell(mi, c, lambda inner: {"type": "moment", "img": inner})
    raw = render_raw(sc, c)
    F = sc.desc.film; O = orc.OrcScene(sc)
    wi = 4 if c["fmt"] == "rgba" else 3
    assert raw.shape[-1] == wi + 7
    if c["spass"]:
        _, oraw = O.render(return_raw=True)
        want = np.concatenate([oraw.astype(np.float64), oraw[..., :3].astype(np.float64) @ XYZ.T], axis=-1)
        raw = raw[..., :wi + 4]
    else:
        n = F.crop_width * F.crop_height * c["spp"]
        pix = np.arange(n) // c["spp"]
        jit = oracle_jitter(orc, sc, n)
        spx = np.float32(pix % F.crop_width + F.crop_offset_x) + jit[:, 0]; spy = np.float32(pix // F.crop_width + F.crop_offset_y) + jit[:, 1]
        want = accumulate(O, F, spx, spy, moment_ref.film_record(O.render_samples(0, n), True, c["fmt"] == "rgba"))
    assert want[..., wi + 1].max() > 0
    assert_film(raw, want, "moment")
    assert_box_weight(raw, wi, c)


# --------------------------------------------------------------------------------------------------------------- aov
@pytest.mark.parametrize("c", [case("box", crop=True), case("tent", "rgba"), case("gaussian", spp=4), case("gaussian1", crop=True),
                               case("gaussian1", spass=1)])
def test_aov_film(mi, orc, c):
    from test_aov_gpu import reference_lanes
    sc = cornell(mi, c, lambda inner: {"type": "aov", "aovs": "g:geo_normal,d:depth", "image": inner})
    _, raw = sc.render(return_raw=True)
    F = sc.desc.film; O = orc.OrcScene(sc)
    assert raw.shape == (F.crop_height, F.crop_width, 5)
    if c["spass"]:
        _, oraw = O.render(return_raw=True)
        assert_film(raw[..., 4:], oraw[..., -1:], "aov W")
        return
    ref = reference_lanes(mi, orc, sc, 0, F.crop_width * F.crop_height * c["spp"])
    rec = np.concatenate([ref["geo_normal"], ref["depth"], np.ones_like(ref["depth"])], axis=1)
    assert ref["valid"].any()
    assert_film(raw, accumulate(O, F, ref["spx"], ref["spy"], rec), "aov")
    assert_box_weight(raw, 4, c)


# --------------------------------------------------------------------------------------------------------------- PRB
@pytest.mark.parametrize("c", [case("box", crop=True), case("tent", "rgba", tiles=True), case("gaussian", crop=True), case("gaussian1", spp=4)])
def test_prb_weight_film(mi, orc, c):
    """The adjoint's delta_L divides by the weight film; the gradients of the axial absorber (case_filter) against the oracle's."""
    f = FILTERS[c["rfilter"]]
    rf = f'<rfilter type="{f["type"]}">' + "".join(f'<float name="{k}" value="{v}"/>' for k, v in f.items() if k != "type") + "</rfilter>"
    crop = "".join(f'<integer name="{k}" value="{v}"/>' for k, v in CROP.items()) if c["crop"] else ""
    xml = case_filter("tent")[0]
    for old, new in (('<integer name="width" value="10"/>', f'<integer name="width" value="{W_TILES if c["tiles"] else W}"/>'),
                     ('<integer name="height" value="6"/>', f'<integer name="height" value="{H}"/><string name="pixel_format" value="{c["fmt"]}"/>{crop}'),
                     ('<rfilter type="tent"/>', rf)):
        assert xml.count(old) == 1
        xml = xml.replace(old, new)
    sc = mi.load_string(xml)
    assert footprint(sc.desc.film) == FOOTPRINT[c["rfilter"]]
    grad = grad_image(sc.film_shape(), seed=9)
    kw = dict(spp=c["spp"], seed=3)
    want = orc.OrcScene(sc).render_backward(grad, **kw)
    parts = [sc.render_backward(grad, tile_rank=r, tile_count=2, **kw) for r in range(2)] if c["tiles"] else [sc.render_backward(grad, **kw)]
    got = {k: sum(np.asarray(p[k], np.float64) for p in parts) for k in ("sigma_t", "albedo", "g")}
    scale = np.abs(want["sigma_t"]).max()
    err = np.abs(got["sigma_t"] - want["sigma_t"]).max()
    print(f"PRB: sigma_t gradient {got['sigma_t']} against {want['sigma_t']}: max error / largest = {err / scale:.3g} (bound 8e-5)")
    assert scale > 0 and err <= 8e-5 * scale
    assert np.all(got["albedo"] == 0) and got["g"] == 0 and np.all(want["albedo"] == 0) and want["g"] == 0          # a pure absorber
