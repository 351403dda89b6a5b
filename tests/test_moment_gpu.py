"""GPU tests of the `moment` integrator (src/integrators/moment.cpp): the per-lane moment values are
tests/moment_ref.py applied to the oracle's lanes bit for bit, the film is a float64 accumulation of those lanes within the
float32 summation bound, closed forms on a scene whose samples take two values, passes and shards, the Z-test of
src/render/tests/test_renders.py:159-228 used as intended, and the EXR round trip.

The summation bound (used wherever "the bound" is said below): a float32 sum of n terms in any order differs from the exact sum
by at most (n - 1) 2^-24 sum|term| to first order; every term value * w carries up to two more roundings (w = wy * wx, then the
product), so |device - exact| <= 2 n 2^-24 sum|term| per pixel and channel, n counting the samples with a nonzero weight there."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import moment_ref
from conftest import LIVER_XML
from scene_gen import fog_xml

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LE = np.float32([18.387, 13.9873, 6.75357])          # the Cornell box's light (mi.cornell_box)


# ----------------------------------------------------------------------------------------------------------- scenes
def cornell_moment(mi, size=16, spp=5, sampler="independent", rfilter="box", fmt="rgb", spass=None, integ=None, crop=None):
    d = mi.cornell_box()
    m = {"type": "moment", "img": integ or d["integrator"]}
    if spass:
        m["samples_per_pass"] = spass
    d["integrator"] = m
    d["sensor"]["sampler"] = {"type": sampler, "sample_count": spp}
    d["sensor"]["film"].update(width=size, height=size, rfilter={"type": rfilter}, pixel_format=fmt)
    if crop:
        d["sensor"]["film"].update(crop_offset_x=crop[0], crop_offset_y=crop[1], crop_width=crop[2], crop_height=crop[3])
    return mi.load_dict(d)


def cornell_fog_moment(mi, integ, size, spp):
    """test_oracle_pins.cornell_fog_scene (MitsubaRunner.py:8-40) under a moment integrator, box filter."""
    d = mi.cornell_box()
    d["fog_medium_id"] = {"type": "homogeneous", "sigma_t": {"type": "rgb", "value": [0.2, 0.2, 0.2]},
                          "albedo": {"type": "rgb", "value": [0.75, 0.75, 0.75]}, "scale": 2.5, "phase": {"type": "isotropic"}}
    d["integrator"] = {"type": "moment", "img": {"type": integ, "max_depth": -1}}
    d["sensor"]["film"].update({"width": size, "height": size, "rfilter": {"type": "box"}})
    d["sensor"]["sampler"]["sample_count"] = spp
    d["sensor"]["medium"] = {"type": "ref", "id": "fog_medium_id"}
    return mi.load_dict(d)


def wrap_file(mi, xml, base_dir, **defines):
    """A scene text with its integrator element nested into a moment integrator under the name `img`."""
    xml, n = re.subn(r'<integrator type="([^"]+)">(.*?)</integrator>', r'<integrator type="moment"><integrator type="\1" name="img">\2</integrator></integrator>',
                     xml, count=1, flags=re.S)
    assert n == 1
    return mi.load_string(xml, base_dir, **defines)


def plain_render(mi, sc, **kw):
    """lrt_render of the scene's description (the nested integrator alone): its raw film."""
    h, w, _ = sc.film_shape()
    raw = np.empty((h, w, sc.raw_channels()), np.float32)
    o = mi._lib.make_opts(**kw)
    mi._lib.check(sc._lib.lrt_render(sc._h, C.byref(o), raw.ctypes.data, None))
    return raw


def is_path(sc):
    return sc.desc.integrator.type == 0


def check_lanes(orc, sc, begin, n):
    want = moment_ref.moment_lanes(orc.OrcScene(sc).render_samples(begin, n), is_path(sc))
    got = sc.render_moment_samples(begin, n)
    assert got.shape == (n, 6)
    same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
    assert same.all(), f"{(~same).sum()} of {n} lanes differ, first at {begin + int(np.argmin(same))}: {got[np.argmin(same)]} != {want[np.argmin(same)]}"
    assert (want[:, 1] > 0).any()
    return want


# ------------------------------------------------------------------------------------------------ 1. lanes, bit for bit
def test_lanes_cornell_path(mi, orc):
    sc = cornell_moment(mi, size=32, spp=4, rfilter="gaussian")
    check_lanes(orc, sc, 0, 32 * 32 * 4)
    check_lanes(orc, sc, 1237, 1003)                    # a window aligned to neither a pixel (4 lanes) nor a wave (64)


@pytest.mark.parametrize("integrator", ["volpath", None])
def test_lanes_liver(mi, orc, integrator):
    """Liver-SingleMesh small: volpath, and the file's own default (biovolpath on the liver medium)."""
    kw = dict(spp=4, res_width=64, res_height=36)
    if integrator:
        kw["integrator"] = integrator
    sc = wrap_file(mi, open(LIVER_XML).read(), os.path.dirname(LIVER_XML), **kw)
    assert sc.desc.integrator.type == (1 if integrator else 3)
    check_lanes(orc, sc, 0, 64 * 36 * 4)
    check_lanes(orc, sc, 3001, 777)


def test_lanes_fog_volpathmis(mi, orc):
    sc = wrap_file(mi, fog_xml(rf="box").replace('<integrator type="volpath">', '<integrator type="volpathmis">'), ".")
    assert sc.desc.integrator.type == 5
    check_lanes(orc, sc, 32 * (64 * 20 + 11) + 5, 20011)


# ------------------------------------------------------------------- 2. film against a float64 accumulation of the lanes
def oracle_jitter(orc, sc, n, seed=0):
    d = sc.desc; L = orc.lib(); out = (C.c_float * 2)(); jit = np.empty((n, 2), np.float32)
    assert d.sampler_type == 0
    for lane in range(n):
        L.orc_lane_stream(d.sampler_seed, seed, lane, 2, out)
        jit[lane] = out[0], out[1]
    return jit


def exact_film(orc, sc):
    """(film, abs_film, count): the float64 accumulation of tests/moment_ref.film_record of the oracle's lanes with the oracle's jitter
    and filter weights, the same sum of absolute values, and the number of contributing samples per pixel."""
    d = sc.desc; F = d.film
    w, h, spp = F.crop_width, F.crop_height, d.sample_count
    n = w * h * spp
    O = orc.OrcScene(sc)
    rec = moment_ref.film_record(O.render_samples(0, n), is_path(sc), bool(F.has_alpha)).astype(np.float64)
    jit = oracle_jitter(orc, sc, n)
    radius = {0: 0.5, 1: 4.0 * F.rfilter_param, 2: F.rfilter_param}[F.rfilter]
    rad = int(np.ceil(np.float32(radius) - np.float32(0.5)))
    film = np.zeros((h, w, rec.shape[1])); absf = np.zeros_like(film); count = np.zeros((h, w), np.int64)
    for k in range(n):
        pix = k // spp
        spx = np.float32(pix % w + F.crop_offset_x) + jit[k, 0]; spy = np.float32(pix // w + F.crop_offset_y) + jit[k, 1]
        x0, y0 = int(np.floor(spx)) - rad, int(np.floor(spy)) - rad
        for ys in range(2 * rad + 1):
            wy = O.rfilter_eval(np.float32(np.float32(y0) + np.float32(0.5) - spy) + np.float32(ys))
            for xs in range(2 * rad + 1):
                wx = O.rfilter_eval(np.float32(np.float32(x0) + np.float32(0.5) - spx) + np.float32(xs))
                x, y = x0 + xs - F.crop_offset_x, y0 + ys - F.crop_offset_y
                if 0 <= x < w and 0 <= y < h and wy * wx != 0.0:
                    term = rec[k] * (float(wy) * float(wx))
                    film[y, x] += term; absf[y, x] += np.abs(term); count[y, x] += 1
    return film, absf, count


@pytest.mark.parametrize("fmt", ["rgb", "rgba"])
@pytest.mark.parametrize("rfilter", ["box", "gaussian", "tent"])
def test_film_is_the_float64_accumulation_of_the_lanes(mi, orc, rfilter, fmt):
    from test_parity_gpu import film_close
    sc = cornell_moment(mi, size=16, spp=5, rfilter=rfilter, fmt=fmt)
    img, raw = sc.render(return_raw=True)
    m = sc.moment_desc()
    assert raw.shape == (16, 16, m.n_raw_channels) and img.shape == (16, 16, m.n_channels)
    film, absf, count = exact_film(orc, sc)
    bound = 2.0 * count[..., None] * U * absf
    err = np.abs(raw.astype(np.float64) - film)
    print(f"{rfilter} {fmt}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}, samples per pixel {count.min()} .. {count.max()}")
    assert (err <= bound).all(), np.argwhere(err > bound)[:5]
    assert (film[..., 5 if fmt == "rgba" else 4] > 0).any()
    # the colour part is the plain render's film
    wi = 4 if fmt == "rgba" else 3
    assert film_close(raw[..., :wi + 1], plain_render(mi, sc)).all()
    # develop: every channel but W over W
    W = raw[..., wi:wi + 1].astype(np.float64)
    dev = np.delete(raw.astype(np.float64), wi, axis=2) / np.where(W == 0, 1, W)
    np.testing.assert_allclose(img, dev, rtol=2 * U, atol=0)


def test_film_with_a_crop_window(mi, orc):
    sc = cornell_moment(mi, size=24, spp=3, rfilter="tent", crop=(5, 7, 12, 9))
    _, raw = sc.render(return_raw=True)
    assert raw.shape == (9, 12, 10)
    film, absf, count = exact_film(orc, sc)
    assert (np.abs(raw.astype(np.float64) - film) <= 2.0 * count[..., None] * U * absf).all()


# -------------------------------------------------------------------------------------------------------- 3. closed form
def xyz_of_le():
    return moment_ref.moment_values(LE[None])[0, :3].astype(np.float64)


def check_two_valued_film(raw, n):
    """path with max_depth = 1 on the Cornell box: a sample is 0 or the light's radiance, so per pixel and channel
    m2_c W = XYZ_c(Le) (m1_c W) exactly; both sides are float32 sums of n terms (the bound), the squares carry one rounding each."""
    x, m2 = raw[..., 4:7].astype(np.float64), raw[..., 7:10].astype(np.float64)
    rhs = xyz_of_le() * x
    bound = 2.0 * n * U * (m2 + rhs)
    assert (x > 0).any()
    assert (np.abs(m2 - rhs) <= bound).all()
    # linearity: sum X = row . (sum R, sum G, sum B) within the bound (three roundings per sample on the left, none on the right)
    lin = raw[..., :3].astype(np.float64) @ moment_ref.SRGB_TO_XYZ.astype(np.float64).T
    assert (np.abs(x - lin) <= 2.0 * n * U * (x + lin) + 3 * U * lin).all()


def test_closed_form_two_valued_samples(mi):
    spp = 6
    sc = cornell_moment(mi, size=64, spp=spp, integ={"type": "path", "max_depth": 1})
    img, raw = sc.render(return_raw=True)
    assert np.array_equal(raw[..., 3], np.full((64, 64), float(spp), np.float32))
    check_two_valued_film(raw, spp)
    var, mean = mi.moment_variance(img, sc, spp)
    light = raw[..., 0] >= (spp - 0.5) * LE[0]; black = raw[..., 0] == 0
    assert light.sum() >= 4 and black.sum() > 1000 and (~light & ~black).any()
    assert (var[black] == 0).all() and (mean[black] == 0).all()
    # a pixel that sees only the light: m1 = X(Le) and m2 = X(Le)^2, each a sum within the bound and one division:
    # |m2 - m1^2| <= (2 n + 1) 2^-24 (m2 + 2 m1^2), and the variance of the mean is that over n - 1
    X = xyz_of_le()
    np.testing.assert_allclose(mean[light], np.broadcast_to(X, mean[light].shape), rtol=(2 * spp + 1) * U)
    assert (var[light] <= (2 * spp + 1) * U * 3 * X * X / (spp - 1)).all()
    assert (var[~light & ~black].max(axis=-1) > 1.0).all()          # a mixed pixel has a real variance


# -------------------------------------------------------------------------------------------------- 4. passes and shards
@pytest.mark.parametrize("sampler", ["independent", "ldsampler"])
def test_split_render(mi, sampler):
    """A render split by samples_per_pass draws other samples than the one-pass render, in the reference and here (a lane is seeded
    by its index in the pass's wavefront, pixel * spp_per_pass + s; the oracle's films of the two differ by more than 10 % per pixel),
    so the two films agree only statistically.  What must hold exactly, and is asserted with the bound: the colour part of the split
    moment film is the plain split render's film (the pass-state carry is the plain render's), and the moment channels of EVERY pass
    are formed from that pass's samples: the two-valued closed form and the linearity of X, Y, Z in the film hold over all passes, as
    they do for the one-pass film.  That the plain split film is the reference's is test_parity_gpu's
    test_multi_pass_render_matches_oracle; no statistical comparison with the one-pass film is made here."""
    from test_parity_gpu import film_close
    spp, integ = 16, {"type": "path", "max_depth": 1}
    one = cornell_moment(mi, size=48, spp=spp, sampler=sampler, integ=integ)
    split = cornell_moment(mi, size=48, spp=spp, sampler=sampler, integ=integ, spass=4)
    assert split.desc.samples_per_pass == 4 and one.desc.samples_per_pass == 0
    _, raw1 = one.render(return_raw=True, seed=3)
    _, raw4 = split.render(return_raw=True, seed=3)
    assert split.stats()["n_launches"] >= 4 and split.stats()["n_samples"] == 48 * 48 * spp
    assert np.array_equal(raw4[..., 3], np.full((48, 48), float(spp), np.float32))
    check_two_valued_film(raw1, spp); check_two_valued_film(raw4, spp)
    assert film_close(raw4[..., :4], plain_render(mi, split, seed=3)).all()
    assert not np.array_equal(raw1, raw4)


def test_split_render_wide_filter_carries_the_jitter(mi):
    """Gaussian filter and the independent sampler: W depends on every lane's jitter in every pass."""
    from test_parity_gpu import film_close
    sc = cornell_moment(mi, size=24, spp=8, rfilter="gaussian", spass=2, fmt="rgba")
    _, raw = sc.render(return_raw=True, seed=1)
    assert film_close(raw[..., :5], plain_render(mi, sc, seed=1)).all()


@pytest.mark.parametrize("rfilter", ["box", "tent"])
def test_tile_shards_add_up(mi, rfilter):
    spp = 6
    sc = cornell_moment(mi, size=80, spp=spp, rfilter=rfilter)
    _, whole = sc.render(return_raw=True, seed=5)
    parts = [sc.render(return_raw=True, seed=5, tile_rank=r, tile_count=2)[1].astype(np.float64) for r in range(2)]
    assert all((p[..., 3] > 0).any() and (p[..., 3] == 0).any() for p in parts) or rfilter != "box"
    total = parts[0] + parts[1]
    # every channel is a sum of non-negative terms here (Cornell box: radiance, weights and squares >= 0): sum|term| is the film itself.
    # Box: n = spp samples per pixel; tent (radius 1): the samples of the 3 x 3 neighbourhood.
    n = spp if rfilter == "box" else 9 * spp
    assert (np.abs(total - whole) <= 2.0 * n * U * np.maximum(total, whole)).all()
    if rfilter == "box":
        assert np.array_equal(total[..., 3], np.full((80, 80), float(spp)))


# ------------------------------------------------------------------------------------------ 5. the Z-test, used as intended
def test_z_test_accepts_what_agrees_and_rejects_a_ten_percent_error(mi):
    """The fog Cornell box (MitsubaRunner.py:8-40) under `moment`, Y channel, box filter, the reference's condition: alpha = 0.01 with
    Sidak correction, at least 99.75 % of the pixels pass (test_renders.py:159-176, 203-228).

    Resolution and spp were fixed from the CPU oracle's lanes through tests/moment_ref.py, before any device render.  The medium makes
    every pixel noisy: at 48 x 48 x 256 spp the best pixel's standard error of the mean is 11 % and the test cannot tell a 10 % error
    (z <= 0.6 everywhere; the oracle ACCEPTS the image scaled by 1.1), and at 48 x 48 x 4096 still z <= 2.0.  A rejection needs
    z > 4.1 (the corrected level of 256 pixels), i.e. a standard error below 1.6 %: 16 x 16 pixels at 65536 spp, 2^24 samples, the
    same count as a 256 x 256 x 256 render.  There the oracle alone gives: seed 0 against seed 1 100 % of the pixels pass
    (min p = 0.0081), volpath seed 0 against volpathmis seed 2 100 %, seed 0 against itself scaled by 1.1 59 % (median z = 3.8,
    best pixel z = 5.8).

    With 256 pixels the 99.75 % condition allows no failure (255 / 256 = 99.6 %): ONE failing pixel fails an accepting comparison.
    The corrected level is p > 3.9e-5; the oracle's smallest p of the accepting comparisons is 0.0029, a factor 70 above it."""
    size, spp = 16, 65536

    def render(integ, seed):
        sc = cornell_fog_moment(mi, integ, size, spp)
        img = sc.render(seed=seed)
        assert np.isfinite(img).all()
        var, mean = mi.moment_variance(img, sc, spp)
        return mean[..., 1], var[..., 1]
    a, b, c = render("volpath", 0), render("volpath", 1), render("volpathmis", 2)
    zero = (a[1] == 0) & (b[1] == 0)
    p, frac_ab = mi.z_test(a[0], a[1], b[0], b[1])
    _, frac_mis = mi.z_test(a[0], a[1], c[0], c[1])
    _, frac_scaled = mi.z_test(a[0], a[1], a[0] * 1.1, a[1] * 1.21)
    print(f"seed A / seed B: {frac_ab:.4f} (min p {p.min():.3g}); volpath / volpathmis: {frac_mis:.4f}; A / 1.1 A: {frac_scaled:.4f}; pixels without variance: {zero.sum()}")
    assert frac_ab >= 0.9975
    assert frac_mis >= 0.9975
    assert frac_scaled < 0.9975


# ----------------------------------------------------------------------------------------------------- 6. EXR round trip
def test_exr_round_trip(mi, tmp_path):
    sc = cornell_moment(mi, size=32, spp=4, fmt="rgba")
    img = mi.render(sc)
    names = sc.moment_channel_names()
    assert img.shape == (32, 32, len(names)) and len(names) == 10
    p = tmp_path / "moment.exr"
    mi.write_exr(p, img, channel_names=names)
    bmp = mi.Bitmap(os.fspath(p))
    assert sorted(bmp.channel_names) == sorted(names) and bmp.channel_names[:4] == ["R", "G", "B", "A"]
    for k, nm in enumerate(names):
        assert np.array_equal(bmp.data[..., bmp.channel_names.index(nm)], img[..., k]), nm
    assert np.array_equal(bmp.select("img"), img[..., 4:7])
