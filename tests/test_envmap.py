"""Environment-map importance sampling against float64 mathematics (envmap_ref.py), on the CPU through the oracle's hooks
orc.envmap_sample / envmap_pdf / envmap_eval.  tests/test_envmap_gpu.py runs the same checks (envmap_cases.py) on the device and
holds the device bit for bit to the oracle.  DESIGN.md, "Envmap sampling against float64", has the formulas and the measured margins.

The maps are written at test time with the project's EXR writer: the loader's smallest map, the reference's own three
(src/emitters/tests/test_envmap.py), odd sizes that leave a padded cell on every level of the hierarchy, zeros, a rotation."""
import numpy as np
import pytest

import envmap_cases as ec
import envmap_ref as er


@pytest.fixture(scope="module")
def cases(mi, orc, tmp_path_factory):
    """name -> (scene, float64 reference, oracle scene, the oracle's probe of the round-trip samples), made once per map"""
    tmp = tmp_path_factory.mktemp("envmaps"); smp = ec.round_trip_samples(); cache = {}
    def get(name):
        if name not in cache:
            sc, ref = ec.load(mi, tmp, name)
            o = orc.OrcScene(sc)
            cache[name] = (sc, ref, o, ec.orc_probe(o, smp))
        return cache[name]
    get.samples = smp
    return get


# ------------------------------------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("name", ["rand_5x3", "zeros_16x9", "rand_33x31"])
def test_reference_is_consistent(cases, name):
    """The density integrates to 1 and its box integrals match a midpoint rule; the inverse warp is a bijection of the unit square
    whose Jacobian determinant is the density (so a uniform sample pushed through the warp has that density); radiance and
    density agree with the definition at the nodes."""
    ref = cases(name)[1]
    m = ref.box_masses(np.linspace(0, 1, 8), np.linspace(0, 1, 6))
    assert abs(m.sum() - 1) < 1e-12 and (m >= 0).all()
    n = 400
    uu, vv = (np.arange(7 * n) + 0.5) / (7 * n), (np.arange(5 * n) + 0.5) / (5 * n)
    quad = ref.density(uu[None, :], vv[:, None]).reshape(5, n, 7, n).mean((1, 3)) / 35
    assert np.abs(quad - m).max() < 2e-5 * m.max()
    rng = np.random.default_rng(1)
    i, j = rng.integers(0, ref.w, 2000), rng.integers(0, ref.h - 1, 2000)
    a, b = rng.uniform(0.05, 0.95, 2000), rng.uniform(0.05, 0.95, 2000)
    live = ref.P[j, i] > 0
    i, j, a, b = i[live], j[live], a[live], b[live]
    e = 1e-6
    sx0, sy0, qx, qy = ref.invert_patch(i, j, a, b)
    assert np.allclose(qx * qy, ref.P[j, i], rtol=1e-12)
    sxa, sya = ref.invert_patch(i, j, a + e, b)[:2]; sxb, syb = ref.invert_patch(i, j, a, b + e)[:2]
    det = ((sxa - sx0) * (syb - sy0) - (sxb - sx0) * (sya - sy0)) / e ** 2 * ref.w * (ref.h - 1)
    assert np.allclose(det, ref.density((i + a) / ref.w, (j + b) / (ref.h - 1)), rtol=1e-4)
    assert (sx0 >= 0).all() and (sx0 <= 1).all() and (sy0 >= 0).all() and (sy0 <= 1).all()
    # corners of the square map to corners of the square
    assert np.allclose(ref.invert_patch(np.array([0]), np.array([0]), np.array([0.0]), np.array([1e-9]))[:2], [[0], [0]], atol=1e-6) or ref.P[0, 0] == 0
    # nodes: direction of node (x, y) -> that texel's radiance, its luminance * sin(theta) / normalisation
    y, x = 1 + np.arange(ref.h - 2), np.arange(ref.h - 2) % ref.w
    d = ref.uv_to_dir(x / ref.w, y / (ref.h - 1))
    assert np.allclose(ref.radiance(d), ref.rgb[y, x] * ref.scale, rtol=1e-9, atol=1e-12)
    u, v, st = ref.dir_to_uv(d)
    assert np.allclose(st, np.sin(np.pi * y / (ref.h - 1)))
    assert np.allclose(ref.pdf(d) * 2 * np.pi ** 2 * st, ref.D[y, x], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ a, b, d, c
@pytest.mark.parametrize("name", ec.MAPS)
def test_round_trip(cases, name):
    """a: the float64 inverse warp at the returned direction is the input sample, within the derived float32 bound"""
    sc, ref, o, pr = cases(name)
    for k in (0, 1, len(pr["pdf"]) - 1):                            # (orc.envmap_sample one at a time gives what the batched call gives)
        d, pdf, w = o.envmap_sample(float(cases.samples[k, 0]), float(cases.samples[k, 1]))
        assert (d == pr["d"][k]).all() and pdf == pr["pdf"][k] and (w == pr["weight"][k]).all()
    ec.check_round_trip(ref, pr, cases.samples, "oracle " + name)


@pytest.mark.parametrize("name", ec.MAPS)
def test_pdf_is_the_density_and_weights_are_radiance(cases, name):
    """b, d: pdf = float64 density = pdf_direction at the sampled direction; weight * pdf = float64 radiance = eval there"""
    sc, ref, o, pr = cases(name)
    ec.check_pdf_and_weight(ref, pr, "oracle " + name)


@pytest.mark.parametrize("name", ec.MAPS)
def test_chi_square(cases, name):
    """c: 2^18 samples against the exact box integrals of the density"""
    sc, ref, o, pr = cases(name)
    ec.check_chi2(ref, ec.orc_sample(o, ec.chi2_samples())["d"], "oracle " + name)


def test_one_texel_known_answer(cases):
    """d: the reference's known answer (test_envmap.py: every sampling weight on the one-texel map lies in (0.018, 0.02)); the
    solid angle of the tent around the texel, 2 pi^2 sin(theta) / (w (h - 1)) at row 40 of 100, is 0.0190"""
    sc, ref, o, pr = cases("one_texel_10x100")
    live = pr["pdf"] > 0
    w = pr["weight"][live, 0]
    assert live.mean() > 0.99 and (w > 0.018).all() and (w < 0.02).all(), (w.min(), w.max())
    assert abs(2 * np.pi ** 2 * np.sin(np.pi * 40 / 99) / (10 * 99) - 0.0190) < 1e-4
    assert (pr["weight"][~live] == 0).all()


# -------------------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("name", [m for m in ec.MAPS if m != "cavidade"])
def test_eval_and_pdf_at_chosen_directions(cases, name):
    """e: orc.envmap_eval and orc.envmap_pdf on the axes, next to the poles, on and beside the seam, and at random directions"""
    sc, ref, o, _ = cases(name)
    d = ec.chosen_directions(ref)
    pdf, rgb = ec.orc_dirs(o, d)
    for k in (0, 7, len(d) - 1):                                    # (the hooks one at a time give what the batched calls give)
        assert pdf[k] == o.envmap_pdf(d[k]) and (rgb[k] == o.envmap_eval(d[k])).all()
    ec.check_directions(ref, d, pdf, rgb, "oracle " + name)


# -------------------------------------------------------------------------------------------------------------------- f
def test_two_emitters(mi, orc, tmp_path):
    """f: beside a rectangle light the envmap's pdf carries 1/2, its weight 2, and sx is re-stretched: the round trip of check a
    on the samples that pick the envmap"""
    sc, ref = ec.load_two_emitters(mi, tmp_path)
    o = orc.OrcScene(sc)
    smp = ec.round_trip_samples()
    smp = smp[smp[:, 0] >= 0.5]                                  # (the envmap is the scene's second emitter)
    pr = ec.orc_probe(o, smp)
    ec.check_round_trip(ref, pr, smp, "oracle two emitters", sx_scale=2.0, sx_offset=1.0)
    ec.check_pdf_and_weight(ref, pr, "oracle two emitters", pmf=0.5)
