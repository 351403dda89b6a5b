"""Environment-map importance sampling on the device against float64 mathematics (envmap_ref.py): the checks of
tests/test_envmap.py (envmap_cases.py) on what Scene.emitter_probe and Scene.envmap_probe return, the device bit for bit against
the oracle's hooks on every map, and the exact NEE early rejection under a map with zeros."""
import numpy as np
import pytest

import envmap_cases as ec

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def cases(mi, orc, tmp_path_factory):
    """name -> (scene, float64 reference, oracle scene, the device's probe of the round-trip samples), made once per map"""
    tmp = tmp_path_factory.mktemp("envmaps"); smp = ec.round_trip_samples(); cache = {}
    def get(name):
        if name not in cache:
            sc, ref = ec.load(mi, tmp, name)
            cache[name] = (sc, ref, orc.OrcScene(sc), sc.emitter_probe(np.zeros((len(smp), 3), np.float32), smp))
        return cache[name]
    get.samples = smp
    return get


@pytest.mark.parametrize("name", ec.MAPS)
def test_probe_equals_the_oracle_bit_for_bit(cases, name):
    """h: direction, pdf and weight of every sample, pdf_emitter_direction and emitter_eval at every sampled direction (hit_pdf,
    hit_le), and pdf / eval at the chosen directions of check e"""
    sc, ref, o, pr = cases(name)
    want = ec.orc_sample(o, cases.samples)
    for k in ("d", "pdf", "weight"):
        same = same_bits(pr[k], want[k])
        assert same.all(), (name, k, int((~same).sum()), cases.samples[np.argmin(same.reshape(len(same), -1).all(1))])
    assert (pr["hit_shape"] == -1).all() and (pr["emitter"] == 0).all()
    live = pr["pdf"] > 0                                          # (the probe sends no ray for a sample of pdf 0)
    hpdf, hle = ec.orc_dirs(o, pr["d"][live])
    assert same_bits(pr["hit_pdf"][live], hpdf).all() and same_bits(pr["hit_le"][live], hle).all(), name
    assert (pr["hit_pdf"][~live] == 0).all() and (pr["hit_le"][~live] == 0).all()
    d = ec.chosen_directions(ref)
    pdf, rgb = sc.envmap_probe(d)
    opdf, orgb = ec.orc_dirs(o, d)
    assert same_bits(pdf, opdf).all() and same_bits(rgb, orgb).all(), name


@pytest.mark.parametrize("name", ec.MAPS)
def test_round_trip(cases, name):
    sc, ref, o, pr = cases(name)
    ec.check_round_trip(ref, pr, cases.samples, "device " + name)


@pytest.mark.parametrize("name", ec.MAPS)
def test_pdf_is_the_density_and_weights_are_radiance(cases, name):
    sc, ref, o, pr = cases(name)
    ec.check_pdf_and_weight(ref, pr, "device " + name)


@pytest.mark.parametrize("name", ec.MAPS)
def test_chi_square(cases, name):
    sc, ref, o, pr = cases(name)
    smp = ec.chi2_samples()
    ec.check_chi2(ref, sc.emitter_probe(np.zeros((len(smp), 3), np.float32), smp)["d"], "device " + name)


def test_one_texel_known_answer(cases):
    sc, ref, o, pr = cases("one_texel_10x100")
    live = pr["pdf"] > 0
    w = pr["weight"][live, 0]
    assert live.mean() > 0.99 and (w > 0.018).all() and (w < 0.02).all(), (w.min(), w.max())
    assert (pr["weight"][~live] == 0).all()


@pytest.mark.parametrize("name", [m for m in ec.MAPS if m != "cavidade"])
def test_eval_and_pdf_at_chosen_directions(cases, name):
    sc, ref, o, _ = cases(name)
    d = ec.chosen_directions(ref)
    pdf, rgb = sc.envmap_probe(d)
    ec.check_directions(ref, d, pdf, rgb, "device " + name)


def test_envmap_probe_needs_an_environment(mi):
    with pytest.raises(RuntimeError, match="no environment emitter"):
        mi.load_dict(mi.cornell_box()).envmap_probe(np.float32([[0, 1, 0]]))


def test_two_emitters(mi, orc, tmp_path):
    sc, ref = ec.load_two_emitters(mi, tmp_path)
    smp = ec.round_trip_samples()
    smp = smp[smp[:, 0] >= 0.5]
    pr = sc.emitter_probe(np.zeros((len(smp), 3), np.float32), smp)
    assert (pr["emitter"] == 1).all()
    want = ec.orc_sample(orc.OrcScene(sc), smp)
    for k in ("d", "pdf", "weight"):
        assert same_bits(pr[k], want[k]).all(), k
    miss = pr["hit_shape"] == -1                              # (a ray that meets the small rectangle evaluates that emitter)
    assert miss.mean() > 0.999
    pr = {k: v[miss] for k, v in pr.items()}; smp = smp[miss]
    ec.check_round_trip(ref, pr, smp, "device two emitters", sx_scale=2.0, sx_offset=1.0)
    ec.check_pdf_and_weight(ref, pr, "device two emitters", pmf=0.5)
    pdf, rgb = sc.envmap_probe(pr["d"][:1000])
    assert same_bits(pdf, pr["hit_pdf"][:1000]).all() and same_bits(rgb, pr["hit_le"][:1000]).all()


@pytest.mark.parametrize("name", ["zeros_16x9", "rand_17x9"])
def test_early_rejection_is_invisible(mi, orc, tmp_path, monkeypatch, name):
    """g: a medium in a dielectric cube under a map with zero texels (the rejection switches itself off) and under a positive one
    (it is active): lanes bit-identical to the oracle, and with and without LRT_NO_NEE_REJECT.
    Whether the rejection is on is not observed: no statistic counts rejected samples, n_shadow counts what the reference's loop
    needs in either state, and the render kernels are not this test's to change.  What is held is that no lane moves under either
    map in either state; a rejection wrongly left on under the zeros map would show only in a lane whose emitter sample lands
    where the density is zero."""
    n = 32 * 32 * 16
    sc = ec.load_cube(mi, tmp_path, name)
    g = sc.render_samples(0, n)
    o = orc.OrcScene(sc)
    c = o.render_samples(0, n)
    assert (bits(g) == bits(c)).all(), int((bits(g) != bits(c)).any(1).sum())
    assert np.isfinite(g).all() and (g[:, :3] > 0).any()
    assert o.last_stats["n_shadow"] > n                          # most lanes take the NEE branch, more than once
    assert sc.stats()["n_shadow"] == o.last_stats["n_shadow_needed"]
    monkeypatch.setenv("LRT_NO_NEE_REJECT", "1")
    off = ec.load_cube(mi, tmp_path, name)
    assert (bits(off.render_samples(0, n)) == bits(g)).all()
