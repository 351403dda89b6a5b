"""The box-filter film route of the 64-byte-record volpath kernels (film.h: count_born_wave, finish_paths_wave_closed; film_runs.h; DESIGN.md
section 6g).  W is counted once per sample where the sample is born, as an integer taken from ballots; alpha is counted with it when a path is
valid from birth and from the retiring lanes' ballot otherwise; RGB costs no scan and no atomic where it is zero.  None of that may show in a
film: W is the sample count bit for bit (small integers add exactly in float, in any grouping), alpha is a count too, and RGB is the same set
of non-negative terms per pixel and channel in another order.

The reference inside the build is LRT_NO_CLOSED_RECORDS=1 (read at render time): the 80-byte kernels, whose film route this change leaves
alone.  Liver-SingleMesh (its file asks for an rgba film: five film channels, alpha at 3, W last) at 128 x 72:
  - 16 spp, both samplers: four pixels per wave, several runs per tile.  W = 16.0 in every pixel; RGB against the oracle's film (film_close,
    the bound tests/test_closed_records_gpu.py holds films of this size to) and against the 80-byte film (the order of 16 additions, the bound
    of tests/test_primary_entry_gpu.py); the per-lane output, which does not pass through the film route, is bit-identical with either record
    layout; n_iter, n_shadow and n_records are the same with either layout, for the film and for the lanes; n_proven and n_primary_entry,
    which only the 64-byte kernels count, are the same whether the kernel writes a film or lanes.
  - sixteen passes of one sample: a pixel's film is a fixed sequence of additions, so RGB, alpha and W are bit-identical to the 80-byte film.
  - 3 and 48 spp (no powers of two: lane / spp is a division, and at 48 the runs straddle wave boundaries) through a 50 x 33 crop window at
    (37, 5), whose last fresh tile is partial.  The film a render returns is the crop window's, so "nothing outside it" is its shape.
  - two tile shards (the pixel-list route), an rgb film, hide_emitters (paths are born invalid: alpha from the retiring lanes), and an
    environment of radiance zero (no lane ever carries radiance: the film's RGB must be +0 as bits, not -0 and not "close")."""
import numpy as np
import pytest

from test_closed_records_gpu import ld, liver
from test_parity_gpu import bits, film_close
from test_primary_entry_gpu import crop

pytestmark = pytest.mark.gpu

SEED = 3
N = 128 * 72 * 16
COUNTS = ("n_iter", "n_shadow", "n_records")
CLOSED_COUNTS = ("n_proven", "n_primary_entry")


def both_layouts(monkeypatch, run):
    """(run() with the 64-byte kernels, run() with LRT_NO_CLOSED_RECORDS=1)"""
    monkeypatch.delenv("LRT_NO_CLOSED_RECORDS", raising=False)
    a = run()
    monkeypatch.setenv("LRT_NO_CLOSED_RECORDS", "1")
    b = run()
    monkeypatch.delenv("LRT_NO_CLOSED_RECORDS", raising=False)
    return a, b


def film_and_stats(sc, **kw):
    raw = sc.render(return_raw=True, seed=SEED, **kw)[1]
    return raw, sc.stats()


def assert_layouts(sa, sb):
    assert sa["record_bytes"] == 64 and sa["n_closed_guard"] == 0 and sb["record_bytes"] == 80, (sa, sb)
    for k in COUNTS:
        assert sa[k] == sb[k], (k, sa, sb)


def assert_w(raw, spp):
    w = raw[..., -1]
    assert (bits(w) == bits(np.float32(spp))).all(), ("W", spp, np.unique(w))


def assert_sums_equal_up_to_order(a, b, n):
    """n non-negative terms per pixel and channel added in two orders: each order is within (n - 1) * 2^-24 of the exact sum, relative to it"""
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (b >= 0).all()
    err = np.abs(a.astype(np.float64) - b.astype(np.float64)); bound = 2 * (n - 1) * 2.0 ** -24 * np.maximum(a, b).astype(np.float64)
    print("max |a - b| / bound = %.3g" % np.max(err / np.maximum(bound, 1e-300)))
    assert (err <= bound).all()


@pytest.mark.parametrize("sampler", ["independent", "ld"])
def test_sixteen_samples_counts_colour_lanes_and_counters(mi, orc, monkeypatch, sampler):
    sc = liver(mi, ld if sampler == "ld" else None)
    (fa, sa), (fb, sb) = both_layouts(monkeypatch, lambda: film_and_stats(sc))
    print("film", {k: sa[k] for k in COUNTS + CLOSED_COUNTS}, "80-byte", {k: sb[k] for k in COUNTS + CLOSED_COUNTS})
    assert fa.shape == (72, 128, 5)
    assert_layouts(sa, sb)
    assert_w(fa, 16); assert_w(fb, 16)
    assert (bits(fa[..., 3]) == bits(fb[..., 3])).all() and (fa[..., 3] == 16.0).all()                  # (envmap, emitters not hidden: every sample is valid)
    assert fa[..., :3].max() > 0
    assert_sums_equal_up_to_order(fa[..., :3], fb[..., :3], 16)
    oraw = orc.OrcScene(sc).render(return_raw=True, seed=SEED)[1]
    assert film_close(fa, oraw).all()
    (la, sla), (lb, slb) = both_layouts(monkeypatch, lambda: (sc.render_samples(0, N, seed=SEED), sc.stats()))
    assert_layouts(sla, slb)
    same = (bits(la) == bits(lb)).all(axis=1)
    assert same.all(), f"{(~same).sum()} of {N} lanes differ; first: lane {int(np.argmin(same))} 64-byte={la[np.argmin(same)]} 80-byte={lb[np.argmin(same)]}"
    for k in COUNTS + CLOSED_COUNTS:
        assert sa[k] == sla[k], (k, sa, sla)
    assert sa["n_proven"] > 0 and sa["n_primary_entry"] > 0 and sb["n_proven"] == 0


def test_sixteen_passes_of_one_sample_are_bit_identical(mi, monkeypatch):
    def passes(xml):
        out = xml.replace('<integer name="max_depth" value="$max_depth"/>', '<integer name="max_depth" value="$max_depth"/><integer name="samples_per_pass" value="1"/>')
        assert out != xml
        return out
    sc = liver(mi, passes)
    assert sc.desc.samples_per_pass == 1 and sc.spp == 16
    (fa, sa), (fb, sb) = both_layouts(monkeypatch, lambda: film_and_stats(sc))
    assert_layouts(sa, sb)
    assert_w(fa, 16)
    assert fa[..., :3].max() > 0 and (bits(fa) == bits(fb)).all(), int((bits(fa) != bits(fb)).sum())


@pytest.mark.parametrize("spp", [3, 48])
def test_crop_window_and_sample_counts_that_are_no_power_of_two(mi, monkeypatch, spp):
    sc = liver(mi, crop, spp=spp)
    (fa, sa), (fb, sb) = both_layouts(monkeypatch, lambda: film_and_stats(sc))
    assert fa.shape == (33, 50, 5) and (50 * 33 * spp) % 64 != 0
    assert_layouts(sa, sb)
    assert_w(fa, spp); assert_w(fb, spp)
    assert (bits(fa[..., 3]) == bits(fb[..., 3])).all()
    assert fa[..., :3].max() > 0
    assert_sums_equal_up_to_order(fa[..., :3], fb[..., :3], spp)


def test_two_tile_shards(mi, monkeypatch):
    sc = liver(mi)
    full, _ = film_and_stats(sc)
    parts = 0
    for r in range(2):
        f, st = film_and_stats(sc, tile_rank=r, tile_count=2)
        assert st["record_bytes"] == 64 and st["n_closed_guard"] == 0 and f.any()
        assert np.isin(f[..., -1], (0.0, 16.0)).all()                      # a pixel belongs to one shard
        parts = parts + f
    assert_w(parts, 16)
    assert (parts[..., 3] == 16.0).all()
    assert film_close(parts, full).all()


def rgb(xml):
    out = xml.replace('<string name="pixel_format" value="rgba"/>', '<string name="pixel_format" value="rgb"/>')
    assert out != xml
    return out


@pytest.mark.parametrize("case", ["rgba", "rgba-hide-emitters", "rgb"])
def test_alpha_and_film_formats(mi, monkeypatch, case):
    sc = liver(mi, rgb if case == "rgb" else None)
    kw = dict(hide_emitters=True) if case == "rgba-hide-emitters" else {}
    (fa, sa), (fb, sb) = both_layouts(monkeypatch, lambda: film_and_stats(sc, **kw))
    assert_layouts(sa, sb)
    assert fa.shape == (72, 128, 4 if case == "rgb" else 5)
    assert_w(fa, 16); assert_w(fb, 16)
    assert_sums_equal_up_to_order(fa[..., :3], fb[..., :3], 16)
    if case != "rgb":
        alpha = fa[..., 3]
        print("alpha values", np.unique(alpha)[:20])
        assert (bits(alpha) == bits(fb[..., 3])).all(), int((bits(alpha) != bits(fb[..., 3])).sum())
        if case == "rgba":
            assert (alpha == 16.0).all()
        else:
            assert (alpha < 16.0).any() and (alpha > 0.0).any()              # hidden background, visible liver


def test_an_environment_of_radiance_zero_leaves_rgb_at_plus_zero(mi, monkeypatch):
    def dark(xml):
        a, b = xml.index('<emitter type="envmap">'), xml.index("</emitter>") + len("</emitter>")
        return xml[:a] + '<emitter type="constant"><rgb name="radiance" value="0, 0, 0"/></emitter>' + xml[b:]
    sc = liver(mi, dark)
    (fa, sa), (fb, sb) = both_layouts(monkeypatch, lambda: film_and_stats(sc))
    assert_layouts(sa, sb)
    assert (bits(fa[..., :3]) == 0).all(), np.unique(bits(fa[..., :3]))
    assert_w(fa, 16)
    assert (bits(fa[..., 3]) == bits(fb[..., 3])).all()
