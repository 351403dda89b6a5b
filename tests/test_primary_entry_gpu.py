"""The per-pixel primary entry (scene_prep.cpp: build_primary_entry) lets a camera ray of the 64-byte-record volpath kernels
start its BVH traversal at the lowest node or leaf that holds every triangle a ray through its pixel can hit first, or skip it where there is
none.  The entry only leaves out nodes and triangles the ray cannot hit first, so the table may be visible in speed and in `n_primary_entry`
alone: every lane bit-identical with and without it (LRT_NO_PRIMARY_ENTRY, read when the scene is uploaded) and to the CPU oracle, the same
trips, shadow queries, records and proven records.

Liver-SingleMesh at 128 x 72 x 16 spp, both samplers: sixteen samples per pixel put four pixels, and so different entries, into one wave.
`n_primary_entry` counts the fresh lanes whose query did not start at the root: every lane is fresh once, so it is spp times the number of pixels
with a non-root item (read back with primary_entry()); 0 with the switch and with the 80-byte kernels, which do not read the table.
Further: a crop window, 1 spp, the folded prism of the cone test (lanes); two tile shards, which go through the pixel list, and sixteen passes
of one sample (films: the lanes' values are the same, so two films differ by the order of the float atomics alone: 16 non-negative terms per
pixel and channel, each order within 15 * 2^-24 of the exact sum relative to it)."""
import re

import numpy as np
import pytest

from test_closed_records_gpu import ld, liver
from test_cone_proof_gpu import folded_box_obj
from test_parity_gpu import assert_lanes_equal, bits

pytestmark = pytest.mark.gpu

COUNTS = ("n_iter", "n_shadow", "n_records", "n_proven")
SEED = 3


def with_and_without(mi, monkeypatch, make, run):
    """[(result of run(scene), stats, scene)] with the table, then without it"""
    out = []
    for table in (True, False):
        if table:
            monkeypatch.delenv("LRT_NO_PRIMARY_ENTRY", raising=False)
        else:
            monkeypatch.setenv("LRT_NO_PRIMARY_ENTRY", "1")
        sc = make()
        out.append((run(sc), sc.stats(), sc))
    monkeypatch.delenv("LRT_NO_PRIMARY_ENTRY", raising=False)
    return out


def all_lanes(sc):
    return sc.render_samples(0, int(np.prod(sc.film_shape()[:2])) * sc.spp, seed=SEED)


def assert_table_invisible(mi, orc, monkeypatch, xml_edit=None, closed=True, **kw):
    (a, sa, sc), (b, sb, sc_b) = with_and_without(mi, monkeypatch, lambda: liver(mi, xml_edit, **kw), all_lanes)
    tab = sc.primary_entry()
    print("table", {k: sa[k] for k in COUNTS + ("n_primary_entry", "record_bytes")}, "none", {k: sb[k] for k in COUNTS + ("n_primary_entry", "record_bytes")},
          "items: none %d, leaf %d, node %d, root %d" % ((tab == 0xffff).sum(), ((tab & 0x8000) != 0).sum() - (tab == 0xffff).sum(), ((tab & 0x8000) == 0).sum() - (tab == 0).sum(), (tab == 0).sum()))
    assert sa["record_bytes"] == sb["record_bytes"] == (64 if closed else 80) and sa["n_closed_guard"] == 0 and sb["n_closed_guard"] == 0
    same = (bits(a) == bits(b)).all(axis=1)
    assert same.all(), f"{(~same).sum()} of {len(a)} lanes differ with the table; first: lane {int(np.argmin(same))} table={a[np.argmin(same)]} none={b[np.argmin(same)]}"
    for k in COUNTS:
        assert sa[k] == sb[k], (k, sa, sb)
    o = orc.OrcScene(sc)
    c = o.render_samples(0, len(a), seed=SEED)
    same = (bits(a) == bits(c)).all(axis=1)
    assert same.all(), f"{(~same).sum()} of {len(a)} lanes differ from the oracle; first: lane {int(np.argmin(same))} gpu={a[np.argmin(same)]} cpu={c[np.argmin(same)]}"
    assert sa["n_iter"] == o.last_stats["n_iter"] and sa["n_shadow"] == o.last_stats["n_shadow_needed"]
    assert tab.any() and not sc_b.primary_entry().any() and sb["n_primary_entry"] == 0
    if closed:
        assert 0 < sa["n_primary_entry"] == sc.spp * int((tab != 0).sum()), (sa, int((tab != 0).sum()))
    else:
        assert sa["n_primary_entry"] == 0, sa
    return sa, tab


@pytest.mark.parametrize("sampler", ["independent", "ld"])
def test_liver_lanes_identical_and_the_entries_in_use(mi, orc, monkeypatch, sampler):
    sa, tab = assert_table_invisible(mi, orc, monkeypatch, ld if sampler == "ld" else None)
    assert tab.shape == (72, 128) and (tab == 0xffff).sum() > 0.3 * tab.size and ((tab & 0x8000) != 0).sum() > (tab == 0xffff).sum()      # background and single leaves


def test_wide_kernels_do_not_read_the_table(mi, orc, monkeypatch):
    monkeypatch.setenv("LRT_NO_CLOSED_RECORDS", "1")
    assert_table_invisible(mi, orc, monkeypatch, closed=False)


def crop(xml):
    out = xml.replace('<integer name="height" value="$res_height"/>', '<integer name="height" value="$res_height"/><integer name="crop_offset_x" value="37"/>'
                      '<integer name="crop_offset_y" value="5"/><integer name="crop_width" value="50"/><integer name="crop_height" value="33"/>')
    assert out != xml
    return out


def test_crop_window(mi, orc, monkeypatch):
    """a window whose offset is no multiple of anything, across the silhouette: the table is indexed by the crop-local pixel"""
    sa, tab = assert_table_invisible(mi, orc, monkeypatch, crop)
    assert tab.shape == (33, 50) and (tab == 0xffff).any() and (tab != 0xffff).any()


def test_one_sample_per_pixel(mi, orc, monkeypatch):
    """sixty-four pixels, and as many entries, in a wave"""
    assert_table_invisible(mi, orc, monkeypatch, spp=1)


def assert_films_equal_up_to_order(a, b):
    """16 non-negative terms per pixel and channel, summed by float atomics in two orders (the module's docstring)"""
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (b >= 0).all()
    err = np.abs(a.astype(np.float64) - b.astype(np.float64)); bound = 2 * 15 * 2.0 ** -24 * np.maximum(a, b).astype(np.float64)
    print("max |a - b| / bound = %.3g" % np.max(err / np.maximum(bound, 1e-300)))
    assert (err <= bound).all()


def test_two_tile_shards(mi, monkeypatch):
    """tile_rank / tile_count: the lanes come from the rank's pixel list"""
    def run(sc):
        films, stats = [], []
        for r in range(2):
            films.append(sc.render(return_raw=True, seed=SEED, tile_rank=r, tile_count=2)[1]); stats.append(sc.stats())
        return films, stats
    ((fa, sa), _, sc), ((fb, sb), _, _) = with_and_without(mi, monkeypatch, lambda: liver(mi), run)
    tab = sc.primary_entry()
    for r in range(2):
        assert fa[r].any()
        assert_films_equal_up_to_order(fa[r], fb[r])
        for k in COUNTS:
            assert sa[r][k] == sb[r][k], (r, k, sa[r], sb[r])
        assert sa[r]["n_primary_entry"] > 0 and sb[r]["n_primary_entry"] == 0
    assert sa[0]["n_primary_entry"] + sa[1]["n_primary_entry"] == sc.spp * int((tab != 0).sum())


def test_sixteen_passes_of_one_sample(mi, monkeypatch):
    def passes(xml):
        out = xml.replace('<integer name="max_depth" value="$max_depth"/>', '<integer name="max_depth" value="$max_depth"/><integer name="samples_per_pass" value="1"/>')
        assert out != xml
        return out
    def run(sc):
        return sc.render(return_raw=True, seed=SEED)[1]
    (fa, sa, sc), (fb, sb, _) = with_and_without(mi, monkeypatch, lambda: liver(mi, passes), run)
    assert sc.desc.samples_per_pass == 1 and sc.spp == 16
    assert_films_equal_up_to_order(fa, fb)
    for k in COUNTS:
        assert sa[k] == sb[k], (k, sa, sb)
    assert sa["n_primary_entry"] == 16 * int((sc.primary_entry() != 0).sum()) > 0 and sb["n_primary_entry"] == 0


def test_folded_prism_lanes_match_the_oracle(mi, orc, monkeypatch, tmp_path):
    """the cone test's prism: a concave fold, where a ray through one pixel can meet the floor, the folded wall or the back"""
    obj = str(tmp_path / "fold.obj")
    centre, n_faces = folded_box_obj(obj)
    centre = centre + np.array([-5.0, 5.0, -5.0])                                            # the scene file's to_world

    def edit(xml):
        out = xml.replace('value="liver2.obj"', 'value="%s"' % obj)
        eye = centre + np.array([6.0, -7.0, 5.0])
        out, n = re.subn(r"<lookat [^>]*/>", '<lookat up="0, 0, 1" target="%g, %g, %g" origin="%g, %g, %g"/>' % (*centre, *eye), out, flags=re.S)
        assert n == 1 and out != xml
        return out

    (a, sa, sc), (b, sb, _) = with_and_without(mi, monkeypatch, lambda: liver(mi, edit, res_width=64, res_height=64), all_lanes)
    tab = sc.primary_entry()
    assert sc.desc.n_faces == n_faces == 110 and sa["record_bytes"] == 64 and sb["record_bytes"] == 64 and sa["n_closed_guard"] == 0
    print("table", sa, "none", sb)
    assert (bits(a) == bits(b)).all()
    for k in COUNTS:
        assert sa[k] == sb[k], (k, sa, sb)
    assert 0 < sa["n_primary_entry"] == 16 * int((tab != 0).sum()) and sb["n_primary_entry"] == 0
    assert_lanes_equal(sc, orc.OrcScene(sc), 0, 64 * 64 * 16, seed=SEED)
