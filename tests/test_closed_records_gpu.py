"""64-byte path records (record_layout.h, RecordLayout::Closed; closed_records() in device.hip): volpath on a scene where only a path's last trip adds
radiance queues no radiance and no last-scatter pdf.  Liver-SingleMesh qualifies (one dielectric-bounded homogeneous medium, one envmap).
The layout must change nothing but speed: lanes bit-identical to the 80-byte layout (LRT_NO_CLOSED_RECORDS) and to the oracle, the same
trips, shadow rays and records, the film equal up to the order of the float atomics.  Scenes that do not qualify keep 80 / 88 B."""
import os

import numpy as np
import pytest

from conftest import LIVER_XML
from test_parity_gpu import assert_lanes_equal, bits, center_lane, film_close

pytestmark = pytest.mark.gpu

BASE = os.path.dirname(LIVER_XML)
SMALL = dict(integrator="volpath", spp=16, res_width=128, res_height=72)
N_SMALL = 128 * 72 * 16


def liver(mi, xml_edit=None, **kw):
    xml = open(LIVER_XML).read()
    if xml_edit:
        xml = xml_edit(xml)
    return mi.load_string(xml, base_dir=BASE, **{**SMALL, **kw})


def ld(xml):
    return xml.replace('<sampler type="independent">', '<sampler type="ldsampler">')


def run(sc, monkeypatch, closed, **kw):
    if closed:
        monkeypatch.delenv("LRT_NO_CLOSED_RECORDS", raising=False)
    else:
        monkeypatch.setenv("LRT_NO_CLOSED_RECORDS", "1")
    lanes = sc.render_samples(0, N_SMALL, **kw); st = sc.stats()
    img, raw = sc.render(return_raw=True, **kw); st_img = sc.stats()
    monkeypatch.delenv("LRT_NO_CLOSED_RECORDS", raising=False)
    return lanes, st, raw, st_img


def assert_same_render(sc, monkeypatch, **kw):
    a, sa, raw_a, sia = run(sc, monkeypatch, True, **kw)
    b, sb, raw_b, sib = run(sc, monkeypatch, False, **kw)
    assert sa["record_bytes"] == 64 and sia["record_bytes"] == 64, (sa, sia)
    assert sb["record_bytes"] == 80 and sib["record_bytes"] == 80, (sb, sib)
    assert sa["n_closed_guard"] == 0 and sia["n_closed_guard"] == 0
    assert (bits(a) == bits(b)).all()
    for x, y in ((sa, sb), (sia, sib)):
        assert x["n_iter"] == y["n_iter"] and x["n_shadow"] == y["n_shadow"] and x["n_records"] == y["n_records"]
    assert np.isfinite(raw_a).all() and film_close(raw_a, raw_b).all()
    return a


@pytest.mark.parametrize("sampler", ["independent", "ld"])
def test_liver_closed_records_match_compact_and_oracle(mi, orc, monkeypatch, sampler):
    sc = liver(mi, ld if sampler == "ld" else None)
    o = orc.OrcScene(sc)
    assert_same_render(sc, monkeypatch, seed=3)
    assert_lanes_equal(sc, o, 0, N_SMALL, seed=3)
    assert sc.stats()["record_bytes"] == 64
    for g, seed in ((0.7, 1), (-0.4, 2)):                      # HG phase function through param_set
        sc.param_set("LiverMedium.phase_function.g", g); o.param_set("LiverMedium.phase_function.g", g)
        assert_same_render(sc, monkeypatch, seed=seed)
        assert_lanes_equal(sc, o, 0, N_SMALL, seed=seed)
        assert sc.stats()["record_bytes"] == 64 and sc.stats()["n_closed_guard"] == 0


def test_closed_records_multi_pass_and_tile_sharded(mi, orc, monkeypatch):
    xml_pass = lambda x: x.replace('<integer name="max_depth" value="$max_depth"/>', '<integer name="max_depth" value="$max_depth"/><integer name="samples_per_pass" value="4"/>')
    sc = liver(mi, xml_pass)
    assert sc.desc.samples_per_pass == 4
    o = orc.OrcScene(sc)
    _, raw = sc.render(return_raw=True, seed=2); st = sc.stats()
    assert st["record_bytes"] == 64 and st["n_closed_guard"] == 0 and st["n_launches"] >= 4
    monkeypatch.setenv("LRT_NO_CLOSED_RECORDS", "1")
    _, raw_c = sc.render(return_raw=True, seed=2); st_c = sc.stats()
    monkeypatch.delenv("LRT_NO_CLOSED_RECORDS")
    assert st_c["record_bytes"] == 80
    assert st["n_iter"] == st_c["n_iter"] and st["n_shadow"] == st_c["n_shadow"] and st["n_records"] == st_c["n_records"]
    assert film_close(raw, raw_c).all()
    _, oraw = o.render(return_raw=True, seed=2)
    assert st["n_iter"] == o.last_stats["n_iter"] and st["n_shadow"] == o.last_stats["n_shadow_needed"]
    assert film_close(raw, oraw).all()
    # 2-way tile sharding of the plain scene: the ranks' films add up to the full film, with either layout
    sc = liver(mi)
    _, full = sc.render(return_raw=True, seed=4)
    parts = 0
    for r in range(2):
        parts = parts + sc.render(return_raw=True, seed=4, tile_rank=r, tile_count=2)[1]
        assert sc.stats()["record_bytes"] == 64 and sc.stats()["n_closed_guard"] == 0
    assert film_close(parts, full).all()
    monkeypatch.setenv("LRT_NO_CLOSED_RECORDS", "1")
    full_c = sc.render(return_raw=True, seed=4)[1]
    assert film_close(full_c, full).all()


def _het_edit(vol):
    def edit(x):
        smoke = ('<medium type="heterogeneous" id="smoke"><volume name="sigma_t" type="gridvolume"><string name="filename" value="%s"/>'
                 '<transform name="to_world"><scale value="0.5"/><translate x="-5.5" y="3.5" z="-5.5"/></transform></volume>'
                 '<rgb name="albedo" value="0.9, 0.8, 0.6"/><float name="scale" value="3"/></medium>' % vol)
        cube = ('<shape type="cube"><transform name="to_world"><scale value="0.25"/><translate x="-5.25" y="3.75" z="-5.25"/></transform>'
                '<ref id="ParenchymaBSDF"/><ref name="interior" id="smoke"/></shape>')
        return x.replace('<shape type="obj" id="liver2">', smoke + cube + '<shape type="obj" id="liver2">')
    return edit


DIFFUSE_FLOOR = ('<shape type="rectangle"><transform name="to_world"><scale value="4"/><rotate x="1" angle="-90"/><translate x="-5" y="2.5" z="-5"/></transform>'
                 '<ref id="FloorBSDF"/></shape>')
AREA_LIGHT = ('<shape type="rectangle"><transform name="to_world"><scale value="0.5"/><rotate x="1" angle="90"/><translate x="-5" y="8" z="-5"/></transform>'
              '<bsdf type="dielectric"/><emitter type="area"><rgb name="radiance" value="5, 5, 5"/></emitter></shape>')
POINT_LIGHT = '<emitter type="point"><point name="position" x="-3" y="8" z="-3"/><rgb name="intensity" value="20, 20, 20"/></emitter>'


@pytest.mark.parametrize("case", ["diffuse-shape", "area-emitter", "null-boundary", "heterogeneous", "path", "sigma-t-zero"])
def test_scenes_that_do_not_qualify_keep_their_layout(mi, orc, tmp_path, case):
    if case == "diffuse-shape":
        sc = liver(mi, lambda x: x.replace("</scene>", DIFFUSE_FLOOR + "</scene>")); want = 80
    elif case == "area-emitter":
        sc = liver(mi, lambda x: x.replace("</scene>", AREA_LIGHT + "</scene>")); want = 88
    elif case == "null-boundary":
        sc = liver(mi, lambda x: x.replace('<ref id="GlissonCapsuleBSDF"/>', '<bsdf type="null"/>')); want = 80
    elif case == "heterogeneous":
        vol = str(tmp_path / "smoke.vol")
        g = np.random.default_rng(5).random((8, 8, 8)).astype(np.float32)
        mi.write_volume_grid(vol, g)
        sc = liver(mi, _het_edit(vol)); want = 104
    elif case == "path":
        sc = liver(mi, integrator="path"); want = 80
    else:
        sc = liver(mi)
        sc.render_samples(0, 4096)
        assert sc.stats()["record_bytes"] == 64
        sig = sc.param_get("LiverMedium.sigma_t.value")
        sc.param_set("LiverMedium.sigma_t.value", [float(sig[0]), 0.0, float(sig[2])])
        want = 80
    o = orc.OrcScene(sc)
    lane0 = center_lane(sc, 16)
    if case == "sigma-t-zero":
        o.param_set("LiverMedium.sigma_t.value", sc.param_get("LiverMedium.sigma_t.value"))
        # (a zero channel: where the oracle's radiance is NaN the device returns 0, with either record layout; the other lanes, the trips and
        # the shadow rays agree)
        g = sc.render_samples(lane0, 1 << 14, seed=1); c = o.render_samples(lane0, 1 << 14, seed=1)
        fin = np.isfinite(c).all(axis=1)
        assert fin.mean() > 0.5 and (bits(g[fin]) == bits(c[fin])).all()
        assert sc.stats()["n_iter"] == o.last_stats["n_iter"] and sc.stats()["n_shadow"] == o.last_stats["n_shadow_needed"]
    else:
        assert_lanes_equal(sc, o, lane0, 1 << 14, seed=1)
    st = sc.stats()
    assert st["record_bytes"] == want and st["n_closed_guard"] == 0, (case, st)


def test_point_emitter_keeps_its_layout(mi, monkeypatch):
    """A point emitter is a second emitter (and an EXT scene): wide records.  The oracle has no point emitters: same lanes with the
    switch set or not."""
    sc = liver(mi, lambda x: x.replace("</scene>", POINT_LIGHT + "</scene>"))
    a = sc.render_samples(0, 1 << 14); st = sc.stats()
    assert st["record_bytes"] == 88 and st["n_closed_guard"] == 0
    monkeypatch.setenv("LRT_NO_CLOSED_RECORDS", "1")
    b = sc.render_samples(0, 1 << 14)
    assert (bits(a) == bits(b)).all() and np.isfinite(a).all()


def test_wide_records_switch_still_wins(mi, monkeypatch):
    sc = liver(mi)
    monkeypatch.setenv("LRT_WIDE_RECORDS", "1")
    sc.render_samples(0, 4096)
    assert sc.stats()["record_bytes"] == 88
