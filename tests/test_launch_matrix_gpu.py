"""Every way device.hip picks a forward render kernel, on the smallest scene the suite has for each kernel mode: path (Cornell box: area
emitter, wide records; Liver-SingleMesh: compact), volpath (Liver-SingleMesh: 64-byte closed records), biovolpath / biovolpath06,
volpath through a grid volume (VOLPATH_HET), volpathmis with and without spectral MIS, and a sphere scene for the EXT instances; each with
the independent and the ld sampler, under each launch switch: none, LRT_NO_LDS_BVH (BVH in global memory), LRT_WIDE_RECORDS,
LRT_NO_CLOSED_RECORDS.  A switch changes the kernel instance and the record layout and nothing else: the lanes of all variants are bit-identical
to one another and, where the oracle renders the scene, to the oracle with its trip and shadow-ray counts; the queued records are the same
wherever the BVH lives in the same place; lrt_render_stats.record_bytes is the layout's size, written out per cell below.

LRT_NO_LDS_BVH is read when the device image of a scene is built: every variant loads a fresh scene."""
import os

import numpy as np
import pytest

import scene_gen
from conftest import LIVER_XML
from test_parity_gpu import bits
from test_sphere_gpu import FLOOR, SPHERES, scene_xml, sphere_xml

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 4                      # spp: a square power of two, so that both samplers take it
N = W * H * SPP
VARIANTS = {"default": None, "no-lds-bvh": "LRT_NO_LDS_BVH", "wide-records": "LRT_WIDE_RECORDS", "no-closed-records": "LRT_NO_CLOSED_RECORDS"}
SWITCHES = [v for v in VARIANTS.values() if v]


def _same(b):
    return {v: b for v in VARIANTS}


# cell -> (oracle renders it, record_bytes per variant)
CELLS = {
    "path-cornell":       (True, _same(88)),                                                                         # area emitter: wide
    "path-liver":         (True, {"default": 80, "no-lds-bvh": 88, "wide-records": 88, "no-closed-records": 80}),
    "volpath-liver":      (True, {"default": 64, "no-lds-bvh": 88, "wide-records": 88, "no-closed-records": 80}),
    "biovolpath-liver":   (True, {"default": 88, "no-lds-bvh": 96, "wide-records": 96, "no-closed-records": 88}),
    "biovolpath06-liver": (True, {"default": 88, "no-lds-bvh": 96, "wide-records": 96, "no-closed-records": 88}),
    "volpath-het":        (True, _same(104)),
    "volpathmis":         (True, _same(168)),
    "volpathmis-plain":   (True, _same(168)),
    "path-spheres":       (False, _same(88)),                                                                        # EXT: wide
    "volpath-spheres":    (False, _same(88)),
}


@pytest.fixture(scope="module")
def smoke_vol(mi, tmp_path_factory):
    vol = str(tmp_path_factory.mktemp("launch_matrix") / "smoke.vol")
    mi.write_volume_grid(vol, scene_gen.smoke_grid())
    return vol


def load(mi, cell, sampler, vol):
    ld = sampler == "ld"
    name = "ldsampler" if ld else "independent"
    if cell == "path-cornell":
        d = mi.cornell_box()
        d["integrator"]["type"] = "path"
        d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = W, H
        d["sensor"]["sampler"] = {"type": name, "sample_count": SPP}
        return mi.load_dict(d)
    if cell.endswith("-liver"):
        xml = open(LIVER_XML).read()
        if ld:
            xml = xml.replace('<sampler type="independent">', '<sampler type="ldsampler">')
        return mi.load_string(xml, base_dir=os.path.dirname(LIVER_XML), integrator=cell.split("-")[0], spp=SPP, res_width=W, res_height=H)
    if cell.endswith("-spheres"):
        shapes = "".join(sphere_xml(c, r) for c, r in SPHERES) + FLOOR
        return mi.load_string(scene_xml(shapes, integrator='<integrator type="%s"/>' % cell.split("-")[0], size=(W, H), spp=SPP, sampler=name))
    if cell == "volpath-het":
        xml = scene_gen.het_xml(vol, sampler=name)
    else:
        xml = scene_gen.two_media_xml(vol, sampler=name).replace(
            '<integrator type="volpath">', '<integrator type="volpathmis"><boolean name="use_spectral_mis" value="%s"/>' % ("true" if cell == "volpathmis" else "false"))
    return mi.load_string(scene_gen.resized(xml, W, H, SPP))


@pytest.mark.parametrize("sampler", ["independent", "ld"])
@pytest.mark.parametrize("cell", list(CELLS))
def test_launch_variants_render_the_same_lanes(mi, orc, monkeypatch, smoke_vol, cell, sampler):
    has_oracle, record_bytes = CELLS[cell]
    lanes, stats, ref = {}, {}, None
    for variant, switch in VARIANTS.items():
        for s in SWITCHES:
            monkeypatch.delenv(s, raising=False)
        if switch:
            monkeypatch.setenv(switch, "1")
        sc = load(mi, cell, sampler, smoke_vol)
        assert tuple(sc.film_shape()[:2]) == (H, W)
        lanes[variant] = sc.render_samples(0, N); stats[variant] = sc.stats()
        if variant == "default" and has_oracle:
            o = orc.OrcScene(sc)
            ref = (o.render_samples(0, N), dict(o.last_stats))
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    assert np.isfinite(lanes["default"]).all() and lanes["default"][:, :3].max() > 0
    for variant in VARIANTS:
        st = stats[variant]
        print(cell, sampler, variant, {k: st[k] for k in ("record_bytes", "lds_resident", "n_iter", "n_shadow", "n_records", "n_closed_guard")})
        assert (bits(lanes[variant]) == bits(lanes["default"])).all(), variant
        assert st["record_bytes"] == record_bytes[variant], (variant, st)
        assert st["lds_resident"] == (0 if variant == "no-lds-bvh" else 1) and st["n_closed_guard"] == 0, (variant, st)
        assert st["n_samples"] == N and st["n_iter"] == stats["default"]["n_iter"] and st["n_shadow"] == stats["default"]["n_shadow"], (variant, st)
        if variant != "no-lds-bvh":
            assert st["n_records"] == stats["default"]["n_records"], (variant, st)
        if ref:
            assert (bits(lanes[variant]) == bits(ref[0])).all(), variant
            assert st["n_iter"] == ref[1]["n_iter"] and st["n_shadow"] == ref[1]["n_shadow_needed"], (variant, st, ref[1])
