"""One Scene object whose path-record workspace (device.hip, ensure_workspace; the stream table of record_layout.h) is regrown and re-laid-out
between renders: a 64-lane volpath render allocates the smallest pool, the 20 736-lane renders after it regrow the streams (pool_geometry raises
the paths per workgroup above 64 once the lanes exceed 64 x the workgroup count, 256 with the LDS BVH), volpathmis adds the hit and w streams and
later finds them again, prbvolpath through render_samples (the deterministic primal PRB pass) brings in the delta_L streams.  Every result equals,
bit for bit, the same call on a scene freshly loaded from the same XML, with the same trips, shadow rays, records and record bytes.

No render_backward here: its double-precision sums are not bit-reproducible, and it adds no layout."""
import pytest

import scene_gen
from test_parity_gpu import bits

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 54, 4
N = W * H * SPP                            # 20 736 lanes
SEQUENCE = [(64, "volpath")] + [(N, i) for i in ("volpath", "volpathmis", "volpath", "path", "prbvolpath", "volpathmis")]
STATS = ("n_iter", "n_shadow", "n_records", "record_bytes")


def test_one_scene_through_every_workspace_layout(mi, tmp_path):
    vol = str(tmp_path / "smoke.vol")
    mi.write_volume_grid(vol, scene_gen.smoke_grid())
    xml = scene_gen.resized(scene_gen.two_media_xml(vol, sampler="independent"), W, H, SPP)
    scene = mi.load_string(xml)
    assert tuple(scene.film_shape()[:2]) == (H, W)
    for step, (n, integrator) in enumerate(SEQUENCE):
        got, got_stats = scene.render_samples(0, n, integrator=integrator), scene.stats()
        fresh = mi.load_string(xml)
        ref, ref_stats = fresh.render_samples(0, n, integrator=integrator), fresh.stats()
        print(step, n, integrator, {k: got_stats[k] for k in STATS}, {k: ref_stats[k] for k in STATS})
        assert ref[:, :3].max() > 0, (step, integrator)
        assert (bits(got) == bits(ref)).all(), (step, n, integrator, int((bits(got) != bits(ref)).any(axis=1).sum()))
        assert {k: got_stats[k] for k in STATS} == {k: ref_stats[k] for k in STATS}, (step, n, integrator)
