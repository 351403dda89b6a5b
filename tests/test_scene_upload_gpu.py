"""The device image end to end: what scene_prep.cpp prepares is what device.hip uploads, on both sides of the LDS-fit boundary
and through a parameter update."""
import numpy as np
import pytest

from conftest import LIVER_XML

pytestmark = pytest.mark.gpu

# K x K planar quad grids (2 K^2 triangles) on the two sides of the LDS-fit boundary, found on the host with
# `scene_prep_main grid-fit 40 75` (tests/host/scene_prep_main.cpp) at lds_limit = 160 KiB - 512:
# K = 57, 6498 faces: the image fits with 16-triangle leaves (161040 bytes); K = 58, 6728 faces: no leaf size fits.
FITS_K, FITS_FACES = 57, 6498
TOO_LARGE_K, TOO_LARGE_FACES = 58, 6728


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def quad_grid(k):
    """the grid of scene_prep_main.cpp's add_grid(2 k^2): vertices (x, y, 0) row by row, quad (a, b, e), (a, e, c)"""
    y, x = np.mgrid[0:k + 1, 0:k + 1]
    v = np.stack([x.ravel(), y.ravel(), np.zeros((k + 1) ** 2)], 1).astype(np.float32)
    a = (np.arange(k)[:, None] * (k + 1) + np.arange(k)[None, :]).ravel()
    b, c, e = a + 1, a + k + 1, a + k + 2
    f = np.stack([np.stack([a, b, e], 1), np.stack([a, e, c], 1)], 1).reshape(-1, 3).astype(np.uint32)
    return v, f


@pytest.mark.parametrize("k,faces,resident", [(FITS_K, FITS_FACES, 1), (TOO_LARGE_K, TOO_LARGE_FACES, 0)])
def test_lds_fit_boundary(mi, monkeypatch, k, faces, resident):
    v, f = quad_grid(k)
    assert f.shape[0] == faces
    rng = np.random.default_rng(5)                                     # 256 fixed rays from above the grid, most of them down into it
    o = np.concatenate([rng.uniform(-2, k + 2, (256, 2)), rng.uniform(0.5, 3, (256, 1))], 1).astype(np.float32)
    d = np.concatenate([rng.normal(0, 0.5, (256, 2)), -np.ones((256, 1))], 1); d[::16, 2] = 1.0
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    sc = mi.scene_from_buffers(v, f)
    got = sc.trace(o, d)
    sc.render_samples(0, 64)                                            # (the statistics are a render's)
    assert sc.stats()["lds_resident"] == resident
    monkeypatch.setenv("LRT_NO_LDS_BVH", "1")
    ref = mi.scene_from_buffers(v, f)
    want = ref.trace(o, d)
    ref.render_samples(0, 64)
    assert ref.stats()["lds_resident"] == 0
    hit = want[3] != 0xffffffff
    assert 0.5 < hit.mean() < 1.0
    for a, b in zip(got, want):                                        # (t, u, v, prim), bit for bit
        assert (bits(a) == bits(b)).all() if a.dtype == np.float32 else (a == b).all()


def test_parameter_update_equals_a_fresh_scene(mi):
    """device_scene_update_params and device_scene_create fill the media tables through the same prepare_media: a scene whose
    sigma_t changes after its device image exists renders what a scene does that had the value before its image was built."""
    key, value = "LiverMedium.sigma_t.value", [0.05, 0.08, 0.11]
    load = lambda: mi.load_file(LIVER_XML, integrator="volpath", spp=16, res_width=128, res_height=72)
    lane0 = 36 * 128 * 16 + 60 * 16                                    # the middle of the film: the liver
    a = load()
    before = a.render_samples(lane0, 64)                                # builds the device image with the file's sigma_t
    a.param_set(key, value)
    updated = a.render_samples(lane0, 64)
    b = load()
    b.param_set(key, value)                                             # no device image yet: the create sees the value
    fresh = b.render_samples(lane0, 64)
    assert (bits(updated) == bits(fresh)).all()
    assert (bits(updated) != bits(before)).any()                        # the update reached the device
