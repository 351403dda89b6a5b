"""bench.py --dump-outputs without a GPU: the writer of the timed path's outputs (dtypes, the 64 MB bound, the seeded pixel sample)."""
import os

import numpy as np

import bench


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_small_outputs_are_written_whole(tmp_path):
    h, w = 6, 8
    rng = np.random.default_rng(1)
    img = rng.random((h, w, 3), dtype=np.float32); film = rng.random((h, w, 4), dtype=np.float32)
    shapes = bench.dump_outputs(str(tmp_path), {"image": img, "film": film, "grad_g": 0.25, "grad_albedo": np.ones(3, np.float32)}, h, w)
    got = _files(tmp_path)
    assert set(got) == {"image", "film", "grad_g", "grad_albedo"} and shapes["image"] == (h, w, 3)
    assert np.array_equal(got["image"], img) and np.array_equal(got["film"], film)
    assert got["image"].dtype == np.float32 and got["grad_albedo"].dtype == np.float32 and got["grad_g"].dtype == np.float64
    assert got["grad_g"].shape == () and got["grad_g"] == 0.25


def test_large_outputs_are_a_fixed_pixel_sample_within_64mb(tmp_path):
    h, w = 1080, 1920                                          # image + film with alpha: 74 MB, over the bound
    img = np.arange(h * w * 4, dtype=np.float32).reshape(h, w, 4)
    film = -np.arange(h * w * 5, dtype=np.float32).reshape(h, w, 5)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), {"image": img, "film": film}, h, w)
    bench.dump_outputs(str(b), {"image": img, "film": film}, h, w)
    size = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert size <= 64 * 1000 * 1000
    ga, gb = _files(a), _files(b)
    assert set(ga) == {"image", "film", "pixel_index"} and all(x.dtype in (np.float32, np.float64) for x in ga.values())
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k                 # same arguments, same elements
    idx = ga["pixel_index"].astype(np.int64)
    assert np.array_equal(ga["pixel_index"], idx) and np.all(np.diff(idx) > 0) and idx[-1] < h * w
    assert len(idx) > h * w // 2                               # the bound is used, not a token sample
    assert np.array_equal(ga["image"], img.reshape(h * w, 4)[idx]) and np.array_equal(ga["film"], film.reshape(h * w, 5)[idx])
