"""The `<medium>.sigma_t.data` parameter of a heterogeneous medium on the host side (lrt_param_set / lrt_param_get, mi.traverse), and
the float64 helper of the per-voxel gradient tests (grid_grad_ref.py) against itself.  No GPU."""
import os

import numpy as np
import pytest

import grid_grad_ref as gr
import scene_gen

SHAPE = (3, 2, 2)                       # (res_z, res_y, res_x): small and non-cubic, an index-order mistake shows


def _grid(seed, shape=SHAPE):
    return (0.2 + 0.7 * np.random.default_rng(seed).random(shape)).astype(np.float32)


def _load(mi, tmp_path, grid, name="g.vol", xml=None, w=16, h=12, spp=4):
    vol = os.path.join(str(tmp_path), name); mi.write_volume_grid(vol, grid)
    return mi.load_string(scene_gen.resized((xml or scene_gen.het_xml)(vol), w, h, spp))


def test_param_round_trip(mi, orc, tmp_path):
    g1, g2 = _grid(1), _grid(2)
    g2[2, 1, 0] = 1.25                                          # a new maximum: grid_max must follow
    sc = _load(mi, tmp_path, g1)
    assert np.array_equal(sc.param_get("smoke.sigma_t.data"), g1)
    sc.param_set("smoke.sigma_t.data", g2)
    got = sc.param_get("smoke.sigma_t.data")
    assert got.shape == SHAPE and got.dtype == np.float32 and np.array_equal(got, g2)
    m = sc.desc.media[0]
    assert m.grid_max == g2.max() == np.float32(1.25)
    assert np.array_equal(np.ctypeslib.as_array(m.grid_data, (g2.size,)), g2.reshape(-1))
    ref = _load(mi, tmp_path, g2, "g2.vol")
    a = orc.OrcScene(sc).render(integrator="volpath", seed=2)
    b = orc.OrcScene(ref).render(integrator="volpath", seed=2)
    assert a.shape == (12, 16, 3) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, orc.OrcScene(_load(mi, tmp_path, g1, "g1.vol")).render(integrator="volpath", seed=2))
    sc.param_set("smoke.sigma_t.data", g1.reshape(-1))          # the flattened array is the C layout (x fastest)
    assert np.array_equal(sc.param_get("smoke.sigma_t.data"), g1) and sc.desc.media[0].grid_max == g1.max()


@pytest.mark.parametrize("bad", ["length", "negative", "nan", "inf", "zero"])
def test_param_set_rejections(mi, tmp_path, bad):
    g1 = _grid(1)
    sc = _load(mi, tmp_path, g1)
    v = _grid(5)
    if bad == "length": v = v.reshape(-1)[:-1]
    elif bad == "negative": v[1, 0, 1] = -1e-3
    elif bad == "nan": v[0, 1, 0] = np.nan
    elif bad == "inf": v[2, 1, 1] = np.inf
    else: v[:] = 0.0
    L = mi._lib.lib()
    import ctypes as C
    flat = np.ascontiguousarray(v, np.float32).reshape(-1)
    assert L.lrt_param_set(sc._h, b"smoke.sigma_t.data", flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size) == mi._lib.INVALID
    assert L.lrt_last_error()
    assert np.array_equal(sc.param_get("smoke.sigma_t.data"), g1) and sc.desc.media[0].grid_max == g1.max()


def test_key_is_for_heterogeneous_media_only(mi, tmp_path):
    sc = _load(mi, tmp_path, _grid(1), xml=scene_gen.two_media_xml)
    assert sc.medium_ids() == ["smoke", "fog"] and sc.heterogeneous_media() == [0]
    L = mi._lib.lib()
    import ctypes as C
    v = np.ones(12, np.float32)
    assert L.lrt_param_set(sc._h, b"fog.sigma_t.data", v.ctypes.data_as(C.POINTER(C.c_float)), 12) == mi._lib.INVALID
    assert L.lrt_param_get(sc._h, b"fog.sigma_t.data", v.ctypes.data_as(C.POINTER(C.c_float)), 12) == mi._lib.INVALID
    with pytest.raises(RuntimeError, match="unknown parameter"):
        sc.param_set("fog.sigma_t.data", v)
    assert np.array_equal(sc.param_get("fog.sigma_t.value"), np.float32([0.9, 0.3, 1.6]))


def test_traverse_lists_the_grid(mi, tmp_path):
    g1, g2 = _grid(1), _grid(2)
    sc = _load(mi, tmp_path, g1, xml=scene_gen.two_media_xml)
    p = mi.traverse(sc)
    assert "smoke.sigma_t.data" in p and "fog.sigma_t.data" not in p
    assert p["smoke.sigma_t.data"].shape == SHAPE and np.array_equal(p["smoke.sigma_t.data"], g1)
    p["smoke.sigma_t.data"] = g2
    p.update()
    assert np.array_equal(sc.param_get("smoke.sigma_t.data"), g2)
    with pytest.raises(ValueError):
        p["smoke.sigma_t.data"] = np.ones(5, np.float32)


def test_exported_symbol_and_version(mi):
    L = mi._lib.lib()
    assert L.lrt_version() >= 112 and hasattr(L, "lrt_render_backward_grid") and "lrt_render_backward_grid" in mi._lib.EXPORTED_SYMBOLS


@pytest.mark.parametrize("shape", [SHAPE, (3, 2, 1), (4, 5, 6)])
def test_helper_against_itself(shape):
    rng = np.random.default_rng(7)
    grid = rng.random(shape)
    p = rng.random((500, 3)) * 1.2 - 0.1                        # some points outside the unit cube: clamped lookups
    p[:8] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [0.25, 0.75, 1 / 6], [0.999, 0.001, 0.5], [0, 1, 0], [0.75, 0.25, 0.5], [1, 0, 1]]
    idx, wgt = gr.corners(p, shape)
    assert idx.min() >= 0 and idx.max() < grid.size and wgt.min() >= 0
    assert np.abs(wgt.sum(-1) - 1).max() < 1e-14
    W = gr.weights(p, shape)
    assert np.abs(W.sum(-1) - 1).max() < 1e-14
    assert np.abs(W @ grid.reshape(-1) - gr.trilinear(grid, p)).max() < 1e-14
    if shape[2] == 1:                                           # both x corners clamp onto the one voxel
        assert (idx[:, 0] == idx[:, 1]).all()
    # line integrals: the weights integrate to the segment length, and a constant grid integrates to length * value
    o = np.float64([0.2, -0.1, -2.0]); d = rng.normal(size=(20, 3)) * 0.1 + [0, 0, 1]; d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t0, t1 = np.full(20, 1.0), np.full(20, 3.0)
    LW = gr.line_weights(o, d, t0, t1, gr.cube_to_local(), shape, n=64)
    assert np.abs(LW.sum(-1) - 2.0).max() < 1e-12
