"""Heterogeneous media on the device: lrt_medium_probe against the float64 reference of tests/medium_ref.py with the
bounds of test_medium.py and bit for bit against the oracle's probe; the pure-absorber and emitter-march scenes of test_medium.py rendered
on the device with the same seeds, sizes and assertions, and film against film with the oracle."""
import ctypes as C

import numpy as np
import pytest

import medium_cases as mc
import test_medium as tm
from test_medium import probe_scenes                                       # noqa: F401  (the module-scoped fixture)
from test_parity_gpu import film_close

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(mc.VOLUMES) + ["f"])
def test_probe_matches_float64_and_the_oracle(mi, orc, probe_scenes, name):        # noqa: F811
    sc = probe_scenes[name]; o = orc.OrcScene(sc)
    inp = tm.all_inputs()[name]
    got = sc.medium_probe(0, *tm.probe_inputs(inp))
    tm.check_probe(name, got, inp, None if name == "f" else tm.desc_frame(sc), "device")
    want = o.medium_probe(0, *tm.probe_inputs(inp))
    same = (bits(got["raw"]) == bits(want["raw"])) | (np.isnan(got["raw"]) & np.isnan(want["raw"]))      # a NaN is a NaN: payloads are not compared
    kinds = np.array(inp[5])
    print(f"device {name}: {len(kinds)} lanes against the oracle, {int((~same.all(1)).sum())} differ; "
          f"face lanes {int((kinds == 'face').sum())}, NaN lanes {int((kinds == 'nan').sum())}, NaN payload bits equal: {bool((bits(got['raw']) == bits(want['raw'])).all())}")
    assert same.all(), (name, np.flatnonzero(~same.all(1))[:8], kinds[~same.all(1)][:8])
    assert np.isnan(got["raw"][kinds == "nan"]).any()
    if name != "f":
        g = tm.check_lookups(name, lambda *a: sc.medium_probe(0, *a), "device")
        w = o.medium_probe(0, g["local"], np.zeros_like(g["local"]), np.full(len(g["grid"]), np.nan, np.float32), np.zeros(len(g["grid"]), np.float32), np.zeros(len(g["grid"]), np.uint32))
        assert (bits(g["raw"]) == bits(w["raw"])).all()


def test_probe_refuses_bad_arguments(mi, probe_scenes):                            # noqa: F811
    sc = probe_scenes["b"]; L = mi._lib.lib()
    FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    f3 = np.zeros((2, 3), np.float32); f1 = np.zeros(2, np.float32); u1 = np.zeros(2, np.uint32)
    out = np.zeros((2, mi._lib.MEDIUM_PROBE_FLOATS), np.float32)
    good = [f3.ctypes.data_as(FP), f3.ctypes.data_as(FP), f1.ctypes.data_as(FP), f1.ctypes.data_as(FP), u1.ctypes.data_as(UP)]
    assert L.lrt_medium_probe(sc._h, 0, *good, 2, out.ctypes.data_as(FP), 0) == mi._lib.OK
    for medium in (-1, 1, 1 << 20):
        assert L.lrt_medium_probe(sc._h, medium, *good, 2, out.ctypes.data_as(FP), 0) == mi._lib.INVALID
    for k in range(5):
        args = list(good); args[k] = None
        assert L.lrt_medium_probe(sc._h, 0, *args, 2, out.ctypes.data_as(FP), 0) == mi._lib.INVALID
    assert L.lrt_medium_probe(sc._h, 0, *good, 2, None, 0) == mi._lib.INVALID
    assert L.lrt_medium_probe(None, 0, *good, 2, out.ctypes.data_as(FP), 0) == mi._lib.INVALID
    assert L.lrt_medium_probe(sc._h, 0, *good, 0, out.ctypes.data_as(FP), 0) == mi._lib.OK          # nothing to do
    with pytest.raises(ValueError):
        sc.medium_probe(0, f3, f3, f1, f1[:1], u1)


def render_pair(sc, o, spp):
    """Device and oracle films over the fixed seeds: the device's statistics, and film_close on every seed"""
    dev, ora = [], []
    for s in tm.SEEDS:
        img, raw = sc.render(spp=spp, seed=s, return_raw=True)
        oimg, oraw = o.render(spp=spp, seed=s, return_raw=True)
        assert film_close(raw, oraw).all(), s
        dev.append(np.asarray(img, np.float64)[..., :3].mean(-1)); ora.append(np.asarray(oimg, np.float64)[..., :3].mean(-1))
    dev, ora = np.array(dev), np.array(ora)
    assert np.isfinite(dev).all()
    n = len(tm.SEEDS)
    return dev.mean(0), dev.std(0, ddof=1) / np.sqrt(n), np.abs(dev.mean(0) - ora.mean(0)).max()


@pytest.mark.parametrize("integrator,flag", tm.ABSORBER_VARIANTS)
@pytest.mark.parametrize("name", sorted(mc.VOLUMES))
def test_absorber_pixels_device(mi, orc, tmp_path, name, integrator, flag):
    s, T, spp = tm.absorber_reference(name)
    sc = mi.load_string(tm.absorber_xml(mi, tmp_path, name, integrator, flag))
    mean, se, gap = render_pair(sc, orc.OrcScene(sc), spp)
    tm.assert_pixels(mean, se, T, f"device absorber {name} {integrator} {flag} scale {s:.4f} spp {spp} (|device - oracle| <= {gap:.2e})")


@pytest.mark.parametrize("integrator,flag", tm.MARCH_VARIANTS)
@pytest.mark.parametrize("name", tm.MARCH_VOLUMES)
def test_emitter_march_device(mi, orc, tmp_path, name, integrator, flag):
    s, ref, spp = tm.march_reference(name)
    sc = mi.load_string(tm.march_xml(mi, tmp_path, name, integrator, flag))
    mean, se, gap = render_pair(sc, orc.OrcScene(sc), spp)
    tm.assert_pixels(mean, se, ref, f"device march {name} {integrator} {flag} scale {s:.4f} spp {spp} (|device - oracle| <= {gap:.2e})")
