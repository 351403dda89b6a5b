"""The perspective sensor and the film on the device: lrt_sensor_probe against the float64 restatement of
tests/sensor_ref.py with the K table of test_sensor.py, bit for bit against the oracle's probe, the reference's own vectors, k_develop on
crafted films against numpy's float32 division, and one closed form per pixel through the whole chain (sensor, integrator, splat,
develop) for a rectangle emitter cut by the clip planes."""
import ctypes as C

import numpy as np
import pytest

import sensor_cases as sc
import test_sensor as ts

pytestmark = pytest.mark.gpu


def device_probe_of(mi):
    return lambda sensor, rfilter, inp: mi.load_dict(sc.scene_dict(mi, sensor, rfilter)).sensor_probe(inp)


@pytest.mark.parametrize("sensor,rfilter", ts.PROBE_CASES)
def test_device_probe_matches_float64_and_oracle(mi, orc, sensor, rfilter):
    scene = ts.load(mi, sensor, rfilter); inp = sc.probe_inputs(sensor, rfilter)
    got = scene.sensor_probe(inp)
    ts.check_probe(got, sensor, rfilter, "device")
    want = orc.OrcScene(scene).sensor_probe(inp)
    bad = np.argwhere(got["raw"].view(np.uint32) != want["raw"].view(np.uint32))
    assert len(bad) == 0, (sensor, rfilter, bad[:8], got["raw"][bad[0][0]], want["raw"][bad[0][0]])


def test_probe_arguments(mi):
    scene = ts.load(mi, "a", "box"); L = mi._lib.lib(); FP = C.POINTER(C.c_float)
    inp = sc.probe_inputs("a", "box")[:3].copy(); out = np.zeros((3, mi._lib.SENSOR_PROBE_FLOATS), np.float32)
    assert L.lrt_sensor_probe(scene._h, inp.ctypes.data_as(FP), 3, out.ctypes.data_as(FP), 0) == mi._lib.OK and out[:, 14].tolist() == [1.0] * 3
    assert L.lrt_sensor_probe(None, inp.ctypes.data_as(FP), 3, out.ctypes.data_as(FP), 0) == mi._lib.INVALID
    assert L.lrt_sensor_probe(scene._h, None, 3, out.ctypes.data_as(FP), 0) == mi._lib.INVALID
    assert L.lrt_sensor_probe(scene._h, inp.ctypes.data_as(FP), 3, None, 0) == mi._lib.INVALID
    assert L.lrt_sensor_probe(scene._h, inp.ctypes.data_as(FP), 0, out.ctypes.data_as(FP), 0) == mi._lib.OK            # nothing to do


def test_known_filters_device(mi):
    ts.check_known_filters(device_probe_of(mi))


def test_known_perspective_device(mi):
    ts.check_known_perspective(device_probe_of(mi))


def test_known_imageblock_device(mi):
    ts.check_known_imageblock(device_probe_of(mi))


def test_develop_device(mi):
    """k_develop against numpy's float32 film / where(W == 0, 1, W), bit for bit, a NaN equal to a NaN: W zero, negative zero, denormal,
    negative, infinite and NaN beside ordinary, non-finite and denormal colours; rgb and rgba"""
    ts.check_develop(lambda sensor, fmt, film: ts.load(mi, sensor, "box", "path", fmt).develop(film))


# -------------------------------------------------------------------------------------------------------- closed form
@pytest.mark.parametrize("integrator", sc.CLOSED_INTEGRATORS)
@pytest.mark.parametrize("rfilter", sc.CLOSED_FILTERS)
@pytest.mark.parametrize("sensor", sc.CLOSED_SENSORS)
def test_rectangle_closed_form(mi, sensor, rfilter, integrator):
    scene = ts.load(mi, sensor, rfilter, integrator, "rgba", 4)
    ts.check_closed_form(mi, sensor, rfilter, integrator, lambda seed: scene.render(spp=sc.SPP, seed=seed), "device")
