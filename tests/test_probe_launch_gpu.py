"""The launch path the six probes share (csrc/probes.h k_probe, device.hip device_probe): the lane stride, the
packing of the input columns into lane records, the tail guard and the block boundary.  No reference is needed: every probe is compared
with itself at another batch size.  On the smallest scene of its case module, with that module's own probe inputs, a call of
LRT_BLOCK + 1 = 257 lanes must return in rows 0, 255 and 256 the very bits that three one-lane calls return for those lanes, must not
write behind row 256, and a call of 0 lanes must write nothing."""
import ctypes as C

import numpy as np
import pytest

import envmap_cases as ec
import medium_cases as mc
import phase_cases as pc
import sensor_cases as sn
import spot_cases as sp
import surface_cases as sf
import surface_ref as sr

pytestmark = pytest.mark.gpu

N = 257                                   # LRT_BLOCK + 1: two blocks, the second with one live lane
ROWS = (0, 255, 256)                      # the first lane, the last lane of the first block, the only lane of the second
SENTINEL = np.uint32(0xDEADBEEF)


def tiled(a, n=N):
    """the first n rows of a, repeated from the start if it has fewer"""
    a = np.asarray(a)
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


def emitter_case(mi, tmp):
    case = sp.configs()[0]
    return mi.load_string(sp.scene_xml(case)), None, [tiled(c) for c in sp.make_inputs(case)], mi._lib.PROBE_FLOATS


def envmap_case(mi, tmp):
    scene, ref = ec.load(mi, tmp, "rand_5x3")
    return scene, None, [tiled(ec.chosen_directions(ref))], 4


def bsdf_case(mi, tmp):
    scene, surf = sf.build(mi, tmp, [("rectangle", ("dielectric", "1.5"))])
    rng = np.random.default_rng(1)
    o, d, s1 = sf.sweep_rays(surf[0], 1.5, rng)               # the rays of check_dielectric, its samples and query directions
    n = len(s1)
    smp = np.stack([s1, rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)], 1)
    woq = sr.unit(rng.normal(size=(n, 3)))
    return scene, None, [tiled(np.asarray(c, np.float32)) for c in (o, d, smp, woq)], mi._lib.BSDF_PROBE_FLOATS


def phase_case(mi, tmp):
    p = pc.configs()[0]
    return mi.load_dict(pc.scene_dict(p)), 0, [tiled(c) for c in pc.make_inputs(p)], mi._lib.PHASE_PROBE_FLOATS


def medium_case(mi, tmp):
    """volume b (the 2 x 3 x 1 grid): its rays, with the lane whose origin holds a NaN in row 255 and a lookup-only lane (maxt = NaN)
    in row 256"""
    scene = mi.load_string(mc.probe_scene_xml(mi, tmp, "b"))
    o, d, maxt, smp, ch, kind = mc.probe_rays("b")
    cols = [tiled(c, N - 2) for c in (o, d, maxt, smp, ch)]
    k = len(kind) - 1 - kind[::-1].index("nan")               # (the last such lane: it carries a random sample)
    pts, _ = mc.local_points(mc.VOLUMES["b"]["grid"].shape)
    tail = [np.stack([o[k], pts[0]]), np.stack([d[k], np.zeros(3, np.float32)]), np.float32([maxt[k], np.nan]), np.float32([smp[k], 0]), np.uint32([ch[k], 0])]
    cols = [np.ascontiguousarray(np.concatenate([c, t])) for c, t in zip(cols, tail)]
    assert np.isnan(cols[0][255]).any() and np.isnan(cols[2][256])
    return scene, 0, cols, mi._lib.MEDIUM_PROBE_FLOATS


def sensor_case(mi, tmp):
    return mi.load_dict(sn.scene_dict(mi, "a", "box")), None, [tiled(sn.probe_inputs("a", "box"))], mi._lib.SENSOR_PROBE_FLOATS


MAKE = {"emitter": emitter_case, "envmap": envmap_case, "bsdf": bsdf_case, "phase": phase_case, "medium": medium_case, "sensor": sensor_case}


@pytest.fixture(scope="module")
def cases(mi, tmp_path_factory):
    """kind -> run(first, n, out): lanes first .. first + n - 1 of the kind's 257 input lanes through its C entry point into `out`; the status"""
    tmp = tmp_path_factory.mktemp("probe_launch"); made = {}; L = mi._lib.lib()
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32 if a.dtype == np.uint32 else C.c_float))

    def get(kind):
        if kind not in made:
            scene, medium, cols, width = MAKE[kind](mi, tmp)
            assert all(len(c) == N for c in cols)
            fn = getattr(L, f"lrt_{kind}_probe")

            def run(first, n, out):
                part = [np.ascontiguousarray(c[first:first + n]) for c in cols]
                return fn(scene._h, *([] if medium is None else [medium]), *map(ptr, part), n, ptr(out), 0)
            made[kind] = (run, width)
        return made[kind]
    return get


def sentinels(rows, width):
    return np.full((rows, width), SENTINEL, np.uint32).view(np.float32)


@pytest.mark.parametrize("kind", list(MAKE))
def test_rows_of_a_257_lane_call_equal_one_lane_calls(mi, cases, kind):
    run, width = cases(kind)
    out = sentinels(N + 1, width)                                 # one row more than the call may write
    assert run(0, N, out) == mi._lib.OK
    bits = out.view(np.uint32)
    assert (bits[N] == SENTINEL).all(), "the row behind the last lane was written"
    assert not (bits[:N] == SENTINEL).all(1).any(), "a lane was not written"
    for i in ROWS:
        one = sentinels(1, width)
        assert run(i, 1, one) == mi._lib.OK
        assert np.array_equal(bits[i], one.view(np.uint32)[0]), (kind, i, out[i], one[0])
    assert len({bits[i].tobytes() for i in ROWS}) > 1, "the three lanes cannot be told apart"


@pytest.mark.parametrize("kind", list(MAKE))
def test_a_call_of_no_lanes_writes_nothing(mi, cases, kind):
    run, width = cases(kind)
    out = sentinels(2, width)
    assert run(0, 0, out) == mi._lib.OK
    assert (out.view(np.uint32) == SENTINEL).all()
