"""CPU tests of the `moment` integrator (src/integrators/moment.cpp): loading from XML and from a dict, channel names and counts,
the lrt_moment_desc layout, the rejected cases, the numpy restatement of the per-sample arithmetic (tests/moment_ref.py) against a
float64 evaluation, mi.moment_variance / mi.z_test on arrays with known answers, and the resources of the k_moment_* kernels read
from the built code object.  No compute call is made."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import moment_ref
from conftest import ROOT

XML = """<scene version="3.0.0">
    <integrator type="moment">{extra}
        {nested}
    </integrator>
    <sensor type="perspective">
        <float name="fov" value="45"/>
        <sampler type="independent"><integer name="sample_count" value="8"/></sampler>
        <film type="hdrfilm">
            <integer name="width" value="32"/>
            <integer name="height" value="24"/>
            <string name="pixel_format" value="{fmt}"/>
        </film>
    </sensor>
    <shape type="rectangle"/>
</scene>"""


def moment_xml(nested='<integrator type="path" name="img"/>', fmt="rgb", extra=""):
    return XML.format(nested=nested, fmt=fmt, extra=extra)


def moment_dict(key="nested", inner=None, fmt="rgb"):
    return {"type": "scene",
            "integrator": {"type": "moment", key: inner or {"type": "path"}},
            "sensor": {"type": "perspective", "fov": 45.0,
                       "film": {"type": "hdrfilm", "width": 32, "height": 24, "pixel_format": fmt}},
            "rect": {"type": "rectangle"}}


# ------------------------------------------------------------------------------------------------------------ loading
def test_xml_form_names_and_counts(mi):
    sc = mi.load_string(moment_xml())
    assert sc.is_moment() and not sc.is_aov()
    assert sc.moment_channel_names() == ["R", "G", "B", "img.X", "img.Y", "img.Z", "m2_img.X", "m2_img.Y", "m2_img.Z"]
    m = sc.moment_desc()
    assert (m.n_channels, m.n_raw_channels, m.name) == (9, 10, b"img")
    assert (m.integrator.type, m.integrator.max_depth, m.integrator.rr_depth, m.integrator.hide_emitters) == (0, -1, 5, 0)
    # the description is an ordinary scene: its integrator is the nested one
    d = sc.desc.integrator
    assert (d.type, d.max_depth, d.rr_depth, d.hide_emitters) == (0, -1, 5, 0)


def test_alpha_film(mi):
    sc = mi.load_string(moment_xml(fmt="rgba"))
    assert sc.moment_channel_names() == ["R", "G", "B", "A", "img.X", "img.Y", "img.Z", "m2_img.X", "m2_img.Y", "m2_img.Z"]
    m = sc.moment_desc()
    assert (m.n_channels, m.n_raw_channels) == (10, 11)


def test_unnamed_child_gets_the_parsers_name(mi):
    """src/core/parser.cpp:1023-1025: an object without `name` becomes property "_arg_<k>" of its parent."""
    sc = mi.load_string(moment_xml(nested='<integrator type="volpath"><integer name="max_depth" value="7"/></integrator>'))
    assert sc.moment_desc().name == b"_arg_0"
    assert sc.moment_channel_names()[3:] == ["_arg_0.X", "_arg_0.Y", "_arg_0.Z", "m2__arg_0.X", "m2__arg_0.Y", "m2__arg_0.Z"]
    assert (sc.desc.integrator.type, sc.desc.integrator.max_depth) == (1, 7)


def test_dict_form(mi):
    xml = mi.dict_to_xml(moment_dict())
    assert '<integrator type="moment">' in xml and '<integrator type="path" name="nested">' in xml
    sc = mi.load_dict(moment_dict())
    assert sc.moment_channel_names()[3:6] == ["nested.X", "nested.Y", "nested.Z"]
    sc = mi.load_dict(moment_dict("vp", {"type": "volpathmis", "max_depth": 9, "use_spectral_mis": False}, fmt="rgba"))
    assert sc.moment_desc().name == b"vp" and sc.moment_desc().n_raw_channels == 11
    assert (sc.desc.integrator.type, sc.desc.integrator.max_depth, sc.desc.use_spectral_mis) == (5, 9, 0)


@pytest.mark.parametrize("typ, code", [("path", 0), ("volpath", 1), ("volpathmis", 5), ("biovolpath", 3), ("biovolpath06", 4)])
def test_every_supported_nested_integrator(mi, typ, code):
    sc = mi.load_string(moment_xml(nested=f'<integrator type="{typ}" name="n"><integer name="rr_depth" value="3"/></integrator>'))
    assert (sc.moment_desc().integrator.type, sc.moment_desc().integrator.rr_depth, sc.desc.integrator.type) == (code, 3, code)


def test_samples_per_pass_comes_from_the_moment_integrator(mi):
    sc = mi.load_string(moment_xml(extra='<integer name="samples_per_pass" value="2"/>'))
    assert sc.desc.samples_per_pass == 2


def test_ordinary_scene_is_not_a_moment_scene(mi, cornell):
    assert cornell.moment_desc() is None and not cornell.is_moment()
    with pytest.raises(RuntimeError, match="no moment integrator"):
        cornell.moment_channel_names()
    with pytest.raises(RuntimeError, match="no moment integrator"):
        cornell.render_moment_samples(0, 4)
    with pytest.raises(RuntimeError, match="no moment integrator"):
        mi.moment_variance(np.zeros((2, 2, 9), np.float32), cornell, 4)
    L = mi._lib.lib()
    assert L.lrt_moment_channel_name(cornell._h, 0) is None
    img = np.zeros(4, np.float32)
    o = mi._lib.make_opts()
    assert L.lrt_render_moment(cornell._h, C.byref(o), None, img.ctypes.data) == 1 and "no moment integrator" in L.lrt_last_error().decode()
    sc = mi.load_string(moment_xml())
    assert L.lrt_moment_channel_name(sc._h, 9) is None and L.lrt_moment_channel_name(sc._h, -1) is None
    assert L.lrt_moment_channel_name(sc._h, 8) == b"m2_img.Z"


# ------------------------------------------------------------------------------------------------------- rejected cases
def _load_error(mi, xml):
    L = mi._lib.lib()
    h = C.c_void_p()
    st = L.lrt_scene_load_xml_string(xml.encode(), b".", None, 0, C.byref(h))
    assert not h.value
    return st, L.lrt_last_error().decode()


UNSUPPORTED, INVALID = 4, 1


def test_unsupported_nestings(mi):
    st, msg = _load_error(mi, moment_xml(nested='<integrator type="path" name="a"/><integrator type="volpath" name="b"/>'))
    assert st == UNSUPPORTED and "two or more nested integrators" in msg and "sampler stream" in msg
    for typ in ("aov", "moment", "prbvolpath"):
        st, msg = _load_error(mi, moment_xml(nested=f'<integrator type="{typ}" name="a"/>'))
        assert st == UNSUPPORTED and f'nested "{typ}" integrator is not supported' in msg, (typ, st, msg)
    # the other way round: a moment integrator under aov
    aov = moment_xml().replace('type="moment"', 'type="aov"').replace('<integrator type="path" name="img"/>',
                                                                       '<integrator type="moment" name="m"><integrator type="path"/></integrator>')
    st, msg = _load_error(mi, aov)
    assert st == UNSUPPORTED and 'aov: a nested "moment" integrator is not supported' in msg, (st, msg)


def test_a_moment_integrator_without_a_child_is_an_error(mi):
    st, msg = _load_error(mi, moment_xml(nested=""))
    assert st == INVALID and "no nested integrator" in msg
    st, msg = _load_error(mi, moment_xml(nested='<bsdf type="diffuse"/>'))
    assert st == INVALID and "SamplingIntegrator" in msg


def test_backward_and_multi_are_rejected_before_any_device_call(mi):
    sc = mi.load_string(moment_xml())
    L = mi._lib.lib()
    o = mi._lib.make_opts()
    g = np.zeros((24, 32, 3), np.float32); out = mi._lib.ParamGrads(); img = np.zeros((24, 32, 9), np.float32)
    assert L.lrt_render_backward(sc._h, C.byref(o), g.ctypes.data, C.byref(out)) == UNSUPPORTED
    assert "moment integrator has no adjoint" in L.lrt_last_error().decode()
    ids = (C.c_int * 1)(0)
    assert L.lrt_render_backward_multi(sc._h, C.byref(o), 1, ids, g.ctypes.data, C.byref(out)) == UNSUPPORTED
    assert "moment integrator has no adjoint" in L.lrt_last_error().decode()
    assert L.lrt_render_multi(sc._h, C.byref(o), 1, ids, None, img.ctypes.data) == UNSUPPORTED
    assert "moment scene renders on one device" in L.lrt_last_error().decode()
    # the nested integrator comes from the scene
    o2 = mi._lib.make_opts(max_depth=3)
    assert L.lrt_render_moment(sc._h, C.byref(o2), None, img.ctypes.data) == INVALID
    assert "come from the scene's nested integrator" in L.lrt_last_error().decode()
    assert L.lrt_render_moment_samples(sc._h, C.byref(o2), 0, 4, img.ctypes.data) == INVALID


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_version_and_symbols(mi):
    L = mi._lib.lib()
    assert L.lrt_version() >= 110
    assert {"lrt_scene_moment_get", "lrt_moment_channel_name", "lrt_render_moment", "lrt_render_moment_samples"} <= set(mi._lib.EXPORTED_SYMBOLS)
    for name in ("lrt_scene_moment_get", "lrt_moment_channel_name", "lrt_render_moment", "lrt_render_moment_samples"):
        assert hasattr(L, name)


def test_moment_desc_layout_matches_the_compiler(mi):
    """sizeof / offsetof of lrt_moment_desc as the C compiler lays it out, against the ctypes mirror."""
    fields = [f for f, _ in mi._lib.MomentDesc._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "liverrt.h"\nint main(void) {\n  printf("%zu\\n", sizeof(lrt_moment_desc));\n'
    src += "".join(f'  printf("%zu\\n", offsetof(lrt_moment_desc, {f}));\n' for f in fields) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(c, "w").write(src)
        subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        vals = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == C.sizeof(mi._lib.MomentDesc)
    assert vals[1:] == [getattr(mi._lib.MomentDesc, f).offset for f in fields]
    assert C.sizeof(mi._lib.MomentDesc) == 16 + 64 + 8


# ------------------------------------------------------------------------------------------- the restated arithmetic
M32 = moment_ref.SRGB_TO_XYZ.astype(np.float64)
U = 2.0 ** -24                   # unit roundoff of binary32


def test_fma32_is_correctly_rounded():
    """Against exact rational arithmetic on cases built to sit at float32 rounding midpoints (where a float64 sum rounded twice
    goes wrong) and on random inputs."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(2000).astype(np.float32); b = rng.standard_normal(2000).astype(np.float32)
    c = (rng.standard_normal(2000) * 10.0 ** rng.integers(-12, 3, 2000)).astype(np.float32)
    # midpoint cases: a * b = 1 + 2^-24 exactly (a = 1 + 2^-12, b = 1 - 2^-12 + 2^-24 is not representable; use c to land on a tie)
    a = np.concatenate([a, np.float32([1.0, 1.0, 3.0, 1.0 + 2.0 ** -23])]); b = np.concatenate([b, np.float32([1.0, 1.0, 1.0, 1.0 + 2.0 ** -23])])
    c = np.concatenate([c, np.float32([2.0 ** -24, 2.0 ** -24 + 2.0 ** -60, 2.0 ** -23, 2.0 ** -24])])
    got = moment_ref.fma32(a, b, c)
    for k in range(len(a)):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo = np.float32(float(exact))                    # float(Fraction) rounds correctly to double; refine to the nearest float32 exactly
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        err = [abs(Fraction(float(v)) - exact) for v in cands]
        best = min(err)
        winners = [v for v, e in zip(cands, err) if e == best]
        if len(winners) == 2:                            # a tie: the even mantissa
            winners = [v for v in winners if (np.float32(v).view(np.uint32) & 1) == 0]
        assert got[k] == winners[0], (k, a[k], b[k], c[k], got[k], winners)


def test_moment_ref_against_float64():
    rng = np.random.default_rng(7)
    L = np.concatenate([rng.random((4000, 3)) * 30.0, rng.standard_normal((1000, 3)) * 1e-3, rng.random((500, 3)) * 1e30,
                        np.zeros((1, 3)), np.float64([[1e-45, 0, 0], [1e-40, 2e-41, 3e-42], [1.4e-45, 1.4e-45, 1.4e-45], [1e-38, 0, 1e-39]])]).astype(np.float32)
    out = moment_ref.moment_values(L)
    L64 = L.astype(np.float64)
    exact = L64 @ M32.T
    # three roundings (the product, two fmas), each of a partial sum no larger than sum |m c|: relative error 2^-24 each, or half the
    # denormal spacing, 2^-150, where the partial sum lies in the denormal range
    bound = 3 * (U * (np.abs(L64) @ np.abs(M32).T) * (1 + 4 * U) + 2.0 ** -150)
    assert np.all(np.abs(out[:, :3].astype(np.float64) - exact) <= bound)
    with np.errstate(over="ignore"):
        sq = (out[:, :3].astype(np.float64) ** 2).astype(np.float32)               # one rounding of the exact square (overflow: inf on both sides)
    assert np.array_equal(out[:, 3:], sq)
    assert np.array_equal(out[-5], np.zeros(6, np.float32))
    # denormal inputs give denormal (or zero) results, never a flush of a representable value: X of (2^-149, 0, 0) is round(0.412 * 2^-149) = 0,
    # of (1e-40, ...) a denormal
    assert out[-4, 0] == 0 and 0 < out[-3, 0] < 1.2e-38


def test_moment_ref_non_finite_inputs():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    L = np.float32([[inf, 0, 0], [0, inf, 1], [1, 2, -inf], [inf, -inf, 0], [nan, 1, 1], [1, nan, 1], [1, 1, nan], [3e38, 3e38, 3e38], [-inf, -inf, -inf]])
    out = moment_ref.moment_values(L)
    with np.errstate(invalid="ignore", over="ignore"):
        exact = L.astype(np.float64) @ M32.T                    # inf - inf = NaN in any precision; every matrix entry is positive
        ex32 = exact.astype(np.float32)
    assert np.array_equal(np.isnan(out[:, :3]), np.isnan(ex32))
    assert np.array_equal(np.isinf(out[:, :3]), np.isinf(ex32)) and np.array_equal(np.sign(out[:, :3][np.isinf(ex32)]), np.sign(ex32[np.isinf(ex32)]))
    assert np.all(out[0, :3] == inf) and np.all(out[2, :3] == -inf) and np.isnan(out[3, :3]).all() and np.isnan(out[4:7]).all()
    assert np.all(out[0, 3:] == inf) and np.all(out[8, 3:] == inf)                   # squares of +-inf
    assert np.isfinite(out[7, :3]).all() and np.all(out[7, 3:] == inf)               # 3e38: X finite, X * X overflows


def test_moment_ref_zeroes_invalid_path_samples():
    lanes = np.float32([[1, 2, 3, 1], [4, 5, 6, 0]])
    a = moment_ref.moment_lanes(lanes, integrator_is_path=True)
    assert np.array_equal(a[1], np.zeros(6, np.float32)) and a[0, 1] > 0
    b = moment_ref.moment_lanes(lanes, integrator_is_path=False)
    assert b[1, 1] > 0
    rec = moment_ref.film_record(lanes, True, True)
    assert rec.shape == (2, 11) and np.array_equal(rec[1], np.float32([0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0])) and np.array_equal(rec[0, :5], np.float32([1, 2, 3, 1, 1]))
    assert moment_ref.film_record(lanes, False, False).shape == (2, 10)


# ----------------------------------------------------------------------------------------- moment_variance and z_test
def test_moment_variance_known_answers(mi):
    sc = mi.load_string(moment_xml())
    sca = mi.load_string(moment_xml(fmt="rgba"))
    # a pixel whose 4 samples have X = 1, 2, 3, 6: m1 = 3, m2 = 12.5, unbiased sample variance 14 / 3, of the mean 14 / 12
    img = np.zeros((2, 3, 9), np.float32)
    img[0, 0, 3:6] = [3.0, 0.5, 0.0]; img[0, 0, 6:9] = [12.5, 0.25, 0.0]
    img[1, 2, 3:6] = [1.0, 1.0, 1.0]; img[1, 2, 6:9] = [0.999, 1.0, 2.0]          # rounding made m2 < m1^2: clamped at 0
    var, mean = mi.moment_variance(img, sc, 4)
    assert var.shape == (2, 3, 3) and var.dtype == np.float64 and mean.shape == (2, 3, 3)
    assert var[0, 0, 0] == pytest.approx(14.0 / 12.0, rel=1e-12) and var[0, 0, 1] == 0.0 and var[0, 0, 2] == 0.0
    assert var[1, 2, 0] == 0.0 and var[1, 2, 1] == 0.0 and var[1, 2, 2] == pytest.approx(1.0 / 3.0, rel=1e-12)
    assert np.array_equal(mean[0, 0], [3.0, 0.5, 0.0])
    imga = np.zeros((2, 3, 10), np.float32); imga[..., 4:] = img[..., 3:]
    vara, meana = mi.moment_variance(imga, sca, 4)
    assert np.array_equal(vara, var) and np.array_equal(meana, mean)
    with pytest.raises(RuntimeError, match="channels"):
        mi.moment_variance(img, sca, 4)
    with pytest.raises(ValueError):
        mi.moment_variance(img, sc, 1)
    # against numpy on random samples
    rng = np.random.default_rng(1)
    s = rng.random((5, 7, 3, 16))
    img = np.zeros((5, 7, 9)); img[..., 3:6] = s.mean(-1); img[..., 6:9] = (s * s).mean(-1)
    var, _ = mi.moment_variance(img, sc, 16)
    np.testing.assert_allclose(var, s.var(-1, ddof=1) / 16, rtol=1e-9)


def test_z_test_known_answers(mi):
    a = np.zeros((4, 5)); b = np.zeros((4, 5)); va = np.full((4, 5), 0.5); vb = np.full((4, 5), 0.5)
    b[0, 0] = 1.0          # z = 1: p = erfc(1 / sqrt 2) = 0.31731...
    b[0, 1] = 1.959964     # z = 1.96: p = 0.05
    b[0, 2] = 6.0          # z = 6: p = 1.97e-9 < the corrected level
    p, frac = mi.z_test(a, va, b, vb)
    assert p.shape == (4, 5)
    assert p[0, 0] == pytest.approx(0.3173105078629141, rel=1e-12) and p[0, 1] == pytest.approx(0.05, rel=1e-5) and p[0, 2] == pytest.approx(math.erfc(6 / math.sqrt(2)), rel=1e-12)
    assert np.all(p[1:] == 1.0)
    level = 1 - 0.99 ** (1 / 20)                                   # Sidak over 20 pixels: 5.02e-4
    assert level == pytest.approx(5.0240e-4, rel=1e-3)
    assert frac == 19 / 20
    # z = 3.4: p = 6.7e-4 passes the corrected level of 20 pixels, and fails uncorrected-like levels of a single pixel
    b[:] = 0; b[2, 2] = 3.4
    assert mi.z_test(a, va, b, vb)[1] == 1.0
    assert mi.z_test(a[2:3, 2:3], va[2:3, 2:3], b[2:3, 2:3], vb[2:3, 2:3])[1] == 0.0
    assert mi.z_test(a, va, b, vb, alpha=0.5)[1] == 19 / 20
    # symmetric, and the two variances add
    assert np.array_equal(mi.z_test(b, vb, a, va)[0], mi.z_test(a, va, b, vb)[0])
    assert mi.z_test(a, va * 2, b, vb * 0)[0][2, 2] == mi.z_test(a, va, b, vb)[0][2, 2]


def test_z_test_pixels_without_an_error_bar(mi):
    a = np.float64([[1.0, 2.0], [0.0, 5.0]]); b = np.float64([[1.0, 2.5], [0.0, 5.0]])
    z = np.zeros((2, 2))
    p, frac = mi.z_test(a, z, b, z)
    assert np.array_equal(p, [[1.0, 0.0], [1.0, 1.0]]) and frac == 0.75          # compared for equality, counted in the denominator
    with pytest.raises(ValueError):
        mi.z_test(a, z, b[:1], z)
    with pytest.raises(ValueError):
        mi.z_test(a, z - 1, b, z)
    # three channels: N is the pixel count, the fraction runs over every value
    a3 = np.zeros((2, 2, 3)); v3 = np.ones((2, 2, 3)); b3 = a3.copy(); b3[0, 0, 1] = 100.0
    p, frac = mi.z_test(a3, v3, b3, v3)
    assert frac == 11 / 12


# -------------------------------------------------------------------------------------------------- kernel resources
LIB = os.path.join(ROOT, "liverrenderer_amd", "libliverrt.so")
LLVM = "/opt/rocm/llvm/bin"
TOOLS = {k: os.path.join(LLVM, k) for k in ("clang-offload-bundler", "llvm-objcopy", "llvm-readelf")}
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MOMENT_KERNELS = {"_ZN3lrt14k_moment_splatI": 4, "_ZN3lrt16k_moment_developI": 2, "_ZN3lrt14k_moment_lanesE": 1}    # prefix -> instances


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS.values()), reason="LLVM offload tools missing")
def test_moment_kernels_use_no_scratch(tmp_path):
    """Zero scratch and zero spills for every instance of the moment kernels, from the metadata of the gfx950 code object inside the
    built library (no GPU needed)."""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([TOOLS["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fat, LIB, str(tmp_path / "stripped.so")], check=True, capture_output=True)
    subprocess.run([TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co], check=True, capture_output=True)
    notes = subprocess.run([TOOLS["llvm-readelf"], "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for entry in re.split(r"\n  - ", notes):
        m = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if m:
            kernels[m.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", entry, re.M)}
    for prefix, count in MOMENT_KERNELS.items():
        names = sorted(n for n in kernels if n.startswith(prefix))
        assert len(names) == count, (prefix, names)
        for n in names:
            md = kernels[n]
            print(f"{n}: {md['vgpr_count']} VGPRs")
            assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, (n, md)
            assert md["vgpr_count"] <= 64, (n, md)               # eight waves per SIMD
