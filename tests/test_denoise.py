"""Guided denoiser, the part that needs no GPU: properties of the specification on its numpy restatement
(tests/denoise_ref.py), the host logic of mi.Denoiser / mi.Bitmap, and the denoise kernels' resources read from the built code
object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as R

U = 2.0 ** -24          # unit roundoff of binary32


@pytest.fixture(scope="module")
def exp32(orc):
    return lambda x: orc.math_eval(1, x)[0]


# ---------------------------------------------------------------------------------------------- the restatement
def test_constant_image_comes_back(exp32):
    """Each pass is a convex combination of at most 25 values followed by one division: 26 roundings a pass, five passes."""
    for value, shape in ((0.7, (23, 31, 3)), (3.1e-3, (9, 40, 4)), (117.3, (33, 17, 3))):
        img = np.full(shape, value, np.float32)
        out = R.denoise_f32(exp32, img, denoise_alpha=True)
        rel = np.abs(out.astype(np.float64) / img.astype(np.float64) - 1).max()
        print(f"constant {value}: max relative deviation {rel:.3e} (bound {5 * 26 * U:.3e})")
        assert rel <= 5 * 26 * U


def test_demodulation_removes_texture_edges(exp32):
    """rgb = albedo * E with an arbitrary albedo pattern >= eps_a and constant E: the demodulated image is the constant E, so the
    texture's edges do not stop the filter and the input comes back: the constant-image bound plus the two roundings of
    demodulation and re-modulation."""
    rng = np.random.default_rng(5)
    h, w = 28, 37
    albedo = (0.05 + 0.9 * rng.random((h, w, 3))).astype(np.float32)
    eps_a = 0.01
    albedo[:, ::7] = 0.02; albedo[5:9, 3:30] = np.float32(eps_a)                    # hard edges, and the floor itself
    E = np.float32(2.75)
    rgb = (albedo * E).astype(np.float32)
    normals = np.zeros((h, w, 3), np.float32); normals[..., 2] = 1
    for nrm in (None, normals):
        out = R.denoise_f32(exp32, rgb, albedo, nrm, eps_a=eps_a)
        rel = np.abs(out.astype(np.float64) / rgb.astype(np.float64) - 1).max()
        print(f"albedo * E: max relative deviation {rel:.3e} (bound {(5 * 26 + 2) * U:.3e})")
        assert rel <= (5 * 26 + 2) * U


def f32_vs_f64_bound(M, d_max, sigma_color, iterations, demodulated):
    """Worst-case bound on |float32 result - float64 result| for colours c in [0, M] (after demodulation) and divisors <= d_max.

    E_k bounds the absolute error of c_k.  One pass:
      * accumulation: sum_ch has 1 product and <= 25 additions per term, sum_w <= 25 additions, then one division: the quotient of
        the two sums of positive terms is off by at most (26 + 25 + 1) u relative, i.e. 52 u M absolute;
      * weights: w = h_ij exp(-e).  Rounding inside e (one subtraction, one square, two additions, one product per norm, one
        addition per guide term: <= 8 u relative) moves w by w e 8 u <= 0.37 * 8 u h_ij (x exp(-x) <= 1 / e); m_exp is good to
        2 ulp = 4 u and the product with h_ij adds u: together <= 8 u h_ij.  The error E_k of both colours of a difference moves
        |dc|^2 by <= 2 |dc| 2 sqrt(3) E_k, hence e by that times ic_k, hence w by <= 4 sqrt(3) * 0.43 * sqrt(ic_k) E_k h_ij
        (sqrt(x) exp(-x) <= 0.43), sqrt(ic_k) = 2^k / sigma_color.  (Below -86 m_exp returns 0 where exp is < 1e-37: nothing.)
      * a weighted mean whose weights move by dw_i moves by <= sum |dw_i| * spread / sum_w, spread <= M, sum h_ij = 1 and
        sum_w >= h_00 = 9 / 64;
      * a convex combination passes the error of its inputs on unamplified: + E_k.
    E_0 = u M (the division of the demodulation), result error <= E_N d_max + u M d_max (the re-modulation)."""
    E = U * M if demodulated else 0.0
    for k in range(iterations):
        dw = 8 * U + 4 * np.sqrt(3) * 0.43 * (2 ** k / sigma_color) * E
        E = E + 52 * U * M + (64 / 9) * M * dw
    return E * d_max + (U * M * d_max if demodulated else 0.0)


@pytest.mark.parametrize("guides", ["none", "normals", "both"])
def test_float32_stays_within_rounding_bound_of_float64(exp32, guides):
    rng = np.random.default_rng(11)
    h, w = 40, 52
    noisy = rng.random((h, w, 4)).astype(np.float32)
    albedo = (0.5 + 0.5 * rng.random((h, w, 3))).astype(np.float32) if guides == "both" else None
    normals = None
    if guides != "none":
        normals = rng.standard_normal((h, w, 3)); normals = (normals / np.linalg.norm(normals, axis=2, keepdims=True)).astype(np.float32)
    prm = dict(sigma_color=64.0, sigma_normal=2.0, sigma_albedo=1.0, iterations=5)
    a = R.denoise_f32(exp32, noisy, albedo, normals, True, **prm)
    b = R.denoise_f64(noisy, albedo, normals, True, **prm)
    M = 2.0 if albedo is not None else 1.0          # colours in [0, 1], divisors in [0.5, 1]
    bound = f32_vs_f64_bound(M, 1.0, 64.0, 5, albedo is not None)
    err = np.abs(a.astype(np.float64) - b).max()
    moved = np.abs(b - noisy).max()
    print(f"guides={guides}: max |f32 - f64| = {err:.3e}, bound {bound:.3e}; the filter moved the image by up to {moved:.3f}")
    assert moved > 0.1                              # the filter did something
    assert err <= bound


def test_single_nan_stays_single(exp32):
    rng = np.random.default_rng(2)
    h, w = 70, 70
    noisy = rng.random((h, w, 3)).astype(np.float32)
    albedo = np.full((h, w, 3), 0.5, np.float32); normals = np.zeros((h, w, 3), np.float32)
    for where in ("colour", "albedo", "normals"):
        n, a, nr = noisy.copy(), albedo.copy(), normals.copy()
        {"colour": n, "albedo": a, "normals": nr}[where][35, 35, 1] = np.nan
        if where == "colour": n[20, 50, 0] = np.inf
        out = R.denoise_f32(exp32, n, a, nr, sigma_color=10.0)
        bad = ~np.isfinite(out).all(axis=2)
        expect = np.zeros((h, w), bool); expect[35, 35] = where == "colour"
        if where == "colour": expect[20, 50] = True
        assert (bad == expect).all(), where
        assert (out[35, 35].view(np.uint32) == n[35, 35].view(np.uint32)).all()        # copied through unchanged


# ---------------------------------------------------------------------------------------------- host logic
def test_bitmap_channel_selection(mi, tmp_path):
    rng = np.random.default_rng(3)
    names = ["img.R", "img.G", "img.B", "img.A", "alb.R", "alb.G", "alb.B", "nn.X", "nn.Y", "nn.Z", "dd.T"]
    data = rng.random((6, 9, len(names))).astype(np.float32)
    bmp = mi.Bitmap(data, channel_names=names)
    assert bmp.channel_count() == 11 and bmp.channel_names == names
    assert (bmp.select("alb") == data[..., 4:7]).all() and (bmp.select("nn") == data[..., 7:10]).all()
    assert (bmp.select("img") == data[..., 0:3]).all()
    with pytest.raises(RuntimeError, match="dd"):
        bmp.select("dd")
    with pytest.raises(RuntimeError, match="R"):
        bmp.select("<root>")                                     # a named bitmap without R, G, B
    with pytest.raises(ValueError, match="channel names"):
        mi.Bitmap(data, channel_names=names[:3])
    # "<root>": R, G, B[, A] by name, wherever they are ...
    mixed = mi.Bitmap(data[..., :7], channel_names=["alb.R", "B", "alb.G", "G", "A", "R", "alb.B"])
    assert (mixed.select("<root>") == data[..., [5, 3, 1, 4]]).all() and (mixed.select("alb") == data[..., [0, 2, 6]]).all()
    # ... or the first three or four channels of a bitmap without names
    assert (mi.Bitmap(data[..., :4]).select() == data[..., :4]).all() and (mi.Bitmap(data[..., :3]).select() == data[..., :3]).all()
    assert (mi.Bitmap(data).select() == data[..., :3]).all()
    with pytest.raises(RuntimeError, match="without channel names"):
        mi.Bitmap(data).select("alb")
    # names travel through an EXR file: every channel of the file comes back, R, G, B, A first
    plain = ["R", "G", "B", "A"] + names[4:]
    mi.write_exr(tmp_path / "multi.exr", data, channel_names=plain)
    back = mi.Bitmap(str(tmp_path / "multi.exr"))
    assert back.channel_names[:4] == ["R", "G", "B", "A"] and sorted(back.channel_names) == sorted(plain)
    assert (back.select("<root>") == data[..., :4]).all() and (back.select("alb") == data[..., 4:7]).all() and (back.select("nn") == data[..., 7:10]).all()
    assert (mi.read_image(tmp_path / "multi.exr") == data[..., :4]).all()              # the plain reader is unchanged
    back.write(str(tmp_path / "again.exr"))
    assert (mi.Bitmap(str(tmp_path / "again.exr")).select("nn") == data[..., 7:10]).all()
    # the converting constructor Denoise.py uses
    rgb8 = mi.Bitmap(mi.Bitmap(data[..., :4]), mi.Bitmap.PixelFormat.RGB, mi.Struct.Type.UInt8, srgb_gamma=True)
    assert rgb8.channel_count() == 3 and rgb8.srgb_gamma and rgb8.component_format == mi.Struct.Type.UInt8


def test_denoiser_interface_names_and_temporal(mi):
    assert mi.OptixDenoiser is mi.Denoiser
    with pytest.raises(RuntimeError, match="unsupported"):
        mi.Denoiser((16, 16), temporal=True)
    with pytest.raises(RuntimeError, match="unsupported"):
        mi.OptixDenoiser((16, 16), True, True, True)             # positional order of optixdenoiser.h:57-59


def test_argument_errors_without_a_device(mi):
    for kw, msg in ((dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(sigma_color=0.0), "sigma_color"),
                    (dict(sigma_normal=-1.0), "sigma_normal"), (dict(sigma_albedo=float("nan")), "sigma_albedo"), (dict(eps_a=-1e-3), "eps_a")):
        with pytest.raises(ValueError, match=msg):
            mi.Denoiser((16, 16), **kw)
    with pytest.raises(TypeError, match="sigma_colour"):
        mi.Denoiser((16, 16), sigma_colour=1.0)
    # the C ABI checks its arguments before it touches a device
    from liverrenderer_amd import _lib
    L = _lib.lib()
    assert L.lrt_version() >= 109

    def create(w, h, **p):
        hd = C.c_void_p()
        st = L.lrt_denoiser_create(w, h, 1, 1, 0, C.byref(_lib.DenoiseParams(**p)), 0, C.byref(hd))
        assert hd.value is None
        return st, L.lrt_last_error().decode()
    for args, msg in (((0, 16, {}), "size"), ((16, -3, {}), "size"), ((16, 1 << 20, {}), "size"), ((16, 16, dict(iterations=9)), "iterations"),
                      ((16, 16, dict(iterations=-1)), "iterations"), ((16, 16, dict(sigma_color=-2.0)), "sigma_color"),
                      ((16, 16, dict(sigma_normal=float("inf"))), "sigma_normal"), ((16, 16, dict(sigma_albedo=-0.5)), "sigma_albedo"),
                      ((16, 16, dict(eps_a=float("nan"))), "eps_a")):
        st, err = create(args[0], args[1], **args[2])
        assert st == 1 and msg in err, (args, st, err)           # LRT_ERR_INVALID
    assert L.lrt_denoise(None, None, 3, None, None, None, 0) == 1 and "null" in L.lrt_last_error().decode()
    assert {"lrt_denoiser_create", "lrt_denoise", "lrt_denoiser_free"} <= set(_lib.EXPORTED_SYMBOLS)


# ---------------------------------------------------------------------------------------------- kernel resources
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "liverrenderer_amd", "libliverrt.so")
LLVM = "/opt/rocm/llvm/bin"
TOOLS = {k: os.path.join(LLVM, k) for k in ("clang-offload-bundler", "llvm-objcopy", "llvm-readelf")}
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
DENOISE_KERNELS = {"_ZN3lrt14k_denoise_packI": 8, "_ZN3lrt14k_denoise_passI": 8, "_ZN3lrt16k_denoise_unpackI": 2}    # prefix -> instances


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS.values()), reason="LLVM offload tools missing")
def test_denoise_kernels_use_no_scratch(tmp_path):
    """Zero scratch and zero spills for every instance of the three denoise kernels, from the metadata of the gfx950 code object
    inside the built library (no GPU needed)."""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([TOOLS["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fat, LIB, str(tmp_path / "stripped.so")], check=True, capture_output=True)
    subprocess.run([TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co], check=True, capture_output=True)
    notes = subprocess.run([TOOLS["llvm-readelf"], "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for entry in re.split(r"\n  - ", notes):
        m = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if m:
            kernels[m.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", entry, re.M)}
    for prefix, count in DENOISE_KERNELS.items():
        names = sorted(n for n in kernels if n.startswith(prefix))
        assert len(names) == count, (prefix, names)
        for n in names:
            md = kernels[n]
            print(f"{n}: {md['vgpr_count']} VGPRs")
            assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, (n, md)
            assert md["vgpr_count"] <= 128, (n, md)              # four waves per SIMD at least
