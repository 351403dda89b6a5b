"""Guided denoiser on the device: every output value bit-identical to the numpy restatement of DESIGN.md section 9.1
(tests/denoise_ref.py with the oracle's exp), the torch-tensor path, the direction of the quality change, and the C ABI's errors.

Measured on one MI355X (8 spp against 1024 spp at 128 x 72, default parameters; RMSE noisy -> denoised, ratio): Cornell box
0.05065 -> 0.04942 (0.976), Liver-SingleMesh volpath 0.06107 -> 0.04942 (0.809); the test asserts the direction only
(DESIGN.md section 9.3)."""
import itertools
import os
import re

import numpy as np
import pytest

import denoise_ref as R
from conftest import LIVER_XML

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exp32(orc):
    return lambda x: orc.math_eval(1, x)[0]


def inputs(h, w, channels, seed):
    """A piecewise-smooth image under noise with guides that have edges: weights take every size between 0 and 1."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    region = ((x // 7 + y // 5) % 3).astype(np.float32)
    albedo = (0.2 + 0.3 * region[..., None] + 0.02 * rng.random((h, w, 3))).astype(np.float32)
    if h > 2: albedo[h // 2, :, 1] = 0.0                                   # below eps_a: the floor of the divisor
    normals = np.stack([np.sin(0.1 * x + region), np.cos(0.07 * y), np.ones_like(x)], axis=2)
    normals = (normals / np.linalg.norm(normals, axis=2, keepdims=True) + 0.01 * rng.standard_normal((h, w, 3))).astype(np.float32)
    light = 1.0 + 0.5 * np.sin(0.05 * (x + 2 * y))
    noisy = (albedo * light[..., None] * (1 + 0.4 * rng.standard_normal((h, w, 3)))).astype(np.float32)
    if channels == 4:
        noisy = np.concatenate([noisy, rng.random((h, w, 1)).astype(np.float32)], axis=2)
    return noisy, albedo, normals


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def check(mi, exp32, noisy, albedo, normals, denoise_alpha=False, **params):
    h, w = noisy.shape[:2]
    dn = mi.Denoiser((w, h), albedo is not None, normals is not None, False, denoise_alpha, **params)
    got = dn(noisy, albedo, normals)
    ref = R.denoise_f32(exp32, noisy, albedo, normals, denoise_alpha, **dn.params)
    share = (got.view(np.uint32) == ref.view(np.uint32)).all(axis=2).mean()
    assert same_bits(got, ref), f"{share:.6f} of {h * w} pixels bit-identical"          # every pixel, every channel
    return got


@pytest.mark.parametrize("h,w", [(1, 1), (3, 300), (67, 45), (256, 256)])
@pytest.mark.parametrize("channels", [3, 4])
def test_bit_identical_at_border_stressing_sizes(mi, exp32, h, w, channels):
    noisy, albedo, normals = inputs(h, w, channels, seed=h * 1000 + w + channels)
    out = check(mi, exp32, noisy, albedo, normals)
    if h > 1:
        assert not same_bits(out, noisy)                                              # the filter did something


@pytest.mark.parametrize("use_albedo,use_normals,denoise_alpha,channels", list(itertools.product([False, True], [False, True], [False, True], [3, 4])))
def test_bit_identical_for_every_combination_of_guides_and_alpha(mi, exp32, use_albedo, use_normals, denoise_alpha, channels):
    noisy, albedo, normals = inputs(67, 45, channels, seed=7)
    out = check(mi, exp32, noisy, albedo if use_albedo else None, normals if use_normals else None, denoise_alpha)
    if channels == 4:
        assert same_bits(out[..., 3], noisy[..., 3]) != denoise_alpha                 # copied through, or filtered


@pytest.mark.parametrize("params", [dict(iterations=8), dict(iterations=1, sigma_color=0.3), dict(iterations=3, sigma_color=7.5, sigma_normal=1.5, sigma_albedo=0.6, eps_a=0.05),
                                    dict(iterations=8, sigma_color=100.0, sigma_normal=10.0, sigma_albedo=10.0)])
def test_bit_identical_with_other_parameters(mi, exp32, params):
    """iterations=8: steps 32, 64 and 128 exceed the 67 x 45 image, the centre tap stands alone."""
    noisy, albedo, normals = inputs(67, 45, 4, seed=21)
    check(mi, exp32, noisy, albedo, normals, True, **params)


def aov_scene(mi, which, spp):
    if which == "cornell":
        d = mi.cornell_box()
        d["integrator"] = {"type": "aov", "aovs": "albedo:albedo,nn:sh_normal", "image": d["integrator"]}
        d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = 128, 72
        d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
        return mi.load_dict(d)
    xml = open(LIVER_XML).read()
    xml, n = re.subn(r'<integrator type="\$integrator">(.*?)</integrator>',
                     r'<integrator type="aov"><string name="aovs" value="albedo:albedo,nn:sh_normal"/><integrator type="$integrator" name="image">\1</integrator></integrator>', xml, flags=re.S)
    assert n == 1
    return mi.load_string(xml, os.path.dirname(LIVER_XML), integrator="volpath", spp=spp, res_width=128, res_height=72)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))          # bench.py's rmse_vs_oracle definition


@pytest.mark.parametrize("which", ["cornell", "liver"])
def test_rendered_aov_frames_bit_identical_and_closer_to_the_converged_render(mi, exp32, which):
    sc = aov_scene(mi, which, 8)
    img = mi.render(sc, spp=8, seed=1)
    names = sc.aov_channel_names()
    bmp = mi.Bitmap(img, channel_names=names)
    inner = names[0].rsplit(".", 1)[0]
    n_inner = sum(n.startswith(inner + ".") for n in names)                           # image.R/.G/.B, and .A with an rgba film (the liver's)
    noisy, albedo, normals = np.ascontiguousarray(img[..., :n_inner]), bmp.select("albedo"), bmp.select("nn")
    assert noisy.shape == (72, 128, n_inner) and n_inner == sc.film_shape()[2]
    out = check(mi, exp32, noisy, albedo, normals)
    assert same_bits(mi.denoise(img, sc), out)                                        # the convenience picks the same inputs
    # the bitmap form too; a channel prefix selects <prefix>.R/.G/.B, so its result is the colour part
    assert same_bits(mi.Denoiser((128, 72), True, True)(bmp, "albedo", "nn", None, "", "", inner).data, np.ascontiguousarray(out[..., :3]))
    ref = mi.render(sc, spp=1024, seed=2)[..., :noisy.shape[2]]
    before, after = rmse(noisy[..., :3], ref[..., :3]), rmse(out[..., :3], ref[..., :3])
    print(f"{which}: RMSE against 1024 spp: noisy {before:.5f}, denoised {after:.5f}, ratio {after / before:.3f}")
    assert after < before


def test_torch_tensors_stay_on_the_gpu_and_give_the_same_bits(mi):
    import torch
    noisy, albedo, normals = inputs(67, 45, 4, seed=3)
    dn = mi.Denoiser((45, 67), True, True, denoise_alpha=True)
    ref = dn(noisy, albedo, normals)
    tn, ta, tr = (torch.from_numpy(a).cuda() for a in (noisy, albedo, normals))
    keep = tn.clone()
    out = dn(tn, ta, tr)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.device == tn.device and out.dtype == torch.float32
    assert out.data_ptr() != tn.data_ptr() and torch.equal(tn, keep)                  # the input is unchanged
    assert same_bits(out.cpu().numpy(), ref)
    with pytest.raises(RuntimeError, match="float32 tensor on"):
        dn(tn, ta.cpu(), tr)


def test_nan_rule_on_the_device(mi, exp32):
    noisy, albedo, normals = inputs(80, 90, 4, seed=9)
    noisy[40, 40, 2] = np.nan; noisy[10, 70, 0] = -np.inf; albedo[60, 20, 0] = np.nan; normals[70, 80, 1] = np.inf; noisy[5, 5, 3] = np.nan
    for alpha in (False, True):
        out = check(mi, exp32, noisy, albedo, normals, alpha, sigma_color=5.0)
        bad = ~np.isfinite(out).all(axis=2)
        expect = np.zeros((80, 90), bool); expect[40, 40] = expect[10, 70] = expect[5, 5] = True     # (an alpha NaN is copied through either way)
        assert (bad == expect).all()
        for p in ((40, 40), (10, 70), (60, 20), (70, 80)) + (((5, 5),) if alpha else ()):
            assert (out[p].view(np.uint32) == noisy[p].view(np.uint32)).all()         # unfiltered pixels: the input, bit for bit


def test_error_statuses(mi):
    from liverrenderer_amd import _lib
    L = _lib.lib()
    noisy, albedo, normals = inputs(20, 30, 3, seed=1)
    dn = mi.Denoiser((30, 20), albedo=True)
    with pytest.raises(RuntimeError, match="shape"):
        dn(noisy[:, :29], albedo[:, :29])
    with pytest.raises(RuntimeError, match="shape"):
        dn(noisy, albedo[..., :2])
    out = np.empty_like(noisy)
    st = L.lrt_denoise(dn._h, noisy.ctypes.data, 3, None, None, out.ctypes.data, 0)
    assert st == 1 and "no albedo was given" in L.lrt_last_error().decode()
    st = L.lrt_denoise(dn._h, noisy.ctypes.data, 3, albedo.ctypes.data, normals.ctypes.data, out.ctypes.data, 0)
    assert st == 1 and "without the normals guide" in L.lrt_last_error().decode()
    st = L.lrt_denoise(dn._h, noisy.ctypes.data, 5, albedo.ctypes.data, None, out.ctypes.data, 0)
    assert st == 1 and "channels" in L.lrt_last_error().decode()
    with pytest.raises(RuntimeError, match="no albedo"):
        dn(noisy)
    with pytest.raises(RuntimeError, match="without the albedo guide"):
        mi.Denoiser((30, 20))(noisy, albedo)
    with pytest.raises(RuntimeError, match="device"):
        mi.Denoiser((30, 20), device=4096)
    assert (dn(noisy, albedo) == dn(noisy, albedo)).all()                             # still usable after the errors


def test_two_denoisers_alive_and_reuse_leaks_no_state(mi, exp32):
    a_in, b_in = inputs(33, 150, 4, seed=4), inputs(120, 64, 3, seed=5)
    a = mi.Denoiser((150, 33), True, True, denoise_alpha=True)
    b = mi.Denoiser((64, 120), True, True)
    a1 = a(*a_in); b1 = b(*b_in)
    other = inputs(33, 150, 3, seed=6)
    other[0][10, 10] = np.nan
    a(*other)                                                                         # another image (and a marked pixel) through the same workspace
    a2 = a(*a_in); b2 = b(*b_in)
    assert same_bits(a1, a2) and same_bits(b1, b2)
    assert same_bits(a1, R.denoise_f32(exp32, *a_in, True, **a.params)) and same_bits(b1, R.denoise_f32(exp32, *b_in, False, **b.params))
