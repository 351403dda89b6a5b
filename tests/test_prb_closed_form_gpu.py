"""The cases of test_prb_closed_form.py on the device (Scene.render_backward, kernels_prb.h), with GPU sample counts: the seed-split SE
must be <= 1 % of every compared gradient.  Plus the device-only routes (render_backward_multi), device == oracle where no closed form
holds, and device finite differences at the reference's thresholds (test_ad_integrators.py:148-153)."""
import os

import numpy as np
import pytest

import prb_closed_form as cf
from test_prb_closed_form import (ABS_CAM, ABS_H, ABS_W, HET_SIGMA, LE, SLAB_ALBEDO, SLAB_D, SLAB_SIGMA, absorber_xml, case_absorber,
                                  case_filter, case_het, case_slab, case_zero, check, grad_image, het_slab_xml, image_estimate,
                                  seed_split, slab_xml)

pytestmark = pytest.mark.gpu

DEVICE_SE = 0.01


def _device_check(mi, xml, grad, expect, zero, spp, k=8):
    sc = mi.load_string(xml)
    assert sc.film_shape() == grad.shape
    lines = check(seed_split(sc.render_backward, grad, spp, k), expect, DEVICE_SE, zero)
    print("\n  " + "\n  ".join(lines))
    return sc


def test_chords_match_device_trace(mi):
    """The float64 camera's chords at pixel centres against the device's ray casts (first hit and the exit behind it)."""
    sc = mi.load_string(absorber_xml())
    c = ABS_CAM
    org, d = cf.camera_directions(c["origin"], c["target"], c["up"], c["fov"], ABS_W, ABS_H, 1)
    d = d[:, :, 0].reshape(-1, 3)
    ch = cf.pixel_chords(c["origin"], c["target"], c["up"], c["fov"], ABS_W, ABS_H, (-1, -1, -1), (1, 1, 1), sub=1)[..., 0].reshape(-1)
    t0, _, _, prim = sc.trace(np.broadcast_to(org, d.shape), d)
    hit = prim != 0xffffffff
    assert (hit == (ch > 0)).all() and hit.sum() > 100
    eps = 1e-3
    t1, _, _, prim1 = sc.trace(org + d[hit] * (t0[hit, None] + eps), d[hit])
    assert (prim1 != 0xffffffff).all()
    assert np.abs(t1 + eps - ch[hit]).max() <= 1e-4


@pytest.mark.parametrize("variant", ["plain", "alpha", "crop", "pixel", "spp8"])
def test_absorber_gradients_gpu(mi, variant):
    if variant == "spp8":                            # the box filter's 1/spp normalisation of delta_L at a small spp
        _device_check(mi, *case_absorber("plain"), spp=8, k=128)
    else:
        _device_check(mi, *case_absorber(variant), spp=65536 if variant == "pixel" else 8192)


@pytest.mark.parametrize("rfilter", ["tent", "gaussian"])
def test_filter_gradients_gpu(mi, rfilter):
    _device_check(mi, *case_filter(rfilter), spp=16384)


@pytest.mark.parametrize("g", [0.4, -0.3])
@pytest.mark.parametrize("sample_emitters", [True, False])
def test_single_scatter_gradients_gpu(mi, g, sample_emitters):
    sc = _device_check(mi, *case_slab(g, sample_emitters), spp=65536)
    m, se = image_estimate(lambda spp, seed: sc.render(spp=spp, seed=seed, integrator="prbvolpath"), 65536)
    L = cf.slab_single_scatter(SLAB_SIGMA, SLAB_ALBEDO, g, SLAB_D, LE)["L"]
    assert (np.abs(m - L) <= 4 * se + 1e-6).all() and (se <= 0.002 * L).all(), (m, L, se)


@pytest.mark.parametrize("ratio", [2.5, 1.25])
def test_heterogeneous_constant_grid_gradients_gpu(mi, tmp_path, ratio):
    _device_check(mi, *case_het(mi, tmp_path, ratio), spp=65536)


@pytest.mark.parametrize("which", ["albedo", "sigma_t", "het"])
def test_zero_channel_gradients_gpu(mi, tmp_path, which):
    _device_check(mi, *case_zero(mi, tmp_path, which), spp=65536)


def _device_vs_oracle(mi, orc, xml, spp=256, seed=5):
    sc = mi.load_string(xml); o = orc.OrcScene(sc)
    grad = grad_image(sc.film_shape(), seed=6)
    gg, gc = sc.render_backward(grad, spp=spp, seed=seed), o.render_backward(grad, spp=spp, seed=seed)
    for k in ("sigma_t", "albedo"):
        assert np.isfinite(gg[k]).all() and np.abs(gg[k] - gc[k]).max() <= 2e-4 * np.abs(gc[k]).max(), (k, gg[k], gc[k])
    assert np.isfinite(gg["g"]) and abs(gg["g"] - gc["g"]) <= 2e-4 * max(abs(gc["g"]), 1e-6), (gg["g"], gc["g"])
    return gg


def test_zero_sigma_t_other_channels_match_oracle(mi, orc):
    """sigma_t = (0.6, 0, 1.2): the channels next to the zero one have no closed form (hero channel 1 never samples a collision);
    device == oracle there, all outputs finite."""
    _device_vs_oracle(mi, orc, slab_xml(sigma=np.array([0.6, 0.0, 1.2])))


def test_tight_majorant_matches_oracle(mi, orc, tmp_path):
    """Majorant == density (no null collisions): the reference detaches the majorant (src/media/heterogeneous.cpp:163,174), so passing
    paths carry no d/d(scale) and sum_k d_sigma_t is biased (a documented limitation of the reference's estimator);
    only device == oracle is asserted."""
    _device_vs_oracle(mi, orc, het_slab_xml(mi, tmp_path, 0.4, 0.4))


def test_render_backward_multi_matches_closed_form(mi):
    """(f) the C-ABI multi-device route (the 7-float reduction), two shards on device 0, against the (c) closed form."""
    xml, grad, expect, zero = case_slab(0.4, True)
    sc = mi.load_string(xml)
    est = seed_split(lambda g, spp, seed: sc.render_backward_multi(g, [0, 0], spp=spp, seed=seed), grad, 65536)
    print("\n  " + "\n  ".join(check(est, expect, DEVICE_SE, zero)))


# ---- device finite differences (the oracle's FD tests in test_oracle_pins.py, at the reference's thresholds) ----
def _fd_split(sc, grad, spp, params, k=8):
    """mean and SE over k seeds of the adjoint and of central differences of the device primal with common random numbers.
    params: list of (label, key, base value array, index or None, eps)."""
    loss = lambda seed: float((sc.render(spp=spp, seed=seed, integrator="prbvolpath").astype(np.float64) * grad).sum())
    adj, fd = [], []
    for s in range(k):
        g = sc.render_backward(grad, spp=spp, seed=s)
        row_a, row_f = [], []
        for label, key, base, idx, eps in params:
            vp, vm = base.copy(), base.copy()
            if idx is None: vp += eps; vm -= eps
            else: vp[idx] += eps; vm[idx] -= eps
            sc.param_set(key, vp); lp = loss(s); sc.param_set(key, vm); lm = loss(s); sc.param_set(key, base)
            row_f.append((lp - lm) / (2 * eps))
            row_a.append(float(np.atleast_1d(g[label])[0 if idx is None else idx]) if label != "scale" else float(g["sigma_t"].sum()))
        adj.append(row_a); fd.append(row_f)
    adj, fd = np.array(adj), np.array(fd)
    return adj.mean(0), fd.mean(0), fd.std(0, ddof=1) / np.sqrt(k)


def _fd_assert(labels, adj, fd, fd_se, thr):
    """error relative to the largest FD value of the same parameter (as the oracle's FD tests); the FD's own SE must be below half the
    threshold"""
    ref = {l.split("[")[0]: max(abs(f) for m, f in zip(labels, fd) if m.split("[")[0] == l.split("[")[0]) for l in labels}
    report = [f"{l}: adjoint {a:.6g} fd {f:.6g} (SE {s:.3g}) err/scale {abs(a - f) / ref[l.split('[')[0]]:.4f}" for l, a, f, s in zip(labels, adj, fd, fd_se)]
    print("\n  " + "\n  ".join(report))
    for l, a, f, s, t in zip(labels, adj, fd, fd_se, thr):
        r = ref[l.split("[")[0]]
        assert abs(a - f) <= t * r, report
        assert s <= t / 2 * r, ("FD noise too large", report)


@pytest.mark.parametrize("case", ["null+area", "dielectric+env"])
def test_prb_gradients_match_device_finite_differences(mi, case):
    """GPU mirror of test_prb_gradients_match_finite_differences: sigma_t and g within 5 %, albedo within 2 %."""
    from test_oracle_pins import PRB_AREA, PRB_ENV, prb_scene_xml
    xml = prb_scene_xml("null", PRB_AREA) if case == "null+area" else prb_scene_xml("dielectric", PRB_ENV)
    sc = mi.load_string(xml)
    grad = grad_image(sc.film_shape(), seed=7)
    st, al = np.array([1.2, 0.7, 1.6], np.float32), np.array([0.8, 0.9, 0.6], np.float32)
    params = [("sigma_t", "fog.sigma_t.value", st, c, 0.02) for c in range(3)] + [("albedo", "fog.albedo.value", al, c, 0.02) for c in range(3)]
    params.append(("g", "fog.phase_function.g", np.array([0.4], np.float32), None, 0.02))
    adj, fd, se = _fd_split(sc, grad, 65536, params)
    labels = [f"{p[0]}[{p[3]}]" for p in params]
    thr = [0.05] * 3 + [0.02] * 3 + [0.05]
    if case == "dielectric+env":
        # d/dg is small in the refractive case (the oracle test checks it only to an absolute 0.01): sign and 4 SE only
        assert adj[6] * fd[6] > 0 and abs(adj[6] - fd[6]) <= 4 * se[6] + 1e-6, (adj[6], fd[6], se[6])
        labels, adj, fd, se, thr = labels[:6], adj[:6], fd[:6], se[:6], thr[:6]
    _fd_assert(labels, adj, fd, se, thr)


def test_prb_null_collision_gradients_match_device_finite_differences(mi, tmp_path):
    """GPU mirror of test_prb_null_collision_gradients_match_finite_differences: albedo within 2 %, g and d/d(scale) within 5 %."""
    import scene_gen
    vol = os.path.join(str(tmp_path), "smoke.vol"); mi.write_volume_grid(vol, scene_gen.smoke_grid())
    xml = scene_gen.resized(scene_gen.het_xml(vol, md=8), 12, 9, 16).replace('type="volpath"', 'type="prbvolpath"')
    sc = mi.load_string(xml)
    sc.param_set("smoke.scale", 8.0)
    grad = grad_image(sc.film_shape(), seed=8)
    al = np.array([0.9, 0.8, 0.6], np.float32)
    params = [("albedo", "smoke.albedo.value", al, c, 0.02) for c in range(3)]
    params += [("g", "smoke.phase_function.g", np.array([0.3], np.float32), None, 0.02), ("scale", "smoke.scale", np.array([8.0], np.float32), None, 0.4)]
    adj, fd, se = _fd_split(sc, grad, 32768, params)
    _fd_assert([f"{p[0]}[{p[3]}]" for p in params], adj, fd, se, [0.02] * 3 + [0.05, 0.05])
