"""Per-voxel gradients of a heterogeneous medium's sigma_t grid on the device (Scene.render_backward(grid=True),
lrt_render_backward_grid, k_render_prb_grid): exact identities with the scalar gradient, finite differences of the device's own
primal, a Beer-Lambert closed form in float64 (grid_grad_ref.py), exact zeros, linearity, shards, selection and errors.

Grids are small and non-cubic, (res_z, res_y, res_x) = (3, 2, 2) and (3, 2, 1): an index-order mistake shows.  grad = 1 / (H W C)
unless stated.  "Absolute mass" below is sum_v |.|, the normalisation that keeps the cancellation between the real-collision
(positive) and null-collision (negative) terms from hiding a failure; 2e-3 of it is the project's float-order tolerance for sums
taken in another order (test_prb_through_heterogeneous_media)."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_grad_ref as gr
import prb_closed_form as cf
import scene_gen

pytestmark = pytest.mark.gpu

W, H = 16, 12
FLOAT_ORDER = 2e-3
SCALAR_TOL = 3e-4


def _grid(seed=1, shape=(3, 2, 2)):
    """values in [0.2, 0.9] and one voxel at 1.0: the majorant, which the finite differences never touch"""
    g = (0.2 + 0.7 * np.random.default_rng(seed).random(shape)).astype(np.float32)
    g.reshape(-1)[np.random.default_rng(seed + 100).integers(g.size)] = 1.0
    return g


def _load(mi, tmp_path, grid, xml_fn=scene_gen.het_xml, name="g.vol", spp=None, edit=None, **kw):
    vol = os.path.join(str(tmp_path), name); mi.write_volume_grid(vol, grid)
    xml = xml_fn(vol, **kw)
    if edit: xml = edit(xml)
    sc0 = mi.load_string(xml)
    return mi.load_string(scene_gen.resized(xml, W, H, spp or sc0.spp))


def _uniform(sc):
    h, w, c = sc.film_shape()
    return np.full((h, w, c), 1.0 / (h * w * c), np.float32)


def _scalars_close(a, b):
    for k in ("sigma_t", "albedo"):
        assert np.abs(a[k] - b[k]).max() <= SCALAR_TOL * max(np.abs(b[k]).max(), 1e-7), (k, a[k], b[k])
    assert abs(a["g"] - b["g"]) <= SCALAR_TOL * max(abs(b["g"]), 1e-6) + 1e-9


# ------------------------------------------------------------------------------------------------- 1. identity with d / d scale
@pytest.mark.parametrize("case", ["null", "dielectric-ld", "two-media", "one-x-voxel"])
def test_identity_with_scalar_gradient(mi, tmp_path, case):
    """sum_v grid[v] d/dgrid[v] = scale d/dscale holds for every sample: sigma_t(p) = scale sum_v w_v grid[v] is homogeneous of
    degree one in both.  And `out` is what lrt_render_backward returns."""
    grid = _grid(1, (3, 2, 1) if case == "one-x-voxel" else (3, 2, 2))
    kw = dict(seed=3)
    if case == "dielectric-ld": sc = _load(mi, tmp_path, grid, boundary="dielectric", sampler="ldsampler"); kw = dict(seed=1, rr_depth=2)
    elif case == "two-media": sc = _load(mi, tmp_path, grid, xml_fn=scene_gen.two_media_xml)
    else: sc = _load(mi, tmp_path, grid)
    grad = _uniform(sc)
    r = sc.render_backward(grad, medium=0, grid=True, **kw)
    plain = sc.render_backward(grad, medium=0, **kw)
    d = r["sigma_t_data"]
    assert d.shape == grid.shape and d.dtype == np.float32 and np.isfinite(d).all()
    scale = float(sc.param_get("smoke.scale", 1)[0])
    lhs, rhs = float((grid.astype(np.float64) * d).sum()), scale * float(plain["sigma_t"].astype(np.float64).sum())
    mass = float(np.abs(grid.astype(np.float64) * d).sum())
    print(f"\n  {case}: sum grid d_grid {lhs:.6e}  scale d/dscale {rhs:.6e}  |difference| / mass {abs(lhs - rhs) / mass:.2e}")
    assert mass > 0 and abs(lhs - rhs) <= FLOAT_ORDER * mass
    _scalars_close(r, plain)


# ------------------------------------------------------------------------------------------------- 2. finite differences per voxel
FD_SPP, FD_SEEDS, FD_H = 16384, 4, 0.02


def test_finite_differences_per_voxel(mi, tmp_path):
    """Central differences (h = 0.02) of the mean of the device's own prbvolpath primal render, per voxel, with common random numbers:
    the voxel at 1.0 is never perturbed, so the majorant and every free-flight distance stay fixed.  Seed means of d_grid[v] and of the
    differences agree within 4 standard errors of the per-seed differences (fd_s - g_s); power: that standard error is at most 10 %
    of max_v |fd_v|.  FD_SPP is the spp at which the finite differences alone meet that condition (measured: DESIGN.md section 12)."""
    grid = _grid(1)
    sc = _load(mi, tmp_path, grid, md=8, spp=FD_SPP)
    grad = _uniform(sc)
    flat = grid.reshape(-1)
    voxels = [v for v in range(grid.size) if flat[v] != 1.0]
    assert len(voxels) == grid.size - 1
    fd, g = np.zeros((FD_SEEDS, grid.size)), np.zeros((FD_SEEDS, grid.size))
    for s in range(FD_SEEDS):
        sc.param_set("smoke.sigma_t.data", grid)
        g[s] = sc.render_backward(grad, medium=0, grid=True, seed=s)["sigma_t_data"].reshape(-1)
        for v in voxels:
            val = []
            for sign in (+1, -1):
                p = flat.copy(); p[v] += sign * FD_H
                sc.param_set("smoke.sigma_t.data", p)
                assert sc.desc.media[0].grid_max == 1.0
                val.append(float(sc.render(integrator="prbvolpath", seed=s).astype(np.float64).mean()))
            fd[s, v] = (val[0] - val[1]) / (2 * FD_H)
    fd, g = fd[:, voxels], g[:, voxels]
    se = (fd - g).std(axis=0, ddof=1) / np.sqrt(FD_SEEDS)
    se_fd = fd.std(axis=0, ddof=1) / np.sqrt(FD_SEEDS)
    dev = np.abs(fd.mean(0) - g.mean(0))
    top = np.abs(fd.mean(0)).max()
    print(f"\n  spp {FD_SPP}: max|fd| {top:.4e}; SE(fd - g) / max|fd|: max {se.max() / top:.3f}; SE(fd) / max|fd|: max {se_fd.max() / top:.3f}; "
          f"deviation / SE: max {(dev / se).max():.2f}")
    for v, a, b, e in zip(voxels, fd.mean(0), g.mean(0), se): print(f"    voxel {v:2d}: fd {a:+.5e}  d_grid {b:+.5e}  SE {e:.2e}")
    assert (se <= 0.10 * top).all(), "no power: raise FD_SPP"
    assert (dev <= 4 * se).all()


# ------------------------------------------------------------------------------------------------- 3. Beer-Lambert closed form
BL_CAM = dict(origin=(0.0, 0.0, -100.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=1.0)     # half width at z = 1: 101 tan(0.5 deg) = 0.88 < 1
BL_SCALE, BL_SPP, BL_SEEDS = 1.5, 65536, 8


def _beer_lambert_xml(vol):
    c = BL_CAM
    return f"""<scene version="3.0.0">
  <integrator type="prbvolpath"><integer name="max_depth" value="4"/></integrator>
  <sensor type="perspective"><float name="fov" value="{c['fov']}"/>
    <transform name="to_world"><lookat origin="{', '.join(map(str, c['origin']))}" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="independent"><integer name="sample_count" value="{BL_SPP}"/></sampler>
    <film type="hdrfilm"><integer name="width" value="2"/><integer name="height" value="2"/><rfilter type="box"/></film>
  </sensor>
  <medium type="heterogeneous" id="smoke">
    <volume name="sigma_t" type="gridvolume"><string name="filename" value="{vol}"/>
      <transform name="to_world"><scale value="2"/><translate x="-1" y="-1" z="-1"/></transform></volume>
    <rgb name="albedo" value="0, 0, 0"/><float name="scale" value="{BL_SCALE}"/></medium>
  <shape type="cube"><bsdf type="null"/><ref name="interior" id="smoke"/></shape>
  <emitter type="constant"><rgb name="radiance" value="1, 1, 1"/></emitter>
</scene>"""


def test_beer_lambert_closed_form(mi, tmp_path):
    """A pure absorber in front of a constant emitter of radiance 1: pixel = footprint mean of T = exp(-scale int grid), and
    d pixel / d grid[v] = footprint mean of -scale W_v T with W_v the line integral of voxel v's trilinear weight.  Only the path's
    null-collision terms are at work (no scattering: nothing for the emitter march to carry)."""
    grid = _grid(2)
    vol = os.path.join(str(tmp_path), "bl.vol"); mi.write_volume_grid(vol, grid)
    sc = mi.load_string(_beer_lambert_xml(vol))
    c = BL_CAM; sub = 16
    o, d = cf.camera_directions(c["origin"], c["target"], c["up"], c["fov"], 2, 2, sub)              # (2, 2, sub^2, 3)
    t0, t1 = cf.box_span(o, d, (-1, -1, -1), (1, 1, 1))
    assert (t1 - t0 > 1.99).all()                                                                     # the whole film looks through the cube
    Wv = gr.line_weights(o, d.reshape(-1, 3), t0.reshape(-1), t1.reshape(-1), gr.cube_to_local(), grid.shape, n=512)
    T = np.exp(-BL_SCALE * (Wv @ grid.reshape(-1).astype(np.float64)))
    pix = T.reshape(2, 2, sub * sub).mean(-1)                                                         # (2, 2), the same in every channel
    dpix = (-BL_SCALE * Wv * T[:, None]).reshape(2, 2, sub * sub, -1).mean(2)                         # (2, 2, n_voxels)
    grad = _uniform(sc)
    expect = dpix.mean((0, 1))                                                                        # sum_pc grad_pc dpix_p = mean over pixels
    g = np.stack([sc.render_backward(grad, medium=0, grid=True, seed=s)["sigma_t_data"].reshape(-1).astype(np.float64) for s in range(BL_SEEDS)])
    img = np.stack([sc.render(seed=s).astype(np.float64) for s in range(BL_SEEDS)])
    se, dev = g.std(0, ddof=1) / np.sqrt(BL_SEEDS), np.abs(g.mean(0) - expect)
    top = np.abs(expect).max()
    print(f"\n  d_grid: max|closed form| {top:.4e}; SE / max: max {se.max() / top:.4f}; deviation / SE: max {(dev / se).max():.2f}")
    for v in range(grid.size): print(f"    voxel {v:2d}: closed form {expect[v]:+.5e}  d_grid {g.mean(0)[v]:+.5e}  SE {se[v]:.2e}")
    ise, idev = img.std(0, ddof=1) / np.sqrt(BL_SEEDS), np.abs(img.mean(0) - pix[..., None])
    print(f"  primal: pixels {pix.reshape(-1)}; SE / max: max {ise.max() / pix.max():.4f}; deviation / SE: max {(idev / ise).max():.2f}")
    assert (se <= 0.05 * top).all() and (dev <= 4 * se).all()
    assert (ise <= 0.05 * pix.max()).all() and (idev <= 4 * ise).all()


# ------------------------------------------------------------------------------------------------- 4. exact zeros
def test_voxels_without_support_stay_exactly_zero(mi, tmp_path):
    """The volume's to_world stretches an 8-voxel-wide grid to [-1, 3] in x while the medium exists only inside the cube [-1, 1]^3:
    lookups reach x corners 0 .. 4, so the voxels with x index 5, 6, 7 receive no add at all and keep the zero of the memset."""
    grid = _grid(3, (3, 2, 8))
    stretch = lambda xml: xml.replace('<scale value="2"/><translate x="-1" y="-1" z="-1"/>', '<scale x="4" y="2" z="2"/><translate x="-1" y="-1" z="-1"/>')
    sc = _load(mi, tmp_path, grid, edit=stretch)
    assert list(sc.desc.media[0].grid_bbox_max) == [3.0, 1.0, 1.0]
    d = sc.render_backward(_uniform(sc), medium=0, grid=True, seed=3)["sigma_t_data"]
    assert d.shape == (3, 2, 8)
    assert (d[:, :, 5:] == 0.0).all() and not np.signbit(d[:, :, 5:]).any()
    assert (d[:, :, :4] != 0.0).any() and (d[:, :, :5] != 0.0).sum() >= 12


# ------------------------------------------------------------------------------------------------- 5. linearity and shards
def test_linearity_and_shards(mi, tmp_path):
    grid = _grid(1)
    sc = _load(mi, tmp_path, grid)
    h, w, c = sc.film_shape()
    rng = np.random.default_rng(11)
    ga, gb = (rng.random((h, w, c)).astype(np.float32) / (h * w * c) for _ in range(2))
    run = lambda grad, **kw: sc.render_backward(grad, medium=0, grid=True, seed=3, **kw)["sigma_t_data"].astype(np.float64)
    da, db, dab = run(ga), run(gb), run(ga + 2 * gb)
    mass = np.abs(da + 2 * db).sum()
    print(f"\n  linearity: |difference| / mass {np.abs(dab - (da + 2 * db)).sum() / mass:.2e}")
    assert mass > 0 and np.abs(dab - (da + 2 * db)).sum() <= FLOAT_ORDER * mass
    # shards own whole 32 x 32 tiles: a 40 x 36 film has four, two per shard
    vol = os.path.join(str(tmp_path), "g.vol")
    big = mi.load_string(scene_gen.resized(scene_gen.het_xml(vol), 40, 36, 8))
    gs = rng.random(big.film_shape()).astype(np.float32) / np.prod(big.film_shape())
    runb = lambda **kw: big.render_backward(gs, medium=0, grid=True, seed=3, **kw)
    full, parts = runb(), [runb(tile_rank=r, tile_count=2) for r in (0, 1)]
    df, dp = full["sigma_t_data"].astype(np.float64), [p["sigma_t_data"].astype(np.float64) for p in parts]
    print(f"  shards: |difference| / mass {np.abs(dp[0] + dp[1] - df).sum() / np.abs(df).sum():.2e}")
    assert np.abs(dp[0]).sum() > 0 and np.abs(dp[1]).sum() > 0
    assert np.abs(dp[0] + dp[1] - df).sum() <= FLOAT_ORDER * np.abs(df).sum()
    for k in ("sigma_t", "albedo"):
        assert np.allclose(parts[0][k] + parts[1][k], full[k], rtol=FLOAT_ORDER, atol=1e-7)


# ------------------------------------------------------------------------------------------------- 6. selection and errors
def _status(mi, sc, grad, medium, n):
    out, d = mi._lib.ParamGrads(), np.full(n, 7.0, np.float32)
    o = mi._lib.make_opts(grad_medium=medium)
    st = mi._lib.lib().lrt_render_backward_grid(sc._h, C.byref(o), grad.ctypes.data, C.byref(out), d.ctypes.data)
    return st, mi._lib.lib().lrt_last_error().decode(), d


def test_selection_and_errors(mi, tmp_path):
    grid = _grid(1)
    sc = _load(mi, tmp_path, grid, xml_fn=scene_gen.two_media_xml)
    grad = _uniform(sc)
    for m in (1, -1, 2):                                     # the homogeneous medium, "all media", no medium at all
        st, msg, d = _status(mi, sc, grad, m, grid.size)
        assert st == mi._lib.INVALID and "not a heterogeneous medium" in msg and (d == 7.0).all(), (m, st, msg)
    with pytest.raises(RuntimeError, match="not a heterogeneous medium"):
        sc.render_backward(grad, medium=1, grid=True)
    picked = sc.render_backward(grad, grid=True, seed=3)["sigma_t_data"]             # the scene's only heterogeneous medium
    named = sc.render_backward(grad, medium=0, grid=True, seed=3)["sigma_t_data"]
    assert np.abs(picked.astype(np.float64) - named).sum() <= FLOAT_ORDER * np.abs(named).sum() and np.abs(named).sum() > 0
    fog = mi.load_string(scene_gen.resized(scene_gen.fog_xml(md="6", rf="box"), W, H, 4))
    with pytest.raises(RuntimeError, match="0 heterogeneous media"):
        fog.render_backward(_uniform(fog), grid=True)
    with pytest.raises(TypeError):
        sc.render_backward(grad, medium=0, out=np.zeros(grid.shape, np.float32))
    moment = lambda xml: xml.replace('<integrator type="volpath"><integer name="max_depth" value="12"/></integrator>',
                                     '<integrator type="moment"><integrator type="volpath" name="img"><integer name="max_depth" value="12"/></integrator></integrator>')
    ms = _load(mi, tmp_path, grid, edit=moment, spp=4)
    assert ms.is_moment()
    st, msg, _ = _status(mi, ms, _uniform(ms)[..., :3].copy(), 0, grid.size)
    assert st == mi._lib.UNSUPPORTED and "moment" in msg, (st, msg)
    import torch
    out = torch.full(grid.shape, 7.0, dtype=torch.float32, device="cuda")
    r = sc.render_backward(grad, medium=0, grid=True, seed=3, out=out)
    assert r["sigma_t_data"] is out
    dev = out.cpu().numpy().astype(np.float64)
    assert np.abs(dev - named).sum() <= FLOAT_ORDER * np.abs(named).sum()
    r2 = sc.render_backward(torch.from_numpy(grad).cuda(), medium=0, grid=True, seed=3, out=out)     # grad image on the device too, out overwritten
    assert np.abs(out.cpu().numpy().astype(np.float64) - named).sum() <= FLOAT_ORDER * np.abs(named).sum()
    _scalars_close(r2, r)
    with pytest.raises(RuntimeError, match="contiguous float32 CUDA tensor"):
        sc.render_backward(grad, medium=0, grid=True, out=torch.zeros((2, 2, 3), dtype=torch.float32, device="cuda"))


# ------------------------------------------------------------------------------------------------- 7. the sampler is untouched
def test_sampler_untouched_and_plain_backward_unchanged(mi, orc, tmp_path):
    """The second emitter march runs on a copy of the sampler: the lanes' own streams, and with them every later draw of the adjoint,
    are those of lrt_render_backward (its seven numbers still match the oracle's), and nothing the call leaves behind changes a
    forward render: all of its lanes are bit-identical before and after."""
    grid = _grid(1)
    sc = _load(mi, tmp_path, grid, md=8)
    o = orc.OrcScene(sc)
    grad = np.random.default_rng(11).random(sc.film_shape()).astype(np.float32) / np.prod(sc.film_shape())
    h, w, _ = sc.film_shape()
    n = h * w * sc.spp
    before, img_before = sc.render_samples(0, n, seed=5), sc.render(seed=5)
    r = sc.render_backward(grad, medium=0, grid=True, seed=3)
    after, img_after = sc.render_samples(0, n, seed=5), sc.render(seed=5)
    # bit for bit where the forward render is reproducible at all: every lane's radiance.  The film sums those lanes with float atomics
    # whose order varies between any two renders, so images compare as everywhere else in the suite (test_parity_gpu.film_close)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert (np.abs(img_after - img_before) <= 8e-5 * np.maximum(np.abs(img_before).max(axis=-1, keepdims=True), 1.0)).all()
    ref = o.render_backward(grad, medium=0, seed=3)
    _scalars_close(sc.render_backward(grad, medium=0, seed=3), ref)
    _scalars_close(r, ref)
    assert np.abs(ref["sigma_t"]).max() > 0
