"""GPU tests of the `aov` integrator (src/integrators/aov.cpp): the inner images are the standalone renders bit for bit, the per-lane
AOVs match a CPU reference built from the oracle's sampler, camera and brute-force tracer plus compute_si restated in float32 numpy,
the AOV film's weights follow the lanes' jitter (pass-state carry), and a full-size C3 frame is sane."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import LIVER_XML, MULTIMESH_XML

pytestmark = pytest.mark.gpu

AOVS_ALL = "a:albedo,d:depth,p:position,u:uv,g:geo_normal,s:sh_normal,du:dp_du,dv:dp_dv,pi:prim_index,si:shape_index"


def aov_file(mi, path, aovs, nested=True, extra="", **defines):
    """A scene file of the repository with its integrator wrapped into an aov integrator (nested under the name `image`)."""
    xml = open(path).read()
    inner = r'<integrator type="$integrator" name="image">\1</integrator>' if nested else ""
    xml, n = re.subn(r'<integrator type="\$integrator">(.*?)</integrator>',
                     f'<integrator type="aov"><string name="aovs" value="{aovs}"/>{extra}{inner}</integrator>', xml, flags=re.S)
    assert n == 1
    return mi.load_string(xml, os.path.dirname(path), **defines)


def cornell_aov(mi, aovs=AOVS_ALL, size=32, spp=4, sampler="independent", rfilter="gaussian", spass=None, nested=True):
    d = mi.cornell_box()
    integ = {"type": "aov", "aovs": aovs}
    if spass:
        integ["samples_per_pass"] = spass
    if nested:
        integ["image"] = dict(d["integrator"], **({"samples_per_pass": spass} if spass else {}))
    d["integrator"] = integ
    d["sensor"]["sampler"] = {"type": sampler, "sample_count": spp}
    d["sensor"]["film"].update(width=size, height=size, rfilter={"type": rfilter})
    return mi.load_dict(d)


def plain_render(mi, sc, return_raw=False):
    """lrt_render of the scene's description (its first nested integrator alone)."""
    h, w, c = sc.film_shape()
    img = np.empty((h, w, c), np.float32); raw = np.empty((h, w, sc.raw_channels()), np.float32)
    o = mi._lib.make_opts()
    mi._lib.check(sc._lib.lrt_render(sc._h, C.byref(o), raw.ctypes.data, img.ctypes.data))
    return (img, raw) if return_raw else img


# ------------------------------------------------------------------------------------------------ CPU reference of the lanes
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _normalize(v):
    return (v / np.sqrt((v * v).sum(1, keepdims=True))).astype(np.float32)


def _coordinate_system(n):
    """include/mitsuba/core/vector.h coordinate_system (Frisvad / Duff et al.)."""
    sign = np.copysign(np.float32(1), n[:, 2]).astype(np.float32)
    a = np.float32(-1) / (sign + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    s = np.stack([n[:, 0] * n[:, 0] * a * sign + 1, b * sign, -n[:, 0] * sign], 1)
    t = np.stack([b, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], 1)
    return s.astype(np.float32), t.astype(np.float32)


def _dot(a, b):
    return (a * b).sum(1, dtype=np.float32)


def _fma(a, b, c):
    """fmaf in float32: the product of two float32 values is exact in float64, so one rounding at the end."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _tex_uv(T, uv):
    to = np.array(T.to_uv[:], np.float32)
    uv = np.atleast_2d(np.asarray(uv, np.float32))
    return _fma(to[1], uv[:, 1], _fma(to[0], uv[:, 0], to[2])), _fma(to[4], uv[:, 1], _fma(to[3], uv[:, 0], to[5]))


def _tex_eval(T, uv):
    """tex_eval of dshade.h: rgb (srgb.cpp), checkerboard (checkerboard.cpp:70-88); bitmaps are not diffuse reflectances here: 0."""
    if T.type == 0:
        return np.array(T.color0[:], np.float32)
    if T.type == 1:
        u, v = _tex_uv(T, uv)
        mx, my = (u - np.floor(u)) > 0.5, (v - np.floor(v)) > 0.5
        return np.array(T.color0[:] if mx[0] == my[0] else T.color1[:], np.float32)
    return np.zeros(3, np.float32)


def _tex_eval_1_grad(T, uv):
    """Bitmap::eval_1_grad (src/textures/bitmap.cpp:509-578): bilinear, repeat, on the per-texel luminance
    r * 0.212671 + g * 0.715160 + b * 0.072169 (bitmap.cpp:540-552) of the description's texels."""
    w, h = T.width, T.height
    px = np.ctypeslib.as_array(T.data, (w * h * T.channels,)).reshape(h * w, T.channels).astype(np.float32)
    lum = px[:, 0] if T.channels == 1 else (px[:, 0] * np.float32(0.212671) + px[:, 1] * np.float32(0.715160)) + px[:, 2] * np.float32(0.072169)
    u, v = _tex_uv(T, uv)
    fx, fy = _fma(u, np.float32(w), np.float32(-0.5)), _fma(v, np.float32(h), np.float32(-0.5))
    ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    w1x, w1y = fx - ix.astype(np.float32), fy - iy.astype(np.float32)
    w0x, w0y = np.float32(1) - w1x, np.float32(1) - w1y
    x0, x1, y0, y1 = ix % w, (ix + 1) % w, iy % h, (iy + 1) % h
    f00, f10, f01, f11 = lum[y0 * w + x0], lum[y0 * w + x1], lum[y1 * w + x0], lum[y1 * w + x1]
    dx = _fma(w0y, f10 - f00, w1y * (f11 - f01)); dy = _fma(w0x, f01 - f00, w1x * (f11 - f10))
    to = np.array(T.to_uv[:], np.float32)
    du = to[0] * dx + to[3] * dy; dv = to[1] * dx + to[4] * dy
    return np.stack([np.float32(w) * du, np.float32(h) * dv], 1)


def reference_lanes(mi, orc, sc, lane_begin, n):
    """Pass-0 AOV values of lanes [lane_begin, lane_begin + n): jitter from orc_lane_stream / orc_ld_sample, the camera ray from
    orc_sample_ray, the hit from orc_trace(brute_force), then compute_si (src/render/mesh.cpp:1489-1659) in float32.  Returns a dict of
    per-type arrays and the hit mask."""
    d = sc.desc; F = d.film
    O = orc.OrcScene(sc); L = orc.lib()
    spp = d.sample_count
    lanes = np.arange(lane_begin, lane_begin + n, dtype=np.uint64)
    jit = np.empty((n, 2), np.float32); out = (C.c_float * 2)()
    for k, lane in enumerate(lanes):
        lane = int(lane)
        if d.sampler_type == 1:                      # ld: scramble TEA(base, spp * pixel + seed), index lane % spp (sampler.cpp:97-117)
            v0, v1 = C.c_uint32(), C.c_uint32()
            L.orc_tea32(d.sampler_seed, spp * (lane // spp), 4, C.byref(v0), C.byref(v1))
            L.orc_ld_sample(spp, v0.value, lane % spp, 0, 1, out)
        else:
            L.orc_lane_stream(d.sampler_seed, 0, lane, 2, out)
        jit[k] = out[0], out[1]
    pix = (lanes // np.uint64(spp)).astype(np.int64)
    px = (pix % F.crop_width + F.crop_offset_x).astype(np.float32); py = (pix // F.crop_width + F.crop_offset_y).astype(np.float32)
    sclx, scly = np.float32(1) / np.float32(F.crop_width), np.float32(1) / np.float32(F.crop_height)
    offx, offy = -np.float32(F.crop_offset_x) * sclx, -np.float32(F.crop_offset_y) * scly
    spx, spy = px + jit[:, 0], py + jit[:, 1]
    ax = (spx.astype(np.float64) * sclx + offx).astype(np.float32); ay = (spy.astype(np.float64) * scly + offy).astype(np.float32)   # one rounding: fma
    o = np.empty((n, 3), np.float32); dr = np.empty((n, 3), np.float32); mt = np.empty(n, np.float32)
    for k in range(n):
        o[k], dr[k], mt[k] = O.sample_ray(float(ax[k]), float(ay[k]))
    t, u, v, prim = O.trace(o, dr, mt, brute_force=True)
    valid = prim != 0xffffffff
    nv, nf = d.n_vertices, d.n_faces
    P = np.ctypeslib.as_array(d.positions, (nv * 3,)).reshape(-1, 3)
    N = np.ctypeslib.as_array(d.normals, (nv * 3,)).reshape(-1, 3)
    T = np.ctypeslib.as_array(d.texcoords, (nv * 2,)).reshape(-1, 2)
    Fc = np.ctypeslib.as_array(d.faces, (nf * 3,)).reshape(-1, 3)
    FS = np.ctypeslib.as_array(d.face_shape, (nf,))
    f = np.where(valid, prim, 0).astype(np.int64)
    shape = FS[f].astype(np.int64)
    sh = [d.shapes[i] for i in range(d.n_shapes)]
    has_n = np.array([s.has_normals for s in sh], bool)[shape]; has_t = np.array([s.has_texcoords for s in sh], bool)[shape]
    flip = np.array([s.flip_normals for s in sh], bool)[shape]; first = np.array([s.first_face for s in sh], np.int64)[shape]
    rect = np.array([s.kind == 1 for s in sh], bool)[shape]; bsdf = np.array([s.bsdf for s in sh], np.int64)[shape]
    i0, i1, i2 = Fc[f, 0], Fc[f, 1], Fc[f, 2]
    b1, b2 = u.astype(np.float32), v.astype(np.float32); b0 = np.float32(1) - b1 - b2
    p0, p1, p2 = P[i0], P[i1], P[i2]
    p = p0 * b0[:, None] + p1 * b1[:, None] + p2 * b2[:, None]
    dp0, dp1 = p1 - p0, p2 - p0
    ng = _normalize(_cross(dp0, dp1))
    dpdu, dpdv = _coordinate_system(ng)
    uv = np.stack([b1, b2], 1)
    t0, t1, t2 = T[i0], T[i1], T[i2]
    uvt = t2 * b2[:, None] + t1 * b1[:, None] + t0 * b0[:, None]
    duv0, duv1 = t1 - t0, t2 - t0
    det = duv0[:, 0] * duv1[:, 1] - duv0[:, 1] * duv1[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float32(1) / det
        du_t = (duv1[:, 1:2] * dp0 - duv0[:, 1:2] * dp1) * inv[:, None]
        dv_t = (-duv1[:, 0:1] * dp0 + duv0[:, 0:1] * dp1) * inv[:, None]
    use = has_t & (det != 0)
    uv = np.where(has_t[:, None], uvt, uv)
    dpdu = np.where(use[:, None], du_t, dpdu); dpdv = np.where(use[:, None], dv_t, dpdv)
    ni = N[i2] * b2[:, None] + N[i1] * b1[:, None] + N[i0] * b0[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        shn = np.where(has_n[:, None], _normalize(ni), ng)
    ng = np.where(flip[:, None], -ng, ng); shn = np.where(flip[:, None], -shn, shn)
    # the shading frame and wi (interaction.h:290-300, 516-536)
    shs = _normalize(dpdu - shn * _dot(shn, dpdu)[:, None])
    zero_du = (dpdu == 0).all(1)
    shs = np.where(zero_du[:, None], _coordinate_system(shn)[0], shs)
    sht = _cross(shn, shs)
    md = -dr
    wi = np.stack([_dot(md, shs), _dot(md, sht), _dot(md, shn)], 1)
    # albedo: eval_diffuse_reflectance (diffuse.cpp:181 through tex_eval; bumpmap: the nested BSDF, bumpmap.cpp:259; else 0)
    alb = np.zeros((n, 3), np.float32)
    for k in range(n):
        if not valid[k]:
            continue
        B = d.bsdfs[int(bsdf[k])]
        if B.type == 2:
            B = d.bsdfs[B.nested]
        if B.type == 0:
            alb[k] = _tex_eval(d.textures[B.reflectance], uv[k])
    # sh_normal through a bumpmap: BumpMap::sh_frame (bumpmap.cpp:224-257), its normal left in the old shading frame's local coordinates
    bump = np.array([d.bsdfs[int(b)].type == 2 for b in bsdf], bool) & valid
    shn_out = shn.copy(); borderline = np.zeros(n, bool)
    for bi in np.unique(bsdf[bump]):
        B = d.bsdfs[int(bi)]
        m = bump & (bsdf == bi)
        g = _tex_eval_1_grad(d.textures[B.texture], uv[m])
        gx, gy = np.float32(B.scale) * g[:, 0], np.float32(B.scale) * g[:, 1]
        sn, du, dv = shn[m], dpdu[m], dpdv[m]
        pdu = sn * (gx - _dot(sn, du))[:, None] + du
        pdv = sn * (gy - _dot(sn, dv))[:, None] + dv
        nb = _normalize(_cross(pdu, pdv))
        side = _dot(ng[m], nb)
        nb = np.where((side < 0)[:, None], -nb, nb)
        nl = np.stack([_dot(nb, shs[m]), _dot(nb, sht[m]), _dot(nb, sn)], 1)          # si.to_local, never converted back
        w = wi[m]
        test = w[:, 2] * _dot(w, nl)
        nl = np.where((test <= 0)[:, None], nl * np.float32([-1, -1, 1]), nl)         # m_flip_invalid_normals (bumpmap.cpp:242-246)
        shn_out[m] = nl
        # lanes whose two sign tests sit within rounding of zero may take the other branch on the device (fma vs. numpy)
        borderline[np.where(m)[0]] = (np.abs(side) < 1e-5) | (np.abs(test) < 1e-5)
    z = lambda a: np.where(valid.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0).astype(np.float32)
    return dict(valid=valid, bump=bump, borderline=borderline, albedo=z(alb), depth=z(t.astype(np.float32))[:, None], position=z(p), uv=z(uv),
                geo_normal=z(ng), sh_normal=z(shn_out), dp_du=z(dpdu), dp_dv=z(dpdv),
                prim_index=np.where(valid & ~rect, (prim.astype(np.int64) - first), 0).astype(np.float32)[:, None],
                shape_index=np.where(valid, shape + 1, 0).astype(np.float32)[:, None], spx=spx, spy=spy)


def split(vals, names):
    """(n, n_aov_channels) -> {aov name: (n, width)} following the channel names."""
    out, k = {}, 0
    for nm in names:
        base = nm.rsplit(".", 1)[0]
        out.setdefault(base, []).append(vals[:, k]); k += 1
    return {b: np.stack(v, 1) for b, v in out.items()}


def check_lanes(mi, orc, sc, lane_begin, n, bump_scene=False):
    names = sc.aov_channel_names()[sc.aov_desc().n_channels - sc.aov_desc().n_aov_channels:]
    got = split(sc.render_aov_samples(lane_begin, n), names)
    ref = reference_lanes(mi, orc, sc, lane_begin, n)
    valid = ref["valid"]
    assert valid.any() and np.isfinite(np.concatenate(list(got.values()), 1)).all()
    key = dict(a="albedo", d="depth", p="position", u="uv", g="geo_normal", s="sh_normal", du="dp_du", dv="dp_dv", pi="prim_index", si="shape_index")
    for short, typ in key.items():
        if short not in got:
            continue
        g, r = got[short], ref[typ]
        assert np.array_equal(g[~valid], np.zeros_like(g[~valid])), f"{typ}: a miss must give zeros"
        if typ in ("prim_index", "shape_index"):
            assert np.array_equal(g, r), typ
        elif typ == "albedo":
            assert np.array_equal(g, r), typ
        elif typ == "sh_normal":
            # bumpmap: the restated bump frame (1e-4); every other BSDF: si.sh.n (1e-5)
            m = valid & ref["bump"]
            assert m.any() == bump_scene, typ
            if m.any():
                keep = m & ~ref["borderline"]
                assert keep.sum() >= 0.999 * m.sum(), typ
                np.testing.assert_allclose(g[keep], r[keep], rtol=0, atol=1e-4, err_msg=typ + " (bumpmap)")
            np.testing.assert_allclose(g[valid & ~ref["bump"]], r[valid & ~ref["bump"]], rtol=1e-5, atol=1e-5, err_msg=typ)
        else:
            np.testing.assert_allclose(g, r, rtol=1e-5, atol=1e-5, err_msg=typ)
    return got, ref


# ------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("which", ["cornell", "liver"])
def test_inner_images_are_the_standalone_renders(mi, which):
    if which == "cornell":
        # box filter and 1 spp: one float atomic per pixel, so the film does not depend on the order in which paths retire (with an
        # area emitter they retire in different waves; two plain renders at several spp differ in the last bits: see the next test)
        sc = cornell_aov(mi, aovs="d:depth,n:sh_normal", size=48, spp=1, rfilter="box")
        plain = mi.load_dict(dict(mi.cornell_box(), sensor=dict(mi.cornell_box()["sensor"], sampler={"type": "independent", "sample_count": 1},
                                                                 film=dict(mi.cornell_box()["sensor"]["film"], width=48, height=48, rfilter={"type": "box"}))))
    else:                                              # volpath, rgba film
        sc = aov_file(mi, LIVER_XML, "d:depth,n:sh_normal", integrator="volpath", spp=4, res_width=64, res_height=36)
        plain = mi.load_file(LIVER_XML, integrator="volpath", spp=4, res_width=64, res_height=36)
    img = mi.render(sc)
    ref = mi.render(plain)
    c = ref.shape[2]
    assert img.shape == ref.shape[:2] + (c + 4,)
    assert np.array_equal(img[..., :c].view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(plain_render(mi, sc).view(np.uint32), ref.view(np.uint32))        # lrt_render on the aov scene: the nested integrator


def test_inner_image_cornell_gaussian(mi):
    """Several spp and the Gaussian filter: the inner image is the standalone render up to the order of the film's float atomics."""
    sc = cornell_aov(mi, aovs="d:depth", size=48, spp=8)
    plain = mi.load_dict(dict(mi.cornell_box(), sensor=dict(mi.cornell_box()["sensor"], sampler={"type": "independent", "sample_count": 8},
                                                             film=dict(mi.cornell_box()["sensor"]["film"], width=48, height=48))))
    img, ref = mi.render(sc), mi.render(plain)
    np.testing.assert_allclose(img[..., :3], ref, rtol=1e-5, atol=1e-6)


def test_lanes_cornell(mi, orc):
    sc = cornell_aov(mi, size=24, spp=4)
    check_lanes(mi, orc, sc, 0, 24 * 24 * 4)


def test_lanes_cornell_ld_sampler(mi, orc):
    sc = cornell_aov(mi, size=16, spp=16, sampler="ldsampler")
    check_lanes(mi, orc, sc, 0, 16 * 16 * 16)


@pytest.mark.parametrize("lds", [True, False])
def test_lanes_liver(mi, orc, monkeypatch, lds):
    if not lds:
        monkeypatch.setenv("LRT_NO_LDS_BVH", "1")      # read when the device image is built: a fresh scene
    sc = aov_file(mi, LIVER_XML, AOVS_ALL, nested=False, integrator="volpath", spp=2, res_width=64, res_height=36)
    check_lanes(mi, orc, sc, 0, 64 * 36 * 2, bump_scene=True)
    assert sc.stats()["lds_resident"] == (1 if lds else 0)


def test_lanes_multimesh(mi, orc):
    sc = aov_file(mi, MULTIMESH_XML, AOVS_ALL, nested=False, spp=2, res_width=48, res_height=27)
    got, ref = check_lanes(mi, orc, sc, 0, 48 * 27 * 2)
    assert len(np.unique(ref["shape_index"])) >= 2


def test_film_weights_follow_the_carried_pass_state(mi):
    """Gaussian filter, samples_per_pass < spp, one nested integrator: W of the AOV film is the colour film's W, which depends on every
    lane's jitter in every pass."""
    sc = cornell_aov(mi, aovs="d:depth", size=24, spp=8, spass=2)
    img, raw = sc.render(return_raw=True)
    _, craw = plain_render(mi, sc, return_raw=True)
    W, cW = raw[..., -1], craw[..., -1]
    assert np.all(np.abs(W - cW) <= 1e-5 * np.maximum(cW, 1.0))
    # and not the weights of freshly seeded passes
    fresh = cornell_aov(mi, aovs="d:depth", size=24, spp=8, spass=2, nested=False)
    _, fraw = fresh.render(return_raw=True)
    assert not np.allclose(fraw[..., -1], cW, rtol=0, atol=1e-6)


def test_developed_film_matches_the_reference_lanes(mi, orc):
    size, spp = 16, 4
    sc = cornell_aov(mi, aovs="d:depth,g:geo_normal,si:shape_index", size=size, spp=spp, nested=False)
    img, raw = sc.render(return_raw=True)
    ref = reference_lanes(mi, orc, sc, 0, size * size * spp)
    O = orc.OrcScene(sc); F = sc.desc.film
    vals = np.concatenate([ref["depth"], ref["geo_normal"], ref["shape_index"], np.ones((len(ref["depth"]), 1), np.float32)], 1).astype(np.float64)
    film = np.zeros((size, size, vals.shape[1]))
    rad = 2                                           # gaussian stddev 0.5: radius 2, footprint of 5 x 5 pixels
    for k in range(len(vals)):
        sx, sy = float(ref["spx"][k]), float(ref["spy"][k])
        for y in range(int(np.floor(sy)) - rad, int(np.floor(sy)) + rad + 1):
            wy = O.rfilter_eval(np.float32(y + 0.5 - sy))
            for x in range(int(np.floor(sx)) - rad, int(np.floor(sx)) + rad + 1):
                if 0 <= x < size and 0 <= y < size:
                    film[y, x] += vals[k] * wy * O.rfilter_eval(np.float32(x + 0.5 - sx))
    np.testing.assert_allclose(raw, film, rtol=1e-4, atol=1e-5)
    W = np.where(film[..., -1:] == 0, 1, film[..., -1:])
    np.testing.assert_allclose(img, film[..., :-1] / W, rtol=1e-4, atol=1e-5)


def test_full_size_c3(mi, tmp_path):
    sc = aov_file(mi, LIVER_XML, "albedo:albedo,nn:sh_normal,dd:depth,si:shape_index", nested=False,
                  integrator="volpath", spp=512, res_width=1920, res_height=1080)
    img, raw = sc.render(return_raw=True)
    names = sc.aov_channel_names()
    assert img.shape == (1080, 1920, len(names)) and raw.shape == (1080, 1920, len(names) + 1)
    assert np.array_equal(raw[..., -1], np.full((1080, 1920), 512.0, np.float32))
    assert np.isfinite(img).all() and np.isfinite(raw).all()
    depth, si = img[..., names.index("dd.T")], img[..., names.index("si.I")]
    assert (si > 0).any() and (depth[si > 0] > 0).all()
    p = tmp_path / "liver_aov.exr"
    mi.write_exr(p, img, channel_names=names)
    from test_aov import read_exr_float
    got_names, got = read_exr_float(p)
    assert got_names == sorted(names)
    assert np.array_equal(got[..., got_names.index("dd.T")], depth)
