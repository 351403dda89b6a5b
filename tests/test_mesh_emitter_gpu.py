"""GPU tests of area emitters on triangle meshes: the device's emitter sampling (lrt_emitter_probe) against the numpy restatement of
mesh_emitter_ref.py; direct light from an emissive triangle against Lambert's closed form (path and volpath); an emissive cavity
(furnace) around a diffuse cube and around an albedo-1 medium; a rectangle light against the same quad as a 2-triangle obj
through four integrators; one-sidedness; and the multi-device and aov paths."""
import numpy as np
import pytest

import mesh_emitter_ref as mr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float32).eps


def _close(a, b, k=8, scale=0.0):
    """|a - b| within k float32 ulps of the larger magnitude (or of `scale`, for vectors whose components may be near zero)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    tol = k * EPS * np.maximum(np.maximum(np.abs(a), np.abs(b)), scale)
    return np.abs(a - b) <= tol + 1e-30


def _grid_patch(n=4, seed=0):
    """A flat n x n grid in the plane y = 1.5 facing down, with perturbed vertex normals (shading normals differ from the face normal)."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-1, 1, n + 1)
    v = np.array([(x, 1.5, z) for z in xs for x in xs], np.float32)
    f = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            f += [(a, b, c), (b, d, c)]
    nrm = np.array([0.0, -1.0, 0.0]) + 0.3 * rng.normal(size=(len(v), 3)) * np.array([1, 0, 1])
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return v, np.array(f), nrm


def _probe_scenes(mi, tmp_path):
    tri = mr.write_obj(tmp_path / "tri.obj", [(-1, 1.5, -1), (1, 1.5, -1), (0, 1.5, 1.2)], [(0, 1, 2)])
    gv, gf, gn = _grid_patch()
    grid = mr.write_obj(tmp_path / "grid.obj", gv, gf, gn)
    # zero-area faces first, between and last (collinear and repeated vertices)
    zv = [(-1, 1.5, -1), (1, 1.5, -1), (0, 1.5, 1), (2, 1.5, 1), (3, 1.5, 1), (4, 1.5, 1), (2, 1.5, -1)]
    zf = [(0, 1, 1), (0, 1, 2), (3, 4, 5), (1, 6, 3), (1, 3, 2), (2, 2, 2), (4, 4, 5)]
    zero = mr.write_obj(tmp_path / "zero.obj", zv, zf)
    cube = ('<shape type="cube"><transform name="to_world"><scale x="0.8" y="0.5" z="1.2"/><rotate y="1" angle="30"/><translate y="2"/></transform>'
            '<emitter type="area"><rgb name="radiance" value="1, 2, 3"/></emitter></shape>')
    second = mr.write_obj(tmp_path / "tri2.obj", [(3, 1.2, 0), (4, 1.0, 0.5), (3.5, 1.4, 1.5)], [(0, 1, 2)])     # no ray to one passes the other
    return {
        "flat_triangle": (mr.scene_xml(mr.obj_xml(tri, "4, 5, 6")), True),
        "normals_flipped": (mr.scene_xml(mr.obj_xml(grid, "2", '<boolean name="flip_normals" value="true"/>')), False),
        "zero_area_faces": (mr.scene_xml(mr.obj_xml(zero, "3")), True),
        "cube": (mr.scene_xml(cube), True),
        "two_emitters": (mr.scene_xml(mr.obj_xml(tri, "1, 2, 3") + mr.obj_xml(second, "7")), True),
    }


def _restate(ems, ne, ref, sx, sy):
    """Scene::sample_emitter_direction over the mesh emitters: the emitter from sx (re-scaled), then the mesh's own sampling"""
    n = len(sx)
    if ne > 1:
        scaled = (sx * np.float32(ne)).astype(np.float32)
        index = np.minimum(scaled.astype(np.int64), ne - 1)
        sx = (scaled - index.astype(np.float32)).astype(np.float32)
    else:
        index = np.zeros(n, np.int64)
    out = {k: np.zeros((n, 3), np.float32) for k in ("p", "n", "d", "w")}
    out.update(dist=np.zeros(n, np.float32), pdf=np.zeros(n, np.float32), face=np.zeros(n, np.int64), index=index)
    for k, m in ems.items():
        sel = index == k
        face, p, nn, d, dist, pdf, w = mr.sample_direction(m, ref[sel], sx[sel], sy[sel])
        out["p"][sel], out["n"][sel], out["d"][sel], out["dist"][sel], out["face"][sel] = p, nn, d, dist, face
        out["pdf"][sel] = (pdf * np.float32(1.0 / ne)).astype(np.float32)
        out["w"][sel] = (w * np.float32(ne)).astype(np.float32)
    return out


PROBE_SCENES = ["flat_triangle", "normals_flipped", "zero_area_faces", "cube", "two_emitters"]


@pytest.mark.parametrize("name", PROBE_SCENES)
def test_probe_matches_the_restatement(mi, tmp_path, name):
    xml, flat = _probe_scenes(mi, tmp_path)[name]
    sc = mi.load_string(xml)
    ems, ne = mr.mesh_emitters(sc)
    assert len(ems) == ne >= 1
    rng = np.random.default_rng(100 + PROBE_SCENES.index(name))
    n = 20000
    ref = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.5, 0.8, n) if name != "normals_flipped" else rng.uniform(1.8, 3.0, n),
                    rng.uniform(-2.5, 2.5, n)], 1).astype(np.float32)
    smp = rng.random((n, 2)).astype(np.float32)
    smp[:64] = np.array([[0, 0], [0, 1 - EPS / 2], [1 - EPS / 2, 0.5]] * 21 + [[0.5, 0.5]], np.float32)     # the corners of the square
    got = sc.emitter_probe(ref, smp)
    want = _restate(ems, ne, ref, smp[:, 0].copy(), smp[:, 1].copy())
    assert (got["emitter"] == want["index"]).all()
    # the face: the restatement's face index is exact; a sample whose p lands elsewhere picked another face.  That may only happen
    # where value * sum lies within an ulp of a CDF entry (the device computes the same float32 product: expect none)
    same_face = np.all(_close(got["p"], want["p"], 16, 1.0), axis=1)
    boundary = np.zeros(n, bool)
    for k, m in ems.items():
        sel = want["index"] == k
        s = (smp[sel, 1] * m.sum).astype(np.float32)
        gap = np.abs(s[:, None].astype(np.float64) - m.cdf[None, :].astype(np.float64)).min(1)
        boundary[np.flatnonzero(sel)] = gap <= np.spacing(np.float32(m.sum))
    assert (same_face | boundary).all() and (~same_face).sum() <= max(2, n // 5000), (~same_face).sum()
    ok = same_face
    assert np.all(_close(got["n"][ok], want["n"][ok], 16, 1.0))
    assert np.all(_close(got["d"][ok], want["d"][ok], 16, 1.0))
    assert np.all(_close(got["dist"][ok], want["dist"][ok], 8))
    assert np.all(_close(got["pdf"][ok], want["pdf"][ok], 32))
    assert np.all(_close(got["weight"][ok], want["w"][ok], 32))
    active = ok & (want["pdf"] > 0) & (want["w"].max(1) > 0)
    assert active.mean() > 0.2
    active[:64] = False                  # (the corner samples land on vertices and edges: which face a ray meets there is not the question)
    # the hit: the sampled point's shape (nothing else lies in the way in these scenes), its pdf on the shading normal, emission
    pos, nrm, faces, shapes, emitters = mr.scene_arrays(sc)
    shape_of = np.array([emitters[k].shape for k in range(ne)])
    assert (got["hit_shape"][active] == shape_of[want["index"][active]]).all()
    rad = np.stack([np.asarray(list(emitters[k].radiance), np.float32) for k in range(ne)])
    assert (got["hit_le"][active] == rad[want["index"][active]]).all()
    cos = np.abs(mr.dot(got["d"], got["n"]))
    steep = active & (cos > 0.05)        # (at grazing angles the hit point's rounding moves dist^2 / |cos| by more than a few ulps)
    assert steep.sum() > 0.1 * n
    # sampling and the hit pdf read the same interpolated normal: the two pdfs of one point agree
    assert np.allclose(got["hit_pdf"][steep], got["pdf"][steep], rtol=1e-3)
    if not flat:
        t, u, v, prim = sc.trace(ref, got["d"])
        m = ems[0]
        sel = np.flatnonzero(active)
        fi = faces[prim[sel]]
        b1, b2 = u[sel], v[sel]
        b0 = ((np.float32(1) - b1).astype(np.float32) - b2).astype(np.float32)
        p0, p1, p2 = pos[fi[:, 0]], pos[fi[:, 1]], pos[fi[:, 2]]
        ph = np.stack([mr.fma(p0[:, k], b0, mr.fma(p1[:, k], b1, mr.mul(p2[:, k], b2))) for k in range(3)], 1)
        shn = mr.shading_normal(m, prim[sel] - shapes[emitters[0].shape].first_face, b1, b2)
        want_hit = (mr.pdf_hit(m, ref[sel], ph, shn) * np.float32(1.0 / ne)).astype(np.float32)
        assert np.all(_close(got["hit_pdf"][sel], want_hit, 64))
        # with the geometric normal (si.n) the hit pdf would differ: the shading normal is what the record carries
        geo = mr.normalize(mr.cross((p1 - p0).astype(np.float32), (p2 - p0).astype(np.float32)))
        geo = -geo if m.flip else geo
        with_geo = (mr.pdf_hit(m, ref[sel], ph, geo) * np.float32(1.0 / ne)).astype(np.float32)
        assert np.median(np.abs(with_geo / got["hit_pdf"][sel] - 1)) > 1e-2


# ------------------------------------------------------------------ closed forms
FLOOR = ('<shape type="rectangle"><transform name="to_world"><scale value="20"/><rotate x="1" angle="-90"/></transform>'
         '<bsdf type="diffuse"><rgb name="reflectance" value="{rho}"/></bsdf></shape>')
LIGHT = [(-0.6, 2.0, -0.3), (0.6, 2.0, -0.3), (0.0, 2.0, 0.7)]          # faces down (-y); symmetric about x = 0


def _floor_points(size, fov, sub, H):
    """World points of the floor y = 0 seen by a camera at (0, H, 0) looking down with up = +z: camera +x is world +x (film
    left), camera +y is world +z (film top).  sub x sub stratified points per pixel: (size, size, sub * sub, 3)."""
    tn = np.tan(np.radians(fov) / 2)
    o = (np.arange(sub) + 0.5) / sub
    iy, ix = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    u = (ix[..., None, None] + o[None, None, None, :]) / size
    v = (iy[..., None, None] + o[None, None, :, None]) / size
    cx, cy = (1 - 2 * u) * tn, (1 - 2 * v) * tn
    x, z = cx * H, cy * H
    x, z = np.broadcast_arrays(x, z)
    return np.stack([x, np.zeros_like(x), z], -1).reshape(size, size, sub * sub, 3)


@pytest.mark.parametrize("integrator", ["path", "volpath"])
def test_direct_light_from_a_triangle_closed_form(mi, tmp_path, integrator):
    """max_depth = 2: a diffuse floor of albedo rho under an emissive triangle, the camera between them looking down (the light is
    behind it): rho / pi * E(x) per pixel, E from Lambert's polygon formula; NEE and the BSDF-sampled hits on the light, MIS-weighted."""
    rho, L, H, size, fov, spp = 0.6, 5.0, 1.0, 24, 60.0, 256
    tri = mr.write_obj(tmp_path / "light.obj", LIGHT, [(0, 1, 2)])
    xml = mr.scene_xml(FLOOR.format(rho=rho) + mr.obj_xml(tri, L), integrator=f'<integrator type="{integrator}"><integer name="max_depth" value="2"/></integrator>',
                       cam=((0, H, 0), (0, 0, 0), (0, 0, 1)), fov=fov, size=(size, size), spp=spp)
    sc = mi.load_string(xml)
    lanes = sc.render_samples(0, size * size * spp, seed=3).astype(np.float64)[:, :3].reshape(size, size, spp, 3)
    mean, se = lanes.mean(2), lanes.std(2) / np.sqrt(spp)
    x = _floor_points(size, fov, 8, H)
    ref = (rho / np.pi * mr.polygon_irradiance(x, (0, 1, 0), LIGHT, L)).mean(-1)
    assert ref.min() > 0.05
    z = np.abs(mean - ref[..., None]) / (se + 1e-4 * ref[..., None] + 1e-6)
    assert (z ** 2).mean() < 1.5 and z.max() < 5, ((z ** 2).mean(), z.max())


def _cavity(mi, integrator, md, L, rho, inner, medium=False, size=24, spp=64):
    med = ('<medium type="homogeneous" id="fog"><rgb name="sigma_t" value="1.5"/><rgb name="albedo" value="1"/></medium>' if medium else "")
    box = ('<shape type="cube"><transform name="to_world"><scale value="2"/></transform><boolean name="flip_normals" value="true"/>'
           '<bsdf type="diffuse"><rgb name="reflectance" value="0"/></bsdf>' + ('<ref name="interior" id="fog"/>' if medium else "") +
           f'<emitter type="area"><rgb name="radiance" value="{L}"/></emitter></shape>')
    obj = (f'<shape type="cube"><transform name="to_world"><scale value="0.5"/><rotate y="1" angle="25"/></transform>'
           f'<bsdf type="diffuse"><rgb name="reflectance" value="{rho}"/></bsdf></shape>') if inner else ""
    xml = mr.scene_xml(box + obj, head=med, integrator=f'<integrator type="{integrator}"><integer name="max_depth" value="{md}"/></integrator>',
                       cam=((0.3, 0.4, -1.7), (0, 0, 0), (0, 1, 0)), fov=70, size=(size, size), spp=spp,
                       sensor_extra='<ref id="fog"/>' if medium else "")
    return mi.load_string(xml)


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
def test_emissive_cavity_furnace(mi, integrator):
    """A flipped cube emitter of radiance L (black reflectance) around a diffuse cube of albedo rho, max_depth = 2: a lane that sees
    the wall is exactly L; the object reflects rho L (it sees the emitter over its whole hemisphere)."""
    L, rho, size, spp = 2.0, 0.7, 24, 128
    sc = _cavity(mi, integrator, 2, L, rho, inner=True, size=size, spp=spp)
    lanes = sc.render_samples(0, size * size * spp, seed=5).astype(np.float64)[:, :3].reshape(size, size, spp, 3)
    wall = np.all(np.abs(lanes - L) <= 1e-6 * L, axis=-1)
    assert wall.mean() > 0.4
    px_wall, px_obj = wall.all(-1), (~wall).all(-1)
    assert px_wall.sum() > 100 and px_obj.sum() > 40
    obj = lanes[px_obj]                                                   # (pixels, spp, 3)
    mean, se = obj.mean(1), obj.std(1) / np.sqrt(spp)
    z = np.abs(mean - rho * L) / (se + 1e-6)
    assert (z ** 2).mean() < 1.5 and z.max() < 5, ((z ** 2).mean(), z.max())
    allobj = obj.reshape(-1, 3)
    assert abs(allobj.mean() - rho * L) < 4 * allobj.std() / np.sqrt(allobj.shape[0])


@pytest.mark.parametrize("integrator", ["volpath", "volpathmis"])
def test_emissive_cavity_with_a_scattering_medium(mi, integrator):
    """The same cavity filled with an index-matched albedo-1 medium, the camera inside it, max_depth high: every path ends on the
    wall, so every pixel estimates L."""
    L, size, spp = 1.5, 16, 64
    sc = _cavity(mi, integrator, 256, L, 0.0, inner=False, medium=True, size=size, spp=spp)
    lanes = sc.render_samples(0, size * size * spp, seed=8).astype(np.float64)[:, :3]
    assert np.isfinite(lanes).all()
    m, se = lanes.mean(), lanes.std() / np.sqrt(lanes.shape[0])
    assert abs(m - L) < 4 * se + 1e-3 * L, (m, se)
    assert se < 0.02 * L


# ------------------------------------------------------------------ a rectangle and the same quad as two triangles
def _tissue_scene(light, integrator, size=32, spp=64):
    """A cube of liver tissue (the medium of test_bio_gpu.py's scenes) on a diffuse floor, lit by `light` and a dim sky (biovolpath
    erases surface NEE outside a medium, biovolpath.cpp:297-300: there the light reaches the image through the tissue's NEE)"""
    coeffs = "".join(f'<float name="sigma_{k}{l}_{c}" value="{v:.4f}"/>' for k, base in (("collagen", 0.9), ("elastin", 0.5))
                     for l in range(1, 5) for c, v in zip("RGB", (base * l, base * l * 0.6 + 0.1, base * (5 - l) * 0.4)))
    limits = '<float name="layer1Limit" value="0.1"/><float name="layer2Limit" value="0.2"/><float name="layer3Limit" value="0.35"/><float name="layer4Limit" value="0.6"/>'
    return f"""<scene version="3.0.0">
  <integrator type="{integrator}"><integer name="max_depth" value="8"/></integrator>
  <medium type="liver" id="tissue">{coeffs}{limits}<rgb name="sigma_blood" value="0.3, 0.9, 1.1"/><rgb name="sigma_bile" value="0.02, 0.0, 0.3"/>
    <rgb name="sigma_lipid_water" value="0.05, 0.01, 0.2"/><float name="sigma_hepatocity" value="9.5"/>
    <boolean name="has_spectral_extinction" value="true"/><rgb name="sigma_t" value="0.4, 0.2, 0.6"/><phase type="hg"><float name="g" value="0.4"/></phase></medium>
  <sensor type="perspective"><float name="fov" value="40"/>
    <transform name="to_world"><lookat origin="3, 2.5, 4" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="independent"><integer name="sample_count" value="{spp}"/></sampler>
    <film type="hdrfilm"><integer name="width" value="{size}"/><integer name="height" value="{size}"/><rfilter type="box"/></film></sensor>
  <shape type="cube"><bsdf type="null"/><ref name="interior" id="tissue"/></shape>
  <shape type="rectangle"><transform name="to_world"><scale value="6"/><rotate x="1" angle="-90"/><translate y="-1.001"/></transform>
    <bsdf type="diffuse"><rgb name="reflectance" value="0.5"/></bsdf></shape>
  {light}
  <emitter type="constant"><rgb name="radiance" value="0.3, 0.4, 0.6"/></emitter>
</scene>"""


RECT = ('<shape type="rectangle"><transform name="to_world"><scale value="0.9"/><rotate x="1" angle="90"/><rotate z="1" angle="20"/>'
        '<translate y="3"/></transform><emitter type="area"><rgb name="radiance" value="20, 18, 15"/></emitter></shape>')


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis", "biovolpath"])
def test_rectangle_equals_two_triangles(mi, tmp_path, integrator):
    """Per 8x8 block, the quad light as a `rectangle` and as a 2-triangle obj (same world vertices and faces) give statistically equal
    images (z-scores of the block means from the per-lane spread)."""
    size, spp = 32, 64
    rect = mi.load_string(_tissue_scene(RECT, integrator, size, spp))
    pos, nrm, faces, shapes, emitters = mr.scene_arrays(rect)
    s = shapes[emitters[0].shape]
    fq = faces[s.first_face:s.first_face + s.n_faces]
    used = np.unique(fq)
    remap = {int(v): i for i, v in enumerate(used)}
    path = mr.write_obj(tmp_path / "quad.obj", pos[used], [[remap[int(v)] for v in t] for t in fq])
    mesh = mi.load_string(_tissue_scene(mr.obj_xml(path, "20, 18, 15"), integrator, size, spp))
    a = rect.render_samples(0, size * size * spp, seed=1).astype(np.float64)[:, :3].reshape(size, size, spp, 3)
    b = mesh.render_samples(0, size * size * spp, seed=2).astype(np.float64)[:, :3].reshape(size, size, spp, 3)
    assert np.isfinite(a).all() and np.isfinite(b).all() and a.mean() > 1e-3
    blk = lambda x: x.reshape(size // 8, 8, size // 8, 8, spp, 3).transpose(0, 2, 1, 3, 4, 5).reshape(size // 8, size // 8, -1, 3)
    ba, bb = blk(a), blk(b)
    n = ba.shape[2]
    se = np.sqrt(ba.var(2) / n + bb.var(2) / n) + 1e-6
    z = np.abs(ba.mean(2) - bb.mean(2)) / se
    assert (z ** 2).mean() < 1.5 and z.max() < 5, ((z ** 2).mean(), z.max())


# ------------------------------------------------------------------ one-sidedness, multi-device, aov
def test_one_sided(mi, tmp_path):
    """A triangle facing up above a floor: seen from below it is black, and NEE from the floor (behind it) finds nothing; flipped, it lights the floor."""
    up = mr.write_obj(tmp_path / "up.obj", [(-1, 1, 1), (1, 1, 1), (0, 1, -1)], [(0, 1, 2)])
    floor = FLOOR.format(rho=0.8)
    cam = ((0.5, 0.3, 3.0), (0, 0.5, 0), (0, 1, 0))
    for integrator in ("path", "volpath", "volpathmis"):
        dark = mi.load_string(mr.scene_xml(floor + mr.obj_xml(up, 10), integrator=f'<integrator type="{integrator}"/>', cam=cam, size=(24, 24), spp=16))
        img = dark.render(seed=1)
        assert (img[..., :3] == 0).all()
        lit = mi.load_string(mr.scene_xml(floor + mr.obj_xml(up, 10, '<boolean name="flip_normals" value="true"/>'),
                                          integrator=f'<integrator type="{integrator}"/>', cam=cam, size=(24, 24), spp=16))
        assert lit.render(seed=1)[..., :3].mean() > 0.05


def test_multi_device_and_aov(mi, tmp_path):
    tri = mr.write_obj(tmp_path / "light.obj", LIGHT, [(0, 1, 2)])
    xml = mr.scene_xml(FLOOR.format(rho=0.5) + mr.obj_xml(tri, 5) + '<shape type="cube"><transform name="to_world"><scale value="0.3"/><translate y="0.3"/></transform></shape>',
                       integrator='<integrator type="volpath"><integer name="max_depth" value="6"/></integrator>',
                       cam=((2, 1.5, 2), (0, 0.3, 0), (0, 1, 0)), size=(32, 24), spp=8)
    sc = mi.load_string(xml)
    img, raw = sc.render(seed=6, return_raw=True)
    imgn, rawn = sc.render_multi([0, 0], seed=6, return_raw=True)
    assert img[..., :3].mean() > 1e-3
    assert np.allclose(rawn, raw, rtol=1e-5, atol=1e-6) and np.allclose(imgn, img, rtol=2e-4, atol=1e-6)
    aov = mi.load_string(xml.replace('<integrator type="volpath"><integer name="max_depth" value="6"/></integrator>',
                                     '<integrator type="aov"><string name="aovs" value="d:depth"/>'
                                     '<integrator type="volpath" name="image"><integer name="max_depth" value="6"/></integrator></integrator>'))
    a = mi.render(aov, seed=6)
    assert a.shape == img.shape[:2] + (4,)
    np.testing.assert_allclose(a[..., :3], img[..., :3], rtol=1e-5, atol=1e-6)
    assert (a[..., 3] > 0).mean() > 0.5
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath"):
        sc.render(integrator="prbvolpath")
