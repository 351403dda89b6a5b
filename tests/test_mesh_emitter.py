"""CPU tests of area emitters on triangle meshes: obj and cube emitters load (alone and beside rectangle, point and environment
emitters, through XML, load_dict and lrt_scene_from_desc); the rejected cases keep their errors; and the numpy restatement
(mesh_emitter_ref.py) is consistent with itself and with the reference's own checks (test_area.py::test04_sample_direction:
the sampled pdf equals the pdf of the sampled point) and with a chi-square test of the face search against the area pmf."""
import os

import numpy as np
import pytest

import mesh_emitter_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVMAP = os.path.join(ROOT, "scenes", "assets", "cavidade_latitude.exr")

TRI = [(-1.0, 2.0, -1.0), (1.0, 2.0, -1.0), (0.0, 2.0, 1.0)]


def _tri_obj(tmp_path, name="tri.obj", verts=TRI, faces=((0, 2, 1),), normals=None):
    return mr.write_obj(tmp_path / name, verts, faces, normals)


def _emitter_kinds(sc):
    pos, nrm, faces, shapes, emitters = mr.scene_arrays(sc)
    return [(e.type, shapes[e.shape].kind if e.type == 0 else None) for e in emitters]


def test_obj_emitter_loads(mi, tmp_path):
    sc = mi.load_string(mr.scene_xml(mr.obj_xml(_tri_obj(tmp_path), radiance="2, 3, 4")))
    assert _emitter_kinds(sc) == [(0, 0)]
    e = sc.desc.emitters[0]
    assert list(e.radiance) == [2.0, 3.0, 4.0] and sc.desc.shapes[e.shape].emitter == 0


def test_cube_emitter_loads_beside_other_emitters(mi, tmp_path):
    cube = '<shape type="cube"><boolean name="flip_normals" value="true"/><emitter type="area"><rgb name="radiance" value="1"/></emitter></shape>'
    rect = ('<shape type="rectangle"><transform name="to_world"><translate y="-0.5"/></transform>'
            '<emitter type="area"><rgb name="radiance" value="5"/></emitter></shape>')
    point = '<emitter type="point"><point name="position" x="0" y="0.5" z="0"/><rgb name="intensity" value="3"/></emitter>'
    env = f'<emitter type="envmap"><string name="filename" value="{ENVMAP}"/></emitter>'
    obj = mr.obj_xml(_tri_obj(tmp_path))
    assert _emitter_kinds(mi.load_string(mr.scene_xml(cube))) == [(0, 0)]
    assert _emitter_kinds(mi.load_string(mr.scene_xml(cube + rect))) == [(0, 0), (0, 1)]
    assert _emitter_kinds(mi.load_string(mr.scene_xml(obj + cube, point))) == [(0, 0), (0, 0), (3, None)]
    assert _emitter_kinds(mi.load_string(mr.scene_xml(rect + obj, env))) == [(0, 1), (0, 0), (1, None)]


def test_load_dict_obj_and_cube_emitters(mi, tmp_path):
    path = _tri_obj(tmp_path)
    d = {"type": "scene", "integrator": {"type": "volpath", "max_depth": 4},
         "sensor": {"type": "perspective", "film": {"type": "hdrfilm", "width": 8, "height": 8}},
         "light": {"type": "obj", "filename": path, "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [1.0, 2.0, 3.0]}}},
         "box": {"type": "cube", "to_world": mi.ScalarTransform4f().scale([0.2, 0.2, 0.2]), "emitter": {"type": "area"}}}
    sc = mi.load_dict(d)
    assert _emitter_kinds(sc) == [(0, 0), (0, 0)]
    assert list(sc.desc.emitters[0].radiance) == [1.0, 2.0, 3.0] and list(sc.desc.emitters[1].radiance) == [1.0, 1.0, 1.0]


def test_scene_from_desc_accepts_a_mesh_area_emitter(mi):
    v = np.array(TRI, np.float32); f = np.array([[0, 2, 1]], np.uint32)
    sc = mi.scene_from_buffers(v, f, area_radiance=(1.0, 2.0, 3.0), constant_radiance=(0.1, 0.1, 0.1))
    assert _emitter_kinds(sc) == [(0, 0), (2, None)] and sc.desc.shapes[0].emitter == 0
    with pytest.raises(RuntimeError, match="no surface area"):
        mi.scene_from_buffers(np.zeros((3, 3), np.float32), f, area_radiance=(1.0, 1.0, 1.0))


def test_rejections(mi, tmp_path):
    empty = tmp_path / "empty.obj"; empty.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\n")
    with pytest.raises(RuntimeError, match="Cannot create sampling table for an empty mesh"):
        mi.load_string(mr.scene_xml(mr.obj_xml(str(empty))))
    flat = _tri_obj(tmp_path, "flat.obj", [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 0, 0)], ((0, 1, 2), (0, 3, 1)))
    with pytest.raises(RuntimeError, match="no surface area"):
        mi.load_string(mr.scene_xml(mr.obj_xml(flat).replace('<shape type="obj">', '<shape type="obj" id="flat_light">')))
    with pytest.raises(RuntimeError, match="flat_light"):
        mi.load_string(mr.scene_xml(mr.obj_xml(flat).replace('<shape type="obj">', '<shape type="obj" id="flat_light">')))
    with pytest.raises(RuntimeError, match="Found a 'to_world' transformation"):
        mi.load_string(mr.scene_xml(mr.obj_xml(_tri_obj(tmp_path), emitter_extra='<transform name="to_world"><translate x="1"/></transform>')))
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath"):
        mi.load_string(mr.scene_xml(mr.obj_xml(_tri_obj(tmp_path)), integrator='<integrator type="prbvolpath"/>'))
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath"):
        mi.load_string(mr.scene_xml('<shape type="cube"><emitter type="area"/></shape>',
                                    integrator='<integrator type="aov"><string name="aovs" value="dd.y:depth"/><integrator type="prbvolpath"/></integrator>'))
    with pytest.raises(RuntimeError, match="unsupported: an area emitter on a sphere"):
        mi.load_string(mr.scene_xml('<shape type="sphere"><emitter type="area"/></shape>'))
    with pytest.raises(RuntimeError, match="only area emitters can be attached to shapes"):
        mi.load_string(mr.scene_xml('<shape type="cube"><emitter type="point"/></shape>'))


# ------------------------------------------------------------------ the restatement
def test_cdf_search_and_reuse_small_tables():
    pmf = np.array([0, 1, 0, 0, 2, 3, 0], np.float32)
    cdf = mr.cdf_sequential(pmf)
    assert list(cdf) == [0, 1, 1, 1, 3, 6, 6]
    u = np.array([0.0, 1e-7, 1 / 6 - 1e-7, 1 / 6 + 1e-7, 0.4, 0.5 + 1e-7, 0.999999], np.float32)
    idx = mr.search(cdf, cdf[-1], u)
    assert list(idx) == [1, 1, 1, 4, 4, 5, 5]                      # zero-mass faces are never chosen
    idx2, re = mr.sample_reuse(pmf, cdf, cdf[-1], u)
    assert (idx2 == idx).all() and (re >= 0).all() and (re <= 1 + 1e-6).all()
    # a single face: no trip at all, the sample passes through unchanged
    one = np.array([2.5], np.float32)
    i1, r1 = mr.sample_reuse(one, mr.cdf_sequential(one), one[0], u)
    assert (i1 == 0).all() and (r1 == u).all()


def test_face_frequencies_match_the_area_pmf():
    """chi-square of the search's face counts against the area pmf, on a mesh of unequal and zero-area faces"""
    rng = np.random.default_rng(3)
    pos = rng.normal(size=(60, 3)).astype(np.float32)
    faces = rng.integers(0, 60, size=(40, 3)).astype(np.uint32)
    faces[5] = [1, 1, 2]; faces[17] = [3, 4, 3]                      # two degenerate faces
    pmf = mr.area_table(pos, faces)
    assert pmf[5] == 0 and pmf[17] == 0 and (pmf > 0).sum() >= 30
    cdf = mr.cdf_sequential(pmf)
    n = 400000
    idx = mr.search(cdf, cdf[-1], rng.random(n).astype(np.float32))
    counts = np.bincount(idx, minlength=len(pmf))
    assert (counts[pmf == 0] == 0).all()
    expected = n * pmf.astype(np.float64) / pmf.astype(np.float64).sum()
    live = expected > 0
    chi2 = (((counts - expected) ** 2)[live] / expected[live]).sum()
    dof = live.sum() - 1
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)


def test_sampled_pdf_equals_pdf_at_the_sample():
    """test_area.py::test04_sample_direction: on a flat-normal mesh the sampled pdf equals pdf_direction of the sampled point"""
    rng = np.random.default_rng(7)
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.3], [2, 0, 0.5]], np.float32)
    faces = np.array([[0, 1, 2], [1, 3, 2], [1, 4, 3]], np.uint32)
    for flip in (False, True):
        m = mr.MeshEmitter(pos, np.zeros_like(pos), faces, 0, 3, False, flip, (1.0, 2.0, 3.0))
        ref = np.tile(np.array([0.3, 0.4, -2.0 if flip else 2.0], np.float32), (2000, 1))     # on the side the normals face
        sx, sy = rng.random(2000).astype(np.float32), rng.random(2000).astype(np.float32)
        face, p, n, d, dist, pdf, w = mr.sample_direction(m, ref, sx, sy)
        active = pdf > 0
        assert active.mean() > 0.5
        # the triangle's shading normal there is its face normal
        sh = mr.shading_normal(m, face, np.zeros(2000, np.float32), np.zeros(2000, np.float32))
        assert np.abs(sh - n).max() < 1e-6
        ph = mr.pdf_hit(m, ref, p, n)
        cos = mr.dot(d, n)
        front = active & (cos < 0)
        assert np.allclose(ph[front], pdf[front], rtol=1e-5)
        assert (ph[cos >= 0] == 0).all() and (w[~front] == 0).all()
        assert np.allclose(w[front], np.array([1.0, 2.0, 3.0], np.float32) / pdf[front, None], rtol=1e-6)
        # sampled points lie on their faces
        fi = faces[face]
        e0 = pos[fi[:, 1]] - pos[fi[:, 0]]; e1 = pos[fi[:, 2]] - pos[fi[:, 0]]; r = p - pos[fi[:, 0]]
        nn = np.cross(e0, e1)
        assert np.abs((r * nn).sum(1)).max() < 1e-5


def test_uniform_area_density_and_the_triangle_warp():
    """sample_position spreads points uniformly by area: the mean of the samples is the area-weighted centroid"""
    rng = np.random.default_rng(11)
    pos = np.array([[0, 0, 0], [4, 0, 0], [0, 1, 0], [0, 0, 2], [0, 3, 2]], np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 4]], np.uint32)
    m = mr.MeshEmitter(pos, np.zeros_like(pos), faces, 0, 2, False, False, (1, 1, 1))
    n = 200000
    face, p, nrm, pdf = mr.sample_position(m, rng.random(n).astype(np.float32), rng.random(n).astype(np.float32))
    areas = np.array([2.0, 3.0])
    assert np.allclose(m.pmf, areas) and pdf[0] == np.float32(1 / 5)
    cent = (pos[faces].mean(1) * areas[:, None]).sum(0) / areas.sum()
    assert np.abs(p.mean(0) - cent).max() < 0.02
    assert abs((face == 1).mean() - 0.6) < 0.005


def test_polygon_irradiance_closed_form():
    """Lambert's formula against a float64 Monte Carlo integral of L cos(theta) over the triangle's solid angle"""
    rng = np.random.default_rng(5)
    V = np.array(TRI, np.float64)
    x = np.array([0.3, 0.0, 0.2]); N = np.array([0.0, 1.0, 0.0]); L = 2.0
    E = mr.polygon_irradiance(x, N, V, L)
    n = 400000
    a, b = rng.random(n), rng.random(n)
    t = np.sqrt(1 - a); bx, by = 1 - t, t * b
    p = V[0] + (V[1] - V[0]) * bx[:, None] + (V[2] - V[0]) * by[:, None]
    area = 0.5 * np.linalg.norm(np.cross(V[1] - V[0], V[2] - V[0]))
    r = p - x; d2 = (r * r).sum(1); w = r / np.sqrt(d2)[:, None]
    f = L * (w @ N) * np.abs(w[:, 1]) / d2 * area
    assert abs(f.mean() - E) < 4 * f.std() / np.sqrt(n)
