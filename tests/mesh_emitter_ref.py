"""Numpy restatement of area emitters on triangle meshes for the tests: the area table (src/render/mesh.cpp:449-482 build_pmf),
the sequential float32 CDF (include/mitsuba/core/distr_1d.h:219-234), the fixed-trip binary search and sample_reuse
(distr_1d.h:117-182 with Dr.Jit's binary_search), the triangle warp and Mesh::sample_position (mesh.cpp:861-935,
include/mitsuba/core/warp.h:153-156), Shape::sample_direction (src/render/shape.cpp:344-361) with area.cpp's activity test, and
the pdf of a direction that hits the emitter on the shading normal (include/mitsuba/render/records.h:76-78,173-180,
shape.cpp:363-374).  fma is emulated through float64 (the product of two float32 values is exact there), as in sphere_ref.py.
Also a float64 closed form: Lambert's irradiance from a polygon of uniform radiance."""
import ctypes as C

import numpy as np

f32 = np.float32


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def mul(a, b):
    return (np.asarray(a, f32) * np.asarray(b, f32)).astype(f32)


def dot(a, b):
    """dmath.h / Dr.Jit dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], mul(a[..., 0], b[..., 0])))


def cross(a, b):
    """Dr.Jit cross, the fmsub form: (fma(a.y, b.z, -a.z b.y), fma(a.z, b.x, -a.x b.z), fma(a.x, b.y, -a.y b.x))."""
    return np.stack([fma(a[..., 1], b[..., 2], -mul(a[..., 2], b[..., 1])),
                     fma(a[..., 2], b[..., 0], -mul(a[..., 0], b[..., 2])),
                     fma(a[..., 0], b[..., 1], -mul(a[..., 1], b[..., 0]))], -1)


def normalize(v):
    """v * (1 / sqrt(dot(v, v))), both operations correctly rounded (dmath.h rsqrt_)."""
    with np.errstate(all="ignore"):
        inv = (f32(1) / np.sqrt(dot(v, v)).astype(f32)).astype(f32)
    return (v * inv[..., None]).astype(f32)


# ------------------------------------------------------------------ the scene as the device sees it
def scene_arrays(scene):
    """World-space positions / normals (nv x 3), faces (nf x 3), shapes and emitters (ctypes structs) of a loaded scene."""
    d = scene.desc
    nv, nf = d.n_vertices, d.n_faces
    pos = np.ctypeslib.as_array(C.cast(d.positions, C.POINTER(C.c_float)), (nv * 3,)).reshape(nv, 3).copy() if nv else np.zeros((0, 3), f32)
    nrm = np.ctypeslib.as_array(C.cast(d.normals, C.POINTER(C.c_float)), (nv * 3,)).reshape(nv, 3).copy() if nv else np.zeros((0, 3), f32)
    faces = np.ctypeslib.as_array(C.cast(d.faces, C.POINTER(C.c_uint32)), (nf * 3,)).reshape(nf, 3).copy() if nf else np.zeros((0, 3), np.uint32)
    shapes = [d.shapes[i] for i in range(d.n_shapes)]
    emitters = [d.emitters[i] for i in range(d.n_emitters)]
    return pos.astype(f32), nrm.astype(f32), faces, shapes, emitters


class MeshEmitter:
    """One area emitter on a mesh: its faces, the area table and the CDF, as device.hip builds them."""

    def __init__(self, pos, nrm, faces, first_face, n_faces, has_normals, flip_normals, radiance):
        self.pos, self.nrm = pos, nrm
        self.faces = faces[first_face:first_face + n_faces]
        self.has_normals, self.flip = bool(has_normals), bool(flip_normals)
        self.radiance = np.asarray(radiance, f32)
        self.pmf = area_table(pos, self.faces)
        self.cdf = cdf_sequential(self.pmf)
        self.sum = self.cdf[-1]
        self.normalization = (f32(1) / self.sum).astype(f32)


def mesh_emitters(scene):
    """{emitter index: MeshEmitter} for every area emitter on an LRT_SHAPE_MESH shape, and the number of emitters."""
    pos, nrm, faces, shapes, emitters = scene_arrays(scene)
    out = {}
    for k, e in enumerate(emitters):
        if e.type == 0 and shapes[e.shape].kind == 0:
            s = shapes[e.shape]
            out[k] = MeshEmitter(pos, nrm, faces, s.first_face, s.n_faces, s.has_normals, s.flip_normals, list(e.radiance))
    return out, len(emitters)


# ------------------------------------------------------------------ the table and its search
def area_table(pos, faces):
    """build_pmf: .5 * norm(cross(p1 - p0, p2 - p0)) in float32."""
    p0, p1, p2 = pos[faces[:, 0]], pos[faces[:, 1]], pos[faces[:, 2]]
    c = cross((p1 - p0).astype(f32), (p2 - p0).astype(f32))
    return (f32(0.5) * np.sqrt(dot(c, c)).astype(f32)).astype(f32)


def cdf_sequential(pmf):
    """Inclusive prefix sum, left to right in float32 (the host's scan)."""
    out = np.empty(len(pmf), f32); acc = f32(0)
    for i, v in enumerate(np.asarray(pmf, f32)):
        acc = f32(acc + v); out[i] = acc
    return out


def search(cdf, total, value):
    """DiscreteDistribution::sample in Dr.Jit's binary_search: log2i(n - 1) + 1 trips, JIT predicate
    ((cdf[m] < s) || cdf[m] == 0) && cdf[m] != sum with s = value * sum."""
    value = np.asarray(value, f32)
    n = len(cdf)
    s = (value * f32(total)).astype(f32)
    start = np.zeros(value.shape, np.int64); end = np.full(value.shape, n - 1, np.int64)
    trips = int(n - 1).bit_length() if n > 1 else 0          # log2i(n - 1) + 1
    for _ in range(trips):
        middle = (start + end) >> 1
        c = cdf[middle]
        pred = ((c < s) | (c == 0)) & (c != f32(total))
        start = np.where(pred, np.minimum(middle + 1, end), start)
        end = np.where(pred, end, middle)
    return start


def sample_reuse(pmf, cdf, total, value):
    """(index, (value - cdf[index - 1] * norm) / (pmf[index] * norm)); the cdf term is 0 at index 0."""
    value = np.asarray(value, f32)
    norm = (f32(1) / f32(total)).astype(f32)
    idx = search(cdf, total, value)
    p = (pmf[idx] * norm).astype(f32)
    c = np.where(idx > 0, (cdf[np.maximum(idx - 1, 0)] * norm).astype(f32), f32(0)).astype(f32)
    with np.errstate(all="ignore"):
        return idx, ((value - c).astype(f32) / p).astype(f32)


# ------------------------------------------------------------------ position and direction
def sample_position(m, sx, sy):
    """Mesh::sample_position: (face, p, n, pdf).  `sy` picks the face and is re-scaled; square_to_uniform_triangle on (sx, sy')."""
    sx = np.asarray(sx, f32)
    idx, sy2 = sample_reuse(m.pmf, m.cdf, m.sum, sy)
    fi = m.faces[idx]
    p0, p1, p2 = m.pos[fi[:, 0]], m.pos[fi[:, 1]], m.pos[fi[:, 2]]
    e0, e1 = (p1 - p0).astype(f32), (p2 - p0).astype(f32)
    t = np.sqrt(np.maximum((f32(1) - sx).astype(f32), f32(0))).astype(f32)
    bx, by = (f32(1) - t).astype(f32), mul(t, sy2)
    p = np.stack([fma(e0[:, k], bx, fma(e1[:, k], by, p0[:, k])) for k in range(3)], 1)
    if m.has_normals:
        n0, n1, n2 = m.nrm[fi[:, 0]], m.nrm[fi[:, 1]], m.nrm[fi[:, 2]]
        b0 = ((f32(1) - bx).astype(f32) - by).astype(f32)
        n = np.stack([fma(n0[:, k], b0, fma(n1[:, k], bx, mul(n2[:, k], by))) for k in range(3)], 1)
    else:
        n = cross(e0, e1)
    n = normalize(n)
    if m.flip:
        n = -n
    return idx, p, n, np.full(len(sx), m.normalization, f32)


def sample_direction(m, ref, sx, sy):
    """Shape::sample_direction + AreaEmitter::sample_direction: (face, p, n, d, dist, pdf, weight)."""
    ref = np.asarray(ref, f32)
    idx, p, n, pdf = sample_position(m, sx, sy)
    d = (p - ref).astype(f32)
    dist2 = dot(d, d)
    dist = np.sqrt(dist2).astype(f32)
    with np.errstate(all="ignore"):
        d = (d / dist[:, None]).astype(f32)
        cos = dot(d, n)
        x = (dist2 / np.abs(cos)).astype(f32)
        pdf = (pdf * np.where(np.isfinite(x), x, f32(0))).astype(f32)
        active = (cos < 0) & (pdf != 0)
        w = np.where(active[:, None], (m.radiance[None, :] / pdf[:, None]).astype(f32), f32(0)).astype(f32)
    return idx, p, n, d, dist, pdf, w


def pdf_hit(m, ref, p, sh_n):
    """DirectionSample(scene, si, ref) + AreaEmitter::pdf_direction: the record's normal is si.sh_frame.n."""
    ref = np.asarray(ref, f32)
    rel = (p - ref).astype(f32)
    dist = np.sqrt(dot(rel, rel)).astype(f32)
    with np.errstate(all="ignore"):
        d = (rel / dist[:, None]).astype(f32)
        dp = dot(d, sh_n)
        adp = np.abs(dp)
        v = np.where(adp != 0, (mul(dist, dist) / adp).astype(f32), f32(0))
        return np.where(dp < 0, (m.normalization * v).astype(f32), f32(0)).astype(f32)


def shading_normal(m, face, u, v):
    """The mesh's si.sh_frame.n at barycentrics (u, v) of `face` (index into the emitter's faces): compute_si's interpolation
    fma(n2, v, fma(n1, u, n0 * (1 - u - v))), normalised, flipped; the face normal without vertex normals."""
    fi = m.faces[face]
    u = np.asarray(u, f32); v = np.asarray(v, f32)
    p0, p1, p2 = m.pos[fi[:, 0]], m.pos[fi[:, 1]], m.pos[fi[:, 2]]
    if m.has_normals:
        n0, n1, n2 = m.nrm[fi[:, 0]], m.nrm[fi[:, 1]], m.nrm[fi[:, 2]]
        b0 = ((f32(1) - u).astype(f32) - v).astype(f32)
        n = np.stack([fma(n2[:, k], v, fma(n1[:, k], u, mul(n0[:, k], b0))) for k in range(3)], 1)
    else:
        n = cross((p1 - p0).astype(f32), (p2 - p0).astype(f32))
    n = normalize(n)
    return -n if m.flip else n


# ------------------------------------------------------------------ closed forms (float64)
def polygon_irradiance(x, normal, verts, radiance):
    """Lambert: E(x) = L / 2 * |sum_i Theta_i (n_i . N)| for a polygon of uniform radiance L wholly above the tangent plane of x and
    facing it.  Theta_i: angle subtended by edge i, n_i: unit normal of the plane through x and that edge.  x: (..., 3)."""
    x = np.asarray(x, np.float64); N = np.asarray(normal, np.float64)
    V = np.asarray(verts, np.float64)
    acc = np.zeros(x.shape[:-1])
    for i in range(len(V)):
        a = V[i] - x; b = V[(i + 1) % len(V)] - x
        a /= np.linalg.norm(a, axis=-1, keepdims=True); b /= np.linalg.norm(b, axis=-1, keepdims=True)
        theta = np.arccos(np.clip((a * b).sum(-1), -1, 1))
        c = np.cross(a, b); c /= np.linalg.norm(c, axis=-1, keepdims=True)
        acc += theta * (c * N).sum(-1)
    return 0.5 * radiance * np.abs(acc)


# ------------------------------------------------------------------ scenes for the tests
def write_obj(path, verts, faces, normals=None):
    """A Wavefront OBJ of triangles (0-based `faces`); `normals`: one per vertex, or None."""
    with open(path, "w") as f:
        for v in verts:
            f.write("v %r %r %r\n" % tuple(float(x) for x in v))
        if normals is not None:
            for n in normals:
                f.write("vn %r %r %r\n" % tuple(float(x) for x in n))
        for t in faces:
            if normals is not None:
                f.write("f " + " ".join(f"{i + 1}//{i + 1}" for i in t) + "\n")
            else:
                f.write("f " + " ".join(str(i + 1) for i in t) + "\n")
    return str(path)


def obj_xml(path, radiance=1.0, extra="", emitter_extra=""):
    return (f'<shape type="obj"><string name="filename" value="{path}"/>{extra}'
            f'<emitter type="area"><rgb name="radiance" value="{radiance}"/>{emitter_extra}</emitter></shape>')


def scene_xml(shapes, emitters="", integrator='<integrator type="path"/>', cam=((0, 0, -5), (0, 0, 0), (0, 1, 0)), fov=40,
              size=(16, 16), spp=4, rfilter="box", sensor_extra="", head=""):
    """`head`: objects the sensor refers to (a medium), declared before it"""
    (o, t, u) = cam
    return f"""<scene version="3.0.0">{integrator}{head}
  <sensor type="perspective"><float name="fov" value="{fov}"/>{sensor_extra}
    <transform name="to_world"><lookat origin="{o[0]}, {o[1]}, {o[2]}" target="{t[0]}, {t[1]}, {t[2]}" up="{u[0]}, {u[1]}, {u[2]}"/></transform>
    <sampler type="independent"><integer name="sample_count" value="{spp}"/></sampler>
    <film type="hdrfilm"><integer name="width" value="{size[0]}"/><integer name="height" value="{size[1]}"/><rfilter type="{rfilter}"/></film></sensor>
  {shapes}
  {emitters}
</scene>"""
