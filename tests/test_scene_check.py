"""The scene checks (liverrenderer_amd/csrc/scene_check.cpp) without a GPU.

1. Every refusal of lrt_scene_from_desc, through the ABI: one case per throw site of the validator, with its status code and its full text
   (the texts were recorded from the validator as it stood in capi.cpp before it moved), and per group the same edit made harmlessly.
2. tests/host/scene_check_main.cpp under AddressSanitizer and UBSan (compiled and run as tests/test_scene_prep.py does its program): the
   refusals of the scene preparation that a render can still reach, the feature table, and descriptions with every index out of range.
3. What the XML loader builds passes the validator, for the scene families of this suite.
4. prbvolpath's five refusals at load, and which one wins when two apply."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES, LIVER_XML, PARENCHYMA_XML, GLISSON_XML, REALTIME_XML, MULTIMESH_XML, MULTIMESH_FULL_XML, layer_scene_variant

CSRC = os.path.join(ROOT, "liverrenderer_amd", "csrc")
OK, INVALID, UNSUPPORTED = 0, 1, 4
P = "lrt_scene_from_desc: "
NAN, INF = float("nan"), float("inf")

HEAD = ('<scene version="3.0.0"><integrator type="volpath"/><sensor type="perspective"><film type="hdrfilm"><integer name="width" value="8"/>'
        '<integer name="height" value="8"/><rfilter type="box"/></film></sensor>')
SKY = '<emitter type="constant"/>'


def _flat_png(tmp):
    from rough_cases import write_flat_png
    path = os.path.join(str(tmp), "flat.png")
    write_flat_png(path)
    return path


def base_xml(name, tmp):
    """the smallest scene that has the objects a group of cases edits"""
    if name == "medium":          # media: 0 hg, 1 by phase-table entry 2; phases: 0 tabulated, 1 hg, 2 their blend
        return HEAD + SKY + ('<shape type="cube"><bsdf type="null"/><medium name="interior" type="homogeneous"><phase type="hg"><float name="g" value="0.5"/></phase></medium>'
                             '<medium name="exterior" type="homogeneous"><phase type="blendphase"><float name="weight" value="0.3"/>'
                             '<phase type="tabphase"><string name="values" value="1, 2, 3"/></phase><phase type="hg"/></phase></medium></shape></scene>')
    if name == "surfaces":        # bsdfs: 0 diffuse, 1 bumpmap over it, 2 dielectric, 3 roughdielectric; textures: 0 rgb, 1 bitmap
        return HEAD + SKY + (f'<shape type="rectangle"><bsdf type="bumpmap"><texture name="t" type="bitmap"><boolean name="raw" value="true"/><string name="filename" value="{_flat_png(tmp)}"/></texture>'
                             '<bsdf type="diffuse"/></bsdf></shape><shape type="rectangle"><bsdf type="dielectric"/></shape><shape type="rectangle"><bsdf type="roughdielectric"/></shape></scene>')
    if name == "smooth":          # bsdfs: 0 conductor, 1 plastic, 2 diffuse, 3 twosided over it, 4 dielectric, 5 diffuse, 6 bumpmap over it; the last texture is a bitmap
        return HEAD + SKY + ('<shape type="rectangle"><bsdf type="conductor"/></shape><shape type="rectangle"><bsdf type="plastic"><rgb name="specular_reflectance" value="0.9"/></bsdf></shape>'
                             '<shape type="rectangle"><bsdf type="twosided"><bsdf type="diffuse"/></bsdf></shape><shape type="rectangle"><bsdf type="dielectric"/></shape>'
                             f'<shape type="rectangle"><bsdf type="bumpmap"><texture name="t" type="bitmap"><boolean name="raw" value="true"/><string name="filename" value="{_flat_png(tmp)}"/></texture>'
                             '<bsdf type="diffuse"/></bsdf></shape></scene>')
    if name == "lights":          # shapes: 0 cube, 1 sphere; emitters: 0 constant, 1 point, 2 spot with a checkerboard, 3 directional; texture 0: a colour; the spot's: a checkerboard
        return HEAD + SKY + ('<shape type="cube"/><shape type="sphere"><point name="center" x="3" y="0" z="0"/></shape><emitter type="point"/>'
                             '<emitter type="spot"><float name="cutoff_angle" value="40"/><float name="beam_width" value="25"/><texture type="checkerboard" name="texture"/></emitter>'
                             '<emitter type="directional"/></scene>')
    if name == "mesh_light":      # shape 0: a cube with emitter 0
        return HEAD + '<shape type="cube"><emitter type="area"/></shape></scene>'
    assert name == "het"          # medium 0: a 2 x 2 x 2 grid
    import liverrenderer_amd as mi
    vol = os.path.join(str(tmp), "grid.vol")
    mi.write_volume_grid(vol, np.arange(1, 9, dtype=np.float32).reshape(2, 2, 2))
    return HEAD + SKY + f'<shape type="cube"><bsdf type="null"/><medium name="interior" type="heterogeneous"><volume name="sigma_t" type="gridvolume"><string name="filename" value="{vol}"/></volume></medium></shape></scene>'


@pytest.fixture(scope="module")
def bases(mi, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scene_check_bases")
    out = {n: mi.load_string(base_xml(n, tmp)) for n in ("medium", "surfaces", "smooth", "lights", "mesh_light", "het")}
    out["cornell"] = mi.load_dict(mi.cornell_box())
    return out


class Edit:
    """A shallow copy of a loaded description with its object arrays cloned (as test_host.py::test_scene_from_desc_validation builds them)."""
    def __init__(self, scene):
        from liverrenderer_amd import _lib
        self.d = d = _lib.SceneDesc.from_buffer_copy(scene.desc)
        self.keep = [scene]
        for name, typ, n in (("shapes", _lib.ShapeDesc, d.n_shapes), ("bsdfs", _lib.BsdfDesc, d.n_bsdfs), ("textures", _lib.TextureDesc, d.n_textures),
                             ("media", _lib.MediumDesc, d.n_media), ("emitters", _lib.EmitterDesc, d.n_emitters), ("phases", _lib.PhaseDesc, d.n_phases)):
            setattr(self, name, self.clone(name, typ, n))
        self.sh, self.bs, self.tx, self.med, self.em, self.ph = self.shapes, self.bsdfs, self.textures, self.media, self.emitters, self.phases

    def clone(self, name, typ, n, owner=None):
        owner = owner or self.d
        arr = (typ * max(n, 1))(*[getattr(owner, name)[i] for i in range(n)])
        self.keep.append(arr)
        setattr(owner, name, C.cast(arr, C.POINTER(typ)))
        return arr

    def floats(self, owner, name, values):
        arr = (C.c_float * len(values))(*values)
        self.keep.append(arr)
        setattr(owner, name, C.cast(arr, C.POINTER(C.c_float)))


def attempt(scene, mutate):
    from liverrenderer_amd import _lib
    L = _lib.lib()
    e = Edit(scene)
    mutate(e)
    h = C.c_void_p()
    st = L.lrt_scene_from_desc(C.byref(e.d), C.byref(h))
    if st == 0:
        L.lrt_scene_free(h)
    return st, (L.lrt_last_error().decode() if st else "")


def put(obj, **kw):
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(obj, k)[i] = x
        else:
            setattr(obj, k, v)


BITMAP = "unsupported: a bitmap texture as %s (bitmaps are supported as bump-map heights only)"
SPOT_ANGLES = "spot emitter: 0 < beam_width <= cutoff_angle <= 180 degrees is required (beam_width %s, cutoff_angle %s)"

# (name, base, edit, status, text)
REFUSED = [
    # ---- the arrays
    ("null geometry array", "cornell", lambda e: put(e.d, normals=None), INVALID, P + "null geometry array"),
    ("null object array", "cornell", lambda e: put(e.d, textures=None), INVALID, P + "null object array"),
    ("face vertex", "cornell", lambda e: e.clone("faces", C.c_uint32, 3 * e.d.n_faces).__setitem__(5, 10 ** 6), INVALID, P + "face references an invalid vertex"),
    ("face shape", "cornell", lambda e: e.clone("face_shape", C.c_uint32, e.d.n_faces).__setitem__(3, 8), INVALID, P + "face references an invalid shape"),
    # ---- textures
    ("texture type", "cornell", lambda e: put(e.tx[0], type=3), INVALID, P + "invalid texture type"),
    ("texture type negative", "cornell", lambda e: put(e.tx[0], type=-1), INVALID, P + "invalid texture type"),
    ("bitmap without texels", "surfaces", lambda e: put(e.tx[1], data=None), INVALID, P + "bitmap texture without texels or with invalid dimensions"),
    ("bitmap with two channels", "surfaces", lambda e: put(e.tx[1], channels=2), INVALID, P + "bitmap texture without texels or with invalid dimensions"),
    # ---- BSDFs
    ("bsdf type", "cornell", lambda e: put(e.bs[0], type=8), INVALID, P + "invalid bsdf type"),
    ("diffuse texture", "cornell", lambda e: put(e.bs[0], reflectance=3), INVALID, P + "diffuse bsdf references an invalid texture"),
    ("diffuse texture negative", "cornell", lambda e: put(e.bs[0], reflectance=-1), INVALID, P + "diffuse bsdf references an invalid texture"),
    ("diffuse bitmap", "surfaces", lambda e: put(e.bs[0], reflectance=1), UNSUPPORTED, BITMAP % "diffuse reflectance"),
    ("bumpmap nested", "surfaces", lambda e: put(e.bs[1], nested=4), INVALID, P + "bumpmap references an invalid nested bsdf"),
    ("bumpmap over bumpmap", "surfaces", lambda e: put(e.bs[1], nested=1), INVALID, P + "bumpmap references an invalid nested bsdf"),
    ("bumpmap over twosided", "smooth", lambda e: put(e.bs[6], nested=3), UNSUPPORTED, "unsupported: a twosided BSDF nested in a bumpmap"),
    ("bumpmap texture", "surfaces", lambda e: put(e.bs[1], texture=2), INVALID, P + "bumpmap references an invalid texture"),
    ("dielectric eta", "surfaces", lambda e: put(e.bs[2], eta=0.0), INVALID, P + "dielectric with a non-positive relative index of refraction"),
    ("rough eta one", "surfaces", lambda e: put(e.bs[3], eta=1.0), INVALID, P + "roughdielectric: the interior and exterior indices of refraction must be positive and differ"),
    ("rough eta nan", "surfaces", lambda e: put(e.bs[3], eta=NAN), INVALID, P + "roughdielectric: the interior and exterior indices of refraction must be positive and differ"),
    ("rough alpha", "surfaces", lambda e: put(e.bs[3], alpha_v=-0.1), INVALID, P + "roughdielectric with an invalid roughness"),
    ("rough alpha inf", "surfaces", lambda e: put(e.bs[3], alpha_u=INF), INVALID, P + "roughdielectric with an invalid roughness"),
    ("rough distribution", "surfaces", lambda e: put(e.bs[3], distribution=2), INVALID, P + "roughdielectric with an invalid distribution (0: beckmann, 1: ggx)"),
    ("rough texture", "surfaces", lambda e: put(e.bs[3], specular_transmittance=2), INVALID, P + "roughdielectric references an invalid texture"),
    ("rough bitmap", "surfaces", lambda e: put(e.bs[3], specular_reflectance=1), UNSUPPORTED, "unsupported: a bitmap texture as roughdielectric specular_reflectance / specular_transmittance"),
    # ---- conductor, plastic, twosided: their texts pass bare
    ("conductor texture", "smooth", lambda e: put(e.bs[0], specular_reflectance=-1), INVALID, "conductor specular_reflectance references an invalid texture"),
    ("conductor bitmap", "smooth", lambda e: put(e.bs[0], specular_reflectance=e.d.n_textures - 1), UNSUPPORTED, BITMAP % "conductor specular_reflectance"),
    ("conductor eta inf", "smooth", lambda e: put(e.bs[0], k_g=INF), INVALID, "conductor with an index of refraction that is not finite"),
    ("conductor eta k zero", "smooth", lambda e: put(e.bs[0], eta_b=0.0, k_b=0.0), INVALID,
     "conductor with eta = k = 0 in a channel (no index of refraction: its Fresnel term is 0 / 0 at normal incidence; the plugin's default is eta = 0, k = 1)"),
    ("plastic eta", "smooth", lambda e: put(e.bs[1], eta=0.0), INVALID, "The interior and exterior indices of refraction must be positive!"),
    ("plastic diffuse texture", "smooth", lambda e: put(e.bs[1], diffuse_reflectance=-1), INVALID, "plastic diffuse_reflectance references an invalid texture"),
    ("plastic specular texture", "smooth", lambda e: put(e.bs[1], specular_reflectance=-2), INVALID, "plastic specular_reflectance references an invalid texture"),
    ("plastic specular bitmap", "smooth", lambda e: put(e.bs[1], specular_reflectance=e.d.n_textures - 1), UNSUPPORTED, BITMAP % "plastic specular_reflectance"),
    ("twosided without child", "smooth", lambda e: put(e.bs[3], nested=-1), INVALID, "A nested one-sided material is required!"),
    ("twosided child", "smooth", lambda e: put(e.bs[3], nested_back=7), INVALID, "twosided references an invalid nested bsdf"),
    ("twosided over dielectric", "smooth", lambda e: put(e.bs[3], nested=4), INVALID, "Only materials without a transmission component can be nested!"),
    ("twosided over bumpmap", "smooth", lambda e: put(e.bs[3], nested_back=6), UNSUPPORTED, "unsupported: a bumpmap nested in a twosided BSDF (its children are diffuse, conductor or plastic)"),
    ("twosided over twosided", "smooth", lambda e: put(e.bs[3], nested=3), UNSUPPORTED, "unsupported: a twosided nested in a twosided BSDF (its children are diffuse, conductor or plastic)"),
    # ---- media
    ("medium type", "medium", lambda e: put(e.med[0], type=5), INVALID, P + "invalid medium type"),
    ("grid data", "het", lambda e: put(e.med[0], grid_data=None), INVALID, P + "heterogeneous medium without grid data"),
    ("grid resolution", "het", lambda e: put(e.med[0], grid_res=[2, 0, 2]), INVALID, P + "heterogeneous medium without grid data"),
    ("grid frame", "het", lambda e: put(e.med[0], grid_to_local=[NAN]), INVALID, P + "heterogeneous medium: grid_to_local is not finite (a singular volume to_world?)"),
    ("grid box", "het", lambda e: put(e.med[0], grid_bbox_max=[1.0, 0.0, 1.0]), INVALID, P + "heterogeneous medium: empty or unbounded grid bounding box"),
    ("medium phase", "medium", lambda e: put(e.med[0], phase=2), INVALID, P + "invalid phase function"),
    ("medium g", "medium", lambda e: put(e.med[0], g=1.0), INVALID, P + "The asymmetry parameter must lie in the interval (-1, 1)!"),
    # ---- the phase table
    ("phases null", "medium", lambda e: put(e.d, phases=None), INVALID, P + "phase table: null array"),
    ("phase type", "medium", lambda e: put(e.ph[0], type=5), INVALID, P + "phase table: invalid phase function"),
    ("phase g", "medium", lambda e: put(e.ph[1], g=-1.0), INVALID, P + "phase table: The asymmetry parameter must lie in the interval (-1, 1)!"),
    ("tabulated without values", "medium", lambda e: put(e.ph[0], values=None), INVALID, P + "phase table: tabulated phase function without values"),
    ("tabulated nan", "medium", lambda e: e.floats(e.ph[0], "values", [1.0, NAN, 3.0]), INVALID, P + "phase table: tabulated phase function with a value that is not finite"),
    ("tabulated one value", "medium", lambda e: put(e.ph[0], n_values=1), INVALID, P + "ContinuousDistribution: needs at least two entries!"),
    ("tabulated negative", "medium", lambda e: e.floats(e.ph[0], "values", [1.0, -2.0, 3.0]), INVALID, P + "ContinuousDistribution: entries must be non-negative!"),
    ("tabulated zeros", "medium", lambda e: e.floats(e.ph[0], "values", [0.0, 0.0, 0.0]), INVALID, P + "ContinuousDistribution: no probability mass found!"),
    ("tabulated overflow", "medium", lambda e: e.floats(e.ph[0], "values", [3e38, 3e38, 3e38]), INVALID, P + "phase table: ContinuousDistribution: no probability mass found!"),
    ("blend weight", "medium", lambda e: put(e.ph[2], weight=NAN), INVALID, P + "phase table: blendphase with a weight that is not a number"),
    ("blend child", "medium", lambda e: put(e.ph[2], child=[0, 3]), INVALID, P + "phase table: blendphase references an invalid child"),
    ("blend of blend", "medium", lambda e: put(e.ph[2], child=[2, 1]), UNSUPPORTED, "unsupported: a blendphase as the child of a blendphase (one level is built)"),
    ("medium entry", "medium", lambda e: put(e.med[1], phase_index=3), INVALID, P + "phase table: medium references an invalid entry"),
    ("medium hg entry", "medium", lambda e: put(e.med[1], phase_index=1), INVALID,
     P + "phase table: medium references an isotropic / hg entry (a medium's entry is tabulated, rayleigh or blend; use the medium's `phase` / `g`)"),
    # ---- shapes
    ("shape bsdf", "cornell", lambda e: put(e.sh[2], bsdf=3), INVALID, P + "shape references an invalid bsdf"),
    ("shape emitter", "cornell", lambda e: put(e.sh[2], emitter=1), INVALID, P + "shape references an invalid emitter/medium"),
    ("shape medium", "cornell", lambda e: put(e.sh[1], interior_medium=3), INVALID, P + "shape references an invalid emitter/medium"),
    ("shape exterior", "medium", lambda e: put(e.sh[0], exterior_medium=-2), INVALID, P + "shape references an invalid emitter/medium"),
    ("face range", "cornell", lambda e: put(e.sh[7], n_faces=1000), INVALID, P + "shape face range exceeds the face array"),
    ("face range wraps", "cornell", lambda e: put(e.sh[7], first_face=0xffffffff), INVALID, P + "shape face range exceeds the face array"),
    ("shape kind", "cornell", lambda e: put(e.sh[3], kind=3), INVALID, P + "invalid shape kind"),
    ("sphere with faces", "lights", lambda e: put(e.sh[1], n_faces=2), INVALID, P + "a sphere shape has no faces"),
    ("shape and emitter", "cornell", lambda e: put(e.sh[2], emitter=0), INVALID, P + "shape and area emitter do not reference each other"),
    # ---- emitters
    ("emitter type", "lights", lambda e: put(e.em[1], type=6), INVALID, P + "invalid emitter type"),
    ("spot to_world", "lights", lambda e: put(e.em[2], to_world=[0.0, 0.0, 0.0]), INVALID, P + "spot emitter: to_world must be finite and invertible, the value finite"),
    ("directional irradiance", "lights", lambda e: put(e.em[3], radiance=[1.0, INF, 1.0]), INVALID, P + "directional emitter: to_world must be finite and invertible, the value finite"),
    ("spot beam", "lights", lambda e: put(e.em[2], beam_width=50.0), INVALID, P + SPOT_ANGLES % ("50.000000", "40.000000")),
    ("spot cutoff", "lights", lambda e: put(e.em[2], cutoff_angle=181.0), INVALID, P + SPOT_ANGLES % ("25.000000", "181.000000")),
    ("spot texture", "lights", lambda e: put(e.em[2], texture=e.d.n_textures), INVALID, P + "spot emitter references an invalid texture"),
    ("spot bitmap", "lights", lambda e: put(e.tx[e.em[2].texture], type=2, width=1, height=1, channels=1) or e.floats(e.tx[e.em[2].texture], "data", [1.0]), UNSUPPORTED,
     "unsupported: a bitmap texture as the spot emitter's 'texture' (bitmaps are held as one luminance float per texel, for bump maps only; a checkerboard is supported)"),
    ("spot uniform texture", "lights", lambda e: put(e.em[2], texture=0), INVALID, P + "The parameter 'texture' must be spatially varying (e.g. bitmap type)!"),
    ("spot textured cutoff", "lights", lambda e: put(e.em[2], cutoff_angle=90.0), INVALID,
     P + "spot emitter: cutoff_angle must be below 90 degrees when a texture is given (uv_factor = tan(cutoff_angle) must be positive and finite)"),
    ("emitter shape", "cornell", lambda e: put(e.em[0], shape=99) or put(e.sh[0], emitter=-1), INVALID, P + "area emitter references an invalid shape"),
    ("emitter on a sphere", "lights", lambda e: put(e.em[1], type=0, shape=1), UNSUPPORTED, "unsupported: an area emitter on a sphere (area emitters are supported on rectangles and triangle meshes)"),
    ("emitter on an empty rectangle", "cornell", lambda e: put(e.sh[0], n_faces=0), INVALID, P + "area emitter on a rectangle without faces"),
    ("emitter on an empty mesh", "mesh_light", lambda e: put(e.sh[0], n_faces=0), INVALID, "Cannot create sampling table for an empty mesh: shapes[0]"),
    ("emitter on a flat mesh", "mesh_light", lambda e: e.floats(e.d, "positions", [0.0] * (3 * e.d.n_vertices)), INVALID,
     'area emitter on shape "shapes[0]": the mesh has no surface area to sample (total area 0.000000)'),
    ("envmap without data", "lights", lambda e: put(e.em[0], type=1), INVALID, P + "environment map without data or smaller than 2x3 pixels"),
    ("two environments", "lights", lambda e: put(e.em[1], type=2), INVALID, P + "Only one environment emitter can be specified per scene."),
    # ---- sensor and film
    ("sensor medium", "cornell", lambda e: put(e.d.sensor, medium=0), INVALID, P + "sensor references an invalid medium"),
    ("near clip", "cornell", lambda e: put(e.d.sensor, near_clip=0.0), INVALID, P + "invalid clipping planes"),
    ("far clip", "cornell", lambda e: put(e.d.sensor, far_clip=0.0005), INVALID, P + "invalid clipping planes"),
    ("fov", "cornell", lambda e: put(e.d.sensor, fov_x=180.0), INVALID, P + "The horizontal field of view must be in the range [0, 180]!"),
    ("crop window", "cornell", lambda e: put(e.d.film, crop_width=9999), INVALID, P + "Invalid crop window specification!"),
    ("film size", "cornell", lambda e: put(e.d.film, height=0), INVALID, P + "Invalid crop window specification!"),
    ("filter type", "cornell", lambda e: put(e.d.film, rfilter=3), INVALID, P + "invalid reconstruction filter"),
    ("filter radius", "cornell", lambda e: put(e.d.film, rfilter_param=0.0), INVALID, P + "invalid reconstruction filter"),
    ("camera scale", "cornell", lambda e: put(e.d.sensor, to_world=[2.0]), INVALID, P + "Scale factors in the camera-to-world transformation are not allowed!"),
    ("film footprint", "cornell", lambda e: put(e.d.film, rfilter_param=5000.0), INVALID,
     P + "film footprint out of range: a gaussian or tent filter needs a radius of at most 16384 pixels and a film of at most 49151 pixels per side (radius 20000.000000, film 256 x 256)"),
    # ---- integrator and sampler
    ("integrator", "cornell", lambda e: put(e.d.integrator, type=6), INVALID, P + "invalid integrator type"),
    ("max_depth", "cornell", lambda e: put(e.d.integrator, max_depth=-2), INVALID, P + "invalid max_depth / rr_depth"),
    ("rr_depth", "cornell", lambda e: put(e.d.integrator, rr_depth=0), INVALID, P + "invalid max_depth / rr_depth"),
    ("sampler type", "cornell", lambda e: put(e.d, sampler_type=2), INVALID, P + "invalid sampler"),
    ("sample count", "cornell", lambda e: put(e.d, sample_count=0), INVALID, P + "invalid sampler"),
]

# per group, the same fields edited to another valid value
ACCEPTED = [
    ("nothing", "cornell", lambda e: None), ("nothing", "medium", lambda e: None), ("nothing", "surfaces", lambda e: None), ("nothing", "smooth", lambda e: None),
    ("nothing", "lights", lambda e: None), ("nothing", "mesh_light", lambda e: None), ("nothing", "het", lambda e: None),
    ("no geometry", "cornell", lambda e: [put(s, first_face=0, n_faces=0, emitter=-1) for s in e.sh] and put(e.d, n_vertices=0, n_faces=0, n_emitters=0, normals=None, faces=None)),
    ("texture", "cornell", lambda e: put(e.tx[0], type=1)),
    ("bitmap with three channels", "surfaces", lambda e: put(e.tx[1], channels=3) or e.floats(e.tx[1], "data", [0.5] * (3 * e.tx[1].width * e.tx[1].height))),
    ("bsdf", "cornell", lambda e: put(e.bs[0], type=1, reflectance=-1, eta=1.5)),
    ("diffuse texture", "cornell", lambda e: put(e.bs[0], reflectance=2)),
    ("bumpmap over roughdielectric", "surfaces", lambda e: put(e.bs[1], nested=3)),
    ("rough", "surfaces", lambda e: put(e.bs[3], eta=0.5, alpha_u=0.0, alpha_v=3.0, distribution=1, specular_reflectance=0, specular_transmittance=-1)),
    ("conductor", "smooth", lambda e: put(e.bs[0], eta_r=0.0, k_r=2.0, specular_reflectance=1)),
    ("plastic", "smooth", lambda e: put(e.bs[1], eta=0.7, specular_reflectance=-1, diffuse_reflectance=0)),
    ("twosided", "smooth", lambda e: put(e.bs[3], nested=0, nested_back=1)),
    ("medium", "medium", lambda e: put(e.med[0], type=1, phase=0, g=5.0)),
    ("medium g", "medium", lambda e: put(e.med[0], g=-0.99)),
    ("grid", "het", lambda e: put(e.med[0], grid_res=[4, 2, 1], grid_bbox_max=[9.0, 9.0, 9.0], grid_to_local=[0.0] * 12)),
    ("grid maximum zero", "het", lambda e: put(e.med[0], grid_max=0.0)),      # accepted here, refused by the first render
    ("phases", "medium", lambda e: put(e.ph[1], g=0.0) or put(e.ph[2], weight=7.0, child=[1, 0]) or e.floats(e.ph[0], "values", [0.0, 0.0, 1.0])),
    ("medium entry", "medium", lambda e: put(e.med[1], phase_index=0) or put(e.med[0], phase_index=-1)),
    ("no phase table", "medium", lambda e: put(e.d, n_phases=0, phases=None) or put(e.med[1], phase_index=77)),
    ("shape", "cornell", lambda e: put(e.sh[2], bsdf=2, interior_medium=-1, first_face=0, n_faces=e.d.n_faces, kind=0)),
    ("sphere", "lights", lambda e: put(e.sh[1], to_world=[0.0] * 16)),       # a zero radius: accepted here, refused by the first render
    ("emitters", "lights", lambda e: put(e.em[2], beam_width=40.0, texture=-1, cutoff_angle=180.0) or put(e.em[3], to_world=[0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])),
    ("spot textured", "lights", lambda e: put(e.em[2], cutoff_angle=89.0, beam_width=89.0)),
    ("emitter on another rectangle", "cornell", lambda e: put(e.em[0], shape=1) or put(e.sh[0], emitter=-1) or put(e.sh[1], emitter=0)),
    ("emitter on a mesh", "cornell", lambda e: put(e.em[0], shape=6) or put(e.sh[0], emitter=-1) or put(e.sh[6], emitter=0)),
    ("environment", "lights", lambda e: put(e.em[0], type=3)),
    ("sensor and film", "cornell", lambda e: put(e.d.sensor, near_clip=1.0, far_clip=1.5, fov_x=179.0, to_world=[-1.0]) or put(e.d.film, crop_width=1, crop_offset_x=255, rfilter=2, rfilter_param=16384.0)),
    ("box filter on a wide film", "cornell", lambda e: put(e.d.film, width=60000, rfilter=0, rfilter_param=0.0)),
    ("integrator and sampler", "cornell", lambda e: put(e.d.integrator, type=5, max_depth=-1, rr_depth=1) or put(e.d, sampler_type=1, sample_count=1)),
    ("prbvolpath with a sphere", "lights", lambda e: put(e.d.integrator, type=2)),      # refused by the render, not here
]


@pytest.mark.parametrize("name,base,edit,status,text", REFUSED, ids=[f"{c[1]}-{c[0]}".replace(" ", "_") for c in REFUSED])
def test_refused(bases, name, base, edit, status, text):
    assert attempt(bases[base], edit) == (status, text)


@pytest.mark.parametrize("name,base,edit", ACCEPTED, ids=[f"{c[1]}-{c[0]}".replace(" ", "_") for c in ACCEPTED])
def test_accepted(bases, name, base, edit):
    assert attempt(bases[base], edit) == (OK, "")


def test_first_fault_wins(bases):
    """the order of the checks: textures, BSDFs, media, phase table, shapes, emitters, sensor and film, integrator"""
    chains = {
        "cornell": [(lambda e: put(e.tx[0], type=9), "invalid texture type"), (lambda e: put(e.bs[0], type=9), "invalid bsdf type"), (lambda e: put(e.sh[0], kind=9), "invalid shape kind"),
                    (lambda e: put(e.em[0], shape=99) or put(e.sh[0], emitter=-1), "area emitter references an invalid shape"), (lambda e: put(e.d.sensor, fov_x=0.0), "The horizontal field of view must be in the range [0, 180]!"),
                    (lambda e: put(e.d.integrator, type=9), "invalid integrator type")],
        "medium": [(lambda e: put(e.bs[0], type=9), "invalid bsdf type"), (lambda e: put(e.med[0], type=9), "invalid medium type"), (lambda e: put(e.ph[0], type=9), "phase table: invalid phase function"),
                   (lambda e: put(e.sh[0], kind=9), "invalid shape kind"), (lambda e: put(e.em[0], type=9), "invalid emitter type"), (lambda e: put(e.d.film, rfilter=9), "invalid reconstruction filter"),
                   (lambda e: put(e.d, sample_count=0), "invalid sampler")],
    }
    for base, chain in chains.items():
        for k in range(len(chain)):
            assert attempt(bases[base], lambda e: [fn(e) for fn, _ in chain[k:]]) == (INVALID, P + chain[k][1]), (base, k)


# ---- 2. the host program
@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scene_check")
    exe = str(tmp / "scene_check_main")
    src = [os.path.join(ROOT, "tests", "host", "scene_check_main.cpp")] + [os.path.join(CSRC, f) for f in ("scene_prep.cpp", "bvh.cpp", "loader.cpp", "xml.cpp", "image_io.cpp")]
    cc = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                         "-I", CSRC, "-w", *src, "-lz", "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, str(tmp)], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    return [json.loads(l) for l in run.stdout.splitlines()]


def test_preparation_refusals(lines):
    """what a first render still refuses (the reachability table), by the path that reaches it"""
    got = {l["run"]: l["error"] for l in lines if l["case"] == "prepare"}
    assert got == {
        "xml sphere radius 0": "sphere with a zero or invalid radius",
        "desc sphere radius 0": "sphere with a zero or invalid radius",
        "desc sphere radius nan": "sphere with a zero or invalid radius",
        "xml grid of zeros": "heterogeneous medium without a valid grid",
        "desc grid_max 0": "heterogeneous medium without a valid grid",
        "xml 65 media": "at most 64 media are supported",
        "desc 65 media": "at most 64 media are supported",
        "xml plastic int_ior 0": "The interior and exterior indices of refraction must be positive!",
        "desc envmap 16384 wide": None, "desc envmap 16385 wide": "environment map too large for the sampling hierarchy",
        "xml fine": None, "desc fine": None,
    }


FLAGS = ("sphere", "point_emitter", "delta_emitter", "mesh_emitter", "rough_bsdf", "smooth_bsdf", "phase_entry")


def test_feature_table(lines):
    rows = {l["run"]: l for l in lines if l["case"] == "features"}
    want = {"base": [], "sphere": ["sphere"], "point": ["point_emitter"], "spot": ["delta_emitter"], "directional": ["delta_emitter"], "mesh emitter": ["mesh_emitter"],
            "rectangle emitter": [], "roughdielectric": ["rough_bsdf"], "conductor": ["smooth_bsdf"], "plastic": ["smooth_bsdf"], "twosided": ["smooth_bsdf"],
            "bumpmap over roughdielectric": ["rough_bsdf"], "bumpmap over conductor": ["smooth_bsdf"], "bumpmap over plastic": ["smooth_bsdf"], "bumpmap over twosided": ["smooth_bsdf"],
            "roughdielectric unreferenced": [], "conductor unreferenced": [], "plastic unreferenced": [], "twosided unreferenced": [],
            "phase entry on the interior": ["phase_entry"], "phase entry on the exterior": ["phase_entry"], "phase entry on the sensor only": ["phase_entry"],
            "phase entry unreferenced": [], "phase index without a table": [],
            "area emitter shape out of range": [], "area emitter shape negative": [], "shape bsdf out of range": [], "bumpmap nested out of range": [],
            "medium indices out of range": [], "sphere and spot and plastic": ["sphere", "delta_emitter", "smooth_bsdf"]}
    assert sorted(rows) == sorted(want)
    for run, flags in want.items():
        l = rows[run]
        assert [f for f in FLAGS if l[f]] == flags, run
        if l["prepared"]:                  # (the rows with indices out of range are for scene_features alone)
            assert l["ext"] == int(bool(flags)) and l["smooth"] == int("smooth_bsdf" in flags), run
    assert sum(l["prepared"] for l in rows.values()) >= 24


def test_validator_reads_nothing_out_of_range(lines):
    """every index field set below and above its range: the validator throws (the sanitizers watch what it reads on the way)"""
    rows = [l for l in lines if l["case"] == "index" and l["field"] != "none"]
    assert [l["error"] for l in lines if l["case"] == "index" and l["field"] == "none"] == [None, None]      # the scene the rows edit is accepted
    assert len(rows) >= 2 * 20 and all(l["error"] for l in rows), [l for l in rows if not l["error"]]
    fields = {l["field"] for l in rows}
    assert fields >= {"faces", "face_shape", "diffuse.reflectance", "bumpmap.nested", "bumpmap.texture", "roughdielectric.specular_reflectance", "roughdielectric.specular_transmittance",
                      "conductor.specular_reflectance", "plastic.diffuse_reflectance", "plastic.specular_reflectance", "twosided.nested", "twosided.nested_back",
                      "shape.bsdf", "shape.emitter", "shape.interior_medium", "shape.exterior_medium", "shape.first_face", "emitter.shape", "spot.texture", "sensor.medium",
                      "medium.phase_index", "blend.child0", "blend.child1"}


# ---- 3. what the loader builds passes the validator
def accepted_by_validator(sc):
    from liverrenderer_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    st = L.lrt_scene_from_desc(C.byref(sc.desc), C.byref(h))
    msg = L.lrt_last_error().decode() if st else ""
    if st == 0:
        L.lrt_scene_free(h)
    return st, msg


def loaded_families(mi, tmp):
    import scene_gen, phase_cases, rough_cases, smooth_cases, spot_cases, sensor_cases, medium_cases, envmap_cases, surface_cases, mesh_emitter_ref, sphere_ref
    tmp = str(tmp)
    small = dict(spp=1, res_width=16, res_height=9)
    yield "cornell_box", mi.load_dict(mi.cornell_box())
    for name, path in (("liver", LIVER_XML), ("parenchyma", PARENCHYMA_XML), ("glisson", GLISSON_XML), ("realtime", REALTIME_XML), ("multimesh", MULTIMESH_XML), ("multimesh_full", MULTIMESH_FULL_XML)):
        yield name, mi.load_file(path, **small)
    yield "liver volpath", mi.load_file(LIVER_XML, integrator="volpath", **small)
    for name in ("GlissonCapsule", "Parenchyma"):
        xml, base = layer_scene_variant(name)
        yield "layer " + name, mi.load_string(xml, base, **small)
    for d in sphere_ref.SPHERE_SCENES:              # tests/golden/scenes, with RGB coefficients (the files as they are fail to load, as in the reference)
        for fname in ("scene.xml", "scene_temp.xml"):
            yield f"golden {d} {fname}", mi.load_string(sphere_ref.rgb_variant(os.path.join(sphere_ref.GOLDEN_SCENES, d, fname)), os.path.join(sphere_ref.GOLDEN_SCENES, d))
    # tests/scene_gen.py
    vol = os.path.join(tmp, "smoke.vol"); mi.write_volume_grid(vol, scene_gen.smoke_grid(shape=(3, 2, 2)))
    yield "fog", mi.load_string(scene_gen.fog_xml())
    yield "fog sensor inside", mi.load_string(scene_gen.fog_xml(rf="tent", sensor_medium='<ref id="haze"/>', exterior='<ref name="exterior" id="haze"/>', env='<emitter type="constant"/>'))
    yield "het", mi.load_string(scene_gen.het_xml(vol))
    yield "het ld", mi.load_string(scene_gen.het_xml(vol, sampler="ldsampler", spectral="false", boundary="dielectric"))
    yield "two media", mi.load_string(scene_gen.two_media_xml(vol))
    for seed in range(12):
        xml, integrator = scene_gen.sphere_fuzz_xml(seed, os.path.join(SCENES, "assets"))
        yield f"sphere fuzz {seed}", mi.load_string(xml, os.path.join(SCENES, "assets"))
    # the *_cases.py modules
    for i, p in enumerate(phase_cases.configs()):
        yield f"phase {i}", mi.load_dict(phase_cases.scene_dict(p))
    for cfg in rough_cases.configs()[::7]:
        yield f"rough {cfg}", mi.load_string(rough_cases.scene_xml(rough_cases.bsdf_xml(cfg)))
    for name, bsdf, shape, bump in smooth_cases.CASES:
        yield "smooth " + name, mi.load_string(smooth_cases.scene_xml(bsdf, shape, bump, tmp))
    for case in spot_cases.configs():
        yield "spot " + case.label, mi.load_string(spot_cases.scene_xml(case))
    for sensor in sensor_cases.SENSORS:
        for rfilter in sensor_cases.FILTERS:
            yield f"sensor {sensor} {rfilter}", mi.load_dict(sensor_cases.scene_dict(mi, sensor, rfilter))
    for name in list(medium_cases.VOLUMES) + ["f"]:
        yield "medium " + name, mi.load_string(medium_cases.probe_scene_xml(mi, tmp, name))
    for name in ("const_2x3", "rand_5x3"):
        yield "envmap " + name, envmap_cases.load(mi, tmp, name)
        yield "envmap cube " + name, envmap_cases.load_cube(mi, tmp, name)
    yield "envmap two emitters", envmap_cases.load_two_emitters(mi, tmp)
    for what in ("sphere", "plate"):
        yield "surface " + what, surface_cases.transport_scene(mi, tmp, what, "path")
    yield "mesh emitter", mi.load_string(mesh_emitter_ref.scene_xml('<shape type="cube"><emitter type="area"/></shape>'))


def test_loader_output_passes_the_validator(mi, tmp_path):
    refused, n = [], 0
    for name, sc in loaded_families(mi, tmp_path):
        sc = sc if hasattr(sc, "desc") else sc[0]
        st, msg = accepted_by_validator(sc)
        n += 1
        if st != OK:
            refused.append((name, st, msg))
    assert not refused and n >= 100, (n, refused)


# ---- 4. prbvolpath at load
PRB = [
    ("sphere", '<shape type="sphere"/>', "unsupported: prbvolpath on a scene with sphere shapes, point emitters or area emitters on meshes"),
    ("point", '<shape type="cube"/><emitter type="point"/>', "unsupported: prbvolpath on a scene with sphere shapes, point emitters or area emitters on meshes"),
    ("mesh emitter", '<shape type="cube"><emitter type="area"/></shape>', "unsupported: prbvolpath on a scene with sphere shapes, point emitters or area emitters on meshes"),
    ("spot", '<shape type="cube"/><emitter type="spot"/>', "unsupported: prbvolpath on a scene with a spot or directional emitter (no adjoint is built for them)"),
    ("directional", '<shape type="cube"/><emitter type="directional"/>', "unsupported: prbvolpath on a scene with a spot or directional emitter (no adjoint is built for them)"),
    ("roughdielectric", '<shape type="cube"><bsdf type="roughdielectric"/></shape>', "unsupported: prbvolpath on a scene with a roughdielectric BSDF (no adjoint is built for it)"),
    ("bumpmap over roughdielectric", '<shape type="cube"><bsdf type="bumpmap"><texture name="t" type="bitmap"><string name="filename" value="{png}"/></texture><bsdf type="roughdielectric"/></bsdf></shape>',
     "unsupported: prbvolpath on a scene with a roughdielectric BSDF (no adjoint is built for it)"),
    ("conductor", '<shape type="cube"><bsdf type="conductor"/></shape>', "unsupported: prbvolpath on a scene with a conductor / plastic / twosided BSDF (no adjoint is built for them)"),
    ("plastic", '<shape type="cube"><bsdf type="plastic"/></shape>', "unsupported: prbvolpath on a scene with a conductor / plastic / twosided BSDF (no adjoint is built for them)"),
    ("twosided", '<shape type="cube"><bsdf type="twosided"><bsdf type="diffuse"/></bsdf></shape>', "unsupported: prbvolpath on a scene with a conductor / plastic / twosided BSDF (no adjoint is built for them)"),
    ("rayleigh", '<shape type="cube"><bsdf type="null"/><medium name="interior" type="homogeneous"><phase type="rayleigh"/></medium></shape>',
     "unsupported: prbvolpath on a scene with a tabulated / Rayleigh / blended phase function (no adjoint is built for them)"),
    ("rayleigh on the sensor", '<shape type="cube"/>', "unsupported: prbvolpath on a scene with a tabulated / Rayleigh / blended phase function (no adjoint is built for them)"),
    # two at once: the order of precedence is sphere / point / mesh emitter, spot / directional, roughdielectric, conductor / plastic / twosided, phase table
    ("phase and plastic", '<shape type="cube"><bsdf type="plastic"/><medium name="interior" type="homogeneous"><phase type="rayleigh"/></medium></shape>',
     "unsupported: prbvolpath on a scene with a conductor / plastic / twosided BSDF (no adjoint is built for them)"),
    ("plastic and roughdielectric", '<shape type="cube"><bsdf type="plastic"/></shape><shape type="cube"><bsdf type="roughdielectric"/></shape>',
     "unsupported: prbvolpath on a scene with a roughdielectric BSDF (no adjoint is built for it)"),
    ("roughdielectric and spot", '<shape type="cube"><bsdf type="roughdielectric"/></shape><emitter type="spot"/>', "unsupported: prbvolpath on a scene with a spot or directional emitter (no adjoint is built for them)"),
    ("spot and sphere", '<emitter type="spot"/><shape type="sphere"/>', "unsupported: prbvolpath on a scene with sphere shapes, point emitters or area emitters on meshes"),
]
PRB_HEAD = ('<scene version="3.0.0"><integrator type="{integrator}"/><sensor type="perspective"><film type="hdrfilm"><integer name="width" value="8"/>'
            '<integer name="height" value="8"/><rfilter type="box"/></film>{sensor_medium}</sensor>')


def load_status(xml):
    from liverrenderer_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    st = L.lrt_scene_load_xml_string(xml.encode(), b".", None, 0, C.byref(h))
    if st == 0:
        L.lrt_scene_free(h)
    return st, (L.lrt_last_error().decode() if st else "")


@pytest.mark.parametrize("name,body,text", PRB, ids=[c[0].replace(" ", "_") for c in PRB])
def test_prbvolpath_refusals_at_load(tmp_path, name, body, text):
    body = body.replace("{png}", _flat_png(tmp_path)) if "{png}" in body else body
    sensor_medium = '<medium type="homogeneous"><phase type="rayleigh"/></medium>' if name == "rayleigh on the sensor" else ""
    xml = PRB_HEAD + body + SKY + "</scene>"
    assert load_status(xml.format(integrator="prbvolpath", sensor_medium=sensor_medium)) == (UNSUPPORTED, text)
    assert load_status(xml.format(integrator="volpath", sensor_medium=sensor_medium)) == (OK, "")


def test_prbvolpath_unreferenced_objects_load():
    """an object that no shape references takes nothing off the base kernels, and prbvolpath loads"""
    body = ('<bsdf type="roughdielectric" id="a"/><bsdf type="plastic" id="b"/><medium type="homogeneous" id="m"><phase type="rayleigh"/></medium><shape type="cube"/>' + SKY + "</scene>")
    assert load_status(PRB_HEAD.format(integrator="prbvolpath", sensor_medium="") + body) == (OK, "")
