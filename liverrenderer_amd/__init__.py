"""liverrenderer_amd -- host-side mirror of the reference's Python entry points
(`mi.set_variant`, `mi.load_file`, `mi.load_dict`, `mi.cornell_box`, `mi.render`,
`mi.traverse`; src/python/python/util.py:394-702) over the `hip_ad_rgb` C ABI
(include/liverrt.h).  All arithmetic of the render path runs in the HIP kernels
of libliverrt.so; this module only marshals arguments.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import make_opts

__all__ = ["set_variant", "variant", "variants", "load_file", "load_string", "load_dict", "cornell_box", "render",
           "traverse", "Scene", "ScalarTransform4f", "render_stats", "write_volume_grid", "Bitmap", "Struct", "util", "read_image", "write_exr", "write_png",
           "Denoiser", "OptixDenoiser", "denoise", "moment_variance", "z_test"]

_VARIANT = "hip_ad_rgb"


def variants():
    return ["hip_ad_rgb"]


def set_variant(name):
    """mi.set_variant(): only `hip_ad_rgb` exists in this back-end."""
    global _VARIANT
    if name not in variants():
        raise ImportError(f"Requested an unsupported variant \"{name}\". The following variants are available: "
                          + ", ".join(variants()) + ".")
    _VARIANT = name


def variant():
    return _VARIANT


class ScalarTransform4f:
    """Subset of mi.ScalarTransform4f used by scene dictionaries (right-multiplying chain)."""

    def __init__(self, m=None):
        self.matrix = np.eye(4) if m is None else np.array(m, dtype=np.float64).reshape(4, 4)

    def __matmul__(self, o):
        return ScalarTransform4f(self.matrix @ o.matrix)

    def translate(self, v):
        m = np.eye(4); m[:3, 3] = v
        return ScalarTransform4f(self.matrix @ m)

    def scale(self, v):
        v = np.broadcast_to(np.asarray(v, dtype=np.float64), (3,))
        return ScalarTransform4f(self.matrix @ np.diag([v[0], v[1], v[2], 1.0]))

    def rotate(self, axis, angle):
        x, y, z = [float(a) for a in axis]
        a = math.radians(angle); s, c = math.sin(a), math.cos(a); t = 1 - c
        m = np.eye(4)
        m[:3, :3] = [[c + x * x * t, x * y * t - z * s, x * z * t + y * s],
                     [y * x * t + z * s, c + y * y * t, y * z * t - x * s],
                     [z * x * t - y * s, z * y * t + x * s, c + z * z * t]]
        return ScalarTransform4f(self.matrix @ m)

    def look_at(self, origin, target, up):
        o, tg, up = [np.asarray(v, dtype=np.float64) for v in (origin, target, up)]
        d = tg - o; d /= np.linalg.norm(d)
        left = np.cross(up, d); left /= np.linalg.norm(left)
        nup = np.cross(d, left)
        m = np.eye(4); m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, nup, d, o
        return ScalarTransform4f(self.matrix @ m)


def cornell_box():
    """mi.cornell_box() (src/python/python/util.py:567-702): the same scene dictionary."""
    T = ScalarTransform4f
    return {
        'type': 'scene',
        'integrator': {'type': 'path', 'max_depth': 8},
        'sensor': {
            'type': 'perspective', 'fov_axis': 'smaller', 'near_clip': 0.001, 'far_clip': 100.0, 'focus_distance': 1000,
            'fov': 39.3077,
            'to_world': T().look_at(origin=[0, 0, 3.90], target=[0, 0, 0], up=[0, 1, 0]),
            'sampler': {'type': 'independent', 'sample_count': 64},
            'film': {'type': 'hdrfilm', 'width': 256, 'height': 256, 'rfilter': {'type': 'gaussian'},
                     'pixel_format': 'rgb', 'component_format': 'float32'},
        },
        'white': {'type': 'diffuse', 'reflectance': {'type': 'rgb', 'value': [0.885809, 0.698859, 0.666422]}},
        'green': {'type': 'diffuse', 'reflectance': {'type': 'rgb', 'value': [0.105421, 0.37798, 0.076425]}},
        'red': {'type': 'diffuse', 'reflectance': {'type': 'rgb', 'value': [0.570068, 0.0430135, 0.0443706]}},
        'light': {
            'type': 'rectangle',
            'to_world': T().translate([0.0, 0.99, 0.01]).rotate([1, 0, 0], 90).scale([0.23, 0.19, 0.19]),
            'bsdf': {'type': 'ref', 'id': 'white'},
            'emitter': {'type': 'area', 'radiance': {'type': 'rgb', 'value': [18.387, 13.9873, 6.75357]}},
        },
        'floor': {'type': 'rectangle', 'to_world': T().translate([0.0, -1.0, 0.0]).rotate([1, 0, 0], -90),
                  'bsdf': {'type': 'ref', 'id': 'white'}},
        'ceiling': {'type': 'rectangle', 'to_world': T().translate([0.0, 1.0, 0.0]).rotate([1, 0, 0], 90),
                    'bsdf': {'type': 'ref', 'id': 'white'}},
        'back': {'type': 'rectangle', 'to_world': T().translate([0.0, 0.0, -1.0]), 'bsdf': {'type': 'ref', 'id': 'white'}},
        'green-wall': {'type': 'rectangle', 'to_world': T().translate([1.0, 0.0, 0.0]).rotate([0, 1, 0], -90),
                       'bsdf': {'type': 'ref', 'id': 'green'}},
        'red-wall': {'type': 'rectangle', 'to_world': T().translate([-1.0, 0.0, 0.0]).rotate([0, 1, 0], 90),
                     'bsdf': {'type': 'ref', 'id': 'red'}},
        'small-box': {'type': 'cube', 'to_world': T().translate([0.335, -0.7, 0.38]).rotate([0, 1, 0], -17).scale(0.3),
                      'bsdf': {'type': 'ref', 'id': 'white'}},
        'large-box': {'type': 'cube',
                      'to_world': T().translate([-0.33, -0.4, -0.28]).rotate([0, 1, 0], 18.25).scale([0.3, 0.61, 0.3]),
                      'bsdf': {'type': 'ref', 'id': 'white'}},
    }


# ------------------------------------------------------------- dict -> XML
_TAGS = {
    "scene": "scene", "path": "integrator", "volpath": "integrator", "prbvolpath": "integrator", "aov": "integrator", "moment": "integrator",
    "biovolpath": "integrator", "biovolpath06": "integrator", "volpathmis": "integrator",
    "perspective": "sensor", "independent": "sampler", "ldsampler": "sampler", "hdrfilm": "film",
    "box": "rfilter", "gaussian": "rfilter", "tent": "rfilter",
    "diffuse": "bsdf", "dielectric": "bsdf", "bumpmap": "bsdf", "null": "bsdf", "roughdielectric": "bsdf",
    "conductor": "bsdf", "plastic": "bsdf", "twosided": "bsdf",
    "bitmap": "texture", "checkerboard": "texture",
    "homogeneous": "medium", "liver": "medium", "parenchyma": "medium", "glissonCapsule": "medium", "heterogeneous": "medium",
    "gridvolume": "volume",
    "isotropic": "phase", "hg": "phase", "tabphase": "phase", "rayleigh": "phase", "blendphase": "phase",
    "obj": "shape", "rectangle": "shape", "cube": "shape",
    "area": "emitter", "envmap": "emitter", "constant": "emitter", "spot": "emitter", "directional": "emitter",
}


def _esc(s):
    return str(s).replace("&", "&amp;").replace('"', "&quot;").replace("<", "&lt;").replace(">", "&gt;")


def _fmt(v):
    return repr(float(v))


def _dict_to_xml(name, d, out, indent, top_ids, parent=None):
    typ = d.get("type")
    if typ == "ref":
        out.append(f'{indent}<ref id="{_esc(d["id"])}"' + (f' name="{_esc(name)}"' if name and name not in ("bsdf",) else "") + "/>")
        return
    if typ in ("rgb", "srgb", "spectrum"):
        v = d["value"]
        v = ", ".join(_fmt(x) for x in (v if hasattr(v, "__len__") else [v]))
        out.append(f'{indent}<rgb name="{_esc(name)}" value="{v}"/>')
        return
    if typ not in _TAGS:
        raise RuntimeError(f'load_dict(): unsupported plugin type "{typ}"')
    tag = _TAGS[typ]
    attrs = "" if tag == "scene" else f' type="{_esc(typ)}"'
    if tag == "scene":
        attrs += ' version="3.0.0"'
    if name is not None and tag != "scene":
        if indent == "    " and tag in ("bsdf", "medium", "texture", "shape", "emitter"):
            attrs += f' id="{_esc(name)}"'
        elif tag not in ("integrator", "sensor", "sampler", "film", "rfilter", "phase") and not (tag == "bsdf" and name == "bsdf") \
                and not (tag == "emitter" and name == "emitter"):
            attrs += f' name="{_esc(name)}"'
        elif tag == "integrator" and parent == "integrator":
            attrs += f' name="{_esc(name)}"'            # a nested integrator of `aov` / `moment`: the key names its channels (aov.cpp:115-125, moment.cpp:52-60)
    out.append(f"{indent}<{tag}{attrs}>")
    sub = indent + "    "
    for k, v in d.items():
        if k == "type":
            continue
        if isinstance(v, dict):
            _dict_to_xml(k, v, out, sub, top_ids, tag)
        elif isinstance(v, ScalarTransform4f):
            m = " ".join(_fmt(x) for x in v.matrix.reshape(-1))
            out.append(f'{sub}<transform name="{_esc(k)}"><matrix value="{m}"/></transform>')
        elif isinstance(v, bool):
            out.append(f'{sub}<boolean name="{_esc(k)}" value="{"true" if v else "false"}"/>')
        elif isinstance(v, (int, np.integer)):
            out.append(f'{sub}<integer name="{_esc(k)}" value="{int(v)}"/>')
        elif isinstance(v, (float, np.floating)):
            out.append(f'{sub}<float name="{_esc(k)}" value="{_fmt(v)}"/>')
        elif isinstance(v, str):
            out.append(f'{sub}<string name="{_esc(k)}" value="{_esc(v)}"/>')
        elif typ == "tabphase" and k == "values" and isinstance(v, (list, tuple, np.ndarray)):      # the plugin reads a string (tabphase.cpp:45-57)
            out.append(f'{sub}<string name="values" value="{", ".join(_fmt(x) for x in np.asarray(v).reshape(-1))}"/>')
        elif typ == "directional" and k == "direction" and isinstance(v, (list, tuple, np.ndarray)):    # a vector, not a colour (directional.cpp:75)
            out.append(f'{sub}<vector name="direction" value="{", ".join(_fmt(x) for x in np.asarray(v).reshape(-1))}"/>')
        elif isinstance(v, (list, tuple, np.ndarray)):
            out.append(f'{sub}<rgb name="{_esc(k)}" value="{", ".join(_fmt(x) for x in v)}"/>')
        else:
            raise RuntimeError(f'load_dict(): unsupported value for key "{k}": {type(v)}')
    out.append(f"{indent}</{tag}>")


def dict_to_xml(d):
    if d.get("type") != "scene":
        raise RuntimeError("load_dict(): the top-level dictionary must have type 'scene'")
    out = []
    # objects that are referenced must be declared before their first use
    refd = set()

    def scan(x):
        if isinstance(x, dict):
            if x.get("type") == "ref":
                refd.add(x["id"])
            for v in x.values():
                scan(v)
    scan(d)
    ordered = {"type": "scene"}
    for k, v in d.items():
        if k in refd:
            ordered[k] = v
    for k, v in d.items():
        if k not in ordered:
            ordered[k] = v
    _dict_to_xml(None, ordered, out, "", refd)
    return "\n".join(out)


# ------------------------------------------------------------------ scenes
class Scene:
    """Handle to a loaded scene (wraps `lrt_scene*`)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        self._lib = _lib.lib()

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                self._lib.lrt_scene_free(self._h)
                self._h = C.c_void_p(None)
        except Exception:
            pass

    # -- description -----------------------------------------------------
    @property
    def desc(self):
        return self._lib.lrt_scene_desc_get(self._h).contents

    def film_shape(self):
        f = self.desc.film
        return f.crop_height, f.crop_width, (4 if f.has_alpha else 3)

    def raw_channels(self):
        return 5 if self.desc.film.has_alpha else 4

    @property
    def spp(self):
        return self.desc.sample_count

    def medium_ids(self):
        d = self.desc
        return [d.media[i].id.decode() for i in range(d.n_media)]

    # -- the aov integrator ------------------------------------------------
    def aov_desc(self):
        """lrt_aov_desc of a scene loaded with an `aov` integrator, None for any other scene."""
        a = _lib.AovDesc()
        return a if self._lib.lrt_scene_aov_get(self._h, C.byref(a)) == _lib.OK else None

    def is_aov(self):
        return self.aov_desc() is not None

    def aov_channel_names(self):
        """Names of the channels render() returns on an aov scene: each nested integrator's <name>.R/.G/.B[/.A], then the AOVs'
        <name>.<suffix> (aov.cpp merge_channels)."""
        a = self.aov_desc()
        if a is None:
            raise RuntimeError("aov_channel_names(): the scene has no aov integrator")
        return [self._lib.lrt_aov_channel_name(self._h, c).decode() for c in range(a.n_channels)]

    def render_aov_samples(self, lane_begin, n, **kw):
        """lrt_render_aov_samples (test hook): the AOV values of lanes [lane_begin, lane_begin + n) of the AOV pass (its first
        pass), before film accumulation: (n, n_aov_channels) float32."""
        a = self.aov_desc()
        if a is None:
            raise RuntimeError("render_aov_samples(): the scene has no aov integrator")
        out = np.empty((n, a.n_aov_channels), dtype=np.float32)
        o = make_opts(None, None, None, None, kw.get("spp", 0), kw.get("seed", 0), 0, 1, kw.get("device", 0))
        _lib.check(self._lib.lrt_render_aov_samples(self._h, C.byref(o), int(lane_begin), int(n), out.ctypes.data))
        return out

    def _render_aov(self, a, spp, seed, integrator, max_depth, rr_depth, hide_emitters, tile_rank, tile_count, device, return_raw):
        f = self.desc.film
        img = np.empty((f.crop_height, f.crop_width, a.n_channels), dtype=np.float32)
        raw = np.empty((f.crop_height, f.crop_width, a.n_aov_channels + 1), dtype=np.float32) if return_raw else None
        o = make_opts(integrator, max_depth, rr_depth, hide_emitters, spp, seed, tile_rank, tile_count, device)
        _lib.check(self._lib.lrt_render_aov(self._h, C.byref(o), raw.ctypes.data if return_raw else None, img.ctypes.data))
        return (img, raw) if return_raw else img

    # -- the moment integrator ---------------------------------------------
    def moment_desc(self):
        """lrt_moment_desc of a scene loaded with a `moment` integrator, None for any other scene."""
        m = _lib.MomentDesc()
        return m if self._lib.lrt_scene_moment_get(self._h, C.byref(m)) == _lib.OK else None

    def is_moment(self):
        return self.moment_desc() is not None

    def moment_channel_names(self):
        """Names of the channels render() returns on a moment scene: R, G, B, [A], <name>.X/.Y/.Z, m2_<name>.X/.Y/.Z."""
        m = self.moment_desc()
        if m is None:
            raise RuntimeError("moment_channel_names(): the scene has no moment integrator")
        return [self._lib.lrt_moment_channel_name(self._h, c).decode() for c in range(m.n_channels)]

    def render_moment_samples(self, lane_begin, n, **kw):
        """lrt_render_moment_samples (test hook): X, Y, Z, m2_X, m2_Y, m2_Z of lanes [lane_begin, lane_begin + n) before film
        accumulation (first pass): (n, 6) float32."""
        if not self.is_moment():
            raise RuntimeError("render_moment_samples(): the scene has no moment integrator")
        out = np.empty((n, 6), dtype=np.float32)
        o = make_opts(None, None, None, None, kw.get("spp", 0), kw.get("seed", 0), 0, 1, kw.get("device", 0))
        _lib.check(self._lib.lrt_render_moment_samples(self._h, C.byref(o), int(lane_begin), int(n), out.ctypes.data))
        return out

    def _render_moment(self, m, spp, seed, integrator, max_depth, rr_depth, hide_emitters, tile_rank, tile_count, device, return_raw):
        f = self.desc.film
        img = np.empty((f.crop_height, f.crop_width, m.n_channels), dtype=np.float32)
        raw = np.empty((f.crop_height, f.crop_width, m.n_raw_channels), dtype=np.float32) if return_raw else None
        o = make_opts(integrator, max_depth, rr_depth, hide_emitters, spp, seed, tile_rank, tile_count, device)
        _lib.check(self._lib.lrt_render_moment(self._h, C.byref(o), raw.ctypes.data if return_raw else None, img.ctypes.data))
        return (img, raw) if return_raw else img

    def render_moment_to_device(self, film_ptr, image_ptr=None, **kw):
        """lrt_render_moment into caller-provided DEVICE buffers (n_raw_channels / n_channels floats per pixel)."""
        o = make_opts(None, None, None, None, kw.get("spp", 0), kw.get("seed", 0), kw.get("tile_rank", 0), kw.get("tile_count", 1), kw.get("device", 0), True)
        _lib.check(self._lib.lrt_render_moment(self._h, C.byref(o), C.c_void_p(film_ptr) if film_ptr else None, C.c_void_p(image_ptr) if image_ptr else None))

    # -- rendering ---------------------------------------------------------
    def render(self, spp=0, seed=0, integrator=None, max_depth=None, rr_depth=None, hide_emitters=None,
               tile_rank=0, tile_count=1, device=0, return_raw=False):
        """Developed H x W x (3|4) image; on a scene with an `aov` integrator H x W x n_channels (aov_channel_names()), and with
        return_raw the AOV pass's film (AOV channels, then W) as the second value; on a scene with a `moment` integrator
        H x W x n_channels (moment_channel_names()), and with return_raw the moment film (R,G,B,[A],W,X,Y,Z,m2X,m2Y,m2Z)."""
        a = self.aov_desc()
        if a is not None:
            return self._render_aov(a, spp, seed, integrator, max_depth, rr_depth, hide_emitters, tile_rank, tile_count, device, return_raw)
        m = self.moment_desc()
        if m is not None:
            return self._render_moment(m, spp, seed, integrator, max_depth, rr_depth, hide_emitters, tile_rank, tile_count, device, return_raw)
        h, w, c = self.film_shape()
        img = np.empty((h, w, c), dtype=np.float32)
        raw = np.empty((h, w, self.raw_channels()), dtype=np.float32) if return_raw else None
        o = make_opts(integrator, max_depth, rr_depth, hide_emitters, spp, seed, tile_rank, tile_count, device)
        _lib.check(self._lib.lrt_render(self._h, C.byref(o), raw.ctypes.data if return_raw else None, img.ctypes.data))
        return (img, raw) if return_raw else img

    def render_multi(self, devices, spp=0, seed=0, integrator=None, max_depth=None, rr_depth=None, hide_emitters=None, return_raw=False):
        """lrt_render_multi: one process, the image tile-sharded over `devices` (a list of HIP ordinals), films summed by one RCCL
        all-reduce, developed on the first device.  Same image as render()."""
        h, w, c = self.film_shape()
        img = np.empty((h, w, c), dtype=np.float32)
        raw = np.empty((h, w, self.raw_channels()), dtype=np.float32) if return_raw else None
        o = make_opts(integrator, max_depth, rr_depth, hide_emitters, spp, seed)
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        _lib.check(self._lib.lrt_render_multi(self._h, C.byref(o), len(devices), ids, raw.ctypes.data if return_raw else None, img.ctypes.data))
        return (img, raw) if return_raw else img

    def render_backward_multi(self, grad_image, devices, **kw):
        """lrt_render_backward_multi: the PRB adjoint sharded over `devices`, gradients reduced with one all-reduce."""
        g = np.ascontiguousarray(grad_image, dtype=np.float32)
        o = make_opts(kw.get("integrator"), kw.get("max_depth"), kw.get("rr_depth"), kw.get("hide_emitters"), kw.get("spp", 0), kw.get("seed", 0), grad_medium=kw.get("medium", -1))
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        out = _lib.ParamGrads()
        _lib.check(self._lib.lrt_render_backward_multi(self._h, C.byref(o), len(devices), ids, g.ctypes.data, C.byref(out)))
        return {"sigma_t": np.array(out.d_sigma_t[:], dtype=np.float32), "albedo": np.array(out.d_albedo[:], dtype=np.float32), "g": float(out.d_g)}

    def render_to_device(self, film_ptr, image_ptr=None, **kw):
        """Render into caller-provided DEVICE buffers (e.g. torch tensors' data_ptr())."""
        o = make_opts(kw.get("integrator"), kw.get("max_depth"), kw.get("rr_depth"), kw.get("hide_emitters"), kw.get("spp", 0),
                      kw.get("seed", 0), kw.get("tile_rank", 0), kw.get("tile_count", 1), kw.get("device", 0), True)
        _lib.check(self._lib.lrt_render(self._h, C.byref(o), C.c_void_p(film_ptr), C.c_void_p(image_ptr) if image_ptr else None))

    def develop(self, film_raw=None, film_ptr=None, image_ptr=None):
        if film_ptr is not None:
            _lib.check(self._lib.lrt_film_develop(self._h, C.c_void_p(film_ptr), C.c_void_p(image_ptr), 1))
            return None
        h, w, c = self.film_shape()
        film_raw = np.ascontiguousarray(film_raw, dtype=np.float32)
        img = np.empty((h, w, c), dtype=np.float32)
        _lib.check(self._lib.lrt_film_develop(self._h, film_raw.ctypes.data, img.ctypes.data, 0))
        return img

    def render_samples(self, lane_begin, n, **kw):
        out = np.empty((n, 4), dtype=np.float32)
        o = make_opts(kw.get("integrator"), kw.get("max_depth"), kw.get("rr_depth"), kw.get("hide_emitters"), kw.get("spp", 0),
                      kw.get("seed", 0), 0, 1, kw.get("device", 0))
        _lib.check(self._lib.lrt_render_samples(self._h, C.byref(o), int(lane_begin), int(n), out.ctypes.data))
        return out

    def render_backward(self, grad_image, **kw):
        """PRB adjoint.  `medium`: index of the medium whose sigma_t / albedo / g the gradients refer to; the default -1 sums the adjoint
        over all media into one parameter set (the round-1 meaning; lrt_render_opts.grad_medium in the C ABI, where a zero-initialised
        struct selects medium 0).
        grid=True (lrt_render_backward_grid): the dict also holds "sigma_t_data", the gradient w.r.t. the sigma_t grid of the
        heterogeneous medium `medium` (left out: the scene's only heterogeneous medium), float32 of shape (res_z, res_y, res_x) like
        the array write_volume_grid takes.  out=: a float32 CUDA torch tensor of that shape receives it without a host copy
        (grad_image may then be a tensor on that device as well) and is returned in the dict."""
        if kw.get("grid"):
            return self._render_backward_grid(grad_image, kw)
        if kw.get("out") is not None:
            raise TypeError("render_backward: out= goes with grid=True")
        g = np.ascontiguousarray(grad_image, dtype=np.float32)
        o = make_opts(kw.get("integrator"), kw.get("max_depth"), kw.get("rr_depth"), kw.get("hide_emitters"), kw.get("spp", 0),
                      kw.get("seed", 0), kw.get("tile_rank", 0), kw.get("tile_count", 1), kw.get("device", 0), grad_medium=kw.get("medium", -1))
        out = _lib.ParamGrads()
        _lib.check(self._lib.lrt_render_backward(self._h, C.byref(o), g.ctypes.data, C.byref(out)))
        return {"sigma_t": np.array(out.d_sigma_t[:], dtype=np.float32), "albedo": np.array(out.d_albedo[:], dtype=np.float32),
                "g": float(out.d_g)}

    def heterogeneous_media(self):
        """Indices (into desc.media) of the media with a sigma_t grid."""
        d = self.desc
        return [i for i in range(d.n_media) if d.media[i].type == _lib.MEDIUM["heterogeneous"]]

    def grid_shape(self, medium):
        """(res_z, res_y, res_x) of a heterogeneous medium's grid: the shape of the array write_volume_grid takes."""
        r = self.desc.media[medium].grid_res
        return (int(r[2]), int(r[1]), int(r[0]))

    def _render_backward_grid(self, grad_image, kw):
        m = kw.get("medium")
        if m is None or m < 0:
            het = self.heterogeneous_media()
            if len(het) != 1:
                raise RuntimeError(f"render_backward(grid=True): the scene holds {len(het)} heterogeneous media; name one with medium=")
            m = het[0]
        if not 0 <= m < self.desc.n_media or m not in self.heterogeneous_media():
            shape = None                               # the library reports the cause
        else:
            shape = self.grid_shape(m)
        out_t = kw.get("out")
        on_device = out_t is not None
        h, w, c = self.film_shape()
        if on_device:
            import torch
            if not _is_torch(out_t) or not out_t.is_cuda or out_t.dtype != torch.float32 or not out_t.is_contiguous() or (shape is not None and tuple(out_t.shape) != shape):
                raise RuntimeError(f"render_backward(grid=True): out must be a contiguous float32 CUDA tensor of shape {shape}")
            dev = out_t.device.index or 0
            if kw.get("device", dev) != dev:
                raise RuntimeError(f"render_backward(grid=True): out lives on {out_t.device}, the render was asked for device {kw['device']}")
            g = grad_image if _is_torch(grad_image) else torch.from_numpy(np.ascontiguousarray(grad_image, dtype=np.float32))
            g = g.to(device=out_t.device, dtype=torch.float32).contiguous()
            if g.numel() != h * w * c:
                raise RuntimeError(f"render_backward: grad_image has {g.numel()} values, the image {h * w * c}")
            torch.cuda.current_stream(out_t.device).synchronize()     # the library works on a stream of its own
            g_ptr, d_ptr, res = g.data_ptr(), out_t.data_ptr(), out_t
        else:
            g = np.ascontiguousarray(grad_image, dtype=np.float32)
            if g.size != h * w * c:
                raise RuntimeError(f"render_backward: grad_image has {g.size} values, the image {h * w * c}")
            res = np.empty(shape if shape is not None else (1,), dtype=np.float32)
            g_ptr, d_ptr, dev = g.ctypes.data, res.ctypes.data, kw.get("device", 0)
        o = make_opts(kw.get("integrator"), kw.get("max_depth"), kw.get("rr_depth"), kw.get("hide_emitters"), kw.get("spp", 0),
                      kw.get("seed", 0), kw.get("tile_rank", 0), kw.get("tile_count", 1), dev, on_device, grad_medium=m)
        out = _lib.ParamGrads()
        _lib.check(self._lib.lrt_render_backward_grid(self._h, C.byref(o), C.c_void_p(g_ptr), C.byref(out), C.c_void_p(d_ptr)))
        return {"sigma_t": np.array(out.d_sigma_t[:], dtype=np.float32), "albedo": np.array(out.d_albedo[:], dtype=np.float32),
                "g": float(out.d_g), "sigma_t_data": res}

    def primary_entry(self, device=0):
        """The per-pixel primary entry of the device image (lrt_primary_entry_get): uint16 (crop_h, crop_w); all zero when the image has no table."""
        h, w, _ = self.film_shape()
        out = np.zeros((h, w), dtype=np.uint16)
        _lib.check(self._lib.lrt_primary_entry_get(self._h, out.ctypes.data, h * w, device))
        return out

    def stats(self):
        s = _lib.RenderStats()
        _lib.check(self._lib.lrt_render_stats_get(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.RenderStats._fields_}

    def trace(self, o, d, tmax=None, any_hit=False):
        o = np.ascontiguousarray(o, dtype=np.float32); d = np.ascontiguousarray(d, dtype=np.float32)
        n = o.shape[0]
        tmax = np.full(n, np.finfo(np.float32).max, dtype=np.float32) if tmax is None else np.ascontiguousarray(tmax, dtype=np.float32)
        cols = [np.ascontiguousarray(a) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tmax)]
        t = np.empty(n, np.float32); u = np.empty(n, np.float32); v = np.empty(n, np.float32); prim = np.empty(n, np.uint32)
        FP = C.POINTER(C.c_float)
        rays = _lib.RaysSoA(*[c.ctypes.data_as(FP) for c in cols])
        hits = _lib.HitsSoA(t.ctypes.data_as(FP), u.ctypes.data_as(FP), v.ctypes.data_as(FP), prim.ctypes.data_as(C.POINTER(C.c_uint32)))
        _lib.check(self._lib.lrt_trace(self._h, C.byref(rays), C.byref(hits), n, int(any_hit)))
        return t, u, v, prim

    def _probe(self, name, inputs, out_width, alloc=np.empty, medium=None, device=0):
        """One call of the test hook lrt_<name>.  inputs: (argument name, array, floats per lane, dtype) in the C function's order;
        returns the raw n x out_width block, allocated with `alloc`."""
        cols = [np.ascontiguousarray(a, dtype=dt).reshape(-1, w) for _, a, w, dt in inputs]
        n = cols[0].shape[0]
        if any(c.shape[0] != n for c in cols):
            names = [i[0] for i in inputs]
            raise ValueError("%s: %s and %s must have the same number of rows" % (name, ", ".join(names[:-1]), names[-1]))
        out = alloc((n, out_width), dtype=np.float32)
        ptr = lambda a: a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))
        _lib.check(getattr(self._lib, "lrt_" + name)(self._h, *([] if medium is None else [int(medium)]), *map(ptr, cols), n, ptr(out), int(device)))
        return out

    def emitter_probe(self, ref_p, sample, device=0):
        """lrt_emitter_probe (test hook): the device's Scene::sample_emitter_direction at ref_p (n x 3) with sample (n x 2), then a ray
        query along the sampled direction and the integrators' emitter pdf / emission at its hit.  Returns a dict of arrays:
        p, n, d (n x 3), dist, pdf, weight (n x 3), emitter (int), hit_shape (int, -1: miss), hit_pdf, hit_le (n x 3)."""
        out = self._probe("emitter_probe", [("ref_p", ref_p, 3, np.float32), ("sample", sample, 2, np.float32)], _lib.PROBE_FLOATS, device=device)
        return {"p": out[:, 0:3], "n": out[:, 3:6], "d": out[:, 6:9], "dist": out[:, 9], "pdf": out[:, 10], "weight": out[:, 11:14],
                "emitter": out[:, 14].astype(np.int32), "hit_shape": out[:, 15].astype(np.int32), "hit_pdf": out[:, 16], "hit_le": out[:, 17:20]}

    def envmap_probe(self, directions, device=0):
        """lrt_envmap_probe (test hook): the environment emitter at world directions (n x 3), as the integrators evaluate it for a
        ray that leaves the scene.  Returns (pdf (n), radiance (n x 3)): Scene::pdf_emitter_direction of the miss, the emitter's eval."""
        out = self._probe("envmap_probe", [("directions", directions, 3, np.float32)], 4, device=device)
        return out[:, 0].copy(), out[:, 1:4].copy()

    def phase_probe(self, medium, wi, sample, wo_query, device=0):
        """lrt_phase_probe (test hook): the phase function of medium `medium` (an index into desc.media) as the EXT render kernels call it,
        per lane: PhaseFunction::sample(wi, sample = (s1, s2x, s2y)) and eval_pdf(wi, wo_query) (n x 3 each).  Returns a dict of arrays:
        wo (n x 3), weight, pdf, eval, eval_pdf (n each)."""
        out = self._probe("phase_probe", [("wi", wi, 3, np.float32), ("sample", sample, 3, np.float32), ("wo_query", wo_query, 3, np.float32)],
                          _lib.PHASE_PROBE_FLOATS, np.zeros, medium, device)
        return {"wo": out[:, 0:3], "weight": out[:, 3], "pdf": out[:, 4], "eval": out[:, 5], "eval_pdf": out[:, 6]}

    def medium_probe(self, medium, o, d, maxt, sample, channel, device=0):
        """lrt_medium_probe (test hook): free-flight sampling in medium `medium` (an index into desc.media) as the volume integrators call
        it, per lane: Medium::sample_interaction(ray(o, d, maxt), sample, channel) (o, d: n x 3; maxt, sample, channel: n).  A lane with
        maxt = NaN evaluates the grid at the local point o alone.  Returns a dict of arrays: valid (bool), t, p, mint, sigma_t, sigma_s,
        sigma_n, combined (n x 3 each), local (n x 3), grid, and raw (n x LRT_MEDIUM_PROBE_FLOATS, every float as returned)."""
        out = self._probe("medium_probe", [("o", o, 3, np.float32), ("d", d, 3, np.float32), ("maxt", maxt, 1, np.float32), ("sample", sample, 1, np.float32),
                                           ("channel", channel, 1, np.uint32)], _lib.MEDIUM_PROBE_FLOATS, np.zeros, medium, device)
        return _lib.medium_probe_fields(out)

    def sensor_probe(self, inputs, device=0):
        """lrt_sensor_probe (test hook): per lane (inputs: n x 5 = ax, ay, spx, spy, x) the sensor's ray at the adjusted position sample
        (ax, ay), the film-to-sample map and the filter footprint of a sample at the film position (spx, spy), and the reconstruction filter
        at x.  Returns a dict of arrays: o, d (n x 3), maxt, adjusted (n x 2), origin (n x 2, int), rel (n x 2), weight, fcount (int), and
        raw (n x LRT_SENSOR_PROBE_FLOATS, every float as returned)."""
        return _lib.sensor_probe_fields(self._probe("sensor_probe", [("inputs", inputs, 5, np.float32)], _lib.SENSOR_PROBE_FLOATS, np.zeros, device=device))

    def bsdf_probe(self, o, d, sample, wo_query, device=0):
        """lrt_bsdf_probe (test hook): per ray (o, d) (n x 3 each) the closest hit without a ray offset, its surface interaction, the hit
        shape's BSDF sampled with sample (n x 3: s1, s2.x, s2.y) as the integrators do, and its eval / pdf at the world direction
        wo_query (n x 3).  Returns a dict of arrays: shape (int, -1: miss), t, p, n, sh_n, uv, wi (local), wo (world), wo_z (local),
        pdf, eta, type (int), weight, eval, eval_pdf, and raw (n x LRT_BSDF_PROBE_FLOATS, every float as returned)."""
        out = self._probe("bsdf_probe", [("o", o, 3, np.float32), ("d", d, 3, np.float32), ("sample", sample, 3, np.float32), ("wo_query", wo_query, 3, np.float32)],
                          _lib.BSDF_PROBE_FLOATS, device=device)
        return _lib.bsdf_probe_fields(out)

    # -- parameters (mi.traverse) -------------------------------------------
    def param_set(self, key, value):
        """lrt_param_set.  "<id>.sigma_t.data" takes an array of shape (res_z, res_y, res_x) (or its flattening)."""
        v = np.ascontiguousarray(np.atleast_1d(np.asarray(value, dtype=np.float32))).reshape(-1)
        _lib.check(self._lib.lrt_param_set(self._h, key.encode(), v.ctypes.data_as(C.POINTER(C.c_float)), int(v.size)))

    def param_get(self, key, n=3):
        """lrt_param_get.  "<id>.sigma_t.data" returns the grid as (res_z, res_y, res_x), whatever n says."""
        if key.endswith(".sigma_t.data"):
            ids = self.medium_ids(); mid = key[:-len(".sigma_t.data")]
            if mid in ids and ids.index(mid) in self.heterogeneous_media():
                shape = self.grid_shape(ids.index(mid))
                v = np.zeros(shape, dtype=np.float32)
                _lib.check(self._lib.lrt_param_get(self._h, key.encode(), v.ctypes.data_as(C.POINTER(C.c_float)), int(v.size)))
                return v
        v = np.zeros(n, dtype=np.float32)
        _lib.check(self._lib.lrt_param_get(self._h, key.encode(), v.ctypes.data_as(C.POINTER(C.c_float)), n))
        return v


def math_eval(fn, x, y=None, device=0):
    """lrt_math_eval (test hook): the device's transcendental kernels, one value per lane.  Returns (out, out2)."""
    L = _lib.lib()
    x = np.ascontiguousarray(x, np.float32); y = x if y is None else np.ascontiguousarray(y, np.float32)
    out = np.empty_like(x); out2 = np.empty_like(x)
    FP = C.POINTER(C.c_float)
    _lib.check(L.lrt_math_eval(int(fn), x.ctypes.data_as(FP), y.ctypes.data_as(FP), x.size, out.ctypes.data_as(FP), out2.ctypes.data_as(FP), int(device)))
    return out, out2


class SceneParameters(dict):
    """mi.traverse(scene): dict of differentiable medium parameters; assignments are pushed by update()."""

    def __init__(self, scene):
        super().__init__()
        self._scene = scene
        for mid in scene.medium_ids():
            super().__setitem__(f"{mid}.sigma_t.value", scene.param_get(f"{mid}.sigma_t.value", 3))
            super().__setitem__(f"{mid}.albedo.value", scene.param_get(f"{mid}.albedo.value", 3))
            super().__setitem__(f"{mid}.scale", scene.param_get(f"{mid}.scale", 1))
            super().__setitem__(f"{mid}.phase_function.g", scene.param_get(f"{mid}.phase_function.g", 1))
        for i in range(scene.desc.n_media):                   # `parenchyma` also traverses its absorbers (src/media/parenchyma.cpp:154-160)
            m = scene.desc.media[i]
            if m.type == _lib.MEDIUM["parenchyma"]:
                mid = m.id.decode()
                for k in ("sigma_blood.value", "sigma_bile.value", "sigma_lipid_water.value"):
                    super().__setitem__(f"{mid}.{k}", scene.param_get(f"{mid}.{k}", 3))
                super().__setitem__(f"{mid}.sigma_hepatocity", scene.param_get(f"{mid}.sigma_hepatocity", 1))
            if m.type == _lib.MEDIUM["heterogeneous"]:          # the grid volume's values (src/volumes/grid.cpp traverse), as (res_z, res_y, res_x)
                super().__setitem__(f"{m.id.decode()}.sigma_t.data", scene.param_get(f"{m.id.decode()}.sigma_t.data"))
        self._dirty = set()

    def __setitem__(self, k, v):
        if k not in self:
            raise KeyError(k)
        a = np.atleast_1d(np.asarray(v, dtype=np.float32))
        if k.endswith(".sigma_t.data"):
            if a.size != self[k].size:
                raise ValueError(f"{k}: expected {self[k].shape} (res_z, res_y, res_x), got {a.shape}")
            a = a.reshape(self[k].shape)
        super().__setitem__(k, a)
        self._dirty.add(k)

    def update(self, values=None):
        if values:
            for k, v in values.items():
                self[k] = v
        for k in sorted(self._dirty):
            if k.endswith(".phase_function.g") and float(self[k][0]) == 0.0:
                try:                                   # g = 0 is a value of an hg phase function; an isotropic one has no such key
                    self._scene.param_set(k, self[k])
                except RuntimeError as e:
                    if "isotropic" not in str(e): raise
                continue
            self._scene.param_set(k, self[k])
        self._dirty.clear()


def traverse(scene):
    return SceneParameters(scene)


def write_volume_grid(path, data, bbox_min=(0.0, 0.0, 0.0), bbox_max=(1.0, 1.0, 1.0)):
    """mi.VolumeGrid(array).write(path) (src/render/volumegrid.cpp:94-118): a one-channel float32 grid, array shape
    (res_z, res_y, res_x), as the version-3 ".vol" file `gridvolume` reads."""
    import struct
    a = np.ascontiguousarray(data, dtype=np.float32)
    if a.ndim != 3:
        raise ValueError("write_volume_grid: expected an array of shape (res_z, res_y, res_x)")
    with open(path, "wb") as f:
        f.write(b"VOL" + struct.pack("<B", 3) + struct.pack("<iiiii", 1, a.shape[2], a.shape[1], a.shape[0], 1))
        f.write(struct.pack("<6f", *bbox_min, *bbox_max))
        f.write(a.tobytes())


def _defines(kw):
    arr = (C.c_char_p * len(kw))(*[f"{k}={v}".encode() for k, v in kw.items()])
    return arr, len(kw)


def load_file(path, **defines):
    """mi.load_file(path, **defines): `defines` replace `$name` parameters (like `-Dname=value`)."""
    L = _lib.lib()
    h = C.c_void_p()
    arr, n = _defines(defines)
    _lib.check(L.lrt_scene_load_xml(os.fspath(path).encode(), arr, n, C.byref(h)))
    return Scene(h.value)


def load_string(xml, base_dir=".", **defines):
    L = _lib.lib()
    h = C.c_void_p()
    arr, n = _defines(defines)
    _lib.check(L.lrt_scene_load_xml_string(xml.encode(), os.fspath(base_dir).encode(), arr, n, C.byref(h)))
    return Scene(h.value)


def load_dict(d, base_dir="."):
    return load_string(dict_to_xml(d), base_dir)


def render(scene, spp=0, seed=0, integrator=None, **kw):
    """mi.render(scene, spp=..., seed=...): developed H x W x (3|4) float32 image (an aov scene: H x W x n_channels, the inner
    images then the AOVs, channel names from scene.aov_channel_names(); a moment scene: R,G,B,[A] then the XYZ means and second
    moments, scene.moment_channel_names())."""
    return scene.render(spp=spp, seed=seed, integrator=integrator, **kw)


def render_stats(scene):
    return scene.stats()


def scene_from_buffers(positions, faces, normals=None, texcoords=None, reflectance=(0.5, 0.5, 0.5), film=(64, 64),
                       sensor_to_world=None, fov=45.0, spp=4, integrator="path", max_depth=-1, constant_radiance=None,
                       area_radiance=None, flip_normals=False):
    """Build a one-mesh scene from raw buffers through `lrt_scene_from_desc` (the "from buffers" entry of the C ABI).
    The mesh gets a diffuse BSDF; an optional constant environment emitter lights it, and `area_radiance` makes the mesh
    itself an area emitter of that radiance."""
    L = _lib.lib()
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
    nv, nf = pos.shape[0], fc.shape[0]
    nrm = np.zeros((nv, 3), np.float32) if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    uv = np.zeros((nv, 2), np.float32) if texcoords is None else np.ascontiguousarray(texcoords, dtype=np.float32).reshape(-1, 2)
    fshape = np.zeros(nf, np.uint32)
    FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    shape = _lib.ShapeDesc(kind=0, first_face=0, n_faces=nf, bsdf=0, emitter=-1, interior_medium=-1, exterior_medium=-1,
                           has_normals=int(normals is not None), has_texcoords=int(texcoords is not None), flip_normals=int(bool(flip_normals)))
    shape.to_world[:] = list(np.eye(4, dtype=np.float32).reshape(-1))
    tex = _lib.TextureDesc(type=0, width=0, height=0, channels=0)
    tex.color0[:] = list(reflectance); tex.color1[:] = list(reflectance); tex.to_uv[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    bsdf = _lib.BsdfDesc(type=0, reflectance=0, eta=1.0, nested=-1, texture=-1, scale=1.0)
    d = _lib.SceneDesc()
    d.n_vertices, d.n_faces, d.n_shapes, d.n_bsdfs, d.n_textures, d.n_media = nv, nf, 1, 1, 1, 0
    d.positions, d.normals, d.texcoords = pos.ctypes.data_as(FP), nrm.ctypes.data_as(FP), uv.ctypes.data_as(FP)
    d.faces, d.face_shape = fc.ctypes.data_as(UP), fshape.ctypes.data_as(UP)
    d.shapes, d.bsdfs, d.textures = C.pointer(shape), C.pointer(bsdf), C.pointer(tex)
    ems = []
    if area_radiance is not None:
        area = _lib.EmitterDesc(type=0, shape=0, scale=1.0)
        area.radiance[:] = list(area_radiance); area.to_world[:] = list(np.eye(4, dtype=np.float32).reshape(-1))
        shape.emitter = len(ems); ems.append(area)
    if constant_radiance is not None:
        em = _lib.EmitterDesc(type=2, shape=-1, scale=1.0)
        em.radiance[:] = list(constant_radiance); em.to_world[:] = list(np.eye(4, dtype=np.float32).reshape(-1))
        ems.append(em)
    em_arr = (_lib.EmitterDesc * max(len(ems), 1))(*ems)
    if ems:
        d.n_emitters, d.emitters = len(ems), C.cast(em_arr, C.POINTER(_lib.EmitterDesc))
    tw = ScalarTransform4f() if sensor_to_world is None else sensor_to_world
    d.sensor.to_world[:] = [float(x) for x in np.asarray(tw.matrix, dtype=np.float32).reshape(-1)]
    d.sensor.fov_x, d.sensor.near_clip, d.sensor.far_clip, d.sensor.medium = fov, 1e-2, 1e4, -1
    d.film.width, d.film.height = film; d.film.crop_width, d.film.crop_height = film
    d.film.has_alpha, d.film.rfilter, d.film.rfilter_param = 0, 0, 0.5
    d.integrator.type, d.integrator.max_depth, d.integrator.rr_depth, d.integrator.hide_emitters = _lib.INTEGRATOR[integrator], max_depth, 5, 0
    d.use_spectral_mis = 1
    d.sample_count, d.sampler_seed = spp, 0
    h = C.c_void_p()
    _lib.check(L.lrt_scene_from_desc(C.byref(d), C.byref(h)))
    return Scene(h.value)


def read_image(path):
    """mi.Bitmap(path) as a float32 array (h, w, channels); PNG values are in [0, 1] as stored."""
    L = _lib.lib()
    w, h, c = C.c_int(), C.c_int(), C.c_int(); data = C.POINTER(C.c_float)()
    _lib.check(L.lrt_image_read(os.fspath(path).encode(), C.byref(w), C.byref(h), C.byref(c), C.byref(data)))
    try:
        return np.ctypeslib.as_array(data, (h.value, w.value, c.value)).copy()
    finally:
        L.lrt_image_free(data)


def _read_image_named(path):
    """lrt_image_read_named: (array, channel names or None).  An EXR gives every channel of the file."""
    L = _lib.lib()
    w, h, c = C.c_int(), C.c_int(), C.c_int(); data = C.POINTER(C.c_float)(); names = C.c_void_p()
    _lib.check(L.lrt_image_read_named(os.fspath(path).encode(), C.byref(w), C.byref(h), C.byref(c), C.byref(data), C.byref(names)))
    try:
        joined = C.string_at(names.value).decode() if names.value else ""
        return np.ctypeslib.as_array(data, (h.value, w.value, c.value)).copy(), (joined.split("\n") if joined else None)
    finally:
        L.lrt_image_free(data); L.lrt_image_free_names(names)


def write_png(path, image):
    """8-bit sRGB PNG of a linear float image (LiverRenderer.py:383-385: Bitmap.convert(RGBA, UInt8, srgb_gamma=True))."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    if img.ndim == 2:
        img = img[..., None]
    _lib.check(_lib.lib().lrt_image_write_png(os.fspath(path).encode(), img.shape[1], img.shape[0], img.shape[2], img.ctypes.data))


def write_exr(path, image, channel_names=None):
    """Uncompressed float32 EXR.  Without `channel_names`: 1, 3 or 4 channels named Y / R,G,B / R,G,B,A.  With them (one name per
    channel, e.g. scene.aov_channel_names()): any number of channels, written sorted by name as OpenEXR requires."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    if img.ndim == 2:
        img = img[..., None]
    if channel_names is None:
        _lib.check(_lib.lib().lrt_image_write_exr(os.fspath(path).encode(), img.shape[1], img.shape[0], img.shape[2], img.ctypes.data))
        return
    names = [str(n) for n in channel_names]
    if len(names) != img.shape[2]:
        raise ValueError(f"write_exr: {len(names)} channel names for an image of {img.shape[2]} channels")
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    _lib.check(_lib.lib().lrt_image_write_exr_channels(os.fspath(path).encode(), img.shape[1], img.shape[0], img.shape[2], arr, img.ctypes.data))


# ---- the handful of image-side names the reference's drivers use (MitsubaRunner.py:166-167, LiverRenderer.py:383-385),
# so that those scripts run with the import swapped: mi.Bitmap(path | array), Bitmap.convert(RGBA, UInt8, srgb_gamma=True),
# mi.util.write_bitmap(path, image).  Arrays stay float32 and linear; the sRGB / 8-bit conversion happens in the writer.
class Struct:
    class Type:
        UInt8, Float16, Float32 = "uint8", "float16", "float32"


class Bitmap:
    class PixelFormat:
        Y, YA, RGB, RGBA = "y", "ya", "rgb", "rgba"

    def __init__(self, src, pixel_format=None, component_format=None, srgb_gamma=None, channel_names=None):
        """mi.Bitmap(path) | mi.Bitmap(array, channel_names=[...]) | mi.Bitmap(bitmap, pixel_format, component_format, srgb_gamma)
        (the converting constructor Denoise.py uses).  `channel_names` (one per channel, e.g. scene.aov_channel_names()) makes
        the bitmap a multi-channel one; a file's own names are kept (EXR: every channel of the file, R,G,B[,A] first)."""
        if isinstance(src, Bitmap):
            b = src.convert(pixel_format, component_format, srgb_gamma) if (pixel_format or component_format or srgb_gamma is not None) else src
            self.data, self.component_format, self.srgb_gamma, self.channel_names = b.data, b.component_format, b.srgb_gamma, b.channel_names
            return
        names = None
        if isinstance(src, (str, os.PathLike)):
            self.data, names = _read_image_named(src)
        else:
            self.data = np.asarray(src, dtype=np.float32)
        if self.data.ndim == 2:
            self.data = self.data[..., None]
        if channel_names is not None:
            names = [str(n) for n in channel_names]
            if len(names) != self.data.shape[2]:
                raise ValueError(f"Bitmap: {len(names)} channel names for an image of {self.data.shape[2]} channels")
        self.channel_names = names
        self.component_format, self.srgb_gamma = Struct.Type.Float32, False

    def select(self, prefix="<root>"):
        """The H x W x (3|4) image a channel name selects, as OptixDenoiser's bitmap form reads its inputs: a prefix selects
        <prefix>.R/.G/.B or <prefix>.X/.Y/.Z; "<root>" selects R, G, B[, A], or the first three or four channels of a bitmap
        without names (the first three when it has five or more)."""
        names, d = self.channel_names, self.data
        if prefix == "<root>":
            if not names:
                n = d.shape[2] if d.shape[2] in (3, 4) else 3
                if d.shape[2] < 3:
                    raise RuntimeError(f"Bitmap.select: \"<root>\" needs at least 3 channels, the bitmap has {d.shape[2]}")
                return np.ascontiguousarray(d[..., :n])
            want = ["R", "G", "B"] + (["A"] if "A" in names else [])
        else:
            if not names:
                raise RuntimeError(f"Bitmap.select: channel \"{prefix}\" requested from a bitmap without channel names")
            want = next(([f"{prefix}.{c}" for c in sfx] for sfx in ("RGB", "XYZ") if all(f"{prefix}.{c}" in names for c in sfx)), None)
            if want is None:
                raise RuntimeError(f"Bitmap.select: no channels \"{prefix}.R/.G/.B\" or \"{prefix}.X/.Y/.Z\" among {names}")
        missing = [n for n in want if n not in names]
        if missing:
            raise RuntimeError(f"Bitmap.select: no channel {missing} among {names}")
        return np.ascontiguousarray(d[..., [names.index(n) for n in want]])

    def size(self):
        return (self.data.shape[1], self.data.shape[0])

    def channel_count(self):
        return self.data.shape[2]

    def convert(self, pixel_format=None, component_format=None, srgb_gamma=None):
        """src/core/bitmap.cpp Bitmap::convert, for the conversions the drivers request: channel layout now, the transfer
        function and the quantisation when the bitmap is written."""
        d, out = self.data, Bitmap.__new__(Bitmap)
        n = {"y": 1, "ya": 2, "rgb": 3, "rgba": 4}.get(pixel_format, d.shape[2])
        if n != d.shape[2]:
            rgb = d[..., :3] if d.shape[2] >= 3 else np.repeat(d[..., :1], 3, axis=2)
            alpha = d[..., -1:] if d.shape[2] in (2, 4) else np.ones_like(d[..., :1])
            lum = (0.212671 * rgb[..., :1] + 0.715160 * rgb[..., 1:2] + 0.072169 * rgb[..., 2:3])
            d = {1: lum, 2: np.concatenate([lum, alpha], 2), 3: rgb, 4: np.concatenate([rgb, alpha], 2)}[n]
        out.data = np.ascontiguousarray(d, dtype=np.float32)
        out.channel_names = self.channel_names if n == self.data.shape[2] else None
        out.component_format = component_format or self.component_format
        out.srgb_gamma = self.srgb_gamma if srgb_gamma is None else bool(srgb_gamma)
        return out

    def write(self, path):
        util.write_bitmap(path, self)

    def __array__(self, dtype=None):
        return self.data if dtype is None else self.data.astype(dtype)


class util:
    @staticmethod
    def write_bitmap(path, image, write_async=False):
        """src/python/python/util.py write_bitmap: 8-bit formats get the sRGB transfer function, EXR stays linear float."""
        data = image.data if isinstance(image, Bitmap) else np.asarray(image, dtype=np.float32)
        if os.fspath(path).lower().endswith(".png"):
            write_png(path, data)
        elif os.fspath(path).lower().endswith(".exr"):
            names = image.channel_names if isinstance(image, Bitmap) else None
            plain = names is None or names in (["Y"], ["R", "G", "B"], ["R", "G", "B", "A"])
            write_exr(path, data, None if plain else names)
        else:
            raise RuntimeError(f"write_bitmap: unsupported file format \"{path}\" (supported: .png, .exr)")

    cornell_box = staticmethod(lambda: cornell_box())


# ---- mi.OptixDenoiser (include/mitsuba/render/optixdenoiser.h): the denoising step of Denoise.py and of --imode optix.  OptiX's
# network is closed and NVIDIA-only; behind the same interface runs the guided A-Trous wavelet filter of DESIGN.md section 9,
# in the HIP kernels of csrc/kernels_denoise.h.
def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


class Denoiser:
    """mi.Denoiser(input_size, albedo=False, normals=False, temporal=False, denoise_alpha=False, **params); mi.OptixDenoiser is
    the same class (argument order of optixdenoiser.h:57-59).  input_size is (width, height), e.g. Bitmap.size().  `params`:
    iterations (1 .. 8), sigma_color, sigma_normal, sigma_albedo, eps_a (all positive; left out: the library's defaults) and
    device.  The workspace and a stream of its own are allocated here and live as long as the object."""

    PARAMS = ("iterations", "sigma_color", "sigma_normal", "sigma_albedo", "eps_a")

    def __init__(self, input_size, albedo=False, normals=False, temporal=False, denoise_alpha=False, device=0, **params):
        self._h = None
        if temporal:
            raise RuntimeError("Denoiser: temporal denoising is unsupported (it needs an optical flow, which no AOV of this back-end produces)")
        unknown = sorted(set(params) - set(self.PARAMS))
        if unknown:
            raise TypeError(f"Denoiser: unknown parameter(s) {unknown} (known: {list(self.PARAMS)})")
        size = tuple(int(v) for v in input_size)
        if len(size) != 2:
            raise ValueError("Denoiser: input_size is (width, height)")
        prm = _lib.DenoiseParams()
        for k, v in params.items():
            if v is None:
                continue
            if k == "iterations":
                if int(v) != v or not 1 <= int(v) <= 8:
                    raise ValueError(f"Denoiser: iterations {v!r} outside 1 .. 8")
                prm.iterations = int(v)
            else:
                if not (float(v) > 0.0 and math.isfinite(float(v))):      # 0 would select the default in lrt_denoise_params
                    raise ValueError(f"Denoiser: {k} must be positive and finite, got {v!r}")
                setattr(prm, k, float(v))
        self._lib = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._lib.lrt_denoiser_create(size[0], size[1], int(bool(albedo)), int(bool(normals)), int(bool(denoise_alpha)),
                                                 C.byref(prm), int(device), C.byref(h)))
        self._h = h.value
        self.input_size, self.albedo, self.normals, self.denoise_alpha, self.device = size, bool(albedo), bool(normals), bool(denoise_alpha), int(device)
        got = _lib.DenoiseParams()
        _lib.check(self._lib.lrt_denoiser_get(self._h, None, None, C.byref(got)))
        self.params = {k: getattr(got, k) for k in self.PARAMS}

    def __del__(self):
        try:
            if self._h:
                self._lib.lrt_denoiser_free(self._h); self._h = None
        except Exception:
            pass

    def __repr__(self):
        return f"Denoiser[input_size={self.input_size}, albedo={self.albedo}, normals={self.normals}, denoise_alpha={self.denoise_alpha}, params={self.params}]"

    def __call__(self, noisy, albedo=None, normals=None, to_sensor=None, flow=None, previous_denoised=None, noisy_ch="<root>",
                 albedo_ch=None, normals_ch=None, flow_ch="", previous_denoised_ch=""):
        """Array form (optixdenoiser.h:112-117): denoiser(noisy, albedo=None, normals=None, to_sensor=None, flow=None,
        previous_denoised=None) with H x W x (3|4) `noisy` and H x W x 3 guides, float32.  numpy arrays in: a numpy array out.
        torch tensors on the GPU in: a tensor on the same device out, without a host copy (the current torch stream is
        synchronised first: the library works on a stream of its own).
        Bitmap form (optixdenoiser.h:173-179): denoiser(bitmap, albedo_ch="", normals_ch="", to_sensor=None, flow_ch="",
        previous_denoised_ch="", noisy_ch="<root>") reads its inputs from the channels of one multi-channel Bitmap
        (Bitmap.select) and returns a Bitmap.
        `to_sensor` is accepted and ignored: the filter uses only differences of normals, whose lengths a rotation does not
        change.  `flow` / `previous_denoised` belong to temporal denoising, which is unsupported."""
        if isinstance(noisy, Bitmap):
            a_ch = albedo_ch if albedo_ch is not None else (albedo if isinstance(albedo, str) else "")
            n_ch = normals_ch if normals_ch is not None else (normals if isinstance(normals, str) else "")
            if (albedo is not None and not isinstance(albedo, str)) or (normals is not None and not isinstance(normals, str)):
                raise TypeError("Denoiser: with a Bitmap the guides are channel names of that bitmap (albedo_ch, normals_ch)")
            if flow_ch or previous_denoised_ch or isinstance(flow, str) and flow or isinstance(previous_denoised, str) and previous_denoised:
                raise RuntimeError("Denoiser: temporal denoising is unsupported (flow_ch / previous_denoised_ch)")
            if self.albedo and not a_ch:
                raise RuntimeError("Denoiser: the denoiser was created with the albedo guide, but no albedo_ch was given")
            if self.normals and not n_ch:
                raise RuntimeError("Denoiser: the denoiser was created with the normals guide, but no normals_ch was given")
            out = self(noisy.select(noisy_ch), noisy.select(a_ch) if a_ch else None, noisy.select(n_ch) if n_ch else None)
            return Bitmap(out)
        if albedo_ch is not None or normals_ch is not None:
            raise TypeError("Denoiser: albedo_ch / normals_ch go with a Bitmap input")
        if flow is not None or previous_denoised is not None:
            raise RuntimeError("Denoiser: temporal denoising is unsupported (flow / previous_denoised)")
        w, h = self.input_size
        if _is_torch(noisy):
            return self._call_torch(noisy, albedo, normals)

        def arr(x, name, channels):
            a = np.ascontiguousarray(x, dtype=np.float32)
            if a.ndim != 3 or a.shape[0] != h or a.shape[1] != w or a.shape[2] not in channels:
                raise RuntimeError(f"Denoiser: {name} has shape {tuple(a.shape)}, expected ({h}, {w}, {' | '.join(map(str, channels))})")
            return a
        n = arr(noisy, "noisy", (3, 4))
        a = None if albedo is None else arr(albedo, "albedo", (3,))
        nr = None if normals is None else arr(normals, "normals", (3,))
        out = np.empty_like(n)
        _lib.check(self._lib.lrt_denoise(self._h, n.ctypes.data, n.shape[2], None if a is None else a.ctypes.data,
                                         None if nr is None else nr.ctypes.data, out.ctypes.data, 0))
        return out

    def _call_torch(self, noisy, albedo, normals):
        import torch
        w, h = self.input_size

        def ten(x, name, channels):
            if not _is_torch(x):
                raise TypeError(f"Denoiser: {name} must be a torch tensor when noisy is one")
            if not x.is_cuda or x.device != noisy.device or x.dtype != torch.float32:
                raise RuntimeError(f"Denoiser: {name} must be a float32 tensor on {noisy.device} (got {x.dtype} on {x.device})")
            if x.dim() != 3 or x.shape[0] != h or x.shape[1] != w or x.shape[2] not in channels:
                raise RuntimeError(f"Denoiser: {name} has shape {tuple(x.shape)}, expected ({h}, {w}, {' | '.join(map(str, channels))})")
            return x.contiguous()
        n = ten(noisy, "noisy", (3, 4))
        if (n.device.index or 0) != self.device:
            raise RuntimeError(f"Denoiser: the tensors live on {n.device}, the denoiser on device {self.device}")
        a = None if albedo is None else ten(albedo, "albedo", (3,))
        nr = None if normals is None else ten(normals, "normals", (3,))
        out = torch.empty_like(n)
        torch.cuda.current_stream(n.device).synchronize()
        _lib.check(self._lib.lrt_denoise(self._h, n.data_ptr(), n.shape[2], None if a is None else a.data_ptr(),
                                         None if nr is None else nr.data_ptr(), out.data_ptr(), 1))
        return out


OptixDenoiser = Denoiser


def denoise(scene_image, scene, **params):
    """Denoise what mi.render returns on an `aov` scene: the first nested integrator's image is the noisy input, the first
    `albedo` AOV and the first `sh_normal` AOV (by scene.aov_channel_names()) are the guides, whichever of them the scene has.
    Returns the denoised H x W x (3|4) image.  `params` as for Denoiser."""
    a = scene.aov_desc()
    if a is None:
        raise RuntimeError("denoise(): the scene has no aov integrator (render it with <integrator type=\"aov\"> to get the guides)")
    img = np.asarray(scene_image, dtype=np.float32)
    names = scene.aov_channel_names()
    if img.ndim != 3 or img.shape[2] != len(names):
        raise RuntimeError(f"denoise(): the image has shape {tuple(img.shape)}, the scene renders {len(names)} channels")
    bmp = Bitmap(img, channel_names=names)
    inner = a.integrator_names[0].value.decode()
    rgba = [f"{inner}.{c}" for c in "RGBA" if f"{inner}.{c}" in names]
    noisy = np.ascontiguousarray(img[..., [names.index(n) for n in rgba]])
    guide = {}
    for key, typ in (("albedo", "albedo"), ("normals", "sh_normal")):
        k = next((i for i in range(a.n_aovs) if a.aov_types[i] == _lib.AOV_TYPES[typ]), None)
        guide[key] = None if k is None else bmp.select(a.aov_names[k].value.decode())
    dn = Denoiser((img.shape[1], img.shape[0]), albedo=guide["albedo"] is not None, normals=guide["normals"] is not None, **params)
    return dn(noisy, guide["albedo"], guide["normals"])


# ---- error bars from a moment render (src/integrators/moment.cpp; src/render/tests/test_renders.py:159-228)
def moment_variance(image, scene, spp):
    """(variance, mean): from what mi.render returns on a `moment` scene, the per-pixel variance OF THE MEAN of X, Y, Z over the
    pixel's `spp` samples, (m2 - m1 * m1) / (spp - 1) in float64 clamped at 0, and the XYZ means m1; both H x W x 3.
    Exact for the box filter only: with a wider reconstruction filter the samples that reach a pixel carry unequal weights, and
    the developed channels are weighted means."""
    m = scene.moment_desc()
    if m is None:
        raise RuntimeError("moment_variance(): the scene has no moment integrator")
    img = np.asarray(image, dtype=np.float64)
    if img.ndim != 3 or img.shape[2] != m.n_channels:
        raise RuntimeError(f"moment_variance(): the image has shape {tuple(img.shape)}, the scene renders {m.n_channels} channels")
    if int(spp) < 2:
        raise ValueError("moment_variance(): a variance needs spp >= 2")
    o = m.n_channels - 6
    m1, m2 = img[..., o:o + 3], img[..., o + 3:o + 6]
    return np.maximum((m2 - m1 * m1) / (int(spp) - 1), 0.0), m1.copy()


def z_test(mean_a, var_a, mean_b, var_b, alpha=0.01):
    """(p_values, pass_fraction) of the per-pixel two-sided Z-test of test_renders.py:159-176 on the difference of two estimates
    with known variances OF THE MEAN: z = |a - b| / sqrt(var_a + var_b), p = erfc(z / sqrt(2)); a pixel passes when
    p > 1 - (1 - alpha)^(1 / N), the Sidak correction over the N = H * W pixels.  A pixel whose two variances are both 0 has no
    error bar: it passes (p = 1) when the two means are equal and fails (p = 0) otherwise; it counts in the denominator.
    The reference accepts when at least 99.75 % of the pixels pass (test_renders.py:228)."""
    a, b = np.asarray(mean_a, dtype=np.float64), np.asarray(mean_b, dtype=np.float64)
    va, vb = np.asarray(var_a, dtype=np.float64), np.asarray(var_b, dtype=np.float64)
    if not (a.shape == b.shape == va.shape == vb.shape):
        raise ValueError(f"z_test(): shapes differ: {a.shape}, {va.shape}, {b.shape}, {vb.shape}")
    if a.size == 0 or not 0.0 < alpha < 1.0:
        raise ValueError("z_test(): empty input, or alpha outside (0, 1)")
    if (va < 0).any() or (vb < 0).any():
        raise ValueError("z_test(): negative variance")
    n_pixels = a.shape[0] * a.shape[1] if a.ndim >= 2 else a.size
    d, var = np.abs(a - b), va + vb
    p = np.where(d == 0.0, 1.0, 0.0)                       # no error bar: equal or not
    bar = var != 0.0
    with np.errstate(invalid="ignore"):
        z = d[bar] / np.sqrt(var[bar])                     # NaN (a non-finite mean or variance) fails: p = 0
    ok = z == z
    pz = np.zeros(z.shape, dtype=np.float64)
    pz[ok] = _erfc(z[ok] / math.sqrt(2.0)).astype(np.float64) if ok.any() else 0.0
    p[bar] = pz
    level = 1.0 - (1.0 - alpha) ** (1.0 / n_pixels)
    # with H x W x 3 input the fraction is over all H * W * 3 values while the correction counts pixels, as test_renders.py:224-228
    return p, float(np.count_nonzero(p > level)) / p.size


_erfc = np.frompyfunc(math.erfc, 1, 1)                     # scipy may be absent; one C-level loop over the pixels that have an error bar
