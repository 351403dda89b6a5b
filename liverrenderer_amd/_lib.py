"""ctypes binding of libliverrt.so (the C ABI declared in include/liverrt.h).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C
liverrenderer_amd/csrc``).  There is no CPU fallback: every render call goes to
the HIP kernels and raises ``RuntimeError`` when no GPU / no library exists.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_LIBRARY") or os.path.join(_HERE, "libliverrt.so")     # LRT_LIBRARY: developer builds (csrc/Makefile: exp)

OK, INVALID, UNSUPPORTED = 0, 1, 4      # lrt_status values the wrappers and tests name
INTEGRATOR = {"path": 0, "volpath": 1, "prbvolpath": 2, "biovolpath": 3, "biovolpath06": 4, "volpathmis": 5}
MEDIUM = {"homogeneous": 0, "liver": 1, "parenchyma": 2, "glissonCapsule": 3, "heterogeneous": 4}
EMITTER = {"area": 0, "envmap": 1, "constant": 2, "point": 3, "spot": 4, "directional": 5}
PROBE_FLOATS = 20      # include/liverrt.h LRT_PROBE_FLOATS (lrt_emitter_probe)
MEDIUM_PROBE_FLOATS = 22 # include/liverrt.h LRT_MEDIUM_PROBE_FLOATS (lrt_medium_probe)
PHASE_PROBE_FLOATS = 7 # include/liverrt.h LRT_PHASE_PROBE_FLOATS (lrt_phase_probe)
SENSOR_PROBE_FLOATS = 16 # include/liverrt.h LRT_SENSOR_PROBE_FLOATS (lrt_sensor_probe)
BSDF_PROBE_FLOATS = 30 # include/liverrt.h LRT_BSDF_PROBE_FLOATS (lrt_bsdf_probe)


class ShapeDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("first_face", C.c_uint32), ("n_faces", C.c_uint32), ("bsdf", C.c_int32),
                ("emitter", C.c_int32), ("interior_medium", C.c_int32), ("exterior_medium", C.c_int32),
                ("has_normals", C.c_int32), ("has_texcoords", C.c_int32), ("flip_normals", C.c_int32),
                ("to_world", C.c_float * 16)]


class TextureDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("color0", C.c_float * 3), ("color1", C.c_float * 3), ("to_uv", C.c_float * 9),
                ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("data", C.POINTER(C.c_float))]


class BsdfDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("reflectance", C.c_int32), ("eta", C.c_float), ("nested", C.c_int32),
                ("texture", C.c_int32), ("scale", C.c_float),
                ("alpha_u", C.c_float), ("alpha_v", C.c_float), ("distribution", C.c_int32), ("sample_visible", C.c_int32),
                ("specular_reflectance", C.c_int32), ("specular_transmittance", C.c_int32),      # [v114] roughdielectric
                ("eta_r", C.c_float), ("eta_g", C.c_float), ("eta_b", C.c_float), ("k_r", C.c_float), ("k_g", C.c_float), ("k_b", C.c_float),   # [v119] eta_rgb[3], k_rgb[3] (scalars, so that fields compare by value)
                ("diffuse_reflectance", C.c_int32), ("nonlinear", C.c_int32), ("nested_back", C.c_int32)]      # [v119] conductor, plastic, twosided
    eta_rgb = property(lambda self: (self.eta_r, self.eta_g, self.eta_b))
    k_rgb = property(lambda self: (self.k_r, self.k_g, self.k_b))


class MediumDesc(C.Structure):
    _fields_ = [("sigma_t", C.c_float * 3), ("albedo", C.c_float * 3), ("scale", C.c_float),
                ("has_spectral_extinction", C.c_int32), ("sample_emitters", C.c_int32), ("phase", C.c_int32),
                ("g", C.c_float), ("id", C.c_char * 64),
                # bio media (liver / parenchyma / glissonCapsule): include/liverrt.h
                ("type", C.c_int32), ("layer_limit", C.c_float * 4), ("sigma_collagen", (C.c_float * 3) * 4),
                ("sigma_elastin", (C.c_float * 3) * 4), ("sigma_blood", C.c_float * 3), ("sigma_bile", C.c_float * 3),
                ("sigma_lipid_water", C.c_float * 3), ("sigma_hepatocity", C.c_float),
                # heterogeneous medium (grid volume)
                ("grid_res", C.c_int32 * 3), ("grid_to_local", C.c_float * 12), ("grid_bbox_min", C.c_float * 3),
                ("grid_bbox_max", C.c_float * 3), ("grid_max", C.c_float), ("grid_data", C.POINTER(C.c_float)),
                # [v116] read only when SceneDesc.n_phases > 0: index into SceneDesc.phases, -1: none
                ("phase_index", C.c_int32), ("pad_phase", C.c_int32)]


class PhaseDesc(C.Structure):                # [v116] lrt_phase_desc: one entry of the phase-function table
    _fields_ = [("type", C.c_int32), ("g", C.c_float), ("weight", C.c_float), ("child", C.c_int32 * 2), ("n_values", C.c_uint32),
                ("values", C.POINTER(C.c_float))]


class EmitterDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("radiance", C.c_float * 3), ("shape", C.c_int32), ("scale", C.c_float),
                ("to_world", C.c_float * 16), ("width", C.c_int32), ("height", C.c_int32), ("data", C.POINTER(C.c_float)),
                # [v117] read only for a spot (type 4): degrees, degrees, index into SceneDesc.textures of a checkerboard (-1: none)
                ("cutoff_angle", C.c_float), ("beam_width", C.c_float), ("texture", C.c_int32), ("pad_spot", C.c_int32)]


class SensorDesc(C.Structure):
    _fields_ = [("to_world", C.c_float * 16), ("fov_x", C.c_float), ("near_clip", C.c_float), ("far_clip", C.c_float),
                ("medium", C.c_int32), ("principal_point_offset_x", C.c_float), ("principal_point_offset_y", C.c_float), ("pad", C.c_int32)]


class FilmDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("crop_offset_x", C.c_int32), ("crop_offset_y", C.c_int32),
                ("crop_width", C.c_int32), ("crop_height", C.c_int32), ("has_alpha", C.c_int32), ("rfilter", C.c_int32),
                ("rfilter_param", C.c_float)]


class IntegratorDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("max_depth", C.c_int32), ("rr_depth", C.c_int32), ("hide_emitters", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("n_vertices", C.c_uint32), ("n_faces", C.c_uint32), ("n_shapes", C.c_uint32), ("n_bsdfs", C.c_uint32),
                ("n_textures", C.c_uint32), ("n_media", C.c_uint32), ("n_emitters", C.c_uint32),
                ("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("texcoords", C.POINTER(C.c_float)),
                ("faces", C.POINTER(C.c_uint32)), ("face_shape", C.POINTER(C.c_uint32)),
                ("shapes", C.POINTER(ShapeDesc)), ("bsdfs", C.POINTER(BsdfDesc)), ("textures", C.POINTER(TextureDesc)),
                ("media", C.POINTER(MediumDesc)), ("emitters", C.POINTER(EmitterDesc)),
                ("sensor", SensorDesc), ("film", FilmDesc), ("integrator", IntegratorDesc),
                ("sample_count", C.c_uint32), ("sampler_seed", C.c_uint32),
                ("sampler_type", C.c_uint32), ("samples_per_pass", C.c_uint32), ("use_spectral_mis", C.c_uint32), ("pad", C.c_uint32),
                ("n_phases", C.c_uint32), ("pad_phases", C.c_uint32), ("phases", C.POINTER(PhaseDesc))]       # [v116]


AOV_MAX_INTEGRATORS, AOV_MAX_AOVS, AOV_NAME_LEN = 4, 16, 64
AOV_TYPES = {"albedo": 0, "depth": 1, "position": 2, "uv": 3, "geo_normal": 4, "sh_normal": 5, "dp_du": 6, "dp_dv": 7,
             "prim_index": 8, "shape_index": 9}


class AovDesc(C.Structure):
    """lrt_aov_desc: the aov integrator's nested integrators and AOVs (include/liverrt.h)."""
    _fields_ = [("n_integrators", C.c_int32), ("integrators", IntegratorDesc * AOV_MAX_INTEGRATORS),
                ("integrator_names", (C.c_char * AOV_NAME_LEN) * AOV_MAX_INTEGRATORS),
                ("n_aovs", C.c_int32), ("aov_types", C.c_int32 * AOV_MAX_AOVS), ("aov_names", (C.c_char * AOV_NAME_LEN) * AOV_MAX_AOVS),
                ("n_aov_channels", C.c_int32), ("n_channels", C.c_int32)]


class MomentDesc(C.Structure):
    """lrt_moment_desc: the moment integrator's nested integrator, its name and the channel counts (include/liverrt.h)."""
    _fields_ = [("integrator", IntegratorDesc), ("name", C.c_char * AOV_NAME_LEN), ("n_channels", C.c_int32), ("n_raw_channels", C.c_int32)]


class RenderOpts(C.Structure):
    _fields_ = [("integrator", C.c_int32), ("max_depth", C.c_int32), ("rr_depth", C.c_int32), ("hide_emitters", C.c_int32),
                ("spp", C.c_uint32), ("seed", C.c_uint32), ("tile_rank", C.c_uint32), ("tile_count", C.c_uint32),
                ("device", C.c_int32), ("output_on_device", C.c_int32), ("grad_medium", C.c_int32), ("pad", C.c_int32)]


class RenderStats(C.Structure):
    _fields_ = [("n_samples", C.c_uint64), ("n_iter", C.c_uint64), ("n_shadow", C.c_uint64), ("n_launches", C.c_uint64),
                ("n_records", C.c_uint64), ("kernel_ms", C.c_double), ("total_ms", C.c_double), ("lds_resident", C.c_uint64),
                ("record_bytes", C.c_uint64), ("n_closed_guard", C.c_uint64), ("n_proven", C.c_uint64), ("n_primary_entry", C.c_uint64)]


class ParamGrads(C.Structure):
    _fields_ = [("d_sigma_t", C.c_float * 3), ("d_albedo", C.c_float * 3), ("d_g", C.c_float)]


class DenoiseParams(C.Structure):
    """lrt_denoise_params: a field left 0 takes its default (include/liverrt.h)."""
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("eps_a", C.c_float)]


class RaysSoA(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_float)) for n in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax")]


class HitsSoA(C.Structure):
    _fields_ = [("t", C.POINTER(C.c_float)), ("u", C.POINTER(C.c_float)), ("v", C.POINTER(C.c_float)), ("prim", C.POINTER(C.c_uint32))]


def make_opts(integrator=None, max_depth=None, rr_depth=None, hide_emitters=None, spp=0, seed=0,
              tile_rank=0, tile_count=1, device=0, output_on_device=False, grad_medium=0):
    o = RenderOpts()
    o.integrator = -1 if integrator is None else (INTEGRATOR[integrator] if isinstance(integrator, str) else int(integrator))
    o.max_depth = -2 if max_depth is None else int(max_depth)
    o.rr_depth = -1 if rr_depth is None else int(rr_depth)
    o.hide_emitters = -1 if hide_emitters is None else int(bool(hide_emitters))
    o.spp, o.seed, o.tile_rank, o.tile_count = int(spp), int(seed) & 0xffffffff, int(tile_rank), int(tile_count)
    o.device, o.output_on_device = int(device), int(bool(output_on_device))
    o.grad_medium = int(grad_medium)
    return o


_lib = None


def _pytorch_context_first():
    """The PyTorch-ROCm wheel carries its own libamdhip64.so while libliverrt.so links the system one: a process that uses both must
    let PyTorch create its HIP context BEFORE libliverrt's first device call, or PyTorch is left without a device ("No HIP GPUs are
    available") - on an 8-rank launch one mis-ordered import is a whole-job failure.  So when PyTorch is importable its context is
    created here, before the library is loaded, whatever order the caller imports things in.  LRT_NO_TORCH_INIT=1 skips this (a process
    that never uses PyTorch saves the import).  Returns what was done, for the tests."""
    import importlib.util
    import sys
    if os.environ.get("LRT_NO_TORCH_INIT"):
        return "skipped"
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is None:
        return "no torch"
    import torch
    if not torch.cuda.is_available():
        return "no device"
    if not torch.cuda.is_initialized():
        # (a rank of a one-process-per-GPU launch that has not chosen its device yet: its own GPU, not device 0 for every rank)
        lr = os.environ.get("LOCAL_RANK")
        if lr is not None and lr.isdigit() and torch.cuda.device_count() > 0:
            torch.cuda.set_device(int(lr) % torch.cuda.device_count())
        torch.zeros(1, device="cuda")
    if not torch.cuda.is_initialized():
        raise RuntimeError("PyTorch is importable but its HIP context could not be created before libliverrt.so was loaded; "
                           "set LRT_NO_TORCH_INIT=1 if this process does not use PyTorch")
    return "initialised"


def lib():
    """Load libliverrt.so and declare the signatures of every exported symbol."""
    global _lib
    if _lib is not None:
        return _lib
    _pytorch_context_first()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the hip_ad_rgb back-end has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.lrt_last_error.restype = C.c_char_p
    L.lrt_version.restype = C.c_int
    L.lrt_scene_load_xml.argtypes = [C.c_char_p, P(C.c_char_p), C.c_int, P(C.c_void_p)]
    L.lrt_scene_load_xml_string.argtypes = [C.c_char_p, C.c_char_p, P(C.c_char_p), C.c_int, P(C.c_void_p)]
    L.lrt_scene_from_desc.argtypes = [P(SceneDesc), P(C.c_void_p)]
    L.lrt_scene_desc_get.argtypes = [C.c_void_p]
    L.lrt_scene_desc_get.restype = P(SceneDesc)
    L.lrt_scene_free.argtypes = [C.c_void_p]
    L.lrt_scene_free.restype = None
    L.lrt_render.argtypes = [C.c_void_p, P(RenderOpts), C.c_void_p, C.c_void_p]
    L.lrt_render_multi.argtypes = [C.c_void_p, P(RenderOpts), C.c_int, P(C.c_int), C.c_void_p, C.c_void_p]
    L.lrt_render_backward_multi.argtypes = [C.c_void_p, P(RenderOpts), C.c_int, P(C.c_int), C.c_void_p, P(ParamGrads)]
    L.lrt_math_eval.argtypes = [C.c_int, P(C.c_float), P(C.c_float), C.c_uint32, P(C.c_float), P(C.c_float), C.c_int]
    L.lrt_render_stats_get.argtypes = [C.c_void_p, P(RenderStats)]
    L.lrt_film_develop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.lrt_primary_entry_get.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    L.lrt_render_samples.argtypes = [C.c_void_p, P(RenderOpts), C.c_uint64, C.c_uint32, C.c_void_p]
    L.lrt_render_backward.argtypes = [C.c_void_p, P(RenderOpts), C.c_void_p, P(ParamGrads)]
    L.lrt_render_backward_grid.argtypes = [C.c_void_p, P(RenderOpts), C.c_void_p, P(ParamGrads), C.c_void_p]
    L.lrt_render_backward_grid.restype = C.c_int
    L.lrt_trace.argtypes = [C.c_void_p, P(RaysSoA), P(HitsSoA), C.c_uint32, C.c_int]
    # the probes: (scene, [medium,] one pointer per input array, n, out, device); F: float *, U: uint32_t *
    F, U = P(C.c_float), P(C.c_uint32)
    for name, medium, arrays in (("lrt_emitter_probe", 0, [F, F]), ("lrt_envmap_probe", 0, [F]), ("lrt_bsdf_probe", 0, [F, F, F, F]),
                                 ("lrt_phase_probe", 1, [F, F, F]), ("lrt_medium_probe", 1, [F, F, F, F, U]), ("lrt_sensor_probe", 0, [F])):
        getattr(L, name).argtypes = [C.c_void_p] + [C.c_int] * medium + arrays + [C.c_uint32, F, C.c_int]
        getattr(L, name).restype = C.c_int
    L.lrt_param_set.argtypes = [C.c_void_p, C.c_char_p, P(C.c_float), C.c_int]
    L.lrt_param_get.argtypes = [C.c_void_p, C.c_char_p, P(C.c_float), C.c_int]
    L.lrt_image_read.argtypes = [C.c_char_p, P(C.c_int), P(C.c_int), P(C.c_int), P(P(C.c_float))]
    L.lrt_image_free.argtypes = [P(C.c_float)]
    L.lrt_image_free.restype = None
    L.lrt_image_write_exr.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lrt_image_write_png.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lrt_image_write_exr_channels.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, P(C.c_char_p), C.c_void_p]
    L.lrt_scene_aov_get.argtypes = [C.c_void_p, P(AovDesc)]
    L.lrt_aov_channel_name.argtypes = [C.c_void_p, C.c_int]
    L.lrt_aov_channel_name.restype = C.c_char_p
    L.lrt_render_aov.argtypes = [C.c_void_p, P(RenderOpts), C.c_void_p, C.c_void_p]
    L.lrt_render_aov_samples.argtypes = [C.c_void_p, P(RenderOpts), C.c_uint64, C.c_uint32, C.c_void_p]
    L.lrt_scene_moment_get.argtypes = [C.c_void_p, P(MomentDesc)]
    L.lrt_moment_channel_name.argtypes = [C.c_void_p, C.c_int]
    L.lrt_moment_channel_name.restype = C.c_char_p
    L.lrt_render_moment.argtypes = [C.c_void_p, P(RenderOpts), C.c_void_p, C.c_void_p]
    L.lrt_render_moment_samples.argtypes = [C.c_void_p, P(RenderOpts), C.c_uint64, C.c_uint32, C.c_void_p]
    L.lrt_denoiser_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(DenoiseParams), C.c_int, P(C.c_void_p)]
    L.lrt_denoise.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.lrt_denoiser_free.argtypes = [C.c_void_p]
    L.lrt_denoiser_free.restype = None
    L.lrt_denoiser_get.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int), P(DenoiseParams)]
    L.lrt_image_read_named.argtypes = [C.c_char_p, P(C.c_int), P(C.c_int), P(C.c_int), P(P(C.c_float)), P(C.c_void_p)]
    L.lrt_image_free_names.argtypes = [C.c_void_p]
    L.lrt_image_free_names.restype = None
    for name in ("lrt_denoiser_create", "lrt_denoise", "lrt_denoiser_get", "lrt_image_read_named", "lrt_scene_moment_get", "lrt_render_moment", "lrt_render_moment_samples"):
        getattr(L, name).restype = C.c_int
    for name in ("lrt_image_read", "lrt_image_write_exr", "lrt_image_write_png", "lrt_scene_load_xml", "lrt_scene_load_xml_string", "lrt_scene_from_desc", "lrt_render", "lrt_render_multi", "lrt_render_backward_multi", "lrt_math_eval", "lrt_render_stats_get",
                 "lrt_film_develop", "lrt_render_samples", "lrt_render_backward", "lrt_trace", "lrt_param_set", "lrt_param_get",
                 "lrt_image_write_exr_channels", "lrt_scene_aov_get", "lrt_render_aov", "lrt_render_aov_samples"):
        getattr(L, name).restype = C.c_int
    _lib = L
    return L


EXPORTED_SYMBOLS = ["lrt_last_error", "lrt_version", "lrt_scene_load_xml", "lrt_scene_load_xml_string", "lrt_scene_from_desc",
                    "lrt_scene_desc_get", "lrt_scene_free", "lrt_render", "lrt_render_multi", "lrt_render_backward_multi", "lrt_math_eval", "lrt_render_stats_get", "lrt_film_develop",
                    "lrt_render_samples", "lrt_render_backward", "lrt_render_backward_grid", "lrt_trace", "lrt_emitter_probe", "lrt_envmap_probe", "lrt_bsdf_probe", "lrt_phase_probe", "lrt_medium_probe", "lrt_sensor_probe", "lrt_param_set", "lrt_param_get",
                    "lrt_image_read", "lrt_image_free", "lrt_image_write_exr", "lrt_image_write_png",
                    "lrt_vae_model_create", "lrt_vae_model_free", "lrt_vae_scatter",
                    "lrt_scene_aov_get", "lrt_aov_channel_name", "lrt_render_aov", "lrt_render_aov_samples", "lrt_image_write_exr_channels",
                    "lrt_denoiser_create", "lrt_denoise", "lrt_denoiser_free", "lrt_denoiser_get", "lrt_image_read_named", "lrt_image_free_names",
                    "lrt_scene_moment_get", "lrt_moment_channel_name", "lrt_render_moment", "lrt_render_moment_samples", "lrt_primary_entry_get"]


def bsdf_probe_fields(out):
    """the n x LRT_BSDF_PROBE_FLOATS block of lrt_bsdf_probe (or of the oracle's twin) as a dict of arrays"""
    return {"shape": out[:, 0].astype("int32"), "t": out[:, 1], "p": out[:, 2:5], "n": out[:, 5:8], "sh_n": out[:, 8:11], "uv": out[:, 11:13],
            "wi": out[:, 13:16], "wo": out[:, 16:19], "wo_z": out[:, 19], "pdf": out[:, 20], "eta": out[:, 21], "type": out[:, 22].astype("int32"),
            "weight": out[:, 23:26], "eval": out[:, 26:29], "eval_pdf": out[:, 29], "raw": out}


def medium_probe_fields(out):
    """The record of lrt_medium_probe / orc_medium_probe (n x LRT_MEDIUM_PROBE_FLOATS) as a dict of arrays"""
    return {"valid": out[:, 0] != 0, "t": out[:, 1], "p": out[:, 2:5], "mint": out[:, 5], "sigma_t": out[:, 6:9], "sigma_s": out[:, 9:12],
            "sigma_n": out[:, 12:15], "combined": out[:, 15:18], "local": out[:, 18:21], "grid": out[:, 21], "raw": out}


def sensor_probe_fields(out):
    """The record of lrt_sensor_probe / orc_sensor_probe (n x LRT_SENSOR_PROBE_FLOATS) as a dict of arrays"""
    return {"o": out[:, 0:3], "d": out[:, 3:6], "maxt": out[:, 6], "adjusted": out[:, 7:9], "origin": out[:, 9:11].astype("int64"),
            "rel": out[:, 11:13], "weight": out[:, 13], "fcount": out[:, 14].astype("int64"), "raw": out}


def check(status):
    if status != OK:
        raise RuntimeError(lib().lrt_last_error().decode("utf-8", "replace"))
