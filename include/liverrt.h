/*
 * liverrt.h -- C ABI of the MI355X-native `hip_ad_rgb` rendering back-end.
 *
 * This is the drop-in boundary for the ONE hot path of mmigas/LiverRenderer
 * (a Mitsuba 3.8 fork): the forward path / volpath sample loop and its PRB
 * adjoint. Everything below is plain C: opaque handles, POD structs, caller
 * owned buffers, no exceptions (errors: status code + lrt_last_error()).
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference tree):
 *
 *   lrt_scene_load_xml / _xml_string    src/core/parser.cpp (mi.load_file / mi.load_string,
 *                                        `-Dkey=value` defines: src/mitsuba/mitsuba.cpp:161,240-246)
 *   lrt_scene_from_desc                  mi.load_dict (src/python/python/util.py) -- "from buffers"
 *   lrt_render                           Integrator::render(scene, sensor, seed, spp, develop, evaluate)
 *                                        include/mitsuba/render/integrator.h:74,
 *                                        src/render/integrator.cpp:151-395 (JIT branch :274-388)
 *   lrt_render_backward                  Integrator::render_backward include/mitsuba/render/integrator.h:253,
 *                                        src/python/python/ad/integrators/common.py:625-783
 *   lrt_trace                            the ray-tracing callback seam of the LLVM variants
 *                                        src/render/scene_native.inl:135-202 (SoA RayHit layout)
 *   lrt_param_set / lrt_param_get        mi.traverse(scene)[key] (src/media/homogeneous.cpp:146-151,
 *                                        src/phase/hg.cpp:60-62; the tabulated / Rayleigh / blended phase
 *                                        functions of lrt_scene_desc.phases [v116] have no keys)
 *   lrt_scene_desc.phases [v116]         PhaseFunction plugins src/phase/tabphase.cpp, rayleigh.cpp, blendphase.cpp
 *                                        (isotropic.cpp and hg.cpp stay in lrt_medium_desc.phase / g)
 *   lrt_film_develop                     HDRFilm::develop src/films/hdrfilm.cpp:306-410
 *   lrt_last_error                       Throw(...) -> Python RuntimeError
 *
 * Threading: one host thread per lrt_scene; device work runs on a private HIP
 * stream owned by the scene.  All host pointers are caller-owned unless
 * returned by a *_load / *_from_desc call.
 */
#ifndef LIVERRT_H
#define LIVERRT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_API __attribute__((visibility("default")))

typedef enum {
    LRT_OK = 0,
    LRT_ERR_INVALID = 1,      /* bad argument / unsupported plugin / parse error */
    LRT_ERR_IO = 2,           /* file not found / unreadable                      */
    LRT_ERR_DEVICE = 3,       /* HIP runtime failure, or no GPU present           */
    LRT_ERR_UNSUPPORTED = 4
} lrt_status;

/* ---------------------------------------------------------------- enums */
enum { LRT_INTEGRATOR_PATH = 0, LRT_INTEGRATOR_VOLPATH = 1, LRT_INTEGRATOR_PRBVOLPATH = 2,
       LRT_INTEGRATOR_VOLPATHMIS = 5,    /* src/integrators/volpathmis.cpp (spectral MIS)                 */
       LRT_INTEGRATOR_BIOVOLPATH = 3,    /* src/integrators/biovolpath.cpp, JIT-variant lane semantics   */
       LRT_INTEGRATOR_BIOVOLPATH06 = 4   /* src/integrators/biovolpath06.cpp, scalar semantics per lane   */ };
/* medium plugins: src/media/homogeneous.cpp, liver.cpp, parenchyma.cpp, glissonCapsule.cpp (docs/BIO_TRANSPORT_SPEC.md) */
enum { LRT_MEDIUM_HOMOGENEOUS = 0, LRT_MEDIUM_LIVER = 1, LRT_MEDIUM_PARENCHYMA = 2, LRT_MEDIUM_GLISSON = 3,
       LRT_MEDIUM_HETEROGENEOUS = 4   /* src/media/heterogeneous.cpp: sigma_t from a grid volume, delta tracking */ };
enum { LRT_BSDF_DIFFUSE = 0, LRT_BSDF_DIELECTRIC = 1, LRT_BSDF_BUMPMAP = 2, LRT_BSDF_NULL = 3, LRT_BSDF_ROUGHDIELECTRIC = 4,
       LRT_BSDF_CONDUCTOR = 5, LRT_BSDF_PLASTIC = 6, LRT_BSDF_TWOSIDED = 7   /* [v119] src/bsdfs/conductor.cpp, plastic.cpp, twosided.cpp */ };
enum { LRT_TEX_RGB = 0, LRT_TEX_CHECKERBOARD = 1, LRT_TEX_BITMAP = 2 };
enum { LRT_PHASE_ISOTROPIC = 0, LRT_PHASE_HG = 1,
       /* [v116] entries of lrt_scene_desc.phases only (lrt_medium_desc.phase stays ISOTROPIC or HG) */
       LRT_PHASE_TABULATED = 2,       /* src/phase/tabphase.cpp: `values` over cos(theta) in [-1, 1], physics convention (cos = 1: forward) */
       LRT_PHASE_RAYLEIGH = 3,        /* src/phase/rayleigh.cpp                             */
       LRT_PHASE_BLEND = 4            /* src/phase/blendphase.cpp: one level, a constant weight */ };
enum { LRT_EMITTER_AREA = 0, LRT_EMITTER_ENVMAP = 1, LRT_EMITTER_CONSTANT = 2,
       LRT_EMITTER_POINT = 3,         /* [v106] src/emitters/point.cpp: `intensity` in radiance[3], position = to_world * 0 */
       LRT_EMITTER_SPOT = 4,          /* [v117] src/emitters/spot.cpp: `intensity` in radiance[3], at to_world * 0, looking along to_world * (0, 0, 1) */
       LRT_EMITTER_DIRECTIONAL = 5    /* [v117] src/emitters/directional.cpp: `irradiance` in radiance[3], light travels along to_world * (0, 0, 1) */ };
enum { LRT_SHAPE_MESH = 0, LRT_SHAPE_RECTANGLE = 1,
       LRT_SHAPE_SPHERE = 2           /* [v106] src/shapes/sphere.cpp: n_faces = 0, analytic intersection (see lrt_shape_desc) */ };
/* The CPU oracle under oracle/ renders LRT_SHAPE_SPHERE and LRT_EMITTER_POINT too; it refuses LRT_EMITTER_AREA on an
   LRT_SHAPE_MESH with a message. */
enum { LRT_RFILTER_BOX = 0, LRT_RFILTER_GAUSSIAN = 1, LRT_RFILTER_TENT = 2 };

/* ------------------------------------------------- scene description (POD)
 * The flattened, plugin-free form of a loaded scene.  Produced by the XML
 * loader (lrt_scene_desc_get) and accepted by lrt_scene_from_desc; it is also
 * the data format the CPU oracle under oracle/ consumes, so that both sides
 * see byte-identical inputs.  All geometry is in world space.               */

typedef struct {
    int32_t  kind;            /* LRT_SHAPE_*                                       */
    uint32_t first_face;      /* range into faces[]                                */
    uint32_t n_faces;
    int32_t  bsdf;            /* index into bsdfs[], -1: none                      */
    int32_t  emitter;         /* index into emitters[] (area light), -1: none      */
    int32_t  interior_medium; /* index into media[], -1: none                      */
    int32_t  exterior_medium;
    int32_t  has_normals;     /* per-vertex shading normals present                */
    int32_t  has_texcoords;
    int32_t  flip_normals;
    float    to_world[16];    /* row-major; used by LRT_SHAPE_RECTANGLE sampling   */
} lrt_shape_desc;
/* LRT_SHAPE_SPHERE [v106]: first_face = n_faces = 0, has_normals = has_texcoords = 0; to_world holds
   to_world * translate(center) * scale(radius) (sphere.cpp:128-136), so radius = |to_world * (1,0,0)| and
   center = to_world * (0,0,0).  Shear and non-uniform scale only warn, as in the reference.  A ray hit on the k-th
   sphere of shapes[] (counting spheres only) reports prim = n_faces + k, u = v = 0 (lrt_trace included).  Spheres
   carry no area emitter (LRT_ERR_UNSUPPORTED), and prbvolpath rejects scenes with spheres or point emitters.     */

typedef struct {
    int32_t type;             /* LRT_TEX_*                                         */
    float   color0[3];        /* RGB value (LRT_TEX_RGB) / checkerboard color0     */
    float   color1[3];
    float   to_uv[9];         /* row-major 3x3 affine uv transform                 */
    int32_t width, height, channels;   /* bitmap: 1 or 3 channels                  */
    const float *data;        /* bitmap texels, linear, already rounded to the
                                 storage precision the reference uses (fp16 for
                                 8/16-bit inputs: src/textures/bitmap.cpp:268-283) */
} lrt_texture_desc;

typedef struct {
    int32_t type;             /* LRT_BSDF_*                                        */
    int32_t reflectance;      /* texture index (diffuse)                           */
    float   eta;              /* int_ior / ext_ior (dielectric, roughdielectric)   */
    int32_t nested;           /* bumpmap: nested bsdf index                        */
    int32_t texture;          /* bumpmap: height texture index                     */
    float   scale;            /* bumpmap scale                                     */
    /* [v114] roughdielectric (src/bsdfs/roughdielectric.cpp); ignored by the other types */
    float   alpha_u, alpha_v; /* roughness along the tangent / bitangent; values below 1e-4 are raised to it (microfacet.h:425-428) */
    int32_t distribution;     /* 0: beckmann, 1: ggx                               */
    int32_t sample_visible;   /* visible-normal sampling (Heitz and d'Eon)         */
    int32_t specular_reflectance;    /* texture index (rgb or checkerboard), -1: none */
    int32_t specular_transmittance;  /* texture index (rgb or checkerboard), -1: none */
    /* [v119] conductor, plastic, twosided; ignored by the other types.
     * conductor: eta_rgb + i k_rgb, specular_reflectance (a texture index, required).
     * plastic: eta (int_ior / ext_ior), diffuse_reflectance (a texture index, required), specular_reflectance (-1: none), nonlinear.
     * twosided: nested (the front child), nested_back (the back child; -1 or equal to `nested`: one child serves both sides).  The children
     * are diffuse, conductor or plastic. */
    float   eta_rgb[3], k_rgb[3];
    int32_t diffuse_reflectance;
    int32_t nonlinear;
    int32_t nested_back;
} lrt_bsdf_desc;

typedef struct {
    float   sigma_t[3];
    float   albedo[3];
    float   scale;
    int32_t has_spectral_extinction;
    int32_t sample_emitters;
    int32_t phase;            /* LRT_PHASE_*                                       */
    float   g;
    char    id[64];           /* XML id, used to form parameter keys               */
    /* --- bio media (fork): element-competition sampling of the 5-argument Medium::sample_interaction,
       used by the biovolpath integrators only; path / volpath / prbvolpath see the fields above.      */
    int32_t type;             /* LRT_MEDIUM_*                                      */
    float   layer_limit[4];   /* liver / glissonCapsule: layer1Limit..layer4Limit (liver.cpp:143-146)     */
    float   sigma_collagen[4][3];  /* per layer, in the channel order the medium STORES them: the plugins read
                                 G from "..._B" and B from "..._G" (liver.cpp:148-166)                    */
    float   sigma_elastin[4][3];   /* layers 1-2 swapped the same way, layers 3-4 not (liver.cpp:168-186) */
    float   sigma_blood[3], sigma_bile[3], sigma_lipid_water[3];   /* liver / parenchyma                 */
    float   sigma_hepatocity;
    /* --- heterogeneous medium: sigma_t = scale * gridvolume (src/volumes/grid.cpp: one channel, trilinear, clamp), albedo
       constant; majorant = scale * grid_max.  The 4-argument sample_interaction of src/render/medium.cpp:40-82.        */
    int32_t grid_res[3];      /* x, y, z; all 0 when there is no grid                */
    float   grid_to_local[12];/* world -> the grid's unit cube [0,1]^3, rows 0..2 (Volume::m_to_local)            */
    float   grid_bbox_min[3], grid_bbox_max[3];   /* world-space bounds of that cube (Volume::update_bbox)       */
    float   grid_max;         /* maximum of the grid values (Volume::max)            */
    const float *grid_data;   /* x fastest: data[(z * res_y + y) * res_x + x]         */
    /* [v116] read only when lrt_scene_desc.n_phases > 0: index into phases[] of a TABULATED, RAYLEIGH or BLEND entry (an ISOTROPIC / HG
       entry is LRT_ERR_INVALID here), -1: none (`phase` / `g` above describe the medium).  With an entry, `phase` / `g` are ignored by
       the forward integrators. */
    int32_t phase_index;
    int32_t pad_phase;
} lrt_medium_desc;

/* [v116] One phase function of the table lrt_scene_desc.phases.  A medium points at a TABULATED, RAYLEIGH or BLEND entry;
   ISOTROPIC and HG entries exist as the children of a BLEND (a medium that scatters by one of those two says so in `phase` / `g`).
   TABULATED: n_values >= 2 non-negative values with some mass, the nodes of a piecewise linear density over cos(theta) in [-1, 1]
   (ContinuousDistribution, include/mitsuba/core/distr_1d.h:548-597, built as the scalar constructor builds it).
   BLEND: (1 - weight) * child[0] + weight * child[1], weight clipped to [0, 1]; a child is never a BLEND.
   The forward integrators render such media on the EXT kernel instances; prbvolpath refuses the scene, lrt_param_set has no key
   for `values` / `weight`, and the CPU oracle under oracle/ must not be handed such a scene. */
typedef struct {
    int32_t  type;            /* LRT_PHASE_*                                       */
    float    g;               /* HG                                                */
    float    weight;          /* BLEND                                             */
    int32_t  child[2];        /* BLEND: indices into phases[] (phase_0, phase_1), else -1 */
    uint32_t n_values;        /* TABULATED                                         */
    const float *values;
} lrt_phase_desc;

typedef struct {
    int32_t type;             /* LRT_EMITTER_*                                     */
    float   radiance[3];      /* area / constant; point [v106] and spot [v117]: intensity; directional [v117]: irradiance */
    int32_t shape;            /* area: owning shape, a rectangle or [v107] any LRT_SHAPE_MESH */
    float   scale;            /* envmap                                            */
    float   to_world[16];     /* envmap, row-major; point [v106]: position in column 3; spot / directional [v117]: the emitter's pose */
    int32_t width, height;    /* envmap: ORIGINAL bitmap resolution (w, h)         */
    const float *data;        /* envmap: h * w * 3 linear RGB floats               */
    /* [v117] read only when type is LRT_EMITTER_SPOT (a zero-filled description from before v117 means what it meant) */
    float   cutoff_angle;     /* degrees; 0 < beam_width <= cutoff_angle <= 180, and cutoff_angle < 90 with a texture (uv_factor = tan(cutoff)) */
    float   beam_width;       /* degrees; the plugin's default is 3/4 of the cutoff (the XML loader fills it in) */
    int32_t texture;          /* projection texture: index into textures[] of a checkerboard, -1: none */
    int32_t pad_spot;
} lrt_emitter_desc;
/* [v107] An area emitter on an LRT_SHAPE_MESH shape samples a face by area (src/render/mesh.cpp:449-482,861-935; the table
   is built from positions[] and faces[] of its face range).  A mesh without faces, or one whose total area is zero, is
   rejected (LRT_ERR_INVALID).  prbvolpath rejects scenes with such an emitter (LRT_ERR_UNSUPPORTED), and the CPU oracle
   under oracle/ must not be handed one (it samples area emitters as rectangles).                                  */
/* [v117] LRT_EMITTER_SPOT and LRT_EMITTER_DIRECTIONAL are delta emitters (spot.cpp:176-215, directional.cpp:148-176): no ray hits
   them, they are sampled through Scene::sample_emitter_direction alone and share the uniform emitter selection with every other
   emitter.  Both keep their value in `radiance` and their pose in `to_world`, which must be finite and invertible.  A directional
   light is infinite but no environment emitter: it does not count towards "only one environment emitter".  A spot's texture must be
   a checkerboard (an RGB texture is LRT_ERR_INVALID, as the plugin refuses a texture that does not vary; a bitmap is
   LRT_ERR_UNSUPPORTED).  Out-of-range angles are LRT_ERR_INVALID (the plugin only asserts cutoff >= beam in debug builds).  The
   forward integrators render such scenes on the EXT kernel instances; prbvolpath refuses them (LRT_ERR_UNSUPPORTED), lrt_param_set
   has no key for an emitter, and the CPU oracle under oracle/ must not be handed such a scene (it has no branch for either type and
   would treat them as a constant sky).  Not built: sample_ray / sample_position (no integrator here traces from lights), a bitmap
   projection texture, the `projector` emitter, any adjoint. */

/* samplers: src/samplers/independent.cpp (PCG32 stream per lane), src/samplers/ldsampler.cpp ((0,2)-sequence,
   TEA-shuffled permutation + per-pixel scramble) */
enum { LRT_SAMPLER_INDEPENDENT = 0, LRT_SAMPLER_LD = 1 };

typedef struct {
    float   to_world[16];     /* camera-to-world, row-major                        */
    float   fov_x;            /* horizontal field of view, degrees                 */
    float   near_clip, far_clip;
    int32_t medium;           /* medium the sensor sits in, -1: none               */
    float   principal_point_offset_x, principal_point_offset_y;   /* perspective.cpp:147-150,214-221 */
    int32_t pad;
} lrt_sensor_desc;

typedef struct {
    int32_t width, height;
    int32_t crop_offset_x, crop_offset_y, crop_width, crop_height;
    int32_t has_alpha;        /* pixel_format rgba                                 */
    int32_t rfilter;          /* LRT_RFILTER_*                                     */
    float   rfilter_param;    /* gaussian: stddev; tent: radius                    */
} lrt_film_desc;

typedef struct {
    int32_t type;             /* LRT_INTEGRATOR_*                                  */
    int32_t max_depth;        /* -1: unbounded = 65535 (so is any larger value)    */
    int32_t rr_depth;
    int32_t hide_emitters;
} lrt_integrator_desc;

typedef struct {
    uint32_t n_vertices, n_faces, n_shapes, n_bsdfs, n_textures, n_media, n_emitters;
    const float    *positions;    /* 3 * n_vertices                                */
    const float    *normals;      /* 3 * n_vertices (zero where absent)            */
    const float    *texcoords;    /* 2 * n_vertices (zero where absent)            */
    const uint32_t *faces;        /* 3 * n_faces, global vertex ids                */
    const uint32_t *face_shape;   /* n_faces                                       */
    const lrt_shape_desc   *shapes;
    const lrt_bsdf_desc    *bsdfs;
    const lrt_texture_desc *textures;
    const lrt_medium_desc  *media;
    const lrt_emitter_desc *emitters;
    lrt_sensor_desc     sensor;
    lrt_film_desc       film;
    lrt_integrator_desc integrator;
    uint32_t sample_count;        /* sampler sample_count (default spp)            */
    uint32_t sampler_seed;        /* sampler `seed` property (m_base_seed)         */
    uint32_t sampler_type;        /* LRT_SAMPLER_*; ld rounds spp up to 4, 16, 64, 256, 1024, ... */
    uint32_t samples_per_pass;    /* integrator `samples_per_pass` (integrator.cpp:176-184), 0: unset; renders of more than
                                     2^32 - 1 samples are split into passes as well (integrator.cpp:275-293)  */
    uint32_t use_spectral_mis;    /* volpathmis `use_spectral_mis` (volpathmis.cpp:47, default true)                */
    uint32_t pad;
    /* [v116] the phase-function table; n_phases = 0 (a description from before v116, zero-filled here): every medium scatters by its `phase` / `g` */
    uint32_t n_phases, pad_phases;
    const lrt_phase_desc *phases;
} lrt_scene_desc;

/* ----------------------------------------------------------- render call */
typedef struct {
    int32_t  integrator;      /* LRT_INTEGRATOR_*, -1: use the scene's             */
    int32_t  max_depth;       /* -2: use the scene's                               */
    int32_t  rr_depth;        /* -1: use the scene's                               */
    int32_t  hide_emitters;   /* -1: use the scene's                               */
    uint32_t spp;             /* 0: use the scene's sample_count; with the ld sampler
                                 rounded up to 4, 16, 64, 256, ... (ldsampler.cpp:83-93)  */
    uint32_t seed;
    /* image-tile sharding (multi-GPU): this call renders only the 32x32 pixel
       tiles t with t % tile_count == tile_rank, into a full-size zeroed film. */
    uint32_t tile_rank, tile_count;
    int32_t  device;          /* HIP device ordinal                                */
    int32_t  output_on_device;/* film_raw / image are device pointers              */
    int32_t  grad_medium;     /* lrt_render_backward: index (into media[]) of the medium whose sigma_t / albedo / g
                                 the gradients refer to; -1: the sum over all media (one shared parameter set).
                                 lrt_render_backward_grid [v112]: the index of a heterogeneous medium (-1 is invalid) */
    int32_t  pad;
} lrt_render_opts;

typedef struct {
    uint64_t n_samples;       /* camera samples traced                             */
    uint64_t n_iter;          /* path-loop iterations executed (all paths)         */
    uint64_t n_shadow;        /* NEE visibility / march ray queries traced         */
    uint64_t n_launches;      /* iteration-kernel launches                         */
    uint64_t n_records;       /* path records read by those launches (<= n_iter:
                                 trips retired by look-ahead move no record)        */
    double   kernel_ms;       /* sum of iteration-kernel durations (HIP events)    */
    double   total_ms;        /* whole lrt_render device time (HIP events)         */
    uint64_t lds_resident;    /* 1: the kernels ran on the LDS-resident BVH image (1024-thread workgroups);
                                 0: the mesh did not fit, BVH in global memory (256-thread workgroups)  [v103] */
    uint64_t record_bytes;    /* bytes per queued path record of the forward render kernel's layout: 64 (volpath where
                                 only a path's last trip adds radiance), 80 / 88 (compact), 88 / 96 / 104 / 168 (wide);
                                 0 for the PRB adjoint  [v108] */
    uint64_t n_closed_guard;  /* 64-byte records: trips that broke the layout's premise (nonzero radiance on a path that
                                 goes on, an emitter hit that needs its MIS weight); the render then fails  [v108] */
    uint64_t n_proven;        /* 64-byte records: records read whose segment was proven free of surfaces (by the distance
                                 field or the per-face cone table) and ran without a ray query; 0 for every other kernel  [v115] */
    uint64_t n_primary_entry; /* 64-byte records: camera lanes whose first ray query started below the BVH's root, or was skipped because no
                                 triangle projects into the pixel (the per-pixel primary entry); 0 for every other kernel  [v121] */
} lrt_render_stats;

typedef struct {
    float d_sigma_t[3];       /* homogeneous medium: w.r.t. the `sigma_t` property (before `scale`), per channel.
                                 heterogeneous medium [v104]: channel k's share of d / d(scale); the three add up to the derivative
                                 w.r.t. the medium's `scale` (sigma_t(p) = scale * grid(p); the majorant is detached,
                                 src/media/heterogeneous.cpp parameters_changed) */
    float d_albedo[3];
    float d_g;
} lrt_param_grads;

typedef struct lrt_scene lrt_scene;

LRT_API const char *lrt_last_error(void);
LRT_API int         lrt_version(void);   /* 121: lrt_render_stats.n_primary_entry appended (lrt_render_stats_get writes 8 bytes more: rebuild hosts against this header); 119: the conductor, plastic and twosided BSDFs (LRT_BSDF_CONDUCTOR / _PLASTIC / _TWOSIDED, the fields after `specular_transmittance` of lrt_bsdf_desc); 118: lrt_medium_probe; the loader refuses a singular volume to_world and an empty use_grid_bbox header box; 117: spot and directional emitters (LRT_EMITTER_SPOT / _DIRECTIONAL, lrt_emitter_desc grows by cutoff_angle, beam_width, texture: rebuild hosts against this header); 116: tabulated, Rayleigh and blended phase functions (lrt_phase_desc, lrt_scene_desc.phases, lrt_medium_desc.phase_index), lrt_phase_probe, lrt_math_eval fn 11; 115: lrt_render_stats.n_proven appended (lrt_render_stats_get writes 8 bytes more: rebuild hosts against this header); 114: the roughdielectric BSDF (LRT_BSDF_ROUGHDIELECTRIC, the fields after `scale` of lrt_bsdf_desc), lrt_math_eval fn 9 / 10; 113: lrt_bsdf_probe; 112:lrt_render_backward_grid, "<id>.sigma_t.data" parameter keys; 111: lrt_envmap_probe; 110: the moment integrator (lrt_render_moment, lrt_moment_desc); 109: the guided denoiser (lrt_denoiser_create, lrt_denoise, lrt_denoiser_free); 108: lrt_render_stats.record_bytes / n_closed_guard; 107: area emitters on triangle meshes, lrt_emitter_probe; 106: spheres, point emitters */

LRT_API lrt_status lrt_scene_load_xml(const char *path, const char *const *defines,
                                      int n_defines, lrt_scene **out);
LRT_API lrt_status lrt_scene_load_xml_string(const char *xml, const char *base_dir,
                                             const char *const *defines, int n_defines,
                                             lrt_scene **out);
LRT_API lrt_status lrt_scene_from_desc(const lrt_scene_desc *desc, lrt_scene **out);
LRT_API const lrt_scene_desc *lrt_scene_desc_get(const lrt_scene *scene);
LRT_API void       lrt_scene_free(lrt_scene *scene);

/* film_raw: crop_h * crop_w * C floats (C = 5 if has_alpha else 4: R,G,B,[A],W),
 * image:    crop_h * crop_w * (4 if has_alpha else 3) developed floats.
 * Either may be NULL.  Both are overwritten: the film is cleared before the samples are accumulated (ImageBlock::clear, as
 * Film::prepare / SamplingIntegrator::render do before a render); with opts->output_on_device the two pointers are device
 * memory and the call returns after the library's stream has finished with them.  A tile shard (tile_count > 1) fills only
 * its own tiles' samples into the full-size film: shard films add up to the unsharded film.
 * On a scene loaded with an `aov` integrator this renders the description's integrator (the first nested one): see lrt_render_aov;
 * on one loaded with a `moment` integrator [v110] the nested integrator alone: see lrt_render_moment.  */
LRT_API lrt_status lrt_render(lrt_scene *scene, const lrt_render_opts *opts,
                              float *film_raw, float *image);
LRT_API lrt_status lrt_render_stats_get(const lrt_scene *scene, lrt_render_stats *out);
/* The per-pixel primary entry of the scene's device image [v121]: out[y * crop_w + x] = the 16-bit item at which a camera ray of that pixel starts
 * its BVH traversal in the 64-byte-record volpath kernels: 0 = the root (also: the image has no table), 0x8000 | s = the leaf whose first
 * triangle slot is s, 0xffff = no triangle can be hit, any other value = that inner node.  n_pixels must be crop_w * crop_h.  Test access. */
LRT_API lrt_status lrt_primary_entry_get(lrt_scene *scene, uint16_t *out, uint64_t n_pixels, int device);

LRT_API lrt_status lrt_film_develop(lrt_scene *scene, const float *film_raw, float *image,
                                    int on_device);

/* Test hook: per-lane radiance of wavefront lanes [lane_begin, lane_begin+n)
 * of the render described by opts, without film accumulation (of its FIRST pass
 * when `samples_per_pass` or the 2^32 - 1 limit splits the render: lanes then
 * count spp_per_pass samples per pixel).  out: n * 4 floats {R, G, B, valid}.  */
LRT_API lrt_status lrt_render_samples(lrt_scene *scene, const lrt_render_opts *opts,
                                      uint64_t lane_begin, uint32_t n, float *out);

/* PRB adjoint: d(sum(image * grad_image)) / d(sigma_t, albedo, g) of medium opts->grad_medium (the reference
 * differentiates whichever parameters have gradients enabled: one call per medium gives the same numbers).
 * Homogeneous and [v104] heterogeneous media (null collisions, src/python/python/ad/integrators/prbvolpath.py:178-196,
 * 404-415); the bio media are rejected (LRT_ERR_UNSUPPORTED): the reference's prbvolpath reads them as homogeneous. */
LRT_API lrt_status lrt_render_backward(lrt_scene *scene, const lrt_render_opts *opts,
                                       const float *grad_image, lrt_param_grads *out);

/* [v112] lrt_render_backward plus the gradient w.r.t. the sigma_t grid of ONE heterogeneous medium (what dr.backward leaves in
 * mi.traverse(scene)["<medium>.sigma_t.data"]; src/python/python/ad/integrators/prbvolpath.py on src/media/heterogeneous.cpp).
 * opts->grad_medium must be the index of a heterogeneous medium; anything else, -1 included, is LRT_ERR_INVALID.
 * d_grid: res_x * res_y * res_z floats in the layout of grid_data (x fastest); overwritten, not accumulated into; with
 * opts->output_on_device a device pointer (grad_image too, as in lrt_render_backward).  It is the derivative w.r.t. the raw grid
 * values, before `scale`: sigma_t(p) = scale * sum_v w_v(p) grid[v] with the trilinear weights of src/volumes/grid.cpp.  The majorant
 * is detached (parameters_changed).  `out` receives what lrt_render_backward returns for the same arguments.  tile_rank / tile_count
 * as there: shard gradients add up.  The per-voxel sums are float atomic adds whose order of arrival varies: d_grid may differ in its
 * last bits from run to run.  Moment and aov scenes are LRT_ERR_UNSUPPORTED, as are the scenes prbvolpath rejects; there is no
 * multi-device form. */
LRT_API lrt_status lrt_render_backward_grid(lrt_scene *scene, const lrt_render_opts *opts, const float *grad_image,
                                            lrt_param_grads *out, float *d_grid);

/* One process, several devices [v104] (SURVEY.md 8e through the C ABI; no reference counterpart: the reference renders on one device):
 * device i of the list (device_ids, or 0 .. n_devices - 1 when NULL) renders the 32x32 tiles t with t % n_devices == i into its own
 * full-size zeroed film with GLOBAL lane ids - one host thread and one stream per device -, ONE ncclAllReduce (RCCL, bound at run time
 * from /opt/rocm/lib/librccl.so; LRT_RCCL_LIBRARY overrides) sums the films, the first device develops.  film_raw / image as in
 * lrt_render (with output_on_device: pointers on the first device of the list).  The result is the image lrt_render gives (up to the
 * order of the float sums).  opts->tile_rank / tile_count / device are ignored (must be unset).  A list that names ONE device several
 * times is a rehearsal for boxes with a single GPU: the peers' films are added on that device, no collective runs.
 * lrt_render_backward_multi: the same sharding for the PRB adjoint; the 7 gradient sums are reduced with one all-reduce.
 * What the reference-side C++ plugin calls from SamplingIntegrator::render / render_backward
 * (include/mitsuba/render/integrator.h:74, :253) to use a whole node without a second process. */
LRT_API lrt_status lrt_render_multi(lrt_scene *scene, const lrt_render_opts *opts, int n_devices, const int *device_ids,
                                    float *film_raw, float *image);
LRT_API lrt_status lrt_render_backward_multi(lrt_scene *scene, const lrt_render_opts *opts, int n_devices, const int *device_ids,
                                             const float *grad_image, lrt_param_grads *out);

/* Test hook [v104]: the device's own log / exp / sincos / atan2 / acos / log2 kernels (csrc/dmath.h: the arithmetic every path value
 * goes through, standing in for Dr.Jit's dr::log / dr::exp / ... of include/mitsuba/core/math.h users) and its division / sqrt / rcp,
 * one value per lane.  fn: 0 log(x), 1 exp(x), 2 sincos(x) -> out, out2, 3 atan2(y, x), 4 acos(x), 5 log2(x), 6 x / y, 7 sqrt(x), 8 1 / x,
 * [v114] 9 erf(x), 10 erfinv(x) (Beckmann's visible-normal sampling, csrc/dshade.h),
 * [v116] 11 cbrt(x) (the Rayleigh phase function's inversion, csrc/dshade.h). */
LRT_API lrt_status lrt_math_eval(int fn, const float *x, const float *y, uint32_t n, float *out, float *out2, int device);

/* Test hook [v107]: Scene::sample_emitter_direction of the render kernels that serve spheres, point emitters and mesh
 * emitters (csrc/dshade.h), on the device, for n reference points ref_p[3 i ..] and samples sample[2 i ..]; then a ray
 * query from ref_p along the sampled direction and, at its hit, the emitter pdf and emitted radiance the integrators use.
 * out: LRT_PROBE_FLOATS floats per input:
 *   [0..2] p, [3..5] n, [6..8] d, [9] dist, [10] pdf, [11..13] weight (radiance / pdf), [14] emitter index (-1: none),
 *   [15] shape of the hit (-1: miss), [16] pdf_emitter_direction at the hit (0 if the shape carries no emitter),
 *   [17..19] emitter_eval at the hit (area.cpp eval: one-sided through the shading frame).  Indices are stored as floats. */
#define LRT_PROBE_FLOATS 20
LRT_API lrt_status lrt_emitter_probe(lrt_scene *scene, const float *ref_p, const float *sample, uint32_t n, float *out, int device);

/* Test hook [v111]: the environment emitter at n given world directions dir[3 i ..], as the integrators evaluate it for a ray that
 * leaves the scene: out[4 i] = Scene::pdf_emitter_direction for the miss (the factor 1 / n_emitters included), out[4 i + 1 .. 3] =
 * the emitter's eval.  LRT_ERR_* if the scene has no environment emitter. */
LRT_API lrt_status lrt_envmap_probe(lrt_scene *scene, const float *dir, uint32_t n, float *out, int device);

/* Test hook [v113]: the surface code of the render kernels (csrc/dshade.h) at chosen rays, one per lane.  For input i: a closest-hit
 * query along (o[3 i ..], d[3 i ..]) over triangles and spheres, without a ray offset (Scene::ray_intersect); the surface
 * interaction of the hit (Mesh / Sphere::compute_surface_interaction: p, n, sh_frame, uv, wi); then, on the hit shape's BSDF,
 * BSDF::sample(ctx, si, sample[3 i], (sample[3 i + 1], sample[3 i + 2])) in radiance mode as the integrators draw it, and
 * BSDF::eval / BSDF::pdf(ctx, si, si.to_local(wo_query[3 i ..])) as they evaluate it for an emitter sample.
 * out: LRT_BSDF_PROBE_FLOATS floats per input:
 *   [0] shape of the hit (-1: miss, the rest is then 0), [1] t, [2..4] p, [5..7] n (geometric), [8..10] sh_frame.n, [11..12] uv,
 *   [13..15] wi (local); the sample: [16..18] si.to_world(bs.wo), [19] bs.wo.z (local), [20] bs.pdf, [21] bs.eta,
 *   [22] bs.sampled_type as this library keeps it (1 delta, 2 smooth, 4 null, 0 none), [23..25] the BSDF weight;
 *   [26..28] eval and [29] pdf at wo_query.  Indices are stored as floats. */
#define LRT_BSDF_PROBE_FLOATS 30
LRT_API lrt_status lrt_bsdf_probe(lrt_scene *scene, const float *o, const float *d, const float *sample, const float *wo_query,
                                  uint32_t n, float *out, int device);

/* Test hook [v116]: the phase function of medium `medium` as the EXT render kernels call it (csrc/dshade.h phase_sample<true> /
 * phase_eval<true>), one call per lane, whatever the medium's phase type.  For input i: PhaseFunction::sample(ctx, mei with
 * wi = wi[3 i ..], sample[3 i], (sample[3 i + 1], sample[3 i + 2])) and PhaseFunction::eval_pdf(ctx, mei, wo_query[3 i ..]).
 * out: LRT_PHASE_PROBE_FLOATS floats per input: [0..2] the sampled wo, [3] its weight, [4] its pdf, [5] eval and [6] pdf at wo_query. */
#define LRT_PHASE_PROBE_FLOATS 7
LRT_API lrt_status lrt_phase_probe(lrt_scene *scene, int medium, const float *wi, const float *sample, const float *wo_query,
                                   uint32_t n, float *out, int device);

/* Test hook [v118]: free-flight sampling in medium `medium` as the volume integrators call it (csrc/dshade.h het_sample_interaction for a
 * heterogeneous medium, medium_sample_interaction otherwise), one call per lane: Medium::sample_interaction(ray(o[3 i ..], d[3 i ..],
 * maxt[i]), sample[i], channel[i]) (src/render/medium.cpp:40-82); channel > 2 counts as 2.
 * out: LRT_MEDIUM_PROBE_FLOATS floats per input:
 *   [0] 1 if the interaction is valid else 0, [1] t (+inf when not valid), [2..4] p = o + sampled_t d (also when not valid), [5] mint,
 *   [6..8] sigma_t, [9..11] sigma_s, [12..14] sigma_n, [15..17] combined extinction (the majorant);
 *   a grid medium also: [18..20] to_local(p) in the grid's unit cube and [21] the raw grid lookup there (no `scale`); else 0.
 * A lane whose maxt is NaN asks for the grid lookup alone: o[3 i ..] is then the local point, anywhere in space (clamp-to-edge outside the unit
 * cube); [18..21] are written, [0..17] are 0. */
#define LRT_MEDIUM_PROBE_FLOATS 22
LRT_API lrt_status lrt_medium_probe(lrt_scene *scene, int medium, const float *o, const float *d, const float *maxt, const float *sample,
                                    const uint32_t *channel, uint32_t n, float *out, int device);

/* Test hook [v120]: the front and the back end of every lane, one call per lane: the perspective sensor's ray as generate_camera_path asks
 * for it (csrc/kernels.h camera_ray), the film-to-sample map, a sample's filter footprint (csrc/film.h film_footprint) and the
 * reconstruction filter (rfilter_eval).  in: 5 floats per lane: [0..1] the adjusted position sample (ax, ay) handed to
 * PerspectiveCamera::sample_ray, [2..3] a film position (spx, spy) in pixels, [4] a filter argument x.
 * out: LRT_SENSOR_PROBE_FLOATS floats per lane:
 *   [0..2] ray origin, [3..5] ray direction, [6] maxt of sample_ray(ax, ay);
 *   [7..8] fma(spx, scale_x, offset_x), fma(spy, scale_y, offset_y): the film-to-sample map (scale = 1 / crop_size, offset = -crop_offset * scale);
 *   [9..10] the footprint origin of a sample at (spx, spy) in film pixels, stored as floats, [11..12] relx, rely: the filter argument of the
 *   footprint's first column and row (cell k has rel + k);  [13] the filter at x;  [14] the footprint's cells per side;  [15] 0. */
#define LRT_SENSOR_PROBE_FLOATS 16
LRT_API lrt_status lrt_sensor_probe(lrt_scene *scene, const float *in, uint32_t n, float *out, int device);

/* SoA ray queries (layout mirrors RayHit of src/render/scene_native.inl:135-142).
 * Miss: t = +inf, prim = 0xffffffff.  any_hit: only t (0 on hit, +inf on miss). */
typedef struct { const float *ox, *oy, *oz, *dx, *dy, *dz, *tmax; } lrt_rays_soa;
typedef struct { float *t, *u, *v; uint32_t *prim; } lrt_hits_soa;
LRT_API lrt_status lrt_trace(lrt_scene *scene, const lrt_rays_soa *rays,
                             const lrt_hits_soa *hits, uint32_t n, int any_hit);

/* Keys follow mi.traverse(): "<medium id>.sigma_t.value" (3 floats),
 * "<medium id>.albedo.value" (3), "<medium id>.scale" (1),
 * "<medium id>.phase_function.g" (1; switches the phase to HG when != 0);
 * a `parenchyma` medium also has what src/media/parenchyma.cpp:154-160 traverses:
 * "<id>.sigma_blood.value", "<id>.sigma_bile.value", "<id>.sigma_lipid_water.value" (3 each)
 * and "<id>.sigma_hepatocity" (1).
 * [v112] a heterogeneous medium also has "<id>.sigma_t.data": the grid values, n = res_x * res_y * res_z floats in the layout
 * of grid_data (x fastest).  A set needs finite values >= 0 with a maximum above 0 (LRT_ERR_INVALID otherwise, the scene unchanged);
 * it replaces what lrt_scene_desc_get()->media[i].grid_data points to (the pointer stays), takes grid_max again (the majorant is
 * scale * grid_max) and has the next render upload the grid.  The resolution is fixed at load time.                  */
LRT_API lrt_status lrt_param_set(lrt_scene *scene, const char *key, const float *v, int n);
LRT_API lrt_status lrt_param_get(const lrt_scene *scene, const char *key, float *v, int n);

/* Image files around the path (mi.Bitmap(path) / Bitmap.write, src/core/bitmap.cpp): 8/16-bit PNG and
 * scanline OpenEXR (NONE/ZIPS/ZIP/PIZ) readers, uncompressed float32 EXR writer, 8-bit sRGB PNG writer.  *data is
 * h * w * channels floats in R,G,B[,A] (or Y[,A]) order, PNG values in [0,1] as stored (no
 * gamma conversion); release it with lrt_image_free.  */
LRT_API lrt_status lrt_image_read(const char *path, int *width, int *height, int *channels, float **data);
LRT_API void       lrt_image_free(float *data);
LRT_API lrt_status lrt_image_write_exr(const char *path, int width, int height, int channels, const float *data);
/* 8-bit PNG of a LINEAR float image, the export step of LiverRenderer.py:383-385
 * (Bitmap.convert(RGBA, UInt8, srgb_gamma=True) + write): colour channels through the sRGB transfer
 * function, alpha linear, clamped to [0,1], rounded to nearest; 1 to 4 channels.  The reference's
 * blue-noise dithering of 8-bit conversions (src/core/struct.cpp:823-845) is not applied: values agree
 * with its PNGs to within one code value.                                                    */
LRT_API lrt_status lrt_image_write_png(const char *path, int width, int height, int channels, const float *data);

/* ---------------------------------------------------------------------------------------------------------------
 * The `aov` integrator [v105] (src/integrators/aov.cpp): first-hit AOVs of the primary ray beside the images of nested
 * integrators.  An XML `<integrator type="aov">` keeps the scene description an ordinary one: lrt_scene_desc.integrator holds
 * the FIRST nested integrator (path defaults when there is none), so lrt_render on an aov scene renders that integrator alone.
 * The AOV configuration lives beside the description:                                                                 */
#define LRT_AOV_MAX_INTEGRATORS 4
#define LRT_AOV_MAX_AOVS        16
#define LRT_AOV_NAME_LEN        64
/* AOV types (aov.cpp:142-196); duv_dx / duv_dy need ray differentials and are rejected (LRT_ERR_UNSUPPORTED) */
enum { LRT_AOV_ALBEDO = 0,       /* .R .G .B  BSDF::eval_diffuse_reflectance                         */
       LRT_AOV_DEPTH = 1,        /* .T        hit distance, 0 on a miss                              */
       LRT_AOV_POSITION = 2,     /* .X .Y .Z                                                         */
       LRT_AOV_UV = 3,           /* .U .V                                                            */
       LRT_AOV_GEO_NORMAL = 4,   /* .X .Y .Z                                                         */
       LRT_AOV_SH_NORMAL = 5,    /* .X .Y .Z  BSDF::sh_frame(si).n (bumpmap: in the local frame, as the reference returns it) */
       LRT_AOV_DP_DU = 6,        /* .X .Y .Z                                                         */
       LRT_AOV_DP_DV = 7,        /* .X .Y .Z                                                         */
       LRT_AOV_PRIM_INDEX = 8,   /* .I        triangle index within its shape                        */
       LRT_AOV_SHAPE_INDEX = 9   /* .I        1 + index into shapes[], 0 on a miss                   */ };

typedef struct {
    int32_t n_integrators;                                           /* nested integrators, in file order              */
    lrt_integrator_desc integrators[LRT_AOV_MAX_INTEGRATORS];
    char    integrator_names[LRT_AOV_MAX_INTEGRATORS][LRT_AOV_NAME_LEN];
    int32_t n_aovs;
    int32_t aov_types[LRT_AOV_MAX_AOVS];                             /* LRT_AOV_*                                      */
    char    aov_names[LRT_AOV_MAX_AOVS][LRT_AOV_NAME_LEN];
    int32_t n_aov_channels;   /* channels of the AOVs alone (the AOV film has n_aov_channels + 1: ..., W)                 */
    int32_t n_channels;       /* developed output channels: the inner images' R,G,B[,A] each, then the AOV channels       */
} lrt_aov_desc;

/* LRT_ERR_INVALID when the scene has no aov integrator. */
LRT_API lrt_status lrt_scene_aov_get(const lrt_scene *scene, lrt_aov_desc *out);
/* Name of developed output channel c (0 <= c < n_channels): "<integrator name>.R" ... then "<aov name>.<suffix>"; NULL when
 * the scene has no aov integrator or c is out of range.  The string lives as long as the scene. */
LRT_API const char *lrt_aov_channel_name(const lrt_scene *scene, int c);
/* AOVIntegrator::render (aov.cpp:369-395): every nested integrator renders as lrt_render would render it alone (same spp,
 * seed), then one first-hit pass over all camera samples accumulates the AOVs through the reconstruction filter.
 * image:        crop_h * crop_w * n_channels developed floats (merge_channels, aov.cpp:523-545); may be NULL.
 * aov_film_raw: crop_h * crop_w * (n_aov_channels + 1) floats, the AOV pass's own film (AOV channels, then W); may be NULL.
 * opts->integrator / max_depth / rr_depth / hide_emitters must be "use the scene's" (LRT_ERR_INVALID otherwise); spp, seed,
 * device and output_on_device as in lrt_render.  tile_count > 1 is LRT_ERR_UNSUPPORTED, and so are lrt_render_multi,
 * lrt_render_backward and lrt_render_backward_multi on an aov scene; so is a render in several passes of the independent
 * sampler with two or more nested integrators.                                                                        */
LRT_API lrt_status lrt_render_aov(lrt_scene *scene, const lrt_render_opts *opts, float *aov_film_raw, float *image);
/* Test hook: the AOV values of lanes [lane_begin, lane_begin + n) of the AOV pass before film accumulation (its first pass
 * only): out is n * n_aov_channels floats. */
LRT_API lrt_status lrt_render_aov_samples(lrt_scene *scene, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out);
/* Multi-channel float32 EXR with named channels (uncompressed; channel list sorted by name as OpenEXR requires, data
 * permuted to match).  data: h * w * n_channels floats in the order of `names`. */
LRT_API lrt_status lrt_image_write_exr_channels(const char *path, int width, int height, int n_channels,
                                                const char *const *names, const float *data);

/* ---------------------------------------------------------------------------------------------------------------
 * The `moment` integrator [v110] (src/integrators/moment.cpp, *_rgb variants): beside the nested integrator's image, per pixel,
 * the first and second moments of its samples in CIE XYZ - what a variance image and the Z-test of
 * src/render/tests/test_renders.py:159-228 are computed from.  As with `aov`, the scene description stays an ordinary one:
 * lrt_scene_desc.integrator holds the nested integrator, so lrt_render on a moment scene renders that integrator alone.
 * Per camera sample with radiance L (path.cpp:342-345 zeroes an invalid sample first), DESIGN.md section 10.1:
 *   X = fmaf(m02, B, fmaf(m01, G, m00 * R)), Y and Z with rows 1 and 2 of srgb_to_xyz (include/mitsuba/core/spectrum.h:396-402),
 *   m2_X = X * X, ... - all in float32, and all channels go through the reconstruction filter with the sample's weight.
 * Raw film:        R, G, B, [A], W, X, Y, Z, m2_X, m2_Y, m2_Z     (n_raw_channels: 10, 11 with alpha; hdrfilm.cpp:245-258)
 * Developed image: R, G, B, [A],    X, Y, Z, m2_X, m2_Y, m2_Z     (n_channels: 9 or 10), each divided by W (by 1 where W = 0).
 * One nested integrator (path, volpath, volpathmis, biovolpath, biovolpath06); two or more, a nested aov / moment / prbvolpath:
 * LRT_ERR_UNSUPPORTED at load time; none: LRT_ERR_INVALID, as in the reference.                                            */
typedef struct {
    lrt_integrator_desc integrator;          /* the nested integrator (= lrt_scene_desc.integrator)                            */
    char    name[LRT_AOV_NAME_LEN];          /* its property name: the XML `name`, the dict key, "_arg_0" for an unnamed child  */
    int32_t n_channels;                      /* developed channels                                                             */
    int32_t n_raw_channels;                  /* film channels (with W)                                                         */
} lrt_moment_desc;
/* LRT_ERR_INVALID when the scene has no moment integrator. */
LRT_API lrt_status lrt_scene_moment_get(const lrt_scene *scene, lrt_moment_desc *out);
/* Name of developed channel c (0 <= c < n_channels): "R", "G", "B", ["A"], "<name>.X", ".Y", ".Z", "m2_<name>.X", ".Y", ".Z";
 * NULL when the scene has no moment integrator or c is out of range.  The string lives as long as the scene. */
LRT_API const char *lrt_moment_channel_name(const lrt_scene *scene, int c);
/* film_raw: crop_h * crop_w * n_raw_channels floats; image: crop_h * crop_w * n_channels floats; either may be NULL.  Passes
 * (samples_per_pass), crop windows, output_on_device, tile_rank / tile_count (the film is linear in the samples: shard films add
 * up) and the statistics are those of lrt_render.  opts->integrator / max_depth / rr_depth / hide_emitters must be "use the
 * scene's" (LRT_ERR_INVALID otherwise).  lrt_render_multi, lrt_render_backward and lrt_render_backward_multi on a moment scene
 * are LRT_ERR_UNSUPPORTED. */
LRT_API lrt_status lrt_render_moment(lrt_scene *scene, const lrt_render_opts *opts, float *film_raw, float *image);
/* Test hook: X, Y, Z, m2_X, m2_Y, m2_Z of lanes [lane_begin, lane_begin + n) before film accumulation (first pass only, as
 * lrt_render_samples), through the device function the film kernel uses: out is n * 6 floats. */
LRT_API lrt_status lrt_render_moment_samples(lrt_scene *scene, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out);

/* ---------------------------------------------------------------------------------------------------------------
 * Learned subsurface model, network stage only: the shape-adaptive scatter network of
 * include/mitsuba/render/scattereigen.h:249-480 (ScatterModelSimShared<3, 4, 64, 64>::run): feature MLP 23 -> 64 -> 64 -> 64,
 * absorption head 64 -> 32 -> 1 (sigmoid, one sampler draw), decoder (4 Gaussian latents + 64) -> 64 -> 64 -> 64 -> 3, result
 * mapped from the tangent frame of -in_dir to world space and scaled by 1 / fit_scale.  docs/SUBSURFACE_NOTES.md explains
 * why the plugin around it (src/subsurface/vaescatter.cpp) is not built.
 *
 * Weights: one float32 blob in this order (row-major matrices, rows = outputs), as the .bin files of
 * pysrc/outputs/vae3d/models/<model>/variables/ hold them, preceded by the normalisation statistics of
 * pysrc/outputs/vae3d/datasets/<dataset>/train/data_stats.json ("effAlbedo", "g", "mlsPoly3"):                       */
#define LRT_VAE_STATS        0      /* albedo mean, albedo 1/std, g mean, g 1/std, shape mean[20], shape 1/std[20]        */
#define LRT_VAE_PRE0_W      44      /* shared_preproc_mlp_2_shapemlp_fcn_0_weights [64][23], then _biases [64]            */
#define LRT_VAE_PRE1_W    (LRT_VAE_PRE0_W + 64 * 23 + 64)      /* fcn_1 [64][64] + [64]                                   */
#define LRT_VAE_PRE2_W    (LRT_VAE_PRE1_W + 64 * 64 + 64)      /* fcn_2 [64][64] + [64]                                   */
#define LRT_VAE_ABS0_W    (LRT_VAE_PRE2_W + 64 * 64 + 64)      /* absorption_mlp_fcn_0 [32][64] + [32]                    */
#define LRT_VAE_ABSD_K    (LRT_VAE_ABS0_W + 32 * 64 + 32)      /* absorption_dense_kernel [32] + bias [1]                 */
#define LRT_VAE_DEC0_W    (LRT_VAE_ABSD_K + 32 + 1)            /* scatter_decoder_fcn_fcn_0 [64][68] + [64]               */
#define LRT_VAE_DEC1_W    (LRT_VAE_DEC0_W + 64 * 68 + 64)      /* fcn_1 [64][64] + [64]                                   */
#define LRT_VAE_DEC2_W    (LRT_VAE_DEC1_W + 64 * 64 + 64)      /* fcn_2 [64][64] + [64]                                   */
#define LRT_VAE_OUT_K     (LRT_VAE_DEC2_W + 64 * 64 + 64)      /* scatter_dense_2_kernel [3][64] + bias [3]               */
#define LRT_VAE_N_FLOATS  (LRT_VAE_OUT_K + 3 * 64 + 3)
typedef struct lrt_vae_model lrt_vae_model;
LRT_API lrt_status lrt_vae_model_create(const float *blob, uint64_t n_floats, lrt_vae_model **out);
LRT_API void       lrt_vae_model_free(lrt_vae_model *model);
/* n samples; sample i uses in_pos[3i..], in_dir[3i..], poly_coeffs[20i..] (the order-3 polynomial of the surface around in_pos,
 * in the network's "LS" space) and its own PCG32 stream seeded like a render lane (TEA(seed, i)).  Outputs: out_pos[3i..] and
 * out_absorption[i] (1: the sample was absorbed, out_pos = in_pos; 0: out_pos is the predicted exit point).  Host pointers. */
LRT_API lrt_status lrt_vae_scatter(lrt_vae_model *model, uint32_t n, const float *in_pos, const float *in_dir,
                                   const float *poly_coeffs, const float albedo[3], float g, float ior,
                                   const float sigma_t[3], float fit_scale, uint32_t seed,
                                   float *out_pos, float *out_absorption, int device);

/* ---------------------------------------------------------------------------------------------------------------
 * Guided denoiser [v109]: the place of mi.OptixDenoiser (include/mitsuba/render/optixdenoiser.h) in the reference's workflow
 * (Denoise.py; --imode optix, src/mitsuba/realtime.hpp:501-508).  OptiX's network is closed and NVIDIA-only; behind the same
 * interface runs the edge-avoiding A-Trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) with albedo demodulation,
 * specified operation by operation in DESIGN.md section 9.
 * A field of lrt_denoise_params that is 0 takes its default; a negative or non-finite one is LRT_ERR_INVALID, and so is
 * `iterations` outside 1 .. LRT_DENOISE_MAX_ITERATIONS.                                                                   */
#define LRT_DENOISE_MAX_ITERATIONS    8
#define LRT_DENOISE_ITERATIONS        5
#define LRT_DENOISE_SIGMA_COLOR       0.3f
#define LRT_DENOISE_SIGMA_NORMAL      0.1f
#define LRT_DENOISE_SIGMA_ALBEDO      0.05f
#define LRT_DENOISE_EPS_A             0.5f      /* defaults: scripts/study/denoise_study.py, DESIGN.md section 9.3 */
#define LRT_DENOISE_MAX_SIZE          16384    /* width and height */
typedef struct {
    int32_t iterations;       /* passes N, step 2^k in pass k                          */
    float   sigma_color;      /* colour tolerance of pass 0; halves every pass         */
    float   sigma_normal;
    float   sigma_albedo;
    float   eps_a;            /* floor of the demodulation divisor max(albedo, eps_a)  */
} lrt_denoise_params;
typedef struct lrt_denoiser lrt_denoiser;
/* Allocates the workspace (packed planes, ping-pong colour, staging) for width x height on `device` and a non-blocking stream;
 * params may be NULL (all defaults).  The arguments are checked before the device is touched. */
LRT_API lrt_status lrt_denoiser_create(int width, int height, int use_albedo, int use_normals, int denoise_alpha,
                                       const lrt_denoise_params *params, int device, lrt_denoiser **out);
/* noisy / out: height * width * channels floats, channels 3 or 4 (R,G,B[,A]); albedo / normals: height * width * 3 floats,
 * required exactly when the denoiser was created with that guide (NULL otherwise: LRT_ERR_INVALID either way round).  Alpha is
 * filtered when the denoiser was created with denoise_alpha and channels is 4, copied through otherwise.  With device_buffers
 * all four pointers are device memory on the denoiser's device (as lrt_render_opts.output_on_device): the caller has finished
 * writing the inputs, and the call returns after the denoiser's stream has finished with all of them.  out must not alias an input. */
LRT_API lrt_status lrt_denoise(lrt_denoiser *denoiser, const float *noisy, int channels, const float *albedo, const float *normals,
                               float *out, int device_buffers);
LRT_API void       lrt_denoiser_free(lrt_denoiser *denoiser);
/* The parameters a denoiser runs with (defaults resolved) and its size. */
LRT_API lrt_status lrt_denoiser_get(const lrt_denoiser *denoiser, int *width, int *height, lrt_denoise_params *params);
/* lrt_image_read that also reports the file's channel names (EXR: EVERY channel of the file, R,G,B[,A] or Y[,A]
 * first when the file has them, the others after them in file order, e.g. "albedo.R"; PNG: no names, the data of lrt_image_read): *names is one string of the names in data order, separated by '\n', released with lrt_image_free_names; empty
 * when the file has none. */
LRT_API lrt_status lrt_image_read_named(const char *path, int *width, int *height, int *channels, float **data, char **names);
LRT_API void       lrt_image_free_names(char *names);

#ifdef __cplusplus
}
#endif
#endif /* LIVERRT_H */
