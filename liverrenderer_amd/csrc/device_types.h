// POD structures shared by the host driver (render.cpp side of device.hip) and
// the gfx950 kernels.  Uniform scene data is passed to kernels BY VALUE
// (kernarg segment -> scalar loads), bulk data by pointer.
#pragma once
#include <stdint.h>
#include <hip/hip_vector_types.h>

namespace lrt {

struct DShape {
    int32_t bsdf, emitter, interior_medium, exterior_medium;
    int32_t has_normals, has_texcoords, flip_normals, kind;
};

// 32 bytes, as before the roughdielectric: its fields live in the words it leaves unused (a diffuse reflectance, a bumpmap's nested
// BSDF, height texture and scale), so the table stride and every other BSDF's loads stay what they were.
#define LRT_MICRO_GGX 1        // DBsdf::micro: distribution (else beckmann)
#define LRT_MICRO_VISIBLE 2    //               sample_visible
struct DBsdf {
    int32_t type;
    union { int32_t reflectance; int32_t specular_reflectance; };     // texture index; roughdielectric: -1 = none
    union { int32_t nested; int32_t micro; };                         // roughdielectric: LRT_MICRO_* bits
    union { int32_t texture; int32_t specular_transmittance; };
    float eta;
    union { float scale; float alpha_u; };                            // roughdielectric: alphas, clamped to >= 1e-4 by the host
    int32_t flags;
    union { int32_t pad; float alpha_v; };
};
static_assert(sizeof(DBsdf) == 32, "DBsdf stride");
// conductor: specular_reflectance, flags; the complex index lives in DBsdfExt.  plastic: reflectance (= diffuse_reflectance), eta, flags; the rest
// in DBsdfExt.  twosided: nested (= the front child), flags (= the union of the children's); the back child in DBsdfExt.

// What conductor / plastic / twosided need beyond those 32 bytes (src/bsdfs/conductor.cpp, plastic.cpp, twosided.cpp): DScene::bsdf_ext, one
// row per BSDF, indexed like DScene::bsdfs (all zero for every other type); null when the scene has none of the three.  Four 16-byte words:
// one row is four vector (or scalar) loads.
struct alignas(16) DBsdfExt {
    float eta[3]; float inv_eta_2;       // conductor: real part of the index per channel | plastic: 1 / eta^2 (plastic.cpp:193)
    float k[3]; float fdr_int;           // conductor: imaginary part               | plastic: fresnel_diffuse_reflectance(1 / eta) (:196)
    float fdr_ext, spec_weight;          // plastic: fresnel_diffuse_reflectance(eta) (:197), specular_sampling_weight (:200-206)
    int32_t nonlinear, specular_reflectance;   // plastic: `nonlinear`; its specular_reflectance texture, -1: none
    int32_t back; int32_t pad[3];        // twosided: the back child (= DBsdf::nested when there is one child: the same-child branch, twosided.cpp:124)
};
static_assert(sizeof(DBsdfExt) == 64, "DBsdfExt stride");

struct DTexture {
    int32_t type, width, height, channels;
    float color0[3]; float color1[3];
    float to_uv[6];            // first two rows of the 3x3 uv transform
    uint32_t data_offset;      // into tex_data (floats); bitmap: 1 float per texel (luminance or Y)
    uint32_t pad;
};

struct DMedium {
    float sigma_t[3]; float albedo[3];   // sigma_t already multiplied by scale
    int32_t has_spectral_extinction, sample_emitters, phase; float g;
    float scale; int32_t het;            // sigma_t = property * scale (needed by the PRB adjoint); het: heterogeneous (sc.het[index])
    float w_spec[3], w_plain[3];         // real-scattering weights sigma_s / mean(sigma_t / combined), sigma_s / sigma_t (k_medium_prepare)
    float nee_vmin[3];                   // per channel: 1 - u >= nee_vmin proves that the free-flight distance -log(1 - u) / sigma_t stays below the distance
    int32_t phase_ext;                   // of every sample of an infinite emitter (upload_media; volpath_iteration's early NEE rejection)
    float pad2[2];                       // phase_ext: 1 + the medium's entry in DScene::phases, 0: `phase` / `g` above (the EXT instances only read it)
};
static_assert(sizeof(DMedium) == 96, "DMedium stride");

// Phase functions beyond isotropic / HG (src/phase/tabphase.cpp, rayleigh.cpp, blendphase.cpp): DScene::phases, read by the EXT instances only.
// A tabulated entry is ContinuousDistribution's state (include/mitsuba/core/distr_1d.h:599-609) over DScene::phase_pool:
//   rec_off: n - 1 interval records of 4 floats, 16-byte aligned: (values[i], values[i + 1], i ? cdf[i - 1] : 0, cdf[i]), so that the three
//            gathers of eval_pdf / sample (y0, y1, c0) are one vector load from one aligned record;
//   cdf_off: the plain cdf, n - 1 floats, which the binary search walks (one dword per trip).
struct DPhase {
    int32_t type; float g, weight; int32_t child0, child1;      // LRT_PHASE_*; hg; blend (weight clipped to [0, 1], children never blends)
    uint32_t n;                                                 // tabulated: number of values
    float interval_size, inv_interval_size, integral, normalization;
    uint32_t valid_x, valid_y;                                  // first and last interval with mass
    uint32_t rec_off, cdf_off;                                  // into phase_pool (floats)
    uint32_t pad[2];
};
static_assert(sizeof(DPhase) == 64, "DPhase stride");

// bio media (liver / parenchyma / glissonCapsule): element coefficients of the 5-argument sample_interaction
// (kernels_bio.h); kept apart from DMedium so that the path / volpath kernels' medium loads stay as they are
struct DBioMedium {
    int32_t type, has_spectral_extinction;    // LRT_MEDIUM_*
    float layer_limit[4];
    float collagen[4][3], elastin[4][3];      // per layer, channel order as the plugins store them
    float blood[3], bile[3], lipid_water[3];
    float hepatocity, log10_hep;              // log10_hep = log2(hepatocity + 1) / log2(10), filled by k_bio_prepare (device arithmetic)
    float sigmat[3];                          // what get_majorant reports: sigma_t * scale, or parenchyma's constants
    float pad;
};

// heterogeneous media (src/media/heterogeneous.cpp): sigma_t = scale * grid, majorant = scale * max(grid)
struct DHetMedium {
    const float *data;                        // x fastest
    int32_t res[3]; float max_density;        // scale * grid_max (get_majorant)
    float to_local[12];                       // world -> unit cube
    float bbox_min[3], bbox_max[3];
    float scale, pad;
};

struct DEmitter {
    int32_t type, shape; float radiance[3]; float scale;
    float n[3]; float inv_area;          // area: rectangle frame normal (flip applied), 1/area
    float to_world[12];                  // area: rectangle to_world rows 0..2; point: position in to_world[3], [7], [11], intensity in radiance
};

// sphere shapes (src/shapes/sphere.cpp): read through scalar loads (a scene holds a few, every lane tests all of them)
struct DSphere {
    float center[3], radius;
    float to_world[9];                   // linear part of the shape's to_world (dp_du / dp_dv)
    float to_object[12];                 // inverse of to_world, rows 0..2 (uv)
    uint32_t shape; int32_t flip_normals;
    float pad[2];
};

// area emitters on triangle meshes (src/render/mesh.cpp:449-482,861-935): one entry per emitter (DScene::mesh_emitters, indexed like
// DScene::emitters; `mesh` is 0 for every other emitter).  pmf / cdf: the face areas and their inclusive float32 prefix sum, n_faces
// floats each at pmf_offset / cdf_offset of DScene::mesh_emitter_tab.
struct DMeshEmitter {
    uint32_t first_face, n_faces, pmf_offset, cdf_offset;
    float sum, normalization;            // cdf[n_faces - 1] and 1 / sum (DiscreteDistribution::m_sum, m_normalization)
    int32_t has_normals, flip_normals;
    int32_t mesh, pad[3];
};

// spot and directional emitters (src/emitters/spot.cpp, directional.cpp): one entry per emitter (DScene::delta_emitters, indexed like
// DScene::emitters; all zero for every other emitter).  DEmitter keeps its 88 bytes: type and radiance (intensity / irradiance) stay there.
// spot: pos = to_world's translation, to_local = the linear part of to_world^-1, the constructor's derived floats (spot.cpp:104-112).
// directional: dir = to_world * (0, 0, 1), and the scene's bounding sphere as set_scene takes it (directional.cpp:98-108).
struct DDeltaEmitter {
    float pos[3]; float cos_cutoff;
    float to_local[9];
    float cos_beam, cutoff, inv_transition, uv_factor;
    int32_t texture;                     // spot: projection texture (a checkerboard), -1: none
    float dir[3];
    float bsphere_c[3], bsphere_r;
    float pad[3];
};
static_assert(sizeof(DDeltaEmitter) == 112, "DDeltaEmitter stride");

#define LRT_MAX_HIER_LEVELS 16

struct DCamera {
    float s2c[16];             // sample_to_camera, row-major, projective
    float to_world[12];        // rows 0..2
    float near_clip, far_clip;
    int32_t medium, pad;
    float ppo_x, ppo_y;        // film size * principal_point_offset / crop size (perspective.cpp:214-215)
};

struct DFilm {
    int32_t width, height;               // crop size
    int32_t crop_offset_x, crop_offset_y;
    float scale_x, scale_y, offset_x, offset_y;   // render_sample(): adjusted = fmadd(pos, scale, offset)
    int32_t channels, has_alpha, rfilter, fcount; // fcount = 2*ceil(radius-.5)+1
    float rf_radius, rf_inv_radius; int32_t fn, pad;
    float rf_coeff[10];
    int32_t pad2[2];
};

struct DEnv {
    int32_t type;              // -1: none, LRT_EMITTER_ENVMAP, LRT_EMITTER_CONSTANT
    int32_t emitter;           // emitter index
    uint32_t w, h;             // (w+1) x h storage
    float scale;
    float bsphere_c[3]; float bsphere_r;
    float to_world[9];         // rotation part rows
    float to_local[9];
    float patch_size[2], inv_patch_size[2];
    uint32_t max_patch[2];
    int32_t n_levels;
    uint32_t level_offset[LRT_MAX_HIER_LEVELS];   // into env_hier (floats)
    uint32_t level_width[LRT_MAX_HIER_LEVELS];
    float radiance[3];         // constant emitter
};

// Conservative distance field over the triangle soup (see dist_grid_lower_bound() in dshade.h): value = distance from
// the cell centre to the nearest triangle, rounded down.  Lets short in-medium segments prove "no surface within reach"
// without touching the BVH.  The answer of a ray query never depends on it.
struct DDistGrid {
    const uint16_t *d;         // binary16, rounded DOWN (half the bytes of f32: the 192^3 field is 14 MB and caches better)
    float lo[3]; float cell, inv_cell;
    int32_t n[3]; int32_t enabled;
};

struct DScene {
    // acceleration structure
    const float4 *nodes;       // 4 x float4 per BVH2 node (see bvh.h)
    const float4 *tris;        // 3 x float4 per triangle slot: p0 | e1 | e2, prim id in .w of the first
    // geometry attributes
    const float *positions;
    const float4 *vattr;       // per vertex: (n.x, n.y, n.z, 0), (u, v, 0, 0): one 16-byte and one 8-byte load instead of five dword loads
    const uint32_t *faces, *face_shape;
    const DShape *shapes; const DBsdf *bsdfs; const DTexture *textures; const DMedium *media; const DBioMedium *bio; const DHetMedium *het; const DEmitter *emitters;
    const float *tex_data;
    const float4 *env_data;    // (w+1) x h RGBx
    const float *env_hier;
    uint32_t n_faces, n_emitters;
    int32_t root_is_leaf, has_null_bsdf;
    int32_t nee_fast_reject;         // see volpath_iteration(): in-medium NEE can be rejected before sampling the emitter
    int32_t one_shape;               // the scene has a single shape: shape / BSDF table reads are wave-uniform (tab() in dshade.h)
    uint32_t root_leaf_first, root_leaf_count;
    DCamera cam; DFilm film; DEnv env;
    DDistGrid grid;
    const DSphere *spheres;          // sphere k is primitive n_faces + k
    uint32_t n_spheres, pad_sph;
    const DMeshEmitter *mesh_emitters;   // n_emitters entries (the EXT instances only read them)
    const float *mesh_emitter_tab;       // every mesh emitter's pmf and cdf
    const uint2 *cone_tab;               // per face and side (2 * face + side): the free lengths of LRT_CONE_BINS direction cones as binary16, rounded down (scene_prep.cpp: build_cone_table); null: none
    int32_t cone_enabled, primary_enabled;   // the closed-records volpath kernels only read the two tables (primary_tab: at the end of the record)
    const DPhase *phases;                // tabulated / Rayleigh / blended phase functions and a blend's children (DMedium::phase_ext; the EXT instances only read them)
    const float *phase_pool;             // every tabulated entry's interval records and cdf
    const DDeltaEmitter *delta_emitters; // n_emitters entries: spot and directional emitters (the EXT instances only read them); null: the scene has neither
    const DBsdfExt *bsdf_ext;            // one row per BSDF: conductor / plastic / twosided (the EXT instances only read them); null: the scene has none of them
    // per pixel of the crop window (y * film.width + x): the work item at which trace_lds may start a camera ray's closest-hit traversal, 0xffff: no
    // triangle can be hit (scene_prep.cpp: build_primary_entry); null: none.  Last, so that every other field keeps its offset.
    const uint16_t *primary_tab;
};

// Direction bins of DScene::cone_tab: bin k holds the directions whose cosine to the side's geometric normal is at least LRT_CONE_COSk
#define LRT_CONE_BINS 4
#define LRT_CONE_COS0 0.95f
#define LRT_CONE_COS1 0.85f
#define LRT_CONE_COS2 0.70f
#define LRT_CONE_COS3 0.50f

// The scene record lives in device memory and is read through the CONSTANT address space: every `sc.field` is a scalar
// load (s_load_dword*) issued where the value is used, instead of ~190 kernarg SGPRs that stay live through the whole
// persistent kernel and are spilled to VGPR lanes (v_writelane / v_readlane: VALU work) - round-1 k_render: 347 SGPR spills.
#define LRT_CONST __attribute__((address_space(4)))
typedef const LRT_CONST DScene &SceneRef;
typedef const LRT_CONST DFilm &FilmRef;
typedef const LRT_CONST DEnv &EnvRef;
typedef const LRT_CONST DDistGrid &GridRef;
typedef const LRT_CONST DScene *ScenePtr;      // kernel argument (a plain device pointer on the host side)

struct DRenderParams {
    int32_t integrator, max_depth, rr_depth, hide_emitters;
    uint32_t spp, log2_spp;    // log2_spp = 0xffffffff when spp is not a power of two
    uint32_t seed_value;       // sampler base seed + render seed (independent sampler)
    uint32_t base_seed, seed;  // the two terms (the ld sampler keys its per-pixel scramble on them separately)
    uint32_t ld_count, pad1;   // 0: independent sampler; else the ld sampler's sample count (= spp)
    uint32_t tile_rank, tile_count;
    int32_t grad_medium;       // PRB adjoint: medium whose parameters are differentiated, -1: all media into one set
    uint32_t tiles_x, tiles_y, profile;   // profile: per-region tile timing into DCounters (developer aid, LRT_DEBUG_LAUNCH)
    uint32_t pad2;             // (keeps n_lanes at byte 72)
    uint64_t n_lanes;          // lanes this launch renders
    const uint32_t *pixel_slot; // tile-sharded renders: pixel -> index in the rank's pixel list (rank-local lane index), else null
    // multi-pass renders (integrator.cpp:176-184,275-293,343-353): spp above is the samples of ONE pass
    uint32_t pass_index, spp_total;
    const unsigned long long *pass_in;   // independent sampler: every lane's PCG32 state at the start of this pass (pass > 0)
    unsigned long long *pass_out;        // ... and where finished paths leave it for the next pass (null: last / only pass)
};

// Path-state streams (SoA, one entry per path and stream)
struct DPathStreams {
    float4 *o_maxt;            // ray origin, maxt
    float4 *d_eta;             // ray direction, eta
    float4 *tp_pdf;            // throughput rgb, last_scatter_direction_pdf
    float4 *res_flags;         // result rgb, packed flags (bits)
    float4 *lp_lane;           // last scatter position, lane id (bits)
    uint2  *rng;               // PCG32 state; the compact forms reinterpret it as uint4: state | lane | sampler word (the workspace allocates 16 bytes per entry)
    float2 *tdepth;            // biovolpath / biovolpath06 only: the loop state `tissueDepth` (sign bit: the cached competition was won by the hepatocytes), and the
                               // free-flight distance the look-ahead already drew for the next trip (NaN: none)
    float4 *hit;               // volpath with heterogeneous media / volpathmis: the surface interaction a null collision keeps (t, u, v, prim)
    float4 *w1, *w2, *w3, *w4; // volpathmis only: with tp_pdf, the 18 floats of p_over_f and p_over_f_nee
};
// (which layout uses which stream, and the bytes per record: record_layout.h)

#define LRT_INTEGRATOR_VOLPATHMIS_PLAIN 102   // kernel selector: volpathmis with use_spectral_mis = false
#define LRT_INTEGRATOR_VOLPATH_HET 101   // kernel selector (not an API value): volpath on a scene with heterogeneous media
#define LRT_INTEGRATOR_VOLPATH_CLOSED 103   // kernel selector: volpath with 64-byte records, for scenes where only a path's last trip adds radiance (device.hip, closed_records)

// flag word layout
#define PF_DEPTH_MASK   0x0000ffffu
#define PF_MEDIUM_SHIFT 16             // (medium index + 1), 8 bits
#define PF_MEDIUM_MASK  0x00ff0000u
#define PF_CHANNEL_SHIFT 24            // 2 bits
#define PF_SPECULAR     (1u << 26)     // volpath specular_chain / path prev_bsdf_delta
#define PF_VALID        (1u << 27)
#define PF_NOHIT        (1u << 28)     // look-ahead proved that the next free-flight segment reaches no surface
#define PF_BIO_SCATTERED (1u << 29)    // biovolpath06: scattered_chain
#define PF_LONG_QUERY   (1u << 29)     // biovolpath: the queued record's ray query is unbounded (the competition's distance lies beyond the previous query's hit): queue region L
#define PF_HAVE_SI      (1u << 29)     // volpath, heterogeneous media: needs_intersection == false, the record's hit stream holds `si`
#define PF_LAST_NULL    (1u << 30)     // volpathmis: last_event_was_null
#define PF_BIO_EMIT     (1u << 30)     // biovolpath06: type & 0x0001 (EmittedRadiance)
#define PF_BIO_FULL     (1u << 31)     // biovolpath06: type & 0x0004 and type & 0x0008 (they only appear together)

struct DCounters {             // device-resident queue / statistics words
    uint32_t pad[4];
    unsigned long long n_shadow;   // NEE ray queries actually needed
    unsigned long long n_iter;     // loop trips (render kernel)
    unsigned long long next_lane;  // global camera-lane ticket (render kernel)
    unsigned long long n_records;  // path records loaded from the queues
    unsigned long long prof_cycles[4], prof_tiles[4];   // per tile kind (A, C, B, fresh): wall_clock64 ticks and tiles (LRT_DEBUG_LAUNCH)
    unsigned long long prof_wg[6];   // LRT_DEBUG_LAUNCH: workgroup timeline, 100 MHz ticks: sum of start, sum of (loop start - start), sum of end, max end, min start + 2^62 trick see kernels.h, sum of barrier waits of thread 0
    unsigned long long n_closed_guard;   // 64-byte-record kernels: trips that broke the layout's premise (radiance before the last trip, an emitter hit that needs MIS)
    unsigned long long n_proven;   // path records loaded from region A: their segment was proven free of surfaces (the 64-byte-record volpath kernels only)
    unsigned long long n_primary_entry;   // fresh camera lanes whose first ray query did not start at the root, "none" included (DScene::primary_tab; the 64-byte-record volpath kernels only)
};

// LDS image of the scene for the persistent traversal kernel: [nodes | verts (float4) | tris (4 x u16)] copied verbatim
// from `blob`, followed by the per-thread traversal stacks.
struct DLdsInfo {
    const uint4 *blob;
    uint32_t blob_bytes, nodes_off, verts_off, tris_off, stack_off, total_bytes;
};

// Every argument of one launch of k_render / k_render_prb / k_splat_lanes, read through the constant address space like the
// scene record (the host fills one slot of a small ring per launch, device.hip).
struct DLaunch {
    DRenderParams rp; DLdsInfo li; DPathStreams q0, q1;
    float4 *dl0, *dl1;                    // PRB: delta_L streams
    uint32_t P, pad; DCounters *cnt; const uint32_t *pixel_list; uint64_t lane_begin, n;
    float4 *L_buf; const float *grad_image; const float *wfilm; double *grads;
    float *film; float *sample_out; uint64_t sample_base;
    float *dgrid;                         // k_render_prb_grid: gradient w.r.t. the sigma_t grid of medium rp.grad_medium (x fastest, zeroed by the host)
};
typedef const LRT_CONST DRenderParams &RpRef;
typedef const LRT_CONST DLaunch *LaunchPtr;

} // namespace lrt
