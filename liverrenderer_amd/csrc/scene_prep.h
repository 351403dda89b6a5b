// Host half of the scene upload: everything device.hip copies to the device, computed from an lrt_scene_desc with plain
// host arithmetic.  No HIP runtime call and no DeviceScene here, so the unit builds and runs without a GPU
// (tests/host/scene_prep_main.cpp); device.hip uploads the result and patches the device pointers in.
#pragma once
#include "device_types.h"
#include "bvh.h"
#include "host_scene.h"
#include <utility>

namespace lrt {

// The environment switches read while the device image is built, and what the upload side knows about the device.
struct PrepOptions {
    int bvh_leaf = 0;              // LRT_BVH_LEAF=n forces a leaf size (>= 1); 0: the search below
    bool no_lds_bvh = false;       // LRT_NO_LDS_BVH
    bool no_dist_grid = false;     // LRT_NO_DIST_GRID
    int dist_grid_res = 0;         // LRT_DIST_GRID_RES clamped to 8 .. 256; 0: by the face count
    bool no_nee_reject = false;    // LRT_NO_NEE_REJECT
    bool no_cone_proof = false;    // LRT_NO_CONE_PROOF: no per-face cone table (build_cone_table)
    bool no_primary_entry = false; // LRT_NO_PRIMARY_ENTRY: no per-pixel primary entry (build_primary_entry)
    size_t lds_limit = 0;         // LDS bytes a workgroup may ask for (device.hip: the opt-in maximum minus the kernels' static words)
    int n_cus = 256;               // compute units of the device: the upload side sets it and takes it back for the launch geometry; the preparation does not use it
    static PrepOptions from_env(); // reads the seven switches; lds_limit and n_cus stay at their defaults
};

// BSDF leaf flags as DBsdf::flags stores them (dshade.h names the same values F_DELTA, F_SMOOTH, F_NULL; device.hip asserts that they agree)
enum { PREP_F_DELTA = 1, PREP_F_SMOOTH = 2, PREP_F_NULL = 4 };

struct PreparedScene {
    std::vector<DSphere> spheres;
    HostBVH bvh;                                       // nodes, triangle slots, root leaf
    std::vector<unsigned char> lds_blob; DLdsInfo lds{};   // the LDS image (use_lds) and its offsets; lds.blob is the upload side's
    std::vector<float> vattr;                          // 8 floats per vertex
    std::vector<DShape> shapes;
    std::vector<DTexture> textures; std::vector<float> tex_data;
    std::vector<DBsdf> bsdfs;
    std::vector<DBsdfExt> bsdf_ext;                    // DScene::bsdf_ext, one row per BSDF; empty: the description has no conductor, plastic or twosided
    std::vector<DEmitter> emitters;
    std::vector<DMeshEmitter> mesh_emitters; std::vector<float> mesh_emitter_tab;
    std::vector<DDeltaEmitter> delta_emitters;         // DScene::delta_emitters, one entry per emitter; empty: the scene has no spot or directional emitter
    std::vector<float> env_data, env_hier;             // (w+1) x h RGBx texels, sampling hierarchy
    // The scalar part of the scene record: counts, root leaf, one_shape, has_null_bsdf, nee_fast_reject, env (with the bounding sphere),
    // cam, film and the distance field's geometry (grid.enabled set, grid.d null: the upload side builds the field).  Every pointer is null.
    DScene sc{};
    float grid_abs_margin = 0.f;                       // k_build_dist_grid's margin
    std::vector<DPhase> phases; std::vector<float> phase_pool;   // DScene::phases / phase_pool (prepare_phases); empty: the description has no phase table
    std::vector<uint16_t> cone_tab;                    // build_cone_table's rows, 2 * LRT_CONE_BINS binary16 per face; empty: no table (sc.cone_enabled = 0)
    std::vector<uint16_t> primary_tab;                 // build_primary_entry's items, one per pixel of the crop window; empty: no table (sc.primary_enabled = 0)
    bool env_interior_positive = false;               // envmap: rows 1..h-2 of the sampling density strictly positive
    bool ext = false, has_area_emitter = false, has_het = false, has_non_bio = false, prb_null = false, use_lds = false;   // DeviceScene's flags of the same names
    bool smooth_bsdf = false;                          // a conductor / plastic / twosided sits on a shape (it sets `ext` too; prbvolpath names it in its refusal)
    int bvh_leaf = 4;
};
// The two halves of prepare_scene, for a caller that has work to start in between (device.hip launches k_build_dist_grid after the first, so that
// the kernel runs while the host prepares the rest, as it always did).  prepare_geometry: spheres, `ext`, the BVH with its leaf-size search,
// the LDS image, the root leaf and counts, the distance field's geometry.  prepare_shading: everything else; it reads P.spheres for the bounds.
// Precondition of all three: the description has passed the XML loader or validate_scene_desc (scene_check.h).  They follow its indices (a bumpmap's
// child, texture and shape references) without looking at them again.
void prepare_geometry(const lrt_scene_desc &d, const PrepOptions &opt, PreparedScene &P);
void prepare_shading(const lrt_scene_desc &d, const PrepOptions &opt, PreparedScene &P);
PreparedScene prepare_scene(const lrt_scene_desc &d, const PrepOptions &opt);

// DScene::cam and DScene::film of a description (prepare_shading's; build_primary_entry and its host test read the same constants)
void build_camera(const lrt_scene_desc &d, DCamera &cam, DFilm &film);

// Per-face cone table: out[(2 * f + s) * LRT_CONE_BINS + k] = R as binary16, rounded down, with this property: a segment whose origin lies on face f,
// displaced to side s as spawn_ray displaces a float32 hit point (s = 0: along the geometric normal the device computes, flip_normals applied; s = 1:
// against it), whose direction makes a cosine of at least LRT_CONE_COSk with that side's normal and whose length is at most R meets no triangle of
// the scene.  0: nothing is claimed.  (scene_prep.cpp has the construction.)
void build_cone_table(const lrt_scene_desc &d, std::vector<uint16_t> &out);
// a table entry as the device reads it
float cone_table_value(uint16_t h);

// Per-pixel primary entry: out[y * crop_width + x] (crop-local pixel, the index lane_to_pixel forms) = the 16-bit work item of trace_lds at which the
// closest-hit traversal of ANY camera ray through that pixel may start without changing its result: an inner node index (0, the root: nothing is
// claimed), 0x8000 | first slot of a leaf, or LRT_PRIMARY_NONE: no triangle can be hit.  Built from the device's own float32 camera and film constants
// (build_camera) widened to double.  Empty: no table (a camera the construction does not cover, non-finite vertices, a root leaf).
// `tune`: the construction's margins; only the host test changes them, to seed a mistake.  (scene_prep.cpp has the construction.)
#define LRT_PRIMARY_NONE 0xffffu
struct PrimaryEntryTune { double delta = 1.0 / 16.0, depth_margin = 1e-4; };
void build_primary_entry(const lrt_scene_desc &d, const HostBVH &bvh, std::vector<uint16_t> &out, const PrimaryEntryTune &tune = PrimaryEntryTune());
// every item names a node of the BVH, the first slot of one of its leaves, or LRT_PRIMARY_NONE (the upload refuses a table that fails this)
bool primary_entry_valid(const HostBVH &bvh, const std::vector<uint16_t> &tab);

// bytes of the LDS image of a BVH: nodes, float4 vertices, 8-byte triangle slots, 16-bit traversal stacks of 1024 threads
size_t lds_image_bytes(const HostBVH &b, uint32_t n_vertices);
// the image's 16-bit indices hold the scene (faces, vertices, nodes, slots), it fits `opt.lds_limit`, and LRT_NO_LDS_BVH is not set
bool lds_image_fits(const lrt_scene_desc &d, const HostBVH &b, const PrepOptions &opt);

// a medium's extinction as the device sees it: property * scale (homogeneous.cpp:121-126 eval_sigmat; liver.cpp:204-209)
inline float medium_sigma_t(const lrt_medium_desc &M, int k) { return M.sigma_t[k] * M.scale; }
// The media tables (max(n_media, 1) entries each).  DBioMedium::log10_hep and DMedium::w_spec / w_plain are the device's to fill
// (k_bio_prepare, k_medium_prepare); DHetMedium::data is the upload side's.  bsphere_r: DEnv::bsphere_r of the scene.
void prepare_media(const lrt_scene_desc &d, float bsphere_r, std::vector<DMedium> &media, std::vector<DBioMedium> &bio, std::vector<DHetMedium> &het);

// ContinuousDistribution(range = (-1, 1), values, n) as the reference's scalar constructor builds it (include/mitsuba/core/distr_1d.h:548-597):
// the running integral in double, cdf[i] = (float) integral, `valid` = the first and last interval with mass.  Throws the reference's texts
// ("needs at least two entries", "entries must be non-negative", "no probability mass found").
struct PhaseTable { std::vector<float> cdf; float interval_size = 0.f, inv_interval_size = 0.f, integral = 0.f, normalization = 0.f; uint32_t valid_x = 0, valid_y = 0; };
void phase_table(const float *values, size_t n, PhaseTable &out);
// does medium m scatter by an entry of the table?  (n_phases = 0: the indices are not read)
inline bool medium_has_phase_entry(const lrt_scene_desc &d, uint32_t m) { return d.n_phases > 0 && d.media[m].phase_index >= 0; }
// DScene::phases and phase_pool: an entry per description entry, the tabulated ones with their interval records and cdf (after check_phase_table)
void prepare_phases(const lrt_scene_desc &d, std::vector<DPhase> &phases, std::vector<float> &pool);

// SmoothPlastic::parameters_changed (src/bsdfs/plastic.cpp:192-207) in float32, as the plugin's scalar constructor computes it
struct PlasticConstants { float inv_eta_2, fdr_int, fdr_ext, specular_sampling_weight; };
PlasticConstants plastic_constants(float eta, float d_mean, float s_mean);
// Texture::mean() of an RGB value or a checkerboard (src/spectra/srgb.cpp:117-122, src/textures/checkerboard.cpp:112-114)
float texture_mean(const lrt_texture_desc &T);

// spp: samples of ONE pass; spp_total = n_passes * spp (integrator.cpp:176-184,275-293)
struct ResolvedOpts { int integrator, max_depth, rr_depth, hide_emitters; uint32_t spp, seed, tile_rank, tile_count; uint32_t spp_total = 0, n_passes = 1, pass = 0; };
ResolvedOpts resolve(const lrt_scene_desc &d, const lrt_render_opts *o);

// 32x32 pixel tiles in row-major tile order, tile k -> rank k % count: the rank's pixels, and pixel -> index in that list
struct TilePixels { std::vector<uint32_t> list, slot; };
TilePixels tile_pixel_list(const DFilm &film, uint32_t rank, uint32_t count);
// the rank's tiles dilated by `halo` pixels, as a pixel list (row-major order, every pixel once)
std::vector<uint32_t> halo_pixel_list(const DFilm &film, uint32_t rank, uint32_t count, uint32_t halo);

// 64-byte path records: does the scene prove that only a path's last trip adds radiance?  (scene_prep.cpp has the proof.)
bool closed_records(const lrt_scene_desc &d, int sensor_medium);

} // namespace lrt
