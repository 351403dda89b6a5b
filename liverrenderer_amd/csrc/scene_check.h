// Scene checks: is an lrt_scene_desc well formed, and which of its objects take it off the base kernels?  One function per object kind and
// one feature table, shared by lrt_scene_from_desc, the XML loader, the scene preparation and lrt_param_set.  Host only: no HIP call, no DeviceScene.
// A new object kind gets its check in the function of its kind and, if it needs the EXT kernel instances, a flag in SceneFeatures: nothing else
// (DESIGN.md section 22).
#pragma once
#include "host_scene.h"

namespace lrt {

// ---- per-object checks.  Each throws std::runtime_error with the bare text; validate_scene_desc decides about the prefix.
// They read d.textures[i] / d.bsdfs[i] / ... after the caller has checked i, and guard every index they follow from there.
void check_texture(const lrt_scene_desc &d, uint32_t i);
void check_bsdf(const lrt_scene_desc &d, uint32_t i);                 // the type, and all of a diffuse, bumpmap, dielectric or roughdielectric
// The rest of BSDF i when it is an LRT_BSDF_CONDUCTOR, _PLASTIC or _TWOSIDED: its texture and child indices and what the loader refuses.  The plugin's
// own text where it has one, `unsupported: ...` for what is not built.  The preparation calls it again (a plastic with int_ior = 0 passes the loader).
void check_smooth_bsdf(const lrt_scene_desc &d, uint32_t i);
void check_medium(const lrt_scene_desc &d, uint32_t i);
// Every index, count and value of the phase table and of the media's indices into it, texts as "phase table: ..."; `unsupported: ...` for a
// blend as a blend's child.  The preparation calls it again before it builds the device table.
void check_phase_table(const lrt_scene_desc &d);
void check_shape(const lrt_scene_desc &d, uint32_t i);
// Emitter i.  A spot or directional one goes to check_delta_emitter.  (An area emitter on a mesh: validate_scene_desc also builds its sampling
// table once, mesh_emitter_table of host_scene.h, whose texts pass bare.)
void check_emitter(const lrt_scene_desc &d, uint32_t i);
// Emitter i, an LRT_EMITTER_SPOT or _DIRECTIONAL: a finite, invertible to_world; a spot's angles (0 < beam_width <= cutoff_angle <= 180,
// cutoff_angle < 90 with a texture) and its texture's index and type.  The loader and the preparation call it too.
void check_delta_emitter(const lrt_scene_desc &d, uint32_t i);
void check_sensor_film(const lrt_scene_desc &d);                      // the sensor's medium, clipping planes and fov, the crop window and filter, then check_camera_footprint
// What the loader shares of the sensor and the film: the plugin's text for a camera-to-world transform with scale factors
// (src/sensors/perspective.cpp:144-145; Transform::has_scale, include/mitsuba/core/transform.h:242-254: |M M^T - I| > 1e-3 in an entry of the
// linear part, so a mirrored orthonormal frame passes), and a wide-filter film whose size plus footprint leaves what FilmFootprint::key()
// (film.h) packs into 16 bits per axis.
void check_camera_footprint(const lrt_scene_desc &d);
void check_integrator_sampler(const lrt_scene_desc &d);

// ---- what the first render refuses and lrt_scene_from_desc does not (DESIGN.md section 22 lists these gaps).  Only the preparation calls them;
// validate_scene_desc calling them would change what lrt_scene_from_desc accepts.
void check_sphere_radius(float radius);                               // |to_world * (1, 0, 0)| of a sphere shape: positive and finite
void check_medium_grid(const lrt_medium_desc &M);                     // a heterogeneous medium: grid data, a resolution, and a maximum above 0 (it is the majorant)
void check_media_count(const lrt_scene_desc &d);                      // the kernels' medium masks hold 64

// Every index, range and pointer of a caller-built description, in the order textures, BSDFs, media, phase table, shapes, emitters, sensor and
// film, integrator and sampler.  Texts carry the prefix "lrt_scene_from_desc: " except those that start with "unsupported", and those of
// check_smooth_bsdf and of the mesh emitter's sampling table, which pass bare.  tests/test_scene_check.py holds every text, and checks that
// what the XML loader builds passes.
void validate_scene_desc(const lrt_scene_desc &d);

// The asymmetry parameter of a Henyey-Greenstein phase function (src/phase/hg.cpp:45-46): the loader, the validator and lrt_param_set ask here.
constexpr const char *kHgRangeText = "The asymmetry parameter must lie in the interval (-1, 1)!";
inline bool hg_g_valid(float g) { return g > -1.f && g < 1.f; }
// A texture that has to be a colour or a checkerboard: bitmaps are held as one luminance float per texel.  `what`: "diffuse reflectance", ...
void refuse_bitmap(const lrt_texture_desc &T, const std::string &what);

// Texts that two stages state, each about what it has in hand: the XML loader about a file's properties, the checks about the record (the plugins'
// own wording where they have one).  The conditions differ (an index of refraction against a relative one, a tag against a type), the text is one.
namespace text {
constexpr const char *ior_positive = "The interior and exterior indices of refraction must be positive!";
constexpr const char *conductor_no_index = "conductor with eta = k = 0 in a channel (no index of refraction: its Fresnel term is 0 / 0 at normal incidence; the plugin's default is eta = 0, k = 1)";
constexpr const char *twosided_no_child = "A nested one-sided material is required!";
constexpr const char *twosided_transmission = "Only materials without a transmission component can be nested!";
constexpr const char *no_probability_mass = "ContinuousDistribution: no probability mass found!";
constexpr const char *blend_in_blend = "unsupported: a blendphase as the child of a blendphase (one level is built)";
constexpr const char *emitter_on_sphere = "unsupported: an area emitter on a sphere (area emitters are supported on rectangles and triangle meshes)";
constexpr const char *spot_texture_uniform = "The parameter 'texture' must be spatially varying (e.g. bitmap type)!";
constexpr const char *spot_texture_bitmap = "unsupported: a bitmap texture as the spot emitter's 'texture' (bitmaps are held as one luminance float per texel, for bump maps only; a checkerboard is supported)";
constexpr const char *one_environment = "Only one environment emitter can be specified per scene.";
constexpr const char *crop_window = "Invalid crop window specification!";
constexpr const char *fov_range = "The horizontal field of view must be in the range [0, 180]!";
inline std::string twosided_child(const std::string &kind) { return "unsupported: a " + kind + " nested in a twosided BSDF (its children are diffuse, conductor or plastic)"; }
}

// One flag per reason a scene leaves the base kernels (triangles, rectangle / infinite emitters, diffuse / dielectric / null, isotropic / hg).
// Any of them selects the EXT kernel instances; prbvolpath has no adjoint for any of them and says which group it met.
struct SceneFeatures {
    bool sphere = false;             // a sphere shape
    bool point_emitter = false;
    bool delta_emitter = false;      // a spot or directional emitter
    bool mesh_emitter = false;       // an area emitter on a triangle mesh
    bool rough_bsdf = false;         // a roughdielectric on a shape, alone or under a bumpmap (an unreferenced one changes nothing: the scene keeps its kernels)
    bool smooth_bsdf = false;        // a conductor, plastic or twosided on a shape, alone or under a bumpmap
    bool phase_entry = false;        // a tabulated / Rayleigh / blended phase function on a medium that a shape or the sensor references
    bool any() const { return sphere || point_emitter || delta_emitter || mesh_emitter || rough_bsdf || smooth_bsdf || phase_entry; }
};
// Reads every index guarded: a description that has not been validated gives flags, never a fault (an index out of range counts as absent).
SceneFeatures scene_features(const lrt_scene_desc &d);

} // namespace lrt
