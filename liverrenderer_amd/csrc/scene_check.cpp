// Scene checks (scene_check.h): one function per object kind, the validator of lrt_scene_from_desc over them, and the feature table.
// No translation unit of its own: scene_prep.cpp includes this file at its end (the reason is given there), so it is named in no source list.
#include "scene_check.h"
#include "scene_prep.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace lrt {

[[noreturn]] static void bad(const std::string &m) { throw std::runtime_error(m); }
static bool smooth_type(int t) { return t == LRT_BSDF_CONDUCTOR || t == LRT_BSDF_PLASTIC || t == LRT_BSDF_TWOSIDED; }

void refuse_bitmap(const lrt_texture_desc &T, const std::string &what) {
    if (T.type == LRT_TEX_BITMAP) bad("unsupported: a bitmap texture as " + what + " (bitmaps are supported as bump-map heights only)");
}

void check_texture(const lrt_scene_desc &d, uint32_t i) {
    const lrt_texture_desc &T = d.textures[i];
    if (T.type < LRT_TEX_RGB || T.type > LRT_TEX_BITMAP) bad("invalid texture type");
    if (T.type == LRT_TEX_BITMAP && (!T.data || T.width < 1 || T.height < 1 || (T.channels != 1 && T.channels != 3))) bad("bitmap texture without texels or with invalid dimensions");
}

void check_bsdf(const lrt_scene_desc &d, uint32_t i) {
    const lrt_bsdf_desc &B = d.bsdfs[i];
    if (B.type < LRT_BSDF_DIFFUSE || B.type > LRT_BSDF_TWOSIDED) bad("invalid bsdf type");
    if (B.type == LRT_BSDF_DIFFUSE) {
        if (B.reflectance < 0 || (uint32_t) B.reflectance >= d.n_textures) bad("diffuse bsdf references an invalid texture");
        refuse_bitmap(d.textures[B.reflectance], "diffuse reflectance");
    }
    if (B.type == LRT_BSDF_BUMPMAP) {
        if (B.nested < 0 || (uint32_t) B.nested >= d.n_bsdfs || d.bsdfs[B.nested].type == LRT_BSDF_BUMPMAP) bad("bumpmap references an invalid nested bsdf");
        if (d.bsdfs[B.nested].type == LRT_BSDF_TWOSIDED) bad("unsupported: a twosided BSDF nested in a bumpmap");
        if (B.texture < 0 || (uint32_t) B.texture >= d.n_textures) bad("bumpmap references an invalid texture");
    }
    if (B.type == LRT_BSDF_DIELECTRIC && !(B.eta > 0.f)) bad("dielectric with a non-positive relative index of refraction");
    if (B.type == LRT_BSDF_ROUGHDIELECTRIC) {
        if (!(B.eta > 0.f) || B.eta == 1.f) bad("roughdielectric: the interior and exterior indices of refraction must be positive and differ");
        if (!(B.alpha_u >= 0.f) || !(B.alpha_v >= 0.f) || !std::isfinite(B.alpha_u) || !std::isfinite(B.alpha_v)) bad("roughdielectric with an invalid roughness");
        if (B.distribution != 0 && B.distribution != 1) bad("roughdielectric with an invalid distribution (0: beckmann, 1: ggx)");
        for (int32_t t : { B.specular_reflectance, B.specular_transmittance }) {
            if (t < -1 || t >= (int32_t) d.n_textures) bad("roughdielectric references an invalid texture");
            if (t >= 0 && d.textures[t].type == LRT_TEX_BITMAP) bad("unsupported: a bitmap texture as roughdielectric specular_reflectance / specular_transmittance");
        }
    }
}

void check_smooth_bsdf(const lrt_scene_desc &d, uint32_t i) {
    const lrt_bsdf_desc &B = d.bsdfs[i];
    auto tex = [&](int32_t t, bool required, const char *what) {
        if (t < (required ? 0 : -1) || t >= (int32_t) d.n_textures) bad(std::string(what) + " references an invalid texture");
        if (t >= 0) refuse_bitmap(d.textures[t], what);
    };
    if (B.type == LRT_BSDF_CONDUCTOR) {
        tex(B.specular_reflectance, true, "conductor specular_reflectance");
        for (int k = 0; k < 3; ++k) if (!std::isfinite(B.eta_rgb[k]) || !std::isfinite(B.k_rgb[k])) bad("conductor with an index of refraction that is not finite");
        // eta = k = 0 is no index of refraction: fresnel_conductor is 0 / 0 at normal incidence (term_3 = term_4 = 0, fresnel.h:111-114).  A zero-filled
        // tail of the description lands here, so a conductor has to state its index (the plugin's default is 0 + 1i).
        for (int k = 0; k < 3; ++k) if (B.eta_rgb[k] == 0.f && B.k_rgb[k] == 0.f) bad(text::conductor_no_index);
    } else if (B.type == LRT_BSDF_PLASTIC) {
        if (!(B.eta > 0.f) || !std::isfinite(B.eta)) bad(text::ior_positive);
        tex(B.diffuse_reflectance, true, "plastic diffuse_reflectance"); tex(B.specular_reflectance, false, "plastic specular_reflectance");
    } else if (B.type == LRT_BSDF_TWOSIDED) {
        if (B.nested < 0) bad(text::twosided_no_child);
        for (int32_t c : { B.nested, B.nested_back < 0 ? B.nested : B.nested_back }) {      // (nested_back = -1: one child)
            if (c < 0 || (uint32_t) c >= d.n_bsdfs) bad("twosided references an invalid nested bsdf");
            const int t = d.bsdfs[c].type;
            if (t == LRT_BSDF_DIELECTRIC || t == LRT_BSDF_ROUGHDIELECTRIC || t == LRT_BSDF_NULL) bad(text::twosided_transmission);
            if (t == LRT_BSDF_BUMPMAP || t == LRT_BSDF_TWOSIDED) bad(text::twosided_child(t == LRT_BSDF_BUMPMAP ? "bumpmap" : "twosided"));
        }
    }
}

void check_medium(const lrt_scene_desc &d, uint32_t i) {
    const lrt_medium_desc &M = d.media[i];
    if (M.type < LRT_MEDIUM_HOMOGENEOUS || M.type > LRT_MEDIUM_HETEROGENEOUS) bad("invalid medium type");
    if (M.type == LRT_MEDIUM_HETEROGENEOUS) {                      // the volume's frame arrives ready-made (the XML loader derives it from to_world)
        if (!M.grid_data || M.grid_res[0] < 1 || M.grid_res[1] < 1 || M.grid_res[2] < 1) bad("heterogeneous medium without grid data");
        for (int k = 0; k < 12; ++k) if (!std::isfinite(M.grid_to_local[k])) bad("heterogeneous medium: grid_to_local is not finite (a singular volume to_world?)");
        for (int k = 0; k < 3; ++k) if (!(M.grid_bbox_max[k] > M.grid_bbox_min[k]) || !std::isfinite(M.grid_bbox_min[k]) || !std::isfinite(M.grid_bbox_max[k])) bad("heterogeneous medium: empty or unbounded grid bounding box");
    }
    if (M.phase != LRT_PHASE_ISOTROPIC && M.phase != LRT_PHASE_HG) bad("invalid phase function");
    if (M.phase == LRT_PHASE_HG && !hg_g_valid(M.g)) bad(kHgRangeText);
}

void check_medium_grid(const lrt_medium_desc &M) {
    if (!M.grid_data || M.grid_res[0] < 1 || M.grid_res[1] < 1 || M.grid_res[2] < 1 || !(M.grid_max > 0.f)) bad("heterogeneous medium without a valid grid");
}

void check_media_count(const lrt_scene_desc &d) { if (d.n_media > 64) bad("at most 64 media are supported"); }

void check_phase_table(const lrt_scene_desc &d) {
    auto bad = [](const std::string &m) { throw std::runtime_error("phase table: " + m); };
    if (d.n_phases && !d.phases) bad("null array");
    for (uint32_t i = 0; i < d.n_phases; ++i) {
        const lrt_phase_desc &Q = d.phases[i];
        if (Q.type < LRT_PHASE_ISOTROPIC || Q.type > LRT_PHASE_BLEND) bad("invalid phase function");
        if (Q.type == LRT_PHASE_HG && !hg_g_valid(Q.g)) bad(kHgRangeText);
        if (Q.type == LRT_PHASE_TABULATED) {
            if (Q.n_values && !Q.values) bad("tabulated phase function without values");
            for (uint32_t k = 0; k < Q.n_values; ++k) if (!std::isfinite(Q.values[k])) bad("tabulated phase function with a value that is not finite");
            PhaseTable T; phase_table(Q.values, Q.n_values, T);
            if (!(T.integral > 0.f) || !std::isfinite(T.integral)) bad(text::no_probability_mass);
        }
        if (Q.type == LRT_PHASE_BLEND) {
            if (!(Q.weight == Q.weight)) bad("blendphase with a weight that is not a number");
            for (int32_t c : { Q.child[0], Q.child[1] }) {
                if (c < 0 || (uint32_t) c >= d.n_phases) bad("blendphase references an invalid child");
                if (d.phases[c].type == LRT_PHASE_BLEND) throw std::runtime_error(text::blend_in_blend);
            }
        }
    }
    for (uint32_t m = 0; m < d.n_media && d.n_phases; ++m) {
        const int32_t ix = d.media[m].phase_index;
        if (ix < -1 || ix >= (int32_t) d.n_phases) bad("medium references an invalid entry");
        // (isotropic / hg entries are a blend's children: a medium that scatters by one of them says so in `phase` / `g`, keeps its parameter key and its kernels)
        if (ix >= 0 && d.phases[ix].type < LRT_PHASE_TABULATED) bad("medium references an isotropic / hg entry (a medium's entry is tabulated, rayleigh or blend; use the medium's `phase` / `g`)");
    }
}

void check_shape(const lrt_scene_desc &d, uint32_t i) {
    const lrt_shape_desc &s = d.shapes[i];
    if (s.bsdf < 0 || (uint32_t) s.bsdf >= d.n_bsdfs) bad("shape references an invalid bsdf");
    if (s.emitter < -1 || s.emitter >= (int) d.n_emitters || s.interior_medium < -1 || s.interior_medium >= (int) d.n_media || s.exterior_medium < -1 || s.exterior_medium >= (int) d.n_media)
        bad("shape references an invalid emitter/medium");
    if ((uint64_t) s.first_face + s.n_faces > d.n_faces) bad("shape face range exceeds the face array");
    if (s.kind < LRT_SHAPE_MESH || s.kind > LRT_SHAPE_SPHERE) bad("invalid shape kind");
    if (s.kind == LRT_SHAPE_SPHERE && s.n_faces != 0) bad("a sphere shape has no faces");
    if (s.emitter >= 0 && (d.emitters[s.emitter].type != LRT_EMITTER_AREA || d.emitters[s.emitter].shape != (int) i)) bad("shape and area emitter do not reference each other");
}

void check_sphere_radius(float radius) { if (!(radius > 0.f) || !std::isfinite(radius)) bad("sphere with a zero or invalid radius"); }

void check_emitter(const lrt_scene_desc &d, uint32_t i) {
    const lrt_emitter_desc &E = d.emitters[i];
    if (E.type < LRT_EMITTER_AREA || E.type > LRT_EMITTER_DIRECTIONAL) bad("invalid emitter type");
    if (E.type == LRT_EMITTER_SPOT || E.type == LRT_EMITTER_DIRECTIONAL) return check_delta_emitter(d, i);
    if (E.type == LRT_EMITTER_AREA) {
        if (E.shape < 0 || (uint32_t) E.shape >= d.n_shapes) bad("area emitter references an invalid shape");
        const lrt_shape_desc &s = d.shapes[E.shape];
        if (s.kind == LRT_SHAPE_SPHERE) bad(text::emitter_on_sphere);
        if (s.kind == LRT_SHAPE_RECTANGLE && s.n_faces < 1) bad("area emitter on a rectangle without faces");
    }
    if (E.type == LRT_EMITTER_ENVMAP && (!E.data || E.width < 2 || E.height < 3)) bad("environment map without data or smaller than 2x3 pixels");
}

// The plugin only asserts cutoff >= beam in debug builds (spot.cpp:111); here every value that would put an infinity or a NaN into the device table is refused by name.
void check_delta_emitter(const lrt_scene_desc &d, uint32_t i) {
    const lrt_emitter_desc &E = d.emitters[i];
    const char *who = E.type == LRT_EMITTER_SPOT ? "spot emitter" : "directional emitter";
    double m[3][3]; bool finite = true;
    for (int k = 0; k < 16; ++k) finite = finite && std::isfinite(E.to_world[k]);
    for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) m[a][b] = E.to_world[4 * a + b]; finite = finite && std::isfinite(E.radiance[a]); }
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    if (!finite || !(std::fabs(det) > 0.0) || !std::isfinite(1.0 / det)) bad(std::string(who) + ": to_world must be finite and invertible, the value finite");
    if (E.type != LRT_EMITTER_SPOT) return;
    if (!(E.beam_width > 0.f) || !(E.beam_width <= E.cutoff_angle) || !(E.cutoff_angle <= 180.f))
        bad("spot emitter: 0 < beam_width <= cutoff_angle <= 180 degrees is required (beam_width " + std::to_string(E.beam_width) + ", cutoff_angle " + std::to_string(E.cutoff_angle) + ")");
    if (E.texture < -1 || E.texture >= (int32_t) d.n_textures) bad("spot emitter references an invalid texture");
    if (E.texture < 0) return;
    if (d.textures[E.texture].type == LRT_TEX_BITMAP)
        bad(text::spot_texture_bitmap);
    if (d.textures[E.texture].type != LRT_TEX_CHECKERBOARD) bad(text::spot_texture_uniform);    // spot.cpp:98-100
    if (!(E.cutoff_angle < 90.f)) bad("spot emitter: cutoff_angle must be below 90 degrees when a texture is given (uv_factor = tan(cutoff_angle) must be positive and finite)");
}

void check_camera_footprint(const lrt_scene_desc &d) {
    const float *m = d.sensor.to_world;
    for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) {            // transform.h:242-254, float32 as the plugin's scalar transform
        float sum = 0.f;
        for (int k = 0; k < 3; ++k) sum += m[4 * i + k] * m[4 * j + k];
        if (!(std::fabs(sum - (i == j ? 1.f : 0.f)) <= 1e-3f)) bad("Scale factors in the camera-to-world transformation are not allowed!");
    }
    const lrt_film_desc &F = d.film;
    if (F.rfilter == LRT_RFILTER_BOX) return;
    // FilmFootprint::key(): origins lie in [-fn, size - fn], each packed as (coordinate + 0x4000) in 16 bits
    const float radius = F.rfilter == LRT_RFILTER_GAUSSIAN ? 4.f * F.rfilter_param : F.rfilter_param;
    if (!(radius <= 16384.f) || std::max(F.width, F.height) > 0xbfff)
        bad("film footprint out of range: a gaussian or tent filter needs a radius of at most 16384 pixels and a film of at most 49151 pixels per side (radius " +
            std::to_string(radius) + ", film " + std::to_string(F.width) + " x " + std::to_string(F.height) + ")");
}

void check_sensor_film(const lrt_scene_desc &d) {
    if (d.sensor.medium < -1 || d.sensor.medium >= (int) d.n_media) bad("sensor references an invalid medium");
    if (!(d.sensor.near_clip > 0.f) || !(d.sensor.near_clip < d.sensor.far_clip)) bad("invalid clipping planes");
    if (!(d.sensor.fov_x > 0.f && d.sensor.fov_x < 180.f)) bad(text::fov_range);
    const lrt_film_desc &F = d.film;
    if (F.width <= 0 || F.height <= 0 || F.crop_width <= 0 || F.crop_height <= 0 || F.crop_offset_x < 0 || F.crop_offset_y < 0 ||
        F.crop_offset_x + F.crop_width > F.width || F.crop_offset_y + F.crop_height > F.height) bad(text::crop_window);
    if (F.rfilter < LRT_RFILTER_BOX || F.rfilter > LRT_RFILTER_TENT || (F.rfilter != LRT_RFILTER_BOX && !(F.rfilter_param > 0.f))) bad("invalid reconstruction filter");
    check_camera_footprint(d);
}

void check_integrator_sampler(const lrt_scene_desc &d) {
    if (d.integrator.type < LRT_INTEGRATOR_PATH || d.integrator.type > LRT_INTEGRATOR_VOLPATHMIS) bad("invalid integrator type");
    if (d.integrator.max_depth < -1 || d.integrator.rr_depth <= 0) bad("invalid max_depth / rr_depth");
    if (d.sampler_type > LRT_SAMPLER_LD || d.sample_count == 0) bad("invalid sampler");
}

// The one place that decides about the prefix: `bare` texts and those that start with "unsupported" pass as they are.
template <typename F> static void checked(bool bare, F &&check) {
    try { check(); }
    catch (const std::runtime_error &e) {
        if (bare || !strncmp(e.what(), "unsupported", 11)) throw;
        throw std::runtime_error(std::string("lrt_scene_from_desc: ") + e.what());
    }
}

void validate_scene_desc(const lrt_scene_desc &d) {
    checked(false, [&] {
        if ((d.n_vertices && (!d.positions || !d.normals || !d.texcoords)) || (d.n_faces && (!d.faces || !d.face_shape))) bad("null geometry array");
        if ((d.n_shapes && !d.shapes) || (d.n_bsdfs && !d.bsdfs) || (d.n_textures && !d.textures) || (d.n_media && !d.media) || (d.n_emitters && !d.emitters)) bad("null object array");
        for (uint32_t f = 0; f < 3 * d.n_faces; ++f) if (d.faces[f] >= d.n_vertices) bad("face references an invalid vertex");
        for (uint32_t f = 0; f < d.n_faces; ++f) if (d.face_shape[f] >= d.n_shapes) bad("face references an invalid shape");
        for (uint32_t i = 0; i < d.n_textures; ++i) check_texture(d, i);
    });
    for (uint32_t i = 0; i < d.n_bsdfs; ++i) {
        checked(false, [&] { check_bsdf(d, i); });
        if (smooth_type(d.bsdfs[i].type)) checked(true, [&] { check_smooth_bsdf(d, i); });
    }
    checked(false, [&] {
        for (uint32_t i = 0; i < d.n_media; ++i) check_medium(d, i);
        check_phase_table(d);
        for (uint32_t i = 0; i < d.n_shapes; ++i) check_shape(d, i);
    });
    uint32_t n_env = 0;
    for (uint32_t i = 0; i < d.n_emitters; ++i) {
        checked(false, [&] { check_emitter(d, i); });
        const lrt_emitter_desc &E = d.emitters[i];
        if (E.type == LRT_EMITTER_AREA && d.shapes[E.shape].kind == LRT_SHAPE_MESH) {
            const lrt_shape_desc &s = d.shapes[E.shape];
            checked(true, [&] { MeshEmitterTable tab; mesh_emitter_table(d.positions, d.faces, s.first_face, s.n_faces, "shapes[" + std::to_string(E.shape) + "]", tab); });
        }
        if (E.type == LRT_EMITTER_ENVMAP || E.type == LRT_EMITTER_CONSTANT) ++n_env;
    }
    checked(false, [&] {
        if (n_env > 1) bad(text::one_environment);
        check_sensor_film(d);
        check_integrator_sampler(d);
    });
}

SceneFeatures scene_features(const lrt_scene_desc &d) {
    SceneFeatures F;
    auto phase_medium = [&](int32_t m) { return m >= 0 && (uint32_t) m < d.n_media && medium_has_phase_entry(d, (uint32_t) m); };
    F.phase_entry = phase_medium(d.sensor.medium);
    for (uint32_t i = 0; i < d.n_shapes; ++i) {
        const lrt_shape_desc &s = d.shapes[i];
        F.sphere = F.sphere || s.kind == LRT_SHAPE_SPHERE;
        F.phase_entry = F.phase_entry || phase_medium(s.interior_medium) || phase_medium(s.exterior_medium);
        if (s.bsdf < 0 || (uint32_t) s.bsdf >= d.n_bsdfs) continue;
        const lrt_bsdf_desc *B = &d.bsdfs[s.bsdf];
        if (B->type == LRT_BSDF_BUMPMAP && B->nested >= 0 && (uint32_t) B->nested < d.n_bsdfs) B = &d.bsdfs[B->nested];      // one level: bumpmaps do not nest
        F.rough_bsdf = F.rough_bsdf || B->type == LRT_BSDF_ROUGHDIELECTRIC;
        F.smooth_bsdf = F.smooth_bsdf || smooth_type(B->type);
    }
    for (uint32_t i = 0; i < d.n_emitters; ++i) {
        const lrt_emitter_desc &e = d.emitters[i];
        F.point_emitter = F.point_emitter || e.type == LRT_EMITTER_POINT;
        F.delta_emitter = F.delta_emitter || e.type == LRT_EMITTER_SPOT || e.type == LRT_EMITTER_DIRECTIONAL;
        F.mesh_emitter = F.mesh_emitter || (e.type == LRT_EMITTER_AREA && e.shape >= 0 && (uint32_t) e.shape < d.n_shapes && d.shapes[e.shape].kind == LRT_SHAPE_MESH);
    }
    return F;
}

} // namespace lrt
