// extern "C" entry points of libliverrt.so (see include/liverrt.h).
// No exception crosses the ABI: every call returns a status and records a
// thread-local message for lrt_last_error().
#include "host_scene.h"
#include "device_scene.h"
#include "scene_prep.h"
#include "scene_check.h"
#include "image_io.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>

using namespace lrt;

static thread_local std::string g_error;
static lrt_status fail(lrt_status st, const std::string &msg) { g_error = msg; return st; }

#define LRT_TRY try {
#define LRT_CATCH } catch (const std::exception &e) { \
        std::string m = e.what(); \
        lrt_status st = LRT_ERR_INVALID; \
        if (m.find("hip") != std::string::npos || m.find("HIP") != std::string::npos) st = LRT_ERR_DEVICE; \
        if (m.find("cannot open") != std::string::npos || m.find("file not found") != std::string::npos) st = LRT_ERR_IO; \
        if (m.find("unsupported") != std::string::npos || m.find("not supported") != std::string::npos) st = LRT_ERR_UNSUPPORTED; \
        return fail(st, m); \
    } catch (...) { return fail(LRT_ERR_INVALID, "unknown error"); }

extern "C" {

const char *lrt_last_error(void) { return g_error.c_str(); }
int lrt_version(void) { return 121; }    // 1.21: lrt_render_stats::n_primary_entry (the per-pixel primary entry of the 64-byte-record volpath kernels; LRT_NO_PRIMARY_ENTRY); 1.20: lrt_sensor_probe; a camera to_world with scale factors and a film whose size plus filter radius leaves the footprint key's range are refused; 1.19: the conductor, plastic and twosided BSDFs; 1.18: lrt_medium_probe; a singular volume to_world and an empty use_grid_bbox header box are refused; 1.17: spot and directional emitters (lrt_emitter_desc::cutoff_angle / beam_width / texture); 1.16: tabulated / Rayleigh / blended phase functions (lrt_scene_desc.phases), lrt_phase_probe, lrt_math_eval fn 11 (cbrt); 1.15: lrt_render_stats::n_proven (the struct grows by 8 bytes); 1.14: the roughdielectric BSDF, lrt_math_eval fn 9 (erf) / 10 (erfinv); 1.13: lrt_bsdf_probe; 1.12: lrt_render_backward_grid, "<id>.sigma_t.data" in lrt_param_set / lrt_param_get; 1.11: lrt_envmap_probe; 1.10: the moment integrator (lrt_render_moment, lrt_render_moment_samples, lrt_scene_moment_get, lrt_moment_channel_name); 1.9: the guided denoiser (lrt_denoiser_create / lrt_denoise / lrt_denoiser_free), lrt_image_read_named; 1.8: lrt_render_stats.record_bytes, n_closed_guard; 1.7: area emitters on triangle meshes, lrt_emitter_probe; 1.6: sphere shapes and point emitters; 1.5: the aov integrator (lrt_render_aov, lrt_aov_desc), named multi-channel EXR writer; 1.2: bio media fields in lrt_medium_desc, biovolpath integrators, grad_medium in lrt_render_opts; 1.3: lrt_render_stats.lds_resident; 1.4: lrt_render_multi / lrt_render_backward_multi, PRB through heterogeneous media

static std::vector<std::pair<std::string, std::string>> parse_defines(const char *const *defines, int n) {
    std::vector<std::pair<std::string, std::string>> r;
    for (int i = 0; i < n; ++i) {
        std::string s = defines[i]; size_t eq = s.find('=');
        if (eq == std::string::npos) throw std::runtime_error("define \"" + s + "\" must have the form key=value");
        r.emplace_back(s.substr(0, eq), s.substr(eq + 1));
    }
    return r;
}

lrt_status lrt_scene_load_xml_string(const char *xml, const char *base_dir, const char *const *defines, int n_defines, lrt_scene **out) {
    if (!xml || !out) return fail(LRT_ERR_INVALID, "lrt_scene_load_xml_string: null argument");
    *out = nullptr;
    LRT_TRY
        std::unique_ptr<lrt_scene> s(new lrt_scene());
        load_scene_xml(xml, base_dir ? base_dir : "", parse_defines(defines, n_defines), s->st);
        *out = s.release();
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_scene_load_xml(const char *path, const char *const *defines, int n_defines, lrt_scene **out) {
    if (!path || !out) return fail(LRT_ERR_INVALID, "lrt_scene_load_xml: null argument");
    *out = nullptr;
    std::ifstream f(path, std::ios::binary);
    if (!f) return fail(LRT_ERR_IO, std::string("cannot open \"") + path + "\"");
    std::stringstream ss; ss << f.rdbuf();
    std::string p = path, dir; size_t sl = p.rfind('/'); dir = sl == std::string::npos ? "." : p.substr(0, sl);
    return lrt_scene_load_xml_string(ss.str().c_str(), dir.c_str(), defines, n_defines, out);
}

lrt_status lrt_scene_from_desc(const lrt_scene_desc *desc, lrt_scene **out) {
    if (!desc || !out) return fail(LRT_ERR_INVALID, "lrt_scene_from_desc: null argument");
    *out = nullptr;
    LRT_TRY
        validate_scene_desc(*desc);                              // scene_check.cpp
        std::unique_ptr<lrt_scene> s(new lrt_scene());
        s->st.copy_from(*desc);
        *out = s.release();
        return LRT_OK;
    LRT_CATCH
}

const lrt_scene_desc *lrt_scene_desc_get(const lrt_scene *scene) { return scene ? &scene->st.desc : nullptr; }

static void multi_release(lrt_scene *s) {
    if (s->multi_ctx) { multi_context_destroy(s->multi_ctx); s->multi_ctx = nullptr; }
    for (auto *D : s->multi) device_scene_destroy(D);
    s->multi.clear(); s->multi_ids.clear();
}

void lrt_scene_free(lrt_scene *scene) {
    if (!scene) return;
    multi_release(scene);
    if (scene->dev) device_scene_destroy(scene->dev);
    delete scene;
}

// One device image per entry of the device list (device_ids == NULL: devices 0 .. n - 1), kept until another list is asked for.
static void ensure_devices(lrt_scene *s, int n, const int *ids) {
    if (n < 1 || n > 64) throw std::invalid_argument("lrt_render_multi: n_devices must be 1 .. 64");
    std::vector<int> want(n); for (int i = 0; i < n; ++i) want[i] = ids ? ids[i] : i;
    if (want != s->multi_ids) {
        multi_release(s);
        for (int dev : want) s->multi.push_back(device_scene_create(s->st.desc, dev));
        s->multi_ids = want; s->multi_params_dirty = false;
    } else if (s->multi_params_dirty) { for (auto *D : s->multi) device_scene_update_params(D, s->st.desc, s->multi_grids_dirty); s->multi_params_dirty = false; }
    s->multi_grids_dirty = false;
}

// device < 0: whatever device the image already lives on (0 when there is none yet).  A render that names another device
// than the current one moves the scene there (one process per GPU is the intended use; this keeps a mistake from reading
// another GPU's pointers).
static void ensure_device(lrt_scene *s, int device) {
    if (s->dev && device >= 0 && device != s->dev_ordinal) { device_scene_destroy(s->dev); s->dev = nullptr; }
    if (!s->dev) { s->dev_ordinal = device < 0 ? 0 : device; s->dev = device_scene_create(s->st.desc, s->dev_ordinal); s->params_dirty = false; }
    else if (s->params_dirty) { device_scene_update_params(s->dev, s->st.desc, s->grids_dirty); s->params_dirty = false; }
    s->grids_dirty = false;               // (a fresh device image has uploaded the current grids)
}

lrt_status lrt_render(lrt_scene *scene, const lrt_render_opts *opts, float *film_raw, float *image) {
    if (!scene) return fail(LRT_ERR_INVALID, "lrt_render: null scene");
    LRT_TRY
        ensure_device(scene, opts ? opts->device : 0);
        device_render(scene->dev, scene->st.desc, opts, film_raw, image, scene->stats);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_render_multi(lrt_scene *scene, const lrt_render_opts *opts, int n_devices, const int *device_ids, float *film_raw, float *image) {
    if (!scene) return fail(LRT_ERR_INVALID, "lrt_render_multi: null scene");
    LRT_TRY
        if (scene->st.has_aov) return fail(LRT_ERR_UNSUPPORTED, "lrt_render_multi: an aov scene renders on one device (lrt_render_aov)");
        if (scene->st.has_moment) return fail(LRT_ERR_UNSUPPORTED, "lrt_render_multi: a moment scene renders on one device (lrt_render_moment; shard it with tile_rank / tile_count)");
        if (opts && (opts->tile_count > 1 || opts->tile_rank != 0)) throw std::invalid_argument("lrt_render_multi shards the image itself: tile_rank / tile_count must be 0 / 1 (or 0 / 0)");
        ensure_devices(scene, n_devices, device_ids);
        device_render_multi(scene->multi, scene->multi_ctx, scene->st.desc, opts, film_raw, image, scene->stats);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_render_backward_multi(lrt_scene *scene, const lrt_render_opts *opts, int n_devices, const int *device_ids, const float *grad_image, lrt_param_grads *out) {
    if (!scene || !grad_image || !out) return fail(LRT_ERR_INVALID, "lrt_render_backward_multi: null argument");
    LRT_TRY
        if (scene->st.has_aov) return fail(LRT_ERR_UNSUPPORTED, "lrt_render_backward_multi: the aov integrator has no adjoint here");
        if (scene->st.has_moment) return fail(LRT_ERR_UNSUPPORTED, "lrt_render_backward_multi: the moment integrator has no adjoint here");
        if (opts && (opts->tile_count > 1 || opts->tile_rank != 0)) throw std::invalid_argument("lrt_render_backward_multi shards the image itself: tile_rank / tile_count must be 0 / 1 (or 0 / 0)");
        ensure_devices(scene, n_devices, device_ids);
        device_render_backward_multi(scene->multi, scene->multi_ctx, scene->st.desc, opts, grad_image, out, scene->stats);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_math_eval(int fn, const float *x, const float *y, uint32_t n, float *out, float *out2, int device) {
    if (!x || !out) return fail(LRT_ERR_INVALID, "lrt_math_eval: null argument");
    LRT_TRY
        device_math_eval(fn, x, y, n, out, out2, device);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_render_stats_get(const lrt_scene *scene, lrt_render_stats *out) {
    if (!scene || !out) return fail(LRT_ERR_INVALID, "lrt_render_stats_get: null argument");
    *out = scene->stats; return LRT_OK;
}

lrt_status lrt_film_develop(lrt_scene *scene, const float *film_raw, float *image, int on_device) {
    if (!scene || !film_raw || !image) return fail(LRT_ERR_INVALID, "lrt_film_develop: null argument");
    LRT_TRY
        ensure_device(scene, -1);
        device_develop(scene->dev, film_raw, image, on_device);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_render_samples(lrt_scene *scene, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out) {
    if (!scene || !out) return fail(LRT_ERR_INVALID, "lrt_render_samples: null argument");
    LRT_TRY
        ensure_device(scene, opts ? opts->device : 0);
        device_render_samples(scene->dev, scene->st.desc, opts, lane_begin, n, out, scene->stats);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_render_backward(lrt_scene *scene, const lrt_render_opts *opts, const float *grad_image, lrt_param_grads *out) {
    if (!scene || !grad_image || !out) return fail(LRT_ERR_INVALID, "lrt_render_backward: null argument");
    if (scene->st.has_aov) return fail(LRT_ERR_UNSUPPORTED, "lrt_render_backward: the aov integrator has no adjoint here");
    if (scene->st.has_moment) return fail(LRT_ERR_UNSUPPORTED, "lrt_render_backward: the moment integrator has no adjoint here");
    LRT_TRY
        ensure_device(scene, opts ? opts->device : 0);
        device_render_backward(scene->dev, scene->st.desc, opts, grad_image, out, scene->stats);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_render_backward_grid(lrt_scene *scene, const lrt_render_opts *opts, const float *grad_image, lrt_param_grads *out, float *d_grid) {
    if (!scene || !grad_image || !out || !d_grid) return fail(LRT_ERR_INVALID, "lrt_render_backward_grid: null argument");
    if (scene->st.has_aov) return fail(LRT_ERR_UNSUPPORTED, "lrt_render_backward_grid: the aov integrator has no adjoint here");
    if (scene->st.has_moment) return fail(LRT_ERR_UNSUPPORTED, "lrt_render_backward_grid: the moment integrator has no adjoint here");
    const int gm = opts ? opts->grad_medium : 0;
    if (gm < 0 || gm >= (int) scene->st.desc.n_media || scene->st.desc.media[gm].type != LRT_MEDIUM_HETEROGENEOUS)
        return fail(LRT_ERR_INVALID, "lrt_render_backward_grid: grad_medium " + std::to_string(gm) + " is not a heterogeneous medium of the scene (the grid gradient belongs to one medium with a sigma_t grid)");
    LRT_TRY
        ensure_device(scene, opts ? opts->device : 0);
        device_render_backward(scene->dev, scene->st.desc, opts, grad_image, out, scene->stats, d_grid);
        return LRT_OK;
    LRT_CATCH
}

// ---- the aov integrator
lrt_status lrt_scene_aov_get(const lrt_scene *scene, lrt_aov_desc *out) {
    if (!scene || !out) return fail(LRT_ERR_INVALID, "lrt_scene_aov_get: null argument");
    if (!scene->st.has_aov) return fail(LRT_ERR_INVALID, "lrt_scene_aov_get: the scene has no aov integrator");
    *out = scene->st.aov; return LRT_OK;
}

const char *lrt_aov_channel_name(const lrt_scene *scene, int c) {
    if (!scene || !scene->st.has_aov || c < 0 || c >= (int) scene->st.aov_channel_names.size()) return nullptr;
    return scene->st.aov_channel_names[(size_t) c].c_str();
}

// the integrator comes from the scene: lrt_render_opts may not override what the nested integrators are
static lrt_status check_aov_call(const lrt_scene *scene, const lrt_render_opts *opts, const char *fn) {
    if (!scene->st.has_aov) return fail(LRT_ERR_INVALID, std::string(fn) + ": the scene has no aov integrator");
    if (opts && (opts->integrator != -1 || opts->max_depth != -2 || opts->rr_depth != -1 || opts->hide_emitters != -1))
        return fail(LRT_ERR_INVALID, std::string(fn) + ": integrator, max_depth, rr_depth and hide_emitters come from the scene's aov integrator (leave them at -1 / -2 / -1 / -1)");
    if (opts && opts->tile_count > 1) return fail(LRT_ERR_UNSUPPORTED, std::string(fn) + ": tile sharding of an aov render is not supported");
    return LRT_OK;
}

lrt_status lrt_render_aov(lrt_scene *scene, const lrt_render_opts *opts, float *aov_film_raw, float *image) {
    if (!scene) return fail(LRT_ERR_INVALID, "lrt_render_aov: null scene");
    lrt_status st = check_aov_call(scene, opts, "lrt_render_aov");
    if (st != LRT_OK) return st;
    LRT_TRY
        ensure_device(scene, opts ? opts->device : 0);
        device_render_aov(scene->dev, scene->st.desc, scene->st.aov, opts, aov_film_raw, image, scene->stats);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_render_aov_samples(lrt_scene *scene, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out) {
    if (!scene || !out) return fail(LRT_ERR_INVALID, "lrt_render_aov_samples: null argument");
    lrt_status st = check_aov_call(scene, opts, "lrt_render_aov_samples");
    if (st != LRT_OK) return st;
    LRT_TRY
        ensure_device(scene, opts ? opts->device : 0);
        device_render_aov_samples(scene->dev, scene->st.desc, scene->st.aov, opts, lane_begin, n, out, scene->stats);
        return LRT_OK;
    LRT_CATCH
}

// ---- the moment integrator
lrt_status lrt_scene_moment_get(const lrt_scene *scene, lrt_moment_desc *out) {
    if (!scene || !out) return fail(LRT_ERR_INVALID, "lrt_scene_moment_get: null argument");
    if (!scene->st.has_moment) return fail(LRT_ERR_INVALID, "lrt_scene_moment_get: the scene has no moment integrator");
    *out = scene->st.moment; return LRT_OK;
}

const char *lrt_moment_channel_name(const lrt_scene *scene, int c) {
    if (!scene || !scene->st.has_moment || c < 0 || c >= (int) scene->st.moment_channel_names.size()) return nullptr;
    return scene->st.moment_channel_names[(size_t) c].c_str();
}

// the nested integrator comes from the scene, as for aov
static lrt_status check_moment_call(const lrt_scene *scene, const lrt_render_opts *opts, const char *fn) {
    if (!scene->st.has_moment) return fail(LRT_ERR_INVALID, std::string(fn) + ": the scene has no moment integrator");
    if (opts && (opts->integrator != -1 || opts->max_depth != -2 || opts->rr_depth != -1 || opts->hide_emitters != -1))
        return fail(LRT_ERR_INVALID, std::string(fn) + ": integrator, max_depth, rr_depth and hide_emitters come from the scene's nested integrator (leave them at -1 / -2 / -1 / -1)");
    return LRT_OK;
}

lrt_status lrt_render_moment(lrt_scene *scene, const lrt_render_opts *opts, float *film_raw, float *image) {
    if (!scene) return fail(LRT_ERR_INVALID, "lrt_render_moment: null scene");
    lrt_status st = check_moment_call(scene, opts, "lrt_render_moment");
    if (st != LRT_OK) return st;
    LRT_TRY
        ensure_device(scene, opts ? opts->device : 0);
        device_render_moment(scene->dev, scene->st.desc, opts, film_raw, image, scene->stats);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_render_moment_samples(lrt_scene *scene, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out) {
    if (!scene || !out) return fail(LRT_ERR_INVALID, "lrt_render_moment_samples: null argument");
    lrt_status st = check_moment_call(scene, opts, "lrt_render_moment_samples");
    if (st != LRT_OK) return st;
    LRT_TRY
        ensure_device(scene, opts ? opts->device : 0);
        device_render_moment_samples(scene->dev, scene->st.desc, opts, lane_begin, n, out, scene->stats);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_trace(lrt_scene *scene, const lrt_rays_soa *rays, const lrt_hits_soa *hits, uint32_t n, int any_hit) {
    if (!scene || !rays || !hits) return fail(LRT_ERR_INVALID, "lrt_trace: null argument");
    LRT_TRY
        ensure_device(scene, -1);
        device_trace(scene->dev, rays, hits, n, any_hit);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_primary_entry_get(lrt_scene *scene, uint16_t *out, uint64_t n_pixels, int device) {
    if (!scene || (!out && n_pixels)) return fail(LRT_ERR_INVALID, "lrt_primary_entry_get: null argument");
    LRT_TRY
        ensure_device(scene, device);
        const std::vector<uint16_t> &t = device_primary_entry(scene->dev);
        const uint64_t want = (uint64_t) scene->st.desc.film.crop_width * (uint64_t) scene->st.desc.film.crop_height;
        if (n_pixels != want) return fail(LRT_ERR_INVALID, "lrt_primary_entry_get: n_pixels is not the crop window's pixel count");
        for (uint64_t i = 0; i < n_pixels; ++i) out[i] = t.empty() ? (uint16_t) 0 : t[i];
        return LRT_OK;
    LRT_CATCH
}

// The frame of the six probe entry points: the null and medium checks, then device_probe.  `columns`: the inputs in the order of the
// kind's lane record (probes.h).  medium: the index for the kinds that take one (phase, medium), null for the others.
static lrt_status probe_call(const char *fn, ProbeKind kind, lrt_scene *scene, const int *medium, std::initializer_list<ProbeColumn> columns, uint32_t n, float *out, int device) {
    bool null = !scene || (!out && n);
    for (const ProbeColumn &c : columns) null = null || (!c.p && n);
    if (null) return fail(LRT_ERR_INVALID, std::string(fn) + ": null argument");
    if (medium && (*medium < 0 || (size_t) *medium >= scene->st.media.size())) return fail(LRT_ERR_INVALID, std::string(fn) + ": no such medium");
    LRT_TRY
        ensure_device(scene, device);
        device_probe(scene->dev, kind, medium ? *medium : 0, columns, n, out);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_emitter_probe(lrt_scene *scene, const float *ref_p, const float *sample, uint32_t n, float *out, int device) {
    return probe_call("lrt_emitter_probe", PROBE_EMITTER, scene, nullptr, { { ref_p, 3 }, { sample, 2 } }, n, out, device);
}

lrt_status lrt_envmap_probe(lrt_scene *scene, const float *dir, uint32_t n, float *out, int device) {
    return probe_call("lrt_envmap_probe", PROBE_ENVMAP, scene, nullptr, { { dir, 3 } }, n, out, device);
}

lrt_status lrt_bsdf_probe(lrt_scene *scene, const float *o, const float *d, const float *sample, const float *wo_query, uint32_t n, float *out, int device) {
    return probe_call("lrt_bsdf_probe", PROBE_BSDF, scene, nullptr, { { o, 3 }, { d, 3 }, { sample, 3 }, { wo_query, 3 } }, n, out, device);
}

lrt_status lrt_phase_probe(lrt_scene *scene, int medium, const float *wi, const float *sample, const float *wo_query, uint32_t n, float *out, int device) {
    return probe_call("lrt_phase_probe", PROBE_PHASE, scene, &medium, { { wi, 3 }, { sample, 3 }, { wo_query, 3 } }, n, out, device);
}

lrt_status lrt_medium_probe(lrt_scene *scene, int medium, const float *o, const float *d, const float *maxt, const float *sample, const uint32_t *channel,
                            uint32_t n, float *out, int device) {
    LRT_TRY
        std::vector<float> ch;                                   // the lane record carries the channel as a float, clamped to 2
        if (channel) for (uint32_t i = 0; i < n; ++i) ch.push_back((float) std::min<uint32_t>(channel[i], 2u));
        return probe_call("lrt_medium_probe", PROBE_MEDIUM, scene, &medium, { { o, 3 }, { d, 3 }, { maxt, 1 }, { sample, 1 }, { channel ? ch.data() : nullptr, 1 } }, n, out, device);
    LRT_CATCH
}

lrt_status lrt_sensor_probe(lrt_scene *scene, const float *in, uint32_t n, float *out, int device) {
    return probe_call("lrt_sensor_probe", PROBE_SENSOR, scene, nullptr, { { in, 5 } }, n, out, device);
}

static lrt_medium_desc *find_medium(lrt_scene *s, const char *key, const char **rest) {
    for (auto &M : s->st.media) {
        size_t L = strlen(M.id);
        if (!strncmp(key, M.id, L) && key[L] == '.') { *rest = key + L + 1; return &M; }
    }
    return nullptr;
}

lrt_status lrt_param_set(lrt_scene *scene, const char *key, const float *v, int n) {
    if (!scene || !key || !v) return fail(LRT_ERR_INVALID, "lrt_param_set: null argument");
    const char *rest = nullptr; lrt_medium_desc *M = find_medium(scene, key, &rest);
    if (!M) return fail(LRT_ERR_INVALID, std::string("unknown parameter \"") + key + "\"");
    if (!strcmp(rest, "sigma_t.value") || !strcmp(rest, "albedo.value")) {
        if (n != 1 && n != 3) return fail(LRT_ERR_INVALID, "expected 1 or 3 values");
        float *dst = rest[0] == 's' ? M->sigma_t : M->albedo;
        for (int i = 0; i < 3; ++i) dst[i] = v[n == 3 ? i : 0];
    } else if (!strcmp(rest, "sigma_t.data") && M->type == LRT_MEDIUM_HETEROGENEOUS) {
        // mi.traverse's "<medium>.sigma_t.data" (src/volumes/grid.cpp traverse): same resolution, new values; the maximum is taken again
        // as parameters_changed() does (src/media/heterogeneous.cpp).  Checked in full before anything is written.
        std::vector<float> &data = scene->st.meddata[(size_t) (M - scene->st.media.data())];
        if (n < 0 || (size_t) n != data.size()) return fail(LRT_ERR_INVALID, std::string("\"") + key + "\": expected " + std::to_string(data.size()) + " values (res_x * res_y * res_z), got " + std::to_string(n));
        float mx = 0.f;
        for (int i = 0; i < n; ++i) {
            if (!std::isfinite(v[i]) || v[i] < 0.f) return fail(LRT_ERR_INVALID, std::string("\"") + key + "\": the grid values must be finite and >= 0");
            mx = std::max(mx, v[i]);
        }
        if (!(mx > 0.f)) return fail(LRT_ERR_INVALID, std::string("\"") + key + "\": the grid's maximum must be above 0 (it is the majorant)");
        std::copy(v, v + n, data.begin());                  // in place: lrt_scene_desc_get()->media[i].grid_data keeps pointing here
        M->grid_max = mx;
        scene->grids_dirty = true; scene->multi_grids_dirty = true;
    } else if (!strcmp(rest, "scale")) M->scale = v[0];
    else if (M->type == LRT_MEDIUM_PARENCHYMA && (!strcmp(rest, "sigma_blood.value") || !strcmp(rest, "sigma_bile.value") || !strcmp(rest, "sigma_lipid_water.value"))) {
        // what `parenchyma` puts into mi.traverse (src/media/parenchyma.cpp:154-160): the absorbers' coefficients and sigma_hepatocity
        if (n != 1 && n != 3) return fail(LRT_ERR_INVALID, "expected 1 or 3 values");
        float *dst;
        if (!strncmp(rest, "sigma_bile", 10)) dst = M->sigma_bile;
        else if (!strncmp(rest, "sigma_blood", 11)) dst = M->sigma_blood;
        else dst = M->sigma_lipid_water;
        for (int i = 0; i < 3; ++i) dst[i] = v[n == 3 ? i : 0];
    } else if (M->type == LRT_MEDIUM_PARENCHYMA && !strcmp(rest, "sigma_hepatocity")) M->sigma_hepatocity = v[0];
    else if (!strcmp(rest, "phase_function.g") && !(scene->st.desc.n_phases && M->phase_index >= 0)) {     // (a medium with an entry of the phase table has no parameter keys)
        // mi.traverse exposes `g` for an hg phase function only (src/phase/hg.cpp:60-62; isotropic.cpp has no parameter).  The
        // one extension kept from round 1: a NON-ZERO g on an isotropic medium turns it into hg ("HG variant ...
        // supplied through lrt_param_set"); g = 0 on an isotropic medium is rejected like any unknown key.
        if (!hg_g_valid(v[0])) return fail(LRT_ERR_INVALID, kHgRangeText);
        if (M->phase != LRT_PHASE_HG && v[0] == 0.f) return fail(LRT_ERR_INVALID, std::string("unknown parameter \"") + key + "\" (the medium's phase function is isotropic)");
        M->g = v[0]; M->phase = LRT_PHASE_HG;
    } else return fail(LRT_ERR_INVALID, std::string("unknown parameter \"") + key + "\"");
    scene->params_dirty = true; scene->multi_params_dirty = true;
    return LRT_OK;
}

lrt_status lrt_param_get(const lrt_scene *scene, const char *key, float *v, int n) {
    if (!scene || !key || !v) return fail(LRT_ERR_INVALID, "lrt_param_get: null argument");
    const char *rest = nullptr; lrt_medium_desc *M = find_medium(const_cast<lrt_scene *>(scene), key, &rest);
    if (!M) return fail(LRT_ERR_INVALID, std::string("unknown parameter \"") + key + "\"");
    if (!strcmp(rest, "sigma_t.value")) { for (int i = 0; i < n && i < 3; ++i) v[i] = M->sigma_t[i]; }
    else if (!strcmp(rest, "albedo.value")) { for (int i = 0; i < n && i < 3; ++i) v[i] = M->albedo[i]; }
    else if (!strcmp(rest, "sigma_t.data") && M->type == LRT_MEDIUM_HETEROGENEOUS) {
        const size_t nv = (size_t) M->grid_res[0] * M->grid_res[1] * M->grid_res[2];
        if (n < 0 || (size_t) n != nv) return fail(LRT_ERR_INVALID, std::string("\"") + key + "\": expected room for " + std::to_string(nv) + " values (res_x * res_y * res_z), got " + std::to_string(n));
        std::copy(M->grid_data, M->grid_data + nv, v);
    }
    else if (!strcmp(rest, "scale")) v[0] = M->scale;
    else if (!strcmp(rest, "phase_function.g")) v[0] = M->g;
    else if (M->type == LRT_MEDIUM_PARENCHYMA && !strcmp(rest, "sigma_blood.value")) { for (int i = 0; i < n && i < 3; ++i) v[i] = M->sigma_blood[i]; }
    else if (M->type == LRT_MEDIUM_PARENCHYMA && !strcmp(rest, "sigma_bile.value")) { for (int i = 0; i < n && i < 3; ++i) v[i] = M->sigma_bile[i]; }
    else if (M->type == LRT_MEDIUM_PARENCHYMA && !strcmp(rest, "sigma_lipid_water.value")) { for (int i = 0; i < n && i < 3; ++i) v[i] = M->sigma_lipid_water[i]; }
    else if (M->type == LRT_MEDIUM_PARENCHYMA && !strcmp(rest, "sigma_hepatocity")) v[0] = M->sigma_hepatocity;
    else return fail(LRT_ERR_INVALID, std::string("unknown parameter \"") + key + "\"");
    return LRT_OK;
}

lrt_status lrt_image_read(const char *path, int *width, int *height, int *channels, float **data) {
    if (!path || !width || !height || !channels || !data) return fail(LRT_ERR_INVALID, "lrt_image_read: null argument");
    *data = nullptr;
    LRT_TRY
        Image im = read_image_rgb(path);
        float *p = (float *) malloc(im.data.size() * sizeof(float));
        if (!p) throw std::runtime_error("out of memory");
        memcpy(p, im.data.data(), im.data.size() * sizeof(float));
        *width = im.width; *height = im.height; *channels = im.channels; *data = p;
        return LRT_OK;
    LRT_CATCH
}

void lrt_image_free(float *data) { free(data); }

// ---- learned subsurface model, network stage
struct lrt_vae_model { std::vector<float> blob; };

lrt_status lrt_vae_model_create(const float *blob, uint64_t n_floats, lrt_vae_model **out) {
    if (!blob || !out) return fail(LRT_ERR_INVALID, "lrt_vae_model_create: null argument");
    if (n_floats != (uint64_t) LRT_VAE_N_FLOATS) return fail(LRT_ERR_INVALID, "lrt_vae_model_create: expected " + std::to_string(LRT_VAE_N_FLOATS) + " floats (include/liverrt.h)");
    for (uint64_t i = 0; i < n_floats; ++i) if (!std::isfinite(blob[i])) return fail(LRT_ERR_INVALID, "lrt_vae_model_create: non-finite weight");
    lrt_vae_model *m = new lrt_vae_model(); m->blob.assign(blob, blob + n_floats); *out = m;
    return LRT_OK;
}
void lrt_vae_model_free(lrt_vae_model *model) { delete model; }

lrt_status lrt_vae_scatter(lrt_vae_model *model, uint32_t n, const float *in_pos, const float *in_dir, const float *poly_coeffs, const float albedo[3], float g, float ior,
                           const float sigma_t[3], float fit_scale, uint32_t seed, float *out_pos, float *out_absorption, int device) {
    if (!model || !albedo || !sigma_t || (n && (!in_pos || !in_dir || !poly_coeffs || !out_pos || !out_absorption))) return fail(LRT_ERR_INVALID, "lrt_vae_scatter: null argument");
    if (!(fit_scale > 0.f)) return fail(LRT_ERR_INVALID, "lrt_vae_scatter: fit_scale must be positive");
    LRT_TRY
        device_vae_scatter(model->blob.data(), n, in_pos, in_dir, poly_coeffs, albedo, g, ior, sigma_t, fit_scale, seed, out_pos, out_absorption, device);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_image_write_exr(const char *path, int width, int height, int channels, const float *data) {
    if (!path || !data) return fail(LRT_ERR_INVALID, "lrt_image_write_exr: null argument");
    LRT_TRY
        write_exr(path, width, height, channels, data);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_image_write_exr_channels(const char *path, int width, int height, int n_channels, const char *const *names, const float *data) {
    if (!path || !names || !data) return fail(LRT_ERR_INVALID, "lrt_image_write_exr_channels: null argument");
    LRT_TRY
        std::vector<std::string> nm;
        for (int c = 0; c < n_channels; ++c) { if (!names[c]) throw std::invalid_argument("lrt_image_write_exr_channels: null channel name"); nm.emplace_back(names[c]); }
        write_exr_channels(path, width, height, nm, data);
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_image_write_png(const char *path, int width, int height, int channels, const float *data) {
    if (!path || !data) return fail(LRT_ERR_INVALID, "lrt_image_write_png: null argument");
    LRT_TRY
        write_png(path, width, height, channels, data);
        return LRT_OK;
    LRT_CATCH
}

// ---- guided denoiser (device.hip: denoiser_create / denoiser_run; kernels_denoise.h)
struct lrt_denoiser { Denoiser *dev = nullptr; int width = 0, height = 0; bool albedo = false, normals = false, alpha = false; lrt_denoise_params params{}; };

lrt_status lrt_denoiser_create(int width, int height, int use_albedo, int use_normals, int denoise_alpha, const lrt_denoise_params *params, int device, lrt_denoiser **out) {
    if (!out) return fail(LRT_ERR_INVALID, "lrt_denoiser_create: null argument");
    *out = nullptr;
    if (width < 1 || height < 1 || width > LRT_DENOISE_MAX_SIZE || height > LRT_DENOISE_MAX_SIZE)
        return fail(LRT_ERR_INVALID, "lrt_denoiser_create: size " + std::to_string(width) + " x " + std::to_string(height) + " outside 1 .. " + std::to_string(LRT_DENOISE_MAX_SIZE));
    lrt_denoise_params P = params ? *params : lrt_denoise_params{};
    if (P.iterations == 0) P.iterations = LRT_DENOISE_ITERATIONS;
    if (P.iterations < 1 || P.iterations > LRT_DENOISE_MAX_ITERATIONS)
        return fail(LRT_ERR_INVALID, "lrt_denoiser_create: iterations " + std::to_string(P.iterations) + " outside 1 .. " + std::to_string(LRT_DENOISE_MAX_ITERATIONS));
    struct { const char *name; float *v; float def; } fields[] = { { "sigma_color", &P.sigma_color, LRT_DENOISE_SIGMA_COLOR }, { "sigma_normal", &P.sigma_normal, LRT_DENOISE_SIGMA_NORMAL },
                                                                  { "sigma_albedo", &P.sigma_albedo, LRT_DENOISE_SIGMA_ALBEDO }, { "eps_a", &P.eps_a, LRT_DENOISE_EPS_A } };
    for (auto &f : fields) {
        if (*f.v == 0.f) *f.v = f.def;
        if (!(*f.v > 0.f) || !std::isfinite(*f.v)) return fail(LRT_ERR_INVALID, std::string("lrt_denoiser_create: ") + f.name + " must be positive and finite (0 selects the default)");
    }
    LRT_TRY
        lrt_denoiser *d = new lrt_denoiser();
        d->width = width; d->height = height; d->albedo = use_albedo != 0; d->normals = use_normals != 0; d->alpha = denoise_alpha != 0; d->params = P;
        try { d->dev = denoiser_create(width, height, d->albedo, d->normals, d->alpha, P, device); } catch (...) { delete d; throw; }
        *out = d;
        return LRT_OK;
    LRT_CATCH
}

lrt_status lrt_denoise(lrt_denoiser *denoiser, const float *noisy, int channels, const float *albedo, const float *normals, float *out, int device_buffers) {
    if (!denoiser || !noisy || !out) return fail(LRT_ERR_INVALID, "lrt_denoise: null argument");
    if (channels != 3 && channels != 4) return fail(LRT_ERR_INVALID, "lrt_denoise: " + std::to_string(channels) + " channels (expected 3 or 4)");
    if (denoiser->albedo && !albedo) return fail(LRT_ERR_INVALID, "lrt_denoise: the denoiser was created with the albedo guide, but no albedo was given");
    if (!denoiser->albedo && albedo) return fail(LRT_ERR_INVALID, "lrt_denoise: an albedo was given, but the denoiser was created without the albedo guide");
    if (denoiser->normals && !normals) return fail(LRT_ERR_INVALID, "lrt_denoise: the denoiser was created with the normals guide, but no normals were given");
    if (!denoiser->normals && normals) return fail(LRT_ERR_INVALID, "lrt_denoise: normals were given, but the denoiser was created without the normals guide");
    if (out == noisy || out == albedo || out == normals) return fail(LRT_ERR_INVALID, "lrt_denoise: out must not alias an input");
    LRT_TRY
        denoiser_run(denoiser->dev, noisy, channels, albedo, normals, out, device_buffers);
        return LRT_OK;
    LRT_CATCH
}

void lrt_denoiser_free(lrt_denoiser *denoiser) { if (denoiser) { denoiser_destroy(denoiser->dev); delete denoiser; } }

lrt_status lrt_denoiser_get(const lrt_denoiser *denoiser, int *width, int *height, lrt_denoise_params *params) {
    if (!denoiser) return fail(LRT_ERR_INVALID, "lrt_denoiser_get: null argument");
    if (width) *width = denoiser->width;
    if (height) *height = denoiser->height;
    if (params) *params = denoiser->params;
    return LRT_OK;
}

lrt_status lrt_image_read_named(const char *path, int *width, int *height, int *channels, float **data, char **names) {
    if (!path || !width || !height || !channels || !data || !names) return fail(LRT_ERR_INVALID, "lrt_image_read_named: null argument");
    *data = nullptr; *names = nullptr;
    LRT_TRY
        std::string ps = path, ext; size_t dot = ps.rfind('.'); if (dot != std::string::npos) ext = ps.substr(dot + 1);
        for (auto &c : ext) c = (char) tolower(c);
        Image im; std::string joined;
        if (ext == "exr") {
            Image e = read_exr(ps);
            auto idx = [&](const char *n) { for (size_t k = 0; k < e.channel_names.size(); ++k) if (e.channel_names[k] == n) return (int) k; return -1; };
            int r = idx("R"), g = idx("G"), b = idx("B"), a = idx("A"), yc = idx("Y");
            std::vector<int> map;
            if (r >= 0 && g >= 0 && b >= 0) { map = { r, g, b }; if (a >= 0) map.push_back(a); }
            else if (yc >= 0) { map = { yc }; if (a >= 0) map.push_back(a); }
            for (int k = 0; k < e.channels; ++k) { bool used = false; for (int m : map) used = used || m == k; if (!used) map.push_back(k); }
            im.width = e.width; im.height = e.height; im.channels = e.channels; im.data.resize(e.data.size());
            for (size_t p = 0; p < (size_t) e.width * e.height; ++p)
                for (size_t c = 0; c < map.size(); ++c) im.data[p * map.size() + c] = e.data[p * e.channels + map[c]];
            for (size_t c = 0; c < map.size(); ++c) { if (c) joined += '\n'; joined += e.channel_names[map[c]]; }
        } else im = read_image_rgb(ps);
        float *p = (float *) malloc(std::max<size_t>(im.data.size(), 1) * sizeof(float));
        char *nm = (char *) malloc(joined.size() + 1);
        if (!p || !nm) { free(p); free(nm); throw std::runtime_error("out of memory"); }
        memcpy(p, im.data.data(), im.data.size() * sizeof(float)); memcpy(nm, joined.c_str(), joined.size() + 1);
        *width = im.width; *height = im.height; *channels = im.channels; *data = p; *names = nm;
        return LRT_OK;
    LRT_CATCH
}

void lrt_image_free_names(char *names) { free(names); }

} // extern "C"
