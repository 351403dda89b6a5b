// Host driver of the wavefront renderer: device scene upload, queue management,
// kernel launches, timing.  Every HIP runtime call and every kernel lives behind this file.  What a scene's device image holds is
// computed outside it, by the host-only scene_prep.cpp (arrays, scene record, media tables, resolved options, tile lists, the
// 64-byte-record predicate); this file uploads that and launches.
#include "host_scene.h"
#include "device_scene.h"
#include "kernels_prb.h"
#include "kernels_vae.h"
#include "kernels_aov.h"
#include "kernels_denoise.h"
#include "kernels_moment.h"
#include "probes.h"
#include <functional>
#include "scene_prep.h"
#include <cmath>
#include <array>
#include <cstring>
#include <algorithm>
#include <stdexcept>
#include <string>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <chrono>
#include <exception>
#include <dlfcn.h>
#include <rccl/rccl.h>      // types and enums only: the functions are bound with dlopen (librccl.so is not a link-time dependency)

namespace lrt {

#define HIP_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

template <typename T> static T *dev_upload(const T *src, size_t n, hipStream_t st) {
    T *p = nullptr; size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HIP_CHECK(hipMalloc((void **) &p, bytes));
    if (n) HIP_CHECK(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    return p;
}

// A temporary device buffer of one call, freed when the call returns or throws.
struct DevTmp {
    float *p = nullptr;
    DevTmp() = default;
    explicit DevTmp(size_t floats) { alloc(floats); }
    DevTmp(const DevTmp &) = delete; DevTmp &operator=(const DevTmp &) = delete;
    void alloc(size_t floats) { HIP_CHECK(hipMalloc((void **) &p, std::max<size_t>(floats, 1) * sizeof(float))); }
    void upload(const float *src, size_t floats, hipStream_t st) { alloc(floats); HIP_CHECK(hipMemcpyAsync(p, src, floats * sizeof(float), hipMemcpyHostToDevice, st)); }
    ~DevTmp() { if (p) (void) hipFree(p); }
};

// the checks of every entry point that names a device by its ordinal
static void select_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) throw std::runtime_error("no HIP device available: the hip_ad_rgb back-end has no CPU fallback");
    if (device < 0 || device >= count) throw std::runtime_error("invalid HIP device ordinal " + std::to_string(device));
    HIP_CHECK(hipSetDevice(device));
}

// lrt_render_opts of a call without any: everything "the scene's own", one tile
static lrt_render_opts default_opts() { return lrt_render_opts{ -1, -2, -1, -1, 0, 0, 0, 1, 0, 0, 0, 0 }; }

// one launch's (or one nested render's) stats added to a sequential total
static void add_stats(lrt_render_stats &total, const lrt_render_stats &s) {
    total.n_samples += s.n_samples; total.n_iter += s.n_iter; total.n_shadow += s.n_shadow; total.n_launches += s.n_launches;
    total.n_records += s.n_records; total.kernel_ms += s.kernel_ms; total.total_ms += s.total_ms;
    total.record_bytes = s.record_bytes; total.n_closed_guard += s.n_closed_guard; total.n_proven += s.n_proven; total.n_primary_entry += s.n_primary_entry;
}

#define LRT_LAUNCH_SLOTS 64
#define LRT_WIDE_BLOCK 768          // workgroup size of the render kernels with wide path records (volpathmis, volpath with heterogeneous media) on the LDS BVH

struct DeviceScene {
    int device = 0;
    hipStream_t stream = nullptr;
    DScene sc{};                           // host copy of the scene record; the kernels read d_sc (constant address space)
    DScene *d_sc = nullptr;
    // launch-argument slots (DLaunch, read by the kernels through the constant address space): a ring in device memory
    // filled from a pinned host ring, one slot per launch; a slot is reused only after LRT_LAUNCH_SLOTS further launches
    // of the same in-order stream, i.e. long after its kernel has finished
    DLaunch *d_launch = nullptr, *h_launch = nullptr; uint32_t launch_next = 0;
    std::vector<void *> allocs;            // everything freed in the destructor
    // wavefront workspace
    uint32_t capacity = 0;
    DPathStreams q[2]{};
    float4 *dl[2] = { nullptr, nullptr }; size_t dl_records[2] = { 0, 0 }; float4 *L_buf = nullptr; size_t l_buf_lanes = 0;   // PRB: delta_L streams, primal radiance
    double *d_grads = nullptr; float *wfilm = nullptr; size_t wfilm_floats = 0; float *grad_image = nullptr; size_t grad_floats = 0;
    DCounters *counters = nullptr;
    DCounters *h_counters = nullptr;       // pinned
    std::vector<uint16_t> primary_tab;     // host copy of DScene::primary_tab (lrt_primary_entry_get)
    float *film = nullptr; size_t film_floats = 0;
    float *image = nullptr; size_t image_floats = 0;
    unsigned long long *pass_state[2] = { nullptr, nullptr }; size_t pass_state_lanes[2] = { 0, 0 };   // multi-pass renders: per-lane PCG32 states
    const unsigned long long *cur_pass_in = nullptr; unsigned long long *cur_pass_out = nullptr;
    uint32_t *pixel_slot = nullptr;         // inverse of pixel_list (pixel -> index in the list), tile-sharded renders
    uint32_t *pixel_list = nullptr; uint32_t pixel_list_rank = 0xffffffffu, pixel_list_count = 0, n_owned_pixels = 0;
    uint32_t *halo_list = nullptr; uint32_t halo_rank = 0xffffffffu, halo_count = 0, halo_width = 0, n_halo_pixels = 0;   // own tiles dilated by `halo_width` pixels (PRB weight film)
    std::vector<hipEvent_t> ev_pool;
    std::vector<DMedium> h_media; DMedium *d_media = nullptr;
    std::vector<DBioMedium> h_bio; DBioMedium *d_bio = nullptr;
    std::vector<DHetMedium> h_het; DHetMedium *d_het = nullptr; std::vector<float *> het_data; bool has_het = false, has_non_bio = false, need_mis = false; uint32_t ws_layouts = 0;   // ws_layouts: the record layouts the workspace is allocated for (layout_bit mask)
    bool ext = false;                      // spheres, point emitters, area emitters on meshes, a roughdielectric on a shape or a tabulated / Rayleigh / blended phase function on a referenced medium: the EXT kernel instances (ExtTracer, point- / mesh-emitter sampling, the rough BSDF, DScene::phases), wide records
    bool smooth_bsdf = false;              // a conductor / plastic / twosided on a shape (it sets `ext` too): prbvolpath's refusal names it
    bool has_area_emitter = false;         // decides the record layout: only an area emitter's pdf reads the last scatter position (record_layout.h)
    float *dgrid = nullptr; size_t dgrid_floats = 0;   // lrt_render_backward_grid with a host result: the device-side gradient grid
    bool prb_null = false;                 // prbvolpath.py:84-91 `handle_null_scattering`: a heterogeneous medium is attached to a shape
    DLdsInfo lds{}; bool use_lds = false; int n_cus = 256; int bvh_leaf = 4;
    // aov integrator: the AOV table (device copy), the AOV film and the inner images / merged image of the last aov render
    DAovSpec *d_aov_spec = nullptr; uint32_t *d_first_face = nullptr;
    float *aov_film = nullptr; size_t aov_film_floats = 0; float *aov_image = nullptr; size_t aov_image_floats = 0; float *aov_inner = nullptr; size_t aov_inner_floats = 0;

    template <typename T> T *track(T *p) { allocs.push_back((void *) p); return p; }
    void release(void *p) {                // free one tracked allocation now (a workspace that is being replaced by a larger one)
        if (!p) return;
        for (auto it = allocs.begin(); it != allocs.end(); ++it) if (*it == p) { allocs.erase(it); break; }
        (void) hipFree(p);
    }
    // Grows one of the buffers above to `want` elements (`have`: its size counter).  The order is ensure_workspace's: the old buffer is released and
    // pointer and counter are cleared BEFORE the allocation, the counter is set only after it, so a failed hipMalloc leaves p = nullptr, have = 0
    // and the next call allocates again instead of writing through a stale size.
    template <typename T> T *grow(T *&p, size_t &have, size_t want) {
        if (have >= want) return p;
        HIP_CHECK(hipStreamSynchronize(stream));
        release(p); p = nullptr; have = 0;
        HIP_CHECK(hipMalloc((void **) &p, std::max<size_t>(want, 1) * sizeof(T))); track(p);
        have = want;
        return p;
    }
    ~DeviceScene() {
        for (void *p : allocs) (void) hipFree(p);
        for (auto e : ev_pool) (void) hipEventDestroy(e);
        if (h_counters) (void) hipHostFree(h_counters);
        if (h_launch) (void) hipHostFree(h_launch);
        if (stream) (void) hipStreamDestroy(stream);
    }
};

void device_scene_destroy(DeviceScene *d) { delete d; }

static_assert(PREP_F_DELTA == F_DELTA && PREP_F_SMOOTH == F_SMOOTH && PREP_F_NULL == F_NULL, "scene_prep.h restates the BSDF leaf flags of dshade.h");

// log10 of the hepatocyte coefficient with the device's own arithmetic (liver.cpp:376 `dr::log2(att + 1) / dr::log2(10)`)
__global__ void k_bio_prepare(DBioMedium *bio, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bio[i].log10_hep = m_log2(bio[i].hepatocity + 1.f) / m_log2(10.f);
}

// Per-medium constants of the real-scattering weight (volpath.cpp:261-265), evaluated once with the device's own arithmetic:
// sigma_s / mean(sigma_t / combined) (spectral branch) and sigma_s / sigma_t, with sigma_s = sigma_t * albedo, combined = sigma_t.
__global__ void k_medium_prepare(DMedium *media, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DMedium &M = media[i];
    const V3 st(M.sigma_t[0], M.sigma_t[1], M.sigma_t[2]), ss = st * V3(M.albedo[0], M.albedo[1], M.albedo[2]);
    const V3 ws = ss / mean3(st / st), wp = ss / st;
    M.w_spec[0] = ws.x; M.w_spec[1] = ws.y; M.w_spec[2] = ws.z; M.w_plain[0] = wp.x; M.w_plain[1] = wp.y; M.w_plain[2] = wp.z;
}

// The media tables of prepare_media, with the grids' device pointers, and the two kernels that finish them with the device's arithmetic
static void upload_media(DeviceScene *D, const lrt_scene_desc &d) {
    prepare_media(d, D->sc.env.bsphere_r, D->h_media, D->h_bio, D->h_het);
    for (size_t i = 0; i < D->h_het.size(); ++i) D->h_het[i].data = D->het_data[i];
    HIP_CHECK(hipMemcpyAsync(D->d_bio, D->h_bio.data(), D->h_bio.size() * sizeof(DBioMedium), hipMemcpyHostToDevice, D->stream));
    k_bio_prepare<<<1, 64, 0, D->stream>>>(D->d_bio, (uint32_t) std::min<size_t>(D->h_bio.size(), 64));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(D->d_het, D->h_het.data(), D->h_het.size() * sizeof(DHetMedium), hipMemcpyHostToDevice, D->stream));
    HIP_CHECK(hipMemcpyAsync(D->d_media, D->h_media.data(), D->h_media.size() * sizeof(DMedium), hipMemcpyHostToDevice, D->stream));
    k_medium_prepare<<<1, 64, 0, D->stream>>>(D->d_media, (uint32_t) std::min<size_t>(D->h_media.size(), 64));
    HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------ the kernel instances
// Naming an instance's address instantiates it, so the tables below ARE the set of compiled render kernels (tests/golden/kernel_names.txt pins it):
// device_scene_create raises the LDS limit of their LDS rows, the launches pick from them, and a new instance is a new row here.
typedef void (*RenderFn)(ScenePtr, LaunchPtr);
// One k_render<mode, block, lds, ld, compact, ext>.  mode: the kernel selector (an LRT_INTEGRATOR_* value of the API or of device_types.h).
struct RenderRow { int mode; bool lds, ld, compact, ext; uint32_t block, record_bytes; RenderFn fn; };

template <int MODE, int BLOCK, bool LDS, bool LD, bool COMPACT = false, bool EXT = false> static void add_row(std::vector<RenderRow> &t) {
    static_assert(record_form_exists(record_layout(MODE), COMPACT), "this layout has no such form (record_layout.h, kRecordForms)");
    t.push_back({ MODE, LDS, LD, COMPACT, EXT, BLOCK, record_bytes(record_layout(MODE), COMPACT), k_render<MODE, BLOCK, LDS, LD, COMPACT, EXT> });
}
// a mode's wide-record instances: {LDS BVH (LDS_BLOCK threads), global BVH (LRT_BLOCK)} x {independent, ld} x {plain, EXT}
template <int MODE, int LDS_BLOCK> static void add_mode(std::vector<RenderRow> &t) {
    add_row<MODE, LDS_BLOCK, true, false>(t); add_row<MODE, LDS_BLOCK, true, true>(t);
    add_row<MODE, LDS_BLOCK, true, false, false, true>(t); add_row<MODE, LDS_BLOCK, true, true, false, true>(t);
    add_row<MODE, LRT_BLOCK, false, false>(t); add_row<MODE, LRT_BLOCK, false, true>(t);
    add_row<MODE, LRT_BLOCK, false, false, false, true>(t); add_row<MODE, LRT_BLOCK, false, true, false, true>(t);
}
// a mode's compact-record instances (80 / 88 bytes, or the 64-byte closed records): LDS BVH, 1024 threads, no EXT; {independent, ld}
template <int MODE> static void add_compact(std::vector<RenderRow> &t) { add_row<MODE, 1024, true, false, true>(t); add_row<MODE, 1024, true, true, true>(t); }

// every k_render instance, and k_render_prb [adjoint][lds][ld][het] / k_render_prb_grid [lds][ld] (1024 threads on the LDS BVH, else LRT_BLOCK; null: not compiled)
struct KernelTable { std::vector<RenderRow> render; RenderFn prb[2][2][2][2] = {}, prb_grid[2][2] = {}; };
template <bool LDS, bool LD> static void add_prb(KernelTable &t) {
    constexpr int BLOCK = LDS ? 1024 : LRT_BLOCK;
    t.prb[0][LDS][LD][0] = k_render_prb<false, BLOCK, LDS, LD, false>; t.prb[0][LDS][LD][1] = k_render_prb<false, BLOCK, LDS, LD, true>;
    t.prb[1][LDS][LD][0] = k_render_prb<true, BLOCK, LDS, LD, false>; t.prb[1][LDS][LD][1] = k_render_prb<true, BLOCK, LDS, LD, true>;
    t.prb_grid[LDS][LD] = k_render_prb_grid<BLOCK, LDS, LD>;
}
static const KernelTable &kernels() {
    static const KernelTable table = [] {
        KernelTable t; std::vector<RenderRow> &r = t.render;
#ifdef LRT_DEV_VOLPATH_ONLY                 // developer build (make dev): only ONE integrator's render kernels are compiled (default: volpath, independent sampler, LDS BVH;
#ifndef LRT_DEV_INTEGRATOR                  // make dev DEVFLAGS="-DLRT_DEV_INTEGRATOR=LRT_INTEGRATOR_BIOVOLPATH -DLRT_DEV_LD=true" for another) and no PRB kernel
#define LRT_DEV_INTEGRATOR LRT_INTEGRATOR_VOLPATH
#endif
#ifndef LRT_DEV_LD
#define LRT_DEV_LD false
#endif
#ifndef LRT_DEV_BLOCK
#define LRT_DEV_BLOCK 1024
#endif
        // the 64-byte-record instance stands in for "the C3 kernel" of a volpath developer build (any other integrator: its compact instance again, if its layout has a compact form)
#define LRT_DEV_CLOSED (LRT_DEV_INTEGRATOR == LRT_INTEGRATOR_VOLPATH ? LRT_INTEGRATOR_VOLPATH_CLOSED : LRT_DEV_INTEGRATOR)
        add_row<LRT_DEV_INTEGRATOR, LRT_DEV_BLOCK, true, LRT_DEV_LD>(r);
        if constexpr (record_form_exists(record_layout(LRT_DEV_INTEGRATOR), true)) {
            add_row<LRT_DEV_INTEGRATOR, LRT_DEV_BLOCK, true, LRT_DEV_LD, true>(r); add_row<LRT_DEV_CLOSED, LRT_DEV_BLOCK, true, LRT_DEV_LD, true>(r);
        }
#else
        add_mode<LRT_INTEGRATOR_PATH, 1024>(r); add_mode<LRT_INTEGRATOR_VOLPATH, 1024>(r); add_mode<LRT_INTEGRATOR_BIOVOLPATH, 1024>(r); add_mode<LRT_INTEGRATOR_BIOVOLPATH06, 1024>(r);
        // (the wide-record integrators run 768-thread workgroups on the LDS BVH: 3 waves per SIMD, 168 VGPRs instead of 128 + 200 - 430 B of scratch per lane;
        //  measured on the f4 bench configs: volpathmis +58 %, volpath with heterogeneous media +9 %; 512 threads: +54 % / -18 %)
        add_mode<LRT_INTEGRATOR_VOLPATH_HET, LRT_WIDE_BLOCK>(r); add_mode<LRT_INTEGRATOR_VOLPATHMIS, LRT_WIDE_BLOCK>(r); add_mode<LRT_INTEGRATOR_VOLPATHMIS_PLAIN, LRT_WIDE_BLOCK>(r);
        add_compact<LRT_INTEGRATOR_PATH>(r); add_compact<LRT_INTEGRATOR_VOLPATH>(r); add_compact<LRT_INTEGRATOR_BIOVOLPATH>(r); add_compact<LRT_INTEGRATOR_BIOVOLPATH06>(r);
        add_compact<LRT_INTEGRATOR_VOLPATH_CLOSED>(r);
        add_prb<false, false>(t); add_prb<false, true>(t); add_prb<true, false>(t); add_prb<true, true>(t);
#endif
        return t;
    }();
    return table;
}

typedef void (*AovFn)(ScenePtr, LaunchPtr, AovSpecPtr);
static AovFn aov_kernel(bool lds, bool ld, bool ext) {                  // k_aov<LDS, LD, EXT>: 1024 threads on the LDS BVH, else LRT_BLOCK
    static const AovFn t[2][2][2] = { { { k_aov<false, false, false>, k_aov<false, false, true> }, { k_aov<false, true, false>, k_aov<false, true, true> } },
                                      { { k_aov<true, false, false>, k_aov<true, false, true> }, { k_aov<true, true, false>, k_aov<true, true, true> } } };
    return t[lds][ld][ext];
}
typedef decltype(&k_trace<false, false>) TraceFn;
typedef decltype(&k_trace_lds<false, false>) TraceLdsFn;
static TraceFn trace_kernel(bool any_hit, bool ext) {                   // k_trace<ANY_HIT, EXT>: BVH in global memory
    static const TraceFn t[2][2] = { { k_trace<false, false>, k_trace<false, true> }, { k_trace<true, false>, k_trace<true, true> } };
    return t[any_hit][ext];
}
static TraceLdsFn trace_lds_kernel(bool any_hit, bool ext) {            // k_trace_lds<ANY_HIT, EXT>: the render kernels' tracer, BVH image in LDS
    static const TraceLdsFn t[2][2] = { { k_trace_lds<false, false>, k_trace_lds<false, true> }, { k_trace_lds<true, false>, k_trace_lds<true, true> } };
    return t[any_hit][ext];
}
static RenderFn moment_splat_kernel(bool wide, bool alpha) {            // k_moment_splat<WIDE, ALPHA> for a reconstruction filter and a film
    static const RenderFn t[2][2] = { { k_moment_splat<false, false>, k_moment_splat<false, true> }, { k_moment_splat<true, false>, k_moment_splat<true, true> } };
    return t[wide][alpha];
}
typedef decltype(&k_probe<PROBE_EMITTER>) ProbeFn;
static ProbeFn probe_kernel(ProbeKind kind) {                           // k_probe<KIND> (probes.h): one instance per row of kProbes
    static const ProbeFn t[PROBE_KINDS] = { k_probe<PROBE_EMITTER>, k_probe<PROBE_ENVMAP>, k_probe<PROBE_BSDF>, k_probe<PROBE_PHASE>, k_probe<PROBE_MEDIUM>, k_probe<PROBE_SENSOR> };
    return t[kind];
}

DeviceScene *device_scene_create(const lrt_scene_desc &d, int device) {
    select_device(device);
    std::unique_ptr<DeviceScene> D(new DeviceScene());
    D->device = device;
    HIP_CHECK(hipStreamCreateWithFlags(&D->stream, hipStreamNonBlocking));
    hipStream_t st = D->stream;
    // ---- the device: compute units, and the LDS a workgroup may ask for: the opt-in maximum (160 KiB on gfx950), minus the kernel's static __shared__ words
    PrepOptions opt = PrepOptions::from_env();
    hipDeviceProp_t prop; HIP_CHECK(hipGetDeviceProperties(&prop, device)); opt.n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    int optin = 0; if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, device) != hipSuccess || optin <= 0) optin = (int) prop.sharedMemPerBlock;
    (void) hipGetLastError();
    opt.lds_limit = std::min<size_t>((size_t) std::max(optin, 0), 160 * 1024) - 512;
    // ---- the scene's image on the host (scene_prep.cpp), in prepare_scene's two halves: the distance field is built on the device while the host
    // prepares the rest.  P outlives the copies below (the synchronize at the end); the device pointers are patched into its scene record.
    PreparedScene P; DScene &sc = P.sc;
    prepare_geometry(d, opt, P);
    D->n_cus = opt.n_cus; D->bvh_leaf = P.bvh_leaf; D->ext = P.ext; D->smooth_bsdf = P.smooth_bsdf;
    auto up = [&](const auto &v) { return D->track(dev_upload(v.data(), v.size(), st)); };
    sc.spheres = P.spheres.empty() ? nullptr : up(P.spheres);
    sc.nodes = (const float4 *) up(P.bvh.nodes);
    sc.tris = (const float4 *) up(P.bvh.tris);
    if (P.use_lds) {                                   // the LDS image: the kernels that copy it may ask for the whole limit
        D->lds = P.lds; D->lds.blob = (const uint4 *) up(P.lds_blob);
        const size_t lds_limit = opt.lds_limit;
        auto raise_lds = [&](const void *k) { if (k) HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_limit)); };
        const KernelTable &K = kernels();
        for (const RenderRow &r : K.render) if (r.lds && (!r.ext || D->ext)) raise_lds((const void *) r.fn);     // (the EXT instances: scenes with spheres / point emitters / mesh emitters only)
        for (const auto &adjoint : K.prb) for (const auto &ld : adjoint[1]) for (RenderFn fn : ld) raise_lds((const void *) fn);
        for (RenderFn fn : K.prb_grid[1]) raise_lds((const void *) fn);
        for (int i = 0; i < 2; ++i) for (int ext = 0; ext <= (D->ext ? 1 : 0); ++ext) {            // (i: k_aov's LD, k_trace_lds's ANY_HIT)
            raise_lds((const void *) aov_kernel(true, i, ext)); raise_lds((const void *) trace_lds_kernel(i, ext));
        }
        D->use_lds = true;
    }
    if (sc.grid.enabled) {                             // the conservative distance field over the slots and spheres just uploaded
        const size_t n_cells = (size_t) sc.grid.n[0] * sc.grid.n[1] * sc.grid.n[2];
        uint16_t *buf = nullptr; HIP_CHECK(hipMalloc((void **) &buf, n_cells * sizeof(uint16_t))); D->track(buf);
        k_build_dist_grid<<<(uint32_t) ((n_cells + LRT_BLOCK - 1) / LRT_BLOCK), LRT_BLOCK, 0, st>>>(sc.tris, d.n_faces ? (uint32_t) (P.bvh.tris.size() / 12) : 0u, sc.grid, buf, P.grid_abs_margin,
                                                                                             sc.spheres, sc.n_spheres);
        HIP_CHECK(hipGetLastError());
        sc.grid.d = buf;
    }
    prepare_shading(d, opt, P);
    D->has_area_emitter = P.has_area_emitter; D->has_het = P.has_het; D->has_non_bio = P.has_non_bio; D->prb_null = P.prb_null;
    sc.positions = D->track(dev_upload(d.positions, 3 * (size_t) d.n_vertices, st));
    sc.vattr = (const float4 *) up(P.vattr);
    sc.faces = D->track(dev_upload(d.faces, 3 * (size_t) d.n_faces, st));
    sc.face_shape = D->track(dev_upload(d.face_shape, d.n_faces, st));
    sc.shapes = up(P.shapes);
    sc.textures = up(P.textures);
    sc.tex_data = up(P.tex_data);
    sc.bsdfs = up(P.bsdfs);
    // ---- media: the tables are filled by upload_media, here and again after every parameter update
    HIP_CHECK(hipMalloc((void **) &D->d_media, std::max<uint32_t>(d.n_media, 1) * sizeof(DMedium))); D->track(D->d_media);
    HIP_CHECK(hipMalloc((void **) &D->d_bio, std::max<uint32_t>(d.n_media, 1) * sizeof(DBioMedium))); D->track(D->d_bio);
    HIP_CHECK(hipMalloc((void **) &D->d_het, std::max<uint32_t>(d.n_media, 1) * sizeof(DHetMedium))); D->track(D->d_het);
    D->het_data.assign(std::max<uint32_t>(d.n_media, 1), nullptr);
    for (uint32_t i = 0; i < d.n_media; ++i) {
        const lrt_medium_desc &M = d.media[i];
        if (M.type == LRT_MEDIUM_HETEROGENEOUS) D->het_data[i] = D->track(dev_upload(M.grid_data, (size_t) M.grid_res[0] * M.grid_res[1] * M.grid_res[2], st));
    }
    D->sc = sc;                                        // (upload_media reads the bounding sphere there)
    upload_media(D.get(), d); sc.media = D->d_media; sc.bio = D->d_bio; sc.het = D->d_het;
    sc.emitters = up(P.emitters);
    sc.mesh_emitters = up(P.mesh_emitters);
    sc.mesh_emitter_tab = up(P.mesh_emitter_tab);
    sc.delta_emitters = P.delta_emitters.empty() ? nullptr : up(P.delta_emitters);
    sc.bsdf_ext = P.bsdf_ext.empty() ? nullptr : up(P.bsdf_ext);
    sc.cone_tab = P.cone_tab.empty() ? nullptr : (const uint2 *) up(P.cone_tab);      // (sc.cone_enabled: set by the preparation with the table)
    sc.primary_tab = P.primary_tab.empty() ? nullptr : (const uint16_t *) up(P.primary_tab);      // (sc.primary_enabled alike; the preparation has validated every item)
    D->primary_tab = P.primary_tab;
    sc.phases = P.phases.empty() ? nullptr : up(P.phases);
    sc.phase_pool = P.phase_pool.empty() ? nullptr : up(P.phase_pool);
    sc.env_data = (const float4 *) up(P.env_data);
    sc.env_hier = up(P.env_hier);
    HIP_CHECK(hipMalloc((void **) &D->d_sc, sizeof(DScene))); D->track(D->d_sc);
    D->sc = sc;
    HIP_CHECK(hipMemcpyAsync(D->d_sc, &D->sc, sizeof(DScene), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMalloc((void **) &D->d_launch, LRT_LAUNCH_SLOTS * sizeof(DLaunch))); D->track(D->d_launch);
    HIP_CHECK(hipHostMalloc((void **) &D->h_launch, LRT_LAUNCH_SLOTS * sizeof(DLaunch)));
    HIP_CHECK(hipMalloc((void **) &D->counters, sizeof(DCounters))); D->track(D->counters);
    HIP_CHECK(hipHostMalloc((void **) &D->h_counters, sizeof(DCounters)));
    HIP_CHECK(hipStreamSynchronize(st));
    return D.release();
}

void device_scene_update_params(DeviceScene *D, const lrt_scene_desc &d, bool grids) {
    HIP_CHECK(hipSetDevice(D->device));
    if (grids) for (uint32_t i = 0; i < d.n_media; ++i) {         // "<id>.sigma_t.data": same resolution, new values (the description's copy outlives the sync below)
        const lrt_medium_desc &M = d.media[i];
        if (M.type == LRT_MEDIUM_HETEROGENEOUS && D->het_data[i])
            HIP_CHECK(hipMemcpyAsync(D->het_data[i], M.grid_data, (size_t) M.grid_res[0] * M.grid_res[1] * M.grid_res[2] * sizeof(float), hipMemcpyHostToDevice, D->stream));
    }
    upload_media(D, d);
    HIP_CHECK(hipStreamSynchronize(D->stream));
}

static void ensure_workspace(DeviceScene *D, uint32_t capacity) {
    const uint32_t layouts = workspace_layouts(D->has_het, D->need_mis);
    if (D->capacity >= capacity && D->ws_layouts == layouts) return;
    HIP_CHECK(hipStreamSynchronize(D->stream));
    // Exception safety: the old streams are released and every pointer cleared BEFORE anything is allocated, and capacity / ws_layouts are
    // set only after every allocation succeeded: a failed hipMalloc (out of memory) leaves capacity = 0, so the next render allocates again
    // instead of launching on freed memory.
    D->capacity = 0;
    // (a row's pointer inside a DPathStreams: the members are pointers of different types, so it is read and written as bytes)
    auto get = [](const DPathStreams *q, const RecordStream &r) { void *p; memcpy(&p, (const char *) q + r.member, sizeof p); return p; };
    auto set = [](DPathStreams *q, const RecordStream &r, void *p) { memcpy((char *) q + r.member, &p, sizeof p); };
    for (DPathStreams *q : { &D->q[0], &D->q[1] })
        for (const RecordStream &r : kRecordStreams) if (r.member != kNoMember) { D->release(get(q, r)); set(q, r, nullptr); }
    for (DPathStreams *q : { &D->q[0], &D->q[1] })             // one allocation per stream the layouts use, at its widest entry (rng: 16 bytes)
        for (size_t k = 0; k < std::size(kRecordStreams); ++k) if (const uint32_t bytes = workspace_stream_bytes(k, layouts)) {
            void *p = nullptr; HIP_CHECK(hipMalloc(&p, (size_t) capacity * bytes)); D->track(p); set(q, kRecordStreams[k], p);
        }
    D->capacity = capacity; D->ws_layouts = layouts;
}

static hipEvent_t get_event(DeviceScene *D, size_t i) {
    while (D->ev_pool.size() <= i) { hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); D->ev_pool.push_back(e); }
    return D->ev_pool[i];
}

// 32x32 pixel tiles in row-major tile order, tile k -> rank k % tile_count
static void ensure_pixel_list(DeviceScene *D, const ResolvedOpts &O) {
    const DFilm &F = D->sc.film;
    if (O.tile_count == 1) { D->n_owned_pixels = (uint32_t) F.width * F.height; return; }
    if (D->pixel_list && D->pixel_list_rank == O.tile_rank && D->pixel_list_count == O.tile_count) return;
    const TilePixels T = tile_pixel_list(F, O.tile_rank, O.tile_count);
    D->release(D->pixel_list); D->release(D->pixel_slot); D->pixel_list = nullptr; D->pixel_slot = nullptr;
    D->pixel_list = D->track(dev_upload(T.list.data(), T.list.size(), D->stream));
    D->pixel_slot = D->track(dev_upload(T.slot.data(), T.slot.size(), D->stream));
    D->pixel_list_rank = O.tile_rank; D->pixel_list_count = O.tile_count; D->n_owned_pixels = (uint32_t) T.list.size();
}

// The rank's tiles dilated by `halo` pixels (scene_prep.cpp, halo_pixel_list: the PRB weight film's lanes)
static void ensure_halo_list(DeviceScene *D, const ResolvedOpts &O, uint32_t halo) {
    const DFilm &F = D->sc.film;
    if (D->halo_list && D->halo_rank == O.tile_rank && D->halo_count == O.tile_count && D->halo_width == halo) return;
    const std::vector<uint32_t> px = halo_pixel_list(F, O.tile_rank, O.tile_count, halo);
    D->release(D->halo_list); D->halo_list = nullptr;
    D->halo_list = D->track(dev_upload(px.data(), px.size(), D->stream));
    D->halo_rank = O.tile_rank; D->halo_count = O.tile_count; D->halo_width = halo; D->n_halo_pixels = (uint32_t) px.size();
}

static void ensure_prb_workspace(DeviceScene *D, uint32_t records, uint64_t l_buf_lanes) {
    for (int k = 0; k < 2; ++k) D->grow(D->dl[k], D->dl_records[k], records);
    D->grow(D->L_buf, D->l_buf_lanes, l_buf_lanes);
    if (!D->d_grads) { HIP_CHECK(hipMalloc((void **) &D->d_grads, 7 * sizeof(double))); D->track(D->d_grads); }
}

static DRenderParams make_params(const lrt_scene_desc &d, const ResolvedOpts &O, uint64_t n_lanes) {
    DRenderParams rp{};
    rp.integrator = O.integrator; rp.max_depth = O.max_depth; rp.rr_depth = O.rr_depth; rp.hide_emitters = O.hide_emitters;
    rp.spp = O.spp; rp.log2_spp = ((O.spp & (O.spp - 1)) == 0) ? (uint32_t) __builtin_ctz(O.spp) : 0xffffffffu;
    rp.profile = getenv("LRT_DEBUG_LAUNCH") ? 1u : 0u;                 // bit 0: per-tile-kind timing, results unchanged
#ifdef LRT_EXPERIMENT
    if (getenv("LRT_EXP")) rp.profile |= (uint32_t) atoi(getenv("LRT_EXP"));   // cost-attribution switches (`make exp` build only)
    if (getenv("LRT_PRB_DEBUG_LANE")) rp.pad1 = (uint32_t) atoi(getenv("LRT_PRB_DEBUG_LANE")) + 1u;   // per-trip printf of one lane's PRB passes
#endif
    rp.seed_value = d.sampler_seed + O.seed; rp.base_seed = d.sampler_seed; rp.seed = O.seed;
    rp.ld_count = d.sampler_type == LRT_SAMPLER_LD ? O.spp_total : 0u; rp.pass_index = O.pass; rp.spp_total = O.spp_total; rp.tile_rank = O.tile_rank; rp.tile_count = O.tile_count; rp.n_lanes = n_lanes;
    return rp;
}

struct LaunchLog { std::vector<std::pair<hipEvent_t, hipEvent_t>> launches; std::vector<uint32_t> sizes; unsigned long long n_records = 0; size_t ev = 0; uint64_t n_iter = 0; };

static void finish_stats(DeviceScene *D, LaunchLog &log, hipEvent_t e_begin, hipEvent_t e_end, uint64_t n_lanes, lrt_render_stats &stats) {
    hipStream_t st = D->stream;
    HIP_CHECK(hipEventRecord(e_end, st));
    HIP_CHECK(hipMemcpyAsync(D->h_counters, D->counters, sizeof(DCounters), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    stats.n_samples = n_lanes; stats.n_iter = log.n_iter; stats.n_shadow = D->h_counters->n_shadow; stats.n_launches = log.launches.size();
    stats.n_records = log.n_records; if (!log.n_records) for (uint32_t n : log.sizes) stats.n_records += n;
    float ms = 0.f; double ksum = 0.0;
    for (size_t i = 0; i < log.launches.size(); ++i) {
        HIP_CHECK(hipEventElapsedTime(&ms, log.launches[i].first, log.launches[i].second)); ksum += ms;
        if (getenv("LRT_DEBUG_LAUNCH") && i < 40) {
            fprintf(stderr, "[lrt] launch %zu: %.3f ms\n", i, ms);
        }
    }
    stats.kernel_ms = ksum; stats.lds_resident = D->use_lds ? 1 : 0;
    if (getenv("LRT_DEBUG_LAUNCH")) for (int r = 0; r < 4; ++r) {
        fprintf(stderr, "[lrt] tile kind %d (0 proven-free, 1 query, 2 surface, 3 fresh): %llu tiles, %.1f ticks/tile (100 MHz wall clock)\n", r, D->h_counters->prof_tiles[r], D->h_counters->prof_tiles[r] ? (double) D->h_counters->prof_cycles[r] / D->h_counters->prof_tiles[r] : 0.0);
    }
    if (getenv("LRT_DEBUG_LAUNCH") && D->h_counters->prof_wg[1]) {
        const unsigned long long *w = D->h_counters->prof_wg; const double n_wg = D->use_lds ? D->n_cus : 4.0 * D->n_cus, first = (double) ~w[2];
        fprintf(stderr, "[lrt] workgroups (last launch; us): first start 0, last start %.1f, last end %.1f, mean run time %.1f, mean LDS-image copy %.1f, mean barrier wait per wave %.1f\n",
                ((double) w[5] - first) / 100.0, ((double) w[1] - first) / 100.0, (double) w[3] / n_wg / 100.0, (double) w[0] / n_wg / 100.0, (double) w[4] / (n_wg * (D->use_lds ? 16.0 : 4.0)) / 100.0);
    }
    HIP_CHECK(hipEventElapsedTime(&ms, e_begin, e_end)); stats.total_ms = ms;
}

// Geometry of the persistent kernels: one 1024-thread workgroup per CU when the BVH lives in LDS, else four 256-thread
// ones; P = paths in flight per workgroup (multiple of 64), queues of 2P records per workgroup.
struct PoolGeometry { uint32_t n_wg, P; size_t smem; };
static PoolGeometry pool_geometry(DeviceScene *D, uint64_t n_lanes) {
    PoolGeometry g;
    g.n_wg = D->use_lds ? (uint32_t) D->n_cus : 4u * (uint32_t) D->n_cus;
    const uint32_t pool_max = getenv("LRT_POOL") ? std::max(64, atoi(getenv("LRT_POOL"))) : (D->use_lds ? 32768u : 8192u);
    g.P = (uint32_t) std::min<uint64_t>(pool_max, std::max<uint64_t>(64, ((n_lanes + g.n_wg - 1) / g.n_wg + 63) / 64 * 64));
    // a launch with few lanes per workgroup (a rank's share of the frame at 8 GPUs: ~0.5 M) spends a visible part of its time
    // filling and draining the pool: pools of 8 K - 16 K paths were measured best for a 1/8 share of C3 (31.5 ms against 32.4 ms with the full pool): the pool follows the launch, about 48 turnovers per workgroup
    if (!getenv("LRT_POOL") && D->use_lds) {
        const uint64_t per_wg = (n_lanes + g.n_wg - 1) / g.n_wg, want = (per_wg / 48 + 63) / 64 * 64;
        if (want < g.P) g.P = (uint32_t) std::max<uint64_t>(want, std::min<uint64_t>(g.P, 8192));
    }
    g.smem = D->use_lds ? D->lds.total_bytes : (size_t) LRT_STACK * LRT_BLOCK * sizeof(int);
    return g;
}

// Copies the launch arguments into the next ring slot (stream-ordered) and returns the device pointer the kernel reads.
static LaunchPtr push_launch(DeviceScene *D, const DLaunch &a) {
    const uint32_t slot = D->launch_next++ % LRT_LAUNCH_SLOTS;
    if (slot == 0 && D->launch_next > 1) HIP_CHECK(hipStreamSynchronize(D->stream));    // the pinned source ring wraps: every earlier copy has been consumed
    D->h_launch[slot] = a;
    HIP_CHECK(hipMemcpyAsync(&D->d_launch[slot], &D->h_launch[slot], sizeof(DLaunch), hipMemcpyHostToDevice, D->stream));
    return (LaunchPtr) &D->d_launch[slot];
}

template <bool ADJOINT>
static void launch_prb(DeviceScene *D, const DRenderParams &rp, const PoolGeometry &g, const uint32_t *pixel_list, uint64_t lane_begin,
                       float4 *L_buf, const float *grad_image, double *grads, float *film, float *sample_out, float *dgrid = nullptr) {
    hipStream_t st = D->stream;
    HIP_CHECK(hipMemsetAsync(&D->counters->next_lane, 0, sizeof(unsigned long long), st));
    DLaunch a{}; a.rp = rp; a.li = D->lds; a.q0 = D->q[0]; a.q1 = D->q[1]; a.dl0 = D->dl[0]; a.dl1 = D->dl[1]; a.P = g.P; a.cnt = D->counters;
    a.pixel_list = pixel_list; a.lane_begin = lane_begin; a.n = rp.n_lanes; a.L_buf = L_buf; a.grad_image = grad_image; a.wfilm = D->wfilm; a.grads = grads;
    a.film = film; a.sample_out = sample_out; a.sample_base = lane_begin; a.dgrid = dgrid;
    const LaunchPtr lp = push_launch(D, a);             // (compact records, as run_wavefront queues them, were measured on C5: 96-byte records, 5 % SLOWER; the PRB kernels keep the wide layout)
    // ADJOINT && dgrid: lrt_render_backward_grid (the caller has checked that the graded medium is heterogeneous: prb_null)
    const bool ld = rp.ld_count != 0;
    const RenderFn fn = (ADJOINT && dgrid) ? kernels().prb_grid[D->use_lds][ld] : kernels().prb[ADJOINT][D->use_lds][ld][D->prb_null];
    if (!fn) throw std::runtime_error("developer build: volpath only");
    fn<<<g.n_wg, D->use_lds ? 1024 : LRT_BLOCK, g.smem, st>>>((ScenePtr) D->d_sc, lp);
    HIP_CHECK(hipGetLastError());
}

// Which media an integrator can meet: the bio integrators call the 5-argument Medium::sample_interaction, which the base class
// (homogeneous / heterogeneous media) answers with NotImplementedError (src/render/medium.cpp:83-90).
static void check_integrator_media(DeviceScene *D, int integrator) {
    if ((integrator == LRT_INTEGRATOR_BIOVOLPATH || integrator == LRT_INTEGRATOR_BIOVOLPATH06) && D->has_non_bio)
        throw std::runtime_error("NotImplementedError: sample_interaction (the bio integrators need liver / parenchyma / glissonCapsule media)");
    if (integrator == LRT_INTEGRATOR_PRBVOLPATH && D->smooth_bsdf)
        throw std::runtime_error("unsupported: prbvolpath on a scene with a conductor / plastic / twosided BSDF (no adjoint is built for them)");
    if (integrator == LRT_INTEGRATOR_PRBVOLPATH && D->ext)
        throw std::runtime_error("unsupported: prbvolpath on a scene with sphere shapes, point / spot / directional emitters, area emitters on meshes, a roughdielectric BSDF or a tabulated / Rayleigh / blended phase function (its adjoint is built for triangles, rectangle / infinite emitters, the diffuse / dielectric / null BSDFs and the isotropic / hg phase functions)");
    if (integrator == LRT_INTEGRATOR_VOLPATHMIS) D->need_mis = true;          // its wider path record is allocated on first use
}

// The render-kernel instance of a forward render: the row of kernels().render for an integrator on this scene.  compact / closed: run_wavefront's predicates.
static const RenderRow &select_render_kernel(int integrator, bool has_het, bool spectral_mis, bool lds, bool ld, bool ext, bool compact, bool closed) {
    int mode;
    switch (integrator) {
        case LRT_INTEGRATOR_PATH: case LRT_INTEGRATOR_BIOVOLPATH: case LRT_INTEGRATOR_BIOVOLPATH06: mode = integrator; break;
        case LRT_INTEGRATOR_VOLPATHMIS: mode = spectral_mis ? LRT_INTEGRATOR_VOLPATHMIS : LRT_INTEGRATOR_VOLPATHMIS_PLAIN; break;
        default: mode = closed ? LRT_INTEGRATOR_VOLPATH_CLOSED : (has_het ? LRT_INTEGRATOR_VOLPATH_HET : LRT_INTEGRATOR_VOLPATH);      // volpath
    }
    for (const RenderRow &r : kernels().render) if (r.mode == mode && r.lds == lds && r.ld == ld && r.compact == compact && r.ext == ext) return r;
    throw std::runtime_error("no render-kernel instance for mode " + std::to_string(mode) + (lds ? ", LDS BVH" : ", global BVH") + (ld ? ", ld sampler" : ", independent sampler") +
                             (compact ? ", compact records" : ", wide records") + (ext ? ", EXT" : ""));
}

// One persistent launch per render (k_render / k_render_prb): per-workgroup path pools, in-kernel regeneration; see
// kernels.h.  sample_out != nullptr: per-lane test hook for lanes [lane_begin, lane_begin + n_lanes).
static void run_wavefront(DeviceScene *D, const lrt_scene_desc &d, const ResolvedOpts &O, uint64_t lane_begin, uint64_t n_lanes,
                          const uint32_t *pixel_list, float *film, float *sample_out, lrt_render_stats &stats) {
    hipStream_t st = D->stream;
    DRenderParams rp = make_params(d, O, n_lanes);
    rp.pixel_slot = pixel_list ? D->pixel_slot : nullptr;
    rp.pass_in = D->cur_pass_in; rp.pass_out = D->cur_pass_out;
    const bool prb = O.integrator == LRT_INTEGRATOR_PRBVOLPATH;
    check_integrator_media(D, O.integrator);
    PoolGeometry g = pool_geometry(D, n_lanes);
    const uint32_t records = (uint32_t) std::min<uint64_t>((uint64_t) g.n_wg * 2u * g.P, 0xffffffffull);
    ensure_workspace(D, records);
    if (prb) ensure_prb_workspace(D, records, 0);
    HIP_CHECK(hipMemsetAsync(D->counters, 0, sizeof(DCounters), st));
    LaunchLog log;
    hipEvent_t e_begin = get_event(D, log.ev++), e_end = get_event(D, log.ev++);
    HIP_CHECK(hipEventRecord(e_begin, st));
    // path.cpp:103-104 returns before the loop when max_depth == 0: that launch only retires the lanes
    const bool count_iter = !(O.integrator == LRT_INTEGRATOR_PATH && O.max_depth == 0);
    hipEvent_t a = get_event(D, log.ev++), b = get_event(D, log.ev++);
    HIP_CHECK(hipEventRecord(a, st));
    if (prb) { stats.record_bytes = 0; launch_prb<false>(D, rp, g, pixel_list, lane_begin, nullptr, nullptr, nullptr, film, sample_out); }   // (not reported for the PRB kernels; not the last forward render's either)
    else {
        DLaunch a{}; a.rp = rp; a.li = D->lds; a.q0 = D->q[0]; a.q1 = D->q[1]; a.P = g.P; a.cnt = D->counters; a.pixel_list = pixel_list;
        a.lane_begin = lane_begin; a.n = n_lanes; a.film = film; a.sample_out = sample_out; a.sample_base = lane_begin;
        // Compact records (record_layout.h): only an area emitter's pdf reads the last scatter position, so a scene without one does not queue it.
        // Instances exist for the 1024-thread LDS kernels of path / volpath (homogeneous media) / biovolpath / biovolpath06.  LRT_WIDE_RECORDS: developer switch.
        const bool compact = D->use_lds && !D->has_area_emitter && !D->ext && !getenv("LRT_WIDE_RECORDS") && O.integrator != LRT_INTEGRATOR_VOLPATHMIS && !(O.integrator == LRT_INTEGRATOR_VOLPATH && D->has_het);
        // 64-byte records (volpath only; LRT_NO_CLOSED_RECORDS: developer switch back to the 80-byte layout): decided per render, since
        // lrt_param_set can change sigma_t after the scene was loaded
        const bool closed = compact && O.integrator == LRT_INTEGRATOR_VOLPATH && closed_records(d, D->sc.cam.medium) && !getenv("LRT_NO_CLOSED_RECORDS");
#ifdef LRT_DEV_VOLPATH_ONLY
        if (D->ext) throw std::runtime_error("developer build: no EXT instances (spheres / point emitters)");
        if (!(D->use_lds && (O.integrator == LRT_DEV_INTEGRATOR || (LRT_DEV_INTEGRATOR == LRT_INTEGRATOR_VOLPATH_HET && D->has_het)) && (rp.ld_count != 0) == LRT_DEV_LD)) throw std::runtime_error("developer build: one integrator / sampler / LDS BVH only");
#endif
        const RenderRow &row = select_render_kernel(O.integrator, D->has_het, d.use_spectral_mis != 0, D->use_lds, rp.ld_count != 0, D->ext, compact, closed);
        stats.record_bytes = row.record_bytes;
        const LaunchPtr lp = push_launch(D, a);
        row.fn<<<g.n_wg, row.block, g.smem, st>>>((ScenePtr) D->d_sc, lp);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(b, st));
    log.launches.emplace_back(a, b); log.sizes.push_back(0);
    HIP_CHECK(hipMemcpyAsync(D->h_counters, D->counters, sizeof(DCounters), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    log.n_iter = count_iter ? D->h_counters->n_iter : 0;
    log.n_records = D->h_counters->n_records;
    finish_stats(D, log, e_begin, e_end, n_lanes, stats);
    stats.n_closed_guard = D->h_counters->n_closed_guard;
    stats.n_proven = D->h_counters->n_proven;
    stats.n_primary_entry = D->h_counters->n_primary_entry;
    if (stats.n_closed_guard)
        throw std::runtime_error("64-byte path records: " + std::to_string(stats.n_closed_guard) + " trips broke the premise of the layout (radiance before a path's last trip, "
                                 "or an emitter hit that needs its MIS weight); the scene test in closed_records() is wrong for this scene: LRT_NO_CLOSED_RECORDS=1 renders it with 80-byte records");
}

// after_pass (the aov integrator with one nested integrator): called after each pass's colour work, while D->cur_pass_in still
// holds the sampler states at the start of that pass
// moment (the moment integrator, kernels_moment.h): the film has the moment channels, every filter takes the lane-buffer route and
// k_moment_splat / k_moment_develop stand in for k_splat_lanes / k_develop
static void render_passes(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, float *film_raw, float *image, lrt_render_stats &stats,
                          const std::function<void(const ResolvedOpts &)> &after_pass, bool moment = false);

void device_render(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, float *film_raw, float *image, lrt_render_stats &stats) {
    render_passes(D, d, opts, film_raw, image, stats, nullptr);
}

// The tail of a render: develops `film` (device) into the image and downloads what the caller asked for.  image / film_raw are host buffers
// (the image is developed into D->image first) unless on_device; film_raw == nullptr or == film: no film download.
static void develop_and_download(DeviceScene *D, const float *film, float *film_raw, float *image, size_t film_floats, size_t image_floats, bool on_device, bool moment = false) {
    const DFilm &F = D->sc.film; const size_t np = (size_t) F.width * F.height;
    if (image) {
        float *img = on_device ? image : D->grow(D->image, D->image_floats, image_floats);
        if (!moment) k_develop<<<(uint32_t) ((np + 255) / 256), 256, 0, D->stream>>>(F, film, img, (uint32_t) np);
        else if (F.has_alpha) k_moment_develop<true><<<(uint32_t) ((np + 255) / 256), 256, 0, D->stream>>>(film, img, (uint32_t) np);
        else k_moment_develop<false><<<(uint32_t) ((np + 255) / 256), 256, 0, D->stream>>>(film, img, (uint32_t) np);
        if (!on_device) HIP_CHECK(hipMemcpyAsync(image, img, image_floats * 4, hipMemcpyDeviceToHost, D->stream));
    }
    if (film_raw && !on_device) HIP_CHECK(hipMemcpyAsync(film_raw, film, film_floats * 4, hipMemcpyDeviceToHost, D->stream));
    HIP_CHECK(hipStreamSynchronize(D->stream));
    HIP_CHECK(hipGetLastError());
}

static void render_passes(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, float *film_raw, float *image, lrt_render_stats &stats,
                          const std::function<void(const ResolvedOpts &)> &after_pass, bool moment) {
    HIP_CHECK(hipSetDevice(D->device));
    ResolvedOpts O = resolve(d, opts);
    const DFilm &F = D->sc.film;
    bool on_device = opts && opts->output_on_device;
    const size_t film_channels = moment ? (F.has_alpha ? 11 : 10) : (size_t) F.channels, image_channels = moment ? film_channels - 1 : (F.has_alpha ? 4 : 3);
    size_t np = (size_t) F.width * F.height, film_floats = np * film_channels, image_floats = np * image_channels;
    ensure_pixel_list(D, O);
    const uint64_t n_lanes = (uint64_t) D->n_owned_pixels * O.spp;            // this rank's lanes of ONE pass
    float *film = (on_device && film_raw) ? film_raw : D->grow(D->film, D->film_floats, film_floats);
    HIP_CHECK(hipMemsetAsync(film, 0, film_floats * 4, D->stream));
    const uint32_t *pixel_list = O.tile_count > 1 ? D->pixel_list : nullptr;
    const bool carry = O.n_passes > 1 && d.sampler_type != LRT_SAMPLER_LD;     // the independent sampler's streams run on from pass to pass
    if (carry) for (int k = 0; k < 2; ++k) D->grow(D->pass_state[k], D->pass_state_lanes[k], n_lanes);
    const bool lane_splat = moment || (F.rfilter != LRT_RFILTER_BOX && (O.n_passes > 1 || !getenv("LRT_NO_LANE_SPLAT")));
    lrt_render_stats total{};
    for (uint32_t pass = 0; pass < O.n_passes; ++pass) {                       // integrator.cpp:343-353
        O.pass = pass;
        D->cur_pass_in = carry ? D->pass_state[pass & 1] : nullptr;
        D->cur_pass_out = (carry && pass + 1 < O.n_passes) ? D->pass_state[(pass & 1) ^ 1] : nullptr;
        if (!lane_splat) {
            lrt_render_stats st1{};
            run_wavefront(D, d, O, 0, n_lanes, pixel_list, film, nullptr, st1);
            add_stats(total, st1);
            if (after_pass) after_pass(O);
            continue;
        }
        // wide reconstruction filters: per-lane radiance first (16 B / lane, chunks of at most 2^28 lanes), then an in-order
        // splat pass that reduces each pixel's samples inside the wave (k_splat_lanes)
        const uint64_t chunk = std::min<uint64_t>(std::max<uint64_t>(n_lanes, 1), 1ull << 28);
        ensure_prb_workspace(D, 0, chunk);
        for (uint64_t base = 0; base < n_lanes; base += chunk) {
            const uint64_t n = std::min<uint64_t>(chunk, n_lanes - base);
            lrt_render_stats st1{};
            run_wavefront(D, d, O, base, n, pixel_list, nullptr, reinterpret_cast<float *>(D->L_buf), st1);
            DRenderParams rp = make_params(d, O, n); rp.pass_in = D->cur_pass_in;
            DLaunch a{}; a.rp = rp; a.L_buf = D->L_buf; a.pixel_list = pixel_list; a.lane_begin = base; a.n = n; a.film = film;
            const uint32_t grid = (uint32_t) ((n + LRT_BLOCK - 1) / LRT_BLOCK);
            const LaunchPtr lp = push_launch(D, a);
            if (!moment) k_splat_lanes<false><<<grid, LRT_BLOCK, 0, D->stream>>>((ScenePtr) D->d_sc, lp);
            else moment_splat_kernel(F.rfilter != LRT_RFILTER_BOX, F.has_alpha != 0)<<<grid, LRT_BLOCK, 0, D->stream>>>((ScenePtr) D->d_sc, lp);
            HIP_CHECK(hipGetLastError());
            add_stats(total, st1);
        }
        if (after_pass) after_pass(O);
    }
    D->cur_pass_in = nullptr; D->cur_pass_out = nullptr;
    total.lds_resident = D->use_lds ? 1 : 0;
    stats = total;
    develop_and_download(D, film, film_raw, image, film_floats, image_floats, on_device, moment);
}

// ------------------------------------------------------------------ the moment integrator (kernels_moment.h)
void device_render_moment(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, float *film_raw, float *image, lrt_render_stats &stats) {
    render_passes(D, d, opts, film_raw, image, stats, nullptr, true);
}

// lrt_render_samples' lanes, then moment_values per lane
void device_render_moment_samples(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out, lrt_render_stats &stats) {
    HIP_CHECK(hipSetDevice(D->device));
    ResolvedOpts O = resolve(d, opts);
    if (lane_begin + n > 0x100000000ull) throw std::runtime_error("lane range exceeds 2^32");
    if (!n) { stats = lrt_render_stats{}; return; }
    DevTmp buf((size_t) n * 10);                     // n float4 of radiance, then n * 6 floats of moments
    float *d_buf = buf.p, *d_m = d_buf + (size_t) n * 4;
    HIP_CHECK(hipMemsetAsync(d_buf, 0, (size_t) n * 16, D->stream));
    run_wavefront(D, d, O, lane_begin, n, nullptr, nullptr, d_buf, stats);
    k_moment_lanes<<<(n + 255u) / 256u, 256, 0, D->stream>>>(reinterpret_cast<const float4 *>(d_buf), O.integrator == LRT_INTEGRATOR_PATH ? 1 : 0, n, d_m);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, d_m, (size_t) n * 24, hipMemcpyDeviceToHost, D->stream));
    HIP_CHECK(hipStreamSynchronize(D->stream));
}

const std::vector<uint16_t> &device_primary_entry(const DeviceScene *D) { return D->primary_tab; }

void device_develop(DeviceScene *D, const float *film_raw, float *image, int on_device) {
    HIP_CHECK(hipSetDevice(D->device));
    const DFilm &F = D->sc.film;
    size_t np = (size_t) F.width * F.height, film_floats = np * F.channels, image_floats = np * (F.has_alpha ? 4 : 3);
    const float *film = film_raw;
    if (!on_device) {
        film = D->grow(D->film, D->film_floats, film_floats);
        HIP_CHECK(hipMemcpyAsync(D->film, film_raw, film_floats * 4, hipMemcpyHostToDevice, D->stream));
    }
    develop_and_download(D, film, nullptr, image, film_floats, image_floats, on_device != 0);
}

void device_render_samples(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out, lrt_render_stats &stats) {
    HIP_CHECK(hipSetDevice(D->device));
    ResolvedOpts O = resolve(d, opts);
    if (lane_begin + n > 0x100000000ull) throw std::runtime_error("lane range exceeds 2^32");
    DevTmp d_out((size_t) n * 4);
    HIP_CHECK(hipMemsetAsync(d_out.p, 0, (size_t) n * 16, D->stream));
    run_wavefront(D, d, O, lane_begin, n, nullptr, nullptr, d_out.p, stats);
    HIP_CHECK(hipMemcpyAsync(out, d_out.p, (size_t) n * 16, hipMemcpyDeviceToHost, D->stream));
    HIP_CHECK(hipStreamSynchronize(D->stream));
}

// ------------------------------------------------------------------ the aov integrator (kernels_aov.h)
// The AOV table and the shapes' first faces, uploaded (stream-ordered) before each aov render.
static void upload_aov_spec(DeviceScene *D, const lrt_scene_desc &d, const lrt_aov_desc &aov) {
    if (!D->d_aov_spec) { HIP_CHECK(hipMalloc((void **) &D->d_aov_spec, sizeof(DAovSpec))); D->track(D->d_aov_spec); }
    if (!D->d_first_face) {
        std::vector<uint32_t> ff(std::max<uint32_t>(d.n_shapes, 1), 0u);
        for (uint32_t i = 0; i < d.n_shapes; ++i) ff[i] = d.shapes[i].first_face;
        D->d_first_face = D->track(dev_upload(ff.data(), ff.size(), D->stream));
    }
    static thread_local DAovSpec h;              // the source of an asynchronous copy: outlives the call
    h = DAovSpec{}; h.n_aovs = aov.n_aovs; h.first_face = D->d_first_face;
    int off = 0;
    for (int k = 0; k < aov.n_aovs; ++k) {
        h.type[k] = aov.aov_types[k]; h.offset[k] = off;
        off += aov.aov_types[k] == LRT_AOV_DEPTH || aov.aov_types[k] >= LRT_AOV_PRIM_INDEX ? 1 : aov.aov_types[k] == LRT_AOV_UV ? 2 : 3;
    }
    h.n_ch = off;
    if (off != aov.n_aov_channels) throw std::runtime_error("aov: channel count mismatch");
    HIP_CHECK(hipMemcpyAsync(D->d_aov_spec, &h, sizeof(DAovSpec), hipMemcpyHostToDevice, D->stream));
    HIP_CHECK(hipStreamSynchronize(D->stream));
}

// One launch of k_aov over lanes [lane_begin, lane_begin + n) of pass O.pass: into `film`, or per lane into `sample_out`.
static void launch_aov(DeviceScene *D, const lrt_scene_desc &d, const ResolvedOpts &O, uint64_t lane_begin, uint64_t n, float *film, float *sample_out,
                       const unsigned long long *pass_in, unsigned long long *pass_out) {
    if (!n) return;
    hipStream_t st = D->stream;
    DRenderParams rp = make_params(d, O, n);
    rp.pass_in = pass_in; rp.pass_out = pass_out;
    DLaunch a{}; a.rp = rp; a.li = D->lds; a.lane_begin = lane_begin; a.n = n; a.film = film; a.sample_out = sample_out; a.sample_base = lane_begin;
    const LaunchPtr lp = push_launch(D, a);
    const AovSpecPtr spec = (AovSpecPtr) D->d_aov_spec;
    const AovFn fn = aov_kernel(D->use_lds, rp.ld_count != 0, D->ext);
    if (D->use_lds) {
        const uint32_t g = (uint32_t) std::min<uint64_t>((uint64_t) D->n_cus, (n + 1023) / 1024);       // one workgroup per CU: the LDS image is copied once
        fn<<<g, 1024, D->lds.total_bytes, st>>>((ScenePtr) D->d_sc, lp, spec);
    } else {
        const uint32_t g = (uint32_t) std::min<uint64_t>((uint64_t) D->n_cus * 8u, (n + LRT_BLOCK - 1) / LRT_BLOCK);
        fn<<<g, LRT_BLOCK, (size_t) LRT_STACK * LRT_BLOCK * sizeof(int), st>>>((ScenePtr) D->d_sc, lp, spec);
    }
    HIP_CHECK(hipGetLastError());
}

// The AOV pass renders like a (non-PRB) sampling integrator: its pass structure follows samples_per_pass and the 2^32 - 1 lane limit.
static ResolvedOpts resolve_aov(const lrt_scene_desc &d, const lrt_render_opts *opts, lrt_scene_desc &da) {
    da = d; da.integrator = lrt_integrator_desc{ LRT_INTEGRATOR_PATH, -1, 5, 0 };
    return resolve(da, opts);
}

void device_render_aov(DeviceScene *D, const lrt_scene_desc &d, const lrt_aov_desc &aov, const lrt_render_opts *opts, float *aov_film_raw, float *image, lrt_render_stats &stats) {
    HIP_CHECK(hipSetDevice(D->device));
    lrt_scene_desc da; ResolvedOpts O = resolve_aov(d, opts, da);
    if (O.tile_count > 1) throw std::runtime_error("lrt_render_aov: tile sharding is not supported");
    const DFilm &F = D->sc.film;
    const bool on_device = opts && opts->output_on_device;
    const size_t np = (size_t) F.width * F.height;
    const int C = aov.n_aov_channels + 1, T = aov.n_channels, IC = F.has_alpha ? 4 : 3, n_int = aov.n_integrators;
    // the independent sampler runs on from pass to pass, and its state after pass p - 1 includes what the nested integrators drew
    // (aov.cpp:348): one nested integrator -> that integrator's own pass states; none -> the AOV pass's; two or more -> no render here computes it
    const bool carry = O.n_passes > 1 && d.sampler_type != LRT_SAMPLER_LD;
    if (carry && n_int >= 2) throw std::runtime_error("lrt_render_aov: several passes of the independent sampler with two or more nested integrators are not supported");
    if (carry && n_int == 1 && aov.integrators[0].type == LRT_INTEGRATOR_PRBVOLPATH)
        throw std::runtime_error("lrt_render_aov: a nested prbvolpath renders in one pass; several AOV passes around it are not supported");
    upload_aov_spec(D, d, aov);
    hipStream_t st = D->stream;
    float *film = (on_device && aov_film_raw) ? aov_film_raw : D->grow(D->aov_film, D->aov_film_floats, np * C);
    HIP_CHECK(hipMemsetAsync(film, 0, np * C * 4, st));
    float *img = nullptr;
    if (image) img = on_device ? image : D->grow(D->aov_image, D->aov_image_floats, np * T);
    const uint64_t n_lanes = np * O.spp;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t ev_next = 0;
    auto aov_pass = [&](uint32_t pass, const unsigned long long *in, unsigned long long *out) {
        ResolvedOpts Op = O; Op.pass = pass;
        hipEvent_t a = get_event(D, ev_next++), b = get_event(D, ev_next++);
        HIP_CHECK(hipEventRecord(a, st));
        launch_aov(D, da, Op, 0, n_lanes, film, nullptr, in, out);
        HIP_CHECK(hipEventRecord(b, st));
        ev.emplace_back(a, b);
    };
    lrt_render_stats total{};
    bool aov_done = false;
    // 1. the nested integrators, each exactly as lrt_render renders it alone (aov.cpp:375-380)
    for (int k = 0; k < n_int; ++k) {
        const bool hook = carry && k == 0;
        if (!image && !hook) continue;           // nothing of it is asked for
        lrt_scene_desc dk = d; dk.integrator = aov.integrators[k];
        lrt_render_opts ok = opts ? *opts : default_opts();
        ok.output_on_device = 1; ok.tile_rank = 0; ok.tile_count = 1;
        float *inner = image ? D->grow(D->aov_inner, D->aov_inner_floats, np * IC) : nullptr;
        lrt_render_stats sk{};
        std::function<void(const ResolvedOpts &)> after;
        if (hook) after = [&](const ResolvedOpts &Oc) { aov_pass(Oc.pass, D->cur_pass_in, nullptr); };
        render_passes(D, dk, &ok, nullptr, inner, sk, after);
        if (hook) aov_done = true;
        if (image) { k_aov_copy<<<(uint32_t) ((np + 255) / 256), 256, 0, st>>>(inner, IC, img, T, k * IC, (uint32_t) np); HIP_CHECK(hipGetLastError()); }
        add_stats(total, sk);
    }
    // 2. the AOV pass (Base::render, aov.cpp:382-391)
    if (!aov_done) {
        if (carry) for (int k = 0; k < 2; ++k) D->grow(D->pass_state[k], D->pass_state_lanes[k], n_lanes);
        for (uint32_t pass = 0; pass < O.n_passes; ++pass)
            aov_pass(pass, carry ? D->pass_state[pass & 1] : nullptr, (carry && pass + 1 < O.n_passes) ? D->pass_state[(pass & 1) ^ 1] : nullptr);
    }
    // 3. merge (merge_channels, aov.cpp:523-545): the inner images are in place, the AOVs follow them
    if (img) { k_aov_develop<<<(uint32_t) ((np + 255) / 256), 256, 0, st>>>(film, C, img, T, n_int * IC, (uint32_t) np); HIP_CHECK(hipGetLastError()); }
    if (image && !on_device) HIP_CHECK(hipMemcpyAsync(image, img, np * T * 4, hipMemcpyDeviceToHost, st));
    if (aov_film_raw && !on_device) HIP_CHECK(hipMemcpyAsync(aov_film_raw, film, np * C * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    double aov_ms = 0.0;
    for (auto &e : ev) { float ms = 0.f; HIP_CHECK(hipEventElapsedTime(&ms, e.first, e.second)); aov_ms += ms; }
    total.n_samples += n_lanes * O.n_passes; total.n_launches += ev.size(); total.kernel_ms += aov_ms; total.total_ms += aov_ms;
    total.lds_resident = D->use_lds ? 1 : 0;
    stats = total;
}

void device_render_aov_samples(DeviceScene *D, const lrt_scene_desc &d, const lrt_aov_desc &aov, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out, lrt_render_stats &stats) {
    HIP_CHECK(hipSetDevice(D->device));
    lrt_scene_desc da; ResolvedOpts O = resolve_aov(d, opts, da);
    if (O.tile_count > 1) throw std::runtime_error("lrt_render_aov_samples: tile sharding is not supported");
    const uint64_t n_lanes = (uint64_t) D->sc.film.width * D->sc.film.height * O.spp;
    if (lane_begin + n > n_lanes) throw std::runtime_error("lrt_render_aov_samples: lane range exceeds the pass's " + std::to_string(n_lanes) + " lanes");
    upload_aov_spec(D, d, aov);
    const size_t floats = (size_t) n * aov.n_aov_channels;
    if (!floats) { stats = lrt_render_stats{}; return; }
    DevTmp d_out(floats);
    HIP_CHECK(hipMemsetAsync(d_out.p, 0, floats * 4, D->stream));
    O.pass = 0;
    launch_aov(D, da, O, lane_begin, n, nullptr, d_out.p, nullptr, nullptr);
    HIP_CHECK(hipMemcpyAsync(out, d_out.p, floats * 4, hipMemcpyDeviceToHost, D->stream));
    HIP_CHECK(hipStreamSynchronize(D->stream));
    HIP_CHECK(hipGetLastError());
    stats = lrt_render_stats{}; stats.n_samples = n; stats.lds_resident = D->use_lds ? 1 : 0;
}

void device_trace(DeviceScene *D, const lrt_rays_soa *rays, const lrt_hits_soa *hits, uint32_t n, int any_hit) {
    HIP_CHECK(hipSetDevice(D->device));
    hipStream_t st = D->stream;
    DevTmp in[7], res[4];                           // origin, direction, tmax; t, u, v, prim
    const float *src[7] = { rays->ox, rays->oy, rays->oz, rays->dx, rays->dy, rays->dz, rays->tmax };
    for (int k = 0; k < 7; ++k) in[k].upload(src[k], n, st);
    for (DevTmp &r : res) r.alloc(n);
    float *t = res[0].p, *u = res[1].p, *v = res[2].p; uint32_t *prim = (uint32_t *) res[3].p;
    if (n && D->use_lds) {                          // the render kernels' tracer: BVH image in LDS
        const uint32_t g = std::min<uint32_t>((uint32_t) D->n_cus, (n + 1023) / 1024);
        trace_lds_kernel(any_hit != 0, D->ext)<<<g, 1024, D->lds.total_bytes, st>>>((ScenePtr) D->d_sc, D->lds, in[0].p, in[1].p, in[2].p, in[3].p, in[4].p, in[5].p, in[6].p, t, u, v, prim, n);
    } else if (n)
        trace_kernel(any_hit != 0, D->ext)<<<(n + LRT_BLOCK - 1) / LRT_BLOCK, LRT_BLOCK, 0, st>>>((ScenePtr) D->d_sc, in[0].p, in[1].p, in[2].p, in[3].p, in[4].p, in[5].p, in[6].p, t, u, v, prim, n);
    HIP_CHECK(hipMemcpyAsync(hits->t, t, (size_t) n * 4, hipMemcpyDeviceToHost, st));
    if (!any_hit) {
        if (hits->u) HIP_CHECK(hipMemcpyAsync(hits->u, u, (size_t) n * 4, hipMemcpyDeviceToHost, st));
        if (hits->v) HIP_CHECK(hipMemcpyAsync(hits->v, v, (size_t) n * 4, hipMemcpyDeviceToHost, st));
        if (hits->prim) HIP_CHECK(hipMemcpyAsync(hits->prim, prim, (size_t) n * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
}

} // namespace lrt

namespace lrt {

// RBIntegrator.render_backward (common.py:625-783): weight film (non-box filters) -> per chunk: primal pass into L_buf,
// adjoint replay accumulating d(sum(image * grad_image)) / d(sigma_t, albedo, g) into 7 doubles.
// d_grid != null (lrt_render_backward_grid): the adjoint pass is k_render_prb_grid, which also scatters d / d(grid values) of the
// heterogeneous medium opts->grad_medium into a zeroed buffer of res_x * res_y * res_z floats (float atomics: last bits vary from run to run).
void device_render_backward(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, const float *grad_image, lrt_param_grads *out, lrt_render_stats &stats, float *d_grid) {
    HIP_CHECK(hipSetDevice(D->device));
    lrt_render_opts oprb = opts ? *opts : default_opts();
    oprb.integrator = LRT_INTEGRATOR_PRBVOLPATH;                               // resolve as the adjoint integrator: RBIntegrator.render_backward has no pass split (common.py prepare())
    ResolvedOpts O = resolve(d, &oprb);
    check_integrator_media(D, LRT_INTEGRATOR_PRBVOLPATH);
    const int grad_medium = opts ? opts->grad_medium : 0;
    if (grad_medium < -1 || grad_medium >= (int) d.n_media) throw std::runtime_error("lrt_render_backward: grad_medium " + std::to_string(grad_medium) + " is not a medium of the scene");
    hipStream_t st = D->stream;
    float *dg = nullptr; size_t n_vox = 0;
    if (d_grid) {
        if (grad_medium < 0 || d.media[grad_medium].type != LRT_MEDIUM_HETEROGENEOUS)
            throw std::invalid_argument("lrt_render_backward_grid: grad_medium " + std::to_string(grad_medium) + " is not a heterogeneous medium (the grid gradient belongs to one medium with a sigma_t grid)");
        if (!D->prb_null) throw std::runtime_error("unsupported: lrt_render_backward_grid on a heterogeneous medium that is attached to no shape");
        const lrt_medium_desc &M = d.media[grad_medium];
        n_vox = (size_t) M.grid_res[0] * M.grid_res[1] * M.grid_res[2];
        if (opts && opts->output_on_device) dg = d_grid;
        else dg = D->grow(D->dgrid, D->dgrid_floats, n_vox);
    }
    const DFilm &F = D->sc.film;
    const size_t np = (size_t) F.width * F.height, T = F.has_alpha ? 4 : 3;
    if ((uint64_t) np * O.spp > 0xffffffffull) throw std::runtime_error("more than 2^32 samples per render");
    ensure_pixel_list(D, O);
    const uint64_t n_lanes = (uint64_t) D->n_owned_pixels * O.spp;
    const uint32_t *pixel_list = O.tile_count > 1 ? D->pixel_list : nullptr;
    DRenderParams rp = make_params(d, O, n_lanes);
    rp.grad_medium = grad_medium;
    // primal radiance of every lane of a pass is kept (16 B / lane); passes of at most 2^28 lanes bound that buffer to 4.3 GB
    const uint64_t pass = std::min<uint64_t>(std::max<uint64_t>(n_lanes, 1), 1ull << 28);
    PoolGeometry g = pool_geometry(D, pass);
    const uint32_t records = (uint32_t) std::min<uint64_t>((uint64_t) g.n_wg * 2u * g.P, 0xffffffffull);
    ensure_workspace(D, records); ensure_prb_workspace(D, records, pass);
    const float *g_img = grad_image;
    if (!(opts && opts->output_on_device)) {
        g_img = D->grow(D->grad_image, D->grad_floats, np * T);
        HIP_CHECK(hipMemcpyAsync(D->grad_image, grad_image, np * T * 4, hipMemcpyHostToDevice, st));
    }
    if (F.rfilter != LRT_RFILTER_BOX) {
        D->grow(D->wfilm, D->wfilm_floats, np);
        HIP_CHECK(hipMemsetAsync(D->wfilm, 0, np * 4, st));
        // sum of reconstruction-filter weights per pixel: over every lane of the image, or (tile-sharded) over the lanes of the rank's
        // tiles dilated by 2 fn pixels, which completes the sums at every pixel the rank's own footprints read (ensure_halo_list)
        const uint32_t *wlist = nullptr; uint64_t all = (uint64_t) np * O.spp;
        if (O.tile_count > 1) { ensure_halo_list(D, O, 2u * (uint32_t) F.fn); wlist = D->halo_list; all = (uint64_t) D->n_halo_pixels * O.spp; }
        DRenderParams rw = make_params(d, O, all);
        for (uint64_t base = 0; base < all; base += (1ull << 30)) {
            const uint64_t n = std::min<uint64_t>(1ull << 30, all - base);
            DLaunch a{}; a.rp = rw; a.lane_begin = base; a.n = n; a.film = D->wfilm; a.pixel_list = wlist;
            k_splat_lanes<true><<<(uint32_t) ((n + LRT_BLOCK - 1) / LRT_BLOCK), LRT_BLOCK, 0, st>>>((ScenePtr) D->d_sc, push_launch(D, a));
        }
    }
    HIP_CHECK(hipMemsetAsync(D->d_grads, 0, 7 * sizeof(double), st));
    if (dg) HIP_CHECK(hipMemsetAsync(dg, 0, n_vox * 4, st));
    HIP_CHECK(hipMemsetAsync(D->counters, 0, sizeof(DCounters), st));
    LaunchLog log;
    hipEvent_t e_begin = get_event(D, log.ev++), e_end = get_event(D, log.ev++);
    HIP_CHECK(hipEventRecord(e_begin, st));
    for (uint64_t base = 0; base < n_lanes; base += pass) {
        rp.n_lanes = std::min<uint64_t>(pass, n_lanes - base);
        for (int adjoint = 0; adjoint < 2; ++adjoint) {
            hipEvent_t a = get_event(D, log.ev++), b = get_event(D, log.ev++);
            HIP_CHECK(hipEventRecord(a, st));
            if (!adjoint) launch_prb<false>(D, rp, g, pixel_list, base, D->L_buf, nullptr, nullptr, nullptr, nullptr);
            else launch_prb<true>(D, rp, g, pixel_list, base, D->L_buf, g_img, D->d_grads, nullptr, nullptr, dg);
            HIP_CHECK(hipEventRecord(b, st));
            log.launches.emplace_back(a, b); log.sizes.push_back(0);
        }
    }
    HIP_CHECK(hipMemcpyAsync(D->h_counters, D->counters, sizeof(DCounters), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    log.n_iter = D->h_counters->n_iter; log.n_records = D->h_counters->n_records;
    finish_stats(D, log, e_begin, e_end, n_lanes, stats); stats.record_bytes = 0;
    double h[7];
    HIP_CHECK(hipMemcpy(h, D->d_grads, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k) { out->d_sigma_t[k] = (float) h[k]; out->d_albedo[k] = (float) h[3 + k]; }
    out->d_g = (float) h[6];
    if (dg && dg != d_grid) HIP_CHECK(hipMemcpy(d_grid, dg, n_vox * 4, hipMemcpyDeviceToHost));
}

// ---- learned subsurface model, network stage (include/liverrt.h; one lane per sample, weights through the scalar cache)
void device_vae_scatter(const float *blob, uint32_t n, const float *in_pos, const float *in_dir, const float *poly, const float albedo[3], float g, float ior,
                        const float sigma_t[3], float fit_scale, uint32_t seed, float *out_pos, float *out_absorption, int device) {
    select_device(device);
    if (n == 0) return;
    // the medium-level features are the same for every sample: evaluated once, on the device (one thread), with the kernels' own log / exp
    DevTmp d_blob(LRT_VAE_N_FLOATS), d_pos(3 * (size_t) n), d_dir(3 * (size_t) n), d_poly(20 * (size_t) n), d_opos(3 * (size_t) n), d_oabs(n), d_feat(4);
    auto up = [&](DevTmp &t, const float *src, size_t cnt) { HIP_CHECK(hipMemcpy(t.p, src, cnt * sizeof(float), hipMemcpyHostToDevice)); };
    up(d_blob, blob, LRT_VAE_N_FLOATS); up(d_pos, in_pos, 3 * (size_t) n); up(d_dir, in_dir, 3 * (size_t) n); up(d_poly, poly, 20 * (size_t) n);
    k_vae_medium_features<<<1, 1>>>(d_blob.p, albedo[0], albedo[1], albedo[2], g, ior, sigma_t[0], sigma_t[1], sigma_t[2], d_feat.p);
    HIP_CHECK(hipGetLastError());
    float feat[4]; HIP_CHECK(hipMemcpy(feat, d_feat.p, sizeof feat, hipMemcpyDeviceToHost));
    DVaeArgs A{}; A.blob = d_blob.p; A.in_pos = d_pos.p; A.in_dir = d_dir.p; A.poly = d_poly.p; A.out_pos = d_opos.p; A.out_absorption = d_oabs.p;
    A.albedo_norm = feat[0]; A.g_norm = feat[1]; A.ior_norm = feat[2]; A.fit_scale = fit_scale; A.n = n; A.seed = seed;
    const size_t smem = (size_t) 2 * 68 * LRT_VAE_BLOCK * sizeof(float);
    HIP_CHECK(hipFuncSetAttribute((const void *) k_vae_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int) smem));
    k_vae_scatter<<<(n + LRT_VAE_BLOCK - 1) / LRT_VAE_BLOCK, LRT_VAE_BLOCK, smem>>>(A);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(out_pos, d_opos.p, 3 * (size_t) n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_absorption, d_oabs.p, (size_t) n * sizeof(float), hipMemcpyDeviceToHost));
}

// ------------------------------------------------------------------ one process, several devices (include/liverrt.h: lrt_render_multi)
// SURVEY.md 8e through the C ABI: device i renders the 32x32 tiles t with t % N == i into its own full-size zeroed film (global lane
// ids), ONE ncclAllReduce (RCCL over xGMI, sum, f32, H*W*C) merges the films, device 0 develops.  One host thread and one stream per
// device.  RCCL is bound at run time from /opt/rocm/lib/librccl.so (LRT_RCCL_LIBRARY overrides): the library that matches the HIP
// runtime libliverrt.so links, whatever copy another framework in the process carries.
struct Rccl {
    void *h = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr; ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    void load() {
        if (h) return;
        const char *env = getenv("LRT_RCCL_LIBRARY");
        for (const char *name : { env ? env : "/opt/rocm/lib/librccl.so", "librccl.so.1", "librccl.so" }) { h = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (h) break; }
        if (!h) throw std::runtime_error(std::string("hip: cannot load librccl.so (") + (dlerror() ? dlerror() : "?") + "); lrt_render_multi on distinct devices needs RCCL");
        auto sym = [&](const char *n) { void *p = dlsym(h, n); if (!p) throw std::runtime_error(std::string("hip: librccl.so lacks ") + n); return p; };
        CommInitAll = (decltype(CommInitAll)) sym("ncclCommInitAll"); AllReduce = (decltype(AllReduce)) sym("ncclAllReduce");
        GroupStart = (decltype(GroupStart)) sym("ncclGroupStart"); GroupEnd = (decltype(GroupEnd)) sym("ncclGroupEnd");
        CommDestroy = (decltype(CommDestroy)) sym("ncclCommDestroy"); GetErrorString = (decltype(GetErrorString)) sym("ncclGetErrorString");
    }
    void check(ncclResult_t r, const char *what) { if (r != ncclSuccess) throw std::runtime_error(std::string("hip: rccl ") + what + ": " + (GetErrorString ? GetErrorString(r) : "error")); }
};
static Rccl g_rccl;

struct MultiContext {                     // the communicators of one device list (ncclCommInitAll takes about a second: kept with the scene)
    std::vector<int> devices; std::vector<ncclComm_t> comms;
    ~MultiContext() { for (auto c : comms) if (c && g_rccl.CommDestroy) (void) g_rccl.CommDestroy(c); }
};
void multi_context_destroy(MultiContext *m) { delete m; }

__global__ void k_film_add(float *__restrict__ dst, const float *__restrict__ src, size_t n) {
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

// Sums buf[i] (`count` floats or doubles on device i, stream of device i) over the devices, in place.  Distinct devices: one grouped
// ncclAllReduce.  The same device named several times (a rehearsal on a one-GPU box): the peers share the device, so rank 0's buffer
// takes the others' with a kernel and nothing crosses a link.
template <typename T>
static void reduce_across(std::vector<DeviceScene *> &devs, MultiContext *&ctx, std::vector<T *> &buf, size_t count) {
    const int N = (int) devs.size();
    bool distinct = true;
    for (int i = 0; i < N; ++i) for (int j = 0; j < i; ++j) if (devs[i]->device == devs[j]->device) distinct = false;
    for (auto *D : devs) { HIP_CHECK(hipSetDevice(D->device)); HIP_CHECK(hipStreamSynchronize(D->stream)); }
    if (distinct) {
        g_rccl.load();
        std::vector<int> ids; for (auto *D : devs) ids.push_back(D->device);
        if (!ctx || ctx->devices != ids) {
            delete ctx; ctx = new MultiContext(); ctx->devices = ids; ctx->comms.assign(N, nullptr);
            g_rccl.check(g_rccl.CommInitAll(ctx->comms.data(), N, ids.data()), "ncclCommInitAll");
        }
        g_rccl.check(g_rccl.GroupStart(), "ncclGroupStart");
        for (int i = 0; i < N; ++i) {
            HIP_CHECK(hipSetDevice(devs[i]->device));
            g_rccl.check(g_rccl.AllReduce(buf[i], buf[i], count, sizeof(T) == 8 ? ncclDouble : ncclFloat, ncclSum, ctx->comms[i], devs[i]->stream), "ncclAllReduce");
        }
        g_rccl.check(g_rccl.GroupEnd(), "ncclGroupEnd");
        for (auto *D : devs) { HIP_CHECK(hipSetDevice(D->device)); HIP_CHECK(hipStreamSynchronize(D->stream)); }
    } else {
        for (int i = 1; i < N; ++i) if (devs[i]->device != devs[0]->device) throw std::runtime_error("lrt_render_multi: a device list is either all distinct or one device repeated");
        static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
        HIP_CHECK(hipSetDevice(devs[0]->device));
        for (int i = 1; i < N; ++i) {
            if (sizeof(T) == 4) k_film_add<<<(uint32_t) ((count + 255) / 256), 256, 0, devs[0]->stream>>>((float *) buf[0], (const float *) buf[i], count);
            else { std::vector<double> a(count), b(count); HIP_CHECK(hipMemcpy(a.data(), buf[0], count * 8, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(b.data(), buf[i], count * 8, hipMemcpyDeviceToHost));
                   for (size_t k = 0; k < count; ++k) a[k] += b[k]; HIP_CHECK(hipMemcpy(buf[0], a.data(), count * 8, hipMemcpyHostToDevice)); }
        }
        HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(devs[0]->stream));
    }
}

template <typename F> static void on_every_device(size_t n, F fn) {
    std::vector<std::exception_ptr> err(n);
    std::vector<std::thread> th;
    for (size_t i = 0; i < n; ++i) th.emplace_back([&, i]() { try { fn(i); } catch (...) { err[i] = std::current_exception(); } });
    for (auto &t : th) t.join();
    for (auto &e : err) if (e) std::rethrow_exception(e);
}

void device_render_multi(std::vector<DeviceScene *> &devs, MultiContext *&ctx, const lrt_scene_desc &d, const lrt_render_opts *opts, float *film_raw, float *image, lrt_render_stats &stats) {
    const int N = (int) devs.size();
    const DFilm &F = devs[0]->sc.film;
    const size_t np = (size_t) F.width * F.height, film_floats = np * F.channels, image_floats = np * (F.has_alpha ? 4 : 3);
    const bool on_device = opts && opts->output_on_device;                     // film_raw / image then live on the FIRST device of the list
    std::vector<float *> films(N); std::vector<lrt_render_stats> st(N);
    const auto t0 = std::chrono::steady_clock::now();
    on_every_device(N, [&](size_t i) {
        HIP_CHECK(hipSetDevice(devs[i]->device));
        films[i] = (i == 0 && on_device && film_raw) ? film_raw : devs[i]->grow(devs[i]->film, devs[i]->film_floats, film_floats);
        lrt_render_opts o = opts ? *opts : default_opts();
        o.tile_rank = (uint32_t) i; o.tile_count = (uint32_t) N; o.device = devs[i]->device; o.output_on_device = 1;
        device_render(devs[i], d, &o, films[i], nullptr, st[i]);
    });
    if (N > 1 || getenv("LRT_MULTI_ALWAYS_REDUCE")) reduce_across(devs, ctx, films, film_floats);
    DeviceScene *D0 = devs[0];
    HIP_CHECK(hipSetDevice(D0->device));
    develop_and_download(D0, films[0], film_raw, image, film_floats, image_floats, on_device);
    lrt_render_stats total{};
    for (auto &x : st) { total.n_samples += x.n_samples; total.n_iter += x.n_iter; total.n_shadow += x.n_shadow; total.n_launches += x.n_launches; total.n_records += x.n_records;
                         total.kernel_ms = std::max(total.kernel_ms, x.kernel_ms); total.lds_resident = x.lds_resident; total.record_bytes = x.record_bytes; total.n_closed_guard += x.n_closed_guard; total.n_proven += x.n_proven; total.n_primary_entry += x.n_primary_entry; }
    total.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats = total;
}

void device_render_backward_multi(std::vector<DeviceScene *> &devs, MultiContext *&ctx, const lrt_scene_desc &d, const lrt_render_opts *opts, const float *grad_image, lrt_param_grads *out, lrt_render_stats &stats) {
    const int N = (int) devs.size();
    if (opts && opts->output_on_device) throw std::runtime_error("lrt_render_backward_multi: grad_image is a host buffer (every device takes its own copy)");
    std::vector<lrt_param_grads> g(N); std::vector<lrt_render_stats> st(N);
    on_every_device(N, [&](size_t i) {
        lrt_render_opts o = opts ? *opts : default_opts();
        o.tile_rank = (uint32_t) i; o.tile_count = (uint32_t) N; o.device = devs[i]->device; o.output_on_device = 0;
        device_render_backward(devs[i], d, &o, grad_image, &g[i], st[i]);
    });
    // the 7 gradient doubles of every device (still in its d_grads) are reduced like the film: one all-reduce
    std::vector<double *> bufs; for (auto *D : devs) bufs.push_back(D->d_grads);
    if (N > 1) reduce_across(devs, ctx, bufs, 7);
    double h[7]; HIP_CHECK(hipSetDevice(devs[0]->device)); HIP_CHECK(hipMemcpy(h, devs[0]->d_grads, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k) { out->d_sigma_t[k] = (float) h[k]; out->d_albedo[k] = (float) h[3 + k]; }
    out->d_g = (float) h[6];
    lrt_render_stats total{};
    for (auto &x : st) { total.n_samples += x.n_samples; total.n_iter += x.n_iter; total.n_shadow += x.n_shadow; total.n_launches += x.n_launches; total.n_records += x.n_records;
                         total.kernel_ms = std::max(total.kernel_ms, x.kernel_ms); total.total_ms = std::max(total.total_ms, x.total_ms); total.lds_resident = x.lds_resident; }
    stats = total;
}

// Test hooks (include/liverrt.h lrt_*_probe; probes.h): probe `kind` on the scene's device image, `n` lanes.  `columns` are the caller's
// input arrays in the order of the kind's lane record; they are packed into lane records here and uploaded once.  arg: kProbes' note.
void device_probe(DeviceScene *D, ProbeKind kind, int arg, std::initializer_list<ProbeColumn> columns, uint32_t n, float *out) {
    const ProbeRow &P = kProbes[kind];
    HIP_CHECK(hipSetDevice(D->device));
    if (P.needs_env && D->sc.env.emitter < 0) throw std::runtime_error(std::string(P.name) + ": the scene has no environment emitter");
    if (!n) return;
    int width = 0; for (const ProbeColumn &c : columns) width += c.width;
    if (width != P.in) throw std::logic_error(std::string(P.name) + ": the columns do not add up to the lane record");
    std::vector<float> packed((size_t) n * P.in);            // (lives until the synchronise below: the upload reads it asynchronously)
    int at = 0;
    for (const ProbeColumn &c : columns) {
        for (size_t i = 0; i < n; ++i) std::copy_n(c.p + i * c.width, c.width, packed.data() + i * P.in + at);
        at += c.width;
    }
    hipStream_t st = D->stream;
    DevTmp in, dout((size_t) n * P.out);
    in.upload(packed.data(), packed.size(), st);
    probe_kernel(kind)<<<(n + LRT_BLOCK - 1) / LRT_BLOCK, LRT_BLOCK, 0, st>>>((ScenePtr) D->d_sc, arg, in.p, n, dout.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, dout.p, (size_t) n * P.out * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

// Test hook (include/liverrt.h lrt_math_eval): the transcendental kernels of csrc/dmath.h evaluated on the device, one lane per value.
// orc_math.h holds the same polynomials written a second time, so bit-equality of the render lanes says nothing about their accuracy:
// tests/test_parity_gpu.py bounds the DEVICE values against float64 and checks them bit for bit against the oracle's twins.
__global__ void k_math_eval(int fn, const float *__restrict__ x, const float *__restrict__ y, uint32_t n, float *__restrict__ out, float *__restrict__ out2) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = 0.f, b = 0.f;
    switch (fn) {
        case 0: a = m_log(x[i]); break;
        case 1: a = m_exp(x[i]); break;
        case 2: m_sincos(x[i], &a, &b); break;
        case 3: a = m_atan2(y[i], x[i]); break;
        case 4: a = m_acos(x[i]); break;
        case 5: a = m_log2(x[i]); break;
        case 6: a = x[i] / y[i]; break;
        case 7: a = __builtin_sqrtf(x[i]); break;
        case 8: a = rcp(x[i]); break;
        case 9: a = m_erf(x[i]); break;
        case 10: a = m_erfinv(x[i]); break;
        case 11: a = m_cbrt(x[i]); break;
        default: break;
    }
    out[i] = a; out2[i] = b;
}
void device_math_eval(int fn, const float *x, const float *y, uint32_t n, float *out, float *out2, int device) {
    select_device(device);
    if (fn < 0 || fn > 11) throw std::invalid_argument("lrt_math_eval: function 0 .. 11");
    if (!n) return;
    DevTmp dx(n), dy(n), d1(n), d2(n);
    HIP_CHECK(hipMemcpy(dx.p, x, (size_t) n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dy.p, y ? y : x, (size_t) n * 4, hipMemcpyHostToDevice));
    k_math_eval<<<(n + 255) / 256, 256>>>(fn, dx.p, dy.p, n, d1.p, d2.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(out, d1.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    if (out2) HIP_CHECK(hipMemcpy(out2, d2.p, (size_t) n * 4, hipMemcpyDeviceToHost));
}

// ---- guided denoiser (kernels_denoise.h)
struct Denoiser {
    int device = 0, w = 0, h = 0;
    bool alb = false, nrm = false, alpha = false;
    lrt_denoise_params prm{};
    hipStream_t stream = nullptr;
    float4 *colour[2] = { nullptr, nullptr }, *g_normal = nullptr, *g_albedo = nullptr;     // packed planes, ping-pong colour
    float *s_noisy = nullptr, *s_albedo = nullptr, *s_normals = nullptr, *s_out = nullptr;  // staging for host pointers
    ~Denoiser() {
        (void) hipSetDevice(device);
        if (stream) (void) hipStreamSynchronize(stream);
        for (void *p : { (void *) colour[0], (void *) colour[1], (void *) g_normal, (void *) g_albedo, (void *) s_noisy, (void *) s_albedo, (void *) s_normals, (void *) s_out })
            if (p) (void) hipFree(p);
        if (stream) (void) hipStreamDestroy(stream);
    }
};

Denoiser *denoiser_create(int width, int height, bool use_albedo, bool use_normals, bool denoise_alpha, const lrt_denoise_params &params, int device) {
    select_device(device);
    Denoiser *D = new Denoiser();
    try {
        D->device = device; D->w = width; D->h = height; D->alb = use_albedo; D->nrm = use_normals; D->alpha = denoise_alpha; D->prm = params;
        HIP_CHECK(hipStreamCreateWithFlags(&D->stream, hipStreamNonBlocking));
        size_t np = (size_t) width * height;
        for (int k = 0; k < 2; ++k) HIP_CHECK(hipMalloc((void **) &D->colour[k], np * 16));
        if (use_normals) { HIP_CHECK(hipMalloc((void **) &D->g_normal, np * 16)); HIP_CHECK(hipMalloc((void **) &D->s_normals, np * 12)); }
        if (use_albedo)  { HIP_CHECK(hipMalloc((void **) &D->g_albedo, np * 16)); HIP_CHECK(hipMalloc((void **) &D->s_albedo, np * 12)); }
        HIP_CHECK(hipMalloc((void **) &D->s_noisy, np * 16)); HIP_CHECK(hipMalloc((void **) &D->s_out, np * 16));
    } catch (...) { delete D; throw; }
    return D;
}

void denoiser_destroy(Denoiser *d) { delete d; }

template <bool ALB, bool NRM, bool ALPHA>
static void denoise_launch(Denoiser *D, const float *noisy, int channels, const float *albedo, const float *normals, float *out) {
    hipStream_t st = D->stream;
    uint32_t np = (uint32_t) ((size_t) D->w * D->h);
    const lrt_denoise_params &P = D->prm;
    k_denoise_pack<ALB, NRM, ALPHA><<<(np + 255) / 256, 256, 0, st>>>(noisy, channels, albedo, normals, P.eps_a, np, D->colour[0], D->g_normal, D->g_albedo);
    HIP_CHECK(hipGetLastError());
    // the three inverse tolerances, each one float32 operation after another: 4^k / sigma_color^2, 1 / sigma_normal^2, 1 / sigma_albedo^2
    float sc2 = P.sigma_color * P.sigma_color, in = 1.f / (P.sigma_normal * P.sigma_normal), ia = 1.f / (P.sigma_albedo * P.sigma_albedo);
    dim3 block(LRT_DN_BX, LRT_DN_BY), grid((D->w + LRT_DN_BX - 1) / LRT_DN_BX, (D->h + LRT_DN_BY - 1) / LRT_DN_BY);
    for (int k = 0; k < P.iterations; ++k) {
        float ic = (float) (1u << (2 * k)) / sc2;
        k_denoise_pass<ALB, NRM, ALPHA><<<grid, block, 0, st>>>(D->colour[k & 1], D->g_normal, D->g_albedo, D->colour[(k + 1) & 1], D->w, D->h, 1 << k, ic, in, ia);
        HIP_CHECK(hipGetLastError());
    }
    k_denoise_unpack<ALB><<<(np + 255) / 256, 256, 0, st>>>(D->colour[P.iterations & 1], D->g_albedo, noisy, channels, P.eps_a, np, out);
    HIP_CHECK(hipGetLastError());
}

void denoiser_run(Denoiser *D, const float *noisy, int channels, const float *albedo, const float *normals, float *out, int device_buffers) {
    HIP_CHECK(hipSetDevice(D->device));
    hipStream_t st = D->stream;
    size_t np = (size_t) D->w * D->h;
    const float *d_noisy = noisy, *d_albedo = albedo, *d_normals = normals; float *d_out = out;
    if (!device_buffers) {
        HIP_CHECK(hipMemcpyAsync(D->s_noisy, noisy, np * channels * 4, hipMemcpyHostToDevice, st)); d_noisy = D->s_noisy;
        if (D->alb) { HIP_CHECK(hipMemcpyAsync(D->s_albedo, albedo, np * 12, hipMemcpyHostToDevice, st)); d_albedo = D->s_albedo; }
        if (D->nrm) { HIP_CHECK(hipMemcpyAsync(D->s_normals, normals, np * 12, hipMemcpyHostToDevice, st)); d_normals = D->s_normals; }
        d_out = D->s_out;
    }
    bool alpha = D->alpha && channels == 4;
    #define LRT_DN_CASE(A, N, AL) if (D->alb == A && D->nrm == N && alpha == AL) denoise_launch<A, N, AL>(D, d_noisy, channels, d_albedo, d_normals, d_out);
    LRT_DN_CASE(false, false, false) LRT_DN_CASE(false, false, true) LRT_DN_CASE(false, true, false) LRT_DN_CASE(false, true, true)
    LRT_DN_CASE(true, false, false)  LRT_DN_CASE(true, false, true)  LRT_DN_CASE(true, true, false)  LRT_DN_CASE(true, true, true)
    #undef LRT_DN_CASE
    if (!device_buffers) HIP_CHECK(hipMemcpyAsync(out, D->s_out, np * channels * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
}

} // namespace lrt
