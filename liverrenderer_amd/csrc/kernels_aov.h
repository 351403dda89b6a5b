// gfx950 kernels of the `aov` integrator (src/integrators/aov.cpp), included by device.hip after kernels.h.
//
//   k_aov          the AOV pass of AOVIntegrator::render (aov.cpp:382-391, SamplingIntegrator::render underneath): one lane per
//                  camera sample, non-persistent.  The lane's sampler at the start of the pass gives the pixel jitter exactly as
//                  generate_camera_path draws it, the primary ray is traced once (LDS image or global BVH), compute_si, then the
//                  AOVs of the first hit (AOVIntegrator::sample, aov.cpp:203-368) go through the reconstruction filter into a film
//                  of n_ch + 1 channels (the AOVs, then W).  No path loop: the nested integrators' colour comes from their own
//                  renders (device.hip, device_render_aov).
//   k_aov_develop  film / W into a channel range of the merged image (HDRFilm::develop without the colour conversion)
//   k_aov_copy     an inner integrator's developed image into its channel range of the merged image (merge_channels, aov.cpp:523-545)
//
// The film has a run-time channel count: the AOVs go through film_run / film_walk (film.h) one at a time, three channels each, then W.
#pragma once
#include "kernels.h"

namespace lrt {

// Per-render AOV table, read through the constant address space (the loops over it are wave-uniform: scalar loads).
struct DAovSpec {
    int32_t n_aovs, n_ch;                        // AOVs, and their channels (film: n_ch + 1 floats per pixel)
    int32_t type[LRT_AOV_MAX_AOVS];              // LRT_AOV_*
    int32_t offset[LRT_AOV_MAX_AOVS];            // first channel of each AOV
    const uint32_t *first_face;                  // per shape: first face (SI::prim is global, prim_index is within the shape)
};
typedef const LRT_CONST DAovSpec *AovSpecPtr;

DEV int aov_width(int type) {
    switch (type) {
        case LRT_AOV_DEPTH: case LRT_AOV_PRIM_INDEX: case LRT_AOV_SHAPE_INDEX: return 1;
        case LRT_AOV_UV: return 2;
        default: return 3;
    }
}

// The BSDF the first hit sees; -1 for none (a shape without BSDF: the render kernels never meet one, lrt_scene_from_desc rejects it)
DEV int aov_bsdf(SceneRef sc, const SI &si) {
    if (!si.valid) return -1;
    return tab(sc.shapes, si.shape, sc.one_shape).bsdf;
}

// One AOV of one lane (aov.cpp:222-343).  A miss is the zero interaction (aov.cpp:216), so every value is 0 there.
// EXT: the scene may hold a roughdielectric, a conductor, a plastic or a twosided (the EXT instances)
template <bool EXT = false>
DEV void aov_eval(SceneRef sc, AovSpecPtr A, int type, const SI &si, float v[3]) {
    v[0] = v[1] = v[2] = 0.f;
    if (!si.valid) return;
    switch (type) {
        case LRT_AOV_ALBEDO: {                   // BSDF::eval_diffuse_reflectance
            const int b = aov_bsdf(sc, si);
            if (b < 0) break;
            DBsdf B = tab(sc.bsdfs, b, sc.one_shape);
            if (B.type == LRT_BSDF_BUMPMAP) B = sc.bsdfs[B.nested];        // bumpmap.cpp:259: the nested BSDF's, at the unperturbed si
            if (EXT && B.type == LRT_BSDF_TWOSIDED) {                       // twosided.cpp:284-307: the child of the side that was hit; neither at wi.z = 0 with two children
                const int c = twosided_child(sc, b, B, si.wi.z);
                if (c < 0) break;
                B = sc.bsdfs[c];
            }
            // diffuse.cpp:181; plastic.cpp:362-365: its diffuse_reflectance, which DBsdf keeps in the same word (EXT).  dielectric / null /
            // conductor: the base class's eval(wo = +z) * pi = 0 (bsdf.cpp:38-43)
            if (B.type == LRT_BSDF_DIFFUSE || (EXT && B.type == LRT_BSDF_PLASTIC)) {
                const V3 r = tex_eval(sc, B.reflectance, si);
                v[0] = r.x; v[1] = r.y; v[2] = r.z;
            }
            if (EXT && B.type == LRT_BSDF_ROUGHDIELECTRIC) {                // the BSDF base class: eval(si with wi as it is, wo = +z) * pi (bsdf.cpp:38-43)
                const V3 r = leaf_eval<true>(sc, B, si, si.wi, V3(0.f, 0.f, 1.f)) * kPi;
                v[0] = r.x; v[1] = r.y; v[2] = r.z;
            }
            break;
        }
        case LRT_AOV_DEPTH: v[0] = si.t; break;
        case LRT_AOV_POSITION: v[0] = si.p.x; v[1] = si.p.y; v[2] = si.p.z; break;
        case LRT_AOV_UV: v[0] = si.uv.x; v[1] = si.uv.y; break;
        case LRT_AOV_GEO_NORMAL: v[0] = si.n.x; v[1] = si.n.y; v[2] = si.n.z; break;
        case LRT_AOV_SH_NORMAL: {                // BSDF::sh_frame(si).n
            const int b = aov_bsdf(sc, si);
            if (b < 0) break;
            const DBsdf B = tab(sc.bsdfs, b, sc.one_shape);
            // bumpmap.cpp:224-257 returns the perturbed normal in the LOCAL coordinates of the old shading frame (si.to_local, never
            // converted back): bump_frame gives that same frame.  Kept on purpose.
            const V3 n = B.type == LRT_BSDF_BUMPMAP ? bump_frame(sc, B, si).n : si.sh.n;
            v[0] = n.x; v[1] = n.y; v[2] = n.z;
            break;
        }
        case LRT_AOV_DP_DU: v[0] = si.dp_du.x; v[1] = si.dp_du.y; v[2] = si.dp_du.z; break;
        case LRT_AOV_DP_DV: v[0] = si.dp_dv.x; v[1] = si.dp_dv.y; v[2] = si.dp_dv.z; break;
        case LRT_AOV_PRIM_INDEX: {               // analytic shapes (rectangle, sphere) have a single primitive
            const DShape sd = tab(sc.shapes, si.shape, sc.one_shape);
            v[0] = sd.kind != LRT_SHAPE_MESH ? 0.f : (float) (si.prim - A->first_face[si.shape]);
            break;
        }
        case LRT_AOV_SHAPE_INDEX: v[0] = (float) (si.shape + 1u); break;   // aov.cpp:330-343: 1 + position in scene->shapes(), 0 = background
        default: break;
    }
}

// LDS: the BVH image in LDS, 1024-thread workgroups (as k_trace_lds); else the global BVH with LRT_BLOCK threads and the traversal
// stack in (dynamic) LDS.  Grid-stride over lanes [lp->lane_begin, lp->lane_begin + lp->n); every wave runs the same trip count, so the
// wave reductions below always see 64 active lanes.
template <bool LDS, bool LD, bool EXT = false>           // EXT: spheres (ExtTracer)
__global__ void __launch_bounds__(LDS ? 1024 : LRT_BLOCK)
k_aov(ScenePtr scp, LaunchPtr lp, AovSpecPtr A) {
    constexpr uint32_t BS = LDS ? 1024u : (uint32_t) LRT_BLOCK;
    SceneRef sc = *scp;
    RpRef rp = lp->rp;
    FilmRef F = sc.film;
    const uint64_t lane_begin = lp->lane_begin, n = lp->n;
    float *__restrict__ film = lp->film;
    float *__restrict__ sample_out = lp->sample_out;
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t tid = threadIdx.x;
    LdsScene L{};
    if (LDS) {
        const uint4 *src = lp->li.blob; uint4 *dst = reinterpret_cast<uint4 *>(smem);
        for (uint32_t k = tid; k < lp->li.blob_bytes / 16u; k += BS) dst[k] = src[k];
        L.nodes = reinterpret_cast<const float4 *>(smem + lp->li.nodes_off); L.verts = reinterpret_cast<const float4 *>(smem + lp->li.verts_off);
        L.tris = reinterpret_cast<const uint2 *>(smem + lp->li.tris_off);
        L.n_faces = sc.n_faces; L.root_is_leaf = (uint32_t) sc.root_is_leaf; L.root_first = sc.root_leaf_first; L.root_count = sc.root_leaf_count;
        __syncthreads();
    }
    const int n_aovs = A->n_aovs, n_ch = A->n_ch, C = n_ch + 1;
    for (uint64_t base = (uint64_t) blockIdx.x * BS; base < n; base += (uint64_t) gridDim.x * BS) {
        const uint64_t i = base + tid;
        const bool have = i < n;
        const uint64_t j = lane_begin + i;
        const uint32_t lane = (uint32_t) j;
        Ray ray; ray.o = V3(0.f); ray.d = V3(0.f, 0.f, 1.f); ray.maxt = 0.f;
        Hit h; h.t = kInf; h.u = h.v = 0.f; h.prim = 0xffffffffu;
        int px = 0, py = 0; float jx = 0.f, jy = 0.f;
        if (have) {                              // generate_camera_path up to the ray (integrator.cpp:321-338,449-470)
            SamplerT<LD> rng = lane_rng_pass_start<LD>(rp, lane, j);
            lane_to_pixel(sc, rp, lane, &px, &py);
            rng.next2(jx, jy);
            const float spx = (float) px + jx, spy = (float) py + jy;
            ray = camera_ray(sc, fma_(spx, sc.film.scale_x, sc.film.offset_x), fma_(spy, sc.film.scale_y, sc.film.offset_y));
            if (rp.pass_out) rp.pass_out[j] = rng.state;      // no nested integrator: the next pass continues after the jitter
            if (EXT) {
                const LdsTracer<1024> tl{ L, reinterpret_cast<uint16_t *>(smem + lp->li.stack_off) + tid };
                const GlobalTracer tg{ sc, reinterpret_cast<int *>(smem) + tid };
                h = LDS ? ExtTracer<LdsTracer<1024>>{ tl, sc }.closest(ray) : ExtTracer<GlobalTracer>{ tg, sc }.closest(ray);
            }
            else if (LDS) h = trace_lds<false, 1024>(L, ray, reinterpret_cast<uint16_t *>(smem + lp->li.stack_off) + tid);
            else h = trace<false>(sc, ray, reinterpret_cast<int *>(smem) + tid);
        }
        SI si;
        if (EXT && h.prim != 0xffffffffu && h.prim >= sc.n_faces) si = compute_si_sphere(sc, ray, h);
        else si = LDS ? compute_si(sc, ray, h, &L) : compute_si(sc, ray, h);
        if (sample_out) {                        // per-lane test hook: the values before film accumulation
            if (have) {
                float *o = sample_out + i * (uint64_t) n_ch;
                for (int k = 0; k < n_aovs; ++k) {
                    float v[3]; aov_eval<EXT>(sc, A, A->type[k], si, v);
                    const int w = aov_width(A->type[k]), off = A->offset[k];
#pragma unroll
                    for (int c = 0; c < 3; ++c) if (c < w) o[off + c] = v[c];     // constant indices: v stays in registers
                }
            }
            continue;
        }
        if (F.rfilter == LRT_RFILTER_BOX) {
            const FilmRun run = film_run(F, have, px, py);
            const bool head = run.head, tail = run.tail;
            float *p = film + (size_t) run.pixel * C;
            for (int k = 0; k < n_aovs; ++k) {
                const int type = A->type[k], w = aov_width(type), off = A->offset[k];
                float v[3]; aov_eval<EXT>(sc, A, type, si, v);
                wave_segmented_sums(v, head);
                if (tail) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) if (c < w) atomicAdd(p + off + c, v[c]);
                }
            }
            float wv[1] = { have ? 1.f : 0.f };
            wave_segmented_sums(wv, head);
            if (tail) atomicAdd(p + n_ch, wv[0]);
            continue;
        }
        // wider filters: one walk per AOV (channels at or past its width are not live), then W; each AOV is evaluated once per lane
        const FilmFootprint fp = film_footprint(F, px, py, jx, jy);         // (lanes without a sample: zeros, not read)
        for (int k = 0; k < n_aovs; ++k) {
            const int type = A->type[k], w = aov_width(type), off = A->offset[k];
            float v[3]; aov_eval<EXT>(sc, A, type, si, v);
            film_walk<3, -1>(F, have, fp, v, [&](int c) { return c < w; }, [&](int x, int y, const float (&t)[3]) {
                float *p = film + ((size_t) y * F.width + x) * C + off;
#pragma unroll
                for (int c = 0; c < 3; ++c) if (c < w) atomicAdd(p + c, t[c]);
            });
        }
        const float one[1] = { 1.f };
        film_walk<1, 0>(F, have, fp, one, [](int) { return true; }, [&](int x, int y, const float (&t)[1]) {
            atomicAdd(film + ((size_t) y * F.width + x) * C + n_ch, t[0]);
        });
    }
}

// HDRFilm::develop (hdrfilm.cpp:306-410) of the AOV film: channels / W (W = 0: 1, as k_develop), no colour conversion
__global__ void k_aov_develop(const float *__restrict__ film, int C, float *__restrict__ image, int T, int off, uint32_t n_pixels) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    float w = film[(size_t) i * C + C - 1]; if (w == 0.f) w = 1.f;
    for (int c = 0; c < C - 1; ++c) image[(size_t) i * T + off + c] = film[(size_t) i * C + c] / w;
}

// channels [0, S) of a developed image into channels [off, off + S) of the merged one
__global__ void k_aov_copy(const float *__restrict__ src, int S, float *__restrict__ dst, int T, int off, uint32_t n_pixels) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    for (int c = 0; c < S; ++c) dst[(size_t) i * T + off + c] = src[(size_t) i * S + c];
}

} // namespace lrt
