// gfx950 kernels of the `moment` integrator (src/integrators/moment.cpp, *_rgb variants), included by device.hip after kernels.h.
// DESIGN.md section 10 is the specification.
//
//   k_moment_splat    film accumulation of a moment render.  The render kernel has stored each lane's radiance (float4 per lane, the
//                     route k_splat_lanes serves for wide filters); this pass walks the lanes in lane order, forms X, Y, Z and their
//                     squares per lane (moment_values) and accumulates R,G,B,[A],W,X,Y,Z,m2X,m2Y,m2Z through the reconstruction filter.
//                     WIDE = false (box): the lanes of a pixel are runs of consecutive lanes, one segmented wave sum per channel, and
//                     the 10 / 11 sums of a run are handed to 10 / 11 lanes that add one contiguous 40 / 44-byte pixel record each.
//                     WIDE = true (gaussian, tent): film_walk (film.h) over the NC channels.
//   k_moment_develop  HDRFilm::develop of that film: every channel but W, divided by W (by 1 where W = 0)
//   k_moment_lanes    test hook: moment_values of a lane buffer, 6 floats per lane
//
// The channel count is a template parameter (ALPHA): every per-channel array below is indexed by unrolled constants and lives in
// registers.
#pragma once
#include "kernels.h"

namespace lrt {

template <bool ALPHA> struct MomentFilm {
    static constexpr int NC = ALPHA ? 11 : 10;     // film channels: R, G, B, [A], W, X, Y, Z, m2X, m2Y, m2Z (hdrfilm.cpp:245-258)
    static constexpr int W = ALPHA ? 4 : 3;        // index of the weight channel
};

// srgb_to_xyz (include/mitsuba/core/spectrum.h:396-402) and the squares, in the rounding order DESIGN.md section 10.1 fixes:
// row . rgb = fma(m2, B, fma(m1, G, m0 * R)); m2 = x * x.  m: X, Y, Z, m2X, m2Y, m2Z.
DEV void moment_values(V3 L, float (&m)[6]) {
    m[0] = fma_(0.180423f, L.z, fma_(0.357580f, L.y, 0.412453f * L.x));
    m[1] = fma_(0.072169f, L.z, fma_(0.715160f, L.y, 0.212671f * L.x));
    m[2] = fma_(0.950227f, L.z, fma_(0.119193f, L.y, 0.019334f * L.x));
    m[3] = m[0] * m[0]; m[4] = m[1] * m[1]; m[5] = m[2] * m[2];
}

// One sample's film record before the filter weight: v[c] is what ImageBlock::put multiplies by the weight (W: 1).
template <bool ALPHA>
DEV void moment_record(V3 L, float alpha, float (&v)[MomentFilm<ALPHA>::NC]) {
    float m[6]; moment_values(L, m);
    v[0] = L.x; v[1] = L.y; v[2] = L.z;
    if (ALPHA) v[3] = alpha;
    v[MomentFilm<ALPHA>::W] = 1.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[MomentFilm<ALPHA>::W + 1 + k] = m[k];
}

// Every lane of the block stays active to the end (lanes past n carry zeros): the wave reductions need all 64 lanes.
template <bool WIDE, bool ALPHA>
__global__ void __launch_bounds__(LRT_BLOCK)
k_moment_splat(ScenePtr scp, LaunchPtr lp) {
    constexpr int NC = MomentFilm<ALPHA>::NC, WI = MomentFilm<ALPHA>::W;
    RpRef rp = lp->rp;
    const float4 *__restrict__ lane_L = lp->L_buf; const uint32_t *__restrict__ pixel_list = lp->pixel_list;
    const uint64_t slot_base = lp->lane_begin, n = lp->n;
    float *__restrict__ film = lp->film;
    SceneRef sc = *scp;
    FilmRef F = sc.film;
    const uint64_t i = (uint64_t) blockIdx.x * LRT_BLOCK + threadIdx.x;
    const uint32_t me = threadIdx.x & 63u;
    const bool have = i < n;
    float v[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) v[k] = 0.f;
    uint32_t lane = 0; uint64_t j = 0;
    if (have) {
        j = slot_base + i;
        lane = slot_to_lane(rp, pixel_list, j);
        const float4 r = lane_L[i];
        V3 L(r.x, r.y, r.z);
        if (rp.integrator == LRT_INTEGRATOR_PATH && r.w == 0.f) L = V3(0.f);          // path.cpp:342-345, before the conversion to XYZ
        moment_record<ALPHA>(L, r.w, v);
    }
    if (!WIDE) {
        // Box filter (film_run): the last lane of a run holds the run's NC sums.
        int px = 0, py = 0;
        if (have) lane_to_pixel(sc, rp, lane, &px, &py);
        const FilmRun run = film_run(F, have, px, py);
        const uint32_t pixel = run.pixel;
        wave_segmented_sums(v, run.head);
        // The adds of a run are spread over lanes: up to four runs at a time, run s of the group served by lanes 16 s .. 16 s + NC - 1,
        // each of which fetches its channel's sum from the run's last lane and adds it: one atomic instruction writes four contiguous
        // pixel records instead of NC instructions with one lane per record.
        unsigned long long tails = __ballot(run.tail);
        const uint32_t ch = me & 15u, slot = me >> 4;
        while (tails) {
            int src = -1;
#pragma unroll
            for (int s = 0; s < 4; ++s) if (tails) { const int t = __ffsll((long long) tails) - 1; tails &= tails - 1ull; if ((int) slot == s) src = t; }
            const int from = src < 0 ? (int) me : src;
            const uint32_t px = (uint32_t) __shfl((int) pixel, from);
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < NC; ++k) { const float t = __shfl(v[k], from); if ((int) ch == k) sum = t; }
            if (src >= 0 && ch < (uint32_t) NC) atomicAdd(film + (size_t) px * NC + ch, sum);
        }
        return;
    }
    FilmFootprint fp{};
    if (have) {
        int px, py; lane_to_pixel(sc, rp, lane, &px, &py);
        float jx, jy; lane_jitter(rp, lane, j, jx, jy);
        fp = film_footprint(F, px, py, jx, jy);
    }
    film_walk<NC, WI>(F, have, fp, v, [](int) { return true; }, [&](int x, int y, const float (&t)[NC]) {
        float *p = film + ((size_t) y * F.width + x) * NC;
#pragma unroll
        for (int k = 0; k < NC; ++k) atomicAdd(p + k, t[k]);
    });
}

// src/films/hdrfilm.cpp:306-410 for the moment film: W is dropped, the other channels are divided by it
template <bool ALPHA>
__global__ void k_moment_develop(const float *__restrict__ film, float *__restrict__ image, uint32_t n_pixels) {
    constexpr int NC = MomentFilm<ALPHA>::NC, WI = MomentFilm<ALPHA>::W;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const float *p = film + (size_t) i * NC; float *o = image + (size_t) i * (NC - 1);
    float w = p[WI]; if (w == 0.f) w = 1.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) if (c != WI) o[c < WI ? c : c - 1] = p[c] / w;
}

// Test hook (lrt_render_moment_samples): X, Y, Z, m2X, m2Y, m2Z of n lanes of a lane buffer
__global__ void k_moment_lanes(const float4 *__restrict__ lane_L, int zero_invalid, uint32_t n, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 r = lane_L[i];
    V3 L(r.x, r.y, r.z);
    if (zero_invalid && r.w == 0.f) L = V3(0.f);                                      // path.cpp:342-345
    float m[6]; moment_values(L, m);
    float *o = out + (size_t) i * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = m[k];
}

} // namespace lrt
