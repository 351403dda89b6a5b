// Device functions of the hip_ad_rgb hot path: BVH traversal, surface
// interactions, BSDFs, phase functions, media and emitters.  Each function
// cites the reference lines it implements (paths relative to the reference).
#pragma once
#include "device_types.h"
#include "dmath.h"
#include "../../include/liverrt.h"

namespace lrt {

#define LRT_BLOCK 256
#define LRT_STACK 32

// Read-only scene tables (shapes, BSDFs, media, ...): when every active lane of the wave asks for the same entry (one
// medium, one shape: the liver scenes), the entry comes through the scalar cache (constant address space, s_load) instead
// of one vector load per lane and dword.  The kernels never write these tables.
template <class T> DEV T tab(const T *table, uint32_t i, bool worth_a_look = true) {
    if (!worth_a_look) return table[i];                  // (a wave-uniform flag: scenes with many shapes skip the test)
    const uint32_t i0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) i);
    // (scalar loads ignore EXEC: with no active lane i0 is not an index anyone vouches for, so that case takes the masked vector path)
    if (__builtin_amdgcn_ballot_w64(true) != 0ull && __builtin_amdgcn_ballot_w64(i != i0) == 0ull)
    { T out; __builtin_memcpy(&out, reinterpret_cast<const LRT_CONST T *>((uintptr_t) table) + i0, sizeof(T)); return out; }
    return table[i];
}

struct Ray { V3 o, d; float maxt; };
struct Hit { float t, u, v; uint32_t prim; uint32_t slot = 0xffffffffu; };   // slot: the LDS tracer's triangle slot (vertex indices without a global load), else none
struct SI { bool valid; float t; V3 p, n; Frame sh; V2 uv; V3 dp_du, dp_dv, wi; uint32_t prim, shape; };

// ------------------------------------------------------------- traversal
DEV float slab_rcp(float x) { return fmin_(fmax_(__builtin_amdgcn_rcpf(x), -1e20f), 1e20f); }
// Moeller-Trumbore on a pre-gathered triangle slot (include/mitsuba/render/mesh.h:506-527).
// Ties are resolved towards the lower primitive index so that the result does
// not depend on the traversal order.
DEV void test_tri(const float4 *__restrict__ tris, uint32_t slot, V3 o, V3 d, float maxt, Hit &best) {
    float4 a = tris[3 * slot], b = tris[3 * slot + 1], c = tris[3 * slot + 2];
    V3 p0(a.x, a.y, a.z), e1(b.x, b.y, b.z), e2(c.x, c.y, c.z);
    uint32_t f = f2u(a.w);
    V3 pvec = cross(d, e2);
    float inv_det = rcp(dot(e1, pvec));
    V3 tvec = o - p0;
    float u = dot(tvec, pvec) * inv_det;
    if (!(u >= 0.f && u <= 1.f)) return;
    V3 qvec = cross(tvec, e1);
    float v = dot(d, qvec) * inv_det;
    if (!(v >= 0.f && u + v <= 1.f)) return;
    float t = dot(e2, qvec) * inv_det;
    if (!(t >= 0.f && t <= maxt)) return;
    if (t < best.t || (t == best.t && f < best.prim)) { best.t = t; best.u = u; best.v = v; best.prim = f; }
}

// Stack-based BVH2 traversal; the per-lane stack lives in LDS, laid out
// [entry][thread] so that a wave's pushes/pops hit 64 consecutive banks.
template <bool ANY_HIT>
DEV Hit trace(SceneRef sc, const Ray &r, int *__restrict__ stack /* &lds[threadIdx.x] */) {
    Hit best; best.t = kInf; best.u = best.v = 0.f; best.prim = 0xffffffffu;
    if (sc.n_faces == 0) return best;
    const V3 o = r.o, d = r.d;
    if (sc.root_is_leaf) {
        for (uint32_t i = 0; i < sc.root_leaf_count; ++i) test_tri(sc.tris, sc.root_leaf_first + i, o, d, r.maxt, best);
        return best;
    }
    // "while-while" traversal (see trace_lds below for the rationale): descend to the next leaf with box tests only, then
    // test the leaf's triangles.  Work items: inner node index (< 0x7fffffff), or 0x80000000 | first slot; a leaf
    // ends at the slot whose e1.w is non-zero (bvh.cpp).
    // The slab arithmetic only culls (padded boxes, hits decided by the exact triangle tests and the tie rule).
    // reciprocals clamped to +-1e20: a direction component of (almost) zero must give (n - o) * huge = -+huge per plane, not
    // inf - inf = NaN, so that rays parallel to a slab are kept or culled by the side of the origin (the padding decides ties)
    const float ix = slab_rcp(d.x), iy = slab_rcp(d.y), iz = slab_rcp(d.z);
    const float ox = -o.x * ix, oy = -o.y * iy, oz = -o.z * iz;
    const f32x2 vix = { ix, ix }, viy = { iy, iy }, viz = { iz, iz }, vox = { ox, ox }, voy = { oy, oy }, voz = { oz, oz };
    const uint32_t DONE = 0x7fffffffu;
    int sp = 0; uint32_t cur = 0;
    for (;;) {
        while (cur < DONE) {
            const float4 *nd = sc.nodes + 4 * (size_t) cur;
            float4 n0 = nd[0], n1 = nd[1], n2 = nd[2], n3 = nd[3];
            float limit = fmin_(best.t, r.maxt);
            // twelve slab planes as six packed fmas (v_pk_fma_f32: both halves in one issue slot; IEEE fma per element)
            const f32x2 vax = pk_fma(f32x2{ n0.x, n0.y }, vix, vox), vay = pk_fma(f32x2{ n0.z, n0.w }, viy, voy), vaz = pk_fma(f32x2{ n2.x, n2.y }, viz, voz);
            const f32x2 vbx = pk_fma(f32x2{ n1.x, n1.y }, vix, vox), vby = pk_fma(f32x2{ n1.z, n1.w }, viy, voy), vbz = pk_fma(f32x2{ n2.z, n2.w }, viz, voz);
            const float ax0 = vax.x, ax1 = vax.y, ay0 = vay.x, ay1 = vay.y, az0 = vaz.x, az1 = vaz.y;
            const float bx0 = vbx.x, bx1 = vbx.y, by0 = vby.x, by1 = vby.y, bz0 = vbz.x, bz1 = vbz.y;
            float tmin0 = fmax_(fmax_(fmin_(ax0, ax1), fmin_(ay0, ay1)), fmax_(fmin_(az0, az1), 0.f));
            float tmax0 = fmin_(fmin_(fmax_(ax0, ax1), fmax_(ay0, ay1)), fmin_(fmax_(az0, az1), limit));
            float tmin1 = fmax_(fmax_(fmin_(bx0, bx1), fmin_(by0, by1)), fmax_(fmin_(bz0, bz1), 0.f));
            float tmax1 = fmin_(fmin_(fmax_(bx0, bx1), fmax_(by0, by1)), fmin_(fmax_(bz0, bz1), limit));
            bool h0 = tmin0 <= tmax0 * 1.000002f, h1 = tmin1 <= tmax1 * 1.000002f;      // (tmin >= 0, so an additive floor on the right-hand side decides nothing)
            int r0 = (int) f2u(n3.x), r1 = (int) f2u(n3.y);
            uint32_t c0 = r0 < 0 ? (0x80000000u | (uint32_t) ~r0) : (uint32_t) r0;
            uint32_t c1 = r1 < 0 ? (0x80000000u | (uint32_t) ~r1) : (uint32_t) r1;
            if (h0 && h1) {
                bool swap = tmin1 < tmin0;
                stack[sp * LRT_BLOCK] = (int) (swap ? c0 : c1); ++sp;
                cur = swap ? c1 : c0;
            } else if (h0 || h1) cur = h0 ? c0 : c1;                    // (two flat predicated regions instead of these nested three: measured, +0.4 % time)
            else if (sp == 0) cur = DONE;
            else { --sp; cur = (uint32_t) stack[sp * LRT_BLOCK]; }
        }
        if (cur == DONE) break;
        uint32_t slot = cur & 0x7fffffffu; bool last;
        do { last = sc.tris[3 * slot + 1].w != 0.f; test_tri(sc.tris, slot, o, d, r.maxt, best); ++slot; } while (!last);
        if (ANY_HIT && best.prim != 0xffffffffu) return best;
        if (sp == 0) break;
        --sp; cur = (uint32_t) stack[sp * LRT_BLOCK];
    }
    return best;
}

// Ray-query back-ends the integrator loops are templated on.
struct GlobalTracer {                      // BVH in global memory (any scene size), 32-bit stack entries in LDS
    static constexpr bool kExt = false;    // (ExtTracer below: spheres, point emitters and area emitters on meshes)
    SceneRef sc; int *stack;
    DEV Hit closest(const Ray &r) const { return trace<false>(sc, r, stack); }
    DEV Hit closest_from(const Ray &r, uint32_t) const { return trace<false>(sc, r, stack); }      // (the entry is an item of the LDS image: this tracer starts at its root)
    DEV Hit any(const Ray &r) const { return trace<true>(sc, r, stack); }
    DEV SI surface(SceneRef s, const Ray &r, const Hit &h) const;
};

// Whole BVH resident in LDS (scenes whose image fits next to the traversal stacks: the liver meshes and the Cornell
// box do): nodes as in bvh.h, vertices padded to float4, triangle slots as 4 x u16 vertex indices, 16-bit stack
// entries.  Edge vectors are formed in the kernel with the same float subtractions the host builder uses, so hits
// are bit-identical to the global-memory path.
struct LdsScene {
    const float4 *nodes; const float4 *verts; const uint2 *tris;
    uint32_t n_faces, root_is_leaf, root_first, root_count;
};
#define LRT_LDS_BLOCK_MAX 1024

// `ix` = the slot's index words: three 16-bit vertex indices, then (face index << 1 | last-slot-of-the-leaf flag)
// While a traversal runs, best.prim = face index | slot << 16 (both < 0x8000; 0xffffffff = no hit yet).
DEV void test_tri_lds(const LdsScene &L, uint2 ix, uint32_t slot, V3 o, V3 d, float maxt, Hit &best) {
    float4 a = L.verts[ix.x & 0xffffu], b = L.verts[ix.x >> 16], c = L.verts[ix.y & 0xffffu];
    V3 p0(a.x, a.y, a.z), e1(b.x - a.x, b.y - a.y, b.z - a.z), e2(c.x - a.x, c.y - a.y, c.z - a.z);
    V3 pvec = cross(d, e2);
    float inv_det = rcp(dot(e1, pvec));
    V3 tvec = o - p0;
    float u = dot(tvec, pvec) * inv_det;
    if (!(u >= 0.f && u <= 1.f)) return;
    V3 qvec = cross(tvec, e1);
    float v = dot(d, qvec) * inv_det;
    if (!(v >= 0.f && u + v <= 1.f)) return;
    float t = dot(e2, qvec) * inv_det;
    if (!(t >= 0.f && t <= maxt)) return;
    if (t > best.t) return;
    uint32_t f = ix.y >> 17;
    if (t < best.t || f < (best.prim & 0x7fffu)) { best.t = t; best.u = u; best.v = v; best.prim = f | (slot << 16); }
}

#ifdef LRT_TRAV_STATS
__device__ unsigned long long g_trav[8];            // developer counters: [ANY ? 4 : 0] + { node-loop wave iterations, active lanes in them, leaf-loop wave iterations, active lanes }
#define LRT_TRAV_COUNT(k) { const unsigned long long m_ = __ballot(true); if ((threadIdx.x & 63u) == (uint32_t) (__ffsll((long long) m_) - 1)) { atomicAdd(&g_trav[(ANY_HIT ? 4 : 0) + k], 1ull); atomicAdd(&g_trav[(ANY_HIT ? 4 : 0) + k + 1], (unsigned long long) __popcll(m_)); } }
#else
#define LRT_TRAV_COUNT(k)
#endif
// `start`: the work item the traversal begins at: 0, the root, or what the host has proven for this ray (DScene::primary_tab: an inner node or a leaf
// whose subtree holds every triangle the ray can hit first; 0xffff: there is none)
template <bool ANY_HIT, int STRIDE>
DEV Hit trace_lds(const LdsScene &L, const Ray &r, uint16_t *__restrict__ stack /* &lds_stack[threadIdx.x] */, uint32_t start = 0u) {
    Hit best; best.t = kInf; best.u = best.v = 0.f; best.prim = 0xffffffffu;
    if (L.n_faces == 0) return best;
    if (start == 0xffffu) return best;
    const V3 o = r.o, d = r.d;
    if (L.root_is_leaf) {
        for (uint32_t i = 0; i < L.root_count; ++i) test_tri_lds(L, L.tris[L.root_first + i], L.root_first + i, o, d, r.maxt, best);
        if (best.prim != 0xffffffffu) { best.slot = best.prim >> 16; best.prim &= 0x7fffu; }
        return best;
    }
    // The slab arithmetic only culls (hits are decided by the Moeller-Trumbore tests and the tie rule), so it may differ
    // from the oracle's: approximate reciprocal, one fma per plane, 3-input min/max.  The padded boxes absorb the error.
    // "while-while" traversal: every lane first descends to its next leaf (inner loop: box tests only), then the lanes
    // test their leaf triangles together; this keeps far more lanes busy than testing leaves where they are met.
    // Work items are 16-bit: inner node index (< 0x8000) or 0x8000 | first triangle slot; a leaf ends at the slot whose
    // index word carries the "last" flag (device.hip).
    // reciprocals clamped to +-1e20: a direction component of (almost) zero must give (n - o) * huge = -+huge per plane, not
    // inf - inf = NaN, so that rays parallel to a slab are kept or culled by the side of the origin (the padding decides ties)
    const float ix = slab_rcp(d.x), iy = slab_rcp(d.y), iz = slab_rcp(d.z);
    const float ox = -o.x * ix, oy = -o.y * iy, oz = -o.z * iz;
    const f32x2 vix = { ix, ix }, viy = { iy, iy }, viz = { iz, iz }, vox = { ox, ox }, voy = { oy, oy }, voz = { oz, oz };
    const uint32_t DONE = 0x10000u;
    int sp = 0; uint32_t cur = start;
    for (;;) {
        while (cur < 0x8000u) {
            LRT_TRAV_COUNT(0)
            const float4 *nd = L.nodes + 4 * cur;
            float4 n0 = nd[0], n1 = nd[1], n2 = nd[2], n3 = nd[3];
            float limit = fmin_(best.t, r.maxt);
            // twelve slab planes as six packed fmas (v_pk_fma_f32: both halves in one issue slot; IEEE fma per element)
            const f32x2 vax = pk_fma(f32x2{ n0.x, n0.y }, vix, vox), vay = pk_fma(f32x2{ n0.z, n0.w }, viy, voy), vaz = pk_fma(f32x2{ n2.x, n2.y }, viz, voz);
            const f32x2 vbx = pk_fma(f32x2{ n1.x, n1.y }, vix, vox), vby = pk_fma(f32x2{ n1.z, n1.w }, viy, voy), vbz = pk_fma(f32x2{ n2.z, n2.w }, viz, voz);
            const float ax0 = vax.x, ax1 = vax.y, ay0 = vay.x, ay1 = vay.y, az0 = vaz.x, az1 = vaz.y;
            const float bx0 = vbx.x, bx1 = vbx.y, by0 = vby.x, by1 = vby.y, bz0 = vbz.x, bz1 = vbz.y;
            float tmin0 = fmax_(fmax_(fmin_(ax0, ax1), fmin_(ay0, ay1)), fmax_(fmin_(az0, az1), 0.f));
            float tmax0 = fmin_(fmin_(fmax_(ax0, ax1), fmax_(ay0, ay1)), fmin_(fmax_(az0, az1), limit));
            float tmin1 = fmax_(fmax_(fmin_(bx0, bx1), fmin_(by0, by1)), fmax_(fmin_(bz0, bz1), 0.f));
            float tmax1 = fmin_(fmin_(fmax_(bx0, bx1), fmax_(by0, by1)), fmin_(fmax_(bz0, bz1), limit));
            bool h0 = tmin0 <= tmax0 * 1.000002f, h1 = tmin1 <= tmax1 * 1.000002f;      // (tmin >= 0, so an additive floor on the right-hand side decides nothing)
            const uint32_t c0 = f2u(n3.x), c1 = f2u(n3.y);             // already work items (device.hip builds the LDS image)
            if (h0 && h1) {
                bool swap = tmin1 < tmin0;
                stack[sp * STRIDE] = (uint16_t) (swap ? c0 : c1); ++sp;
                cur = swap ? c1 : c0;
            } else if (h0 || h1) cur = h0 ? c0 : c1;
            else if (sp == 0) cur = DONE;
            else { --sp; cur = stack[sp * STRIDE]; }
        }
        if (cur == DONE) break;
        uint32_t slot = cur & 0x7fffu, last;
        do {
            LRT_TRAV_COUNT(2)
            const uint2 ix = L.tris[slot];
            last = (ix.y >> 16) & 1u;
            test_tri_lds(L, ix, slot, o, d, r.maxt, best);
            ++slot;
        } while (!last);
        if (ANY_HIT && best.prim != 0xffffffffu) return best;
        if (sp == 0) break;
        --sp; cur = stack[sp * STRIDE];
    }
    if (best.prim != 0xffffffffu) { best.slot = best.prim >> 16; best.prim &= 0x7fffu; }
    return best;
}

template <int STRIDE>
struct LdsTracer {
    static constexpr bool kExt = false;
    const LdsScene &L; uint16_t *stack;
    DEV Hit closest(const Ray &r) const { return trace_lds<false, STRIDE>(L, r, stack); }
    DEV Hit closest_from(const Ray &r, uint32_t start) const { return trace_lds<false, STRIDE>(L, r, stack, start); }     // (trace_lds: `start`)
    DEV Hit any(const Ray &r) const { return trace_lds<true, STRIDE>(L, r, stack); }
    DEV SI surface(SceneRef s, const Ray &r, const Hit &h) const;
};

// --------------------------------------------------- conservative distance field
// Lower bound of the distance from p to the nearest triangle (0: unknown / outside the grid).  |p - centre| is subtracted
// exactly (1-Lipschitz), the stored value already carries the safety margins (device.hip: build_dist_grid).
DEV float dist_grid_lower_bound(GridRef g, V3 p) {
    // D(c) - |p - c| bounds the distance for ANY p, so the cell index is simply clamped into the grid (a point outside the
    // grid gets a small or negative bound; NaN coordinates give NaN, which proves nothing).
    float fx = (p.x - g.lo[0]) * g.inv_cell, fy = (p.y - g.lo[1]) * g.inv_cell, fz = (p.z - g.lo[2]) * g.inv_cell;
    int ix = min(max((int) fx, 0), g.n[0] - 1), iy = min(max((int) fy, 0), g.n[1] - 1), iz = min(max((int) fz, 0), g.n[2] - 1);
    union { uint16_t u; _Float16 h; } cv; cv.u = g.d[(uint32_t) ((iz * g.n[1] + iy) * g.n[0] + ix)];
    float D = (float) cv.h;
    float cx = fx - ((float) ix + .5f), cy = fy - ((float) iy + .5f), cz = fz - ((float) iz + .5f);
    return D - __builtin_amdgcn_sqrtf(cx * cx + cy * cy + cz * cz) * (g.cell * 1.001f);   // 1-ulp hardware sqrt: inside the margins
}

// True when the segment o + t d, t in [0, maxt], provably meets no triangle: a few sphere-tracing steps through the
// distance field.  Margins: 1 % on the segment length, every advance counted 0.5 % short (f32 error of the
// Moller-Trumbore t is ~1e-6 relative away from grazing incidence).  False means "unknown": run the ray query.
#ifndef LRT_GRID_STEPS
#define LRT_GRID_STEPS 3
#endif
template <int STEPS = LRT_GRID_STEPS>
DEV bool segment_proven_empty(GridRef g, V3 o, V3 d, float maxt) {
    if (!g.enabled || !(maxt < 1e30f)) return false;
    float len = __builtin_amdgcn_sqrtf(dot(d, d));                       // hardware sqrt / rcp (1 ulp): inside the margins
    float remaining = maxt * len * 1.01f, inv_len = __builtin_amdgcn_rcpf(len);
    V3 p = o;
    for (int k = 0; k < STEPS; ++k) {
        float lb = dist_grid_lower_bound(g, p);
        if (remaining < lb) return true;
        if (!(lb > .5f * g.cell)) return false;
        float adv = lb * .99f;
        p = p + d * (adv * inv_len);
        remaining -= adv * .995f;
    }
    return false;
}

// The same question answered with K INDEPENDENT lookups instead of a chain of dependent ones: lower bounds at K points spread over the
// segment; the segment is free of surfaces when the balls around those points (radius = the bound) cover it end to end.  One memory round
// trip instead of three (the dependent lookups were the largest stall of a medium trip: section timers of the proven-free tiles), and the
// cover test uses the bounds actually found, so one large ball in the middle can do it alone.  Same margins as above.
// `start` (the closed-records volpath kernels; 0 elsewhere: the code of every other caller is what it was): the stretch from the origin that
// the caller has already proven free, in the lengthened units of L (the per-face cone table, scene_prep.cpp: build_cone_table).
template <int K>
DEV bool segment_covered_by_balls(GridRef g, V3 o, V3 d, float maxt, float start = 0.f) {
    if (!g.enabled || !(maxt < 1e30f)) return false;
    const float len = __builtin_amdgcn_sqrtf(dot(d, d));                 // hardware sqrt (1 ulp): inside the margins
    const float L = maxt * len * 1.01f;                                  // the segment, 1 % long
#define LRT_FRAC(k) (((float) (k) + .5f) / (float) K)          /* K = 2: at 1/4 and 3/4 (0.2 / 0.7, 0.3 / 0.8, 0.15 / 0.6 measured: no better) */
    float lb[K];
#pragma unroll
    for (int k = 0; k < K; ++k) lb[k] = dist_grid_lower_bound(g, fma3(d, maxt * LRT_FRAC(k), o)) * .995f;
    float covered = start; bool ok = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float c = L * LRT_FRAC(k);                                // the point's position along the (lengthened) segment
        ok = ok && (lb[k] > 0.f) && (c - lb[k] <= covered);
        covered = fmax_(covered, c + lb[k]);
    }
    return ok && covered >= L;
#undef LRT_FRAC
}

// What the kernels call.  Two balls: measured on C3 against the three dependent steps above: 4.6 % more segments proven (20.35 M
// proven-free tiles per launch against 19.45 M), every medium tile 1 - 2 % shorter, launch -2.3 ... -3.5 %; 3, 4 and 6 balls prove more
// still but the gathers cost more than they save (226 / 231 / 242 ms against 222), one ball at the midpoint proves less (229).
// LRT_SPHERE_TRACE (build switch) brings the dependent steps back.
DEV bool segment_free_of_surfaces(GridRef g, V3 o, V3 d, float maxt) {
#ifdef LRT_SPHERE_TRACE
    return segment_proven_empty(g, o, d, maxt);
#else
    return segment_covered_by_balls<2>(g, o, d, maxt);
#endif
}
// The closed-records volpath kernels' form.  `cone`: what the per-face cone table says about a segment that starts on a surface, in the cover
// test's lengthened units: > 0 the free stretch from the origin; < 0 the table holds nothing for it (an empty row, or a direction flatter than
// the widest bin): the lookups are not made and the segment goes to its ray query.  That gives up, by choice, the proofs the balls alone would still
// find: the first ball sits a quarter of the way along and has to reach back to an origin that spawn_ray lifted off its triangle by no more than
// the ray epsilon, so only segments of a few hundred epsilons qualify (below about 0.7 units on the liver; 8 - 26 % of refracted-in segments in
// DESIGN.md section 6e).  PF_NOHIT only elides a query that finds nothing, so no lane changes, and leaving those segments to the balls timed the same.
// 0: the segment does not start on a surface.  A segment that the cone covers alone needs no lookup.
DEV bool segment_free_of_surfaces_from(GridRef g, V3 o, V3 d, float maxt, float cone) {
    if (cone < 0.f || !g.enabled || !(maxt < 1e30f)) return false;
    if (cone > 0.f && cone >= maxt * __builtin_amdgcn_sqrtf(dot(d, d)) * 1.01f) return true;
    return segment_covered_by_balls<2>(g, o, d, maxt, cone);
}
// A face's row of the cone table for a direction d leaving the face whose geometric normal (as the surface interaction holds it) is n:
// `rows` = the face's two sides (cone_tab[2 f], cone_tab[2 f + 1]), binary16 lengths of the bins LRT_CONE_COS0 .. 3.  Returns the free length in the
// cover test's lengthened units, or -1 when the row holds none or the direction's cosine is below LRT_CONE_COS3.
DEV float cone_free_length(uint4 rows, V3 d, V3 n) {
    const float cs = dot(d, n), c = __builtin_fabsf(cs) * __builtin_amdgcn_rsqf(dot(d, d));
    const uint32_t lo = cs < 0.f ? rows.z : rows.x, hi = cs < 0.f ? rows.w : rows.y;
    const uint32_t w = c >= LRT_CONE_COS1 ? lo : hi;
    uint32_t h = (c >= LRT_CONE_COS0 || (c < LRT_CONE_COS1 && c >= LRT_CONE_COS2)) ? (w & 0xffffu) : (w >> 16);
    if (!(c >= LRT_CONE_COS3)) h = 0u;
    union { uint16_t u; _Float16 f; } cv; cv.u = (uint16_t) h;
    const float r = (float) cv.f;
    return r > 0.f ? r * 1.01f : -1.f;
}

// --------------------------------------------------- surface interaction
// src/render/mesh.cpp:1489-1659 + include/mitsuba/render/interaction.h:290-300,516-536
// `L` (LDS tracer only): vertex indices and positions of the hit triangle come from the LDS image (same values as the
// global arrays), which takes the index loads out of the dependent chain of global loads.
DEV SI compute_si(SceneRef sc, const Ray &r, const Hit &h, const LdsScene *L = nullptr) {
    const bool valid = h.prim != 0xffffffffu;
    // every field is written through plain locals (no member addresses escape): keeps the record in VGPRs
    float t = kInf; V3 p(0.f), n(0.f), shn(0.f), shs(0.f), sht(0.f), dp_du(0.f), dp_dv(0.f), wi = -r.d;
    V2 uv = { 0.f, 0.f }; uint32_t f = 0xffffffffu, shp = 0xffffffffu;
    if (valid) {
        f = h.prim; shp = 0u; if (!sc.one_shape) shp = sc.face_shape[f];
        const DShape sd = tab(sc.shapes, shp, sc.one_shape);
        uint32_t i0, i1, i2; V3 p0, p1, p2;
        if (L && h.slot != 0xffffffffu) {
            const uint2 ix = L->tris[h.slot];
            i0 = ix.x & 0xffffu; i1 = ix.x >> 16; i2 = ix.y & 0xffffu;
            const float4 a = L->verts[i0], b = L->verts[i1], c = L->verts[i2];
            p0 = V3(a.x, a.y, a.z); p1 = V3(b.x, b.y, b.z); p2 = V3(c.x, c.y, c.z);
        } else {
            i0 = sc.faces[3 * f]; i1 = sc.faces[3 * f + 1]; i2 = sc.faces[3 * f + 2];
            p0 = V3(sc.positions[3 * i0], sc.positions[3 * i0 + 1], sc.positions[3 * i0 + 2]);
            p1 = V3(sc.positions[3 * i1], sc.positions[3 * i1 + 1], sc.positions[3 * i1 + 2]);
            p2 = V3(sc.positions[3 * i2], sc.positions[3 * i2 + 1], sc.positions[3 * i2 + 2]);
        }
        float b1 = h.u, b2 = h.v, b0 = 1.f - b1 - b2;
        t = h.t;
        p = V3(fma_(p0.x, b0, fma_(p1.x, b1, p2.x * b2)), fma_(p0.y, b0, fma_(p1.y, b1, p2.y * b2)), fma_(p0.z, b0, fma_(p1.z, b1, p2.z * b2)));
        V3 dp0 = p1 - p0, dp1 = p2 - p0;
        n = normalize(cross(dp0, dp1));
        uv = { b1, b2 };
        Basis bs = coordinate_system(n);
        dp_du = bs.s; dp_dv = bs.t;
        if (sd.has_texcoords) {
            const float2 t0 = *reinterpret_cast<const float2 *>(sc.vattr + 2 * (size_t) i0 + 1), t1 = *reinterpret_cast<const float2 *>(sc.vattr + 2 * (size_t) i1 + 1),
                         t2 = *reinterpret_cast<const float2 *>(sc.vattr + 2 * (size_t) i2 + 1);
            V2 uv0 = { t0.x, t0.y }, uv1 = { t1.x, t1.y }, uv2 = { t2.x, t2.y };
            uv = { fma_(uv2.x, b2, fma_(uv1.x, b1, uv0.x * b0)), fma_(uv2.y, b2, fma_(uv1.y, b1, uv0.y * b0)) };
            V2 duv0 = { uv1.x - uv0.x, uv1.y - uv0.y }, duv1 = { uv2.x - uv0.x, uv2.y - uv0.y };
            float det = fma_(duv0.x, duv1.y, -(duv0.y * duv1.x)), inv_det = rcp(det);
            if (det != 0.f) {
                dp_du = V3(fma_(duv1.y, dp0.x, -(duv0.y * dp1.x)), fma_(duv1.y, dp0.y, -(duv0.y * dp1.y)), fma_(duv1.y, dp0.z, -(duv0.y * dp1.z))) * inv_det;
                dp_dv = V3(fma_(-duv1.x, dp0.x, duv0.x * dp1.x), fma_(-duv1.x, dp0.y, duv0.x * dp1.y), fma_(-duv1.x, dp0.z, duv0.x * dp1.z)) * inv_det;
            }
        }
        if (sd.has_normals) {
            const float4 a0 = sc.vattr[2 * (size_t) i0], a1 = sc.vattr[2 * (size_t) i1], a2 = sc.vattr[2 * (size_t) i2];
            V3 n0(a0.x, a0.y, a0.z), n1(a1.x, a1.y, a1.z), n2(a2.x, a2.y, a2.z);
            V3 ni(fma_(n2.x, b2, fma_(n1.x, b1, n0.x * b0)), fma_(n2.y, b2, fma_(n1.y, b1, n0.y * b0)), fma_(n2.z, b2, fma_(n1.z, b1, n0.z * b0)));
            float il = rsqrt_(squared_norm(ni));
            shn = ni * il;
        } else shn = n;
        if (sd.flip_normals) { n = V3(-n.x, -n.y, -n.z); shn = V3(-shn.x, -shn.y, -shn.z); }
        shs = normalize(fma3(shn, -dot(shn, dp_du), dp_du));
        if (dp_du.x == 0.f && dp_du.y == 0.f && dp_du.z == 0.f) shs = coordinate_system(shn).s;
        sht = cross(shn, shs);
        V3 md(-r.d.x, -r.d.y, -r.d.z);
        wi = V3(dot(md, shs), dot(md, sht), dot(md, shn));
    }
    SI si;
    si.valid = valid; si.t = t; si.p = p; si.n = n; si.sh.s = shs; si.sh.t = sht; si.sh.n = shn; si.uv = uv;
    si.dp_du = dp_du; si.dp_dv = dp_dv; si.wi = wi; si.prim = f; si.shape = shp;
    return si;
}

DEV SI GlobalTracer::surface(SceneRef s, const Ray &r, const Hit &h) const { return compute_si(s, r, h); }
template <int STRIDE> DEV SI LdsTracer<STRIDE>::surface(SceneRef s, const Ray &r, const Hit &h) const { return compute_si(s, r, h, &L); }

// ------------------------------------------------------------------ spheres
// Sphere shapes (src/shapes/sphere.cpp) in float32: llvm_ad_rgb takes the `is_diff_v` branch of ray_intersect_preliminary_impl
// and compute_surface_interaction.  A scene holds a few spheres, kept out of the triangle BVH and read through scalar loads
// (the loop index is wave-uniform); a hit on sphere k is primitive n_faces + k, u = v = 0.

// include/mitsuba/core/math.h:360-400
DEV bool solve_quadratic(float a, float b, float c, float &x0, float &x1) {
    const bool linear_case = a == 0.f, valid_linear = linear_case && b != 0.f;
    x0 = x1 = -c / b;
    const float discrim = fma_(b, b, -(4.f * a * c));
    const bool valid_quadratic = !linear_case && discrim >= 0.f;
    const float sqrt_discrim = __builtin_sqrtf(discrim);
    const float temp = -0.5f * (b + __builtin_copysignf(sqrt_discrim, b));
    const float x0p = temp / a, x1p = c / temp;
    const float x0m = fmin_(x0p, x1p), x1m = fmax_(x0p, x1p);
    if (!linear_case) { x0 = x0m; x1 = x1m; }
    return valid_linear || valid_quadratic;
}
// sphere.cpp:515-572 ray_intersect_preliminary_impl: t of the hit, +inf when there is none
DEV float sphere_intersect(V3 center, float radius, const Ray &r) {
    const V3 l = r.o - center, d = r.d;
    const float plane_t = dot(-l, d) / norm(d);       // the plane through the centre perpendicular to the ray: a robust origin
    const V3 o = fma3(d, plane_t, r.o) - center;
    const float A = squared_norm(d), B = 2.f * dot(o, d), C = squared_norm(o) - sqr(radius);
    float near_t, far_t;
    const bool found = solve_quadratic(A, B, C, near_t, far_t);
    near_t += plane_t; far_t += plane_t;
    const bool out_bounds = !(near_t <= r.maxt && far_t >= 0.f);        // NaN-aware
    const bool in_bounds = near_t < 0.f && far_t > r.maxt;
    const float t = near_t < 0.f ? far_t : near_t;
    return (found && !out_bounds && !in_bounds) ? t : kInf;
}
// sphere.cpp:574-618 ray_test_impl (no plane shift)
DEV bool sphere_test(V3 center, float radius, const Ray &r) {
    const V3 o = r.o - center, d = r.d;
    const float A = squared_norm(d), B = 2.f * dot(o, d), C = squared_norm(o) - sqr(radius);
    float near_t, far_t;
    const bool found = solve_quadratic(A, B, C, near_t, far_t);
    const bool out_bounds = !(near_t <= r.maxt && far_t >= 0.f);
    const bool in_bounds = near_t < 0.f && far_t > r.maxt;
    return found && !out_bounds && !in_bounds;
}
DEV const LRT_CONST DSphere &sphere_ref(SceneRef sc, uint32_t k) { return reinterpret_cast<const LRT_CONST DSphere *>((uintptr_t) sc.spheres)[k]; }
// Closest sphere hit (ties: the lower index)
DEV Hit spheres_closest(SceneRef sc, const Ray &r) {
    Hit best; best.t = kInf; best.u = best.v = 0.f; best.prim = 0xffffffffu;
    const uint32_t ns = sc.n_spheres;
    for (uint32_t k = 0; k < ns; ++k) {
        const LRT_CONST DSphere &S = sphere_ref(sc, k);
        const float t = sphere_intersect(V3(S.center[0], S.center[1], S.center[2]), S.radius, r);
        if (t < best.t) { best.t = t; best.prim = sc.n_faces + k; }
    }
    return best;
}
DEV bool spheres_any(SceneRef sc, const Ray &r) {
    const uint32_t ns = sc.n_spheres;
    bool hit = false;
    for (uint32_t k = 0; k < ns; ++k) {
        const LRT_CONST DSphere &S = sphere_ref(sc, k);
        hit = hit || sphere_test(V3(S.center[0], S.center[1], S.center[2]), S.radius, r);
    }
    return hit;
}
// Closest hit over spheres and triangles: the spheres first, their t tightens maxt for the BVH walk (a triangle at the same t
// wins, the lower primitive index).  Any hit: the spheres first, early return.
template <bool ANY_HIT, class WALK> DEV Hit trace_ext(SceneRef sc, const Ray &r, const WALK &walk) {
    if (ANY_HIT) {
        if (spheres_any(sc, r)) { Hit h; h.t = 0.f; h.u = h.v = 0.f; h.prim = sc.n_faces; return h; }
        return walk(r);
    }
    const Hit s = spheres_closest(sc, r);
    Ray r2 = r; r2.maxt = fmin_(r.maxt, s.t);
    const Hit h = walk(r2);
    return h.prim != 0xffffffffu ? h : s;
}

// src/core/vector.h dir_to_sph -> unit_angle_z (Dr.Jit: 2 asin(|v - (0, 0, sign z)| / 2), mirrored for z < 0)
DEV float unit_angle_z(V3 v) {
    const float temp = 2.f * m_asin(.5f * norm(V3(v.x, v.y, v.z - signf_(v.z))));
    return v.z >= 0.f ? temp : kPi - temp;
}
// sphere.cpp:626-740 compute_surface_interaction, the IsDiff / !follow_shape branch: p = ray(t) without re-projection
DEV SI compute_si_sphere(SceneRef sc, const Ray &r, const Hit &h) {
    const uint32_t k = h.prim - sc.n_faces;
    const DSphere S = tab(reinterpret_cast<const DSphere *>(sc.spheres), k);
    const V3 c(S.center[0], S.center[1], S.center[2]);
    SI si;
    si.valid = true; si.t = h.t;
    si.p = fma3(r.d, h.t, r.o);
    V3 n = normalize(si.p - c);
    const V3 local = xform_point12(S.to_object, si.p);
    const float theta = unit_angle_z(local);
    float phi = m_atan2(local.y, local.x);
    if (phi < 0.f) phi += 2.f * kPi;
    si.uv = { phi * kInvTwoPi, theta * kInvPi };
    V3 dp_du(-local.y, local.x, 0.f);
    const float rd = __builtin_sqrtf(sqr(local.x) + sqr(local.y)), inv_rd = rcp(rd);
    const float cos_phi = local.x * inv_rd, sin_phi = local.y * inv_rd;
    V3 dp_dv(local.z * cos_phi, local.z * sin_phi, -rd);
    if (rd == 0.f) dp_dv = V3(1.f, 0.f, 0.f);
    si.dp_du = xform_vec9(S.to_world, dp_du) * (2.f * kPi);
    si.dp_dv = xform_vec9(S.to_world, dp_dv) * kPi;
    if (S.flip_normals) n = V3(-n.x, -n.y, -n.z);
    si.n = n; si.sh.n = n;
    // shading frame as for meshes (compute_si above)
    V3 shs = normalize(fma3(n, -dot(n, si.dp_du), si.dp_du));
    if (si.dp_du.x == 0.f && si.dp_du.y == 0.f && si.dp_du.z == 0.f) shs = coordinate_system(n).s;
    si.sh.s = shs; si.sh.t = cross(n, shs);
    const V3 md(-r.d.x, -r.d.y, -r.d.z);
    si.wi = V3(dot(md, si.sh.s), dot(md, si.sh.t), dot(md, si.sh.n));
    si.prim = h.prim; si.shape = S.shape;
    return si;
}

// The tracer of the EXT kernel instances (scenes with spheres, point emitters or mesh area emitters): a triangle tracer plus the spheres.  The
// other instances keep the plain tracers, so triangle-only scenes run the code they ran before.
template <class BASE> struct ExtTracer {
    static constexpr bool kExt = true;
    const BASE &base; SceneRef sc;
    DEV Hit closest(const Ray &r) const { return trace_ext<false>(sc, r, [&](const Ray &rr) { return base.closest(rr); }); }
    DEV Hit any(const Ray &r) const { return trace_ext<true>(sc, r, [&](const Ray &rr) { return base.any(rr); }); }
    DEV SI surface(SceneRef s, const Ray &r, const Hit &h) const {
        if (h.prim != 0xffffffffu && h.prim >= s.n_faces) return compute_si_sphere(s, r, h);
        return base.surface(s, r, h);
    }
};
template <bool SECOND, class A, class B> DEV const auto &pick(const A &a, const B &b) { if constexpr (SECOND) return b; else return a; }
// What the hide_emitters loops ask of a hit: its surface (without the LDS shortcut, as they always did) and whether it lies on an
// area emitter.  Spheres carry none (the loader refuses an area light on a sphere).
template <class TR> DEV SI surface_of(const TR &, SceneRef sc, const Ray &r, const Hit &h) { return compute_si(sc, r, h); }
template <class B> DEV SI surface_of(const ExtTracer<B> &tr, SceneRef sc, const Ray &r, const Hit &h) { return tr.surface(sc, r, h); }
template <class TR> DEV bool hit_on_emitter(const TR &, SceneRef sc, const Hit &h) {
    return h.prim != 0xffffffffu && tab(sc.shapes, sc.face_shape[h.prim], sc.one_shape).emitter >= 0;
}
template <class B> DEV bool hit_on_emitter(const ExtTracer<B> &, SceneRef sc, const Hit &h) {
    return h.prim != 0xffffffffu && h.prim < sc.n_faces && tab(sc.shapes, sc.face_shape[h.prim], sc.one_shape).emitter >= 0;
}

// include/mitsuba/render/interaction.h:140-168
DEV V3 offset_p(V3 p, V3 n, V3 d) {
    float mag = (1.f + max3(abs3(p))) * kRayEpsilon;
    mag = mulsign(mag, dot(n, d));
    return fma3(n, mag, p);
}
DEV Ray spawn_ray(V3 p, V3 n, V3 d) { Ray r; r.o = offset_p(p, n, d); r.d = d; r.maxt = kLargest; return r; }
DEV Ray spawn_ray_to(V3 p, V3 n, V3 t) {
    Ray r; r.o = offset_p(p, n, t - p);
    V3 d = t - r.o; float dist = norm(d);
    r.d = d / dist; r.maxt = dist * (1.f - kShadowEpsilon);
    return r;
}

// --------------------------------------------------------------- warping
// include/mitsuba/core/warp.h:54-92, :412-420, :250-256
DEV V2 square_to_uniform_disk_concentric(float sx, float sy) {
    float x = fma_(2.f, sx, -1.f), y = fma_(2.f, sy, -1.f);
    bool is_zero = (x == 0.f) && (y == 0.f), q13 = __builtin_fabsf(x) < __builtin_fabsf(y);
    float r = q13 ? y : x, rp = q13 ? x : y;
    float phi = 0.25f * kPi * rp / r;
    if (q13) phi = 0.5f * kPi - phi;
    if (is_zero) phi = 0.f;
    float s, c; m_sincos(phi, &s, &c);
    return { r * c, r * s };
}
DEV V3 square_to_cosine_hemisphere(float sx, float sy) {
    V2 p = square_to_uniform_disk_concentric(sx, sy);
    float z = safe_sqrt(1.f - fma_(p.x, p.x, p.y * p.y));
    return V3(p.x, p.y, z);
}
DEV V3 square_to_uniform_sphere(float sx, float sy) {
    float z = fma_(-2.f, sy, 1.f), r = safe_sqrt(fma_(-z, z, 1.f));
    float s, c; m_sincos(2.f * kPi * sx, &s, &c);
    return V3(r * c, r * s, z);
}

// -------------------------------------------------------------- textures
DEV V3 tex_eval(SceneRef sc, int tex, const SI &si) {
    const DTexture &T = sc.textures[tex];
    if (T.type == LRT_TEX_CHECKERBOARD) {        // src/textures/checkerboard.cpp:70-88
        float u = fma_(T.to_uv[1], si.uv.y, fma_(T.to_uv[0], si.uv.x, T.to_uv[2]));
        float v = fma_(T.to_uv[4], si.uv.y, fma_(T.to_uv[3], si.uv.x, T.to_uv[5]));
        bool mx = u - __builtin_floorf(u) > .5f, my = v - __builtin_floorf(v) > .5f;
        return (mx == my) ? V3(T.color0[0], T.color0[1], T.color0[2]) : V3(T.color1[0], T.color1[1], T.color1[2]);
    }
    if (T.type == LRT_TEX_RGB) return V3(T.color0[0], T.color0[1], T.color0[2]);
    return V3(0.f);
}

// src/textures/bitmap.cpp:509-578 eval_1_grad; texels hold the per-texel
// luminance (precomputed on the host with the same float expression).
DEV V2 tex_eval_1_grad(SceneRef sc, int tex, const SI &si) {
    const DTexture &T = sc.textures[tex];
    if (T.type != LRT_TEX_BITMAP) return { 0.f, 0.f };
    float u = fma_(T.to_uv[1], si.uv.y, fma_(T.to_uv[0], si.uv.x, T.to_uv[2]));
    float v = fma_(T.to_uv[4], si.uv.y, fma_(T.to_uv[3], si.uv.x, T.to_uv[5]));
    int w = T.width, h = T.height;
    float fx = fma_(u, (float) w, -0.5f), fy = fma_(v, (float) h, -0.5f);
    int ix = (int) __builtin_floorf(fx), iy = (int) __builtin_floorf(fy);
    float w1x = fx - (float) ix, w1y = fy - (float) iy, w0x = 1.f - w1x, w0y = 1.f - w1y;
    int x0 = ix % w; if (x0 < 0) x0 += w; int x1 = (ix + 1) % w; if (x1 < 0) x1 += w;
    int y0 = iy % h; if (y0 < 0) y0 += h; int y1 = (iy + 1) % h; if (y1 < 0) y1 += h;
    const float *d = sc.tex_data + T.data_offset;
    float f00 = d[y0 * w + x0], f10 = d[y0 * w + x1], f01 = d[y1 * w + x0], f11 = d[y1 * w + x1];
    float dx = fma_(w0y, f10 - f00, w1y * (f11 - f01)), dy = fma_(w0x, f01 - f00, w1x * (f11 - f10));
    float du = T.to_uv[0] * dx + T.to_uv[3] * dy, dv = T.to_uv[1] * dx + T.to_uv[4] * dy;
    return { (float) w * du, (float) h * dv };
}

// ----------------------------------------------------------------- BSDFs
enum { F_DELTA = 1, F_SMOOTH = 2, F_NULL = 4 };
struct BSDFSample { V3 wo; float pdf, eta; int type; V3 weight; };

// include/mitsuba/render/fresnel.h:35-73
DEV void fresnel(float cos_theta_i, float eta, float *r, float *cos_theta_t, float *eta_it, float *eta_ti) {
    bool outside = cos_theta_i >= 0.f;
    float rcp_eta = rcp(eta);
    *eta_it = outside ? eta : rcp_eta; *eta_ti = outside ? rcp_eta : eta;
    float cos_theta_t_sqr = fma_(-fma_(-cos_theta_i, cos_theta_i, 1.f), *eta_ti * *eta_ti, 1.f);
    float cti = __builtin_fabsf(cos_theta_i), ctt = safe_sqrt(cos_theta_t_sqr);
    bool index_matched = eta == 1.f, special = index_matched || cti == 0.f;
    float r_sc = index_matched ? 0.f : 1.f;
    float a_s = fma_(-*eta_it, ctt, cti) / fma_(*eta_it, ctt, cti);
    float a_p = fma_(-*eta_it, cti, ctt) / fma_(*eta_it, cti, ctt);
    float rr = 0.5f * (sqr(a_s) + sqr(a_p));
    if (special) rr = r_sc;
    *r = rr; *cos_theta_t = mulsign_neg(ctt, cos_theta_i);
}

// src/bsdfs/bumpmap.cpp:226-251
DEV Frame bump_frame(SceneRef sc, const DBsdf &B, const SI &si) {
    V2 g = tex_eval_1_grad(sc, B.texture, si);
    float gx = B.scale * g.x, gy = B.scale * g.y;
    V3 dp_du = fma3(si.sh.n, gx - dot(si.sh.n, si.dp_du), si.dp_du);
    V3 dp_dv = fma3(si.sh.n, gy - dot(si.sh.n, si.dp_dv), si.dp_dv);
    Frame r;
    r.n = normalize(cross(dp_du, dp_dv));
    if (dot(si.n, r.n) < 0.f) r.n = r.n * -1.f;
    r.n = si.sh.to_local(r.n);
    if (si.wi.z * dot(si.wi, r.n) <= 0.f) r.n = V3(-r.n.x, -r.n.y, r.n.z);
    r.s = normalize(fma3(r.n, -dot(r.n, si.dp_du), si.dp_du));
    r.t = cross(r.n, r.s);
    return r;
}
DEV float tan_theta_2(V3 v) { float t = fma_(-v.z, v.z, 1.f); return fmax_(t, 0.f) / sqr(v.z); }
DEV float shadow_terminator(V3 pn, V3 wo) {       // src/bsdfs/normalmap_helpers.h:20-25
    float alpha2 = fmin_(0.125f * tan_theta_2(pn), 1.f);
    return 2.f / (1.f + __builtin_sqrtf(1.f + alpha2 * tan_theta_2(wo)));
}

// ------------------------------------------------- roughdielectric (src/bsdfs/roughdielectric.cpp)
// Compiled into the EXT instances, the bsdf probe (probes.h) and k_math_eval (fn 9, 10) alone (leaf_sample / leaf_eval / leaf_pdf below).
// erf: |x| < 1 the odd polynomial of Cephes' single-precision erff (ndtrf.c, table T), beyond it Abramowitz & Stegun 7.1.26
// (|error| <= 1.5e-7).  erfinv: M. Giles, "Approximating the erfinv function" (GPU Computing Gems, Jade edition, 2012), the
// single-precision pair of polynomials in w = -log((1 - x)(1 + x)).  Both stand in for Dr.Jit's dr::erf / dr::erfinv
// (microfacet.h:382-404); they are held to float64 through lrt_math_eval fn 9 / 10.
DEV float m_erf(float x) {
    const float a = __builtin_fabsf(x);
    if (a < 1.f) {
        const float z = x * x;
        float p = 7.853861353153693E-5f;
        p = fma_(p, z, -8.010193625184903E-4f);
        p = fma_(p, z, 5.188327685732524E-3f);
        p = fma_(p, z, -2.685381193529856E-2f);
        p = fma_(p, z, 1.128358514861418E-1f);
        p = fma_(p, z, -3.761262582423300E-1f);
        p = fma_(p, z, 1.128379165726710E+0f);
        return x * p;
    }
    const float t = rcp(fma_(0.3275911f, a, 1.f));
    float q = 1.061405429f;
    q = fma_(q, t, -1.453152027f);
    q = fma_(q, t, 1.421413741f);
    q = fma_(q, t, -0.284496736f);
    q = fma_(q, t, 0.254829592f);
    const float r = fma_(-(q * t), m_exp(-(a * a)), 1.f);
    return mulsign(r, x);                        // (NaN stays NaN: the comparison above fails, t and r are NaN)
}
DEV float m_erfinv(float x) {
    float w = -m_log((1.f - x) * (1.f + x)), p;
    if (w < 5.f) {
        w -= 2.5f;
        p = 2.81022636e-08f;
        p = fma_(p, w, 3.43273939e-07f);
        p = fma_(p, w, -3.5233877e-06f);
        p = fma_(p, w, -4.39150654e-06f);
        p = fma_(p, w, 0.00021858087f);
        p = fma_(p, w, -0.00125372503f);
        p = fma_(p, w, -0.00417768164f);
        p = fma_(p, w, 0.246640727f);
        p = fma_(p, w, 1.50140941f);
    } else {
        w = __builtin_sqrtf(w) - 3.f;
        p = -0.000200214257f;
        p = fma_(p, w, 0.000100950558f);
        p = fma_(p, w, 0.00134934322f);
        p = fma_(p, w, -0.00367342844f);
        p = fma_(p, w, 0.00573950773f);
        p = fma_(p, w, -0.0076224613f);
        p = fma_(p, w, 0.00943887047f);
        p = fma_(p, w, 1.00167406f);
        p = fma_(p, w, 2.83297682f);
    }
    return p * x;
}

// MicrofacetDistribution (include/mitsuba/render/microfacet.h:174-440).  One set-up (microfacet_of) serves sample, eval and pdf.
struct Microfacet {
    float au, av; bool ggx, visible;
    DEV void scale_alpha(float v) { au *= v; av *= v; }                           // :174-177
    DEV float eval(V3 m) const {                                                  // :185-207
        const float alpha_uv = au * av, cos_theta = m.z, cos_theta_2 = sqr(cos_theta);
        const float e = sqr(m.x / au) + sqr(m.y / av);
        float result;
        if (!ggx) result = m_exp(-e / cos_theta_2) / (kPi * alpha_uv * sqr(cos_theta_2));
        else result = rcp(kPi * alpha_uv * sqr(e + sqr(m.z)));
        return result * cos_theta > 1e-20f ? result : 0.f;
    }
    DEV float smith_g1(V3 v, V3 m) const {                                        // :341-365
        const float xy_alpha_2 = sqr(au * v.x) + sqr(av * v.y), tan_theta_alpha_2 = xy_alpha_2 / sqr(v.z);
        float result;
        if (!ggx) {
            const float a = rsqrt_(tan_theta_alpha_2), a_sqr = sqr(a);
            result = a >= 1.6f ? 1.f : (3.535f * a + 2.181f * a_sqr) / (1.f + 2.276f * a + 2.577f * a_sqr);
        } else result = 2.f / (1.f + __builtin_sqrtf(1.f + tan_theta_alpha_2));
        if (xy_alpha_2 == 0.f) result = 1.f;
        if (dot(v, m) * v.z <= 0.f) result = 0.f;
        return result;
    }
    DEV float G(V3 wi, V3 wo, V3 m) const { return smith_g1(wi, m) * smith_g1(wo, m); }   // :329-331
    DEV float pdf(V3 wi, V3 m) const {                                            // :219-228
        float result = eval(m);
        if (visible) result *= smith_g1(wi, m) * __builtin_fabsf(dot(wi, m)) / wi.z;
        else result *= m.z;
        return result;
    }
    // sin_theta_i: of the same direction, from the caller (formed as sqrt(x^2 + y^2), which keeps its relative accuracy near normal incidence where
    // the reference's sqrt(1 - cos^2) cancels)
    DEV V2 sample_visible_11(float cos_theta_i, float sin_theta_i, float sx, float sy) const {        // :368-421
        if (!ggx) {
            const float tan_theta_i = sin_theta_i / cos_theta_i, cot_theta_i = rcp(tan_theta_i);
            const float maxval = m_erf(cot_theta_i);
            sx = fmax_(fmin_(sx, 1.f - 1e-6f), 1e-6f); sy = fmax_(fmin_(sy, 1.f - 1e-6f), 1e-6f);
            float x = maxval - (maxval + 1.f) * m_erf(__builtin_sqrtf(-m_log(sx)));
            const float kInvSqrtPi = 0.56418958354775628695f;
            sx *= 1.f + maxval + kInvSqrtPi * tan_theta_i * m_exp(-sqr(cot_theta_i));
            for (int i = 0; i < 3; ++i) {                                         // three Newton steps
                const float slope = m_erfinv(x);
                const float value = 1.f + x + kInvSqrtPi * tan_theta_i * m_exp(-sqr(slope)) - sx, derivative = 1.f - slope * tan_theta_i;
                x -= value / derivative;
            }
            return { m_erfinv(x), m_erfinv(fma_(2.f, sy, -1.f)) };
        }
        V2 p = square_to_uniform_disk_concentric(sx, sy);
        const float s = .5f * (1.f + cos_theta_i);
        p.y = lerpf(safe_sqrt(1.f - sqr(p.x)), p.y, s);
        const float x = p.x, y = p.y, z = safe_sqrt(1.f - fma_(p.x, p.x, p.y * p.y));
        const float nrm = rcp(fma_(sin_theta_i, y, cos_theta_i * z));
        return { fma_(cos_theta_i, y, -(sin_theta_i * z)) * nrm, x * nrm };
    }
    DEV V3 sample(V3 wi, float sx, float sy, float *pdf_out) const {               // :244-326
        if (!visible) {
            float sin_phi, cos_phi, cos_theta, cos_theta_2, alpha_2, pdf, tan_theta_2;
            if (au == av) {
                m_sincos(kTwoPi * sy, &sin_phi, &cos_phi);
                alpha_2 = au * au;
            } else {
                float st, ct; m_sincos(kTwoPi * sy, &st, &ct);                  // (dr::tan)
                const float ratio = av / au, tmp = ratio * (st / ct);
                cos_phi = rsqrt_(fma_(tmp, tmp, 1.f));
                cos_phi = mulsign(cos_phi, __builtin_fabsf(sy - .5f) - .25f);
                sin_phi = cos_phi * tmp;
                alpha_2 = rcp(sqr(cos_phi / au) + sqr(sin_phi / av));
            }
            if (!ggx) {
                const float lg = m_log(1.f - sx);
                tan_theta_2 = -alpha_2 * lg;
                cos_theta = rsqrt_(fma_(-alpha_2, lg, 1.f));
                cos_theta_2 = sqr(cos_theta);
                const float cos_theta_3 = fmax_(cos_theta_2 * cos_theta, 1e-20f);
                pdf = (1.f - sx) / (kPi * au * av * cos_theta_3);
            } else {
                const float tan_theta_m_2 = alpha_2 * sx / (1.f - sx);
                tan_theta_2 = tan_theta_m_2;
                cos_theta = rsqrt_(1.f + tan_theta_m_2);
                cos_theta_2 = sqr(cos_theta);
                const float temp = 1.f + tan_theta_m_2 / alpha_2, cos_theta_3 = fmax_(cos_theta_2 * cos_theta, 1e-20f);
                pdf = rcp(kPi * au * av * cos_theta_3 * sqr(temp));
            }
            // sin = tan cos, not the reference's sqrt(1 - cos^2): equal, but that one cancels for a small alpha (at the clamp 1e-4 float32 returns
            // the surface normal itself while the pdf keeps its 1 - s_x: weight * pdf then misses eval at the sampled wo by orders of magnitude)
            const float sin_theta = __builtin_sqrtf(tan_theta_2) * cos_theta;
            *pdf_out = pdf;
            return V3(cos_phi * sin_theta, sin_phi * sin_theta, cos_theta);
        }
        const V3 wi_p = normalize(V3(au * wi.x, av * wi.y, wi.z));               // stretch
        const float sin_theta_2 = fma_(wi_p.x, wi_p.x, wi_p.y * wi_p.y), inv_sin_theta = rsqrt_(sin_theta_2);   // Frame3f::sincos_phi (frame.h:111-122); 1 - z^2 there: see sample_visible_11
        float cos_phi = clampf(wi_p.x * inv_sin_theta, -1.f, 1.f), sin_phi = clampf(wi_p.y * inv_sin_theta, -1.f, 1.f);
        if (__builtin_fabsf(sin_theta_2) <= 4.f * kEpsilon) { cos_phi = 1.f; sin_phi = 0.f; }
        const V2 s11 = sample_visible_11(wi_p.z, __builtin_sqrtf(sin_theta_2), sx, sy);
        const float slx = fma_(cos_phi, s11.x, -(sin_phi * s11.y)) * au, sly = fma_(sin_phi, s11.x, cos_phi * s11.y) * av;   // rotate, unstretch
        const V3 m = normalize(V3(-slx, -sly, 1.f));
        *pdf_out = eval(m) * smith_g1(wi, m) * __builtin_fabsf(dot(wi, m)) / wi.z;
        return m;
    }
};
DEV Microfacet microfacet_of(const DBsdf &B) { Microfacet d; d.au = B.alpha_u; d.av = B.alpha_v; d.ggx = (B.micro & LRT_MICRO_GGX) != 0; d.visible = (B.micro & LRT_MICRO_VISIBLE) != 0; return d; }

// roughdielectric.cpp:242-358 sample(), radiance mode, both lobes enabled
DEV BSDFSample rough_sample(SceneRef sc, const DBsdf &B, const SI &si, V3 wi, float s1, float s2x, float s2y) {
    BSDFSample bs;
    bs.wo = V3(0.f); bs.pdf = 0.f; bs.eta = 0.f; bs.type = 0; bs.weight = V3(0.f);
    const float cos_theta_i = wi.z;
    bool active = cos_theta_i != 0.f;
    const Microfacet distr = microfacet_of(B);
    Microfacet sample_distr = distr;
    if (!distr.visible) sample_distr.scale_alpha(1.2f - .2f * __builtin_sqrtf(__builtin_fabsf(cos_theta_i)));
    float pdf;
    const V3 m = sample_distr.sample(V3(mulsign(wi.x, cos_theta_i), mulsign(wi.y, cos_theta_i), mulsign(wi.z, cos_theta_i)), s2x, s2y, &pdf);
    active = active && pdf != 0.f;
    float F, cos_theta_t, eta_it, eta_ti;
    const float wi_m = dot(wi, m);
    fresnel(wi_m, B.eta, &F, &cos_theta_t, &eta_it, &eta_ti);
    const bool selected_r = s1 <= F && active;
    pdf *= selected_r ? F : 1.f - F;
    bs.eta = selected_r ? 1.f : eta_it;
    bs.type = F_SMOOTH;                                                         // GlossyReflection / GlossyTransmission: both smooth
    V3 weight(1.f); float dwh_dwo;
    if (selected_r) {
        bs.wo = V3(fma_(m.x, 2.f * wi_m, -wi.x), fma_(m.y, 2.f * wi_m, -wi.y), fma_(m.z, 2.f * wi_m, -wi.z));      // reflect(wi, m), fresnel.h:282-284
        if (B.specular_reflectance >= 0) weight = tex_eval(sc, B.specular_reflectance, si);
        dwh_dwo = rcp(4.f * dot(bs.wo, m));
    } else {
        const float k = fma_(wi_m, eta_ti, cos_theta_t);                         // refract(wi, m, cos_theta_t, eta_ti), fresnel.h:311-314
        bs.wo = V3(fma_(m.x, k, -(wi.x * eta_ti)), fma_(m.y, k, -(wi.y * eta_ti)), fma_(m.z, k, -(wi.z * eta_ti)));
        weight = V3(sqr(eta_ti));
        if (B.specular_transmittance >= 0) weight = weight * tex_eval(sc, B.specular_transmittance, si);
        const float wo_m = dot(bs.wo, m);
        dwh_dwo = (sqr(bs.eta) * wo_m) / sqr(wi_m + bs.eta * wo_m);
    }
    if (distr.visible) weight = weight * distr.smith_g1(bs.wo, m);
    else weight = weight * (distr.G(wi, bs.wo, m) * wi_m / (cos_theta_i * m.z));
    bs.pdf = pdf * __builtin_fabsf(dwh_dwo);
    if (!active) { weight = V3(0.f); bs.wo = V3(0.f); bs.pdf = 0.f; }         // neither lobe is selected: wo and dwh_dwo stay 0 (:307-347)
    bs.weight = weight;
    return bs;
}
// roughdielectric.cpp:501-608 eval_pdf(): what eval() (:360-434) and pdf() (:436-499) return, from one half-vector and one distribution
DEV void rough_eval_pdf(SceneRef sc, const DBsdf &B, const SI &si, V3 wi, V3 wo, V3 *value_out, float *pdf_out) {
    const float cos_theta_i = wi.z, cos_theta_o = wo.z;
    bool active = cos_theta_i != 0.f;
    const bool reflect = cos_theta_i * cos_theta_o > 0.f;
    const float inv_m_eta = rcp(B.eta);
    const float eta = cos_theta_i > 0.f ? B.eta : inv_m_eta, inv_eta = cos_theta_i > 0.f ? inv_m_eta : B.eta;
    V3 m = normalize(wi + wo * (reflect ? 1.f : eta));
    m = V3(mulsign(m.x, m.z), mulsign(m.y, m.z), __builtin_fabsf(m.z));
    const float wi_m = dot(wi, m), wo_m = dot(wo, m);
    Microfacet distr = microfacet_of(B);
    const float D = distr.eval(m);
    float F, ctt, e0, e1; fresnel(wi_m, B.eta, &F, &ctt, &e0, &e1);
    const float G = distr.G(wi, wo, m);
    V3 result(0.f);
    if (active && reflect) {
        result = V3(F * D * G / (4.f * __builtin_fabsf(cos_theta_i)));
        if (B.specular_reflectance >= 0) result = result * tex_eval(sc, B.specular_reflectance, si);
    } else if (active) {
        const float scale = sqr(inv_eta);
        result = V3(__builtin_fabsf((scale * (1.f - F) * D * G * eta * eta * wi_m * wo_m) / (cos_theta_i * sqr(wi_m + eta * wo_m))));
        if (B.specular_transmittance >= 0) result = result * tex_eval(sc, B.specular_transmittance, si);
    }
    *value_out = result;
    active = active && wi_m * cos_theta_i > 0.f && wo_m * cos_theta_o > 0.f;
    if (!distr.visible) distr.scale_alpha(1.2f - .2f * __builtin_sqrtf(__builtin_fabsf(cos_theta_i)));
    float pdf = distr.pdf(V3(mulsign(wi.x, cos_theta_i), mulsign(wi.y, cos_theta_i), mulsign(wi.z, cos_theta_i)), m);
    pdf *= reflect ? F : 1.f - F;
    const float dwh_dwo = reflect ? rcp(4.f * wo_m) : (eta * eta * wo_m) / sqr(wi_m + eta * wo_m);
    *pdf_out = active ? pdf * __builtin_fabsf(dwh_dwo) : 0.f;
}

// ------------------------------------------------- conductor, plastic, twosided (src/bsdfs/conductor.cpp, plastic.cpp, twosided.cpp)
// Compiled into the EXT instances, the bsdf probe (probes.h) and the EXT aov kernels alone, like the roughdielectric.  X: the BSDF's row of DScene::bsdf_ext.
DEV BSDFSample bsdf_sample_zero() { BSDFSample bs; bs.wo = V3(0.f); bs.pdf = 0.f; bs.eta = 0.f; bs.type = 0; bs.weight = V3(0.f); return bs; }   // dr::zeros<BSDFSample3f>
// include/mitsuba/render/fresnel.h:92-117, one channel.  eta = 0, k = 1 (the plugin's defaults, a perfect mirror) gives exactly 1: temp_1 = -(1 + sin^2),
// a_2_pb_2 = sqrt(temp_1^2) = -temp_1, a = 0, so r_s = term_1 / term_1 and r_p = r_s * term_3 / term_3.
DEV float fresnel_conductor(float cos_theta_i, float eta_r, float eta_i) {
    const float cos_theta_i_2 = cos_theta_i * cos_theta_i, sin_theta_i_2 = 1.f - cos_theta_i_2, sin_theta_i_4 = sin_theta_i_2 * sin_theta_i_2;
    const float temp_1 = eta_r * eta_r - eta_i * eta_i - sin_theta_i_2;
    const float a_2_pb_2 = safe_sqrt(temp_1 * temp_1 + 4.f * eta_i * eta_i * eta_r * eta_r);
    const float a = safe_sqrt(.5f * (a_2_pb_2 + temp_1));
    const float term_1 = a_2_pb_2 + cos_theta_i_2, term_2 = 2.f * cos_theta_i * a;
    const float r_s = (term_1 - term_2) / (term_1 + term_2);
    const float term_3 = a_2_pb_2 * cos_theta_i_2 + sin_theta_i_4, term_4 = term_2 * sin_theta_i_2;
    const float r_p = r_s * (term_3 - term_4) / (term_3 + term_4);
    return 0.5f * (r_s + r_p);
}
// conductor.cpp:247-307 sample(), unpolarized; eval() and pdf() are 0 (:309-317)
DEV BSDFSample conductor_sample(SceneRef sc, const DBsdf &B, const DBsdfExt &X, const SI &si, V3 wi) {
    BSDFSample bs = bsdf_sample_zero();
    const float cos_theta_i = wi.z;
    if (!(cos_theta_i > 0.f)) return bs;
    bs.type = F_DELTA; bs.wo = V3(-wi.x, -wi.y, wi.z); bs.eta = 1.f; bs.pdf = 1.f;       // reflect(wi), fresnel.h:269-271
    const V3 reflectance = tex_eval(sc, B.specular_reflectance, si);
    bs.weight = V3(reflectance.x * fresnel_conductor(cos_theta_i, X.eta[0], X.k[0]), reflectance.y * fresnel_conductor(cos_theta_i, X.eta[1], X.k[1]),
                   reflectance.z * fresnel_conductor(cos_theta_i, X.eta[2], X.k[2]));
    return bs;
}
DEV float fresnel_r(float cos_theta_i, float eta) { float r, ctt, e0, e1; fresnel(cos_theta_i, eta, &r, &ctt, &e0, &e1); return r; }
// the diffuse base with its internal scattering, plastic.cpp:264-265 / :290-291: diff /= 1 - (nonlinear ? diff * fdr_int : fdr_int)
DEV V3 plastic_base(SceneRef sc, const DBsdf &B, const DBsdfExt &X, const SI &si) {
    const V3 d = tex_eval(sc, B.reflectance, si);
    if (X.nonlinear) return V3(d.x / (1.f - d.x * X.fdr_int), d.y / (1.f - d.y * X.fdr_int), d.z / (1.f - d.z * X.fdr_int));
    const float den = 1.f - X.fdr_int;
    return V3(d.x / den, d.y / den, d.z / den);
}
// plastic.cpp:209-271 sample(), both components enabled: the 1-D sample chooses the lobe
DEV BSDFSample plastic_sample(SceneRef sc, const DBsdf &B, const DBsdfExt &X, const SI &si, V3 wi, float s1, float s2x, float s2y) {
    BSDFSample bs = bsdf_sample_zero();
    const float cos_theta_i = wi.z;
    if (!(cos_theta_i > 0.f)) return bs;
    const float f_i = fresnel_r(cos_theta_i, B.eta);
    float prob_specular = f_i * X.spec_weight, prob_diffuse = (1.f - f_i) * (1.f - X.spec_weight);
    prob_specular = prob_specular / (prob_specular + prob_diffuse);
    prob_diffuse = 1.f - prob_specular;
    bs.eta = 1.f;
    if (s1 < prob_specular) {
        bs.wo = V3(-wi.x, -wi.y, wi.z); bs.pdf = prob_specular; bs.type = F_DELTA;
        V3 value(f_i / bs.pdf);
        if (X.specular_reflectance >= 0) value = value * tex_eval(sc, X.specular_reflectance, si);
        bs.weight = value;
    } else {
        bs.wo = square_to_cosine_hemisphere(s2x, s2y);
        bs.pdf = prob_diffuse * (kInvPi * bs.wo.z); bs.type = F_SMOOTH;
        const float f_o = fresnel_r(bs.wo.z, B.eta);
        bs.weight = plastic_base(sc, B, X, si) * (X.inv_eta_2 * (1.f - f_i) * (1.f - f_o) / prob_diffuse);
    }
    return bs;
}
// plastic.cpp:325-360 eval_pdf(): what eval() (:273-297) and pdf() (:299-323) return, operation for operation
DEV void plastic_eval_pdf(SceneRef sc, const DBsdf &B, const DBsdfExt &X, const SI &si, V3 wi, V3 wo, V3 *value_out, float *pdf_out) {
    *value_out = V3(0.f); *pdf_out = 0.f;
    const float cos_theta_i = wi.z, cos_theta_o = wo.z;
    if (!(cos_theta_i > 0.f && cos_theta_o > 0.f)) return;
    const float f_i = fresnel_r(cos_theta_i, B.eta), f_o = fresnel_r(cos_theta_o, B.eta);
    const float hemi_pdf = kInvPi * cos_theta_o;
    *value_out = plastic_base(sc, B, X, si) * (hemi_pdf * X.inv_eta_2 * (1.f - f_i) * (1.f - f_o));
    const float prob_specular = f_i * X.spec_weight;
    float prob_diffuse = (1.f - f_i) * (1.f - X.spec_weight);
    prob_diffuse = prob_diffuse / (prob_specular + prob_diffuse);
    *pdf_out = hemi_pdf * prob_diffuse;
}
// twosided.cpp:124-145: the child that serves a hit with this cos theta_i; -1: neither (two children and wi.z = 0: both masks are off).
// One child (the same-child branch, :124-127): it serves both sides.  Either way the child sees (wi.x, wi.y, |wi.z|) and wo.z carries the sign
// of wi.z (`abs` / `mulsign` there, the two negations of the back side here: the same bits).
DEV int twosided_child(SceneRef sc, int b, const DBsdf &B, float wi_z) {
    const int back = sc.bsdf_ext[b].back;
    if (back == B.nested) return back;
    return wi_z > 0.f ? B.nested : (wi_z < 0.f ? back : -1);
}

// Leaf BSDFs (diffuse / dielectric / null; EXT: roughdielectric, conductor and plastic too), evaluated in the frame `wi` is given in.
// DIELECTRIC: the caller has proven that the leaf is a dielectric (the 64-byte-record kernels, closed_records (b) in device.hip): no dispatch.
// EXT: the scene may hold a roughdielectric, a conductor or a plastic (the EXT instances, the bsdf probe of probes.h); without it their code is not compiled in.
// b: the leaf's index, for its row of DScene::bsdf_ext (EXT alone reads it).
template <bool DIELECTRIC = false, bool EXT = false>
DEV BSDFSample leaf_sample(SceneRef sc, const DBsdf &B, const SI &si, V3 wi, float s1, float s2x, float s2y, int b = -1) {
    if (EXT && !DIELECTRIC && B.type == LRT_BSDF_ROUGHDIELECTRIC) return rough_sample(sc, B, si, wi, s1, s2x, s2y);
    if (EXT && !DIELECTRIC && B.type == LRT_BSDF_CONDUCTOR) return conductor_sample(sc, B, tab(sc.bsdf_ext, b, sc.one_shape), si, wi);
    if (EXT && !DIELECTRIC && B.type == LRT_BSDF_PLASTIC) return plastic_sample(sc, B, tab(sc.bsdf_ext, b, sc.one_shape), si, wi, s1, s2x, s2y);
    BSDFSample bs;
    bs.wo = V3(0.f); bs.pdf = 0.f; bs.eta = 0.f; bs.type = 0; bs.weight = V3(0.f);       // dr::zeros<BSDFSample3f>
    if (!DIELECTRIC && B.type == LRT_BSDF_DIFFUSE) {               // src/bsdfs/diffuse.cpp sample()
        if (wi.z > 0.f) {
            bs.wo = square_to_cosine_hemisphere(s2x, s2y);
            bs.pdf = kInvPi * bs.wo.z; bs.eta = 1.f; bs.type = F_SMOOTH;
            if (bs.pdf > 0.f) bs.weight = tex_eval(sc, B.reflectance, si);
        }
    } else if (DIELECTRIC || B.type == LRT_BSDF_DIELECTRIC) {     // src/bsdfs/dielectric.cpp:230-367
        float r_i, ctt, eta_it, eta_ti;
        fresnel(wi.z, B.eta, &r_i, &ctt, &eta_it, &eta_ti);
        float t_i = 1.f - r_i;
        bool sel_r = s1 <= r_i;
        bs.pdf = sel_r ? r_i : t_i;
        bs.type = F_DELTA;
        bs.wo = sel_r ? V3(-wi.x, -wi.y, wi.z) : V3(-eta_ti * wi.x, -eta_ti * wi.y, ctt);
        bs.eta = sel_r ? 1.f : eta_it;
        bs.weight = V3(1.f);
        if (!sel_r) bs.weight = bs.weight * sqr(eta_ti);
    } else {                                       // src/bsdfs/null.cpp sample()
        // ROCm 7.2 / gfx950 code generation drops the negated z component when this branch's values meet the
        // other branches' phis (reproducer: scripts/dbg/t_null.hip); the empty asm keeps them in their own VGPRs.
        float nx = -wi.x, ny = -wi.y, nz = -wi.z;
        asm volatile("" : "+v"(nx), "+v"(ny), "+v"(nz));
        bs.wo = V3(nx, ny, nz); bs.type = F_NULL; bs.eta = 1.f; bs.pdf = 1.f; bs.weight = V3(1.f);
    }
    return bs;
}
template <bool EXT = false>
DEV V3 leaf_eval(SceneRef sc, const DBsdf &B, const SI &si, V3 wi, V3 wo, int b = -1) {
    if (EXT && B.type == LRT_BSDF_ROUGHDIELECTRIC) { V3 v; float p; rough_eval_pdf(sc, B, si, wi, wo, &v, &p); return v; }
    if (EXT && B.type == LRT_BSDF_PLASTIC) { V3 v; float p; plastic_eval_pdf(sc, B, tab(sc.bsdf_ext, b, sc.one_shape), si, wi, wo, &v, &p); return v; }
    if (B.type == LRT_BSDF_DIFFUSE) {
        if (!(wi.z > 0.f && wo.z > 0.f)) return V3(0.f);
        return tex_eval(sc, B.reflectance, si) * kInvPi * wo.z;
    }
    return V3(0.f);
}
template <bool EXT = false>
DEV float leaf_pdf(SceneRef sc, const DBsdf &B, const SI &si, V3 wi, V3 wo, int b = -1) {
    if (EXT && B.type == LRT_BSDF_ROUGHDIELECTRIC) { V3 v; float p; rough_eval_pdf(sc, B, si, wi, wo, &v, &p); return p; }
    if (EXT && B.type == LRT_BSDF_PLASTIC) { V3 v; float p; plastic_eval_pdf(sc, B, tab(sc.bsdf_ext, b, sc.one_shape), si, wi, wo, &v, &p); return p; }
    if (B.type == LRT_BSDF_DIFFUSE) return (wi.z > 0.f && wo.z > 0.f) ? kInvPi * wo.z : 0.f;
    return 0.f;
}

// EXT: a twosided (twosided.cpp:111-258) hands the hit to one of its children, a leaf, with |wi.z|, and the sign of wi.z goes onto wo.z: of the
// sample on the way out, of the query on the way in (twosided_child).  Every other BSDF keeps its wi and a sign of +1, which changes no bit.
struct LeafRef { DBsdf B; int b; V3 wi; float sign; bool none; };
template <bool EXT>
DEV LeafRef leaf_of(SceneRef sc, int b, const DBsdf &B, V3 wi) {
    LeafRef r; r.B = B; r.b = b; r.wi = wi; r.sign = 1.f; r.none = false;
    if (EXT && B.type == LRT_BSDF_TWOSIDED) {
        r.b = twosided_child(sc, b, B, wi.z); r.none = r.b < 0;
        r.B = tab(sc.bsdfs, r.none ? B.nested : r.b, sc.one_shape); r.wi.z = __builtin_fabsf(wi.z); r.sign = wi.z;
    }
    return r;
}
template <bool DIELECTRIC = false, bool EXT = false>                 // (every leaf is a dielectric, see leaf_sample)
DEV BSDFSample bsdf_sample(SceneRef sc, int b, const SI &si, float s1, float s2x, float s2y) {
    const DBsdf B = tab(sc.bsdfs, b, sc.one_shape);
    if (B.type == LRT_BSDF_BUMPMAP) {               // src/bsdfs/bumpmap.cpp:138-162
        Frame pf = bump_frame(sc, B, si);
        V3 pwi = pf.to_local(si.wi);
        BSDFSample bs = leaf_sample<DIELECTRIC, EXT>(sc, tab(sc.bsdfs, B.nested, sc.one_shape), si, pwi, s1, s2x, s2y, B.nested);
        bool active = any_nonzero(bs.weight);
        V3 pwo = pf.to_world(bs.wo);
        active = active && (bs.wo.z * pwo.z > 0.f);
        bs.wo = pwo;
        V3 w = bs.weight * shadow_terminator(pf.n, bs.wo);
        bs.weight = active ? w : V3(0.f);
        return bs;
    }
    if constexpr (EXT && !DIELECTRIC) {
        const LeafRef l = leaf_of<true>(sc, b, B, si.wi);
        if (l.none) return bsdf_sample_zero();
        BSDFSample bs = leaf_sample<false, true>(sc, l.B, si, l.wi, s1, s2x, s2y, l.b);
        bs.wo.z = mulsign(bs.wo.z, l.sign);
        return bs;
    } else
        return leaf_sample<DIELECTRIC, EXT>(sc, B, si, si.wi, s1, s2x, s2y);
}
template <bool EXT = false>
DEV V3 bsdf_eval(SceneRef sc, int b, const SI &si, V3 wo) {
    const DBsdf B = tab(sc.bsdfs, b, sc.one_shape);
    if (B.type == LRT_BSDF_BUMPMAP) {               // src/bsdfs/bumpmap.cpp:164-183
        Frame pf = bump_frame(sc, B, si);
        V3 pwi = pf.to_local(si.wi), pwo = pf.to_local(wo);
        if (!(wo.z * pwo.z > 0.f)) return V3(0.f);
        return leaf_eval<EXT>(sc, tab(sc.bsdfs, B.nested, sc.one_shape), si, pwi, pwo, B.nested) * shadow_terminator(pf.n, wo);
    }
    if constexpr (EXT) {
        const LeafRef l = leaf_of<true>(sc, b, B, si.wi);
        if (l.none) return V3(0.f);
        return leaf_eval<true>(sc, l.B, si, l.wi, V3(wo.x, wo.y, mulsign(wo.z, l.sign)), l.b);
    } else
        return leaf_eval<EXT>(sc, B, si, si.wi, wo);
}
template <bool EXT = false>
DEV float bsdf_pdf(SceneRef sc, int b, const SI &si, V3 wo) {
    const DBsdf B = tab(sc.bsdfs, b, sc.one_shape);
    if (B.type == LRT_BSDF_BUMPMAP) {
        Frame pf = bump_frame(sc, B, si);
        V3 pwi = pf.to_local(si.wi), pwo = pf.to_local(wo);
        if (!(wo.z * pwo.z > 0.f)) return 0.f;
        return leaf_pdf<EXT>(sc, tab(sc.bsdfs, B.nested, sc.one_shape), si, pwi, pwo, B.nested);
    }
    if constexpr (EXT) {
        const LeafRef l = leaf_of<true>(sc, b, B, si.wi);
        if (l.none) return 0.f;
        return leaf_pdf<true>(sc, l.B, si, l.wi, V3(wo.x, wo.y, mulsign(wo.z, l.sign)), l.b);
    } else
        return leaf_pdf<EXT>(sc, B, si, si.wi, wo);
}
DEV float bsdf_null_transmission(SceneRef sc, int b) { return tab(sc.bsdfs, b, sc.one_shape).type == LRT_BSDF_NULL ? 1.f : 0.f; }

// -------------------------------------------------------------- emitters
struct DirSample { V3 p, n, d; float pdf, dist; bool delta; int emitter; };

// include/mitsuba/core/distr_2d.h:517-602 + include/mitsuba/core/warp.h:446-494
DEV float interval_to_linear(float v0, float v1, float sample) {
    if (__builtin_fabsf(v0 - v1) > 1e-4f * (v0 + v1))
        return (v0 - safe_sqrt(lerpf(sqr(v0), sqr(v1), sample))) / (v0 - v1);
    return sample;
}
DEV void hier_sample(SceneRef sc, float sx, float sy, float *ox, float *oy, float *pdf) {
    EnvRef E = sc.env;
    sx = clampf(sx, 0.f, 1.f); sy = clampf(sy, 0.f, 1.f);
    uint32_t offx = 0, offy = 0;
    for (int l = E.n_levels - 2; l > 0; --l) {
        offx <<= 1; offy <<= 1;
        uint32_t width = E.level_width[l];
        uint32_t oi = ((offx & 1u) | (((offx & ~1u) | (offy & 1u)) << 1)) + ((offy & ~1u) * width);
        const float4 q = *reinterpret_cast<const float4 *>(sc.env_hier + E.level_offset[l] + oi);   // 2x2 patches are contiguous
        float v00 = q.x, v10 = q.y, v01 = q.z, v11 = q.w;
        sx = clampf(sx, 0.f, 1.f); sy = clampf(sy, 0.f, 1.f);
        float r0 = v00 + v10, r1 = v01 + v11;
        sy *= r0 + r1;
        bool mask = sy > r0;
        if (mask) { offy += 1; sy -= r0; }
        sy /= mask ? r1 : r0;
        float c0 = mask ? v01 : v00, c1 = mask ? v11 : v10;
        sx *= c0 + c1;
        mask = sx > c0;
        if (mask) sx -= c0;
        sx /= mask ? c1 : c0;
        if (mask) offx += 1;
    }
    uint32_t w0 = E.level_width[0];
    const float *l0 = sc.env_hier + E.level_offset[0];
    uint32_t oi = offx + offy * w0;
    float v00 = l0[oi], v10 = l0[oi + 1], v01 = l0[oi + w0], v11 = l0[oi + w0 + 1];
    float r0 = v00 + v10, r1 = v01 + v11;
    sy = interval_to_linear(r0, r1, sy);
    float c0 = lerpf(v00, v01, sy), c1 = lerpf(v10, v11, sy);
    sx = interval_to_linear(c0, c1, sx);
    *pdf = lerpf(c0, c1, sx);
    *ox = ((float) (int) offx + sx) * E.patch_size[0];
    *oy = ((float) (int) offy + sy) * E.patch_size[1];
}
// include/mitsuba/core/distr_2d.h:695-726
DEV float hier_eval(SceneRef sc, float px, float py) {
    EnvRef E = sc.env;
    px = clampf(px, 0.f, 1.f); py = clampf(py, 0.f, 1.f);
    px *= E.inv_patch_size[0]; py *= E.inv_patch_size[1];
    uint32_t ox = min((uint32_t) (int) px, E.max_patch[0]), oy = min((uint32_t) (int) py, E.max_patch[1]);
    px -= (float) (int) ox; py -= (float) (int) oy;
    uint32_t w0 = E.level_width[0];
    const float *l0 = sc.env_hier + E.level_offset[0];
    uint32_t oi = ox + oy * w0;
    float v00 = l0[oi], v10 = l0[oi + 1], v01 = l0[oi + w0], v11 = l0[oi + w0 + 1];
    return lerpf(lerpf(v00, v10, px), lerpf(v01, v11, px), py);
}

// src/emitters/envmap.cpp:528-560
DEV V3 env_eval_uv(SceneRef sc, float u, float v) {
    EnvRef E = sc.env;
    uint32_t rx = E.w, ry = E.h;
    u -= .5f / (float) (rx - 1u);
    u -= __builtin_floorf(u); v -= __builtin_floorf(v);
    u *= (float) (rx - 1u); v *= (float) (ry - 1u);
    uint32_t px = min((uint32_t) u, rx - 2u), py = min((uint32_t) v, ry - 2u);
    float w1x = u - (float) px, w1y = v - (float) py, w0x = 1.f - w1x, w0y = 1.f - w1y;
    uint32_t idx = py * rx + px;
    float4 a = sc.env_data[idx], b = sc.env_data[idx + 1], c = sc.env_data[idx + rx], d = sc.env_data[idx + rx + 1];
    V3 v00(a.x, a.y, a.z), v10(b.x, b.y, b.z), v01(c.x, c.y, c.z), v11(d.x, d.y, d.z);
    V3 t0 = v10 * w1x, t1 = v11 * w1x;
    V3 v0(fma_(w0x, v00.x, t0.x), fma_(w0x, v00.y, t0.y), fma_(w0x, v00.z, t0.z));
    V3 v1(fma_(w0x, v01.x, t1.x), fma_(w0x, v01.y, t1.y), fma_(w0x, v01.z, t1.z));
    V3 t2 = v1 * w1y;
    V3 vv(fma_(w0y, v0.x, t2.x), fma_(w0y, v0.y, t2.y), fma_(w0y, v0.z, t2.z));
    return vv * E.scale;
}
DEV V3 emitter_eval_env(SceneRef sc, V3 dir_world) {
    EnvRef E = sc.env;
    if (E.type == LRT_EMITTER_CONSTANT) return V3(E.radiance[0], E.radiance[1], E.radiance[2]);
    V3 v = xform_vec9(E.to_local, dir_world);           // src/emitters/envmap.cpp:353-362
    float uu = m_atan2(v.x, -v.z) * kInvTwoPi, vv = safe_acos(v.y) * kInvPi;
    return env_eval_uv(sc, uu, vv);
}

// ------------------------------------------------------- mesh area emitters
// DiscreteDistribution::sample (include/mitsuba/core/distr_1d.h:117-135, the JIT predicate) inside Dr.Jit's binary_search, restated
// from Dr.Jit's public header (the reference tree leaves ext/drjit empty): log2i(end - start) + 1 trips over [0, n - 1], each
// middle = (start + end) >> 1, start = pred ? min(middle + 1, end) : start, end = pred ? end : middle.  The trip count depends on n
// alone, so the lanes of a wave that sample one emitter run the same loop.
DEV uint32_t mesh_emitter_search(const float *__restrict__ cdf, uint32_t n, float sum, float value) {
    const float s = value * sum;
    uint32_t start = 0u, end = n - 1u;
    const uint32_t trips = n > 1u ? 32u - (uint32_t) __builtin_clz(n - 1u) : 0u;
    for (uint32_t i = 0; i < trips; ++i) {
        const uint32_t middle = (start + end) >> 1;
        const float c = cdf[middle];
        const bool pred = (c < s || c == 0.f) && c != sum;
        start = pred ? min(middle + 1u, end) : start;
        end = pred ? end : middle;
    }
    return start;
}
// The same loop over [start, end] with `s` already scaled by the distribution's total: ContinuousDistribution::sample (distr_1d.h:429-446, the
// tabulated phase function below) runs it over [valid.x, valid.y] with the same predicate.  (Kept beside mesh_emitter_search, not under it:
// folding the two moved instructions in the kernels that sample mesh emitters, which this addition leaves as they were.)
DEV uint32_t cdf_search(const float *__restrict__ cdf, uint32_t start, uint32_t end, float total, float s) {
    const uint32_t trips = end > start ? 32u - (uint32_t) __builtin_clz(end - start) : 0u;
    for (uint32_t i = 0; i < trips; ++i) {
        const uint32_t middle = (start + end) >> 1;
        const float c = cdf[middle];
        const bool pred = (c < s || c == 0.f) && c != total;
        start = pred ? min(middle + 1u, end) : start;
        end = pred ? end : middle;
    }
    return start;
}
// Mesh::sample_position (src/render/mesh.cpp:861-935): `sy` picks the face (DiscreteDistribution::sample_reuse, distr_1d.h:174-182)
// and is replaced by its re-scaled value, then warp::square_to_uniform_triangle (include/mitsuba/core/warp.h:153-156).
DEV void mesh_emitter_position(SceneRef sc, const DMeshEmitter &M, float sx, float sy, V3 *p_out, V3 *n_out) {
    const float *tab_f = sc.mesh_emitter_tab;
    const uint32_t idx = mesh_emitter_search(tab_f + M.cdf_offset, M.n_faces, M.sum, sy);
    const float pmf = tab_f[M.pmf_offset + idx] * M.normalization;
    const float cdf = idx > 0u ? tab_f[M.cdf_offset + idx - 1u] * M.normalization : 0.f;
    sy = (sy - cdf) / pmf;
    const uint32_t f = M.first_face + idx;
    const uint32_t i0 = sc.faces[3 * f], i1 = sc.faces[3 * f + 1], i2 = sc.faces[3 * f + 2];
    const V3 p0(sc.positions[3 * i0], sc.positions[3 * i0 + 1], sc.positions[3 * i0 + 2]);
    const V3 p1(sc.positions[3 * i1], sc.positions[3 * i1 + 1], sc.positions[3 * i1 + 2]);
    const V3 p2(sc.positions[3 * i2], sc.positions[3 * i2 + 1], sc.positions[3 * i2 + 2]);
    const V3 e0 = p1 - p0, e1 = p2 - p0;
    const float t = safe_sqrt(1.f - sx), bx = 1.f - t, by = t * sy;
    *p_out = V3(fma_(e0.x, bx, fma_(e1.x, by, p0.x)), fma_(e0.y, bx, fma_(e1.y, by, p0.y)), fma_(e0.z, bx, fma_(e1.z, by, p0.z)));
    V3 n;
    if (M.has_normals) {
        const float4 a0 = sc.vattr[2 * (size_t) i0], a1 = sc.vattr[2 * (size_t) i1], a2 = sc.vattr[2 * (size_t) i2];
        const float b0 = 1.f - bx - by;
        n = V3(fma_(a0.x, b0, fma_(a1.x, bx, a2.x * by)), fma_(a0.y, b0, fma_(a1.y, bx, a2.y * by)), fma_(a0.z, b0, fma_(a1.z, bx, a2.z * by)));
    } else n = cross(e0, e1);
    n = normalize(n);
    *n_out = M.flip_normals ? -n : n;
}

// Scene::sample_emitter_direction without visibility test (src/render/scene.cpp:333-383)
// EXT: the scene may hold point emitters or area emitters on meshes (the EXT kernel instances only)
template <bool EXT = false>
DEV V3 sample_emitter_direction(SceneRef sc, V3 ref_p, float sx, float sy, DirSample *ds) {
    uint32_t ne = sc.n_emitters;
    ds->p = V3(0.f); ds->n = V3(0.f); ds->d = V3(0.f); ds->pdf = 0.f; ds->dist = 0.f; ds->delta = false; ds->emitter = -1;
    if (ne == 0) return V3(0.f);
    uint32_t index = 0; float emitter_weight = 1.f, pmf = 1.f;
    if (ne > 1) {
        float scaled = sx * (float) ne;
        index = min((uint32_t) scaled, ne - 1u);
        emitter_weight = (float) ne; sx = scaled - (float) index; pmf = 1.f / (float) ne;
    }
    const DEmitter &E = sc.emitters[index];
    ds->emitter = (int) index;
    V3 spec(0.f);
    if (E.type == LRT_EMITTER_AREA) {
        // src/shapes/rectangle.cpp:181-199 (a mesh: mesh.cpp:861-935), src/render/shape.cpp:343-361, src/emitters/area.cpp:118-168 sample_direction
        const DMeshEmitter M = EXT ? tab(sc.mesh_emitters, index) : DMeshEmitter{};
        if (EXT && M.mesh) {
            mesh_emitter_position(sc, M, sx, sy, &ds->p, &ds->n);
            ds->pdf = M.normalization;
        } else {
            ds->p = xform_point12(E.to_world, V3(fma_(sx, 2.f, -1.f), fma_(sy, 2.f, -1.f), 0.f));
            ds->n = V3(E.n[0], E.n[1], E.n[2]);
            ds->pdf = E.inv_area;
        }
        ds->d = ds->p - ref_p;
        float dist2 = squared_norm(ds->d);
        ds->dist = __builtin_sqrtf(dist2);
        ds->d = ds->d / ds->dist;
        float dp = __builtin_fabsf(dot(ds->d, ds->n)), x = dist2 / dp;
        ds->pdf *= finite_(x) ? x : 0.f;
        bool active = dot(ds->d, ds->n) < 0.f && ds->pdf != 0.f;
        V3 rad(E.radiance[0], E.radiance[1], E.radiance[2]);
        spec = active ? rad / ds->pdf : V3(0.f);
    } else if (EXT && E.type == LRT_EMITTER_POINT) {   // src/emitters/point.cpp:119-148: a delta position, pdf 1, no surface reaches it
        ds->p = V3(E.to_world[3], E.to_world[7], E.to_world[11]);
        ds->pdf = 1.f; ds->delta = true;
        ds->d = ds->p - ref_p;
        const float dist2 = squared_norm(ds->d), inv_dist = rsqrt_(dist2);
        ds->dist = __builtin_sqrtf(dist2);
        ds->d = ds->d * inv_dist;
        spec = V3(E.radiance[0], E.radiance[1], E.radiance[2]) * sqr(inv_dist);
    } else if (EXT && E.type == LRT_EMITTER_SPOT) {    // src/emitters/spot.cpp:176-210: a delta position, pdf 1, n = 0
        const DDeltaEmitter S = tab(sc.delta_emitters, index);      // (one emitter: wave-uniform, scalar loads; several: per lane)
        ds->p = V3(S.pos[0], S.pos[1], S.pos[2]);
        ds->pdf = 1.f; ds->delta = true;
        ds->d = ds->p - ref_p;
        ds->dist = norm(ds->d);
        const float inv_dist = rcp(ds->dist);                        // dr::rcp: dmath.h rcp, a correctly rounded 1 / x
        ds->d = ds->d * inv_dist;
        const V3 local_d = xform_vec9(S.to_local, -ds->d);
        // falloff_curve (spot.cpp:142-150) on the normalised local direction; only the lanes of the transition ring pay the acos (dr::acos: m_acos)
        const float cos_theta = normalize(local_d).z;
        float falloff = 0.f;
        if (cos_theta > S.cos_cutoff) falloff = cos_theta >= S.cos_beam ? 1.f : (S.cutoff - m_acos(cos_theta)) * S.inv_transition;
        V3 radiance(0.f);
        if (falloff > 0.f) {                                         // (`active &= falloff > 0`: the dark lanes skip the texture)
            radiance = V3(E.radiance[0], E.radiance[1], E.radiance[2]);
            if (S.texture >= 0) {                                    // direction_to_uv (spot.cpp:129-134) on local_d as it is, not normalised
                SI tsi; const float den = local_d.z * S.uv_factor;
                tsi.uv.x = .5f + .5f * local_d.x / den; tsi.uv.y = .5f + .5f * local_d.y / den;
                radiance = radiance * tex_eval(sc, S.texture, tsi);
            }
        }
        spec = radiance * (falloff * sqr(inv_dist));
    } else if (EXT && E.type == LRT_EMITTER_DIRECTIONAL) {   // src/emitters/directional.cpp:148-176: a delta direction, pdf 1, n = d
        const DDeltaEmitter S = tab(sc.delta_emitters, index);
        const V3 d(S.dir[0], S.dir[1], S.dir[2]), c(S.bsphere_c[0], S.bsphere_c[1], S.bsphere_c[2]);
        const float radius = fmax_(S.bsphere_r, norm(ref_p - c)), dist = 2.f * radius;
        ds->p = ref_p - d * dist; ds->n = d; ds->d = -d; ds->dist = dist;
        ds->pdf = 1.f; ds->delta = true;
        spec = V3(E.radiance[0], E.radiance[1], E.radiance[2]);
    } else if (E.type == LRT_EMITTER_ENVMAP) {         // src/emitters/envmap.cpp:415-459
        EnvRef EV = sc.env;
        float u, v, pdf; hier_sample(sc, sx, sy, &u, &v, &pdf);
        u += .5f / (float) (EV.w - 1u);
        bool active = pdf > 0.f;
        float theta = v * kPi, phi = u * kTwoPi;
        float st, ct, sp, cp; m_sincos(theta, &st, &ct); m_sincos(phi, &sp, &cp);
        V3 d(cp * st, sp * st, ct);
        d = V3(d.y, d.z, -d.x);
        V3 c(EV.bsphere_c[0], EV.bsphere_c[1], EV.bsphere_c[2]);
        float radius = fmax_(EV.bsphere_r, norm(ref_p - c)), dist = 2.f * radius;
        float inv_sin_theta = safe_rsqrt(fmax_(sqr(d.x) + sqr(d.z), sqr(kEpsilon)));
        d = xform_vec9(EV.to_world, d);
        ds->p = ref_p + d * dist; ds->n = -d;
        ds->pdf = active ? pdf * inv_sin_theta * (1.f / (2.f * sqr(kPi))) : 0.f;
        ds->d = d; ds->dist = dist;
        V3 val = env_eval_uv(sc, u, v);
        spec = active ? val / ds->pdf : V3(0.f);
    } else {                                            // src/emitters/constant.cpp sample_direction
        EnvRef EV = sc.env;
        V3 d = square_to_uniform_sphere(sx, sy);
        V3 c(EV.bsphere_c[0], EV.bsphere_c[1], EV.bsphere_c[2]);
        float radius = fmax_(EV.bsphere_r, norm(ref_p - c)), dist = 2.f * radius;
        ds->p = fma3(d, dist, ref_p); ds->n = -d; ds->pdf = kInvFourPi; ds->d = d; ds->dist = dist;
        spec = V3(E.radiance[0], E.radiance[1], E.radiance[2]) / ds->pdf;
    }
    ds->pdf *= pmf;
    spec = spec * emitter_weight;
    return spec;
}

// DirectionSample(scene, si, ref) + Scene::pdf_emitter_direction
// (include/mitsuba/render/records.h:76-78,173-180, src/render/scene.cpp:395-406, src/render/shape.cpp:363-374, area.cpp:170-197)
// The record's normal is si.sh_frame.n, the interpolated shading normal.  A rectangle's equals si.n; on a mesh with vertex normals
// it does not, and the EXT instances read it there (a mesh emitter samples with the interpolated normal too, mesh.cpp:914-925).
template <bool EXT = false>
DEV float pdf_emitter_direction(SceneRef sc, V3 ref_p, const SI &si, int emitter) {
    V3 rel = si.p - ref_p;
    float dist = norm(rel);
    V3 d = si.valid ? rel / dist : -si.wi;
    float pmf = 1.f / (float) sc.n_emitters;
    const DEmitter &E = sc.emitters[emitter];
    float value;
    if (E.type == LRT_EMITTER_AREA) {
        float pos_pdf = E.inv_area; V3 n = si.n;
        if (EXT) { const DMeshEmitter M = tab(sc.mesh_emitters, (uint32_t) emitter); if (M.mesh) { pos_pdf = M.normalization; n = si.sh.n; } }
        float dp = dot(d, n);
        if (!(dp < 0.f)) return 0.f;
        float adp = __builtin_fabsf(dp);
        value = pos_pdf * (adp != 0.f ? (dist * dist) / adp : 0.f);
    } else if (E.type == LRT_EMITTER_ENVMAP) {          // src/emitters/envmap.cpp:461-475
        EnvRef EV = sc.env;
        V3 dl = xform_vec9(EV.to_local, d);
        float u = m_atan2(dl.x, -dl.z) * kInvTwoPi, v = safe_acos(dl.y) * kInvPi;
        u -= .5f / (float) (EV.w - 1u);
        u -= __builtin_floorf(u); v -= __builtin_floorf(v);
        float inv_sin_theta = safe_rsqrt(fmax_(sqr(dl.x) + sqr(dl.z), sqr(kEpsilon)));
        value = hier_eval(sc, u, v) * inv_sin_theta * (1.f / (2.f * sqr(kPi)));
    } else value = kInvFourPi;
    return value * pmf;
}

DEV int si_emitter(SceneRef sc, const SI &si) { return si.valid ? tab(sc.shapes, si.shape, sc.one_shape).emitter : sc.env.emitter; }
DEV V3 emitter_eval(SceneRef sc, int e, const SI &si) {
    if (!si.valid) return emitter_eval_env(sc, -si.wi);
    const DEmitter &E = sc.emitters[e];                 // src/emitters/area.cpp eval()
    return (si.wi.z > 0.f) ? V3(E.radiance[0], E.radiance[1], E.radiance[2]) : V3(0.f);
}

// exp(-t * c) per channel; a medium whose channels are equal (the usual case: sigma_t = 1 * scale) pays one exponential.  The
// values are the ones the three separate calls give (the same operation on the same operands).
DEV V3 exp_neg(float t, V3 c) {
    const float ex = m_exp(-t * c.x);
    if (c.y == c.x && c.z == c.x) return V3(ex);
    return V3(ex, m_exp(-t * c.y), m_exp(-t * c.z));
}
DEV V3 div_uniform(V3 a, float b) {              // a / b with one correctly rounded division when the channels of a are equal
    const float q = a.x / b;
    if (a.y == a.x && a.z == a.x) return V3(q);
    return V3(q, a.y / b, a.z / b);
}

DEV float mis_weight(float a, float b) { a *= a; b *= b; float w = a / (a + b); return finite_(w) ? w : 0.f; }

// ----------------------------------------------------------------- media
struct MI { float t; V3 p, wi; V3 sigma_s, sigma_n, sigma_t, combined; float mint;
            DEV bool valid() const { return t != kInf; } };

// src/render/medium.cpp:40-82 + src/media/homogeneous.cpp:153-181
// The free-flight distance alone (the look-ahead of volpath_iteration draws it one trip early and keeps it in the record)
DEV float medium_sampled_t(const DMedium &M, float sample, uint32_t channel) {
    const float mm = channel == 0 ? M.sigma_t[0] : (channel == 1 ? M.sigma_t[1] : M.sigma_t[2]);
    return 0.f + (-m_log(1.f - sample) / mm);
}
DEV MI medium_interaction_at(const DMedium &M, const Ray &ray, float sampled_t) {
    MI mei; mei.wi = -ray.d;
    float mint = 0.f, maxt = fmin_(ray.maxt, kInf);
    V3 sigmat(M.sigma_t[0], M.sigma_t[1], M.sigma_t[2]);
    bool valid = sampled_t <= maxt;
    mei.t = valid ? sampled_t : kInf;
    mei.p = fma3(ray.d, sampled_t, ray.o);
    mei.mint = mint;
    V3 albedo(M.albedo[0], M.albedo[1], M.albedo[2]);
    mei.sigma_t = valid ? sigmat : V3(0.f);
    mei.sigma_s = valid ? sigmat * albedo : V3(0.f);
    mei.sigma_n = V3(0.f);
    mei.combined = sigmat;
    return mei;
}
DEV MI medium_sample_interaction(const DMedium &M, const Ray &ray, float sample, uint32_t channel) {
    return medium_interaction_at(M, ray, medium_sampled_t(M, sample, channel));
}

// src/volumes/grid.cpp (one channel) through Dr.Jit's Texture3f::eval (trilinear, clamp): texel centres at (i + .5) / res,
// lerp along x, then y, then z, each as fmadd(w0, a, w1 * b)
DEV float grid_eval(const DHetMedium &H, V3 pl) {
    const int rx = H.res[0], ry = H.res[1], rz = H.res[2];
    float fx = fma_(pl.x, (float) rx, -.5f), fy = fma_(pl.y, (float) ry, -.5f), fz = fma_(pl.z, (float) rz, -.5f);
    float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy), flz = __builtin_floorf(fz);
    float w1x = fx - flx, w1y = fy - fly, w1z = fz - flz, w0x = 1.f - w1x, w0y = 1.f - w1y, w0z = 1.f - w1z;
    auto cl = [](float v, int n) { int i = (v < -2e9f) ? -2000000000 : (v > 2e9f ? 2000000000 : (int) v); return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); };
    int x0 = cl(flx, rx), x1 = cl(flx + 1.f, rx), y0 = cl(fly, ry), y1 = cl(fly + 1.f, ry), z0 = cl(flz, rz), z1 = cl(flz + 1.f, rz);
    const float *d = H.data;
    auto at = [&](int x, int y, int z) { return d[((size_t) z * ry + y) * rx + x]; };
    float c00 = fma_(w0x, at(x0, y0, z0), w1x * at(x1, y0, z0)), c10 = fma_(w0x, at(x0, y1, z0), w1x * at(x1, y1, z0));
    float c01 = fma_(w0x, at(x0, y0, z1), w1x * at(x1, y0, z1)), c11 = fma_(w0x, at(x0, y1, z1), w1x * at(x1, y1, z1));
    float c0 = fma_(w0y, c00, w1y * c10), c1 = fma_(w0y, c01, w1y * c11);
    return fma_(w0z, c0, w1z * c1);
}

// The transpose of grid_eval for the PRB adjoint (kernels_prb.h, GRID): dg[v] += a * scale * w_v(pl) over the eight corners, with the
// float32 weights and the clamped corner indices of the lookup above (two corners that clamp onto one voxel both add there).
// sigma_t(p) = scale * sum_v w_v grid[v], so `a` is d / d sigma_t(p).  One no-return global_atomic_add_f32 per non-zero corner.
DEV void grid_scatter(const DHetMedium &H, float *__restrict__ dg, V3 pl, float a) {
    const int rx = H.res[0], ry = H.res[1], rz = H.res[2];
    float fx = fma_(pl.x, (float) rx, -.5f), fy = fma_(pl.y, (float) ry, -.5f), fz = fma_(pl.z, (float) rz, -.5f);
    float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy), flz = __builtin_floorf(fz);
    float w1x = fx - flx, w1y = fy - fly, w1z = fz - flz, w0x = 1.f - w1x, w0y = 1.f - w1y, w0z = 1.f - w1z;
    auto cl = [](float v, int n) { int i = (v < -2e9f) ? -2000000000 : (v > 2e9f ? 2000000000 : (int) v); return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); };
    int x0 = cl(flx, rx), x1 = cl(flx + 1.f, rx), y0 = cl(fly, ry), y1 = cl(fly + 1.f, ry), z0 = cl(flz, rz), z1 = cl(flz + 1.f, rz);
    const float as = a * H.scale;
#ifdef LRT_COUNT_SCATTER_ADDS                                   // (`make count`: the number of adds per voxel instead of their sum, for scripts/bench_grid_grad.py)
    auto add = [&](int x, int y, int z, float w) { const float v = as * w; if (v != 0.f) atomicAdd(&dg[((size_t) z * ry + y) * rx + x], 1.f); };
#else
    auto add = [&](int x, int y, int z, float w) { const float v = as * w; if (v != 0.f) atomicAdd(&dg[((size_t) z * ry + y) * rx + x], v); };
#endif
    add(x0, y0, z0, w0x * w0y * w0z); add(x1, y0, z0, w1x * w0y * w0z); add(x0, y1, z0, w0x * w1y * w0z); add(x1, y1, z0, w1x * w1y * w0z);
    add(x0, y0, z1, w0x * w0y * w1z); add(x1, y0, z1, w1x * w0y * w1z); add(x0, y1, z1, w0x * w1y * w1z); add(x1, y1, z1, w1x * w1y * w1z);
}

// include/mitsuba/core/bbox.h:303-340 (Williams et al.)
DEV bool bbox_ray_intersect(const float *lo, const float *hi, const Ray &ray, float &mint, float &maxt) {
    bool active = ray.d.x != 0.f || ray.d.y != 0.f || ray.d.z != 0.f;
    const float dx = rcp(ray.d.x), dy = rcp(ray.d.y), dz = rcp(ray.d.z);
    float t0x = ((dx >= 0.f ? lo[0] : hi[0]) - ray.o.x) * dx, t1x = ((dx >= 0.f ? hi[0] : lo[0]) - ray.o.x) * dx;
    float t0y = ((dy >= 0.f ? lo[1] : hi[1]) - ray.o.y) * dy, t1y = ((dy >= 0.f ? hi[1] : lo[1]) - ray.o.y) * dy;
    float t0z = ((dz >= 0.f ? lo[2] : hi[2]) - ray.o.z) * dz, t1z = ((dz >= 0.f ? hi[2] : lo[2]) - ray.o.z) * dz;
    auto max_safe = [](float a, float b) { return (a > b || !finite_(b)) ? a : b; };
    auto min_safe = [](float a, float b) { return (a < b || !finite_(b)) ? a : b; };
    active = active && !((t0x > t1y) || (t0y > t1x));
    t0x = max_safe(t0x, t0y); t1x = min_safe(t1x, t1y);
    active = active && !((t0x > t1z) || (t0z > t1x));
    t0x = max_safe(t0x, t0z); t1x = min_safe(t1x, t1z);
    mint = t0x; maxt = t1x;
    return active;
}

// src/render/medium.cpp:40-82 + src/media/heterogeneous.cpp:178-200: delta-tracking majorant, sigma_n = majorant - sigma_t(p)
DEV MI het_sample_interaction(const DMedium &M, const DHetMedium &H, const Ray &ray, float sample) {
    MI mei; mei.wi = -ray.d;
    float mint, maxt;
    bool active = bbox_ray_intersect(H.bbox_min, H.bbox_max, ray, mint, maxt);
    active = active && (finite_(mint) || finite_(maxt));
    if (!active) { mint = 0.f; maxt = kInf; }
    mint = fmax_(0.f, mint); maxt = fmin_(ray.maxt, maxt);
    const float max_density = H.max_density;
    float sampled_t = mint + (-m_log(1.f - sample) / max_density);
    bool valid = active && sampled_t <= maxt;
    mei.t = valid ? sampled_t : kInf;
    mei.p = fma3(ray.d, sampled_t, ray.o);
    mei.mint = mint;
    float st = 0.f;
    if (valid) st = H.scale * grid_eval(H, xform_point12(H.to_local, mei.p));
    V3 albedo(M.albedo[0], M.albedo[1], M.albedo[2]);
    mei.sigma_t = V3(st); mei.sigma_s = mei.sigma_t * (valid ? albedo : V3(0.f));
    mei.sigma_n = V3(max_density) - mei.sigma_t;
    mei.combined = V3(max_density);
    return mei;
}

// src/phase/hg.cpp:64-99, src/phase/isotropic.cpp:39-58
DEV float hg_eval(float g, float cos_theta) {
    float temp = 1.f + sqr(g) + 2.f * g * cos_theta;
    return kInvFourPi * (1.f - sqr(g)) / (temp * __builtin_sqrtf(temp));
}
DEV void phase_sample(const DMedium &M, V3 wi, float s2x, float s2y, V3 *wo, float *pdf) {
    if (M.phase == LRT_PHASE_HG) {
        float g = M.g;
        float sqr_term = (1.f - sqr(g)) / (1.f - g + 2.f * g * s2x);
        float cos_theta = (1.f + sqr(g) - sqr(sqr_term)) / (2.f * g);
        if (__builtin_fabsf(g) < kEpsilon) cos_theta = 1.f - 2.f * s2x;
        float sin_theta = safe_sqrt(1.f - sqr(cos_theta));
        float sp, cp; m_sincos(2.f * kPi * s2y, &sp, &cp);
        Frame f(wi);
        *wo = f.to_world(V3(sin_theta * cp, sin_theta * sp, -cos_theta));
        *pdf = hg_eval(g, -cos_theta);
    } else {
        *wo = square_to_uniform_sphere(s2x, s2y);
        *pdf = kInvFourPi;
    }
}
DEV float phase_eval(const DMedium &M, V3 wi, V3 wo) { return M.phase == LRT_PHASE_HG ? hg_eval(M.g, dot(wo, wi)) : kInvFourPi; }

// ------------------------------------------------- tabulated, Rayleigh and blended phase functions
// (src/phase/tabphase.cpp, rayleigh.cpp, blendphase.cpp; DPhase in device_types.h).  Compiled into the EXT instances, the phase probe (probes.h) and k_math_eval
// (fn 11) alone: phase_sample<false> / phase_eval<false> are the two functions above.
// cbrt stands in for Dr.Jit's dr::cbrt (rayleigh.cpp:63-64): exp(log|x| / 3) and one Newton step on y^3 = |x| with the residual formed by an
// fma; measured against float64 through lrt_math_eval fn 11: at most 1 ulp over the normal floats.  +-0, inf and NaN
// return x; subnormal arguments are not served (the Rayleigh inversion's arguments lie in [0.236, 4.24]).
DEV float m_cbrt(float x) {
    const float a = __builtin_fabsf(x);
    if (!(a > 0.f) || a == kInf) return x;
    float y = m_exp(m_log(a) * 0.333333343f);
    const float y2 = y * y;
    y = y - fma_(y2, y, -a) / (3.f * y2);
    return mulsign(y, x);
}
// ContinuousDistribution::eval_pdf_normalized over [-1, 1] (distr_1d.h:370-392): 0 outside the range (the masked gathers read 0)
DEV float tab_eval_pdf(SceneRef sc, const DPhase &P, float x) {
    if (!(x >= -1.f && x <= 1.f)) return 0.f;
    const float xs = (x - (-1.f)) * P.inv_interval_size;
    const uint32_t index = min((uint32_t) xs, P.n - 2u);
    const float4 r = *(const float4 *) (sc.phase_pool + P.rec_off + 4u * index);
    const float w1 = xs - (float) index, w0 = 1.f - w1;
    return fma_(w0, r.x, w1 * r.y) * P.normalization;
}
// ContinuousDistribution::sample (distr_1d.h:429-459)
DEV float tab_sample(SceneRef sc, const DPhase &P, float sample) {
    sample *= P.integral;
    const uint32_t index = cdf_search(sc.phase_pool + P.cdf_off, P.valid_x, P.valid_y, P.integral, sample);
    const float4 r = *(const float4 *) (sc.phase_pool + P.rec_off + 4u * index);
    const float y0 = r.x, y1 = r.y, c0 = r.z;
    sample = (sample - c0) * P.inv_interval_size;
    const float t_linear = (y0 - safe_sqrt(fma_(y0, y0, 2.f * sample * (y1 - y0)))) * rcp(y0 - y1),
                t_const = sample * rcp(y0),
                t = y0 == y1 ? t_const : t_linear;
    return fma_((float) index + t, P.interval_size, -1.f);
}
DEV float rayleigh_eval(float cos_theta) { return ((3.f / 16.f) * kInvPi) * (1.f + sqr(cos_theta)); }    // rayleigh.cpp:50-52

// One leaf (isotropic, hg, tabphase, rayleigh): PhaseFunction::sample -> wo, pdf (every leaf's weight is 1), and eval_pdf (eval = pdf in all four)
DEV void phase_leaf_sample(SceneRef sc, const DPhase &P, V3 wi, float s2x, float s2y, V3 *wo, float *pdf) {
    if (P.type == LRT_PHASE_TABULATED) {                    // tabphase.cpp:77-103
        const float cos_theta_prime = tab_sample(sc, P, s2x);
        const float sin_theta_prime = safe_sqrt(1.f - cos_theta_prime * cos_theta_prime);
        float sp, cp; m_sincos(2.f * kPi * s2y, &sp, &cp);
        Frame f(wi);
        *wo = -f.to_world(V3(sin_theta_prime * cp, sin_theta_prime * sp, cos_theta_prime));
        *pdf = tab_eval_pdf(sc, P, cos_theta_prime) * kInvTwoPi;
    } else if (P.type == LRT_PHASE_RAYLEIGH) {              // rayleigh.cpp:54-74
        const float z = 2.f * (2.f * s2x - 1.f);
        const float tmp = __builtin_sqrtf(sqr(z) + 1.f);
        const float A = m_cbrt(z + tmp), B = m_cbrt(z - tmp);
        const float cos_theta = A + B;
        const float sin_theta = safe_sqrt(1.f - sqr(cos_theta));
        float sp, cp; m_sincos(kTwoPi * s2y, &sp, &cp);
        Frame f(wi);
        *wo = f.to_world(V3(sin_theta * cp, sin_theta * sp, cos_theta));
        *pdf = rayleigh_eval(-cos_theta);
    } else {
        DMedium M; M.phase = P.type; M.g = P.g;
        phase_sample(M, wi, s2x, s2y, wo, pdf);
    }
}
DEV float phase_leaf_eval(SceneRef sc, const DPhase &P, V3 wi, V3 wo) {
    if (P.type == LRT_PHASE_TABULATED) return tab_eval_pdf(sc, P, -dot(wo, wi)) * kInvTwoPi;     // tabphase.cpp:105-118
    if (P.type == LRT_PHASE_RAYLEIGH) return rayleigh_eval(dot(wo, wi));                         // rayleigh.cpp:76-83
    return P.type == LRT_PHASE_HG ? hg_eval(P.g, dot(wo, wi)) : kInvFourPi;
}

// PhaseFunction::sample(ctx, mei, s1, (s2x, s2y)) -> wo, pdf, weight.  EXT: the medium may carry an entry of DScene::phases; without it
// this is phase_sample above, `s1` unused and the weight 1.
template <bool EXT>
DEV void phase_sample(SceneRef sc, const DMedium &M, V3 wi, float s1, float s2x, float s2y, V3 *wo, float *pdf, float *weight) {
    *weight = 1.f;
    if (!EXT || M.phase_ext == 0) { phase_sample(M, wi, s2x, s2y, wo, pdf); return; }
    const DPhase P = tab(sc.phases, (uint32_t) (M.phase_ext - 1));
    if (P.type != LRT_PHASE_BLEND) { phase_leaf_sample(sc, P, wi, s2x, s2y, wo, pdf); return; }
    // blendphase.cpp:122-153 (the children are leaves: they ignore the re-scaled s1, and their weights are 1)
    const float w = P.weight;
    const bool m0 = s1 > w;
    const DPhase Ps = tab(sc.phases, (uint32_t) (m0 ? P.child0 : P.child1)), Po = tab(sc.phases, (uint32_t) (m0 ? P.child1 : P.child0));
    float pdf_s; phase_leaf_sample(sc, Ps, wi, s2x, s2y, wo, &pdf_s);
    const float pdf_o = phase_leaf_eval(sc, Po, wi, *wo);
    const float pdf0 = m0 ? pdf_s : pdf_o, pdf1 = m0 ? pdf_o : pdf_s;
    const float pdf_weighted = w * pdf1 + (1.f - w) * pdf0;
    // (with the sampled child's weight 1 and eval = pdf, both of the source's numerators, w * eval1 + (1 - w) * w0 * pdf0 and
    //  w * w1 * pdf1 + (1 - w) * eval0, are pdf_weighted's own expression: the quotient is 1 up to the rounding of rcp, or 0)
    *weight = pdf_weighted * (pdf_weighted > 0.f ? rcp(pdf_weighted) : 0.f);
    *pdf = pdf_weighted;
}
// PhaseFunction::eval_pdf: the value (the pdf equals it in every family)
template <bool EXT>
DEV float phase_eval(SceneRef sc, const DMedium &M, V3 wi, V3 wo) {
    if (!EXT || M.phase_ext == 0) return phase_eval(M, wi, wo);
    const DPhase P = tab(sc.phases, (uint32_t) (M.phase_ext - 1));
    if (P.type != LRT_PHASE_BLEND) return phase_leaf_eval(sc, P, wi, wo);
    const float v0 = phase_leaf_eval(sc, tab(sc.phases, (uint32_t) P.child0), wi, wo), v1 = phase_leaf_eval(sc, tab(sc.phases, (uint32_t) P.child1), wi, wo);
    return fma_(v1, P.weight, fma_(-v0, P.weight, v0));         // dr::lerp(v0, v1, weight), blendphase.cpp:182-188
}

DEV int target_medium(const DShape &sd, V3 d, V3 n) { return dot(d, n) > 0.f ? sd.exterior_medium : sd.interior_medium; }
DEV bool is_medium_transition(const DShape &sd) { return sd.interior_medium >= 0 || sd.exterior_medium >= 0; }

} // namespace lrt
