// A queued path: its registers (PathState) and the load and store of its record under a layout of record_layout.h (included by kernels.h).
#pragma once
#include "record_layout.h"

namespace lrt {

struct PathState {
    V3 o, d, tp, res, lp; float maxt, eta, last_pdf; uint32_t flags, lane; uint64_t rng_state;
    uint32_t rng_word;         // compact records: the TEA word behind the lane's sampler stream (independent: v1, ld: v0), kept instead of recomputed every trip
    float tdepth, si_t;        // biovolpath / biovolpath06: `tissueDepth`, distance returned by the previous trip's ray query
    float ff_t;                // volpath (homogeneous media): the free-flight distance the look-ahead already drew for this trip (NaN: none); rides in the maxt slot
    float bio_dist; bool bio_hep;   // biovolpath: the element competition the look-ahead already ran for this trip (distance, NaN = none; hepatocytes won)
    float4 hit;                // volpath, heterogeneous media: the surface hit (t, u, v, prim) a null collision keeps (PF_HAVE_SI)
    float W[2][3][3];          // volpathmis: p_over_f, p_over_f_nee
};

// What rides where, per stream the layout has (record_layout.h says which):
//   o_maxt     o | the maxt slot.  Only a layout with the hit stream queues rays whose maxt matters; everywhere else a queued ray comes from
//              spawn_ray (maxt = largest float) and the slot carries si_t (layouts with tdepth) or ff_t (the others).
//   d_eta      d | eta
//   tp_pdf     throughput | last-scatter pdf; without res_flags (closed records): throughput | flags, and `result`, the pdf and lp are never read;
//              with w1..w4: the first four of the 18 MIS weights, W[0..17] = p_over_f then p_over_f_nee in memory order, tp_pdf | w1 | w2 | w3 | w4.xy
//   res_flags  result | flags
//   lp_lane    last scatter position | lane id, and rng the PCG32 state (8-byte entries); compact forms: neither, rng holds state | lane | sampler
//              word in 16-byte entries: one stream and 8 bytes less, five memory instructions each way instead of six, no TEA rounds at the start of a trip
//   tdepth     tissueDepth, its sign bit: the cached element competition was won by the hepatocytes | that competition's distance (NaN: none)
//   hit        the surface hit (t, u, v, prim) a null collision keeps
#define LRT_HAS(m) record_has(LAYOUT, COMPACT, offsetof(DPathStreams, m))
template <RecordLayout LAYOUT = RecordLayout::Wide, bool COMPACT = false, typename QS>
DEV void load_state(const QS &q, size_t i, PathState &s) {
    static_assert(record_form_exists(LAYOUT, COMPACT), "no such record form (record_layout.h, kRecordForms)");
    constexpr bool has_res = LRT_HAS(res_flags), rng16 = record_has(LAYOUT, COMPACT, offsetof(DPathStreams, rng), 16), has_td = LRT_HAS(tdepth), has_hit = LRT_HAS(hit), has_w = LRT_HAS(w1);
    static_assert(rng16 == !LRT_HAS(lp_lane) && LRT_HAS(o_maxt) && LRT_HAS(d_eta) && LRT_HAS(tp_pdf), "load_state / store_state assume it");
    const float4 a = q.o_maxt[i], b = q.d_eta[i], c = q.tp_pdf[i];
    float4 d, e, w1, w2, w3, w4; uint2 r; uint4 r4; float2 td;          // every load first, the unpacking after them
    if (has_res) d = q.res_flags[i];
    if (rng16) r4 = reinterpret_cast<const uint4 *>(q.rng)[i];
    else { e = q.lp_lane[i]; r = q.rng[i]; }
    if (has_td) td = q.tdepth[i];
    if (has_hit) s.hit = q.hit[i];                       // (not through a local: that one stays a <4 x float> across the loop and the het / mis kernels come out different)
    if (has_w) { w1 = q.w1[i]; w2 = q.w2[i]; w3 = q.w3[i]; w4 = q.w4[i]; }
    s.o = V3(a.x, a.y, a.z); s.maxt = has_hit ? a.w : kLargest; s.d = V3(b.x, b.y, b.z); s.eta = b.w;
    if (!has_hit) { if (has_td) s.si_t = a.w; else s.ff_t = a.w; }
    s.tp = V3(c.x, c.y, c.z);
    if (has_res) { s.last_pdf = c.w; s.res = V3(d.x, d.y, d.z); s.flags = f2u(d.w); }
    else { s.flags = f2u(c.w); s.res = V3(0.f); s.last_pdf = 1.f; }
    if (rng16) { s.lp = V3(0.f); s.lane = r4.z; s.rng_word = r4.w; s.rng_state = ((uint64_t) r4.y << 32) | r4.x; }
    else { s.lp = V3(e.x, e.y, e.z); s.lane = f2u(e.w); s.rng_state = ((uint64_t) r.y << 32) | r.x; }
    if (has_td) { s.tdepth = __builtin_fabsf(td.x); s.bio_hep = (f2u(td.x) >> 31) != 0u; s.bio_dist = td.y; }
    if (has_w) {
        float *W = &s.W[0][0][0];
        W[0] = c.x; W[1] = c.y; W[2] = c.z; W[3] = c.w; W[4] = w1.x; W[5] = w1.y; W[6] = w1.z; W[7] = w1.w; W[8] = w2.x;
        W[9] = w2.y; W[10] = w2.z; W[11] = w2.w; W[12] = w3.x; W[13] = w3.y; W[14] = w3.z; W[15] = w3.w; W[16] = w4.x; W[17] = w4.y;
    }
}
template <RecordLayout LAYOUT = RecordLayout::Wide, bool COMPACT = false, typename QS>
DEV void store_state(const QS &q, size_t i, const PathState &s) {
    constexpr bool has_res = LRT_HAS(res_flags), rng16 = record_has(LAYOUT, COMPACT, offsetof(DPathStreams, rng), 16), has_td = LRT_HAS(tdepth), has_hit = LRT_HAS(hit), has_w = LRT_HAS(w1);
    q.o_maxt[i] = make_float4(s.o.x, s.o.y, s.o.z, has_hit ? s.maxt : (has_td ? s.si_t : s.ff_t));
    q.d_eta[i] = make_float4(s.d.x, s.d.y, s.d.z, s.eta);
    if (has_w) {
        const float *W = &s.W[0][0][0];
        q.tp_pdf[i] = make_float4(W[0], W[1], W[2], W[3]); q.w1[i] = make_float4(W[4], W[5], W[6], W[7]); q.w2[i] = make_float4(W[8], W[9], W[10], W[11]);
        q.w3[i] = make_float4(W[12], W[13], W[14], W[15]); q.w4[i] = make_float4(W[16], W[17], 0.f, 0.f);
    } else q.tp_pdf[i] = make_float4(s.tp.x, s.tp.y, s.tp.z, has_res ? s.last_pdf : u2f(s.flags));
    if (has_res) q.res_flags[i] = make_float4(s.res.x, s.res.y, s.res.z, u2f(s.flags));
    if (rng16) reinterpret_cast<uint4 *>(q.rng)[i] = make_uint4((uint32_t) s.rng_state, (uint32_t) (s.rng_state >> 32), s.lane, s.rng_word);
    else {
        q.lp_lane[i] = make_float4(s.lp.x, s.lp.y, s.lp.z, u2f(s.lane));
        q.rng[i] = make_uint2((uint32_t) s.rng_state, (uint32_t) (s.rng_state >> 32));
    }
    if (has_td) q.tdepth[i] = make_float2(s.bio_hep ? -s.tdepth : s.tdepth, s.bio_dist);
    if (has_hit) q.hit[i] = s.hit;
}
#undef LRT_HAS

} // namespace lrt
