// Test probes (include/liverrt.h lrt_*_probe): each runs one piece of the shading code once per lane on the scene's device image and
// writes a flat record of floats.  A probe is a ProbeKind (device_scene.h), a row of kProbes, and a probe_lane body; k_probe<KIND>
// carries the lane indexing for all of them and device_probe (device.hip) the upload, the launch and the copy back.  DESIGN.md section 21.
#pragma once
#include "kernels.h"
#include "device_scene.h"

namespace lrt {

// in / out: floats per lane of the packed input record and of the output record; traces: the body walks the BVH (k_probe gives it a
// traversal stack in LDS); needs_env: the scene must hold an environment emitter; name: the entry point, for error messages.
struct ProbeRow { int in, out; bool traces, needs_env; const char *name; };
constexpr ProbeRow kProbes[PROBE_KINDS] = {
    /* PROBE_EMITTER */ { 5,  LRT_PROBE_FLOATS,        true,  false, "lrt_emitter_probe" },     // ref_p[3], sample[2]
    /* PROBE_ENVMAP  */ { 3,  4,                       false, true,  "lrt_envmap_probe" },      // dir[3]
    /* PROBE_BSDF    */ { 12, LRT_BSDF_PROBE_FLOATS,   true,  false, "lrt_bsdf_probe" },        // o[3], d[3], sample[3], wo_query[3]
    /* PROBE_PHASE   */ { 9,  LRT_PHASE_PROBE_FLOATS,  false, false, "lrt_phase_probe" },       // wi[3], sample[3], wo_query[3]
    /* PROBE_MEDIUM  */ { 9,  LRT_MEDIUM_PROBE_FLOATS, false, false, "lrt_medium_probe" },      // o[3], d[3], maxt, sample, channel
    /* PROBE_SENSOR  */ { 5,  LRT_SENSOR_PROBE_FLOATS, false, false, "lrt_sensor_probe" },      // ax, ay, spx, spy, x
};
static_assert(PROBE_EMITTER == 0 && PROBE_ENVMAP == 1 && PROBE_BSDF == 2 && PROBE_PHASE == 3 && PROBE_MEDIUM == 4 && PROBE_SENSOR == 5 && PROBE_KINDS == 6,
              "kProbes is indexed by ProbeKind");
static_assert(kProbes[PROBE_EMITTER].out == 20 && kProbes[PROBE_BSDF].out == 30 && kProbes[PROBE_PHASE].out == 7 && kProbes[PROBE_MEDIUM].out == 22 && kProbes[PROBE_SENSOR].out == 16,
              "the record widths are part of the ABI (include/liverrt.h, liverrenderer_amd/_lib.py)");

// One lane of probe KIND.  in / o: the lane's input and output records (kProbes[KIND].in / .out floats); arg: the medium index of the
// phase and medium probes, unused elsewhere; stack: the lane's traversal stack where the row says `traces`, null elsewhere.
template <int KIND> DEV void probe_lane(SceneRef sc, int arg, const float *in, float *o, int *stack);

// lrt_emitter_probe: the EXT instances' Scene::sample_emitter_direction for one reference point and sample per lane, then a
// closest-hit query from the reference point along the sampled direction and what the integrators evaluate at its hit
// (pdf_emitter_direction, emitter_eval).  No ray offset: the tests put the reference points in free space.
template <> DEV void probe_lane<PROBE_EMITTER>(SceneRef sc, int, const float *in, float *o, int *stack) {
    const V3 ref(in[0], in[1], in[2]);
    DirSample ds; const V3 w = sample_emitter_direction<true>(sc, ref, in[3], in[4], &ds);
    o[0] = ds.p.x; o[1] = ds.p.y; o[2] = ds.p.z; o[3] = ds.n.x; o[4] = ds.n.y; o[5] = ds.n.z; o[6] = ds.d.x; o[7] = ds.d.y; o[8] = ds.d.z;
    o[9] = ds.dist; o[10] = ds.pdf; o[11] = w.x; o[12] = w.y; o[13] = w.z; o[14] = (float) ds.emitter;
    float shape = -1.f, pdf = 0.f; V3 le(0.f);
    if (ds.pdf > 0.f) {
        const GlobalTracer tg{ sc, stack };
        const ExtTracer<GlobalTracer> tr{ tg, sc };
        Ray r; r.o = ref; r.d = ds.d; r.maxt = kLargest;
        const Hit h = tr.closest(r);
        const SI si = tr.surface(sc, r, h);
        if (si.valid) shape = (float) si.shape;
        const int e = si_emitter(sc, si);
        if (e >= 0) { pdf = pdf_emitter_direction<true>(sc, ref, si, e); le = emitter_eval(sc, e, si); }
    }
    o[15] = shape; o[16] = pdf; o[17] = le.x; o[18] = le.y; o[19] = le.z;
}

// lrt_envmap_probe: what the integrators evaluate for a ray that leaves the scene along dir, one direction per lane:
// pdf_emitter_direction of the environment emitter for a miss, then emitter_eval_env.  The scene must hold an environment emitter.
template <> DEV void probe_lane<PROBE_ENVMAP>(SceneRef sc, int, const float *in, float *o, int *) {
    const V3 d(in[0], in[1], in[2]);
    SI si{}; si.valid = false; si.wi = -d;
    const float pdf = pdf_emitter_direction<true>(sc, V3(0.f), si, sc.env.emitter);
    const V3 le = emitter_eval_env(sc, d);
    o[0] = pdf; o[1] = le.x; o[2] = le.y; o[3] = le.z;
}

// lrt_bsdf_probe: the surface code at a chosen ray, one per lane: a closest-hit query through the EXT tracer (spheres count),
// no ray offset; the surface interaction; bsdf_sample with the lane's (s1, s2x, s2y) as path_iteration calls it; bsdf_eval and bsdf_pdf
// at the world direction woq, brought into the shading frame as the integrators bring an emitter sample's direction.
template <> DEV void probe_lane<PROBE_BSDF>(SceneRef sc, int, const float *in, float *o, int *stack) {
    const float *smp = in + 6, *woq = in + 9;
    const GlobalTracer tg{ sc, stack };
    const ExtTracer<GlobalTracer> tr{ tg, sc };
    Ray r; r.o = V3(in[0], in[1], in[2]); r.d = V3(in[3], in[4], in[5]); r.maxt = kLargest;
    const Hit h = tr.closest(r);
    const SI si = tr.surface(sc, r, h);
    if (!si.valid) {
        o[0] = -1.f;
        for (int j = 1; j < LRT_BSDF_PROBE_FLOATS; ++j) o[j] = 0.f;
        return;
    }
    const int b = tab(sc.shapes, si.shape, sc.one_shape).bsdf;
    const BSDFSample bs = bsdf_sample<false, true>(sc, b, si, smp[0], smp[1], smp[2]);
    const V3 wow = si.sh.to_world(bs.wo);
    const V3 wo = si.sh.to_local(V3(woq[0], woq[1], woq[2]));
    const V3 ev = bsdf_eval<true>(sc, b, si, wo);
    const float pdf = bsdf_pdf<true>(sc, b, si, wo);
    o[0] = (float) si.shape; o[1] = si.t; o[2] = si.p.x; o[3] = si.p.y; o[4] = si.p.z; o[5] = si.n.x; o[6] = si.n.y; o[7] = si.n.z;
    o[8] = si.sh.n.x; o[9] = si.sh.n.y; o[10] = si.sh.n.z; o[11] = si.uv.x; o[12] = si.uv.y; o[13] = si.wi.x; o[14] = si.wi.y; o[15] = si.wi.z;
    o[16] = wow.x; o[17] = wow.y; o[18] = wow.z; o[19] = bs.wo.z; o[20] = bs.pdf; o[21] = bs.eta; o[22] = (float) bs.type;
    o[23] = bs.weight.x; o[24] = bs.weight.y; o[25] = bs.weight.z; o[26] = ev.x; o[27] = ev.y; o[28] = ev.z; o[29] = pdf;
}

// lrt_phase_probe: the phase function of medium `medium`, phase_sample<true> with the lane's wi and (s1, s2x, s2y) as the EXT
// instances of the volume integrators call it, and phase_eval<true> at the world direction woq.
template <> DEV void probe_lane<PROBE_PHASE>(SceneRef sc, int medium, const float *in, float *o, int *) {
    const float *smp = in + 3, *woq = in + 6;
    const DMedium M = tab(sc.media, medium);
    const V3 wi(in[0], in[1], in[2]);
    V3 wo; float pdf, weight; phase_sample<true>(sc, M, wi, smp[0], smp[1], smp[2], &wo, &pdf, &weight);
    const float ev = phase_eval<true>(sc, M, wi, V3(woq[0], woq[1], woq[2]));
    o[0] = wo.x; o[1] = wo.y; o[2] = wo.z; o[3] = weight; o[4] = pdf; o[5] = ev; o[6] = ev;     // (eval = pdf in every family)
}

// lrt_medium_probe: free-flight sampling in medium `medium` as volpath_iteration<HET> and any_medium_sample call it:
// het_sample_interaction for a grid medium, medium_sample_interaction otherwise, on the ray (o, d, maxt) = in[0..6] with sample = in[7]
// and channel = in[8].  A NaN maxt asks for the grid lookup alone: in[0..2] is then a point in the grid's local frame, wherever it lies.
template <> DEV void probe_lane<PROBE_MEDIUM>(SceneRef sc, int medium, const float *in, float *o, int *) {
    const DMedium M = tab(sc.media, medium);
    Ray ray; ray.o = V3(in[0], in[1], in[2]); ray.d = V3(in[3], in[4], in[5]); ray.maxt = in[6];
    for (int j = 0; j < LRT_MEDIUM_PROBE_FLOATS; ++j) o[j] = 0.f;
    if (ray.maxt != ray.maxt) {
        if (M.het) { o[18] = ray.o.x; o[19] = ray.o.y; o[20] = ray.o.z; o[21] = grid_eval(tab(sc.het, medium), ray.o); }
        return;
    }
    const float ch = in[8];
    const uint32_t channel = ch >= 2.f ? 2u : (ch >= 1.f ? 1u : 0u);
    const MI mei = M.het ? het_sample_interaction(M, tab(sc.het, medium), ray, in[7]) : medium_sample_interaction(M, ray, in[7], channel);
    o[0] = mei.valid() ? 1.f : 0.f; o[1] = mei.t; o[2] = mei.p.x; o[3] = mei.p.y; o[4] = mei.p.z; o[5] = mei.mint;
    o[6] = mei.sigma_t.x; o[7] = mei.sigma_t.y; o[8] = mei.sigma_t.z; o[9] = mei.sigma_s.x; o[10] = mei.sigma_s.y; o[11] = mei.sigma_s.z;
    o[12] = mei.sigma_n.x; o[13] = mei.sigma_n.y; o[14] = mei.sigma_n.z; o[15] = mei.combined.x; o[16] = mei.combined.y; o[17] = mei.combined.z;
    if (M.het) {
        const DHetMedium H = tab(sc.het, medium);
        const V3 pl = xform_point12(H.to_local, mei.p);
        o[18] = pl.x; o[19] = pl.y; o[20] = pl.z; o[21] = grid_eval(H, pl);
    }
}

// lrt_sensor_probe: camera_ray at the adjusted position sample in[0..1] as generate_camera_path calls it, the film-to-sample map and
// film_footprint at the film position in[2..3], rfilter_eval at in[4]; the record of include/liverrt.h.
template <> DEV void probe_lane<PROBE_SENSOR>(SceneRef sc, int, const float *in, float *o, int *) {
    const Ray ray = camera_ray(sc, in[0], in[1]);
    const float spx = in[2], spy = in[3];
    const FilmFootprint fp = film_footprint(sc.film, 0, 0, spx, spy);            // (float) 0 + spx is spx
    o[0] = ray.o.x; o[1] = ray.o.y; o[2] = ray.o.z; o[3] = ray.d.x; o[4] = ray.d.y; o[5] = ray.d.z; o[6] = ray.maxt;
    o[7] = fma_(spx, sc.film.scale_x, sc.film.offset_x); o[8] = fma_(spy, sc.film.scale_y, sc.film.offset_y);
    o[9] = (float) fp.pix; o[10] = (float) fp.piy; o[11] = fp.relx; o[12] = fp.rely;
    o[13] = rfilter_eval(sc.film, in[4]); o[14] = (float) sc.film.fcount; o[15] = 0.f;
}

// Lane i of probe KIND: the tail guard, the lane's records, and the traversal stack of the kinds that trace (the others use no LDS).
template <int KIND>
__global__ void __launch_bounds__(LRT_BLOCK)
k_probe(ScenePtr scp, int arg, const float *__restrict__ in, uint32_t n, float *__restrict__ out) {
    SceneRef sc = *scp;
    constexpr ProbeRow P = kProbes[KIND];
    const uint32_t i = blockIdx.x * LRT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *lane_in = in + (size_t) P.in * i;
    float *lane_out = out + (size_t) P.out * i;
    if constexpr (P.traces) {
        __shared__ int s_stack[LRT_STACK * LRT_BLOCK];
        probe_lane<KIND>(sc, arg, lane_in, lane_out, s_stack + threadIdx.x);
    } else {
        probe_lane<KIND>(sc, arg, lane_in, lane_out, nullptr);
    }
}

} // namespace lrt
