// Film accumulation on the device: the reconstruction filter, a sample's footprint, and the two wave-level routes every kernel that writes
// a film takes (box-filter runs, wide-filter group walk), and the box-filter route of the 64-byte-record kernels.  Text of kernels.h:
// included there, inside namespace lrt, after the lane helpers (lane_to_pixel, lane_jitter, lane_local_index) it builds on;
// kernels_prb.h, kernels_aov.h and kernels_moment.h use it through kernels.h.

template <typename FP> DEV float estrin10(float x, FP c) {
    float x2 = x * x, x4 = x2 * x2, x8 = x4 * x4;
    float a0 = fma_(x, c[1], c[0]), a1 = fma_(x, c[3], c[2]), a2 = fma_(x, c[5], c[4]), a3 = fma_(x, c[7], c[6]), a4 = fma_(x, c[9], c[8]);
    float b0 = fma_(x2, a1, a0), b1 = fma_(x2, a3, a2);
    float c0 = fma_(x4, b1, b0);
    return fma_(x8, a4, c0);
}
DEV float rfilter_eval(FilmRef F, float x) {
    if (F.rfilter == LRT_RFILTER_GAUSSIAN) return fmax_(estrin10(sqr(x), F.rf_coeff), 0.f);
    if (F.rfilter == LRT_RFILTER_TENT) return fmax_(0.f, 1.f - __builtin_fabsf(x * F.rf_inv_radius));
    return (x >= -0.5f && x < 0.5f) ? 1.f : 0.f;             // src/rfilters/box.cpp:42: half open
}

// Index of pixel (px, py) (film coordinates, as lane_to_pixel gives them) in the crop window's row-major film
DEV size_t film_pixel_index(FilmRef F, int px, int py) {
    return (size_t) (py - F.crop_offset_y) * F.width + (px - F.crop_offset_x);
}

// The filter footprint of a sample at (px + jx, py + jy) (imageblock.cpp:431-447): F.fcount x F.fcount pixels from (pix, piy); the filter
// is evaluated at rely + ys, relx + xs for cell (xs, ys).
struct FilmFootprint {
    int pix, piy; float relx, rely;
    // one word that is equal for equal origins (coordinates are within +-0x4000 of the film)
    DEV uint32_t key() const { return (uint32_t) (piy + 0x4000) << 16 | (uint32_t) (pix + 0x4000); }
};
DEV FilmFootprint film_footprint(FilmRef F, int px, int py, float jx, float jy) {
    const float spx = (float) px + jx, spy = (float) py + jy;
    FilmFootprint f;
    f.pix = (int) __builtin_floorf(spx) - F.fn; f.piy = (int) __builtin_floorf(spy) - F.fn;
    f.relx = (float) f.pix + .5f - spx; f.rely = (float) f.piy + .5f - spy;
    return f;
}

// A finished path: splat {R,G,B,[A],W=1} (integrator.cpp:499-520, imageblock.cpp:174-232,431-500),
// or, for the per-lane test hook, store the radiance.
DEV void finish_path(SceneRef sc, RpRef rp, float *__restrict__ film, float *__restrict__ sample_out,
                     uint64_t sample_base, uint32_t lane, V3 L, bool valid) {
    if (rp.integrator == LRT_INTEGRATOR_PATH && !valid) L = V3(0.f);                 // path.cpp:342-345
    if (sample_out) {                               // per-lane output, indexed by the rank-local lane index
        const uint64_t j = lane_local_index(rp, lane);
        float4 *o = reinterpret_cast<float4 *>(sample_out) + (j - sample_base);
        *o = make_float4(L.x, L.y, L.z, valid ? 1.f : 0.f);
        return;
    }
    FilmRef F = sc.film;
    int px, py; lane_to_pixel(sc, rp, lane, &px, &py);
    const int C = F.channels;
    const float alpha = valid ? 1.f : 0.f;
    auto splat = [&](float *p, float w) {
        atomicAdd(p + 0, L.x * w); atomicAdd(p + 1, L.y * w); atomicAdd(p + 2, L.z * w);
        if (F.has_alpha) { atomicAdd(p + 3, alpha * w); atomicAdd(p + 4, 1.f * w); } else atomicAdd(p + 3, 1.f * w);
    };
    if (F.rfilter == LRT_RFILTER_BOX) {
        int x = px - F.crop_offset_x, y = py - F.crop_offset_y;
        float *p = film + ((size_t) y * F.width + x) * C;
        atomicAdd(p + 0, L.x); atomicAdd(p + 1, L.y); atomicAdd(p + 2, L.z);
        if (F.has_alpha) { atomicAdd(p + 3, alpha); atomicAdd(p + 4, 1.f); } else atomicAdd(p + 3, 1.f);
        return;
    }
    float jx, jy; lane_jitter(rp, lane, lane_local_index(rp, lane), jx, jy);
    const FilmFootprint fp = film_footprint(F, px, py, jx, jy);
    int count = F.fcount;
    for (int ys = 0; ys < count; ++ys) {
        int y = fp.piy - F.crop_offset_y + ys;
        float wy = rfilter_eval(F, fp.rely + (float) ys);
        if (y < 0 || y >= F.height || (wy == 0.f && finite3(L))) continue;
        for (int xs = 0; xs < count; ++xs) {
            int x = fp.pix - F.crop_offset_x + xs;
            if (x < 0 || x >= F.width) continue;
            float w = wy * rfilter_eval(F, fp.relx + (float) xs);
            if (w == 0.f && finite3(L)) continue;                  // rule 1 of film_walk, per sample
            splat(film + ((size_t) y * F.width + x) * C, w);
        }
    }
}

// Box filter, called by every lane of a wave: queues and lane buffers keep lanes in lane order, so the lanes of one pixel sit in RUNS of
// consecutive lanes.  Returns the lane's film pixel and whether it is the first / last lane of its run; a lane without a sample is a run of
// its own (head, never tail).  wave_segmented_sums(v, head) then adds up every run at once (no loop over the pixels, no LDS round trip) and
// the tail lane holds the run's sums and issues the atomics.  A pixel that appears in two runs simply gets two sets of atomics.
struct FilmRun { uint32_t pixel; bool head, tail; };
DEV FilmRun film_run(FilmRef F, bool have, int px, int py) {
    FilmRun r;
    r.pixel = have ? (uint32_t) film_pixel_index(F, px, py) : 0xffffffffu;
    const uint32_t prev = wave_prev(r.pixel, 0xfffffffeu), next = wave_next(r.pixel, 0xfffffffeu);
    r.head = r.pixel != prev || !have; r.tail = have && r.pixel != next;
    return r;
}

// Film accumulation called by EVERY lane of a wave (`finishing` selects the lanes that retire a path).  Box filter:
// lanes that splat into the same pixel are summed inside the wave first (the wavefront keeps a pixel's samples in
// neighbouring lanes, so a wave usually holds one or two distinct pixels) and one lane issues the atomics.
DEV void finish_paths_wave(SceneRef sc, RpRef rp, float *__restrict__ film, float *__restrict__ sample_out,
                           uint64_t sample_base, bool finishing, uint32_t lane, V3 L, bool valid) {
    FilmRef F = sc.film;
    if (sample_out || F.rfilter != LRT_RFILTER_BOX) {
        if (finishing) finish_path(sc, rp, film, sample_out, sample_base, lane, L, valid);
        return;
    }
    if (rp.integrator == LRT_INTEGRATOR_PATH && !valid) L = V3(0.f);
    uint32_t pixel = 0xffffffffu;
    if (finishing) { int px, py; lane_to_pixel(sc, rp, lane, &px, &py); pixel = (uint32_t) (py - F.crop_offset_y) * (uint32_t) F.width + (uint32_t) (px - F.crop_offset_x); }
    if (__ballot(finishing) == 0ull) return;
    // film_run and film_pixel_index written out: through the helpers the compiler schedules this block differently inside every render kernel
    const uint32_t prev = wave_prev(pixel, 0xfffffffeu), next = wave_next(pixel, 0xfffffffeu);
    float v[5] = { finishing ? L.x : 0.f, finishing ? L.y : 0.f, finishing ? L.z : 0.f, finishing ? 1.f : 0.f, (finishing && valid) ? 1.f : 0.f };
    wave_segmented_sums(v, pixel != prev || !finishing);
    if (finishing && pixel != next) {
        float *p = film + (size_t) pixel * F.channels;
        atomicAdd(p + 0, v[0]); atomicAdd(p + 1, v[1]); atomicAdd(p + 2, v[2]);
        if (F.has_alpha) { atomicAdd(p + 3, v[4]); atomicAdd(p + 4, v[3]); } else atomicAdd(p + 3, v[3]);
    }
}

// ---- The box-filter route of the 64-byte-record volpath kernels (closed_records(): only a path's last trip adds radiance, so a lane that retires
// anywhere else carries L = +0 exactly).  W and alpha are counts of lanes, taken from ballots (film_runs.h), and RGB costs nothing where it is zero:
//   W      once per sample, where the sample is born (count_born_wave, the fresh tiles): a lane born in a launch retires in it, the sum of small
//          integers in float is exact in any grouping, so the film's W is the same number whenever it is added;
//   RGB    the runs and the scan's tree are finish_paths_wave's (runs of consecutive retiring lanes of one pixel: the non-zero members of a run are
//          associated as there), but the scan is skipped when no retiring lane of the wave has a non-zero L and a run whose sums are all zero issues
//          no atomic: x + (+-0) = x for every x a film holds (sums start at +0 and never become -0).  NaN compares non-zero and goes through;
//   alpha  the valid samples.  A path's validity is only ever switched on (volpath_iteration), and generate_camera_path switches it on at birth
//          when the environment is visible (LRT_BORN_VALID: the same for every lane of a launch): alpha is then W and is counted with it.  Otherwise it
//          is the run's valid retiring lanes, at retirement, when the wave retires a valid lane at all.
// Both form the film pixel as lane / spp: lane_to_pixel splits that index by the film's width and film_pixel_index puts it together again.
DEV uint32_t lane_film_pixel(RpRef rp, uint32_t lane) { return (rp.log2_spp != 0xffffffffu) ? (lane >> rp.log2_spp) : (lane / rp.spp); }

// called by EVERY lane of a fresh tile, right after generate_camera_path: `born` = the lane holds a new sample, of film pixel `pixel` (0xffffffff without one)
DEV void count_born_wave(SceneRef sc, RpRef rp, float *__restrict__ film, const float *__restrict__ sample_out, bool born, uint32_t pixel) {
    FilmRef F = sc.film;
    if (sample_out || F.rfilter != LRT_RFILTER_BOX) return;                       // (finish_path counts these at retirement)
    const uint32_t prev = wave_prev(pixel, 0xfffffffeu), next = wave_next(pixel, 0xfffffffeu);
    const unsigned long long heads = __ballot(pixel != prev || !born), members = __ballot(born);
    if (born && pixel != next) {
        float *p = film + (size_t) pixel * (uint32_t) F.channels;
        const float n = (float) film_run_count(heads, members, threadIdx.x & 63u);
        atomicAdd(p + F.channels - 1, n);                                         // W is a film's last channel
        if (F.has_alpha && LRT_BORN_VALID(sc, rp)) atomicAdd(p + 3, n);
    }
}

// called by EVERY lane of a wave, as finish_paths_wave is
DEV void finish_paths_wave_closed(SceneRef sc, RpRef rp, float *__restrict__ film, float *__restrict__ sample_out,
                                  uint64_t sample_base, bool finishing, uint32_t lane, V3 L, bool valid) {
    FilmRef F = sc.film;
    if (sample_out || F.rfilter != LRT_RFILTER_BOX) {
        if (finishing) finish_path(sc, rp, film, sample_out, sample_base, lane, L, valid);
        return;
    }
    const unsigned long long lit = __ballot(finishing && (L.x != 0.f || L.y != 0.f || L.z != 0.f));
    const unsigned long long opaque = (F.has_alpha && !LRT_BORN_VALID(sc, rp)) ? __ballot(finishing && valid) : 0ull;
    if ((lit | opaque) == 0ull) return;
    const uint32_t pixel = finishing ? lane_film_pixel(rp, lane) : 0xffffffffu;
    const uint32_t prev = wave_prev(pixel, 0xfffffffeu), next = wave_next(pixel, 0xfffffffeu);
    const bool head = pixel != prev || !finishing;
    float v[3] = { finishing ? L.x : 0.f, finishing ? L.y : 0.f, finishing ? L.z : 0.f };
    if (lit) wave_segmented_sums(v, head);
    const unsigned long long heads = opaque ? __ballot(head) : 0ull;
    if (finishing && pixel != next) {
        float *p = film + (size_t) pixel * (uint32_t) F.channels;
        if (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f) { atomicAdd(p + 0, v[0]); atomicAdd(p + 1, v[1]); atomicAdd(p + 2, v[2]); }
        if (opaque) atomicAdd(p + 3, (float) film_run_count(heads, opaque, threadIdx.x & 63u));       // (every lane of a tail's run retires)
    }
}

// Wide filters (Gaussian, tent; ImageBlock::put, imageblock.cpp:174-232,431-500), called by EVERY lane of a wave whose lanes are in lane
// order, so that its 64 lanes belong to one or two pixels.  v is a lane's record before the filter weight: what ImageBlock::put multiplies
// by the weight, W's entry (index WI) being 1; WI < 0: a record without W.  live(k) is a wave-uniform "channel k is accumulated"; a
// channel that is not costs no reduction and its total is 0.
//
// Lanes with the same footprint origin form a group (first lane with a sample left = leader; the others compare keys with it).  The
// group's footprint is reduced inside the wave, one butterfly per cell and live channel; lane c keeps the totals of cell (chunk base + c)
// and, when a chunk of (up to) 64 cells is complete, calls flush(x, y, totals) for its cell if that lies inside the crop window (x, y
// relative to it).  Compared with splatting per sample this divides the float atomics by the group size (up to 64).  The rules:
//  1. A cell of weight zero is skipped unless a non-finite value made a total NaN: imageblock.cpp adds value * 0 there.  The filters are
//     non-negative, so "W's total is nonzero or some total is NaN" says it; without W, "some total is nonzero or NaN" names the same
//     cells up to ones whose adds are all zeros.
//  2. Lanes outside the group add exact zeros, not value * 0: their weight 0 would turn a non-finite value into NaN for this group's pixels.
//  3. Footprints wider than 8 x 8 pixels (gaussian stddev > 0.875, tent radius > 3.5) take several chunks; lanes past the last cell of
//     the last chunk hold nothing (cell <= ci).
// Every array is indexed by unrolled constants and stays in registers.
template <int NC, int WI, typename Live, typename Flush>
DEV void film_walk(FilmRef F, bool have, const FilmFootprint &fp, const float (&v)[NC], Live live, Flush flush) {
    const uint32_t me = threadIdx.x & 63u, key = fp.key();
    const int count = F.fcount, n_cells = count * count;
    unsigned long long todo = __ballot(have);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const bool mine = have && key == (uint32_t) __shfl((int) key, leader);
        const int gx = __shfl(fp.pix, leader), gy = __shfl(fp.piy, leader);
        float t[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) t[k] = 0.f;
        for (int ys = 0, ci = 0; ys < count; ++ys) {
            const float wy = mine ? rfilter_eval(F, fp.rely + (float) ys) : 0.f;
            for (int xs = 0; xs < count; ++xs, ++ci) {
                const float w = mine ? wy * rfilter_eval(F, fp.relx + (float) xs) : 0.f;
                const bool keep = (int) me == (ci & 63);
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    if (!live(k)) continue;
                    const float s = wave_sum(mine ? v[k] * w : 0.f);
                    if (keep) t[k] = s;
                }
                if ((ci & 63) != 63 && ci != n_cells - 1) continue;
                const int cell = (ci & ~63) + (int) me;
                bool add = false;
#pragma unroll
                for (int k = 0; k < NC; ++k) add = add || ((WI < 0 || k == WI) ? t[k] != 0.f : t[k] != t[k]);      // (NaN != 0 too)
                if (cell <= ci && add) {
                    const int cy = cell / count, cx = cell - cy * count;
                    const int x = gx - F.crop_offset_x + cx, y = gy - F.crop_offset_y + cy;
                    if (x >= 0 && x < F.width && y >= 0 && y < F.height) flush(x, y, t);
                }
#pragma unroll
                for (int k = 0; k < NC; ++k) t[k] = 0.f;
            }
        }
        todo &= ~__ballot(mine);
    }
}
