// The body of k_render_prb and k_render_prb_grid (kernels_prb.h), included inside each kernel: no include guard, not a header of its own.
// In scope: scp, lp and the constants ADJOINT, BLOCK, LDS_BVH, LD, HET, GRID.
    constexpr RecordLayout LAYOUT = record_layout(HET ? LRT_INTEGRATOR_VOLPATH_HET : LRT_INTEGRATOR_PRBVOLPATH);      // + the delta_L stream (record_layout.h)
    SceneRef sc = *scp;
    const LRT_CONST DLaunch &A = *lp;
    RpRef rp = A.rp;
    const LRT_CONST DLdsInfo &li = A.li;
    const uint32_t P = A.P;
    float4 *__restrict__ L_buf = A.L_buf; const float *__restrict__ grad_image = A.grad_image; const float *__restrict__ wfilm = A.wfilm;
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ uint32_t s_in[3], s_out[3], s_ticket, s_fresh;
    __shared__ unsigned long long s_fresh_base;
    __shared__ double s_grad[7];
    const uint32_t tid = threadIdx.x, lane_in_wave = tid & 63u;
    LdsScene L{};
    if (LDS_BVH) {
        const uint4 *src = li.blob; uint4 *dst = reinterpret_cast<uint4 *>(smem);
        for (uint32_t k = tid; k < li.blob_bytes / 16u; k += BLOCK) dst[k] = src[k];
        L.nodes = reinterpret_cast<const float4 *>(smem + li.nodes_off); L.verts = reinterpret_cast<const float4 *>(smem + li.verts_off);
        L.tris = reinterpret_cast<const uint2 *>(smem + li.tris_off);
        L.n_faces = sc.n_faces; L.root_is_leaf = (uint32_t) sc.root_is_leaf; L.root_first = sc.root_leaf_first; L.root_count = sc.root_leaf_count;
    }
    const LdsTracer<BLOCK> tr_lds{ L, reinterpret_cast<uint16_t *>(smem + li.stack_off) + tid };
    const GlobalTracer tr_glb{ sc, reinterpret_cast<int *>(smem) + tid };
    const size_t pool = (size_t) blockIdx.x * 2u * P;
    uint32_t parity = 0;                                      // queue the round reads: parity ? q1 : q0 (scalar loads at the point of use)
    if (tid == 0) { s_in[0] = s_in[1] = s_in[2] = 0; }
    if (tid < 7) s_grad[tid] = 0.0;
    bool lanes_left = true;                                   // thread 0
    uint32_t n_shadow = 0, n_trips = 0, n_loaded = 0;
    for (;;) {
        if (tid == 0) {
            const uint32_t want = P - (s_in[0] + s_in[1] + s_in[2]);
            uint32_t got = 0; unsigned long long base = 0;
            if (want && lanes_left) {
                base = atomicAdd(&A.cnt->next_lane, (unsigned long long) want);
                if (base < rp.n_lanes) got = (uint32_t) (rp.n_lanes - base < (unsigned long long) want ? rp.n_lanes - base : (unsigned long long) want);
                lanes_left = base + want < rp.n_lanes;
            }
            s_fresh = got; s_fresh_base = base; s_ticket = 0; s_out[0] = s_out[1] = s_out[2] = 0;
        }
        __syncthreads();
        // queue regions as in k_render: A [0, n_a) proven-free in-medium paths, C [P, P + n_c) in-medium paths that need their
        // ray query, B 2P-1-j paths outside media
        const uint32_t n_a = s_in[0], n_c = s_in[1], n_s = s_in[2], fresh = s_fresh;
        const unsigned long long fresh_base = s_fresh_base;
        if (n_a + n_c + n_s + fresh == 0) break;
        const uint32_t ta = (n_a + 63u) >> 6, tc = (n_c + 63u) >> 6, ts = (n_s + 63u) >> 6, tf = (fresh + 63u) >> 6, tm = ta + tc;
        for (;;) {
            uint32_t t = 0;
            if (lane_in_wave == 0) t = atomicAdd(&s_ticket, 1u);
            t = (uint32_t) __builtin_amdgcn_readfirstlane((int) t);
            if (t >= tm + ts + tf) break;
            bool had_path = false, alive = false;
            PathState s; s.flags = 0; s.lane = 0; s.res = V3(0.f);
            float4 dl = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < tm + ts) {
                uint32_t i;
                if (t < ta) { i = (t << 6) + lane_in_wave; had_path = i < n_a; }
                else if (t < tm) { i = ((t - ta) << 6) + lane_in_wave; had_path = i < n_c; i += P; }
                else { i = ((t - tm) << 6) + lane_in_wave; had_path = i < n_s; i = 2u * P - 1u - i; }
                if (had_path) { load_state<LAYOUT>(parity ? A.q1 : A.q0, pool + i, s); dl = (parity ? A.dl1 : A.dl0)[pool + i]; n_loaded += 1; }
            } else {
                const uint32_t i = ((t - tm - ts) << 6) + lane_in_wave;
                had_path = i < fresh;
                if (had_path) {                                // common.py:231-309 + prbvolpath.py:113-137
                    const unsigned long long slot = fresh_base + i;
                    s = generate_camera_path<LD>(sc, rp, A.pixel_list, A.lane_begin + slot);
                    s.flags = PF_SPECULAR | (s.flags & (3u << PF_CHANNEL_SHIFT));      // valid_ray = false, specular_chain = true, medium = none
                    V3 dL(0.f);
                    if (ADJOINT) { float4 l = L_buf[slot]; s.res = V3(l.x, l.y, l.z); dL = lane_delta_L(sc, rp, s.lane, grad_image, wfilm); }
                    dl = make_float4(dL.x, dL.y, dL.z, u2f((uint32_t) slot));
                }
            }
            PrbGrads G; G.sigma_t[0] = G.sigma_t[1] = G.sigma_t[2] = G.albedo[0] = G.albedo[1] = G.albedo[2] = G.g = 0.f;
            if (had_path) {
                SamplerT<LD> rng = lane_rng_resume<LD>(rp, s.lane, s.rng_state);
                alive = LDS_BVH ? prb_iteration<ADJOINT, HET, GRID>(sc, rp, s, rng, tr_lds, n_shadow, V3(dl.x, dl.y, dl.z), G, GRID ? A.dgrid : nullptr)
                                : prb_iteration<ADJOINT, HET, GRID>(sc, rp, s, rng, tr_glb, n_shadow, V3(dl.x, dl.y, dl.z), G, GRID ? A.dgrid : nullptr);
                s.rng_state = rng.state;
                n_trips += 1;
            }
            if (!ADJOINT) {
                if (L_buf) { if (had_path && !alive) L_buf[f2u(dl.w)] = make_float4(s.res.x, s.res.y, s.res.z, (s.flags & PF_VALID) ? 1.f : 0.f); }
                else finish_paths_wave(sc, rp, A.film, A.sample_out, A.sample_base, had_path && !alive, s.lane, s.res, (s.flags & PF_VALID) != 0);
            } else {
                float g[7] = { G.sigma_t[0], G.sigma_t[1], G.sigma_t[2], G.albedo[0], G.albedo[1], G.albedo[2], G.g };
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    const float v = wave_sum(g[k]);
                    if (lane_in_wave == 0 && v != 0.f) atomicAdd(&s_grad[k], (double) v);
                }
            }
            // compaction into the three regions
            const int region = !(s.flags & PF_MEDIUM_MASK) ? 2 : ((s.flags & PF_NOHIT) ? 0 : 1);
            const unsigned long long m0 = __ballot(alive && region == 0), m1 = __ballot(alive && region == 1), m2 = __ballot(alive && region == 2);
            uint32_t base = 0;
            if (lane_in_wave < 3) { const uint32_t c = (uint32_t) __popcll(lane_in_wave == 0 ? m0 : (lane_in_wave == 1 ? m1 : m2)); if (c) base = atomicAdd(&s_out[lane_in_wave], c); }
            const uint32_t b0 = (uint32_t) __builtin_amdgcn_readlane((int) base, 0), b1 = (uint32_t) __builtin_amdgcn_readlane((int) base, 1), b2 = (uint32_t) __builtin_amdgcn_readlane((int) base, 2);
            const uint32_t b = region == 0 ? b0 : (region == 1 ? b1 : b2);          // (v_readlane, not a shuffle through LDS: see retire_and_compact_wave)
            if (alive) {
                const uint32_t slot = b + (uint32_t) __popcll((region == 0 ? m0 : (region == 1 ? m1 : m2)) & ((1ull << lane_in_wave) - 1ull));
                const uint32_t rec = region == 0 ? slot : (region == 1 ? P + slot : 2u * P - 1u - slot);
                store_state<LAYOUT>(parity ? A.q0 : A.q1, pool + rec, s); (parity ? A.dl0 : A.dl1)[pool + rec] = dl;
            }
        }
        __syncthreads();
        if (tid == 0) { s_in[0] = s_out[0]; s_in[1] = s_out[1]; s_in[2] = s_out[2]; }
        parity ^= 1u;
    }
    if (ADJOINT && tid < 7 && s_grad[tid] != 0.0) atomicAdd(&A.grads[tid], s_grad[tid]);
    for (int off = 32; off > 0; off >>= 1) {
        n_shadow += __shfl_down(n_shadow, off); n_trips += __shfl_down(n_trips, off); n_loaded += __shfl_down(n_loaded, off);
    }
    if (lane_in_wave == 0) {
        if (n_shadow) atomicAdd(&A.cnt->n_shadow, (unsigned long long) n_shadow);
        if (n_trips) atomicAdd(&A.cnt->n_iter, (unsigned long long) n_trips);
        if (n_loaded) atomicAdd(&A.cnt->n_records, (unsigned long long) n_loaded);
    }
