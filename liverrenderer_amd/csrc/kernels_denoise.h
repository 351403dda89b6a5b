// Guided denoiser: the edge-avoiding A-Trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) with albedo
// demodulation, as DESIGN.md section 9 specifies it.  Three kernels: k_denoise_pack (prologue: demodulate, build the
// 16-byte records, mark the pixels that are not filtered), k_denoise_pass (one launch per pass, 25 gathered taps per pixel)
// and k_denoise_unpack (epilogue: re-modulate, the caller's layout).  Every operation is a separately rounded float32
// operation in the order the specification fixes (-ffp-contract=off), exp is dmath.h's m_exp: tests/denoise_ref.py restates
// the same text in numpy and the device's lanes are compared with it bit for bit.
#pragma once
#include "dmath.h"

namespace lrt {

// A pixel that is not filtered (its colour, alpha or a guide is not finite) carries a NaN in the first component of its
// colour record; the passes copy such a record and skip it as a tap, the epilogue puts the caller's own values back.
DEV bool dn_finite(float x) { return __builtin_fabsf(x) < kInf; }
DEV bool dn_marked(const float4 &c) { return c.x != c.x; }

// squared norm of a difference: ((dx * dx + dy * dy) + dz * dz)
DEV float dn_dist2(const float4 &a, const float4 &b) {
    float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// colour[p] = {c0.r, c0.g, c0.b, alpha}; normal[p] = {n.x, n.y, n.z, 0}; albedo[p] = {a.r, a.g, a.b, 0} (the raw albedo: the
// divisor d = max(a, eps_a) is formed again by the epilogue)
template <bool ALB, bool NRM, bool ALPHA>
__global__ __launch_bounds__(256) void k_denoise_pack(const float *__restrict__ noisy, int channels, const float *__restrict__ albedo,
                                                      const float *__restrict__ normals, float eps_a, uint32_t n_pixels,
                                                      float4 *__restrict__ colour, float4 *__restrict__ g_normal, float4 *__restrict__ g_albedo) {
    uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pixels) return;
    const float *src = noisy + (size_t) p * channels;
    float4 c = make_float4(src[0], src[1], src[2], channels == 4 ? src[3] : 1.f);
    bool ok = true;
    if (ALB) {
        float4 a = make_float4(albedo[(size_t) p * 3], albedo[(size_t) p * 3 + 1], albedo[(size_t) p * 3 + 2], 0.f);
        ok = ok && dn_finite(a.x) && dn_finite(a.y) && dn_finite(a.z);
        c.x = c.x / (a.x > eps_a ? a.x : eps_a);
        c.y = c.y / (a.y > eps_a ? a.y : eps_a);
        c.z = c.z / (a.z > eps_a ? a.z : eps_a);
        g_albedo[p] = a;
    }
    if (NRM) {
        float4 n = make_float4(normals[(size_t) p * 3], normals[(size_t) p * 3 + 1], normals[(size_t) p * 3 + 2], 0.f);
        ok = ok && dn_finite(n.x) && dn_finite(n.y) && dn_finite(n.z);
        g_normal[p] = n;
    }
    ok = ok && dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z);
    if (ALPHA) ok = ok && dn_finite(c.w);
    if (!ok) c = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
    colour[p] = c;
}

#define LRT_DN_BX 64
#define LRT_DN_BY 4

// One pass: c_out(p) = sum(w * c_in(q)) / sum(w) over the taps q = p + s * (i, j), j = -2 .. 2 outermost, i = -2 .. 2 innermost.
// A row of five taps is fetched with clamped addresses before it is used, so that the loads are unconditional and issue back to
// back; a tap outside the image or a marked one is left out of both sums.
template <bool ALB, bool NRM, bool ALPHA>
__global__ __launch_bounds__(LRT_DN_BX * LRT_DN_BY) void k_denoise_pass(const float4 *__restrict__ c_in, const float4 *__restrict__ g_normal,
                                                                        const float4 *__restrict__ g_albedo, float4 *__restrict__ c_out,
                                                                        int w, int h, int s, float ic, float in, float ia) {
    int x = (int) (blockIdx.x * LRT_DN_BX + threadIdx.x), y = (int) (blockIdx.y * LRT_DN_BY + threadIdx.y);
    if (x >= w || y >= h) return;
    size_t p = (size_t) y * w + x;
    float4 cp = c_in[p];
    if (dn_marked(cp)) { c_out[p] = cp; return; }
    float4 np = make_float4(0.f, 0.f, 0.f, 0.f), ap = np;
    if (NRM) np = g_normal[p];
    if (ALB) ap = g_albedo[p];
    const float hk[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sa = 0.f;
    #pragma unroll
    for (int j = 0; j < 5; ++j) {
        int qy = y + s * (j - 2);
        if (qy < 0 || qy >= h) continue;
        float4 cq[5], nq[5], aq[5]; bool in_x[5];
        #pragma unroll
        for (int i = 0; i < 5; ++i) {
            int qx = x + s * (i - 2);
            in_x[i] = qx >= 0 && qx < w;
            size_t q = (size_t) qy * w + (in_x[i] ? qx : x);
            cq[i] = c_in[q];
            if (NRM) nq[i] = g_normal[q];
            if (ALB) aq[i] = g_albedo[q];
        }
        #pragma unroll
        for (int i = 0; i < 5; ++i) {
            float e = dn_dist2(cp, cq[i]) * ic;
            if (NRM) e = e + dn_dist2(np, nq[i]) * in;
            if (ALB) e = e + dn_dist2(ap, aq[i]) * ia;
            float wt = (hk[i] * hk[j]) * m_exp(-e);
            if (in_x[i] && !dn_marked(cq[i])) {
                sw = sw + wt;
                sr = sr + wt * cq[i].x; sg = sg + wt * cq[i].y; sb = sb + wt * cq[i].z;
                if (ALPHA) sa = sa + wt * cq[i].w;
            }
        }
    }
    c_out[p] = make_float4(sr / sw, sg / sw, sb / sw, ALPHA ? sa / sw : cp.w);
}

// out(p) = c_N(p) * d(p), alpha from the record (filtered, or the input's own); a marked pixel gets the caller's values back
template <bool ALB>
__global__ __launch_bounds__(256) void k_denoise_unpack(const float4 *__restrict__ colour, const float4 *__restrict__ g_albedo, const float *__restrict__ noisy,
                                                        int channels, float eps_a, uint32_t n_pixels, float *__restrict__ out) {
    uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pixels) return;
    float4 c = colour[p];
    float *dst = out + (size_t) p * channels;
    if (dn_marked(c)) {
        const float *src = noisy + (size_t) p * channels;
        for (int k = 0; k < channels; ++k) dst[k] = src[k];
        return;
    }
    if (ALB) {
        float4 a = g_albedo[p];
        c.x = c.x * (a.x > eps_a ? a.x : eps_a);
        c.y = c.y * (a.y > eps_a ? a.y : eps_a);
        c.z = c.z * (a.z > eps_a ? a.z : eps_a);
    }
    dst[0] = c.x; dst[1] = c.y; dst[2] = c.z;
    if (channels == 4) dst[3] = c.w;
}

} // namespace lrt
