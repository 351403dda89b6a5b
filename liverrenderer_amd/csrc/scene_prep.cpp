// Host half of the scene upload (scene_prep.h): the device image of an lrt_scene_desc as host arrays, the media tables, the resolved
// render options, the tile lists and the proof predicate of the 64-byte records.  Plain host arithmetic, no HIP runtime call.
#include "scene_prep.h"
#include "scene_check.h"
#include <functional>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <stdexcept>
#include <string>

namespace lrt {

PrepOptions PrepOptions::from_env() {
    PrepOptions o;
    if (getenv("LRT_BVH_LEAF")) o.bvh_leaf = std::max(1, atoi(getenv("LRT_BVH_LEAF")));
    o.no_lds_bvh = getenv("LRT_NO_LDS_BVH") != nullptr;
    o.no_dist_grid = getenv("LRT_NO_DIST_GRID") != nullptr;
    if (getenv("LRT_DIST_GRID_RES")) o.dist_grid_res = std::max(8, std::min(256, atoi(getenv("LRT_DIST_GRID_RES"))));
    o.no_nee_reject = getenv("LRT_NO_NEE_REJECT") != nullptr;
    o.no_cone_proof = getenv("LRT_NO_CONE_PROOF") != nullptr;
    o.no_primary_entry = getenv("LRT_NO_PRIMARY_ENTRY") != nullptr;
    return o;
}

static void m4_mul(const float *a, const float *b, float *r) {
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { float s = a[4 * i] * b[j]; for (int k = 1; k < 4; ++k) s = fmaf(a[4 * i + k], b[4 * k + j], s); r[4 * i + j] = s; }
}
static void m4_ident(float *m) { for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.f : 0.f; }

// include/mitsuba/render/sensor.h:234-269 + include/mitsuba/core/transform.h:393-410:
// sample_to_camera = inverse of (scale * translate * scale * translate * perspective), built
// from the analytic inverses exactly as Transform::inverse_transpose composes them.
void build_camera(const lrt_scene_desc &d, DCamera &cam, DFilm &film) {
    const lrt_film_desc &F = d.film; const lrt_sensor_desc &C = d.sensor;
    float fw = (float) F.width, fh = (float) F.height;
    float rsx = (float) F.crop_width / fw, rsy = (float) F.crop_height / fh, rox = (float) F.crop_offset_x / fw, roy = (float) F.crop_offset_y / fh;
    float aspect = fw / fh, recip = 1.f / (C.far_clip - C.near_clip);
    float tn = (float) tan((double) (C.fov_x * .5f) * (3.14159265358979323846 / 180.0));
    (void) recip;
    float S1i[16], T1i[16], S2i[16], T2i[16], Pit[16], t0[16], t1[16], t2[16], it[16];
    m4_ident(S1i); S1i[0] = 1.f / (1.f / rsx); S1i[5] = 1.f / (1.f / rsy); S1i[10] = 1.f / 1.f;
    m4_ident(T1i); T1i[12] = rox; T1i[13] = roy; T1i[14] = -0.f;
    m4_ident(S2i); S2i[0] = 1.f / -0.5f; S2i[5] = 1.f / (-0.5f * aspect); S2i[10] = 1.f;
    m4_ident(T2i); T2i[12] = 1.f; T2i[13] = 1.f / aspect; T2i[14] = -0.f;
    // inverse of the perspective matrix, transposed
    float Pinv[16]; m4_ident(Pinv); Pinv[0] = tn; Pinv[5] = tn; Pinv[10] = 0.f; Pinv[15] = 1.f / C.near_clip; Pinv[11] = 1.f;
    Pinv[14] = (C.near_clip - C.far_clip) / (C.far_clip * C.near_clip);
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) Pit[4 * i + j] = Pinv[4 * j + i];
    m4_mul(S1i, T1i, t0); m4_mul(t0, S2i, t1); m4_mul(t1, T2i, t2); m4_mul(t2, Pit, it);
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) cam.s2c[4 * i + j] = it[4 * j + i];
    memcpy(cam.to_world, C.to_world, sizeof(float) * 12);
    cam.near_clip = C.near_clip; cam.far_clip = C.far_clip; cam.medium = C.medium;
    cam.ppo_x = fw * C.principal_point_offset_x / (float) F.crop_width; cam.ppo_y = fh * C.principal_point_offset_y / (float) F.crop_height;

    film.width = F.crop_width; film.height = F.crop_height; film.crop_offset_x = F.crop_offset_x; film.crop_offset_y = F.crop_offset_y;
    film.scale_x = 1.f / (float) F.crop_width; film.scale_y = 1.f / (float) F.crop_height;
    film.offset_x = -(float) F.crop_offset_x * film.scale_x; film.offset_y = -(float) F.crop_offset_y * film.scale_y;
    film.has_alpha = F.has_alpha; film.channels = F.has_alpha ? 5 : 4; film.rfilter = F.rfilter;
    film.rf_radius = 0.5f; film.rf_inv_radius = 1.f;
    if (F.rfilter == LRT_RFILTER_GAUSSIAN) {             // src/rfilters/gaussian.cpp:52-95
        float stddev = F.rfilter_param; film.rf_radius = 4.f * stddev;
        static const double coeff[10] = { 9.992604880e-1, -4.977025247e-1, 1.222248550e-1, -1.932406282e-2, 2.136713061e-3,
                                          -1.679873860e-4, 9.202145248e-6, -3.329417433e-7, 7.128382794e-9, -6.821193280e-11 };
        double sc = 1; for (int i = 0; i < 10; ++i) { film.rf_coeff[i] = (float) (coeff[i] * sc); sc /= (double) stddev * (double) stddev; }
        float x = film.rf_radius * film.rf_radius, x2 = x * x, x4 = x2 * x2, x8 = x4 * x4; const float *c = film.rf_coeff;
        float a0 = fmaf(x, c[1], c[0]), a1 = fmaf(x, c[3], c[2]), a2 = fmaf(x, c[5], c[4]), a3 = fmaf(x, c[7], c[6]), a4 = fmaf(x, c[9], c[8]);
        float b0 = fmaf(x2, a1, a0), b1 = fmaf(x2, a3, a2), c0 = fmaf(x4, b1, b0);
        film.rf_coeff[0] -= fmaf(x8, a4, c0);
    } else if (F.rfilter == LRT_RFILTER_TENT) { film.rf_radius = F.rfilter_param; film.rf_inv_radius = 1.f / film.rf_radius; }
    film.fn = (int) ceilf(film.rf_radius - .5f); film.fcount = 2 * film.fn + 1;
}

static void inverse3(const float *m16, float *out9) {    // double-precision inverse of the linear part
    double m[3][3]; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) m[i][j] = m16[4 * i + j];
    double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    double id = 1.0 / det;
    out9[0] = (float) ((m[1][1] * m[2][2] - m[1][2] * m[2][1]) * id); out9[1] = (float) ((m[0][2] * m[2][1] - m[0][1] * m[2][2]) * id); out9[2] = (float) ((m[0][1] * m[1][2] - m[0][2] * m[1][1]) * id);
    out9[3] = (float) ((m[1][2] * m[2][0] - m[1][0] * m[2][2]) * id); out9[4] = (float) ((m[0][0] * m[2][2] - m[0][2] * m[2][0]) * id); out9[5] = (float) ((m[0][2] * m[1][0] - m[0][0] * m[1][2]) * id);
    out9[6] = (float) ((m[1][0] * m[2][1] - m[1][1] * m[2][0]) * id); out9[7] = (float) ((m[0][1] * m[2][0] - m[0][0] * m[2][1]) * id); out9[8] = (float) ((m[0][0] * m[1][1] - m[0][1] * m[1][0]) * id);
}

static uint32_t log2i_ceil(uint32_t v) { uint32_t r = 0; while ((1u << r) < v) ++r; return r; }

// include/mitsuba/core/distr_2d.h:403-510 (normalised, single slice); levels are
// concatenated with 16-byte aligned offsets so that a 2x2 patch is one float4 load.
static void build_hierarchy(const std::vector<float> &lum, uint32_t w, uint32_t h, DEnv &E, std::vector<float> &out) {
    uint32_t npx = w - 1, npy = h - 1;
    E.patch_size[0] = 1.f / (float) npx; E.patch_size[1] = 1.f / (float) npy;
    E.inv_patch_size[0] = (float) npx; E.inv_patch_size[1] = (float) npy;
    E.max_patch[0] = npx - 1; E.max_patch[1] = npy - 1;
    uint32_t max_level = log2i_ceil(std::max(npx, npy));
    struct L { uint32_t w, h, off; };
    std::vector<L> lv; uint32_t total = 0;
    auto add = [&](uint32_t lw, uint32_t lh) { lv.push_back({ lw, lh, total }); total += (lw * lh + 3u) & ~3u; };
    add(w, h);
    uint32_t lx = npx, ly = npy;
    for (int level = (int) max_level; level >= 0; --level) { lx += lx & 1u; ly += ly & 1u; add(lx, ly); lx >>= 1; ly >>= 1; }
    if (lv.size() > LRT_MAX_HIER_LEVELS) throw std::runtime_error("environment map too large for the sampling hierarchy");
    out.assign(total, 0.f);
    auto index = [](uint32_t x, uint32_t y, uint32_t width) { return ((x & 1u) | (((x & ~1u) | (y & 1u)) << 1)) + ((y & ~1u) * width); };
    float *l0 = &out[lv[0].off], *l1 = &out[lv[1].off];
    const float *in = lum.data(); double sum = 0.0;
    for (uint32_t y = 0; y < npy; ++y) { for (uint32_t x = 0; x < npx; ++x) { float avg = .25f * (in[0] + in[1] + in[w] + in[w + 1]); sum += (double) avg; l1[index(x, y, lv[1].w)] = avg; ++in; } ++in; }
    float scale = (float) ((double) (npx * npy) / sum);
    for (uint32_t i = 0; i < w * h; ++i) l0[i] = lum[i] * scale;
    for (uint32_t i = 0; i < lv[1].w * lv[1].h; ++i) l1[i] *= scale;
    lx = npx; ly = npy;
    for (uint32_t level = 2; level <= max_level + 1; ++level) {
        const float *a = &out[lv[level - 1].off]; float *b = &out[lv[level].off];
        lx = (lx + 1u) >> 1; ly = (ly + 1u) >> 1;
        for (uint32_t y = 0; y < ly; ++y) for (uint32_t x = 0; x < lx; ++x) { const float *d0 = a + index(x * 2, y * 2, lv[level - 1].w); b[index(x, y, lv[level].w)] = d0[0] + d0[1] + d0[2] + d0[3]; }
    }
    E.n_levels = (int) lv.size();
    for (size_t i = 0; i < lv.size(); ++i) { E.level_offset[i] = lv[i].off; E.level_width[i] = lv[i].w; }
}

// The LDS image of a BVH: [nodes | float4 vertices | 8-byte triangle slots], then the 16-bit traversal stacks of 1024 threads
// (max_depth + 2 entries per lane)
struct LdsLayout {
    size_t nodes_b, verts_b, tris_b, stacks_b;
    size_t blob() const { return nodes_b + verts_b + tris_b; }
    size_t total() const { return blob() + stacks_b; }
};
static LdsLayout lds_layout(const HostBVH &b, uint32_t n_vertices) {
    return { b.nodes.size() / 16 * 64, ((size_t) n_vertices * 16 + 15) & ~size_t(15), (b.tris.size() / 12 * 8 + 15) & ~size_t(15), (size_t) 2 * (b.max_depth + 2) * 1024 };
}
size_t lds_image_bytes(const HostBVH &b, uint32_t n_vertices) { return lds_layout(b, n_vertices).total(); }

// the part of lds_image_fits that needs no BVH: decides whether the leaf-size search runs at all
static bool lds_possible(const lrt_scene_desc &d, const PrepOptions &opt) { return d.n_faces > 0 && d.n_faces <= 32767 && d.n_vertices <= 65535 && !opt.no_lds_bvh; }
bool lds_image_fits(const lrt_scene_desc &d, const HostBVH &b, const PrepOptions &opt) {
    return lds_possible(d, opt) && b.nodes.size() / 16 <= 32767 && b.tris.size() / 12 <= 32767 && lds_image_bytes(b, d.n_vertices) <= opt.lds_limit;
}

// 16-bit vertex indices, `face << 1 | last slot of its leaf`, child references as 0x8000 | first slot
static void build_lds_image(const lrt_scene_desc &d, const HostBVH &bvh, PreparedScene &P) {
    const LdsLayout lay = lds_layout(bvh, d.n_vertices);
    const size_t n_nodes = bvh.nodes.size() / 16, n_slots = bvh.tris.size() / 12, n_verts = d.n_vertices;
    const size_t nodes_b = lay.nodes_b, verts_b = lay.verts_b;
    std::vector<unsigned char> &blob = P.lds_blob; blob.assign(lay.blob(), 0);
    memcpy(blob.data(), bvh.nodes.data(), nodes_b);
    float *v = reinterpret_cast<float *>(blob.data() + nodes_b);
    for (size_t i = 0; i < n_verts; ++i) { v[4 * i] = d.positions[3 * i]; v[4 * i + 1] = d.positions[3 * i + 1]; v[4 * i + 2] = d.positions[3 * i + 2]; v[4 * i + 3] = 0.f; }
    uint16_t *t = reinterpret_cast<uint16_t *>(blob.data() + nodes_b + verts_b);
    for (size_t sl = 0; sl < n_slots; ++sl) {               // 4th word: face index << 1 | "last slot of its leaf"
        uint32_t f; memcpy(&f, &bvh.tris[12 * sl + 3], 4);
        for (int k = 0; k < 3; ++k) t[4 * sl + k] = (uint16_t) d.faces[3 * (size_t) f + k];
        t[4 * sl + 3] = (uint16_t) (f << 1);
    }
    for (size_t n = 0; n < n_nodes; ++n) {                 // mark the last slot of every leaf (trace_lds)
        int32_t refs[4]; memcpy(refs, &bvh.nodes[16 * n + 12], 16);
        for (int c = 0; c < 2; ++c) if (refs[c] < 0 && refs[2 + c] > 0) t[4 * ((size_t) (uint32_t) ~refs[c] + (size_t) refs[2 + c] - 1) + 3] |= 1;
        // child references as trace_lds's 16-bit work items (inner node index, or 0x8000 | first slot of the leaf)
        uint32_t enc[2]; for (int c = 0; c < 2; ++c) enc[c] = refs[c] < 0 ? (0x8000u | (uint32_t) ~refs[c]) : (uint32_t) refs[c];
        memcpy(blob.data() + 64 * n + 48, enc, 8);
    }
    // no node names a root leaf: its last slot is marked here, so that the flag holds for every leaf (trace_lds walks a root leaf by its count and does not read it)
    if (bvh.root_is_leaf && bvh.root_count) t[4 * ((size_t) bvh.root_first + bvh.root_count - 1) + 3] |= 1;
    P.lds.blob = nullptr; P.lds.blob_bytes = (uint32_t) blob.size(); P.lds.nodes_off = 0; P.lds.verts_off = (uint32_t) nodes_b; P.lds.tris_off = (uint32_t) (nodes_b + verts_b);
    P.lds.stack_off = (uint32_t) blob.size(); P.lds.total_bytes = (uint32_t) lay.total();
}

// Two boxes with two meanings, kept apart on purpose.
// The distance field's: the vertices that faces reference, and the spheres.
static void referenced_bounds(const lrt_scene_desc &d, const std::vector<DSphere> &spheres, float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (uint32_t f = 0; f < 3 * d.n_faces; ++f) for (int a = 0; a < 3; ++a) { float v = d.positions[3 * (size_t) d.faces[f] + a]; lo[a] = std::min(lo[a], v); hi[a] = std::max(hi[a], v); }
    for (const DSphere &o : spheres) for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], o.center[a] - o.radius); hi[a] = std::max(hi[a], o.center[a] + o.radius); }
}
// The scene's (src/render/scene.cpp:49, the bounding sphere's): all vertices, unreferenced ones included, and the spheres.
static void vertex_bounds(const lrt_scene_desc &d, const std::vector<DSphere> &spheres, float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (uint32_t i = 0; i < d.n_vertices; ++i) for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], d.positions[3 * i + a]); hi[a] = fmaxf(hi[a], d.positions[3 * i + a]); }
    for (const DSphere &o : spheres) for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], o.center[a] - o.radius); hi[a] = fmaxf(hi[a], o.center[a] + o.radius); }   // Sphere::bbox
}

// ---- the per-face cone table (scene_prep.h: build_cone_table).  Float64 throughout; the margins below are for the device's float32.
// Face f, side normal nu (unit), h(x) = (x - a) . nu the height over f's plane, nu_e the in-plane unit normal of edge e pointing away from the face.
// Origins.  The device interpolates the hit point in float32 (compute_si: b0 = 1 - b1 - b2, three fused products per coordinate: below 9 * 2^-24 * amax
// from a point of the triangle, amax the face's largest |coordinate|) and moves it by mag = (1 + max|p|) * kRayEpsilon along its own float32 normal
// (offset_p; one more rounding).  That normal is within 2^-22 / sin(angle at vertex 0) of nu; faces where that sine is below 2e-3 get no row, so the
// normal is within 2.5e-4 rad: a lateral shift of mag * 2.5e-4, and a cosine off by less than the 1e-3 by which every bin is widened here.
// tau = 2e-6 * amax + 1e-9 bounds all of it; mag lies in [mag_min, mag_max] computed from the face's coordinates.
// Region.  A point o + t w, w within theta of nu, has h = h_o + t cos(angle) and has moved sideways by at most (h - h_o) tan(theta): all points
// that segments of the bin can reach lie in Q = { h >= -tau } and { (x - p_e) . nu_e <= h tan(theta) + tau (1 + tan(theta)) for the three edges },
// and a point at height h is reached only by t >= h - h_o.  So a triangle whose part inside Q stays at heights >= hmin bounds nothing shorter
// than hmin - mag_max - 2 tau, and R is the minimum over all other triangles (clipped to Q with Sutherland-Hodgman; hmin over the polygon's vertices).
// Neighbours touch Q at h = 0 and are decided exactly instead (vertices are matched by position, not by index: an OBJ splits a vertex by
// its normals).  The reachable set itself keeps a margin mag_min * tan(theta) - tau > 0 inside the edge planes and mag_min - tau above the face's;
// bins where tau reaches a quarter of the former get 0.
//   shared edge e: the neighbour is the hull of the edge and its far vertex w, and phi_e(x) = (x - p_e) . nu_e - h(x) tan(theta) and h are linear
//     and vanish on the edge: the neighbour stays out iff phi_e(w) > 0 or h(w) < 0.  Otherwise R = 0.
//   shared vertex v: Q lies in the cone { h >= 0, phi <= 0 for the two edges at v } with apex v, and the neighbour is the hull of v and its far
//     edge: it meets the cone away from v iff the far edge does.  Then R = 0.
//   all three: R = 0.  A degenerate neighbour (two of its vertices at one position) that touches f: R = 0.
// Triangles that come close without sharing a vertex (T-junctions, vertices that almost coincide) go through the clip and give R = 0.
namespace {
struct D3 { double x, y, z; };
inline D3 operator-(D3 a, D3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline D3 operator+(D3 a, D3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
inline D3 operator*(D3 a, double s) { return { a.x * s, a.y * s, a.z * s }; }
inline double dot3(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline D3 cross3(D3 a, D3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
inline double len3(D3 a) { return std::sqrt(dot3(a, a)); }
struct ConePlane { D3 n; double c; };                  // inside: n . x <= c
// the smallest `hn . x` over the part of polygon `poly` (n <= 3 vertices) inside the four planes; false: that part is empty
bool clip_min_height(const D3 *tri, const ConePlane *pl, D3 hn, double &hmin) {
    D3 a[8], b[8]; int n = 3; for (int i = 0; i < 3; ++i) a[i] = tri[i];
    for (int p = 0; p < 4 && n > 0; ++p) {
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const D3 u = a[i], v = a[(i + 1) % n];
            const double su = dot3(pl[p].n, u) - pl[p].c, sv = dot3(pl[p].n, v) - pl[p].c;
            if (su <= 0.0) b[m++] = u;
            if ((su <= 0.0) != (sv <= 0.0)) { const double t = su / (su - sv); b[m++] = u + (v - u) * t; }
        }
        n = m; for (int i = 0; i < n; ++i) a[i] = b[i];
    }
    if (n == 0) return false;
    hmin = INFINITY; for (int i = 0; i < n; ++i) hmin = std::min(hmin, dot3(hn, a[i]));
    return true;
}
uint16_t half_round_down(double v) {                   // the largest binary16 <= v; below the smallest normal number: 0
    float f = (float) v; if ((double) f > v) f = std::nextafterf(f, 0.f);
    if (!(f >= 6.103515625e-5f)) return 0;
    if (f >= 65504.f) return 0x7bff;
    uint32_t u; memcpy(&u, &f, 4);
    return (uint16_t) ((((u >> 23) - 112u) << 10) | ((u >> 13) & 0x3ffu));
}
}
float cone_table_value(uint16_t h) {
    if (!h) return 0.f;
    const uint32_t u = (((uint32_t) (h >> 10) + 112u) << 23) | ((uint32_t) (h & 0x3ffu) << 13); float f; memcpy(&f, &u, 4); return f;
}

void build_cone_table(const lrt_scene_desc &d, std::vector<uint16_t> &out) {
    constexpr int K = LRT_CONE_BINS;
    const uint32_t nf = d.n_faces;
    out.assign((size_t) nf * 2 * K, 0);
    if (!nf) return;
    for (size_t i = 0; i < 3 * (size_t) d.n_vertices; ++i) if (!std::isfinite(d.positions[i])) return;
    const double bin_cos[K] = { LRT_CONE_COS0, LRT_CONE_COS1, LRT_CONE_COS2, LRT_CONE_COS3 };
    double tan_k[K], inv_cos_k[K];
    for (int k = 0; k < K; ++k) { const double c = bin_cos[k] - 1e-3; tan_k[k] = std::sqrt(1.0 - c * c) / c; inv_cos_k[k] = 1.0 / c; }
    // vertices at one position get one id
    std::vector<uint32_t> cid(d.n_vertices), order(d.n_vertices);
    for (uint32_t i = 0; i < d.n_vertices; ++i) order[i] = i;
    auto pos = [&](uint32_t v, int a) { return d.positions[3 * (size_t) v + a]; };
    std::sort(order.begin(), order.end(), [&](uint32_t u, uint32_t v) { for (int a = 0; a < 3; ++a) if (pos(u, a) != pos(v, a)) return pos(u, a) < pos(v, a); return false; });
    for (uint32_t i = 0, id = 0; i < d.n_vertices; ++i) {
        if (i && (pos(order[i], 0) != pos(order[i - 1], 0) || pos(order[i], 1) != pos(order[i - 1], 1) || pos(order[i], 2) != pos(order[i - 1], 2))) ++id;
        cid[order[i]] = id;
    }
    struct Face { D3 v[3], cen; double rad; uint32_t c[3]; bool dup; };
    std::vector<Face> F(nf);
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t f = 0; f < nf; ++f) {
        Face &T = F[f];
        for (int j = 0; j < 3; ++j) {
            const uint32_t v = d.faces[3 * (size_t) f + j];
            T.v[j] = { pos(v, 0), pos(v, 1), pos(v, 2) }; T.c[j] = cid[v];
            const double q[3] = { T.v[j].x, T.v[j].y, T.v[j].z };
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], q[a]); hi[a] = std::max(hi[a], q[a]); }
        }
        T.cen = (T.v[0] + T.v[1] + T.v[2]) * (1.0 / 3.0);
        T.rad = std::max(len3(T.v[0] - T.cen), std::max(len3(T.v[1] - T.cen), len3(T.v[2] - T.cen))) * (1.0 + 1e-12);
        T.dup = T.c[0] == T.c[1] || T.c[1] == T.c[2] || T.c[0] == T.c[2];
    }
    // No row claims more than an eighth of the scene's extent: it bounds the pairs that are looked at; free flights longer than that go to the balls or the query
    const double cap = 0.125 * std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    const double ray_eps = 1500.0 * 5.9604644775390625e-8;                              // kRayEpsilon (dmath.h)
    for (uint32_t f = 0; f < nf; ++f) {
        const Face &T = F[f];
        if (T.dup) continue;
        const D3 e1 = T.v[1] - T.v[0], e2 = T.v[2] - T.v[0], N = cross3(e1, e2);
        const double n2 = len3(N);
        if (!(n2 > 0.0) || n2 < 2e-3 * len3(e1) * len3(e2)) continue;
        double amax = 0.0, m_min = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double q[3] = { a == 0 ? T.v[0].x : (a == 1 ? T.v[0].y : T.v[0].z), a == 0 ? T.v[1].x : (a == 1 ? T.v[1].y : T.v[1].z), a == 0 ? T.v[2].x : (a == 1 ? T.v[2].y : T.v[2].z) };
            amax = std::max(amax, std::max(std::fabs(q[0]), std::max(std::fabs(q[1]), std::fabs(q[2]))));
            const bool one_sign = (q[0] > 0 && q[1] > 0 && q[2] > 0) || (q[0] < 0 && q[1] < 0 && q[2] < 0);
            if (one_sign) m_min = std::max(m_min, std::min(std::fabs(q[0]), std::min(std::fabs(q[1]), std::fabs(q[2]))));       // the least max|p| over the face is at least this
        }
        const double tau = 2e-6 * amax + 1e-9, mag_min = (1.0 + m_min) * ray_eps * (1.0 - 1e-5), mag_max = (1.0 + amax) * ray_eps * (1.0 + 1e-5);
        const double h_o_max = mag_max + tau;
        const uint32_t shape = d.face_shape ? d.face_shape[f] : 0u;
        const bool flip = shape < d.n_shapes && d.shapes[shape].flip_normals;
        D3 nu[2], ne[2][3]; double R[2][K];
        for (int s = 0; s < 2; ++s) {
            nu[s] = N * (((s == 0) != flip ? 1.0 : -1.0) / n2);
            for (int e = 0; e < 3; ++e) {                                                // edge e: from vertex e to vertex e + 1, opposite to vertex e + 2
                D3 m = cross3(T.v[(e + 1) % 3] - T.v[e], nu[s]); m = m * (1.0 / len3(m));
                if (dot3(T.v[(e + 2) % 3] - T.v[e], m) > 0.0) m = m * -1.0;
                ne[s][e] = m;
            }
            for (int k = 0; k < K; ++k) R[s][k] = tau < 0.25 * mag_min * tan_k[k] ? cap : 0.0;
        }
        // Two passes: the faces around f first (every neighbour is among them), which bring most rows down to their final length; then the others,
        // culled by bounding spheres against the widest cone at the height the rows still reach.
        bool dead = false;
        for (int pass = 0; pass < 2 && !dead; ++pass) {
        double base[2];
        for (int s = 0; s < 2; ++s) { double r = 0.0; for (int k = 0; k < K; ++k) r = std::max(r, R[s][k]); base[s] = T.rad + (r + h_o_max + tau) * inv_cos_k[K - 1] + 4.0 * tau; }
        for (uint32_t g = 0; g < nf; ++g) {
            if (g == f) continue;
            const Face &G = F[g];
            const D3 dc = G.cen - T.cen; const double dist2 = dot3(dc, dc), near = 3.0 * T.rad + G.rad, far = std::max(base[0], base[1]) + G.rad;
            if ((dist2 <= near * near) != (pass == 0) || dist2 > far * far) continue;
            int match[3], ns = 0;
            for (int j = 0; j < 3; ++j) { match[j] = -1; for (int i = 0; i < 3; ++i) if (G.c[j] == T.c[i]) match[j] = i; ns += match[j] >= 0; }
            if (ns == 3 || (ns > 0 && G.dup)) { for (int s = 0; s < 2; ++s) for (int k = 0; k < K; ++k) R[s][k] = 0.0; dead = true; break; }
            for (int s = 0; s < 2; ++s) {
                const D3 hn = nu[s]; const double h_off = dot3(hn, T.v[0]);
                if (ns == 2) {
                    int jw = 0, seen = 0; for (int j = 0; j < 3; ++j) { if (match[j] < 0) jw = j; else seen |= 1 << match[j]; }
                    const int opp = seen == 3 ? 2 : (seen == 6 ? 0 : 1), e = (opp + 1) % 3;          // the edge opposite to f's unmatched vertex
                    const D3 w = G.v[jw]; const double hw = dot3(hn, w) - h_off, lat = dot3(w - T.v[e], ne[s][e]), slack = 1e-9 * (1.0 + len3(w - T.v[e]));
                    for (int k = 0; k < K; ++k) if (hw >= -slack && lat - hw * tan_k[k] <= slack) R[s][k] = 0.0;
                } else if (ns == 1) {
                    int iv = 0, jv = 0; for (int j = 0; j < 3; ++j) if (match[j] >= 0) { iv = match[j]; jv = j; }
                    const D3 v = T.v[iv], w1 = G.v[(jv + 1) % 3], w2 = G.v[(jv + 2) % 3];
                    const int ea = iv, eb = (iv + 2) % 3;                                            // the two edges of f at vertex iv
                    const double slack = 1e-9 * (1.0 + std::max(len3(w1 - v), len3(w2 - v)));
                    const double h1 = dot3(hn, w1 - v), h2 = dot3(hn, w2 - v);
                    for (int k = 0; k < K; ++k) {
                        // c(x) <= slack for -h, phi_ea, phi_eb along w1 + t (w2 - w1), t in [0, 1]
                        const double c1[3] = { -h1, dot3(w1 - v, ne[s][ea]) - h1 * tan_k[k], dot3(w1 - v, ne[s][eb]) - h1 * tan_k[k] };
                        const double c2[3] = { -h2, dot3(w2 - v, ne[s][ea]) - h2 * tan_k[k], dot3(w2 - v, ne[s][eb]) - h2 * tan_k[k] };
                        double t0 = 0.0, t1 = 1.0;
                        for (int c = 0; c < 3; ++c) {
                            const double u0 = c1[c] - slack, du = c2[c] - c1[c];                       // u0 + t du <= 0
                            if (du == 0.0) { if (u0 > 0.0) t1 = -1.0; }
                            else if (du > 0.0) t1 = std::min(t1, -u0 / du);
                            else t0 = std::max(t0, -u0 / du);
                        }
                        if (t0 <= t1) R[s][k] = 0.0;
                    }
                } else {
                    if (dist2 > (base[s] + G.rad) * (base[s] + G.rad)) continue;
                    const double hc = dot3(hn, G.cen) - h_off;
                    if (hc + G.rad < -tau) continue;
                    double lat[3]; for (int e = 0; e < 3; ++e) lat[e] = dot3(G.cen - T.v[e], ne[s][e]);
                    for (int k = K - 1; k >= 0; --k) {                                               // the widest cone first: a triangle outside it is outside the narrower ones
                        if (!(R[s][k] > 0.0) || hc - G.rad - h_o_max - tau >= R[s][k]) continue;
                        const double tp = tau * (1.0 + tan_k[k]);
                        bool outside = false;
                        for (int e = 0; e < 3; ++e) outside = outside || lat[e] - hc * tan_k[k] - G.rad * inv_cos_k[k] > tp;
                        if (outside) break;
                        ConePlane pl[4]; pl[0] = { hn * -1.0, tau - h_off };
                        for (int e = 0; e < 3; ++e) { const D3 n = ne[s][e] - hn * tan_k[k]; pl[1 + e] = { n, tp + dot3(T.v[e], ne[s][e]) - h_off * tan_k[k] }; }
                        double hmin;
                        if (!clip_min_height(G.v, pl, hn, hmin)) break;
                        R[s][k] = std::max(0.0, std::min(R[s][k], hmin - h_off - h_o_max - tau));
                    }
                }
            }
        }
        }
        for (int s = 0; s < 2; ++s) for (int k = 0; k < K; ++k) out[((size_t) 2 * f + s) * K + k] = half_round_down(R[s][k]);
    }
}

// ---- the per-pixel primary entry (scene_prep.h: build_primary_entry).  Float64 throughout; the margins below are for the device's float32.
// Camera.  camera_ray forms r = s2c (a, b, 0, 1) with a = spx * scale_x + offset_x + ppo_x (b alike), divides by r.w and normalises: with a bottom row
// (0, 0, *, w > 0) the direction is H (a, b, 1) up to a positive factor, H = columns 0, 1, 3 of s2c's first three rows.  So a point Y = to_world^-1 (X - eye)
// of camera space lies on the ray through raster position (q0 / q2 - offset - ppo) / scale, q = H^-1 Y, and only points with q2 > 0 lie on a ray at all.
// s = q2 grows along every ray, and on a plane 1 / s is affine in the raster position (the map is projective): its extremes over a box lie at the corners.
// The ray starts at camera-space depth near_clip and ends at far_clip (near_t, far_t): t >= 0 is Y.z >= near_clip.
// Footprint.  The lanes of pixel (px, py) sample [px, px + 1] x [py, py + 1], closed (px + jitter rounds up to px + 1 in float32); it is dilated by
// delta = 1/16 pixel, eight times what camera_ray's float32 chain (1e-3 px at x = 1920) and Moeller-Trumbore's inclusive edge tests (1e-6 of a
// triangle's extent) can move a hit across an edge.
// Candidates.  Triangles whose projection meets the dilated footprint: bounding box, then the three edge functions moved outward by the box's support
// (exact for a box and a triangle).  A triangle with a vertex nearer than near_clip (1 - 1e-3), or with q2 <= 0, is not projected: it is a candidate
// of every pixel.  A projection of zero area keeps the bounding-box test only.
// Occlusion.  T leaves the set when a candidate A covers the whole dilated footprint (its four corners inside A's projection shrunk by delta, A between
// near_clip (1 + 1e-3) and far_clip (1 - 1e-3): the float32 test cannot miss A) and max s of A over the corners < min s of T's plane over the corners
// by a relative 1e-4; never when T's plane reaches s <= 0 inside the footprint, and never on a tie (test_tri_lds breaks ties by face index).
// Entry.  The lowest node or leaf whose subtree holds every slot left; none left: LRT_PRIMARY_NONE.
namespace {
struct PeTri {
    double x[3], y[3];                                  // raster vertices
    double ex[3], ey[3], ec[3], el[3];                  // edge functions ex * px + ey * py + ec, >= 0 inside; el = |(ex, ey)|
    double gx, gy, g0;                                  // 1 / s as an affine function of the raster position
    double lox, hix, loy, hiy;
    bool projected, has_area, plane_ok, occluder;
};
void inverse3d(const double m[3][3], double o[3][3], double &det) {
    det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    const double id = 1.0 / det;
    o[0][0] = (m[1][1] * m[2][2] - m[1][2] * m[2][1]) * id; o[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * id; o[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * id;
    o[1][0] = (m[1][2] * m[2][0] - m[1][0] * m[2][2]) * id; o[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * id; o[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * id;
    o[2][0] = (m[1][0] * m[2][1] - m[1][1] * m[2][0]) * id; o[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * id; o[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * id;
}
// The BVH as a tree of ids: inner node n -> n, leaf l -> n_nodes + l
struct PeTree {
    uint32_t n_nodes = 0; std::vector<int32_t> parent; std::vector<uint16_t> depth; std::vector<uint32_t> leaf_first, face_leaf;
    bool ok = false;
    explicit PeTree(const HostBVH &b, uint32_t n_faces) {
        n_nodes = (uint32_t) (b.nodes.size() / 16); const size_t n_slots = b.tris.size() / 12;
        if (!n_nodes || b.root_is_leaf) return;
        parent.assign(n_nodes, -2); depth.assign(n_nodes, 0); face_leaf.assign(n_faces, 0xffffffffu);
        std::vector<uint32_t> todo{ 0u }; parent[0] = -1;
        while (!todo.empty()) {
            const uint32_t n = todo.back(); todo.pop_back();
            int32_t refs[4]; memcpy(refs, &b.nodes[16 * (size_t) n + 12], 16);
            for (int c = 0; c < 2; ++c) {
                if (refs[c] >= 0) {
                    if ((uint32_t) refs[c] >= n_nodes || parent[refs[c]] != -2) return;
                    parent[refs[c]] = (int32_t) n; depth[refs[c]] = (uint16_t) (depth[n] + 1); todo.push_back((uint32_t) refs[c]);
                } else {
                    const uint32_t first = (uint32_t) ~refs[c], count = (uint32_t) refs[2 + c];
                    if (!count || (size_t) first + count > n_slots) return;
                    const uint32_t id = n_nodes + (uint32_t) leaf_first.size();
                    leaf_first.push_back(first); parent.push_back((int32_t) n); depth.push_back((uint16_t) (depth[n] + 1));
                    for (uint32_t s = first; s < first + count; ++s) { uint32_t f; memcpy(&f, &b.tris[12 * (size_t) s + 3], 4); if (f >= n_faces) return; face_leaf[f] = id; }
                }
            }
        }
        ok = true;
    }
    int32_t lca(int32_t a, int32_t b) const {           // -1: the empty set
        if (a < 0) return b;
        if (b < 0) return a;
        while (a != b) { if (depth[a] >= depth[b]) a = parent[a]; else b = parent[b]; }
        return a;
    }
    uint16_t item(int32_t id) const { return id < 0 ? (uint16_t) LRT_PRIMARY_NONE : ((uint32_t) id >= n_nodes ? (uint16_t) (0x8000u | leaf_first[(uint32_t) id - n_nodes]) : (uint16_t) id); }
};
}

bool primary_entry_valid(const HostBVH &bvh, const std::vector<uint16_t> &tab) {
    const PeTree T(bvh, (uint32_t) (bvh.tris.size() / 12));           // (every face has one slot: a face index is below the slot count)
    if (!T.ok || T.n_nodes > 0x8000u) return false;
    std::vector<char> starts(0x8000u, 0);
    for (uint32_t f : T.leaf_first) { if (f >= 0x7fffu) return false; starts[f] = 1; }
    for (uint16_t it : tab) if (it != LRT_PRIMARY_NONE && !(it < 0x8000u ? it < T.n_nodes : starts[it & 0x7fffu])) return false;
    return true;
}

void build_primary_entry(const lrt_scene_desc &d, const HostBVH &bvh, std::vector<uint16_t> &out, const PrimaryEntryTune &tune) {
    out.clear();
    const uint32_t nf = d.n_faces;
    if (!nf || bvh.root_is_leaf) return;
    for (size_t i = 0; i < 3 * (size_t) d.n_vertices; ++i) if (!std::isfinite(d.positions[i])) return;
    DCamera cam; DFilm film; memset(&cam, 0, sizeof(cam)); memset(&film, 0, sizeof(film)); build_camera(d, cam, film);
    const int W = film.width, Hh = film.height;
    if (W <= 0 || Hh <= 0) return;
    const float *m = cam.s2c;
    if (m[12] != 0.f || m[13] != 0.f || !(m[15] > 0.f) || !(cam.near_clip > 0.f) || !(cam.far_clip > cam.near_clip)) return;
    if (!(film.scale_x > 0.f) || !(film.scale_y > 0.f)) return;
    const double Hm[3][3] = { { m[0], m[1], m[3] }, { m[4], m[5], m[7] }, { m[8], m[9], m[11] } };
    const double Rm[3][3] = { { cam.to_world[0], cam.to_world[1], cam.to_world[2] }, { cam.to_world[4], cam.to_world[5], cam.to_world[6] }, { cam.to_world[8], cam.to_world[9], cam.to_world[10] } };
    double Hi[3][3], Ri[3][3], dh, dr; inverse3d(Hm, Hi, dh); inverse3d(Rm, Ri, dr);
    if (!std::isfinite(1.0 / dh) || !std::isfinite(1.0 / dr)) return;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(cam.to_world[i])) return;
    const PeTree tree(bvh, nf);
    if (!tree.ok) return;
    for (uint32_t f = 0; f < nf; ++f) if (tree.face_leaf[f] == 0xffffffffu) return;
    const double eye[3] = { cam.to_world[3], cam.to_world[7], cam.to_world[11] };
    const double offx = (double) film.offset_x + (double) cam.ppo_x, offy = (double) film.offset_y + (double) cam.ppo_y, isx = 1.0 / (double) film.scale_x, isy = 1.0 / (double) film.scale_y;
    const double near_lo = (double) cam.near_clip * (1.0 - 1e-3), near_hi = (double) cam.near_clip * (1.0 + 1e-3), far_lo = (double) cam.far_clip * (1.0 - 1e-3);
    const double delta = tune.delta, half = 0.5 + delta;
    const int cox = film.crop_offset_x, coy = film.crop_offset_y;

    std::vector<PeTri> T(nf);
    int32_t everywhere = -1;                                 // the subtree of the triangles that are not projected
    for (uint32_t f = 0; f < nf; ++f) {
        PeTri &t = T[f]; t.projected = true; t.has_area = t.plane_ok = t.occluder = false;
        double w[3], zmin = INFINITY, zmax = -INFINITY;
        for (int j = 0; j < 3; ++j) {
            const float *p = &d.positions[3 * (size_t) d.faces[3 * (size_t) f + j]];
            const double Y[3] = { p[0] - eye[0], p[1] - eye[1], p[2] - eye[2] };
            double c[3], q[3];
            for (int a = 0; a < 3; ++a) c[a] = Ri[a][0] * Y[0] + Ri[a][1] * Y[1] + Ri[a][2] * Y[2];
            for (int a = 0; a < 3; ++a) q[a] = Hi[a][0] * c[0] + Hi[a][1] * c[1] + Hi[a][2] * c[2];
            if (!(c[2] >= near_lo) || !(q[2] > 0.0)) { t.projected = false; break; }
            t.x[j] = (q[0] / q[2] - offx) * isx; t.y[j] = (q[1] / q[2] - offy) * isy; w[j] = 1.0 / q[2];
            zmin = std::min(zmin, c[2]); zmax = std::max(zmax, c[2]);
            if (!std::isfinite(t.x[j]) || !std::isfinite(t.y[j]) || !std::isfinite(w[j])) { t.projected = false; break; }
        }
        if (!t.projected) { everywhere = tree.lca(everywhere, (int32_t) tree.face_leaf[f]); continue; }
        t.lox = std::min(t.x[0], std::min(t.x[1], t.x[2])); t.hix = std::max(t.x[0], std::max(t.x[1], t.x[2]));
        t.loy = std::min(t.y[0], std::min(t.y[1], t.y[2])); t.hiy = std::max(t.y[0], std::max(t.y[1], t.y[2]));
        const double area2 = (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.x[2] - t.x[0]) * (t.y[1] - t.y[0]), sg = area2 > 0.0 ? 1.0 : -1.0;
        double lmax = 0.0;
        for (int i = 0; i < 3; ++i) {
            const int j = (i + 1) % 3;
            t.ex[i] = -sg * (t.y[j] - t.y[i]); t.ey[i] = sg * (t.x[j] - t.x[i]); t.ec[i] = -(t.ex[i] * t.x[i] + t.ey[i] * t.y[i]);
            t.el[i] = std::sqrt(t.ex[i] * t.ex[i] + t.ey[i] * t.ey[i]); lmax = std::max(lmax, t.el[i]);
        }
        t.has_area = area2 != 0.0 && std::isfinite(area2);
        // the plane's 1 / s from its values at the vertices: only where the projection is no sliver (relative conditioning 1e6 at the worst)
        t.plane_ok = t.has_area && std::fabs(area2) > 1e-6 * lmax * lmax;
        if (t.plane_ok) {
            t.gx = ((w[1] - w[0]) * (t.y[2] - t.y[0]) - (w[2] - w[0]) * (t.y[1] - t.y[0])) / area2;
            t.gy = ((t.x[1] - t.x[0]) * (w[2] - w[0]) - (t.x[2] - t.x[0]) * (w[1] - w[0])) / area2;
            t.g0 = w[0] - t.gx * t.x[0] - t.gy * t.y[0];
            t.plane_ok = std::isfinite(t.gx) && std::isfinite(t.gy) && std::isfinite(t.g0);
        }
        t.occluder = t.plane_ok && zmin >= near_hi && zmax <= far_lo;
    }
    // the candidates of every pixel: count, then fill
    const size_t npix = (size_t) W * (size_t) Hh;
    auto for_pixels = [&](uint32_t f, auto &&fn) {
        const PeTri &t = T[f];
        const double x0 = std::ceil(t.lox - 1.0 - delta) - cox, x1 = std::floor(t.hix + delta) - cox, y0 = std::ceil(t.loy - 1.0 - delta) - coy, y1 = std::floor(t.hiy + delta) - coy;
        if (!(x1 >= 0.0) || !(y1 >= 0.0) || !(x0 <= W - 1.0) || !(y0 <= Hh - 1.0)) return;
        const int ix0 = (int) std::max(x0, 0.0), ix1 = (int) std::min(x1, W - 1.0), iy0 = (int) std::max(y0, 0.0), iy1 = (int) std::min(y1, Hh - 1.0);
        double sup[3]; for (int i = 0; i < 3; ++i) sup[i] = half * (std::fabs(t.ex[i]) + std::fabs(t.ey[i]));
        for (int y = iy0; y <= iy1; ++y) {
            const double cy = (double) (y + coy) + 0.5;
            for (int x = ix0; x <= ix1; ++x) {
                const double cx = (double) (x + cox) + 0.5;
                bool in = true;
                if (t.has_area) for (int i = 0; i < 3; ++i) in = in && t.ex[i] * cx + t.ey[i] * cy + t.ec[i] + sup[i] >= 0.0;
                if (in) fn((size_t) y * W + x);
            }
        }
    };
    std::vector<uint32_t> start(npix + 1, 0);
    for (uint32_t f = 0; f < nf; ++f) if (T[f].projected) for_pixels(f, [&](size_t p) { ++start[p + 1]; });
    for (size_t p = 0; p < npix; ++p) start[p + 1] += start[p];
    std::vector<uint16_t> cand(start[npix]); std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (uint32_t f = 0; f < nf; ++f) if (T[f].projected) for_pixels(f, [&](size_t p) { cand[fill[p]++] = (uint16_t) f; });   // (lds_image_fits: faces < 32768; the caller builds the table for LDS images only)
    // occlusion and entry
    out.assign(npix, 0);
    for (int y = 0; y < Hh; ++y) for (int x = 0; x < W; ++x) {
        const size_t p = (size_t) y * W + x; const uint32_t b = start[p], e = start[p + 1];
        int32_t id = everywhere;
        if (e - b == 1) id = tree.lca(id, (int32_t) tree.face_leaf[cand[b]]);
        else if (e > b) {
            const double cx = (double) (x + cox) + 0.5, cy = (double) (y + coy) + 0.5;
            double cover = INFINITY;                         // the least, over the covering candidates, of max s over the footprint
            for (uint32_t k = b; k < e; ++k) {
                const PeTri &A = T[cand[k]];
                if (!A.occluder) continue;
                bool in = true;
                for (int i = 0; i < 3; ++i) in = in && A.ex[i] * cx + A.ey[i] * cy + A.ec[i] - half * (std::fabs(A.ex[i]) + std::fabs(A.ey[i])) >= delta * A.el[i];
                if (!in) continue;
                const double gmin = A.gx * cx + A.gy * cy + A.g0 - half * (std::fabs(A.gx) + std::fabs(A.gy));
                if (gmin > 0.0) cover = std::min(cover, 1.0 / gmin);
            }
            for (uint32_t k = b; k < e; ++k) {
                const PeTri &t = T[cand[k]];
                if (cover < INFINITY && t.plane_ok) {
                    const double gc = t.gx * cx + t.gy * cy + t.g0, gs = half * (std::fabs(t.gx) + std::fabs(t.gy));
                    if (gc - gs > 0.0 && 1.0 / (gc + gs) > cover * (1.0 + tune.depth_margin)) continue;      // behind the cover everywhere in the footprint
                }
                id = tree.lca(id, (int32_t) tree.face_leaf[cand[k]]);
            }
        }
        out[p] = tree.item(id);
    }
}

// include/mitsuba/render/fresnel.h:327-355, in float32 with the fused multiply-adds the reference's dr::fmadd / dr::horner are
static float fresnel_diffuse_reflectance(float eta) {
    const float inv_eta = 1.f / eta;
    const float approx_1 = fmaf(0.0636f, inv_eta, fmaf(eta, fmaf(eta, -1.4399f, 0.7099f), 0.6681f));
    float approx_2 = -1.36881f;
    for (float c : { 4.98554f, -7.80989f, 6.75335f, -3.4793f, 0.919317f }) approx_2 = fmaf(approx_2, inv_eta, c);
    return eta < 1.f ? approx_1 : approx_2;
}
PlasticConstants plastic_constants(float eta, float d_mean, float s_mean) {      // plastic.cpp:192-207
    PlasticConstants c;
    c.inv_eta_2 = 1.f / (eta * eta);
    c.fdr_int = fresnel_diffuse_reflectance(1.f / eta);
    c.fdr_ext = fresnel_diffuse_reflectance(eta);
    c.specular_sampling_weight = s_mean / (d_mean + s_mean);
    return c;
}
float texture_mean(const lrt_texture_desc &T) {
    auto mean3 = [](const float *c) { return (c[0] + c[1] + c[2]) * (1.f / 3.f); };       // src/spectra/srgb.cpp:117-122 (dr::mean of the colour: the sum times 1 / 3, as mean3 of dmath.h)
    if (T.type == LRT_TEX_CHECKERBOARD) return .5f * (mean3(T.color0) + mean3(T.color1));   // checkerboard.cpp:112-114
    return mean3(T.color0);
}
void prepare_geometry(const lrt_scene_desc &d, const PrepOptions &opt, PreparedScene &P) {
    DScene &sc = P.sc;
    memset(&sc, 0, sizeof(sc));                          // the record is uploaded byte for byte: its padding is cleared too
    // ---- sphere shapes (src/shapes/sphere.cpp:146-165): centre, radius and the inverse transform, outside the triangle BVH
    std::vector<DSphere> &spheres = P.spheres;
    for (uint32_t i = 0; i < d.n_shapes; ++i) {
        const lrt_shape_desc &s = d.shapes[i];
        if (s.kind != LRT_SHAPE_SPHERE) continue;
        DSphere o; memset(&o, 0, sizeof(o));
        const float *m = s.to_world;
        for (int a = 0; a < 3; ++a) o.center[a] = m[4 * a + 3];                       // to_world * (0, 0, 0)
        o.radius = sqrtf(fmaf(m[8], m[8], fmaf(m[4], m[4], m[0] * m[0])));           // |to_world * (1, 0, 0)|
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) o.to_world[3 * a + b] = m[4 * a + b];
        double md[16]; for (int k = 0; k < 16; ++k) md[k] = m[k];
        const double c00 = md[5] * md[10] - md[6] * md[9], c01 = md[6] * md[8] - md[4] * md[10], c02 = md[4] * md[9] - md[5] * md[8];
        const double id = 1.0 / (md[0] * c00 + md[1] * c01 + md[2] * c02);
        double inv[12] = { c00 * id, (md[2] * md[9] - md[1] * md[10]) * id, (md[1] * md[6] - md[2] * md[5]) * id, 0,
                           c01 * id, (md[0] * md[10] - md[2] * md[8]) * id, (md[2] * md[4] - md[0] * md[6]) * id, 0,
                           c02 * id, (md[1] * md[8] - md[0] * md[9]) * id, (md[0] * md[5] - md[1] * md[4]) * id, 0 };
        for (int a = 0; a < 3; ++a) inv[4 * a + 3] = -(inv[4 * a] * md[3] + inv[4 * a + 1] * md[7] + inv[4 * a + 2] * md[11]);
        for (int k = 0; k < 12; ++k) o.to_object[k] = (float) inv[k];
        o.shape = i; o.flip_normals = s.flip_normals;
        check_sphere_radius(o.radius);
        spheres.push_back(o);
    }
    sc.n_spheres = (uint32_t) spheres.size();
    const SceneFeatures features = scene_features(d);      // any of them: the EXT kernel instances (scene_check.h)
    P.ext = features.any(); P.smooth_bsdf = features.smooth_bsdf;
    // ---- acceleration structure
    // Leaf size: the smallest of 2, 3, 4, 6, 8, 12, 16 triangles whose BVH image fits the LDS next to the traversal stacks (fatter
    // leaves = fewer nodes: more triangle tests per leaf, but every fetch of the traversal stays in LDS; Liver-MultiMesh's two meshes
    // run 44 % faster with 8-triangle leaves in LDS than with 4-triangle leaves in global memory); 4 when nothing fits.
    // LRT_BVH_LEAF=n forces a size.
    HostBVH &bvh = P.bvh;
    {
        const int forced = opt.bvh_leaf;
        int chosen = forced ? forced : 4;
        bool done = false;
        if (!forced && lds_possible(d, opt)) {                     // the thinnest leaves whose image still fits (measured: 3 beats 4 by 1 % on the liver; 2 does not fit there)
            for (int leaf : { 2, 3, 4, 6, 8, 12, 16 }) {
                HostBVH b2; build_bvh(d.positions, d.faces, d.n_faces, b2, leaf);
                if (lds_image_fits(d, b2, opt)) { bvh = std::move(b2); chosen = leaf; done = true; break; }
            }
        }
        if (!done) build_bvh(d.positions, d.faces, d.n_faces, bvh, chosen);
        P.bvh_leaf = chosen;
    }
    sc.root_is_leaf = bvh.root_is_leaf; sc.root_leaf_first = bvh.root_first; sc.root_leaf_count = bvh.root_count;
    sc.n_faces = d.n_faces; sc.n_emitters = d.n_emitters; sc.one_shape = d.n_shapes == 1;
    // ---- LDS image of the acceleration structure (persistent kernel): used when it fits next to the traversal stacks
    if (lds_image_fits(d, bvh, opt)) { build_lds_image(d, bvh, P); P.use_lds = true; }
    // ---- conservative distance field (scenes with participating media: short free-flight segments deep inside a
    // volume are proven surface-free with one lookup instead of a BVH traversal)
    sc.grid = DDistGrid{};
    // Spheres are surfaces too: their exact distance | |p - c| - r | joins the field's minimum and their bounds the grid's
    // (k_build_dist_grid), or every medium trip inside a sphere would prove its way through the sphere's surface.
    if (d.n_media > 0 && (d.n_faces > 0 || !spheres.empty()) && d.n_faces <= (1u << 17) && !opt.no_dist_grid) {
        float lo[3], hi[3]; referenced_bounds(d, spheres, lo, hi);
        const float ext = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
        const int res = opt.dist_grid_res ? opt.dist_grid_res : (d.n_faces <= (1u << 14) ? 192 : 64);
        if (ext > 0.f && std::isfinite(ext)) {
            DDistGrid g{};
            g.cell = ext / (float) res; g.inv_cell = 1.f / g.cell;
            for (int a = 0; a < 3; ++a) { g.lo[a] = lo[a]; g.n[a] = std::max(1, std::min(res, (int) std::ceil((hi[a] - lo[a]) / g.cell))); }
            float diag = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
            float amax = 0.f; for (int a = 0; a < 3; ++a) amax = std::max(amax, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
            P.grid_abs_margin = 1e-4f * diag + 1e-5f * amax;          // >> f32 rounding of positions and of the field itself
            g.enabled = 1; sc.grid = g;                                    // (g.d: the upload side builds the field, k_build_dist_grid)
        }
    }
    // ---- per-face cone table: proves the segments that start on a surface, which the distance field cannot (build_cone_table).  Only the
    // closed-records volpath kernels read it, and those run on the LDS image, without spheres, beside the distance field, on scenes that
    // closed_records() accepts: the build is quadratic in the faces and is not paid for a scene whose renders can never use it.  (A parameter update
    // that makes a scene qualify later renders it with 64-byte records and no table, as with LRT_NO_CONE_PROOF.)
    const bool closed_lds = P.use_lds && !P.ext && sc.grid.enabled && closed_records(d, d.sensor.medium);
    if (closed_lds && !opt.no_cone_proof) { build_cone_table(d, P.cone_tab); sc.cone_enabled = 1; }
    // ---- per-pixel primary entry: where a camera ray's traversal may start (build_primary_entry).  Read by the same kernels, built under the same
    // condition; it depends on the geometry, the sensor, the film size and the crop window, none of which a parameter update changes.
    if (closed_lds && !bvh.root_is_leaf && !opt.no_primary_entry) {
        build_primary_entry(d, bvh, P.primary_tab);
        if (!P.primary_tab.empty()) {
            if (!primary_entry_valid(bvh, P.primary_tab)) throw std::runtime_error("primary entry table: an item names no node or leaf of the BVH");
            sc.primary_enabled = 1;
        }
    }
}

void prepare_shading(const lrt_scene_desc &d, const PrepOptions &opt, PreparedScene &P) {
    DScene &sc = P.sc; const std::vector<DSphere> &spheres = P.spheres;
    // ---- geometry attributes
    {
        P.vattr.assign(8 * (size_t) d.n_vertices, 0.f); std::vector<float> &va = P.vattr;
        for (size_t v = 0; v < d.n_vertices; ++v) {
            if (d.normals) for (int a = 0; a < 3; ++a) va[8 * v + a] = d.normals[3 * v + a];
            if (d.texcoords) for (int a = 0; a < 2; ++a) va[8 * v + 4 + a] = d.texcoords[2 * v + a];
        }
    }
    std::vector<DShape> &shapes = P.shapes; shapes.resize(d.n_shapes);
    for (uint32_t i = 0; i < d.n_shapes; ++i) { const lrt_shape_desc &s = d.shapes[i]; shapes[i] = { s.bsdf, s.emitter, s.interior_medium, s.exterior_medium, s.has_normals, s.has_texcoords, s.flip_normals, s.kind }; }
    // ---- textures (bitmaps: one luminance float per texel, src/textures/bitmap.cpp:540-552)
    std::vector<DTexture> &tex = P.textures; tex.resize(d.n_textures); std::vector<float> &tex_data = P.tex_data;
    for (uint32_t i = 0; i < d.n_textures; ++i) {
        const lrt_texture_desc &T = d.textures[i]; DTexture &o = tex[i]; memset(&o, 0, sizeof(o));
        o.type = T.type; o.width = T.width; o.height = T.height; o.channels = T.channels;
        for (int k = 0; k < 3; ++k) { o.color0[k] = T.color0[k]; o.color1[k] = T.color1[k]; }
        for (int k = 0; k < 6; ++k) o.to_uv[k] = T.to_uv[k];
        if (T.type == LRT_TEX_BITMAP) {
            o.data_offset = (uint32_t) tex_data.size();
            size_t np = (size_t) T.width * T.height;
            for (size_t p = 0; p < np; ++p) {
                const float *px = T.data + p * T.channels;
                tex_data.push_back(T.channels == 1 ? px[0] : px[0] * 0.212671f + px[1] * 0.715160f + px[2] * 0.072169f);
            }
        }
    }
    // ---- BSDFs
    std::vector<DBsdf> &bsdfs = P.bsdfs; bsdfs.resize(d.n_bsdfs); sc.has_null_bsdf = 0;
    // (roughdielectric: both lobes are glossy; plastic: a delta coat over a diffuse base, plastic.cpp:177-179; twosided: its children's, twosided.cpp:90-100)
    std::function<int(uint32_t)> leaf_flags = [&](uint32_t b) -> int {
        const lrt_bsdf_desc &B = d.bsdfs[b];
        if (B.type == LRT_BSDF_TWOSIDED) { const int32_t back = B.nested_back < 0 ? B.nested : B.nested_back; return leaf_flags((uint32_t) B.nested) | leaf_flags((uint32_t) back); }   // (validated below: the children are leaves)
        return (B.type == LRT_BSDF_DIFFUSE || B.type == LRT_BSDF_ROUGHDIELECTRIC) ? PREP_F_SMOOTH : (B.type == LRT_BSDF_DIELECTRIC || B.type == LRT_BSDF_CONDUCTOR) ? PREP_F_DELTA
             : B.type == LRT_BSDF_PLASTIC ? (PREP_F_DELTA | PREP_F_SMOOTH) : PREP_F_NULL;
    };
    bool any_smooth_bsdf = false;
    for (uint32_t i = 0; i < d.n_bsdfs; ++i) if (d.bsdfs[i].type == LRT_BSDF_CONDUCTOR || d.bsdfs[i].type == LRT_BSDF_PLASTIC || d.bsdfs[i].type == LRT_BSDF_TWOSIDED) { check_smooth_bsdf(d, i); any_smooth_bsdf = true; }
    if (any_smooth_bsdf) P.bsdf_ext.assign(d.n_bsdfs, DBsdfExt{});
    for (uint32_t i = 0; i < d.n_bsdfs; ++i) {
        const lrt_bsdf_desc &B = d.bsdfs[i];
        DBsdf &o = bsdfs[i]; memset(&o, 0, sizeof(o));
        o.type = B.type; o.reflectance = B.reflectance; o.nested = B.nested; o.texture = B.texture; o.eta = B.eta; o.scale = B.scale;
        bsdfs[i].flags = leaf_flags(B.type == LRT_BSDF_BUMPMAP ? (uint32_t) B.nested : i);      // (indices and nesting: check_bsdf, or the loader, has seen them)
        if (B.type == LRT_BSDF_NULL) sc.has_null_bsdf = 1;
        if (B.type == LRT_BSDF_ROUGHDIELECTRIC) {     // the fields share the words a roughdielectric leaves unused (device_types.h)
            bsdfs[i].specular_reflectance = B.specular_reflectance; bsdfs[i].specular_transmittance = B.specular_transmittance;
            bsdfs[i].alpha_u = std::max(B.alpha_u, 1e-4f); bsdfs[i].alpha_v = std::max(B.alpha_v, 1e-4f);      // MicrofacetDistribution::configure (microfacet.h:425-428)
            bsdfs[i].micro = (B.distribution == 1 ? LRT_MICRO_GGX : 0) | (B.sample_visible ? LRT_MICRO_VISIBLE : 0);
        }
        // conductor / plastic / twosided: what DBsdf has no room for lives in the row of the same index (device_types.h)
        if (B.type == LRT_BSDF_CONDUCTOR) {
            DBsdfExt &x = P.bsdf_ext[i];
            o.specular_reflectance = B.specular_reflectance;
            for (int k = 0; k < 3; ++k) { x.eta[k] = B.eta_rgb[k]; x.k[k] = B.k_rgb[k]; }
        }
        if (B.type == LRT_BSDF_PLASTIC) {
            DBsdfExt &x = P.bsdf_ext[i];
            o.reflectance = B.diffuse_reflectance;
            const PlasticConstants c = plastic_constants(B.eta, texture_mean(d.textures[B.diffuse_reflectance]), B.specular_reflectance >= 0 ? texture_mean(d.textures[B.specular_reflectance]) : 1.f);
            x.inv_eta_2 = c.inv_eta_2; x.fdr_int = c.fdr_int; x.fdr_ext = c.fdr_ext; x.spec_weight = c.specular_sampling_weight;
            x.nonlinear = B.nonlinear ? 1 : 0; x.specular_reflectance = B.specular_reflectance;
        }
        if (B.type == LRT_BSDF_TWOSIDED) P.bsdf_ext[i].back = B.nested_back < 0 ? B.nested : B.nested_back;
    }
    // ---- bounds (src/render/scene.cpp:49; include/mitsuba/core/bbox.h:343-346; envmap.cpp:337-351)
    DEnv &E = sc.env; memset(&E, 0, sizeof(E)); E.type = -1; E.emitter = -1;
    {
        float lo[3], hi[3]; vertex_bounds(d, spheres, lo, hi);
        const float ray_eps = 5.9604644775390625e-8f * 1500.f;
        if (d.n_vertices || !spheres.empty()) {
            float c[3], dd[3]; for (int a = 0; a < 3; ++a) { c[a] = (hi[a] + lo[a]) * 0.5f; dd[a] = c[a] - hi[a]; E.bsphere_c[a] = c[a]; }
            float r = sqrtf(fmaf(dd[2], dd[2], fmaf(dd[1], dd[1], dd[0] * dd[0])));
            E.bsphere_r = fmaxf(ray_eps, r * (1.f + ray_eps));
        } else { E.bsphere_c[0] = E.bsphere_c[1] = E.bsphere_c[2] = 0.f; E.bsphere_r = ray_eps; }
    }
    // ---- media: what the scene as a whole needs to know about them (the tables themselves: prepare_media)
    check_media_count(d);
    prepare_phases(d, P.phases, P.phase_pool);
    for (uint32_t i = 0; i < d.n_media; ++i) {
        const lrt_medium_desc &M = d.media[i];
        if (M.type == LRT_MEDIUM_HOMOGENEOUS || M.type == LRT_MEDIUM_HETEROGENEOUS) P.has_non_bio = true;
        if (M.type != LRT_MEDIUM_HETEROGENEOUS) continue;
        check_medium_grid(M);                                   // stricter than check_medium: grid_max > 0
        P.has_het = true;
    }
    for (uint32_t i = 0; i < d.n_shapes; ++i) for (int m : { d.shapes[i].interior_medium, d.shapes[i].exterior_medium })
        if (m >= 0 && d.media[m].type == LRT_MEDIUM_HETEROGENEOUS) P.prb_null = true;
    // ---- emitters
    std::vector<DEmitter> &em = P.emitters; em.resize(d.n_emitters); std::vector<float> &env_rgbx = P.env_data, &hier = P.env_hier; bool &env_interior_positive = P.env_interior_positive;
    std::vector<DMeshEmitter> &mesh_em = P.mesh_emitters; mesh_em.resize(d.n_emitters); std::vector<float> &mesh_tab = P.mesh_emitter_tab;      // (all zero: no mesh emitter)
    for (uint32_t i = 0; i < d.n_emitters; ++i) {
        const lrt_emitter_desc &S = d.emitters[i]; DEmitter &o = em[i]; memset(&o, 0, sizeof(o));
        o.type = S.type; o.shape = S.shape; o.scale = S.scale; for (int k = 0; k < 3; ++k) o.radiance[k] = S.radiance[k];
        if (S.type == LRT_EMITTER_AREA) {
            P.has_area_emitter = true;
            const lrt_shape_desc &sd = d.shapes[S.shape];      // (a rectangle or a mesh: check_emitter, or the loader, has refused a sphere)
            if (sd.kind == LRT_SHAPE_MESH) {                   // src/render/mesh.cpp:449-482: the area table and its CDF (host_scene.h)
                MeshEmitterTable T; mesh_emitter_table(d.positions, d.faces, sd.first_face, sd.n_faces, "shapes[" + std::to_string(S.shape) + "]", T);
                DMeshEmitter &M = mesh_em[i];
                M.first_face = sd.first_face; M.n_faces = sd.n_faces; M.sum = T.sum; M.normalization = T.normalization;
                M.has_normals = sd.has_normals; M.flip_normals = sd.flip_normals; M.mesh = 1;
                M.pmf_offset = (uint32_t) mesh_tab.size(); mesh_tab.insert(mesh_tab.end(), T.pmf.begin(), T.pmf.end());
                M.cdf_offset = (uint32_t) mesh_tab.size(); mesh_tab.insert(mesh_tab.end(), T.cdf.begin(), T.cdf.end());
                continue;
            }
            memcpy(o.to_world, sd.to_world, sizeof(float) * 12);
            auto xv = [&](float x, float y, float z, float *r) { const float *m = sd.to_world; for (int a = 0; a < 3; ++a) r[a] = fmaf(m[4 * a + 2], z, fmaf(m[4 * a + 1], y, m[4 * a] * x)); };
            float du[3], dv[3]; xv(2.f, 0.f, 0.f, du); xv(0.f, 2.f, 0.f, dv);
            float cx = fmaf(du[1], dv[2], -(du[2] * dv[1])), cy = fmaf(du[2], dv[0], -(du[0] * dv[2])), cz = fmaf(du[0], dv[1], -(du[1] * dv[0]));
            o.inv_area = 1.f / sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
            uint32_t v0 = d.faces[3 * sd.first_face];
            for (int a = 0; a < 3; ++a) o.n[a] = sd.flip_normals ? -d.normals[3 * v0 + a] : d.normals[3 * v0 + a];
        } else if (S.type == LRT_EMITTER_POINT) {             // src/emitters/point.cpp: position and intensity (radiance[])
            memcpy(o.to_world, S.to_world, sizeof(float) * 12);
        } else if (S.type == LRT_EMITTER_SPOT || S.type == LRT_EMITTER_DIRECTIONAL) {
            if (P.delta_emitters.empty()) P.delta_emitters.assign(d.n_emitters, DDeltaEmitter{});
            check_delta_emitter(d, i);
            DDeltaEmitter &D = P.delta_emitters[i]; D.texture = -1;
            memcpy(o.to_world, S.to_world, sizeof(float) * 12);
            if (S.type == LRT_EMITTER_SPOT) {                   // src/emitters/spot.cpp:104-112, in float32 as the plugin's ScalarFloat members
                const float deg = 3.14159265358979323846f / 180.f;       // dr::deg_to_rad: value * (Pi / 180)
                const float cutoff = S.cutoff_angle * deg, beam = S.beam_width * deg;
                D.cutoff = cutoff; D.inv_transition = 1.0f / (cutoff - beam);
                D.cos_cutoff = cosf(cutoff); D.cos_beam = cosf(beam); D.uv_factor = tanf(cutoff);
                for (int a = 0; a < 3; ++a) D.pos[a] = S.to_world[4 * a + 3];
                inverse3(S.to_world, D.to_local);
                D.texture = S.texture;
            } else {                                            // src/emitters/directional.cpp:98-108,153: to_world * (0, 0, 1) and set_scene's sphere
                for (int a = 0; a < 3; ++a) { D.dir[a] = S.to_world[4 * a + 2]; D.bsphere_c[a] = E.bsphere_c[a]; }
                D.bsphere_r = E.bsphere_r;
            }
        } else {
            E.type = S.type; E.emitter = (int) i; E.scale = S.scale; for (int k = 0; k < 3; ++k) E.radiance[k] = S.radiance[k];
            if (S.type == LRT_EMITTER_ENVMAP) {             // src/emitters/envmap.cpp:139-236
                uint32_t w = (uint32_t) S.width, h = (uint32_t) S.height; E.w = w + 1; E.h = h;
                env_rgbx.assign((size_t) E.w * h * 4, 0.f); std::vector<float> lum((size_t) E.w * h);
                float theta_scale = 1.f / (float) (h - 1) * 3.14159265358979323846f;
                const float *in = S.data;
                for (uint32_t y = 0; y < h; ++y) {
                    float sin_theta = (float) sin((double) ((float) y * theta_scale));
                    for (uint32_t x = 0; x < w; ++x) {
                        float l = fmaxf((in[0] * 0.212671f + in[1] * 0.715160f + in[2] * 0.072169f) - 0.f, 0.f);
                        lum[(size_t) y * E.w + x] = l * sin_theta;
                        float *o4 = &env_rgbx[((size_t) y * E.w + x) * 4]; o4[0] = in[0]; o4[1] = in[1]; o4[2] = in[2];
                        in += 3;
                    }
                    lum[(size_t) y * E.w + w] = lum[(size_t) y * E.w];
                    for (int k = 0; k < 3; ++k) env_rgbx[((size_t) y * E.w + w) * 4 + k] = env_rgbx[((size_t) y * E.w) * 4 + k];
                }
                build_hierarchy(lum, E.w, h, E, hier);
                env_interior_positive = true;          // rows 1..h-2 of the sampling density strictly positive?
                for (uint32_t y = 1; y + 1 < h && env_interior_positive; ++y)
                    for (uint32_t x = 0; x < E.w; ++x) if (!(lum[(size_t) y * E.w + x] > 0.f)) { env_interior_positive = false; break; }
                for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) E.to_world[3 * a + b] = S.to_world[4 * a + b];
                inverse3(S.to_world, E.to_local);
            }
        }
    }
    sc.nee_fast_reject = (d.n_emitters == 1 && !sc.has_null_bsdf && !P.has_het && !opt.no_nee_reject &&
                          (E.type == LRT_EMITTER_CONSTANT || (E.type == LRT_EMITTER_ENVMAP && env_interior_positive))) ? 1 : 0;
    build_camera(d, sc.cam, sc.film);
}

PreparedScene prepare_scene(const lrt_scene_desc &d, const PrepOptions &opt) {
    PreparedScene P; prepare_geometry(d, opt, P); prepare_shading(d, opt, P);
    return P;
}

void prepare_media(const lrt_scene_desc &d, float bsphere_r, std::vector<DMedium> &media, std::vector<DBioMedium> &bio, std::vector<DHetMedium> &het) {
    bio.assign(std::max<uint32_t>(d.n_media, 1), DBioMedium{});
    for (uint32_t i = 0; i < d.n_media; ++i) {
        const lrt_medium_desc &M = d.media[i]; DBioMedium &o = bio[i];
        o.type = M.type; o.has_spectral_extinction = M.has_spectral_extinction;
        for (int l = 0; l < 4; ++l) { o.layer_limit[l] = M.layer_limit[l]; for (int k = 0; k < 3; ++k) { o.collagen[l][k] = M.sigma_collagen[l][k]; o.elastin[l][k] = M.sigma_elastin[l][k]; } }
        for (int k = 0; k < 3; ++k) { o.blood[k] = M.sigma_blood[k]; o.bile[k] = M.sigma_bile[k]; o.lipid_water[k] = M.sigma_lipid_water[k]; }
        o.hepatocity = M.sigma_hepatocity; o.log10_hep = 0.f;
        if (M.type == LRT_MEDIUM_PARENCHYMA) { o.sigmat[0] = 77.2f / 255; o.sigmat[1] = 105.0f / 255; o.sigmat[2] = 149.0f / 255; }   // parenchyma.cpp:165
        else for (int k = 0; k < 3; ++k) o.sigmat[k] = medium_sigma_t(M, k);                                                       // liver.cpp:204-209
    }
    media.resize(std::max<uint32_t>(d.n_media, 1));
    for (uint32_t i = 0; i < d.n_media; ++i) {
        const lrt_medium_desc &M = d.media[i]; DMedium &o = media[i];
        for (int k = 0; k < 3; ++k) { o.sigma_t[k] = medium_sigma_t(M, k); o.albedo[k] = M.albedo[k]; }   // homogeneous.cpp:121-126 eval_sigmat
        o.has_spectral_extinction = M.has_spectral_extinction; o.sample_emitters = M.sample_emitters; o.phase = M.phase; o.g = M.g;
        o.scale = M.scale; o.het = M.type == LRT_MEDIUM_HETEROGENEOUS ? 1 : 0;
        o.phase_ext = medium_has_phase_entry(d, i) ? M.phase_index + 1 : 0;
        // Early NEE rejection (volpath_iteration): an infinite emitter's sample lies at distance >= 2 r (r: the scene's bounding sphere); the
        // kernel rejects when -log(1 - u) / sigma_t <= bound(dist), bound(x) = x * 0.998f - 1e-3f (monotone in x).  1 - u >= vmin implies that
        // for dist = 2 r, hence for every sample: vmin = exp(-sigma_t bound(2 r) (1 - 1e-4)) (1 + 1e-4), far outside the 3e-7 relative error
        // of the kernels' logarithm and the rounding of the division; 2 (never true) when sigma_t bound is too small for the margin to mean anything.
        const float bound = (2.f * bsphere_r) * 0.998f - 1e-3f;
        for (int k = 0; k < 3; ++k) {
            const double x = (double) o.sigma_t[k] * (double) bound;
            double v = (x > 0.05 && std::isfinite(x)) ? std::exp(-x * (1.0 - 1e-4)) * (1.0 + 1e-4) : 2.0;
            float vf = (float) v; if ((double) vf < v) vf = std::nextafter(vf, 3.f);
            o.nee_vmin[k] = vf;
        }
    }
    het.assign(std::max<uint32_t>(d.n_media, 1), DHetMedium{});
    for (uint32_t i = 0; i < d.n_media; ++i) {
        const lrt_medium_desc &M = d.media[i]; DHetMedium &o = het[i];
        if (M.type != LRT_MEDIUM_HETEROGENEOUS) continue;
        for (int k = 0; k < 3; ++k) { o.res[k] = M.grid_res[k]; o.bbox_min[k] = M.grid_bbox_min[k]; o.bbox_max[k] = M.grid_bbox_max[k]; }
        for (int k = 0; k < 12; ++k) o.to_local[k] = M.grid_to_local[k];
        o.scale = M.scale; o.max_density = M.scale * M.grid_max;                    // heterogeneous.cpp:164,171
    }
}

void phase_table(const float *values, size_t size, PhaseTable &out) {
    if (size < 2) throw std::runtime_error("ContinuousDistribution: needs at least two entries!");
    out.cdf.assign(size - 1, 0.f);
    uint32_t vx = (uint32_t) -1, vy = (uint32_t) -1;
    const double range = double(1.f) - double(-1.f), interval_size = range / (double) (size - 1);
    double integral = 0.;
    for (size_t i = 0; i < size - 1; ++i) {
        const double y0 = (double) values[i], y1 = (double) values[i + 1];
        const double value = 0.5 * interval_size * (y0 + y1);
        integral += value;
        out.cdf[i] = (float) integral;
        if (y0 < 0. || y1 < 0.) throw std::runtime_error("ContinuousDistribution: entries must be non-negative!");
        else if (value > 0.) { if (vx == (uint32_t) -1) vx = (uint32_t) i; vy = (uint32_t) i; }
    }
    if (vx == (uint32_t) -1 || vy == (uint32_t) -1) throw std::runtime_error(text::no_probability_mass);
    out.valid_x = vx; out.valid_y = vy;
    out.integral = out.cdf[vy]; out.normalization = 1.f / out.integral;
    out.interval_size = (float) interval_size; out.inv_interval_size = 1.f / out.interval_size;
}

void prepare_phases(const lrt_scene_desc &d, std::vector<DPhase> &phases, std::vector<float> &pool) {
    phases.clear(); pool.clear();
    if (!d.n_phases) return;
    check_phase_table(d);
    phases.resize(d.n_phases);
    for (uint32_t i = 0; i < d.n_phases; ++i) {
        const lrt_phase_desc &Q = d.phases[i]; DPhase &o = phases[i]; memset(&o, 0, sizeof(o));
        o.type = Q.type; o.g = Q.g; o.child0 = o.child1 = 0;
        if (Q.type == LRT_PHASE_BLEND) { o.weight = std::min(std::max(Q.weight, 0.f), 1.f); o.child0 = Q.child[0]; o.child1 = Q.child[1]; }   // blendphase.cpp:156-159 eval_weight
        if (Q.type != LRT_PHASE_TABULATED) continue;
        PhaseTable T; phase_table(Q.values, Q.n_values, T);
        o.n = Q.n_values; o.interval_size = T.interval_size; o.inv_interval_size = T.inv_interval_size; o.integral = T.integral; o.normalization = T.normalization;
        o.valid_x = T.valid_x; o.valid_y = T.valid_y;
        o.rec_off = (uint32_t) pool.size();                    // (a multiple of 4 floats: every entry pads its cdf below)
        for (uint32_t k = 0; k + 1 < Q.n_values; ++k) { pool.push_back(Q.values[k]); pool.push_back(Q.values[k + 1]); pool.push_back(k ? T.cdf[k - 1] : 0.f); pool.push_back(T.cdf[k]); }
        o.cdf_off = (uint32_t) pool.size();
        pool.insert(pool.end(), T.cdf.begin(), T.cdf.end());
        while (pool.size() % 4) pool.push_back(0.f);
    }
}

ResolvedOpts resolve(const lrt_scene_desc &d, const lrt_render_opts *o) {
    ResolvedOpts r;
    if (o && o->integrator > LRT_INTEGRATOR_VOLPATHMIS) throw std::invalid_argument("lrt_render_opts.integrator " + std::to_string(o->integrator) + " is not an integrator (LRT_INTEGRATOR_PATH .. LRT_INTEGRATOR_VOLPATHMIS, or -1 for the scene's own)");
    r.integrator = (o && o->integrator >= 0) ? o->integrator : d.integrator.type;
    r.max_depth = (o && o->max_depth != -2) ? o->max_depth : d.integrator.max_depth;
    // A path's depth lives in 16 bits of its record, and -1 ("unbounded") has no end at all when Russian roulette cannot stop a path (the ld sampler's 1-D
    // sample takes `sample_count` values per pixel: for a fifth of the pixels none of them reaches 0.95; found by a fuzz scene whose path had left a leaky
    // mesh with its medium flag set).  -1 and anything above mean 65535 here and in the oracle; the reference would go on.
    if (r.max_depth < 0 || r.max_depth > 65535) r.max_depth = 65535;
    r.rr_depth = (o && o->rr_depth >= 0) ? o->rr_depth : d.integrator.rr_depth;
    r.hide_emitters = (o && o->hide_emitters >= 0) ? (o->hide_emitters != 0) : (d.integrator.hide_emitters != 0);
    r.spp = (o && o->spp) ? o->spp : d.sample_count;
    if (d.sampler_type == LRT_SAMPLER_LD) {            // integrator.cpp:169-171 + ldsampler.cpp:83-93: a square power of two
        uint32_t res = 2;
        while (res * res < r.spp) { ++res; uint32_t p2 = 1; while (p2 < res) p2 <<= 1; res = p2; }
        r.spp = res * res;
    }
    r.seed = o ? o->seed : 0;
    r.tile_rank = o ? o->tile_rank : 0; r.tile_count = (o && o->tile_count) ? o->tile_count : 1;
    if (r.tile_rank >= r.tile_count) throw std::runtime_error("tile_rank must be smaller than tile_count");
    if (r.spp == 0) throw std::runtime_error("spp must be positive");
    // passes: the integrator's `samples_per_pass`, then the 2^32 - 1 limit of a wavefront (whole image, not this rank's share)
    r.spp_total = r.spp; r.n_passes = 1; r.pass = 0;
    if (r.integrator != LRT_INTEGRATOR_PRBVOLPATH) {
        uint32_t per = d.samples_per_pass ? std::min(d.samples_per_pass, r.spp) : r.spp;
        if (r.spp % per != 0) throw std::runtime_error("sample_count (" + std::to_string(r.spp) + ") must be a multiple of spp_per_pass (" + std::to_string(per) + ").");
        const uint64_t wavefront = (uint64_t) d.film.crop_width * d.film.crop_height * per, limit = 0xffffffffull;
        if (wavefront > limit) per /= (uint32_t) ((wavefront + limit - 1) / limit);
        if (per == 0) throw std::runtime_error("film too large: a single sample per pixel exceeds 2^32 lanes");
        r.n_passes = r.spp_total / per; r.spp = per;
    }
    return r;
}

TilePixels tile_pixel_list(const DFilm &F, uint32_t rank, uint32_t count) {
    TilePixels T; std::vector<uint32_t> &px = T.list;
    uint32_t tx = (F.width + 31) / 32, ty = (F.height + 31) / 32;
    for (uint32_t t = rank; t < tx * ty; t += count) {
        uint32_t x0 = (t % tx) * 32, y0 = (t / tx) * 32;
        for (uint32_t y = y0; y < std::min<uint32_t>(y0 + 32, F.height); ++y)
            for (uint32_t x = x0; x < std::min<uint32_t>(x0 + 32, F.width); ++x) px.push_back(y * F.width + x);
    }
    std::vector<uint32_t> &inv = T.slot; inv.assign((size_t) F.width * F.height, 0u);
    for (size_t k = 0; k < px.size(); ++k) inv[px[k]] = (uint32_t) k;
    return T;
}

// The rank's tiles dilated by `halo` pixels, as a pixel list (row-major order inside the dilated tiles, every pixel once).  The PRB
// adjoint normalises by the per-pixel sum of reconstruction-filter weights (common.py:730-746): a rank reads that sum at the pixels its
// own lanes' footprints touch (own tiles + fn pixels), and those sums are complete once every lane within fn of them has been added:
// halo = 2 fn.  Without this every rank would walk all W H spp lanes of the image.
std::vector<uint32_t> halo_pixel_list(const DFilm &F, uint32_t rank, uint32_t count, uint32_t halo) {
    std::vector<uint8_t> mark((size_t) F.width * F.height, 0);
    const uint32_t tx = (F.width + 31) / 32, ty = (F.height + 31) / 32;
    for (uint32_t t = rank; t < tx * ty; t += count) {
        const int x0 = (int) (t % tx) * 32 - (int) halo, y0 = (int) (t / tx) * 32 - (int) halo;
        const int x1 = std::min<int>((int) (t % tx) * 32 + 32, F.width) + (int) halo, y1 = std::min<int>((int) (t / tx) * 32 + 32, F.height) + (int) halo;
        for (int y = std::max(y0, 0); y < std::min(y1, (int) F.height); ++y)
            for (int x = std::max(x0, 0); x < std::min(x1, (int) F.width); ++x) mark[(size_t) y * F.width + x] = 1;
    }
    std::vector<uint32_t> px;
    for (size_t k = 0; k < mark.size(); ++k) if (mark[k]) px.push_back((uint32_t) k);
    return px;
}

// 64-byte path records (record_layout.h, RecordLayout::Closed; instances k_render<LRT_INTEGRATOR_VOLPATH_CLOSED, ...>): volpath on a scene where only a path's last
// trip can add radiance, so that a record carries no radiance and no last-scatter pdf.  Called for every render with the current scene
// description (lrt_param_set may have changed sigma_t since the load); the caller also requires compact records (no area emitter, no EXT
// scene, BVH in LDS) and the volpath integrator.  Conditions:
//   (a) no medium is heterogeneous, every medium has sigma_t * scale finite and >= 1e-30 in every channel, the sensor sits in no medium and no shape has an
//       exterior medium (every medium is the inside of a shape);
//   (b) every shape has a delta-only BSDF: dielectric, or a bumpmap over a dielectric (no F_SMOOTH lobe, no null BSDF);
//   (c) the only emitter is one envmap or constant emitter.
// Proof that a record's radiance is +0 and last_pdf is never read (volpath_iteration):
//   1. surface NEE needs F_SMOOTH (b): it never runs;
//   2. in-medium NEE is +0: the shadow ray's free-flight draw -log(1 - u) / sigma_t is finite (a 24-bit uniform gives 1 - u >= 2^-24, so at
//      most 16.7 / 1e-30 < the largest float, (a)).  Either it lands inside the medium, a real collision (sigma_n = 0 in a homogeneous
//      medium) that zeroes the transmittance, or beyond the medium's boundary, a non-null surface (b) whose null transmission is 0; the
//      emitter sample lies at distance >= 2 r, beyond every surface;
//   3. the only emitter hit is the escape to the infinite emitter (c), and it ends the path.  A lane inside a medium never escapes (its
//      free flight is finite, (a)), so the escape follows a surface event, a delta bounce (b), which sets specular_chain; or it happens
//      at depth 0.  Either way count_direct holds and last_pdf / the last scatter position are not read.
// What the closed instances no longer compile (volpath_iteration<false, CLOSED = true>; each branch below is dead by the clause it names):
//   4. the surface emitter sampling (a second inlined volpath_sample_emitter, bsdf_eval, bsdf_pdf): 1., (b).  Its not-taken rng.skip(1) stays;
//   5. the hide_emitters skip loop at depth 0: it runs only when the first hit is a shape that is an emitter; no shape is one, (c).  The
//      `active_e` test after it still reads hide_emitters (the escape at depth 0 is hidden);
//   6. the in-medium shadow march beyond its observable part.  Its value is +0 by 2. and is not added, so what remains is the emitter sample
//      (two draws; a zero density ends it there), the march's single free-flight draw (or the skipped one when the segment is empty) and
//      the count of the shadow query the reference needs: exactly when that free flight leaves the segment (`!elide`: no null BSDF (b),
//      no heterogeneous medium (a)).  The march has no second trip: a valid collision multiplies the transmittance by sigma_n / combined
//      = 0 (a), an escape meets a non-null surface (b) or nothing.  The query itself is not traced: its result fed the discarded value only;
//   7. the BSDF dispatch of bsdf_sample: every leaf is a dielectric, under a bumpmap or not (b); the diffuse and null branches go;
//   8. emitters on shapes: si_emitter of a hit is -1 and emitter_eval is the infinite emitter's value on a miss, (c).
//      Since then the guard's "emitter hit without count_direct" sees the escape only: an emitting shape on a scene that got past this function
//      would lose its radiance without tripping n_closed_guard.  Clause (c) is tested below on the host for every render and is what rules it out.
//   (target_medium keeps its exterior branch although (a) makes it dead: removing it did not make the kernels smaller)
// So every queued record's radiance is +0 and a path's radiance is its last trip's: 0 + ... + 0 + c = c, bit for bit.  The kernels check 3. on every
// trip (DCounters::n_closed_guard: nonzero radiance on a lane that goes on, an emitter hit without count_direct) and the render fails instead of
// returning a wrong image.  2. is not checked (that check cost 2.5 % on C3): it rests on the conditions above alone.
bool closed_records(const lrt_scene_desc &d, int sensor_medium) {
    if (d.n_emitters != 1 || (d.emitters[0].type != LRT_EMITTER_ENVMAP && d.emitters[0].type != LRT_EMITTER_CONSTANT)) return false;
    if (sensor_medium >= 0) return false;
    for (uint32_t i = 0; i < d.n_media; ++i) {
        const lrt_medium_desc &M = d.media[i];
        if (M.type == LRT_MEDIUM_HETEROGENEOUS) return false;           // (volpath reads the bio media as homogeneous ones: sigma_t * scale)
        for (int k = 0; k < 3; ++k) { const float st = medium_sigma_t(M, k); if (!(std::isfinite(st) && st >= 1e-30f)) return false; }
    }
    for (uint32_t i = 0; i < d.n_shapes; ++i) {
        const lrt_shape_desc &S = d.shapes[i];
        if (S.exterior_medium >= 0 || S.bsdf < 0 || (uint32_t) S.bsdf >= d.n_bsdfs) return false;
        const lrt_bsdf_desc *B = &d.bsdfs[S.bsdf];
        if (B->type == LRT_BSDF_BUMPMAP) { if (B->nested < 0 || (uint32_t) B->nested >= d.n_bsdfs) return false; B = &d.bsdfs[B->nested]; }
        if (B->type != LRT_BSDF_DIELECTRIC) return false;
    }
    return true;
}

} // namespace lrt

// The scene checks are compiled as part of this unit: the preparation, the loader and the ABI all call them, and the host programs under tests/
// that build the preparation from an explicit source list (scene_prep.cpp, bvh.cpp, loader.cpp, xml.cpp, image_io.cpp) keep linking as they are.
#include "scene_check.cpp"
