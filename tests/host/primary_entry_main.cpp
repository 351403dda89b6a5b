// Stand-alone driver of the per-pixel primary entry (liverrenderer_amd/csrc/scene_prep.cpp: build_primary_entry) for tests/test_primary_entry.py.
// argv[1]: the directory that holds liver2.obj.  Prints one JSON line per scene (soundness), two seeded ones (the degenerate mesh and the thin shell), and one for the usefulness gate; it
// asserts nothing itself.
//   soundness: every ray is generated in float32 with camera_ray's own operations (generate_camera_path, kernels.h: fmaf, IEEE divisions) and tested
//     with test_tri_lds's float32 arithmetic and tie rule (dshade.h).  The closest hit over ALL triangles must equal the closest hit over the
//     triangles under the pixel's entry: same face, bit-equal t, u, v; a miss must equal a miss.  25 rays per pixel: the four corners, the four
//     edge midpoints, the centre, jitter 0, the largest float below 1, 14 random positions.
//   seeded: the same with delta = 0 and the occlusion margin reversed: the comparison has to find differences then.
//   usefulness: the liver at 1920 x 1080, every 4th pixel of every 4th row: node steps and triangle tests per ray of trace_lds's loop (restated
//     here in float32) from the entry and from the root, the shares of the four kinds of entry, the build time.
#include "scene_prep.h"
#include <cstdio>
#include <cstring>
#include <cmath>
#include <chrono>
#include <string>
#include <random>
#include <map>
#include <algorithm>

using namespace lrt;

struct F3 { float x, y, z; };
static inline float dotf(F3 a, F3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static inline F3 crossf(F3 a, F3 b) { return { fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)) }; }
struct RayF { F3 o, d; float maxt; };
struct HitF { float t = INFINITY, u = 0.f, v = 0.f; uint32_t prim = 0xffffffffu; };
static inline bool same_hit(const HitF &a, const HitF &b) { return a.prim == b.prim && memcmp(&a.t, &b.t, 4) == 0 && memcmp(&a.u, &b.u, 4) == 0 && memcmp(&a.v, &b.v, 4) == 0; }

// a scene: the description with its storage, the camera constants the device gets, the BVH
struct Scene {
    std::string name; std::vector<float> positions; std::vector<uint32_t> faces, face_shape; lrt_shape_desc shape{}; lrt_scene_desc d{};
    DCamera cam{}; DFilm film{}; HostBVH bvh; std::vector<uint16_t> tab; bool have_tab = false;
    std::vector<int32_t> node_ref;                          // per node: ref0, ref1, count0, count1
    std::vector<int32_t> leaf_count;                        // per slot: the size of the leaf that starts there, or 0
    std::vector<double> sphere;                             // per face: centroid and the radius around it
    uint32_t nf() const { return (uint32_t) (faces.size() / 3); }
    uint32_t vert(double x, double y, double z) { positions.push_back((float) x); positions.push_back((float) y); positions.push_back((float) z); return (uint32_t) (positions.size() / 3 - 1); }
    void tri(uint32_t a, uint32_t b, uint32_t c) { faces.push_back(a); faces.push_back(b); faces.push_back(c); }
    void quad(uint32_t a, uint32_t b, uint32_t c, uint32_t e) { tri(a, b, c); tri(a, c, e); }
    void box(double lo, double hi) {
        uint32_t q[8]; for (int i = 0; i < 8; ++i) q[i] = vert(i & 1 ? hi : lo, i & 2 ? hi : lo, i & 4 ? hi : lo);
        quad(q[0], q[1], q[3], q[2]); quad(q[4], q[6], q[7], q[5]); quad(q[0], q[4], q[5], q[1]); quad(q[2], q[3], q[7], q[6]); quad(q[0], q[2], q[6], q[4]); quad(q[1], q[5], q[7], q[3]);
    }
    // Transform::look_at (include/mitsuba/core/transform.h): columns left, up, dir, origin
    void look_at(const double o[3], const double t[3], const double up[3]) {
        double dir[3], left[3], nu[3], l = 0; for (int a = 0; a < 3; ++a) { dir[a] = t[a] - o[a]; l += dir[a] * dir[a]; } l = std::sqrt(l); for (double &v : dir) v /= l;
        left[0] = up[1] * dir[2] - up[2] * dir[1]; left[1] = up[2] * dir[0] - up[0] * dir[2]; left[2] = up[0] * dir[1] - up[1] * dir[0];
        l = std::sqrt(left[0] * left[0] + left[1] * left[1] + left[2] * left[2]); for (double &v : left) v /= l;
        nu[0] = dir[1] * left[2] - dir[2] * left[1]; nu[1] = dir[2] * left[0] - dir[0] * left[2]; nu[2] = dir[0] * left[1] - dir[1] * left[0];
        float *m = d.sensor.to_world; memset(m, 0, 64); m[15] = 1.f;
        for (int a = 0; a < 3; ++a) { m[4 * a] = (float) left[a]; m[4 * a + 1] = (float) nu[a]; m[4 * a + 2] = (float) dir[a]; m[4 * a + 3] = (float) o[a]; }
    }
    void sensor(double fov, int w, int h) {
        d.sensor.fov_x = (float) fov; d.sensor.near_clip = 1e-2f; d.sensor.far_clip = 1e4f; d.sensor.medium = -1;
        d.film.width = d.film.crop_width = w; d.film.height = d.film.crop_height = h; d.film.crop_offset_x = d.film.crop_offset_y = 0;
    }
    void finish(int leaf, const PrimaryEntryTune &tune = PrimaryEntryTune()) {
        face_shape.assign(nf(), 0u); shape.kind = LRT_SHAPE_MESH; shape.n_faces = nf();
        d.positions = positions.data(); d.faces = faces.data(); d.face_shape = face_shape.data(); d.n_vertices = (uint32_t) (positions.size() / 3); d.n_faces = nf(); d.shapes = &shape; d.n_shapes = 1;
        bvh = HostBVH(); build_bvh(d.positions, d.faces, d.n_faces, bvh, leaf);
        build_camera(d, cam, film);                                 // the camera and the film as the device gets them
        build_primary_entry(d, bvh, tab, tune); have_tab = !tab.empty();
        if (!have_tab) tab.assign((size_t) film.width * film.height, 0);
        node_ref.resize(bvh.nodes.size() / 16 * 4);
        for (size_t n = 0; n < bvh.nodes.size() / 16; ++n) memcpy(&node_ref[4 * n], &bvh.nodes[16 * n + 12], 16);
        sphere.resize(4 * (size_t) nf());
        for (uint32_t f = 0; f < nf(); ++f) {
            double c[3] = { 0, 0, 0 }, r = 0; for (int j = 0; j < 3; ++j) for (int a = 0; a < 3; ++a) c[a] += positions[3 * (size_t) faces[3 * f + j] + a] / 3.0;
            for (int j = 0; j < 3; ++j) { double l = 0; for (int a = 0; a < 3; ++a) { const double e = positions[3 * (size_t) faces[3 * f + j] + a] - c[a]; l += e * e; } r = std::max(r, std::sqrt(l)); }
            sphere[4 * f] = c[0]; sphere[4 * f + 1] = c[1]; sphere[4 * f + 2] = c[2]; sphere[4 * f + 3] = r;
        }
        leaf_count.assign(bvh.tris.size() / 12 + 1, 0);
        if (!bvh.root_is_leaf) for (size_t n = 0; n < node_ref.size() / 4; ++n) for (int c = 0; c < 2; ++c) if (node_ref[4 * n + c] < 0) leaf_count[(uint32_t) ~node_ref[4 * n + c]] = node_ref[4 * n + 2 + c];
    }
    uint32_t slot_face(uint32_t s) const { uint32_t f; memcpy(&f, &bvh.tris[12 * (size_t) s + 3], 4); return f; }
    // the faces under a work item
    void faces_under(uint16_t item, std::vector<uint32_t> &out) const {
        out.clear();
        if (item == LRT_PRIMARY_NONE) return;
        if (bvh.root_is_leaf) { for (uint32_t i = 0; i < bvh.root_count; ++i) out.push_back(slot_face(bvh.root_first + i)); return; }
        if (item & 0x8000u) { const uint32_t first = item & 0x7fffu; for (int32_t i = 0; i < leaf_count[first]; ++i) out.push_back(slot_face(first + (uint32_t) i)); return; }
        std::vector<uint32_t> todo{ item };
        while (!todo.empty()) {
            const uint32_t n = todo.back(); todo.pop_back();
            for (int c = 0; c < 2; ++c) { const int32_t r = node_ref[4 * n + c]; if (r >= 0) todo.push_back((uint32_t) r); else for (int32_t i = 0; i < node_ref[4 * n + 2 + c]; ++i) out.push_back(slot_face((uint32_t) ~r + (uint32_t) i)); }
        }
    }
    // generate_camera_path + camera_ray (kernels.h) for pixel (px, py) of the film and jitter (jx, jy)
    RayF camera_ray(int px, int py, float jx, float jy) const {
        const float spx = (float) px + jx, spy = (float) py + jy;
        const float ax = fmaf(spx, film.scale_x, film.offset_x), ay = fmaf(spy, film.scale_y, film.offset_y);
        const float *m = cam.s2c; const F3 p = { ax + cam.ppo_x, ay + cam.ppo_y, 0.f };
        float r[4]; for (int i = 0; i < 4; ++i) r[i] = fmaf(m[4 * i + 2], p.z, fmaf(m[4 * i + 1], p.y, fmaf(m[4 * i + 0], p.x, m[4 * i + 3])));
        const F3 np = { r[0] / r[3], r[1] / r[3], r[2] / r[3] };
        const float il = 1.f / sqrtf(dotf(np, np)); const F3 dc = { np.x * il, np.y * il, np.z * il };
        const float *w = cam.to_world; RayF ray;
        ray.o = { w[3], w[7], w[11] };
        ray.d = { fmaf(w[2], dc.z, fmaf(w[1], dc.y, w[0] * dc.x)), fmaf(w[6], dc.z, fmaf(w[5], dc.y, w[4] * dc.x)), fmaf(w[10], dc.z, fmaf(w[9], dc.y, w[8] * dc.x)) };
        const float inv_z = 1.f / dc.z, near_t = cam.near_clip * inv_z, far_t = cam.far_clip * inv_z;
        ray.o = { ray.o.x + ray.d.x * near_t, ray.o.y + ray.d.y * near_t, ray.o.z + ray.d.z * near_t };
        ray.maxt = far_t - near_t;
        return ray;
    }
    // test_tri_lds (dshade.h)
    void test_tri(uint32_t f, const RayF &r, HitF &best) const {
        const float *a = &positions[3 * (size_t) faces[3 * f]], *b = &positions[3 * (size_t) faces[3 * f + 1]], *c = &positions[3 * (size_t) faces[3 * f + 2]];
        const F3 e1 = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, e2 = { c[0] - a[0], c[1] - a[1], c[2] - a[2] };
        const F3 pvec = crossf(r.d, e2); const float inv_det = 1.f / dotf(e1, pvec);
        const F3 tvec = { r.o.x - a[0], r.o.y - a[1], r.o.z - a[2] };
        const float u = dotf(tvec, pvec) * inv_det; if (!(u >= 0.f && u <= 1.f)) return;
        const F3 qvec = crossf(tvec, e1);
        const float v = dotf(r.d, qvec) * inv_det; if (!(v >= 0.f && u + v <= 1.f)) return;
        const float t = dotf(e2, qvec) * inv_det; if (!(t >= 0.f && t <= r.maxt)) return;
        if (t > best.t) return;
        if (t < best.t || f < best.prim) { best.t = t; best.u = u; best.v = v; best.prim = f; }
    }
    // The closest hit over all triangles.  A face is left out only when the ray's line passes its bounding sphere at more than 1.001 radii plus 1e-4 of
    // the centre's distance (float64; a thousand times what float32 can move a hit): a cull by geometry alone, which knows nothing of the table.
    HitF closest_of_all(const RayF &r) const {
        HitF best; const double o[3] = { r.o.x, r.o.y, r.o.z }, d[3] = { r.d.x, r.d.y, r.d.z }, dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        for (uint32_t f = 0; f < nf(); ++f) {
            const double *s = &sphere[4 * (size_t) f], e[3] = { s[0] - o[0], s[1] - o[1], s[2] - o[2] }, ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], ed = e[0] * d[0] + e[1] * d[1] + e[2] * d[2];
            const double reach = 1.001 * s[3] + 1e-4 * std::sqrt(ee) + 1e-9;
            if (ee - ed * ed / dd > reach * reach) continue;
            test_tri(f, r, best);
        }
        return best;
    }
    // trace_lds's loop from a start item, counting node steps and triangle tests
    HitF trace(const RayF &r, uint16_t start, uint64_t &n_nodes, uint64_t &n_tris) const {
        HitF best;
        if (start == LRT_PRIMARY_NONE) return best;
        auto rc = [](float x) { return fminf(fmaxf(1.f / x, -1e20f), 1e20f); };
        const float ix = rc(r.d.x), iy = rc(r.d.y), iz = rc(r.d.z), ox = -r.o.x * ix, oy = -r.o.y * iy, oz = -r.o.z * iz;
        uint32_t stack[64]; int sp = 0; uint32_t cur = start; const uint32_t DONE = 0x10000u;
        for (;;) {
            while (cur < 0x8000u) {
                ++n_nodes;
                const float *n = &bvh.nodes[16 * (size_t) cur]; const float limit = fminf(best.t, r.maxt);
                const float ax0 = fmaf(n[0], ix, ox), ax1 = fmaf(n[1], ix, ox), ay0 = fmaf(n[2], iy, oy), ay1 = fmaf(n[3], iy, oy), az0 = fmaf(n[8], iz, oz), az1 = fmaf(n[9], iz, oz);
                const float bx0 = fmaf(n[4], ix, ox), bx1 = fmaf(n[5], ix, ox), by0 = fmaf(n[6], iy, oy), by1 = fmaf(n[7], iy, oy), bz0 = fmaf(n[10], iz, oz), bz1 = fmaf(n[11], iz, oz);
                const float tmin0 = fmaxf(fmaxf(fminf(ax0, ax1), fminf(ay0, ay1)), fmaxf(fminf(az0, az1), 0.f)), tmax0 = fminf(fminf(fmaxf(ax0, ax1), fmaxf(ay0, ay1)), fminf(fmaxf(az0, az1), limit));
                const float tmin1 = fmaxf(fmaxf(fminf(bx0, bx1), fminf(by0, by1)), fmaxf(fminf(bz0, bz1), 0.f)), tmax1 = fminf(fminf(fmaxf(bx0, bx1), fmaxf(by0, by1)), fminf(fmaxf(bz0, bz1), limit));
                const bool h0 = tmin0 <= tmax0 * 1.000002f, h1 = tmin1 <= tmax1 * 1.000002f;
                uint32_t c[2]; for (int k = 0; k < 2; ++k) { const int32_t ref = node_ref[4 * (size_t) cur + k]; c[k] = ref < 0 ? (0x8000u | (uint32_t) ~ref) : (uint32_t) ref; }
                if (h0 && h1) { const bool swap = tmin1 < tmin0; stack[sp++] = swap ? c[0] : c[1]; cur = swap ? c[1] : c[0]; }
                else if (h0 || h1) cur = h0 ? c[0] : c[1];
                else if (sp == 0) cur = DONE;
                else cur = stack[--sp];
            }
            if (cur == DONE) break;
            const uint32_t first = cur & 0x7fffu; const int32_t count = leaf_count[first];
            for (int32_t i = 0; i < count; ++i) { ++n_tris; test_tri(slot_face(first + (uint32_t) i), r, best); }
            if (sp == 0) break;
            cur = stack[--sp];
        }
        return best;
    }
};

static void soundness(const Scene &S, const char *kind = "soundness") {
    const int W = S.film.width, H = S.film.height, cox = S.film.crop_offset_x, coy = S.film.crop_offset_y;
    std::mt19937_64 gen(977u + S.nf()); std::uniform_real_distribution<float> U(0.f, 1.f);
    const float below1 = std::nextafterf(1.f, 0.f);
    uint64_t rays = 0, diffs = 0, hits = 0, kinds[4] = { 0, 0, 0, 0 }; int first_bad[2] = { -1, -1 };
    std::map<uint16_t, std::vector<uint32_t>> under;
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const uint16_t item = S.tab[(size_t) y * W + x];
        ++kinds[item == LRT_PRIMARY_NONE ? 0 : ((item & 0x8000u) ? 1 : (item ? 2 : 3))];
        auto it = under.find(item);
        if (it == under.end()) { it = under.emplace(item, std::vector<uint32_t>()).first; S.faces_under(item, it->second); }
        const std::vector<uint32_t> &sub = it->second;
        float j[25][2] = { { 0.f, 0.f }, { 1.f, 0.f }, { 0.f, 1.f }, { 1.f, 1.f }, { .5f, 0.f }, { 0.f, .5f }, { 1.f, .5f }, { .5f, 1.f }, { .5f, .5f }, { 0.f, 0.f }, { below1, below1 } };
        for (int k = 11; k < 25; ++k) { j[k][0] = U(gen); j[k][1] = U(gen); }
        for (int k = 0; k < 25; ++k) {
            const RayF r = S.camera_ray(x + cox, y + coy, j[k][0], j[k][1]);
            HitF all, part;
            all = S.closest_of_all(r);
            if (item == 0) part = all; else for (uint32_t f : sub) S.test_tri(f, r, part);
            ++rays; hits += all.prim != 0xffffffffu;
            if (!same_hit(all, part)) { if (!diffs) { first_bad[0] = x; first_bad[1] = y; } ++diffs; }
        }
    }
    printf("{\"case\":\"%s\",\"scene\":\"%s\",\"faces\":%u,\"width\":%d,\"height\":%d,\"crop_x\":%d,\"crop_y\":%d,\"table\":%s,\"valid\":%s,\"rays\":%llu,\"hits\":%llu,\"differences\":%llu,\"first_bad\":[%d,%d],"
           "\"none\":%llu,\"leaf\":%llu,\"node\":%llu,\"root\":%llu}\n", kind, S.name.c_str(), S.nf(), W, H, cox, coy, S.have_tab ? "true" : "false", primary_entry_valid(S.bvh, S.tab) || S.bvh.root_is_leaf ? "true" : "false",
           (unsigned long long) rays, (unsigned long long) hits, (unsigned long long) diffs, first_bad[0], first_bad[1],
           (unsigned long long) kinds[0], (unsigned long long) kinds[1], (unsigned long long) kinds[2], (unsigned long long) kinds[3]);
    fflush(stdout);
}

// ---- the small scenes.  Each gets a camera that sees the whole mesh from outside unless its name says otherwise.
static void aim(Scene &S, double ox, double oy, double oz, double tx, double ty, double tz, double fov, int w, int h) {
    const double o[3] = { ox, oy, oz }, t[3] = { tx, ty, tz }, up[3] = { 0.1, 1.0, 0.05 };
    S.sensor(fov, w, h); S.look_at(o, t, up);
}
static void folded_strips(Scene &S, const PrimaryEntryTune &tune) {       // strips folded by 20, 45 and 80 degrees, side by side: the folded part hides, or is hidden by, the flat one
    S.name = "folded_strips";
    int n = 0;
    for (double deg : { 20.0, 45.0, 80.0 }) {
        const double a = deg * 3.14159265358979323846 / 180.0; uint32_t id[5][3];
        for (int i = 0; i < 5; ++i) for (int j = 0; j < 3; ++j) { const double x = i <= 2 ? (double) i : 2.0 + (i - 2) * std::cos(a), z = i <= 2 ? 0.0 : (i - 2) * std::sin(a); id[i][j] = S.vert(x + 3.25, (double) j - 1.5 + 3.0 * n, z + 0.125); }
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 2; ++j) S.quad(id[i][j], id[i + 1][j], id[i + 1][j + 1], id[i][j + 1]);
        ++n;
    }
    aim(S, 14.0, 3.2, 2.5, 5.0, 3.0, 0.4, 50.0, 96, 64); S.finish(2, tune);
}
static void nested_boxes(Scene &S, const PrimaryEntryTune &tune) { S.name = "nested_boxes"; S.box(-2.0, 2.0); S.box(-0.5, 0.75); aim(S, 7.0, 4.0, 9.0, 0.0, 0.0, 0.0, 40.0, 80, 60); S.finish(2, tune); }
static void thin_shell(Scene &S, const PrimaryEntryTune &tune) {
    S.name = "thin_shell";
    for (int sheet = 0; sheet < 2; ++sheet) {
        uint32_t id[3][3]; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) id[i][j] = S.vert(i + 0.3 * sheet, j - 0.2 * sheet, 7.0 + 0.01 * sheet);
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) S.quad(id[i][j], id[i + 1][j], id[i + 1][j + 1], id[i][j + 1]);
    }
    aim(S, 1.2, 0.9, 12.0, 1.1, 1.0, 7.0, 35.0, 80, 60); S.finish(2, tune);
}
static void degenerate(Scene &S, const PrimaryEntryTune &tune) {          // zero-area faces, a repeated vertex, a point, and one face twice (a tie that the face index breaks), seen face-on
    S.name = "degenerate";
    const uint32_t a = S.vert(0, 0, 0), b = S.vert(1, 0, 0), c = S.vert(1, 1, 0), e = S.vert(0, 1, 0), m = S.vert(0.5, 0.5, 0), t = S.vert(0.5, 0.5, 1), a2 = S.vert(0, 0, 0);
    S.quad(a, b, c, e); S.tri(a, m, c); S.tri(b, b, t); S.tri(a2, t, e); S.tri(t, t, t);
    S.tri(a, c, e);                                                 // the quad's second triangle again
    const uint32_t p = S.vert(0.2, 0.2, -0.5), q = S.vert(0.9, 0.2, -0.5), r = S.vert(0.2, 0.9, -0.5); S.tri(p, q, r); S.tri(r, p, q);   // and a pair behind it, one of them rotated
    aim(S, 0.5, 0.5, 4.0, 0.5, 0.5, 0.0, 30.0, 64, 64); S.finish(2, tune);
}
static void single_triangle(Scene &S, const PrimaryEntryTune &tune) { S.name = "single_triangle"; S.tri(S.vert(1, 2, 3), S.vert(2, 2, 3.5), S.vert(1, 3, 3)); aim(S, 1.4, 2.4, 6.0, 1.3, 2.3, 3.0, 30.0, 48, 48); S.finish(2, tune); }
static void near_plane(Scene &S, const PrimaryEntryTune &tune) {          // a floor that passes under the camera and through its near plane, and a box on it
    S.name = "near_plane";
    uint32_t id[5][5]; for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) id[i][j] = S.vert(i - 2.0, -0.02, j - 2.0);
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) S.quad(id[i][j], id[i + 1][j], id[i + 1][j + 1], id[i][j + 1]);
    const size_t v0 = S.positions.size() / 3; S.box(-0.2, 0.2); for (size_t v = v0; v < S.positions.size() / 3; ++v) { S.positions[3 * v + 1] += 0.18f; S.positions[3 * v + 2] -= 1.f; }
    aim(S, 0.1, 0.0, 0.3, 0.0, 0.1, -1.0, 70.0, 64, 48); S.finish(2, tune);
}
static void inside_box(Scene &S, const PrimaryEntryTune &tune) { S.name = "inside_box"; S.box(-2.0, 2.0); S.box(0.4, 0.9); aim(S, -0.5, -0.3, -1.0, 0.65, 0.65, 0.65, 60.0, 64, 48); S.finish(2, tune); }

static void load_liver(Scene &S, const char *dir, int w, int h, int cx, int cy, int cw, int ch, const PrimaryEntryTune &tune = PrimaryEntryTune()) {
    // the liver mesh and the sensor of scenes/Liver-SingleMesh/mitsuba3/scene.xml through the project's loader (textures and environment map are not needed here)
    const std::string xml = "<scene version=\"3.0.0\"><integrator type=\"volpath\"/><sensor type=\"perspective\"><float name=\"fov\" value=\"45\"/><transform name=\"to_world\">"
                            "<lookat up=\"-0.317370, 0.895343, -0.312469\" target=\"6.826270, 5.011984, 5.896974\" origin=\"7.481132, 5.343665, 6.507640\"/></transform>"
                            "<film type=\"hdrfilm\"><integer name=\"width\" value=\"" + std::to_string(w) + "\"/><integer name=\"height\" value=\"" + std::to_string(h) + "\"/><rfilter type=\"box\"/></film><sampler type=\"independent\"/></sensor>"
                            "<shape type=\"obj\"><string name=\"filename\" value=\"liver2.obj\"/><transform name=\"to_world\"><scale value=\"1\"/><translate x=\"-5\" y=\"5\" z=\"-5\"/></transform>"
                            "<bsdf type=\"dielectric\"/></shape><emitter type=\"constant\"/></scene>";
    SceneStorage st; load_scene_xml(xml, dir, {}, st);
    const lrt_scene_desc &d = st.desc;
    S.positions.assign(d.positions, d.positions + 3 * (size_t) d.n_vertices); S.faces.assign(d.faces, d.faces + 3 * (size_t) d.n_faces);
    S.d.sensor = d.sensor; S.d.film = d.film;
    if (cw) { S.d.film.crop_offset_x = cx; S.d.film.crop_offset_y = cy; S.d.film.crop_width = cw; S.d.film.crop_height = ch; }
    S.finish(3, tune);                                              // (the leaf size the preparation chooses for this mesh)
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: primary_entry_main <directory of liver2.obj>\n"); return 2; }
    try {
        const PrimaryEntryTune good;
        { Scene S; folded_strips(S, good); soundness(S); } { Scene S; nested_boxes(S, good); soundness(S); } { Scene S; thin_shell(S, good); soundness(S); }
        { Scene S; degenerate(S, good); soundness(S); } { Scene S; single_triangle(S, good); soundness(S); } { Scene S; near_plane(S, good); soundness(S); } { Scene S; inside_box(S, good); soundness(S); }
        { Scene S; S.name = "liver_160x90"; load_liver(S, argv[1], 160, 90, 0, 0, 0, 0); soundness(S); }
        { Scene S; S.name = "liver_1080p_crop"; load_liver(S, argv[1], 1920, 1080, 1168, 90, 64, 64); soundness(S); }
        // the seeded mistake: no dilation, and the depth margin the wrong way round
        PrimaryEntryTune bad; bad.delta = 0.0; bad.depth_margin = -1e-4;
        { Scene S; degenerate(S, bad); soundness(S, "seeded"); }
        { Scene S; thin_shell(S, bad); soundness(S, "seeded"); }
        // usefulness
        {
            Scene S; S.name = "liver_1080p"; load_liver(S, argv[1], 1920, 1080, 0, 0, 0, 0);
            double best_ms = 1e30;
            for (int rep = 0; rep < 2; ++rep) {                               // (this program is sanitized: an upper figure)
                std::vector<uint16_t> t; const auto t0 = std::chrono::steady_clock::now(); build_primary_entry(S.d, S.bvh, t);
                best_ms = std::min(best_ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            uint64_t kinds[4] = { 0, 0, 0, 0 }; for (uint16_t item : S.tab) ++kinds[item == LRT_PRIMARY_NONE ? 0 : ((item & 0x8000u) ? 1 : (item ? 2 : 3))];
            std::mt19937_64 gen(4242); std::uniform_real_distribution<float> U(0.f, 1.f);
            uint64_t rays = 0, nr = 0, tr = 0, ne = 0, te = 0, diffs = 0;
            for (int y = 0; y < 1080; y += 4) for (int x = 0; x < 1920; x += 4) for (int k = 0; k < 4; ++k) {
                const RayF r = S.camera_ray(x, y, k ? U(gen) : .5f, k ? U(gen) : .5f);
                const HitF a = S.trace(r, 0, nr, tr), b = S.trace(r, S.tab[(size_t) y * 1920 + x], ne, te);
                ++rays; diffs += !same_hit(a, b);
            }
            const double n = (double) rays, np = (double) S.tab.size();
            printf("{\"case\":\"usefulness\",\"scene\":\"liver_1080p\",\"rays\":%llu,\"differences\":%llu,\"nodes\":%zu,\"depth\":%d,\"node_steps_root\":%.4f,\"tri_tests_root\":%.4f,\"node_steps_entry\":%.4f,\"tri_tests_entry\":%.4f,"
                   "\"none\":%.6f,\"leaf\":%.6f,\"node\":%.6f,\"root\":%.6f,\"table_bytes\":%zu,\"build_ms\":%.3f}\n", (unsigned long long) rays, (unsigned long long) diffs, S.bvh.nodes.size() / 16, S.bvh.max_depth,
                   nr / n, tr / n, ne / n, te / n, kinds[0] / np, kinds[1] / np, kinds[2] / np, kinds[3] / np, S.tab.size() * sizeof(uint16_t), best_ms);
        }
    } catch (const std::exception &e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
    return 0;
}
