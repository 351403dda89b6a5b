// Stand-alone driver of the host-only scene preparation (liverrenderer_amd/csrc/scene_prep.cpp) for tests/test_scene_prep.py:
// builds small scene descriptions, calls the preparation unit and prints one JSON line per case.  It asserts nothing itself.
#include "scene_prep.h"
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <string>
#include <stdexcept>

using namespace lrt;

// ---- JSON on stdout (floats as %.9g: a float32 survives the round trip)
static std::string js(const float *v, size_t n) { std::string s = "["; char b[40]; for (size_t i = 0; i < n; ++i) { snprintf(b, sizeof b, "%s%.9g", i ? "," : "", (double) v[i]); s += b; } return s + "]"; }
template <typename T> static std::string ji(const T *v, size_t n) { std::string s = "["; for (size_t i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string((long long) v[i]); return s + "]"; }
static std::string jf(float v) { return js(&v, 1).substr(1, js(&v, 1).size() - 2); }
static std::string hex(const std::vector<unsigned char> &b) { static const char *d = "0123456789abcdef"; std::string s; for (unsigned char c : b) { s += d[c >> 4]; s += d[c & 15]; } return s; }
static std::string jstr(const std::string &s) { std::string r = "\""; for (char c : s) { if (c == '"' || c == '\\') r += '\\'; r += c; } return r + "\""; }

// ---- a scene description that owns its arrays
struct Scene {
    std::vector<float> positions, normals, texcoords; std::vector<uint32_t> faces, face_shape;
    std::vector<lrt_shape_desc> shapes; std::vector<lrt_bsdf_desc> bsdfs; std::vector<lrt_texture_desc> textures;
    std::vector<lrt_medium_desc> media; std::vector<lrt_emitter_desc> emitters;
    lrt_scene_desc base{};
    Scene() {
        base.sensor.fov_x = 40.f; base.sensor.near_clip = 0.01f; base.sensor.far_clip = 100.f; base.sensor.medium = -1;
        for (int i = 0; i < 4; ++i) base.sensor.to_world[5 * i] = 1.f;
        base.film.width = base.film.crop_width = 16; base.film.height = base.film.crop_height = 8;
        base.integrator.type = LRT_INTEGRATOR_VOLPATH; base.integrator.max_depth = 8; base.integrator.rr_depth = 5;
        base.sample_count = 4; base.use_spectral_mis = 1;
    }
    lrt_scene_desc desc() {
        lrt_scene_desc d = base;
        normals.resize(positions.size(), 0.f); texcoords.resize(positions.size() / 3 * 2, 0.f);
        d.n_vertices = (uint32_t) (positions.size() / 3); d.n_faces = (uint32_t) (faces.size() / 3); d.n_shapes = (uint32_t) shapes.size();
        d.n_bsdfs = (uint32_t) bsdfs.size(); d.n_textures = (uint32_t) textures.size(); d.n_media = (uint32_t) media.size(); d.n_emitters = (uint32_t) emitters.size();
        d.positions = positions.data(); d.normals = normals.data(); d.texcoords = texcoords.data(); d.faces = faces.data(); d.face_shape = face_shape.data();
        d.shapes = shapes.data(); d.bsdfs = bsdfs.data(); d.textures = textures.data(); d.media = media.data(); d.emitters = emitters.data();
        return d;
    }
    int add_bsdf(int type, int nested = -1, int reflectance = -1) { lrt_bsdf_desc b{}; b.type = type; b.nested = nested; b.reflectance = reflectance; b.texture = -1; b.eta = 1.5f; b.scale = 1.f; bsdfs.push_back(b); return (int) bsdfs.size() - 1; }
    int add_rgb_texture() { lrt_texture_desc t{}; t.type = LRT_TEX_RGB; t.color0[0] = t.color0[1] = t.color0[2] = .5f; textures.push_back(t); return (int) textures.size() - 1; }
    int add_medium(int type, float sigma_t, float scale) {
        lrt_medium_desc m{}; m.type = type; m.scale = scale; for (int k = 0; k < 3; ++k) { m.sigma_t[k] = sigma_t; m.albedo[k] = .5f; }
        media.push_back(m); return (int) media.size() - 1;
    }
    // a shape over the faces appended since the last shape
    int add_shape(int kind, int bsdf, int interior = -1, int exterior = -1) {
        lrt_shape_desc s{}; s.kind = kind; s.bsdf = bsdf; s.emitter = -1; s.interior_medium = interior; s.exterior_medium = exterior;
        s.first_face = (uint32_t) face_shape.size(); s.n_faces = (uint32_t) (faces.size() / 3 - face_shape.size());
        for (int i = 0; i < 4; ++i) s.to_world[5 * i] = 1.f;
        face_shape.resize(faces.size() / 3, (uint32_t) shapes.size()); shapes.push_back(s); return (int) shapes.size() - 1;
    }
    // planar grid of quads in z = 0, cut to exactly n_faces triangles
    void add_grid(uint32_t n_faces) {
        uint32_t q = (n_faces + 1) / 2, nx = 1; while (nx * nx < q) ++nx; uint32_t ny = (q + nx - 1) / nx, v0 = (uint32_t) (positions.size() / 3);
        for (uint32_t y = 0; y <= ny; ++y) for (uint32_t x = 0; x <= nx; ++x) { positions.push_back((float) x); positions.push_back((float) y); positions.push_back(0.f); }
        uint32_t made = 0;
        for (uint32_t y = 0; y < ny && made < n_faces; ++y) for (uint32_t x = 0; x < nx && made < n_faces; ++x) {
            uint32_t a = v0 + y * (nx + 1) + x, b = a + 1, c = a + nx + 1, e = c + 1;
            for (uint32_t i : { a, b, e }) faces.push_back(i); ++made;
            if (made < n_faces) { for (uint32_t i : { a, e, c }) faces.push_back(i); ++made; }
        }
    }
    // a row of n separate triangles, one per unit of x (the builder can cut it anywhere: leaves of 3 appear, which a quad grid never has)
    void add_row(uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) { uint32_t v = (uint32_t) (positions.size() / 3); for (float c : { (float) i, 0.f, 0.f, (float) i + .5f, 0.f, 0.f, (float) i, 1.f, 0.f }) positions.push_back(c); for (uint32_t k = 0; k < 3; ++k) faces.push_back(v + k); }
    }
    void add_cube() {      // the unit cube [0, 1]^3
        uint32_t v0 = (uint32_t) (positions.size() / 3);
        for (int i = 0; i < 8; ++i) { positions.push_back((float) (i & 1)); positions.push_back((float) ((i >> 1) & 1)); positions.push_back((float) ((i >> 2) & 1)); }
        static const int q[6][4] = { { 0, 1, 3, 2 }, { 4, 6, 7, 5 }, { 0, 4, 5, 1 }, { 2, 3, 7, 6 }, { 0, 2, 6, 4 }, { 1, 5, 7, 3 } };
        for (auto &f : q) { for (int i : { f[0], f[1], f[2] }) faces.push_back(v0 + i); for (int i : { f[0], f[2], f[3] }) faces.push_back(v0 + i); }
    }
    int add_emitter(int type, int shape = -1) { lrt_emitter_desc e{}; e.type = type; e.shape = shape; e.scale = 1.f; for (int k = 0; k < 3; ++k) e.radiance[k] = 1.f; for (int i = 0; i < 4; ++i) e.to_world[5 * i] = 1.f; emitters.push_back(e); return (int) emitters.size() - 1; }
    std::vector<float> env_texels;
    int add_envmap(int w, int h, int zero_x = -1, int zero_y = -1) {
        env_texels.resize((size_t) w * h * 3);
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) for (int k = 0; k < 3; ++k) env_texels[((size_t) y * w + x) * 3 + k] = (x == zero_x && y == zero_y) ? 0.f : 0.25f + 0.125f * (float) ((3 * x + 5 * y + k) % 7);
        int i = add_emitter(LRT_EMITTER_ENVMAP); emitters[i].width = w; emitters[i].height = h; emitters[i].data = env_texels.data(); return i;
    }
};

static PrepOptions generous() { PrepOptions o; o.lds_limit = (size_t) 1 << 30; return o; }

static std::string lds_json(const PreparedScene &P, bool with_blob) {
    std::string s = "\"use_lds\":" + std::to_string((int) P.use_lds) + ",\"bvh_leaf\":" + std::to_string(P.bvh_leaf) + ",\"n_nodes\":" + std::to_string(P.bvh.nodes.size() / 16) +
                    ",\"n_slots\":" + std::to_string(P.bvh.tris.size() / 12) + ",\"root_is_leaf\":" + std::to_string(P.sc.root_is_leaf) + ",\"root_leaf_first\":" + std::to_string(P.sc.root_leaf_first) +
                    ",\"root_leaf_count\":" + std::to_string(P.sc.root_leaf_count) + ",\"n_faces\":" + std::to_string(P.sc.n_faces);
    if (P.use_lds) s += ",\"blob_bytes\":" + std::to_string(P.lds.blob_bytes) + ",\"nodes_off\":" + std::to_string(P.lds.nodes_off) + ",\"verts_off\":" + std::to_string(P.lds.verts_off) +
                        ",\"tris_off\":" + std::to_string(P.lds.tris_off) + ",\"stack_off\":" + std::to_string(P.lds.stack_off) + ",\"total_bytes\":" + std::to_string(P.lds.total_bytes) +
                        ",\"image_bytes\":" + std::to_string(lds_image_bytes(P.bvh, (uint32_t) (P.vattr.size() / 8)));
    if (P.use_lds && with_blob) s += ",\"blob\":\"" + hex(P.lds_blob) + "\"";
    return s;
}

static void case_triangle() {
    Scene S; S.positions = { 0, 0, 0, 1, 0, 0, 0, 1, 0 }; S.faces = { 0, 1, 2 }; S.add_shape(LRT_SHAPE_MESH, S.add_bsdf(LRT_BSDF_DIELECTRIC));
    PreparedScene P = prepare_scene(S.desc(), generous());
    printf("{\"case\":\"triangle\",%s}\n", lds_json(P, true).c_str());
}

// The leaf-size search on a planar grid of quads, or on a row of separate triangles.  One run per leaf size whose image is smaller than every thinner leaf's, with that image's size as
// the limit (the search must skip the thinner ones and stop there); then nothing fits, forced sizes, and the switch.
static void case_grid(const char *mesh, uint32_t n_faces) {
    Scene S; if (mesh[0] == 'g') S.add_grid(n_faces); else S.add_row(n_faces); S.add_shape(LRT_SHAPE_MESH, S.add_bsdf(LRT_BSDF_DIELECTRIC)); lrt_scene_desc d = S.desc();
    size_t bytes[17] = {}, smallest = ~size_t(0);
    struct Run { std::string name; size_t limit; int forced; bool no_lds; }; std::vector<Run> runs;
    for (int leaf : { 2, 3, 4, 6, 8, 12, 16 }) {
        HostBVH b; build_bvh(d.positions, d.faces, d.n_faces, b, leaf); bytes[leaf] = lds_image_bytes(b, d.n_vertices);
        if (bytes[leaf] < smallest) { smallest = bytes[leaf]; runs.push_back({ "limit_of_leaf" + std::to_string(leaf), bytes[leaf], 0, false }); }
    }
    printf("{\"case\":\"grid_sizes\",\"mesh\":\"%s\",\"faces\":%u,\"n_vertices\":%u,\"bytes\":%s}\n", mesh, n_faces, d.n_vertices, ji(bytes, 17).c_str());
    runs.push_back({ "nothing", smallest - 1, 0, false }); runs.push_back({ "forced8", (size_t) 1 << 30, 8, false });
    runs.push_back({ "forced2_small", bytes[2] - 1, 2, false }); runs.push_back({ "switch", (size_t) 1 << 30, 0, true });
    for (const Run &r : runs) {
        PrepOptions o; o.lds_limit = r.limit; o.bvh_leaf = r.forced; o.no_lds_bvh = r.no_lds;
        PreparedScene P = prepare_scene(d, o);
        printf("{\"case\":\"grid\",\"mesh\":\"%s\",\"faces\":%u,\"run\":\"%s\",\"limit\":%zu,\"forced\":%d,\"switch\":%d,%s}\n", mesh, n_faces, r.name.c_str(), r.limit, r.forced, (int) r.no_lds, lds_json(P, true).c_str());
    }
}

static void case_limits16() {
    for (uint32_t nf : { 32767u, 32768u }) {
        Scene S; S.add_grid(nf); S.add_shape(LRT_SHAPE_MESH, S.add_bsdf(LRT_BSDF_DIELECTRIC));
        PreparedScene P = prepare_scene(S.desc(), generous());
        printf("{\"case\":\"limits16\",\"n_vertices\":%zu,%s}\n", S.positions.size() / 3, lds_json(P, false).c_str());
    }
    for (uint32_t nv : { 65535u, 65536u }) {           // 64 triangles and unreferenced vertices up to the count
        Scene S; S.add_grid(64); S.positions.resize(3 * (size_t) nv, 0.5f); S.add_shape(LRT_SHAPE_MESH, S.add_bsdf(LRT_BSDF_DIELECTRIC));
        PreparedScene P = prepare_scene(S.desc(), generous());
        printf("{\"case\":\"limits16\",\"n_vertices\":%zu,%s}\n", S.positions.size() / 3, lds_json(P, false).c_str());
    }
}

static void case_spheres() {
    Scene S; int b = S.add_bsdf(LRT_BSDF_DIELECTRIC); S.add_shape(LRT_SHAPE_SPHERE, b);
    // rotation by 0.7 rad about the normalised axis (1, 2, 3), radius 0.37, centre (1.5, -2.25, 0.75)
    const double ax[3] = { 1 / std::sqrt(14.0), 2 / std::sqrt(14.0), 3 / std::sqrt(14.0) }, c = std::cos(0.7), s = std::sin(0.7), r = 0.37, t[3] = { 1.5, -2.25, 0.75 };
    float *m = S.shapes[0].to_world; memset(m, 0, 64); m[15] = 1.f;
    const double K[3][3] = { { 0, -ax[2], ax[1] }, { ax[2], 0, -ax[0] }, { -ax[1], ax[0], 0 } };      // Rodrigues: c I + (1 - c) a a^T + s [a]x
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) m[4 * i + j] = (float) (r * ((i == j ? c : 0.0) + (1 - c) * ax[i] * ax[j] + s * K[i][j])); m[4 * i + 3] = (float) t[i]; }
    PreparedScene P = prepare_scene(S.desc(), generous());
    const DSphere &o = P.spheres[0];
    printf("{\"case\":\"sphere\",\"to_world\":%s,\"center\":%s,\"radius\":%s,\"lin\":%s,\"to_object\":%s,\"shape\":%u,\"n_spheres\":%u,\"ext\":%d}\n", js(m, 16).c_str(), js(o.center, 3).c_str(), jf(o.radius).c_str(),
           js(o.to_world, 9).c_str(), js(o.to_object, 12).c_str(), o.shape, P.sc.n_spheres, (int) P.ext);
    m[0] = m[4] = m[8] = 0.f;
    try { prepare_scene(S.desc(), generous()); printf("{\"case\":\"sphere_zero\",\"error\":null}\n"); }
    catch (const std::exception &e) { printf("{\"case\":\"sphere_zero\",\"error\":%s}\n", jstr(e.what()).c_str()); }
}

static void bounds_line(const char *name, Scene &S) {
    PreparedScene P = prepare_scene(S.desc(), generous()); const DDistGrid &g = P.sc.grid;
    printf("{\"case\":\"bounds\",\"run\":\"%s\",\"bsphere_c\":%s,\"bsphere_r\":%s,\"grid_enabled\":%d,\"grid_lo\":%s,\"grid_cell\":%s,\"grid_n\":%s,\"abs_margin\":%s}\n", name,
           js(P.sc.env.bsphere_c, 3).c_str(), jf(P.sc.env.bsphere_r).c_str(), g.enabled, js(g.lo, 3).c_str(), jf(g.cell).c_str(), ji(g.n, 3).c_str(), jf(P.grid_abs_margin).c_str());
}
static void case_bounds() {
    { Scene S; bounds_line("empty", S); }
    for (int far = 0; far < 2; ++far) {
        Scene S; S.add_cube(); int m = S.add_medium(LRT_MEDIUM_HOMOGENEOUS, 1.f, 1.f);
        if (far) for (float v : { 10.f, 0.f, 0.f }) S.positions.push_back(v);       // referenced by no face
        S.add_shape(LRT_SHAPE_MESH, S.add_bsdf(LRT_BSDF_DIELECTRIC), m);
        bounds_line(far ? "cube_far_vertex" : "cube", S);
    }
}

static void env_line(const char *name, Scene &S, const PrepOptions &o) {
    PreparedScene P = prepare_scene(S.desc(), o); const DEnv &E = P.sc.env;
    printf("{\"case\":\"envmap\",\"run\":\"%s\",\"w\":%u,\"h\":%u,\"texels\":%s,\"env_data\":%s,\"hier\":%s,\"n_levels\":%d,\"level_offset\":%s,\"level_width\":%s,\"interior_positive\":%d,\"nee_fast_reject\":%d,"
           "\"patch_size\":%s,\"max_patch\":%s}\n", name, E.w, E.h, js(S.env_texels.data(), S.env_texels.size()).c_str(), js(P.env_data.data(), P.env_data.size()).c_str(), js(P.env_hier.data(), P.env_hier.size()).c_str(),
           E.n_levels, ji(E.level_offset, LRT_MAX_HIER_LEVELS).c_str(), ji(E.level_width, LRT_MAX_HIER_LEVELS).c_str(), (int) P.env_interior_positive, P.sc.nee_fast_reject, js(E.patch_size, 2).c_str(), ji(E.max_patch, 2).c_str());
}
static void case_envmap() {
    { Scene S; S.add_envmap(2, 3); env_line("2x3", S, generous()); }
    { Scene S; S.add_envmap(2, 3, 1, 1); env_line("2x3_zero_interior", S, generous()); }
    { Scene S; S.add_envmap(2, 3, 1, 0); env_line("2x3_zero_border", S, generous()); }
    { Scene S; S.add_envmap(5, 4); env_line("5x4", S, generous()); }
    // nee_fast_reject: the base has it, each of the five conditions takes it away
    auto reject = [](const char *name, Scene &S, const PrepOptions &o) { printf("{\"case\":\"nee_fast_reject\",\"run\":\"%s\",\"value\":%d}\n", name, prepare_scene(S.desc(), o).sc.nee_fast_reject); };
    { Scene S; S.add_envmap(2, 3); reject("base_envmap", S, generous()); }
    { Scene S; S.add_emitter(LRT_EMITTER_CONSTANT); reject("base_constant", S, generous()); }
    { Scene S; S.add_envmap(2, 3); S.add_emitter(LRT_EMITTER_POINT); reject("two_emitters", S, generous()); }
    { Scene S; S.add_envmap(2, 3); S.add_bsdf(LRT_BSDF_NULL); reject("null_bsdf", S, generous()); }
    { Scene S; S.add_envmap(2, 3); static const float grid[1] = { 1.f }; int m = S.add_medium(LRT_MEDIUM_HETEROGENEOUS, 1.f, 1.f);
      S.media[m].grid_res[0] = S.media[m].grid_res[1] = S.media[m].grid_res[2] = 1; S.media[m].grid_max = 1.f; S.media[m].grid_data = grid; reject("het_medium", S, generous()); }
    { Scene S; S.add_envmap(2, 3); PrepOptions o = generous(); o.no_nee_reject = true; reject("switch", S, o); }
    { Scene S; S.add_envmap(2, 3, 0, 1); reject("interior_not_positive", S, generous()); }
    { Scene S; S.add_emitter(LRT_EMITTER_POINT); reject("point_only", S, generous()); }
}

static void case_media() {
    const float sig[] = { 0.f, 1e-3f, 0.024f, 0.026f, 0.05f, 0.3f, 1.f, 7.3f, 40.f, 1e4f, INFINITY }; const float radii[] = { 8.9406967e-05f, 0.5f, 1.f, 3.7f };
    for (float r : radii) for (float scale : { 1.f, 0.7f }) {
        Scene S; for (float s : sig) S.add_medium(LRT_MEDIUM_HOMOGENEOUS, s, scale);
        std::vector<DMedium> media; std::vector<DBioMedium> bio; std::vector<DHetMedium> het; prepare_media(S.desc(), r, media, bio, het);
        std::vector<float> st, vmin; for (const DMedium &M : media) { st.push_back(M.sigma_t[0]); vmin.push_back(M.nee_vmin[0]); }
        std::vector<float> same; for (size_t i = 0; i < media.size(); ++i) same.push_back(medium_sigma_t(S.media[i], 0));
        // inf as 1e39 (no JSON spelling): float("1e39") is finite in float64 and reads back as inf in float32
        std::string a = js(st.data(), st.size()), b = js(same.data(), same.size());
        for (std::string *x : { &a, &b }) for (size_t p; (p = x->find("inf")) != std::string::npos;) x->replace(p, 3, "1e39");
        printf("{\"case\":\"nee_vmin\",\"bsphere_r\":%s,\"scale\":%s,\"sigma_t\":%s,\"medium_sigma_t\":%s,\"nee_vmin\":%s,\"sizes\":[%zu,%zu,%zu]}\n", jf(r).c_str(), jf(scale).c_str(), a.c_str(), b.c_str(),
               js(vmin.data(), vmin.size()).c_str(), media.size(), bio.size(), het.size());
    }
}

static void resolve_line(const char *name, Scene &S, const lrt_render_opts *o) {
    try {
        ResolvedOpts r = resolve(S.desc(), o);
        printf("{\"case\":\"resolve\",\"run\":\"%s\",\"error\":null,\"integrator\":%d,\"max_depth\":%d,\"rr_depth\":%d,\"spp\":%u,\"spp_total\":%u,\"n_passes\":%u,\"pass\":%u,\"tile_rank\":%u,\"tile_count\":%u}\n", name,
               r.integrator, r.max_depth, r.rr_depth, r.spp, r.spp_total, r.n_passes, r.pass, r.tile_rank, r.tile_count);
    } catch (const std::exception &e) { printf("{\"case\":\"resolve\",\"run\":\"%s\",\"error\":%s}\n", name, jstr(e.what()).c_str()); }
}
static void case_resolve() {
    const lrt_render_opts none{ -1, -2, -1, -1, 0, 0, 0, 1, 0, 0, 0, 0 };
    for (uint32_t spp : { 1u, 5u, 17u }) { Scene S; S.base.sampler_type = LRT_SAMPLER_LD; lrt_render_opts o = none; o.spp = spp; resolve_line(("ld" + std::to_string(spp)).c_str(), S, &o); }
    { Scene S; S.base.sample_count = 10; S.base.samples_per_pass = 4; resolve_line("not_a_multiple", S, nullptr); }
    { Scene S; S.base.sample_count = 12; S.base.samples_per_pass = 4; resolve_line("three_passes", S, nullptr); }
    { Scene S; S.base.film.crop_width = 65536; S.base.film.crop_height = 32768; S.base.sample_count = 4; resolve_line("wavefront_2e33", S, nullptr); }
    { Scene S; S.base.film.crop_width = 65536; S.base.film.crop_height = 65536; S.base.sample_count = 4; resolve_line("film_2e32", S, nullptr); }
    for (int depth : { -1, 70000, 65535, 12 }) { Scene S; S.base.integrator.max_depth = depth; resolve_line(("depth" + std::to_string(depth)).c_str(), S, nullptr); }
    { Scene S; lrt_render_opts o = none; o.max_depth = -1; resolve_line("opts_depth-1", S, &o); }
    { Scene S; S.base.integrator.type = LRT_INTEGRATOR_PRBVOLPATH; S.base.sample_count = 12; S.base.samples_per_pass = 4; resolve_line("prb", S, nullptr); }
    { Scene S; lrt_render_opts o = none; o.tile_rank = 2; o.tile_count = 2; resolve_line("rank_out_of_range", S, &o); }
    { Scene S; lrt_render_opts o = none; o.tile_rank = 1; o.tile_count = 2; resolve_line("rank1of2", S, &o); }
}

static void case_tiles() {
    struct F { int w, h; uint32_t count; } films[] = { { 33, 5, 2 }, { 9, 5, 2 }, { 70, 37, 3 } };
    for (const F &f : films) for (uint32_t rank = 0; rank < f.count; ++rank) {
        DFilm film{}; film.width = f.w; film.height = f.h;
        TilePixels T = tile_pixel_list(film, rank, f.count);
        printf("{\"case\":\"tiles\",\"w\":%d,\"h\":%d,\"rank\":%u,\"count\":%u,\"list\":%s,\"slot\":%s", f.w, f.h, rank, f.count, ji(T.list.data(), T.list.size()).c_str(), ji(T.slot.data(), T.slot.size()).c_str());
        for (uint32_t halo : { 0u, 2u, 40u }) { std::vector<uint32_t> h = halo_pixel_list(film, rank, f.count, halo); printf(",\"halo%u\":%s", halo, ji(h.data(), h.size()).c_str()); }
        printf("}\n");
    }
}

static void case_closed() {
    // true: one constant emitter, a homogeneous medium inside a dielectric shape and inside a bumpmap over a dielectric, the sensor in no medium
    auto base = [](Scene &S) {
        int m = S.add_medium(LRT_MEDIUM_HOMOGENEOUS, 2.f, 0.5f), di = S.add_bsdf(LRT_BSDF_DIELECTRIC), bump = S.add_bsdf(LRT_BSDF_BUMPMAP, di);
        S.add_shape(LRT_SHAPE_MESH, di, m); S.add_shape(LRT_SHAPE_MESH, bump, m); S.add_emitter(LRT_EMITTER_CONSTANT);
    };
    auto line = [](const char *name, Scene &S) { lrt_scene_desc d = S.desc(); printf("{\"case\":\"closed_records\",\"run\":\"%s\",\"value\":%d}\n", name, (int) closed_records(d, d.sensor.medium)); };
    { Scene S; base(S); line("base", S); }
    { Scene S; base(S); S.emitters[0].type = LRT_EMITTER_ENVMAP; line("base_envmap", S); }
    { Scene S; base(S); S.media[0].type = LRT_MEDIUM_HETEROGENEOUS; line("a_heterogeneous", S); }
    { Scene S; base(S); S.media[0].sigma_t[1] = 0.f; line("a_sigma_t_zero", S); }
    { Scene S; base(S); S.media[0].sigma_t[2] = 1e-30f; line("a_sigma_t_times_scale_small", S); }      // 1e-30 * 0.5 < 1e-30
    { Scene S; base(S); S.media[0].sigma_t[0] = INFINITY; line("a_sigma_t_infinite", S); }
    { Scene S; base(S); S.base.sensor.medium = 0; line("a_sensor_in_medium", S); }
    { Scene S; base(S); S.shapes[1].exterior_medium = 0; line("a_exterior_medium", S); }
    { Scene S; base(S); S.bsdfs[0].type = LRT_BSDF_DIFFUSE; line("b_diffuse", S); }
    { Scene S; base(S); S.bsdfs[0].type = LRT_BSDF_NULL; line("b_null", S); }
    { Scene S; base(S); S.shapes[0].bsdf = -1; line("b_no_bsdf", S); }
    { Scene S; base(S); S.bsdfs[1].nested = S.add_bsdf(LRT_BSDF_DIFFUSE); line("b_bumpmap_over_diffuse", S); }
    { Scene S; base(S); S.bsdfs[1].nested = 7; line("b_bumpmap_nested_out_of_range", S); }
    { Scene S; base(S); S.emitters[0].type = LRT_EMITTER_AREA; line("c_area_emitter", S); }
    { Scene S; base(S); S.emitters[0].type = LRT_EMITTER_POINT; line("c_point_emitter", S); }
    { Scene S; base(S); S.add_emitter(LRT_EMITTER_CONSTANT); line("c_two_emitters", S); }
    { Scene S; base(S); S.emitters.clear(); line("c_no_emitter", S); }
}

// PrepOptions::from_env: the five switches as the environment spells them
static void case_from_env() {
    static const char *names[] = { "LRT_BVH_LEAF", "LRT_NO_LDS_BVH", "LRT_NO_DIST_GRID", "LRT_DIST_GRID_RES", "LRT_NO_NEE_REJECT" };
    struct Env { const char *run; const char *value[5]; } envs[] = {
        { "unset", { nullptr, nullptr, nullptr, nullptr, nullptr } }, { "leaf6_res100", { "6", nullptr, nullptr, "100", nullptr } },
        { "leaf0_res4", { "0", nullptr, nullptr, "4", nullptr } }, { "leaf_negative_res1000", { "-3", nullptr, nullptr, "1000", nullptr } },
        { "leaf_text_res_text", { "abc", nullptr, nullptr, "abc", nullptr } }, { "flags", { nullptr, "1", "1", nullptr, "1" } },
        { "flags_zero_and_empty", { nullptr, "0", "", nullptr, "0" } } };
    for (const Env &e : envs) {
        for (int i = 0; i < 5; ++i) { if (e.value[i]) setenv(names[i], e.value[i], 1); else unsetenv(names[i]); }
        PrepOptions o = PrepOptions::from_env();
        printf("{\"case\":\"from_env\",\"run\":\"%s\",\"bvh_leaf\":%d,\"no_lds_bvh\":%d,\"no_dist_grid\":%d,\"dist_grid_res\":%d,\"no_nee_reject\":%d,\"lds_limit\":%zu,\"n_cus\":%d}\n", e.run,
               o.bvh_leaf, (int) o.no_lds_bvh, (int) o.no_dist_grid, o.dist_grid_res, (int) o.no_nee_reject, o.lds_limit, o.n_cus);
    }
    for (const char *n : names) unsetenv(n);
}

// `scene_prep_main grid-fit K0 K1`: does the LDS image of the K x K quad grid (2 K^2 triangles) fit the real limit, 160 KiB - 512?
// (tests/test_scene_upload_gpu.py takes its two face counts from this.)
static void grid_fit(uint32_t k0, uint32_t k1) {
    for (uint32_t k = k0; k <= k1; ++k) {
        Scene S; S.add_grid(2 * k * k); S.add_shape(LRT_SHAPE_MESH, S.add_bsdf(LRT_BSDF_DIELECTRIC));
        PrepOptions o; o.lds_limit = 160 * 1024 - 512;
        PreparedScene P = prepare_scene(S.desc(), o);
        printf("{\"case\":\"grid_fit\",\"k\":%u,\"n_vertices\":%zu,%s}\n", k, S.positions.size() / 3, lds_json(P, false).c_str());
    }
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "grid-fit")) { grid_fit((uint32_t) atoi(argv[2]), (uint32_t) atoi(argv[3])); return 0; }
    case_triangle(); case_grid("grid", 64); case_grid("row", 96); case_limits16(); case_spheres(); case_bounds(); case_envmap(); case_media(); case_resolve(); case_tiles(); case_closed(); case_from_env();
    return 0;
}
