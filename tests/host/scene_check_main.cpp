// Stand-alone driver of the scene checks (liverrenderer_amd/csrc/scene_check.cpp) for tests/test_scene_check.py: one JSON line per case.
// It asserts nothing itself; the sanitizers it is built with watch what the checks read.  `scene_check_main DIR`: a directory for the one file it writes.
//   prepare:  the refusals of prepare_scene that a render can still reach, each by the path that reaches it: the XML loader's
//             output, or a description built by hand and copied by SceneStorage::copy_from as lrt_scene_from_desc copies it.
//   features: scene_features and the preparation's ext / smooth_bsdf on tiny descriptions.
//   index:    validate_scene_desc on descriptions with one index field out of range.
// -DSCENE_CHECK_PREPARE_ONLY leaves out what needs scene_check.h: the `prepare` lines then build against any tree that has scene_prep.h.
#include "scene_prep.h"
#ifndef SCENE_CHECK_PREPARE_ONLY
#include "scene_check.h"
#endif
#include <cstdio>
#include <cstring>
#include <cmath>
#include <functional>
#include <string>
#include <stdexcept>

using namespace lrt;

static std::string jstr(const std::string &s) { std::string r = "\""; for (char c : s) { if (c == '"' || c == '\\') r += '\\'; r += c; } return r + "\""; }

// ---- a scene description that owns its arrays: one triangle, an 8 x 8 film, and what a case adds
struct Scene {
    std::vector<float> positions{ 0, 0, 0, 1, 0, 0, 0, 1, 0 }, normals{ 0, 0, 1, 0, 0, 1, 0, 0, 1 }, texcoords{ 0, 0, 1, 0, 0, 1 }, grid{ 1, 2, 3, 4, 5, 6, 7, 8 }, tab{ 1, 2, 3 };
    std::vector<uint32_t> faces{ 0, 1, 2 }, face_shape{ 0 };
    std::vector<lrt_shape_desc> shapes; std::vector<lrt_bsdf_desc> bsdfs; std::vector<lrt_texture_desc> textures;
    std::vector<lrt_medium_desc> media; std::vector<lrt_emitter_desc> emitters; std::vector<lrt_phase_desc> phases;
    lrt_scene_desc base{};
    Scene() {
        base.sensor.fov_x = 40.f; base.sensor.near_clip = 0.01f; base.sensor.far_clip = 100.f; base.sensor.medium = -1;
        for (int i = 0; i < 4; ++i) base.sensor.to_world[5 * i] = 1.f;
        base.film.width = base.film.crop_width = base.film.height = base.film.crop_height = 8;
        base.integrator.type = LRT_INTEGRATOR_VOLPATH; base.integrator.max_depth = 8; base.integrator.rr_depth = 5;
        base.sample_count = 4; base.use_spectral_mis = 1;
        add_texture(LRT_TEX_RGB);
        add_shape(LRT_SHAPE_MESH, add_bsdf(LRT_BSDF_DIFFUSE)); shapes[0].n_faces = 1;
        add_emitter(LRT_EMITTER_CONSTANT);
    }
    lrt_scene_desc desc() {
        lrt_scene_desc d = base;
        d.n_vertices = (uint32_t) (positions.size() / 3); d.n_faces = (uint32_t) (faces.size() / 3); d.n_shapes = (uint32_t) shapes.size(); d.n_bsdfs = (uint32_t) bsdfs.size();
        d.n_textures = (uint32_t) textures.size(); d.n_media = (uint32_t) media.size(); d.n_emitters = (uint32_t) emitters.size(); d.n_phases = (uint32_t) phases.size();
        d.positions = positions.data(); d.normals = normals.data(); d.texcoords = texcoords.data(); d.faces = faces.data(); d.face_shape = face_shape.data();
        d.shapes = shapes.data(); d.bsdfs = bsdfs.data(); d.textures = textures.data(); d.media = media.data(); d.emitters = emitters.data(); d.phases = phases.empty() ? nullptr : phases.data();
        return d;
    }
    int add_texture(int type) { lrt_texture_desc t{}; t.type = type; for (int k = 0; k < 3; ++k) { t.color0[k] = .5f; t.color1[k] = .25f; } t.to_uv[0] = t.to_uv[4] = t.to_uv[8] = 1.f; textures.push_back(t); return (int) textures.size() - 1; }
    int add_bsdf(int type, int nested = -1) {
        lrt_bsdf_desc b{}; b.type = type; b.nested = nested; b.nested_back = -1; b.texture = type == LRT_BSDF_BUMPMAP ? 0 : -1; b.eta = 1.5f; b.scale = 1.f; b.alpha_u = b.alpha_v = .1f;
        b.reflectance = type == LRT_BSDF_DIFFUSE ? 0 : -1; b.specular_transmittance = -1; b.specular_reflectance = type == LRT_BSDF_CONDUCTOR ? 0 : -1; b.diffuse_reflectance = type == LRT_BSDF_PLASTIC ? 0 : -1;
        for (int k = 0; k < 3; ++k) b.k_rgb[k] = 1.f;
        bsdfs.push_back(b); return (int) bsdfs.size() - 1;
    }
    int add_shape(int kind, int bsdf) {
        lrt_shape_desc s{}; s.kind = kind; s.bsdf = bsdf; s.emitter = s.interior_medium = s.exterior_medium = -1;
        for (int i = 0; i < 4; ++i) s.to_world[5 * i] = 1.f;
        shapes.push_back(s); return (int) shapes.size() - 1;
    }
    int add_emitter(int type, int shape = -1) {
        lrt_emitter_desc e{}; e.type = type; e.shape = shape; e.scale = 1.f; e.texture = -1; e.cutoff_angle = 20.f; e.beam_width = 15.f;
        for (int k = 0; k < 3; ++k) e.radiance[k] = 1.f;
        for (int i = 0; i < 4; ++i) e.to_world[5 * i] = 1.f;
        emitters.push_back(e); if (shape >= 0) shapes[shape].emitter = (int) emitters.size() - 1; return (int) emitters.size() - 1;
    }
    int add_medium(int type = LRT_MEDIUM_HOMOGENEOUS) {
        lrt_medium_desc m{}; m.type = type; m.scale = 1.f; m.phase_index = -1; for (int k = 0; k < 3; ++k) { m.sigma_t[k] = 1.f; m.albedo[k] = .5f; }
        if (type == LRT_MEDIUM_HETEROGENEOUS) {
            m.grid_res[0] = m.grid_res[1] = m.grid_res[2] = 2; m.grid_max = 8.f; m.grid_data = grid.data();
            m.grid_to_local[0] = m.grid_to_local[5] = m.grid_to_local[10] = 1.f; for (int k = 0; k < 3; ++k) m.grid_bbox_max[k] = 1.f;
        }
        media.push_back(m); return (int) media.size() - 1;
    }
    int add_phase(int type, int c0 = -1, int c1 = -1) {
        lrt_phase_desc q{}; q.type = type; q.g = .5f; q.weight = .5f; q.child[0] = c0; q.child[1] = c1;
        if (type == LRT_PHASE_TABULATED) { q.values = tab.data(); q.n_values = (uint32_t) tab.size(); }
        phases.push_back(q); return (int) phases.size() - 1;
    }
    void set_sphere(int shape, float radius) { lrt_shape_desc &s = shapes[shape]; s.kind = LRT_SHAPE_SPHERE; s.first_face = s.n_faces = 0; s.to_world[0] = s.to_world[5] = s.to_world[10] = radius; }
};

static PrepOptions generous() { PrepOptions o; o.lds_limit = (size_t) 1 << 30; return o; }

// ---- prepare
static void prepare_line(const char *run, const std::function<void(SceneStorage &)> &make) {
    std::string error = "null";
    try { SceneStorage st; make(st); prepare_scene(st.desc, generous()); }
    catch (const std::exception &e) { error = jstr(e.what()); }
    printf("{\"case\":\"prepare\",\"run\":\"%s\",\"error\":%s}\n", run, error.c_str());
}
static void from_xml(const char *run, const std::string &body, const std::string &dir) {
    const std::string xml = "<scene version=\"3.0.0\"><integrator type=\"volpath\"/><sensor type=\"perspective\"><film type=\"hdrfilm\"><integer name=\"width\" value=\"8\"/>"
                            "<integer name=\"height\" value=\"8\"/><rfilter type=\"box\"/></film></sensor><emitter type=\"constant\"/>" + body + "</scene>";
    prepare_line(run, [&](SceneStorage &st) { load_scene_xml(xml, dir, {}, st); });
}
static void from_desc(const char *run, Scene &S) { prepare_line(run, [&](SceneStorage &st) { st.copy_from(S.desc()); }); }

static void case_prepare(const std::string &dir) {
    from_xml("xml fine", "<shape type=\"cube\"/>", dir);
    { Scene S; from_desc("desc fine", S); }
    from_xml("xml sphere radius 0", "<shape type=\"sphere\"><float name=\"radius\" value=\"0\"/></shape>", dir);
    { Scene S; S.set_sphere(S.add_shape(LRT_SHAPE_MESH, 0), 0.f); from_desc("desc sphere radius 0", S); }
    { Scene S; S.set_sphere(S.add_shape(LRT_SHAPE_MESH, 0), NAN); from_desc("desc sphere radius nan", S); }
    {   // a version-3 volume file, 2 x 2 x 2 zeros
        const std::string path = dir + "/zeros.vol";
        FILE *f = fopen(path.c_str(), "wb");
        const int32_t meta[5] = { 1, 2, 2, 2, 1 }; const float box[6] = { 0, 0, 0, 1, 1, 1 }, data[8] = {};
        if (f) { fwrite("VOL\3", 1, 4, f); fwrite(meta, 4, 5, f); fwrite(box, 4, 6, f); fwrite(data, 4, 8, f); fclose(f); }
        from_xml("xml grid of zeros", "<shape type=\"cube\"><bsdf type=\"null\"/><medium name=\"interior\" type=\"heterogeneous\"><volume name=\"sigma_t\" type=\"gridvolume\">"
                                      "<string name=\"filename\" value=\"" + path + "\"/></volume></medium></shape>", dir);
    }
    { Scene S; S.media[S.add_medium(LRT_MEDIUM_HETEROGENEOUS)].grid_max = 0.f; S.shapes[0].interior_medium = 0; from_desc("desc grid_max 0", S); }
    { std::string media; for (int i = 0; i < 65; ++i) media += "<medium type=\"homogeneous\" id=\"m" + std::to_string(i) + "\"/>"; from_xml("xml 65 media", media + "<shape type=\"cube\"/>", dir); }
    { Scene S; for (int i = 0; i < 65; ++i) S.add_medium(); from_desc("desc 65 media", S); }
    {   // 16385 texels a row (as many patches: the map is stored with its first column repeated) need a 17th level of the sampling hierarchy; 16384 do not
        for (int w : { 16384, 16385 }) {
            Scene S; std::vector<float> texels((size_t) w * 3 * 3, 1.f);
            S.emitters[0].type = LRT_EMITTER_ENVMAP; S.emitters[0].width = w; S.emitters[0].height = 3; S.emitters[0].data = texels.data();
            from_desc(w == 16384 ? "desc envmap 16384 wide" : "desc envmap 16385 wide", S);
        }
    }
    // the loader refuses a negative index of refraction, the preparation a relative index that is not positive
    from_xml("xml plastic int_ior 0", "<shape type=\"cube\"><bsdf type=\"plastic\"><float name=\"int_ior\" value=\"0\"/></bsdf></shape>", dir);
}

#ifndef SCENE_CHECK_PREPARE_ONLY
// ---- features
static void features_line(const char *run, Scene &S, bool prepare = true) {
    const lrt_scene_desc d = S.desc();
    const SceneFeatures F = scene_features(d);
    int ext = -1, smooth = -1;
    if (prepare) { PreparedScene P = prepare_scene(d, generous()); ext = P.ext; smooth = P.smooth_bsdf; }
    printf("{\"case\":\"features\",\"run\":\"%s\",\"sphere\":%d,\"point_emitter\":%d,\"delta_emitter\":%d,\"mesh_emitter\":%d,\"rough_bsdf\":%d,\"smooth_bsdf\":%d,\"phase_entry\":%d,\"any\":%d,\"prepared\":%d,\"ext\":%d,\"smooth\":%d}\n",
           run, F.sphere, F.point_emitter, F.delta_emitter, F.mesh_emitter, F.rough_bsdf, F.smooth_bsdf, F.phase_entry, F.any(), (int) prepare, ext, smooth);
}
static int add_smooth(Scene &S, int type) { return type == LRT_BSDF_TWOSIDED ? S.add_bsdf(type, 0) : S.add_bsdf(type); }      // (a twosided over the diffuse BSDF 0)

static void case_features() {
    { Scene S; features_line("base", S); }
    { Scene S; S.set_sphere(0, 1.f); S.faces.clear(); S.face_shape.clear(); features_line("sphere", S); }
    { Scene S; S.emitters[0].type = LRT_EMITTER_POINT; features_line("point", S); }
    { Scene S; S.emitters[0].type = LRT_EMITTER_SPOT; features_line("spot", S); }
    { Scene S; S.emitters[0].type = LRT_EMITTER_DIRECTIONAL; features_line("directional", S); }
    { Scene S; S.emitters.clear(); S.add_emitter(LRT_EMITTER_AREA, 0); features_line("mesh emitter", S); }
    { Scene S; S.emitters.clear(); S.add_emitter(LRT_EMITTER_AREA, 0); S.shapes[0].kind = LRT_SHAPE_RECTANGLE; features_line("rectangle emitter", S); }
    struct B { int type; const char *name; } kinds[] = { { LRT_BSDF_ROUGHDIELECTRIC, "roughdielectric" }, { LRT_BSDF_CONDUCTOR, "conductor" }, { LRT_BSDF_PLASTIC, "plastic" }, { LRT_BSDF_TWOSIDED, "twosided" } };
    for (const B &k : kinds) {
        { Scene S; S.shapes[0].bsdf = add_smooth(S, k.type); features_line(k.name, S); }
        // (a bumpmap over a twosided is refused by check_bsdf and by the loader; the feature table still names what it finds)
        { Scene S; S.shapes[0].bsdf = S.add_bsdf(LRT_BSDF_BUMPMAP, add_smooth(S, k.type)); features_line((std::string("bumpmap over ") + k.name).c_str(), S, k.type != LRT_BSDF_TWOSIDED); }
        { Scene S; add_smooth(S, k.type); features_line((std::string(k.name) + " unreferenced").c_str(), S); }
    }
    auto with_entry = [](Scene &S, int medium) { S.add_phase(LRT_PHASE_RAYLEIGH); S.media[medium].phase_index = 0; };
    { Scene S; S.shapes[0].interior_medium = S.add_medium(); with_entry(S, 0); features_line("phase entry on the interior", S); }
    { Scene S; S.shapes[0].exterior_medium = S.add_medium(); with_entry(S, 0); features_line("phase entry on the exterior", S); }
    { Scene S; S.base.sensor.medium = S.add_medium(); with_entry(S, 0); features_line("phase entry on the sensor only", S); }
    { Scene S; S.shapes[0].interior_medium = S.add_medium(); with_entry(S, S.add_medium()); features_line("phase entry unreferenced", S); }
    { Scene S; S.shapes[0].interior_medium = S.add_medium(); S.media[0].phase_index = 3; features_line("phase index without a table", S); }
    // indices out of range: flags, no fault (no preparation: it follows validated indices only)
    { Scene S; S.emitters[0].type = LRT_EMITTER_AREA; S.emitters[0].shape = 7; features_line("area emitter shape out of range", S, false); }
    { Scene S; S.emitters[0].type = LRT_EMITTER_AREA; S.emitters[0].shape = -3; features_line("area emitter shape negative", S, false); }
    { Scene S; S.shapes[0].bsdf = 1 << 30; features_line("shape bsdf out of range", S, false); }
    { Scene S; S.shapes[0].bsdf = S.add_bsdf(LRT_BSDF_BUMPMAP, -(1 << 30)); features_line("bumpmap nested out of range", S, false); }
    { Scene S; S.add_medium(); S.add_phase(LRT_PHASE_RAYLEIGH); S.media[0].phase_index = 0; S.shapes[0].interior_medium = 1; S.shapes[0].exterior_medium = -2; S.base.sensor.medium = 1 << 30; features_line("medium indices out of range", S, false); }
    { Scene S; S.set_sphere(S.add_shape(LRT_SHAPE_MESH, S.add_bsdf(LRT_BSDF_PLASTIC)), 1.f); S.emitters[0].type = LRT_EMITTER_SPOT; features_line("sphere and spot and plastic", S); }
}

// ---- index: every index field of the description below and above its range
static void index_line(const char *field, const std::function<void(Scene &, int32_t)> &set) {
    for (int32_t v : { -(1 << 30), 1 << 30 }) {
        Scene S;
        S.add_texture(LRT_TEX_CHECKERBOARD);
        const int di = 0, bump = S.add_bsdf(LRT_BSDF_BUMPMAP, di), rough = S.add_bsdf(LRT_BSDF_ROUGHDIELECTRIC), cond = S.add_bsdf(LRT_BSDF_CONDUCTOR), pla = S.add_bsdf(LRT_BSDF_PLASTIC), two = S.add_bsdf(LRT_BSDF_TWOSIDED, di);
        (void) bump; (void) rough; (void) cond; (void) pla; (void) two;
        S.add_medium(); S.add_medium(); S.add_medium(LRT_MEDIUM_HETEROGENEOUS); S.add_phase(LRT_PHASE_RAYLEIGH); S.add_phase(LRT_PHASE_HG); S.add_phase(LRT_PHASE_BLEND, 0, 1); S.add_phase(LRT_PHASE_TABULATED);
        S.media[1].phase_index = 2; S.media[2].phase_index = 3; S.base.film.rfilter = LRT_RFILTER_GAUSSIAN; S.base.film.rfilter_param = .5f;
        S.shapes[0].interior_medium = 0; S.shapes[0].exterior_medium = 1;
        S.add_emitter(LRT_EMITTER_AREA, 0); S.add_emitter(LRT_EMITTER_SPOT); S.emitters[2].texture = 1;
        set(S, v);
        std::string error = "null";
        try { validate_scene_desc(S.desc()); } catch (const std::exception &e) { error = jstr(e.what()); }
        printf("{\"case\":\"index\",\"field\":\"%s\",\"value\":%d,\"error\":%s}\n", field, v, error.c_str());
    }
}
static void case_index() {
    index_line("none", [](Scene &, int32_t) {});                    // the scene the others edit: accepted
    index_line("faces", [](Scene &S, int32_t v) { S.faces[1] = (uint32_t) v; });
    index_line("face_shape", [](Scene &S, int32_t v) { S.face_shape[0] = (uint32_t) v; });
    index_line("diffuse.reflectance", [](Scene &S, int32_t v) { S.bsdfs[0].reflectance = v; });
    index_line("bumpmap.nested", [](Scene &S, int32_t v) { S.bsdfs[1].nested = v; });
    index_line("bumpmap.texture", [](Scene &S, int32_t v) { S.bsdfs[1].texture = v; });
    index_line("roughdielectric.specular_reflectance", [](Scene &S, int32_t v) { S.bsdfs[2].specular_reflectance = v; });
    index_line("roughdielectric.specular_transmittance", [](Scene &S, int32_t v) { S.bsdfs[2].specular_transmittance = v; });
    index_line("conductor.specular_reflectance", [](Scene &S, int32_t v) { S.bsdfs[3].specular_reflectance = v; });
    index_line("plastic.diffuse_reflectance", [](Scene &S, int32_t v) { S.bsdfs[4].diffuse_reflectance = v; });
    index_line("plastic.specular_reflectance", [](Scene &S, int32_t v) { S.bsdfs[4].specular_reflectance = v; });
    index_line("twosided.nested", [](Scene &S, int32_t v) { S.bsdfs[5].nested = v; });
    index_line("twosided.nested_back", [](Scene &S, int32_t v) { S.bsdfs[5].nested_back = v > 0 ? v : 0x7fffffff; });      // (negative: one child, no index)
    index_line("shape.bsdf", [](Scene &S, int32_t v) { S.shapes[0].bsdf = v; });
    index_line("shape.emitter", [](Scene &S, int32_t v) { S.shapes[0].emitter = v; });
    index_line("shape.interior_medium", [](Scene &S, int32_t v) { S.shapes[0].interior_medium = v; });
    index_line("shape.exterior_medium", [](Scene &S, int32_t v) { S.shapes[0].exterior_medium = v; });
    index_line("shape.first_face", [](Scene &S, int32_t v) { S.shapes[0].first_face = (uint32_t) v; });
    index_line("shape.n_faces", [](Scene &S, int32_t v) { S.shapes[0].n_faces = (uint32_t) v; });
    index_line("emitter.shape", [](Scene &S, int32_t v) { S.emitters[1].shape = v; S.shapes[0].emitter = -1; });
    index_line("spot.texture", [](Scene &S, int32_t v) { S.emitters[2].texture = v; });
    index_line("sensor.medium", [](Scene &S, int32_t v) { S.base.sensor.medium = v; });
    index_line("medium.phase_index", [](Scene &S, int32_t v) { S.media[1].phase_index = v; });
    index_line("blend.child0", [](Scene &S, int32_t v) { S.phases[2].child[0] = v; });
    index_line("blend.child1", [](Scene &S, int32_t v) { S.phases[2].child[1] = v; });
}
#endif

int main(int argc, char **argv) {
    case_prepare(argc > 1 ? argv[1] : ".");
#ifndef SCENE_CHECK_PREPARE_ONLY
    case_features(); case_index();
#endif
    return 0;
}
