// Host-side scene object behind the C ABI (include/liverrt.h).
#pragma once
#include "../../include/liverrt.h"
#include <string>
#include <vector>
#include <memory>

namespace lrt {

struct DeviceScene;   // device-resident data + wavefront workspace (device.hip)
struct MultiContext;  // RCCL communicators of a device list (device.hip)

// Owns every array the POD description points into.
struct SceneStorage {
    std::vector<float> positions, normals, texcoords;
    std::vector<uint32_t> faces, face_shape;
    std::vector<lrt_shape_desc> shapes;
    std::vector<lrt_bsdf_desc> bsdfs;
    std::vector<lrt_texture_desc> textures;
    std::vector<std::vector<float>> texdata;
    std::vector<lrt_medium_desc> media;
    std::vector<lrt_emitter_desc> emitters;
    std::vector<std::vector<float>> emdata;
    std::vector<std::vector<float>> meddata;   // heterogeneous media: grid values
    std::vector<lrt_phase_desc> phases;        // the phase-function table
    std::vector<std::vector<float>> phasedata; // tabulated entries: their values
    lrt_scene_desc desc{};
    // `aov` integrator (loader.cpp): its configuration and the developed channel names, beside the ordinary description
    bool has_aov = false;
    lrt_aov_desc aov{};
    std::vector<std::string> aov_channel_names;
    // `moment` integrator (loader.cpp): the nested integrator and the developed channel names
    bool has_moment = false;
    lrt_moment_desc moment{};
    std::vector<std::string> moment_channel_names;
    void fix_pointers();                 // re-point desc at the vectors above
    void copy_from(const lrt_scene_desc &d);
};

// Sampling table of an area emitter on a triangle mesh (loader.cpp): face areas .5 |(p1 - p0) x (p2 - p0)| in float32
// (src/render/mesh.cpp:449-482 build_pmf) and their inclusive prefix sum, summed left to right in float32
// (include/mitsuba/core/distr_1d.h:219-234 compute_cdf).  `positions` / `faces`: the scene's arrays (faces hold vertex indices).
// Throws for a mesh without faces, and for one whose total area is zero (named `name` in the message).
struct MeshEmitterTable { std::vector<float> pmf, cdf; float sum = 0.f, normalization = 0.f; };
void mesh_emitter_table(const float *positions, const uint32_t *faces, uint32_t first_face, uint32_t n_faces, const std::string &name, MeshEmitterTable &out);

// XML -> storage (loader.cpp).  Throws std::runtime_error.
void load_scene_xml(const std::string &xml_text, const std::string &base_dir,
                    const std::vector<std::pair<std::string, std::string>> &defines, SceneStorage &out);

} // namespace lrt

struct lrt_scene {
    lrt::SceneStorage st;
    lrt::DeviceScene *dev = nullptr;     // created lazily on first device call
    bool params_dirty = true;
    bool grids_dirty = false, multi_grids_dirty = false;   // lrt_param_set("<id>.sigma_t.data"): the next update uploads the grids again
    int dev_ordinal = -1;                  // HIP device the device image lives on
    lrt_render_stats stats{};
    // lrt_render_multi: one device image per entry of the last device list, and that list's communicators
    std::vector<lrt::DeviceScene *> multi; std::vector<int> multi_ids; lrt::MultiContext *multi_ctx = nullptr; bool multi_params_dirty = false;
};
