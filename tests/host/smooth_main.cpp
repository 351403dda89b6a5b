// Stand-alone driver of the host-only scene preparation for tests/test_smooth.py: loads the scene files named on the command line,
// prepares each (liverrenderer_amd/csrc/scene_prep.cpp) and prints one JSON line per file: the BSDF table with its flags, the rows of
// DScene::bsdf_ext (conductor / plastic / twosided) and the routing flags.  A scene the loader or the preparation refuses prints its
// message.  It asserts nothing itself.
#include "scene_prep.h"
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <stdexcept>

using namespace lrt;

static std::string jf(float v) { char b[40]; snprintf(b, sizeof b, "%.9g", (double) v); return b; }
static std::string j3(const float *v) { return "[" + jf(v[0]) + "," + jf(v[1]) + "," + jf(v[2]) + "]"; }
static std::string jstr(const std::string &s) { std::string r = "\""; for (char c : s) { if (c == '"' || c == '\\') r += '\\'; if (c == '\n') { r += "\\n"; continue; } r += c; } return r + "\""; }

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        std::string line = "{\"file\":" + jstr(argv[a]);
        try {
            std::ifstream f(argv[a]); if (!f) throw std::runtime_error("cannot open the scene file");
            std::stringstream ss; ss << f.rdbuf();
            SceneStorage S; load_scene_xml(ss.str(), ".", {}, S);
            PreparedScene P = prepare_scene(S.desc, PrepOptions{});
            line += ",\"ext\":" + std::to_string((int) P.ext) + ",\"smooth\":" + std::to_string((int) P.smooth_bsdf) + ",\"row_bytes\":" + std::to_string(sizeof(DBsdfExt)) + ",\"bsdfs\":[";
            for (size_t i = 0; i < P.bsdfs.size(); ++i) {
                const DBsdf &B = P.bsdfs[i];
                line += std::string(i ? "," : "") + "{\"type\":" + std::to_string(B.type) + ",\"flags\":" + std::to_string(B.flags) + ",\"reflectance\":" + std::to_string(B.reflectance)
                      + ",\"nested\":" + std::to_string(B.nested) + ",\"eta\":" + jf(B.eta) + "}";
            }
            line += "],\"rows\":[";
            for (size_t i = 0; i < P.bsdf_ext.size(); ++i) {
                const DBsdfExt &X = P.bsdf_ext[i];
                line += std::string(i ? "," : "") + "{\"eta\":" + j3(X.eta) + ",\"k\":" + j3(X.k) + ",\"inv_eta_2\":" + jf(X.inv_eta_2) + ",\"fdr_int\":" + jf(X.fdr_int) + ",\"fdr_ext\":" + jf(X.fdr_ext)
                      + ",\"spec_weight\":" + jf(X.spec_weight) + ",\"nonlinear\":" + std::to_string(X.nonlinear) + ",\"specular_reflectance\":" + std::to_string(X.specular_reflectance)
                      + ",\"back\":" + std::to_string(X.back) + "}";
            }
            line += "]";
        } catch (const std::exception &e) { line += ",\"error\":" + jstr(e.what()); }
        puts((line + "}").c_str());
    }
    return 0;
}
