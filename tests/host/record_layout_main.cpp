// Stand-alone driver of liverrenderer_amd/csrc/record_layout.h for tests/test_record_layout.py: prints the layout table as JSON lines
// (one per record form that exists, per PRB form, per workspace case, per kernel selector).  It asserts nothing itself.
#include "record_layout.h"
#include <cstdio>
#include <string>

using namespace lrt;

static const char *layout_name(RecordLayout l) {
    static const char *names[] = { "wide", "bio", "het", "mis", "closed" };
    return names[(int) l];
}
static std::string streams(RecordLayout l, bool compact, bool prb) {
    std::string s = "[";
    for (const RecordStream &r : kRecordStreams) if (record_uses(r, l, compact, prb)) s += std::string(s.size() > 1 ? "," : "") + "[\"" + r.name + "\"," + std::to_string(r.bytes) + "]";
    return s + "]";
}

int main() {
    for (const RecordForm &f : kRecordForms)
        printf("{\"case\":\"form\",\"name\":\"%s\",\"layout\":\"%s\",\"compact\":%d,\"bytes\":%u,\"streams\":%s}\n", f.name, layout_name(f.layout), (int) f.compact,
               record_bytes(f.layout, f.compact), streams(f.layout, f.compact, false).c_str());
    for (RecordLayout l : { RecordLayout::Wide, RecordLayout::Het })
        printf("{\"case\":\"prb\",\"layout\":\"%s\",\"bytes\":%u,\"streams\":%s}\n", layout_name(l), record_bytes(l, false, true), streams(l, false, true).c_str());
    for (int c = 0; c < 3; ++c) {                                    // any scene; with a heterogeneous medium; after volpathmis was asked for
        const uint32_t layouts = workspace_layouts(c == 1, c == 2);
        std::string s = "["; uint32_t total = 0;
        for (size_t k = 0; k < sizeof(kRecordStreams) / sizeof(kRecordStreams[0]); ++k) if (const uint32_t b = workspace_stream_bytes(k, layouts)) {
            s += std::string(s.size() > 1 ? "," : "") + "[\"" + kRecordStreams[k].name + "\"," + std::to_string(b) + "]"; total += b;
        }
        printf("{\"case\":\"workspace\",\"has_het\":%d,\"mis\":%d,\"bytes\":%u,\"streams\":%s]}\n", (int) (c == 1), (int) (c == 2), total, s.c_str());
    }
    const struct { const char *name; int value; } selectors[] = {
        { "LRT_INTEGRATOR_PATH", LRT_INTEGRATOR_PATH }, { "LRT_INTEGRATOR_VOLPATH", LRT_INTEGRATOR_VOLPATH }, { "LRT_INTEGRATOR_PRBVOLPATH", LRT_INTEGRATOR_PRBVOLPATH },
        { "LRT_INTEGRATOR_BIOVOLPATH", LRT_INTEGRATOR_BIOVOLPATH }, { "LRT_INTEGRATOR_BIOVOLPATH06", LRT_INTEGRATOR_BIOVOLPATH06 }, { "LRT_INTEGRATOR_VOLPATHMIS", LRT_INTEGRATOR_VOLPATHMIS },
        { "LRT_INTEGRATOR_VOLPATH_HET", LRT_INTEGRATOR_VOLPATH_HET }, { "LRT_INTEGRATOR_VOLPATHMIS_PLAIN", LRT_INTEGRATOR_VOLPATHMIS_PLAIN }, { "LRT_INTEGRATOR_VOLPATH_CLOSED", LRT_INTEGRATOR_VOLPATH_CLOSED },
    };
    for (const auto &s : selectors) printf("{\"case\":\"selector\",\"name\":\"%s\",\"value\":%d,\"layout\":\"%s\"}\n", s.name, s.value, layout_name(record_layout(s.value)));
    return 0;
}
