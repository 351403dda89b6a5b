// The path-record layouts, stated once: which streams of DPathStreams a queued path occupies under each layout, and so the bytes a record moves each
// way.  The kernels' load and store (record.h), the host's workspace (device.hip, ensure_workspace) and lrt_render_stats::record_bytes all read the
// table below.  Plain C++17, no HIP call (tests/host/record_layout_main.cpp prints it).  A new layout touches: a row or a mask of kRecordStreams, a
// line of kRecordForms and its byte static_assert, its branch in load_state / store_state (record.h), its add_row in the kernel table (device.hip).
#pragma once
#include <cstddef>
#include <cstdint>
#include "device_types.h"
#include "../../include/liverrt.h"

namespace lrt {

// Wide: path / volpath / prbvolpath.  Bio: biovolpath*, + tissueDepth and the look-ahead's element competition.  Het: volpath / prbvolpath with
// heterogeneous media, + the surface hit a null collision keeps.  Mis: volpathmis, + the hit and the 18 MIS weights.  Closed: volpath where only a
// path's last trip adds radiance: no radiance, no last-scatter pdf.  (Why each exists: DESIGN.md section 3; what rides in which slot: record.h.)
enum class RecordLayout : int { Wide, Bio, Het, Mis, Closed };
constexpr uint32_t layout_bit(RecordLayout l) { return 1u << (int) l; }

// kernel selector (an LRT_INTEGRATOR_* value of the API or of device_types.h) -> the layout its kernels queue
constexpr RecordLayout record_layout(int selector) {
    return selector == LRT_INTEGRATOR_BIOVOLPATH || selector == LRT_INTEGRATOR_BIOVOLPATH06 ? RecordLayout::Bio
         : selector == LRT_INTEGRATOR_VOLPATH_HET ? RecordLayout::Het
         : selector == LRT_INTEGRATOR_VOLPATHMIS || selector == LRT_INTEGRATOR_VOLPATHMIS_PLAIN ? RecordLayout::Mis
         : selector == LRT_INTEGRATOR_VOLPATH_CLOSED ? RecordLayout::Closed : RecordLayout::Wide;
}

// The combinations that exist.  compact: the scene has no area emitter, so nothing reads the last scatter position: the lane id and the sampler's
// TEA word ride with the generator state in one 16-byte rng entry and lp_lane is not touched.
struct RecordForm { RecordLayout layout; bool compact; const char *name; };
constexpr RecordForm kRecordForms[] = { { RecordLayout::Wide, false, "wide" }, { RecordLayout::Wide, true, "compact" }, { RecordLayout::Bio, false, "bio" },
    { RecordLayout::Bio, true, "bio compact" }, { RecordLayout::Het, false, "het" }, { RecordLayout::Mis, false, "mis" }, { RecordLayout::Closed, true, "closed" } };
constexpr bool record_form_exists(RecordLayout l, bool compact) {
    for (const RecordForm &f : kRecordForms) if (f.layout == l && f.compact == compact) return true;
    return false;
}

// One stream of a record: the DPathStreams member (its offset), the bytes of one entry, the layouts whose wide and whose compact form use it
// (layout_bit masks).  prb: the PRB kernels' delta_L | slot stream, no member (DLaunch::dl0 / dl1, ensure_prb_workspace), beside the wide forms of Wide and Het.
struct RecordStream { const char *name; size_t member; uint32_t bytes, wide, compact; bool prb; };
constexpr size_t kNoMember = ~(size_t) 0;
namespace record_table {
constexpr uint32_t W = layout_bit(RecordLayout::Wide), B = layout_bit(RecordLayout::Bio), H = layout_bit(RecordLayout::Het), M = layout_bit(RecordLayout::Mis), C = layout_bit(RecordLayout::Closed);
#define LRT_STREAM(m) #m, offsetof(DPathStreams, m)
constexpr RecordStream kRecordStreams[] = {
    //                      bytes  wide forms     compact forms
    { LRT_STREAM(o_maxt),    16, W | B | H | M, W | B | C, false },
    { LRT_STREAM(d_eta),     16, W | B | H | M, W | B | C, false },
    { LRT_STREAM(tp_pdf),    16, W | B | H | M, W | B | C, false },
    { LRT_STREAM(res_flags), 16, W | B | H | M, W | B,     false },
    { LRT_STREAM(lp_lane),   16, W | B | H | M, 0,         false },
    { LRT_STREAM(rng),        8, W | B | H | M, 0,         false },    // PCG32 state
    { LRT_STREAM(rng),       16, 0,             W | B | C, false },    // state | lane | sampler word
    { LRT_STREAM(tdepth),     8, B,             B,         false },
    { LRT_STREAM(hit),       16, H | M,         0,         false },
    { LRT_STREAM(w1), 16, M, 0, false }, { LRT_STREAM(w2), 16, M, 0, false }, { LRT_STREAM(w3), 16, M, 0, false }, { LRT_STREAM(w4), 16, M, 0, false },
    { "delta_L", kNoMember,  16, 0,             0,         true },
};
#undef LRT_STREAM
}
using record_table::kRecordStreams;

// does the record of (layout, compact[, beside a PRB kernel]) occupy this row?
constexpr bool record_uses(const RecordStream &r, RecordLayout l, bool compact, bool prb = false) { return r.prb ? prb : ((compact ? r.compact : r.wide) & layout_bit(l)) != 0; }
// ... the stream `member` (an offsetof into DPathStreams) with entries of `bytes` bytes (0: of any size)?
constexpr bool record_has(RecordLayout l, bool compact, size_t member, uint32_t bytes = 0) {
    for (const RecordStream &r : kRecordStreams) if (r.member == member && (!bytes || r.bytes == bytes) && record_uses(r, l, compact)) return true;
    return false;
}
// bytes per queued path record, as lrt_render_stats reports them
constexpr uint32_t record_bytes(RecordLayout l, bool compact, bool prb = false) {
    uint32_t n = 0;
    for (const RecordStream &r : kRecordStreams) if (record_uses(r, l, compact, prb)) n += r.bytes;
    return n;
}
static_assert(record_bytes(RecordLayout::Wide, false) == 88 && record_bytes(RecordLayout::Wide, true) == 80 && record_bytes(RecordLayout::Bio, false) == 96 && record_bytes(RecordLayout::Bio, true) == 88, "wide / bio records");
static_assert(record_bytes(RecordLayout::Het, false) == 104 && record_bytes(RecordLayout::Mis, false) == 168 && record_bytes(RecordLayout::Closed, true) == 64, "het / mis / closed records");
static_assert(record_bytes(RecordLayout::Wide, false, true) == 104 && record_bytes(RecordLayout::Het, false, true) == 120, "PRB records");

// The workspace holds one allocation per DPathStreams member, shared by every form of the layouts in `layouts` (a layout_bit mask): the bytes per entry
// of the member at row `row` (0: no layout uses it, or an earlier row names the same member).  rng comes out at 16: the compact forms read it as uint4.
constexpr uint32_t workspace_stream_bytes(size_t row, uint32_t layouts) {
    uint32_t n = 0;
    for (size_t k = 0; k < sizeof(kRecordStreams) / sizeof(kRecordStreams[0]); ++k) {
        const RecordStream &r = kRecordStreams[k];
        if (r.member != kRecordStreams[row].member || r.member == kNoMember) continue;
        if (k < row) return 0;
        if (((r.wide | r.compact) & layouts) && r.bytes > n) n = r.bytes;
    }
    return n;
}
// The layouts a workspace is allocated for: every scene can run the Wide, Bio and Closed kernels; Het with a heterogeneous medium; Mis once volpathmis was asked for.
constexpr uint32_t workspace_layouts(bool has_het, bool mis) {
    return layout_bit(RecordLayout::Wide) | layout_bit(RecordLayout::Bio) | layout_bit(RecordLayout::Closed) | (has_het ? layout_bit(RecordLayout::Het) : 0u) | (mis ? layout_bit(RecordLayout::Mis) : 0u);
}

} // namespace lrt
