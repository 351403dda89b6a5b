// Counting inside the runs of a wave, from ballots alone.  The box-filter film routes (film.h) group the 64 lanes of a wave into RUNS of consecutive
// lanes of one pixel; what a run adds to a channel that holds a count (W: samples, alpha: valid samples) is a number of lanes, and a number of lanes
// is a popcount of a ballot over the run's range: no float scan.  Plain C++17, no HIP call: the kernels and tests/host/film_runs_main.cpp compile
// this text.
//   heads    bit j: lane j begins a run (lane 0 always does, whatever its bit says)
//   members  bit j: lane j counts
//   i        the lane that asks, 0 .. 63; its run is the lanes from the last head at or below i up to i
#pragma once
#include <cstdint>

namespace lrt {

// the lanes of the run that ends at lane i, as a mask
constexpr uint64_t film_run_lanes(uint64_t heads, uint32_t i) {
    const uint64_t upto = ~0ull >> (63u - i);                                      // lanes 0 .. i
    const uint32_t start = 63u - (uint32_t) __builtin_clzll((heads | 1ull) & upto);
    return upto & (~0ull << start);
}
// (two 32-bit counts: the sum stays a 32-bit value, which converts to float in one instruction on the device)
constexpr uint32_t film_popcount(uint64_t m) { return (uint32_t) __builtin_popcount((uint32_t) m) + (uint32_t) __builtin_popcount((uint32_t) (m >> 32)); }
// how many members the run that ends at lane i holds
constexpr uint32_t film_run_count(uint64_t heads, uint64_t members, uint32_t i) {
    return film_popcount(members & film_run_lanes(heads, i));
}
// ... and how many of them are set in `which` (the kernels' member masks already are the lanes they count: a run that ends at a retiring lane holds
// retiring lanes only, so finish_paths_wave_closed hands its valid retiring lanes to film_run_count; this is the form for a caller whose runs hold others)
constexpr uint32_t film_run_count_of(uint64_t heads, uint64_t members, uint64_t which, uint32_t i) {
    return film_popcount(which & members & film_run_lanes(heads, i));
}

static_assert(film_run_count(0ull, ~0ull, 63u) == 64u && film_run_count(~0ull, ~0ull, 63u) == 1u, "one run of 64 lanes; 64 runs of one");
static_assert(film_run_count(1ull << 40, ~0ull, 63u) == 24u && film_run_count(1ull << 40, ~0ull, 39u) == 40u, "a run that ends at lane 63; the one before it");
static_assert(film_run_count_of(1ull << 8, 0xff00ull, 0x5500ull, 15u) == 4u && film_run_count_of(1ull << 8, 0xf0ffull, 0xffffull, 15u) == 4u, "a third mask; a member mask with holes");

} // namespace lrt
