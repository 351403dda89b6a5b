// Stand-alone driver of liverrenderer_amd/csrc/film_runs.h for tests/test_film_runs.py: the two counts the film routes take from ballots, for
// every lane of a wave, against a plain loop over the 64 lanes.  Prints one JSON line per case (triples checked, lanes that differ, the first
// difference); the exit status is 0 when nothing differs.
#include "film_runs.h"
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>

using namespace lrt;

// the run that ends at lane i, walked lane by lane: back from i to the nearest head (lane 0 is one)
static void by_loop(uint64_t heads, uint64_t members, uint64_t which, uint32_t i, uint32_t *count, uint32_t *count_of) {
    uint32_t n = 0, m = 0;
    for (int j = (int) i; j >= 0; --j) {
        const bool member = (members >> j) & 1u;
        if (member) n += 1;
        if (member && ((which >> j) & 1u)) m += 1;
        if (j == 0 || ((heads >> j) & 1u)) break;
    }
    *count = n; *count_of = m;
}

struct Tally { unsigned long long triples = 0, lanes = 0, wrong = 0; std::string first; };
static void check(Tally &t, uint64_t heads, uint64_t members, uint64_t which) {
    t.triples += 1;
    for (uint32_t i = 0; i < 64; ++i) {
        uint32_t n, m; by_loop(heads, members, which, i, &n, &m);
        const uint32_t gn = film_run_count(heads, members, i), gm = film_run_count_of(heads, members, which, i);
        t.lanes += 1;
        if (gn == n && gm == m) continue;
        if (!t.wrong) {
            char buf[256];
            snprintf(buf, sizeof buf, "heads %016llx members %016llx which %016llx lane %u: count %u (loop %u), of %u (loop %u)", (unsigned long long) heads,
                     (unsigned long long) members, (unsigned long long) which, i, gn, n, gm, m);
            t.first = buf;
        }
        t.wrong += 1;
    }
}
static int report(const char *name, const Tally &t) {
    printf("{\"case\":\"%s\",\"triples\":%llu,\"lanes\":%llu,\"wrong\":%llu,\"first\":\"%s\"}\n", name, t.triples, t.lanes, t.wrong, t.first.c_str());
    return t.wrong ? 1 : 0;
}

int main() {
    const uint64_t all = ~0ull;
    int bad = 0;
    { Tally t; check(t, 1ull, all, all); check(t, 0ull, all, all); check(t, 0ull, all, 0x5555555555555555ull); bad |= report("one run", t); }     // (lane 0 heads a run with or without its bit)
    { Tally t; check(t, all, all, all); check(t, all, all, 0xaaaaaaaaaaaaaaaaull); check(t, all, 0x00ffff0000ffff00ull, all); bad |= report("64 runs of one lane", t); }
    { Tally t; for (int s = 1; s < 64; ++s) { check(t, 1ull | 1ull << s, all, all << s); check(t, 1ull << s, all >> 1, 1ull << 63); } bad |= report("a run that ends at lane 63", t); }
    { Tally t;
      check(t, 0x0001000100010001ull, 0xf0f0ff00ff0f0f0full, 0x00ff00ff00ff00ffull); check(t, 1ull << 8 | 1ull << 40, 0x8000000000000001ull, all);
      check(t, 0x1111111111111111ull, 0ull, all); check(t, 1ull << 20, all & ~(1ull << 20), 1ull << 20);
      bad |= report("member mask with holes", t); }
    { Tally t; std::mt19937_64 g(20240611u);
      for (int k = 0; k < 6000; ++k) {
          uint64_t h = g(), m = g(), w = g();
          if (k % 3 == 1) h &= g() & g();                            // longer runs
          if (k % 3 == 2) { h &= g() & g() & g(); m |= g(); }         // long runs, dense members
          check(t, h, m, w);
      }
      bad |= report("random", t); }
    return bad;
}
