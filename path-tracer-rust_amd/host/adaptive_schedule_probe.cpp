// adaptive_schedule_probe — host::AdaptiveSchedule: which class of tiles a held adaptive frame's call takes next, step by step, on the tile
// table given as arguments, printed for tests/test_adaptive_held_abi.py (test_class_scheduler).
#include "check_common.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../csrc/pt_host.h"
using namespace pt;
// argv: q cap n0 width rows tile_shift closes tiles..: the tiles as cnt:na:E (E "-" = none), `closes` a comma list - how many
// tiles step j closes (missing: none).  Prints every step of the call and what is open at the end.
int main(int argc, char **argv) {
    const unsigned long long q = strtoull(argv[1], 0, 10);
    const uint32_t cap = (uint32_t)strtoul(argv[2], 0, 10), n0 = (uint32_t)strtoul(argv[3], 0, 10);
    const uint32_t width = (uint32_t)atoi(argv[4]), rows = (uint32_t)atoi(argv[5]);
    host::TileGeometry g;
    if (host::tile_geometry(width, rows, (uint32_t)atoi(argv[6]), g) != PT_OK) return 2;
    std::vector<uint32_t> closes;
    for (const char *p = argv[7]; *p && *p != '-';) {
        char *e;
        closes.push_back((uint32_t)strtoul(p, &e, 10));
        p = *e ? e + 1 : e;
    }
    host::TileTable t;
    for (int i = 8; i < argc; ++i) {
        unsigned c, a;
        char es[64];
        if (sscanf(argv[i], "%u:%u:%63s", &c, &a, es) != 3) return 2;
        t.cnt.push_back(c);
        t.na.push_back(a);
        t.err.push_back(es[0] == '-' ? kTileNoError : strtoull(es, 0, 10));
    }
    if (t.cnt.size() != g.tiles) return 3;
    host::AdaptiveSchedule s(t, width, rows, g, q, cap, n0);
    printf("open %u atcap %u\n", s.tiles_open(), s.tiles_at_cap());
    host::AdaptiveStep st;
    for (size_t j = 0; s.next(st) && j < 100; ++j) {
        printf("step c %u na %u n %u T %u m %u runs %u to_a %d %d na_end %u\n", st.c, st.na, st.n, st.T, st.m, st.runs(), (int)st.to_a[0],
               (int)(st.runs() > 1 && st.to_a[1]), st.na_end);
        const uint32_t k = j < closes.size() ? closes[j] : 0u;
        s.done(st, st.n - k, k);
    }
    printf("open %u atcap %u\n", s.tiles_open(), s.tiles_at_cap());
    return 0;
}
