// noise_target_probe — host::noise_quantile_bin / noise_bin_upper / noise_target_met / noise_part_weight on the histogram or the pairs
// given as arguments, printed for tests/test_host_logic.py (test_noise_target_decision).
#include "check_common.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../csrc/pt_host.h"
using namespace pt;
// argv: pixels stats.mean_error target.mean_error target.quantile target.quantile_error [bin count]..: the quantile bin, the bits of
// its upper edge, whether the target is met
int main(int argc, char **argv) {
    if (argv[1][0] == 'w') {  // w nA nB ..: the bits of a part's weight, pair by pair
        for (int i = 2; i + 1 < argc; i += 2) {
            const float w = host::noise_part_weight((uint32_t)atoi(argv[i]), (uint32_t)atoi(argv[i + 1]));
            uint32_t bits;
            memcpy(&bits, &w, 4);
            printf("%u\n", bits);
        }
        return 0;
    }
    pt_noise_stats s{};
    s.pixels = strtoull(argv[1], 0, 10);
    s.mean_error = atof(argv[2]);
    pt_noise_target t{};
    t.mean_error = (float)atof(argv[3]);
    t.quantile = (float)atof(argv[4]);
    t.quantile_error = (float)atof(argv[5]);
    for (int i = 6; i + 1 < argc; i += 2) s.histogram[atoi(argv[i])] = (uint32_t)atoi(argv[i + 1]);
    const uint32_t b = host::noise_quantile_bin(s, t.quantile);
    const float up = host::noise_bin_upper(b);
    uint32_t bits;
    memcpy(&bits, &up, 4);
    printf("%u %u %d\n", b, bits, (int)host::noise_target_met(s, t));
    return 0;
}
