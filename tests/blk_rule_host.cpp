// blk_rule_host.cpp -- the block geometry rules of deltarice_amd/csrc/drx_blocks.h on the host, printed over a grid
// (tests/test_blk_rule_host.py compiles this host-side and compares every line with the Python mirror in tests/block_cells.py).
//   nt <WaveformLength> <k> <nt_for_len> <blk_segw_plan>
//   sw <b10> <blk_segw_bits10>
//   cap <words per lane> <blk_lane_cap>
#include <stdint.h>
#include <stdio.h>

#include "drx_blocks.h"

using namespace drx;

int main() {
    long lines = 0;
    // every length to 40 000 in steps of 7 and 64 (each rule's borders lie at multiples of 64 / (2 k + 7)), the lengths of the
    // tests' cells, and lengths around 2^31 and 2^32 - 1
    for (uint32_t k = 0; k < 16; ++k) {
        for (uint32_t len = 1; len <= 40000u; len += (len % 64u == 0u ? 1u : 7u)) {
            printf("nt %u %u %d %d\n", len, k, nt_for_len(len, k), blk_segw_plan(k));
            ++lines;
        }
        const uint32_t more[] = {2048u, 3000u, 6000u, 20000u, 90000u, 500000u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
        for (uint32_t len : more) {
            printf("nt %u %u %d %d\n", len, k, nt_for_len(len, k), blk_segw_plan(k));
            ++lines;
        }
    }
    for (uint64_t b10 = 0; b10 <= 400u; ++b10) {
        printf("sw %llu %d\n", (unsigned long long)b10, blk_segw_bits10(b10));
        ++lines;
    }
    const int sws[] = {9, 11, 15, 19};
    for (int sw : sws) {
        printf("cap %d %u\n", sw, blk_lane_cap(sw));
        ++lines;
    }
    printf("%ld lines\n", lines);
    return 0;
}
