// Host driver of tests/test_list_tiles_cpu.py: runs the host-and-device functions of csrc/t2n_lists.h on the CPU. Standard input holds one
// case per line, "list_cap c0 .. c7" (raw counters: they may exceed list_cap); per case it prints the tile prefix, the tile total, every
// row's (live, slot index) and every live slot's row.
#include <stdio.h>
#include <vector>

#include "t2n_lists.h"

using namespace t2n;

int main() {
    unsigned cap, c[kLists];
    while (scanf("%u %u %u %u %u %u %u %u %u", &cap, &c[0], &c[1], &c[2], &c[3], &c[4], &c[5], &c[6], &c[7]) == 9) {
        std::vector<unsigned> raw((size_t)kLists * kCounterStride, 0xdeadbeefu);   // (only the strided words are counters)
        for (int l = 0; l < kLists; ++l) raw[(size_t)l * kCounterStride] = c[l];
        TilePrefix tp;
        const unsigned total = tile_prefix(raw.data(), cap, &tp);
        if (tile_prefix(raw.data(), cap, nullptr) != total) return 2;
        printf("case %u\nprefix", cap);
        for (int l = 0; l <= kLists; ++l) printf(" %u", tp.t[l]);
        printf("\nlive");
        for (int l = 0; l < kLists; ++l) printf(" %u", list_live(raw.data(), l, cap));
        printf("\ntotal %u\n", total);
        for (long long row = 0; row < (long long)total * 32; ++row) {
            unsigned idx;
            const bool live = row_to_entry(row, tp, raw.data(), cap, idx);
            printf("row %lld %d %u\n", row, live ? 1 : 0, idx);
        }
        for (int l = 0; l < kLists; ++l)
            for (unsigned s = 0; s < list_live(raw.data(), l, cap); ++s) printf("slot %u %u\n", l * cap + s, slot_to_row(l * cap + s, cap, tp));
    }
    return 0;
}
