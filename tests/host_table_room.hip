// host_table_room.hip - the capacity rule of the keyed tables (csrc/table_room.h), run on the host.
// TEST INFRASTRUCTURE (tests/test_table_room_cpu.py).  No GPU call.  Prints, one line each:
//   fits USED M LOG2 V         table_room_fits(USED, M, LOG2)
//   grow USED M LOG2 V         table_room_grow_to(USED, M, LOG2); V = "full" when no table of at most 2^30 slots fits
//   cap CHUNK LOG2A LOG2B V    table_room_chunk_cap(CHUNK, LOG2A, LOG2B)
#include <cinttypes>
#include <cstdio>

#include "../flow-pipeline_amd/csrc/table_room.h"

using namespace fa;

static void fits(uint64_t used, uint64_t m, uint32_t log2) { printf("fits %" PRIu64 " %" PRIu64 " %u %d\n", used, m, log2, (int)table_room_fits(used, m, log2)); }
static void grow(uint64_t used, uint64_t m, uint32_t log2) {
    const uint32_t nl = table_room_grow_to(used, m, log2);
    if (nl == TABLE_ROOM_FULL) printf("grow %" PRIu64 " %" PRIu64 " %u full\n", used, m, log2);
    else printf("grow %" PRIu64 " %" PRIu64 " %u %u\n", used, m, log2, nl);
}

int main() {
    for (uint32_t log2 = 8; log2 <= 30; log2++) {
        const uint64_t half = 1ull << (log2 - 1);
        // used + m at exactly half of the capacity, split three ways; then one more
        const uint64_t used[3] = {0, half / 3, half};
        for (uint64_t u : used) {
            fits(u, half - u, log2);
            fits(u, half - u + 1, log2);
            grow(u, half - u, log2);
            grow(u, half - u + 1, log2);
        }
        // from the smallest table to every demand of this size
        grow(half - 1, 1, 8);
        grow(half, 1, 8);
        grow(0, half + 1, 8);
    }
    // beyond 2^30 slots: full, from any start
    grow(1ull << 29, 1, 30);
    grow(1ull << 29, 1, 8);
    grow(0, (1ull << 29) + 1, 16);
    grow(1ull << 40, 1ull << 40, 8);
    grow(0, 1ull << 29, 8);  // (exactly half of 2^30: the last demand that fits)
    const uint32_t caps[4] = {8, 18, 19, 30};
    const uint64_t chunks[4] = {1, 1ull << 16, 1ull << 20, 1ull << 28};
    for (uint32_t a : caps)
        for (uint32_t b : caps)
            for (uint64_t ch : chunks) printf("cap %" PRIu64 " %u %u %zu\n", ch, a, b, table_room_chunk_cap((size_t)ch, a, b));
    return 0;
}
