// table_room.h - THE capacity rule of the keyed tables (keytab.cuh, keytab_host.inc: the talker and the port tables).  Plain host
// code with no HIP and no ctx in it, so that a test can compile it alone (tests/host_table_room.hip).
//
// Per table the host keeps an upper bound used_ub of the occupied slots: a chunk of m records (or m merged rows) adds at most m
// keys.  Before a launch, if the table does not fit used_ub + m, the stream is synchronised and the device's exact count replaces
// the bound; while it still does not fit the table doubles (tab_rehash_kernel re-inserts every slot).  So every launch finds its
// table at or below HALF full when it ends - the only reason tab_upsert's unbounded probe loop ends, and no update is ever parked
// or lost.  2^30 slots is the limit: FA_ERR_TABLE_FULL BEFORE the chunk is folded.
// Chunks: at most FA_TALK_CHUNK records (default 2^20), and at most max(2^16, capacity / 4) so that a small table grows in steps
// instead of jumping to the worst case of a large chunk.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fa {

constexpr uint32_t TABLE_ROOM_MAX_LOG2 = 30;
constexpr uint32_t TABLE_ROOM_FULL = 0xFFFFFFFFu;  // grow_to: no table of at most 2^30 slots fits

// used_ub + m keys in a table of 2^log2 slots at a load of at most 1/2
inline bool table_room_fits(uint64_t used_ub, uint64_t m, uint32_t log2) { return (used_ub + m) * 2 <= (1ull << log2); }
// the smallest log2' >= log2 that fits used + m, or TABLE_ROOM_FULL
inline uint32_t table_room_grow_to(uint64_t used, uint64_t m, uint32_t log2) {
    while (!table_room_fits(used, m, log2))
        if (++log2 > TABLE_ROOM_MAX_LOG2) return TABLE_ROOM_FULL;
    return log2;
}
inline size_t table_room_chunk_cap(size_t chunk, uint32_t log2_a, uint32_t log2_b) {
    const uint64_t cap = 1ull << (log2_a < log2_b ? log2_a : log2_b), floor = 1ull << 16;
    const uint64_t step = cap / 4 > floor ? cap / 4 : floor;
    return (size_t)(chunk < step ? chunk : step);
}

}  // namespace fa
