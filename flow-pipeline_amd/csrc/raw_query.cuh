// raw_query.cuh - grouped queries over flows_raw parts: WHERE, several GROUP BYs and their sums in one pass over the slices a
// ranged load leaves (gfx950; host side: raw_query_host.inc; the contract: include/flowagg.h "grouped queries over flows_raw
// parts"; run on the host by tests/host_raw_query.hip).
//
// The five ClickHouse panels of the dashboard (viz-ch.json:74, 233, 358, 479, 604) are
//   SELECT <key>, sum(Bytes*SamplingRate) FROM flows_raw WHERE $timeFilter [AND ...] GROUP BY <key> ORDER BY ...
// over the same rows.  A kind (one FA_RAW_G_* bit, RAW_Q_KINDS of them, numbered by the bit's position) is one such GROUP BY.
//
// Keys.  Every kind's groups live in ONE pair of keyed tables (keytab.cuh) under the talkers' slot and key (talkers.cuh): the
// kind's number stands where a bucketed talker key carries its bucket index (tkey_pack_bucket), so equal values of two kinds are
// two keys, and talker_rows_kernel<true> with the range [kind, kind] hands out one kind's rows.  Kind j lives in table j & 1.
//   address kinds  the talker panels' canonical (key, family): talker_canon_words, nothing restated;
//   scalar kinds   (lo, hi, family) = (the value as a big-endian number in key bytes 0..7, 0, 0): the order of the key BYTES is
//                  the numeric order of the value (little-endian bytes under memcmp put 256 before 255), so the talkers' four
//                  sort passes order a scalar kind numerically as they stand.  MINUTE: t - t % 60; TOTAL: the value 0.
//
// raw_query_fold_kernel, the hot part.  The select's flattened grid of slices (RawSelectPart, raw_select_find; a tile = RAW_SEL_BLOCK
// rows of one slice, a lane one row), walked by a PERSISTENT grid: a workgroup takes tiles tile_lo + blockIdx.x, + gridDim.x, ...
// so the LDS cache is cleared and flushed once per workgroup, not once per tile.  Per tile: the predicate is raw_select_eval with
// the select kernel's loaders; a wave without a match is done.  A matching lane reads Bytes and SamplingRate once - 8-byte
// columns at any byte phase: element-width reads at the element's own address, raw_select.cuh's "no edge path" argument: bytes
// of raw_range_load_spans(rows, r_lo, r_hi) - and EType if an address kind is asked for.  Then one trip per kind of `groups`
// (wave-uniform: a scalar loop, the highest bit first): the kind's column is read by the matching lanes alone, the key packed,
// and the update goes to the workgroup's LDS cache (tab_lds_add) or, past its probes, to the global table (tab_upsert).  An
// address column the predicate loaded is read again (it hits the cache line the predicate pulled); the wave pre-sum for kinds of
// few keys is not built.
// The kinds go from the highest bit down: TOTAL, PROTO, the ASes and MINUTE have few keys, and a cache entry is never evicted, so
// they must claim their entries in a workgroup's first tile BEFORE the ports and addresses fill the cache - behind them they would
// find it full and every lane of the chip would add to the same few global slots (measured: 2.2 against 0.3 ns per update).
// Capacity: a launch over m rows with g kinds creates at most m * g keys per table; raw_query_launch_tiles gives the tiles of a
// launch so that m * g stays at or below the tables' chunk (2^20 keys), the host reserves m * g in both tables before every launch
// (table_room.h: the table grows in one rebuild to hold them at half load).  The step does not follow the table's size as the
// talkers' does: a query knows its rows when it starts, and launches of 2^16 keys - 51 tiles with five kinds - leave the chip idle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/flowagg.h"
#include "keytab.cuh"
#include "raw_select.cuh"
#include "table_room.h"
#include "talkers.cuh"

namespace fa {

constexpr uint32_t RAW_Q_KINDS = 9;
constexpr uint32_t RAW_Q_C_RATE = 4, RAW_Q_C_BYTES = 14;  // SamplingRate, Bytes of RAW_COLS
enum { RAW_Q_K_SRC_ADDR = 0, RAW_Q_K_DST_ADDR, RAW_Q_K_SRC_PORT, RAW_Q_K_DST_PORT, RAW_Q_K_MINUTE, RAW_Q_K_SRC_AS, RAW_Q_K_DST_AS, RAW_Q_K_PROTO, RAW_Q_K_TOTAL };
static_assert((1u << RAW_Q_K_SRC_ADDR) == FA_RAW_G_SRC_ADDR && (1u << RAW_Q_K_DST_PORT) == FA_RAW_G_DST_PORT && (1u << RAW_Q_K_MINUTE) == FA_RAW_G_MINUTE &&
                  (1u << RAW_Q_K_PROTO) == FA_RAW_G_PROTO && (1u << RAW_Q_K_TOTAL) == FA_RAW_G_TOTAL && FA_RAW_G_ALL == (1u << RAW_Q_KINDS) - 1,
              "a kind's number is its bit's position");
static_assert(sizeof(fa_raw_query_t) == 104 && sizeof(fa_query_row) == sizeof(TalkRow), "fa_raw_query_t; a query row is a talker row whose pad is the value");

// ---- the key text (host and device: tests/host_raw_query.hip runs it against naive restatements) ---------------------------------
__host__ __device__ __forceinline__ bool raw_query_kind_is_addr(uint32_t kind) { return kind < 2; }
// the column of RAW_COLS a kind's key is read from (TOTAL: none, RAW_NCOLS)
__host__ __device__ __forceinline__ uint32_t raw_query_kind_col(uint32_t kind) {
    switch (kind) {
    case RAW_Q_K_SRC_ADDR: return RAW_SEL_C_SRC_ADDR;
    case RAW_Q_K_DST_ADDR: return RAW_SEL_C_DST_ADDR;
    case RAW_Q_K_SRC_PORT: return RAW_SEL_C_SRC_PORT;
    case RAW_Q_K_DST_PORT: return RAW_SEL_C_DST_PORT;
    case RAW_Q_K_MINUTE: return RAW_SEL_C_FLOW_START;
    case RAW_Q_K_SRC_AS: return RAW_SEL_C_SRC_AS;
    case RAW_Q_K_DST_AS: return RAW_SEL_C_DST_AS;
    case RAW_Q_K_PROTO: return RAW_SEL_C_PROTO;
    default: return RAW_NCOLS;
    }
}
// the columns a query's kinds read beside the predicate's (bit c: column c): the keys, Bytes, SamplingRate, EType for an address kind
__host__ __device__ inline uint32_t raw_query_cols(uint32_t groups) {
    uint32_t m = (1u << RAW_Q_C_RATE) | (1u << RAW_Q_C_BYTES);
    for (uint32_t j = 0; j < RAW_Q_KINDS; j++)
        if ((groups >> j & 1) && raw_query_kind_col(j) < RAW_NCOLS) m |= 1u << raw_query_kind_col(j);
    if (groups & (FA_RAW_G_SRC_ADDR | FA_RAW_G_DST_ADDR)) m |= 1u << RAW_SEL_C_ETYPE;
    return m;
}
__host__ __device__ __forceinline__ uint32_t raw_query_minute(uint32_t t) { return t - t % 60u; }  // toStartOfMinute
// a scalar as the key's low word: key bytes 0..3 zero, bytes 4..7 the value, most significant byte first
__host__ __device__ __forceinline__ uint64_t raw_query_scalar_lo(uint32_t v) { return __builtin_bswap64((uint64_t)v); }
__host__ __device__ __forceinline__ uint32_t raw_query_scalar_value(uint64_t lo) { return (uint32_t)__builtin_bswap64(lo); }
// a scalar kind's value of a row: v = the kind's column value (TOTAL: anything)
__host__ __device__ __forceinline__ uint32_t raw_query_scalar_of(uint32_t kind, uint32_t v) { return kind == RAW_Q_K_MINUTE ? raw_query_minute(v) : kind == RAW_Q_K_TOTAL ? 0u : v; }
__host__ __device__ __forceinline__ void raw_query_key_scalar(uint32_t kind, uint32_t value, TKey& k) { tkey_pack_bucket(raw_query_scalar_lo(value), 0, 0, kind, k); }
// (lo, hi): the stored 16 bytes as two little-endian words
__host__ __device__ __forceinline__ void raw_query_key_addr(uint32_t kind, uint64_t lo, uint64_t hi, uint32_t etype, TKey& k) {
    const uint32_t fam = talker_canon_words(lo, hi, etype);
    tkey_pack_bucket(lo, hi, fam, kind, k);
}

// ---- the rows of a launch ----------------------------------------------------------------------------------------------------------
// The tiles of one launch with g kinds asked for: tiles * RAW_SEL_BLOCK rows create at most rows * g keys in a table, and that
// stays at or below `chunk` keys whenever one tile's do.  At least one tile.
inline uint32_t raw_query_launch_tiles(size_t chunk, uint32_t g) {
    const uint64_t per_tile = (uint64_t)RAW_SEL_BLOCK * (g ? g : 1u);
    const uint64_t tiles = (uint64_t)chunk / per_tile;
    return (uint32_t)(tiles > 0x7FFFFFFFull ? 0x7FFFFFFFull : tiles ? tiles : 1u);
}
// the keys a launch of `tiles` tiles may create in one table: what the host reserves
inline uint64_t raw_query_launch_keys(uint32_t tiles, uint32_t g) { return (uint64_t)tiles * RAW_SEL_BLOCK * g; }

// ---- the tables' traits: the talkers' slot, key, hash and tally; the fold kernel's own geometry ----------------------------------------
// 256 threads = one tile per trip; 512 entries per table = 40 KiB of LDS per workgroup, three workgroups per CU = 12 waves behind the
// latency of the global upserts (reasoned as talkers.cuh's sizes, not tuned).
struct QueryTab : TalkTab {
    static constexpr int BLOCK = RAW_SEL_BLOCK;
    static constexpr int WG_PER_CU = 3;
    static constexpr char NOUN[] = "query", FN[] = "fa_raw_query", WGPC_ENV[] = "FA_QUERY_WGPC";
};

struct RawQueryArgs {
    const RawSelectPart* parts;  // the slices of the call, tile0 ascending
    uint32_t nparts;
    uint32_t groups;             // FA_RAW_G_* bits, at least one
    const uint8_t* img;
    uint32_t tile_lo, tile_hi;   // the launch's tiles of the flattened grid
    TSlot* tab[2];
    uint32_t mask[2];
    TalkCounters* ctr;           // folded = rows matched, absorbed = updates that ended in an LDS cache
    fa_raw_filter f;
};

__global__ __launch_bounds__(RAW_SEL_BLOCK) void raw_query_fold_kernel(const RawQueryArgs a) {
    __shared__ TabLds<QueryTab> L;
    tab_lds_clear(L);
    uint32_t absorbed = 0, folded = 0, made0 = 0, made1 = 0;
    const uint32_t tid = threadIdx.x;
    for (uint32_t t = a.tile_lo + blockIdx.x; t < a.tile_hi; t += gridDim.x) {  // (tile_hi <= the call's tiles: every t has its slice)
        const RawSelectPart p = a.parts[raw_select_find(a.parts, a.nparts, t)];
        const uint64_t r = (uint64_t)p.r_lo + (uint64_t)(t - p.tile0) * RAW_SEL_BLOCK + tid;
        const bool valid = r < p.r_hi;
        const uint8_t* const part = a.img + p.off;
        auto load4 = [&](uint32_t c) { return raw_load_unaligned32(part + raw_merge_src_offset(raw_merge_col(RAW_COLS_D, c), p.rows, r)); };
        auto load16 = [&](uint32_t c, uint32_t* v) { raw_load_unaligned(part + raw_merge_src_offset(raw_merge_col(RAW_COLS_D, c), p.rows, r), 4, v); };
        const bool hit = raw_select_eval(
            a.f, valid, [&](uint32_t c) { return valid ? load4(c) : 0u; }, load16, [](bool x) { return __ballot(x) != 0; });
        if (__ballot(hit) == 0) continue;  // (wave-uniform; no barrier inside the tile loop)
        uint64_t w = 0;
        uint32_t et = 0;
        if (hit) {  // (hit implies valid: every read below is a read of a row of the slice)
            uint32_t b[4], s[4];
            raw_load_unaligned(part + raw_merge_src_offset(raw_merge_col(RAW_COLS_D, RAW_Q_C_BYTES), p.rows, r), 2, b);
            raw_load_unaligned(part + raw_merge_src_offset(raw_merge_col(RAW_COLS_D, RAW_Q_C_RATE), p.rows, r), 2, s);
            w = ((uint64_t)b[1] << 32 | b[0]) * ((uint64_t)s[1] << 32 | s[0]);
            if (a.groups & (FA_RAW_G_SRC_ADDR | FA_RAW_G_DST_ADDR)) et = load4(RAW_SEL_C_ETYPE);
            folded++;
        }
#pragma unroll 1
        for (uint32_t g = a.groups; g;) {
            const uint32_t kind = 31u - (uint32_t)__builtin_clz(g);  // (uniform; the kinds of few keys first)
            g &= ~(1u << kind);
            if (!hit) continue;
            TKey k;
            if (raw_query_kind_is_addr(kind)) {
                uint32_t v[4];
                load16(raw_query_kind_col(kind), v);
                raw_query_key_addr(kind, (uint64_t)v[1] << 32 | v[0], (uint64_t)v[3] << 32 | v[2], et, k);
            } else {
                const uint32_t v = kind == RAW_Q_K_TOTAL ? 0u : load4(raw_query_kind_col(kind));
                raw_query_key_scalar(kind, raw_query_scalar_of(kind, v), k);
            }
            const uint32_t h = tkey_hash(k);
            const int d = (int)(kind & 1u);
            if (tab_lds_add(L, d, k, h, w)) {
                absorbed++;
            } else {
                uint32_t made[1] = {0};
                tab_upsert<QueryTab>(d ? a.tab[1] : a.tab[0], d ? a.mask[1] : a.mask[0], k, h, w, 1, a.ctr, made);
                made0 += d ? 0u : made[0], made1 += d ? made[0] : 0u;
            }
        }
    }
    uint32_t created[2][1] = {{made0}, {made1}};
    tab_lds_flush(L, a.tab, a.mask, a.ctr, absorbed, folded, created);
}

// a scalar kind's ordered rows, in place: the talker row's key bytes back into `value` (fa_query_row: key and etype 0)
__global__ __launch_bounds__(256) void raw_query_scalar_rows_kernel(TalkRow* rows, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t v = raw_query_scalar_value(rows[i].key[0]);
        rows[i].key[0] = 0, rows[i].key[1] = 0, rows[i].etype = 0, rows[i].pad = v;
    }
}

// ---- adding another ctx's rows to the result held (fa_raw_query_merge_device; the contract: include/flowagg.h) --------------------
// A row of `kind` as a query of that kind produces it (run on the host by tests/host_raw_query_merge.hip against a naive
// restatement): an address kind's canonical key with value 0; a scalar kind's value with a zero key and etype 0, MINUTE on the
// minute grid, TOTAL 0.
__host__ __device__ __forceinline__ bool raw_query_row_ok(uint32_t kind, const TalkRow& r) {
    if (raw_query_kind_is_addr(kind)) return r.pad == 0u && (r.etype == 0u || (r.etype == TALK_FAMILY_V4 && (r.key[0] >> 32) == 0ull && r.key[1] == 0ull));
    if (r.key[0] != 0ull || r.key[1] != 0ull || r.etype != 0u) return false;
    return kind == RAW_Q_K_MINUTE ? r.pad % 60u == 0u : kind == RAW_Q_K_TOTAL ? r.pad == 0u : true;
}
// the key of a row in the tables: the fold's own key text over the row's two little-endian key words and etype, or its value
__host__ __device__ __forceinline__ void raw_query_row_key(uint32_t kind, const TalkRow& r, TKey& k) {
    if (raw_query_kind_is_addr(kind)) raw_query_key_addr(kind, r.key[0], r.key[1], r.etype, k);
    else raw_query_key_scalar(kind, r.pad, k);
}
// The status word of a merge: the rows that are no rows of `kind`.  The adds are launched only after it was read as 0.
__global__ __launch_bounds__(256) void raw_query_rows_check_kernel(const TalkRow* rows, uint64_t n, uint32_t kind, unsigned int* bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (!raw_query_row_ok(kind, rows[i])) atomicAdd(bad, 1u);
}
// raw_query_merge_kernel: one lane per row, n rows of ONE kind (at most the tables' chunk: the host reserved n keys in table
// kind & 1 - the fold's capacity rule), each added through tab_upsert into the table the fold kernel feeds for that kind.  No LDS
// cache: a member's rows hold every key once, so a cache would absorb nothing and every entry would be flushed by one more upsert;
// the keys of different members meet in the global table, where the atomics are memory-side either way.  The row is one 40-byte
// read per lane (rows back to back: a wave reads 2560 contiguous bytes); the cost is the random 64-byte slot per row.
struct RawQueryMergeArgs {
    const TalkRow* rows;
    uint32_t n, kind;
    TSlot* tab;
    uint32_t mask;
    TalkCounters* ctr;
};
__global__ __launch_bounds__(256) void raw_query_merge_kernel(const RawQueryMergeArgs a) {
    uint32_t created[1] = {0};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {  // (n <= 2^28, the grid <= 2^20 threads: no wrap)
        const TalkRow r = a.rows[i];
        TKey k;
        raw_query_row_key(a.kind, r, k);
        tab_upsert<QueryTab>(a.tab, a.mask, k, tkey_hash(k), r.weight, r.count, a.ctr, created);
    }
    tab_count_created<QueryTab>(a.ctr, (int)(a.kind & 1u), created);  // (every lane of every wave gets here)
}

}  // namespace fa
