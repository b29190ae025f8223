// host_raw_query.hip - host instantiation of what a grouped query over flows_raw parts decides without a GPU (csrc/raw_query.cuh):
// the key text (canonical words, minute, scalar pack and unpack, packed order == numeric order) against naive restatements over
// bytes, the rows of a launch against the capacity rule (csrc/table_room.h) for 1 .. 9 kinds, the persistent walk over the tiles,
// and every byte raw_query_fold_kernel loads for a slice - predicate columns, key columns, Bytes, SamplingRate - against the blocks
// stages B and C of a ranged load planned (csrc/raw_range_plan.h).  TEST INFRASTRUCTURE (tests/test_raw_query_cpu.py).  No GPU call.
// Prints "OK <checks>" or the first failure and exits 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../flow-pipeline_amd/csrc/raw_query.cuh"
#include "../flow-pipeline_amd/csrc/raw_range_plan.h"

using namespace fa;

static unsigned long long checks = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        checks++;                         \
        if (!(cond)) {                    \
            fprintf(stderr, "FAILED: "); \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

static_assert(sizeof(fa_raw_query_t) == 104 && sizeof(fa_query_row) == 40 && sizeof(fa_raw_query_stats_t) == 80, "the query's structures");

// ---- 1: the key text --------------------------------------------------------------------------------------------------------------
// a key as the read side sees it: the talker row's 16 key bytes and family, and the kind
struct NaiveKey {
    uint8_t key[16];
    uint32_t family, kind;
    bool operator==(const NaiveKey& o) const { return !memcmp(key, o.key, 16) && family == o.family && kind == o.kind; }
};
static NaiveKey unpacked(const TKey& k) {
    NaiveKey o{};
    unsigned long long lo, hi;
    tkey_unpack(k.w, lo, hi, o.family);
    memcpy(o.key, &lo, 8), memcpy(o.key + 8, &hi, 8);  // (little-endian host: the bytes as stored)
    o.kind = tkey_bucket(k.w);
    return o;
}
static NaiveKey naive_addr(uint32_t kind, const uint8_t addr[16], uint32_t etype) {
    NaiveKey o{};
    o.kind = kind;
    if (etype == 0x800) {  // the dotted quad's preimage: four bytes
        memcpy(o.key, addr, 4);
        o.family = 0x800;
    } else {
        memcpy(o.key, addr, 16);
    }
    return o;
}
static NaiveKey naive_scalar(uint32_t kind, uint32_t value) {
    NaiveKey o{};
    o.kind = kind;
    for (int i = 0; i < 4; i++) o.key[4 + i] = (uint8_t)(value >> (24 - 8 * i));  // most significant byte first
    return o;
}
static void check_keys() {
    std::mt19937_64 rng(31);
    const uint32_t etypes[] = {0x800u, 0x86DDu, 0u, 0x1234u, 0x801u, 0x8000800u};
    for (int round = 0; round < 200000; round++) {
        uint8_t addr[16];
        for (int i = 0; i < 16; i++) addr[i] = round % 7 == 0 ? 0 : (uint8_t)rng();
        if (round % 11 == 0) memset(addr + 4, 0xFF, 12);
        const uint32_t et = etypes[rng() % 6], kind = (uint32_t)(rng() % 2);
        uint64_t lo, hi;
        memcpy(&lo, addr, 8), memcpy(&hi, addr + 8, 8);
        TKey k;
        raw_query_key_addr(kind, lo, hi, et, k);
        CHECK(k.w[0] && k.w[1] && k.w[2], "an address key has an empty word");
        CHECK(unpacked(k) == naive_addr(kind, addr, et), "round %d: the address key of EType 0x%x", round, et);
        // the same bytes under the two families are two keys; 0x800 ignores bytes 4..15; every other EType is one family
        TKey k4, k6, kx;
        raw_query_key_addr(kind, lo, hi, 0x800, k4), raw_query_key_addr(kind, lo, hi, 0x86DD, k6), raw_query_key_addr(kind, lo, hi, 0x1234, kx);
        CHECK(memcmp(&k4, &k6, sizeof k4) != 0 && memcmp(&k6, &kx, sizeof k6) == 0, "the families");
        TKey k4b;
        raw_query_key_addr(kind, lo ^ (rng() << 32), hi ^ rng(), 0x800, k4b);
        CHECK(memcmp(&k4, &k4b, sizeof k4) == 0, "EType 0x800: bytes 4..15 change the key");
        raw_query_key_addr(kind ^ 1, lo, hi, et, kx);
        CHECK(memcmp(&k, &kx, sizeof k) != 0, "the two address kinds share a key");
    }
    std::vector<uint32_t> vals = {0u, 1u, 59u, 60u, 61u, 119u, 120u, 254u, 255u, 256u, 257u, 65535u, 65536u, 65537u, 0x00FFFFFFu, 0x01000000u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFC3u,
                                  0xFFFFFFC4u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (int i = 0; i < 3000; i++) vals.push_back((uint32_t)rng() >> (rng() % 32));
    for (uint32_t v : vals) {
        CHECK(raw_query_minute(v) == (uint32_t)((uint64_t)v / 60 * 60) && raw_query_minute(v) <= v && v - raw_query_minute(v) < 60, "the minute of %u", v);
        CHECK(raw_query_scalar_value(raw_query_scalar_lo(v)) == v, "scalar %u does not come back", v);
        for (uint32_t kind = 2; kind < RAW_Q_KINDS; kind++) {
            TKey k;
            const uint32_t value = raw_query_scalar_of(kind, v);
            CHECK(value == (kind == RAW_Q_K_MINUTE ? v - v % 60 : kind == RAW_Q_K_TOTAL ? 0u : v), "kind %u: the value of %u", kind, v);
            raw_query_key_scalar(kind, value, k);
            CHECK(k.w[0] && k.w[1] && k.w[2], "a scalar key has an empty word");
            CHECK(unpacked(k) == naive_scalar(kind, value), "kind %u value %u: the scalar key", kind, value);
        }
    }
    // packed order == numeric order: the read side orders key bytes 0..7 as a big-endian word (memcmp)
    for (size_t i = 0; i < vals.size(); i++)
        for (size_t j = 0; j < vals.size(); j += 1 + (i % 5)) {
            TKey a, b;
            raw_query_key_scalar(RAW_Q_K_DST_PORT, vals[i], a), raw_query_key_scalar(RAW_Q_K_DST_PORT, vals[j], b);
            const NaiveKey x = unpacked(a), y = unpacked(b);
            const int c = memcmp(x.key, y.key, 16);
            CHECK((c < 0) == (vals[i] < vals[j]) && (c == 0) == (vals[i] == vals[j]), "%u against %u: the key bytes order them differently", vals[i], vals[j]);
            CHECK((memcmp(&a, &b, sizeof a) == 0) == (vals[i] == vals[j]), "%u and %u: key equality", vals[i], vals[j]);
        }
    // a kind's number is its bit's position; the columns
    const uint32_t bits[RAW_Q_KINDS] = {FA_RAW_G_SRC_ADDR, FA_RAW_G_DST_ADDR, FA_RAW_G_SRC_PORT, FA_RAW_G_DST_PORT, FA_RAW_G_MINUTE, FA_RAW_G_SRC_AS, FA_RAW_G_DST_AS, FA_RAW_G_PROTO, FA_RAW_G_TOTAL};
    const uint32_t cols[RAW_Q_KINDS] = {6, 7, 12, 13, 2, 8, 9, 11, RAW_NCOLS};
    uint32_t all = 0;
    for (uint32_t j = 0; j < RAW_Q_KINDS; j++) {
        CHECK(bits[j] == 1u << j && raw_query_kind_col(j) == cols[j] && raw_query_kind_is_addr(j) == (j < 2), "kind %u", j);
        if (cols[j] < RAW_NCOLS) CHECK(RAW_COLS_H[cols[j]].width == (j < 2 ? 16 : 4), "kind %u: its column's width", j);
        all |= bits[j];
    }
    CHECK(all == FA_RAW_G_ALL, "FA_RAW_G_ALL");
    CHECK(RAW_COLS_H[RAW_Q_C_BYTES].width == 8 && !strcmp(RAW_COLS_H[RAW_Q_C_BYTES].name, "Bytes") && RAW_COLS_H[RAW_Q_C_RATE].width == 8 && !strcmp(RAW_COLS_H[RAW_Q_C_RATE].name, "SamplingRate"),
          "Bytes and SamplingRate");
    CHECK(!strcmp(RAW_COLS_H[2].name, "TimeFlowStart") && !strcmp(RAW_COLS_H[12].name, "SrcPort") && !strcmp(RAW_COLS_H[9].name, "DstAS") && !strcmp(RAW_COLS_H[11].name, "Proto"), "the key columns");
    CHECK(raw_query_cols(FA_RAW_G_TOTAL) == ((1u << 4) | (1u << 14)) && raw_query_cols(FA_RAW_G_DST_ADDR) == ((1u << 4) | (1u << 14) | (1u << 7) | (1u << 10)) &&
              raw_query_cols(FA_RAW_G_ALL) == ((1u << 4) | (1u << 14) | (1u << 2) | (3u << 6) | (63u << 8)),
          "the columns a query reads");
}

// ---- 2: the rows of a launch against the capacity rule -------------------------------------------------------------------------------
static void check_room() {
    std::mt19937_64 rng(32);
    for (uint32_t g = 1; g <= RAW_Q_KINDS; g++)
        for (size_t chunk : {(size_t)1, (size_t)255, (size_t)4096, (size_t)1 << 16, (size_t)1 << 20, (size_t)1 << 28}) {
            const uint32_t tiles = raw_query_launch_tiles(chunk, g);
            const uint64_t keys = raw_query_launch_keys(tiles, g);
            CHECK(tiles >= 1 && keys == (uint64_t)tiles * RAW_SEL_BLOCK * g, "g %u: the keys of a launch", g);
            CHECK(keys <= chunk || tiles == 1, "g %u chunk %zu: %llu keys are more than the chunk", g, chunk, (unsigned long long)keys);
            CHECK((uint64_t)(tiles + 1) * RAW_SEL_BLOCK * g > chunk, "g %u: a launch could take another tile", g);
            // whatever the tables hold, the room rule finds a size that keeps them at or below half load, or says there is none
            for (uint32_t log2 = 8; log2 <= TABLE_ROOM_MAX_LOG2; log2++)
                for (uint64_t used : {(uint64_t)0, (uint64_t)1 << (log2 - 1), ((uint64_t)1 << (log2 - 1)) - keys % 100}) {
                    const uint32_t nl = table_room_grow_to(used, keys, log2);
                    CHECK(nl == TABLE_ROOM_FULL ? (used + keys) * 2 > (1ull << TABLE_ROOM_MAX_LOG2) : nl >= log2 && table_room_fits(used, keys, nl) && (nl == log2 || !table_room_fits(used, keys, nl - 1)),
                          "g %u: %llu keys on %llu in 2^%u slots", g, (unsigned long long)keys, (unsigned long long)used, log2);
                }
        }
    // the host's loop, restated: before every launch the bound fits or the exact count replaces it and the table grows; so a launch
    // that adds at most its keys ends at or below half load, whatever it created
    for (int round = 0; round < 3000; round++) {
        const uint32_t g = 1 + (uint32_t)(rng() % RAW_Q_KINDS);
        uint32_t log2[2] = {16, 16};
        uint64_t exact[2] = {0, 0}, ub[2] = {0, 0};
        uint32_t left = 1 + (uint32_t)(rng() % 40000);  // tiles: up to 10^7 rows
        const size_t chunk = round % 3 ? (size_t)1 << 20 : (size_t)1 << (10 + rng() % 12);
        const int distinct = (int)(rng() % 4);  // how many of the possible keys are new: none, few, half, all
        while (left) {
            const uint32_t nt = std::min(left, raw_query_launch_tiles(chunk, g));
            const uint64_t keys = raw_query_launch_keys(nt, g);
            for (int d = 0; d < 2; d++) {
                if (!table_room_fits(ub[d], keys, log2[d])) {
                    ub[d] = exact[d];  // (the settle)
                    const uint32_t nl = table_room_grow_to(ub[d], keys, log2[d]);
                    CHECK(nl != TABLE_ROOM_FULL, "round %d: 10^7 rows x 9 kinds fill 2^30 slots", round);
                    log2[d] = nl;
                }
                CHECK(table_room_fits(ub[d], keys, log2[d]) && exact[d] <= ub[d], "round %d: a launch without room", round);
            }
            for (int d = 0; d < 2; d++) {
                const uint64_t made = distinct == 0 ? 0 : distinct == 1 ? rng() % 8 : distinct == 2 ? keys / 2 : keys;
                exact[d] += made, ub[d] += keys;
                CHECK(exact[d] * 2 <= (1ull << log2[d]), "round %d: table %d above half load behind a launch", round, d);
            }
            left -= nt;
        }
    }
}

// ---- 3: the persistent walk ----------------------------------------------------------------------------------------------------------
static void check_walk() {
    for (uint32_t lo : {0u, 5u})
        for (uint32_t n = 1; n <= 70; n++)
            for (uint32_t grid : {1u, 2u, 3u, 7u, 64u, n}) {
                if (grid > n) continue;  // (the host launches at most a workgroup per tile)
                std::vector<int> seen(n, 0);
                for (uint32_t b = 0; b < grid; b++)
                    for (uint32_t t = lo + b; t < lo + n; t += grid) seen[t - lo]++;
                for (uint32_t i = 0; i < n; i++) CHECK(seen[i] == 1, "tiles [%u, %u) grid %u: tile %u is walked %d times", lo, lo + n, grid, lo + i, seen[i]);
            }
}

// ---- 4: every byte the fold kernel loads lies in a planned block ---------------------------------------------------------------------
constexpr uint32_t FIRST = 3;  // the part's first block of the call
static void check_loads(uint64_t rows, bool dense) {
    const uint64_t bytes = raw_col_offset(RAW_COLS_H, rows, RAW_NCOLS);
    const uint32_t nblocks = (uint32_t)((bytes + RAW_SLOT - 1) / RAW_SLOT);
    std::vector<uint8_t> done(FIRST + nblocks + 2, 0);
    std::vector<uint32_t> tmp;
    raw_range_scan_blocks(RAW_COLS_H, rows, FIRST, nblocks, done, tmp);  // (stage B alone: the probe's blocks are not relied on)
    std::set<uint64_t> pts = {0, rows};
    const uint64_t cand[] = {1, 3, 63, 64, 65, rows / 3, rows / 2, rows / 2 + 1, rows - 65, rows - 4, rows - 1};
    const uint64_t few[] = {1, 65, rows / 3, rows / 2 + 1, rows - 4, rows - 1};
    if (dense) {
        for (uint64_t x : cand)
            if (x <= rows) pts.insert(x);
    } else {
        for (uint64_t x : few)
            if (x <= rows) pts.insert(x);
    }
    auto planned = [&](const std::vector<uint8_t>& pl, uint64_t o, uint64_t len) {
        if (o + len > bytes) return false;
        for (uint64_t x = o; x < o + len; x++)
            if (!pl[FIRST + x / RAW_SLOT]) return false;
        return true;
    };
    // what a query with every condition and every kind reads of a row: the predicate's columns, the keys', Bytes, SamplingRate, EType
    const uint32_t all_cols = raw_select_cols(FA_RAW_F_ALL) | raw_query_cols(FA_RAW_G_ALL);
    CHECK(all_cols == ((1u << 2) | (1u << 4) | (3u << 6) | (63u << 8) | (1u << 14)), "the columns a query can read");
    for (uint64_t r_lo : pts)
        for (uint64_t r_hi : pts) {
            if (r_lo >= r_hi) continue;
            std::vector<uint8_t> d2 = done;
            raw_range_load_blocks(RAW_COLS_H, rows, FIRST, nblocks, r_lo, r_hi, d2, tmp);
            const uint64_t tiles = raw_select_tiles(r_hi - r_lo);
            CHECK(tiles * RAW_SEL_BLOCK >= r_hi - r_lo && (tiles - 1) * RAW_SEL_BLOCK < r_hi - r_lo, "rows %llu: %llu tiles", (unsigned long long)rows, (unsigned long long)tiles);
            for (uint64_t r = r_lo; r < r_hi; r++) {
                if (r_hi - r_lo > 700 && r > r_lo + 300 && r + 300 < r_hi && (r - r_lo) % 97) continue;  // (long slices: both ends and a stride)
                for (uint32_t c = 0; c < RAW_NCOLS; c++) {
                    if (!(all_cols >> c & 1)) continue;
                    const RawMergeCol k = raw_merge_col(RAW_COLS_H, c);
                    const uint64_t o = raw_merge_src_offset(k, rows, r);
                    CHECK(o == raw_col_offset(RAW_COLS_H, rows, c) + raw_col_header_len(RAW_COLS_H[c]) + r * RAW_COLS_H[c].width && k.width == RAW_COLS_H[c].width,
                          "rows %llu column %u row %llu: the element's offset", (unsigned long long)rows, c, (unsigned long long)r);
                    CHECK(planned(d2, o, k.width), "rows %llu [%llu, %llu) column %u row %llu: the kernel's load at part byte %llu leaves the planned blocks", (unsigned long long)rows,
                          (unsigned long long)r_lo, (unsigned long long)r_hi, c, (unsigned long long)r, (unsigned long long)o);
                }
            }
        }
}

int main() {
    check_keys();
    check_room();
    check_walk();
    for (uint64_t rows = 1; rows <= 300; rows++) check_loads(rows, true);
    // the row counts of host_raw_range.hip's grid: varuint(rows) grows at 2^7 and 2^14; a block holds 595.78 rows; a 4-, 8-, 16-byte column fills a block at 16384, 8192, 4096 rows
    std::set<uint64_t> big = {16383, 16384, 16385, 8191, 8192, 8193, 4095, 4096, 4097, 4100, 16380, 16390};
    for (uint64_t k : {1, 2, 3, 7, 11, 27}) big.insert(595 * k - 1), big.insert(595 * k), big.insert(595 * k + 1), big.insert(595 * k + k * 78 / 100), big.insert(595 * k + k * 78 / 100 + 1);
    for (uint64_t rows : big) check_loads(rows, false);
    printf("OK %llu\n", checks);
    return 0;
}
