// host_raw_select.hip - host instantiation of what selecting rows of flows_raw parts decides without a GPU (csrc/raw_select.cuh):
// the prefix comparison against a bit-by-bit loop, the predicate against a naive restatement over bytes, the position rule
// against the list of set bits, and every byte raw_select_kernel and raw_select_emit_kernel load for a slice against the blocks
// stages B and C of a ranged load planned (csrc/raw_range_plan.h).  TEST INFRASTRUCTURE (tests/test_raw_select_cpu.py).  No GPU
// call.  Prints "OK <checks>" or the first failure and exits 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../flow-pipeline_amd/csrc/raw_range_plan.h"
#include "../flow-pipeline_amd/csrc/raw_select.cuh"

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

static_assert(sizeof(fa_raw_filter) == 96, "fa_raw_filter");
static_assert(sizeof(fa_raw_select_stats_t) == 80, "fa_raw_select_stats_t");

// ---- the naive restatement: over the stored bytes, one bit at a time ------------------------------------------------------------
struct NaiveRow {
    uint32_t tfs, src_as, dst_as, etype, proto, src_port, dst_port;
    uint8_t src[16], dst[16];
};
static int bit_of(const uint8_t* a, uint32_t i) { return (a[i / 8] >> (7 - i % 8)) & 1; }
static bool naive_prefix(const uint8_t* a, const uint8_t* b, uint32_t len) {
    for (uint32_t i = 0; i < len; i++)
        if (bit_of(a, i) != bit_of(b, i)) return false;
    return true;
}
static bool naive_range(uint32_t t, uint32_t lo, uint32_t hi) {
    const uint64_t upper = hi == 0xFFFFFFFFu ? (uint64_t)1 << 32 : hi;
    return (uint64_t)t >= lo && (uint64_t)t < upper;
}
static bool naive_dir(const fa_raw_filter& f, uint32_t s_as, uint32_t d_as, uint32_t s_port, uint32_t d_port, const uint8_t* s, const uint8_t* d) {
    if ((f.fields & FA_RAW_F_SRC_AS) && s_as != f.src_as) return false;
    if ((f.fields & FA_RAW_F_DST_AS) && d_as != f.dst_as) return false;
    if ((f.fields & FA_RAW_F_SRC_PORT) && !(f.src_port_lo <= s_port && s_port <= f.src_port_hi)) return false;
    if ((f.fields & FA_RAW_F_DST_PORT) && !(f.dst_port_lo <= d_port && d_port <= f.dst_port_hi)) return false;
    if ((f.fields & FA_RAW_F_SRC_ADDR) && !naive_prefix(s, f.src_addr, f.src_prefix_len)) return false;
    if ((f.fields & FA_RAW_F_DST_ADDR) && !naive_prefix(d, f.dst_addr, f.dst_prefix_len)) return false;
    return true;
}
static bool naive_match(const NaiveRow& r, const fa_raw_filter& f) {
    if ((f.fields & FA_RAW_F_FLOW_START) && !naive_range(r.tfs, f.tf_lo, f.tf_hi)) return false;
    if ((f.fields & FA_RAW_F_ETYPE) && r.etype != f.etype) return false;
    if ((f.fields & FA_RAW_F_PROTO) && r.proto != f.proto) return false;
    if (naive_dir(f, r.src_as, r.dst_as, r.src_port, r.dst_port, r.src, r.dst)) return true;
    return (f.fields & FA_RAW_F_EITHER) && naive_dir(f, r.dst_as, r.src_as, r.dst_port, r.src_port, r.dst, r.src);
}
static RawSelectRow loaded(const NaiveRow& r) {
    RawSelectRow o{r.tfs, r.src_as, r.dst_as, r.etype, r.proto, r.src_port, r.dst_port, {}, {}};
    memcpy(o.src_addr, r.src, 16), memcpy(o.dst_addr, r.dst, 16);  // (little-endian host: the dwords the kernel loads)
    return o;
}

// ---- 1: the prefix comparison ---------------------------------------------------------------------------------------------------
static void check_prefix() {
    std::mt19937 rng(99);
    auto eq = [](const uint8_t* a, const uint8_t* b, uint32_t len) {
        uint32_t x[4], y[4];
        memcpy(x, a, 16), memcpy(y, b, 16);
        return raw_select_prefix_eq(x, y, len);
    };
    for (uint32_t len = 0; len <= 128; len++)
        for (int round = 0; round < 200; round++) {
            uint8_t a[16], b[16];
            for (int i = 0; i < 16; i++) a[i] = (uint8_t)rng(), b[i] = round % 2 ? (uint8_t)rng() : a[i];
            if (round % 4 == 1) memcpy(b, a, len / 8);  // a long common prefix, random behind it
            CHECK(eq(a, b, len) == naive_prefix(a, b, len), "prefix length %u: random pair", len);
            memcpy(b, a, 16);
            if (len >= 1) {  // only bit len - 1 differs: the last bit inside
                b[(len - 1) / 8] ^= (uint8_t)(0x80 >> ((len - 1) % 8));
                CHECK(!eq(a, b, len) && !naive_prefix(a, b, len), "prefix length %u: the last bit inside differs and the strings compare equal", len);
                memcpy(b, a, 16);
            }
            if (len < 128) {  // only bit len differs: the first bit outside
                b[len / 8] ^= (uint8_t)(0x80 >> (len % 8));
                CHECK(eq(a, b, len) && naive_prefix(a, b, len), "prefix length %u: the first bit outside differs and the strings compare unequal", len);
            }
        }
}

// ---- 2: the predicate -----------------------------------------------------------------------------------------------------------
static const uint32_t PORTS[] = {0u, 65535u, 65536u, 0xFFFFFFFFu, 80u, 443u};
static std::vector<NaiveRow> make_rows(size_t n, std::mt19937& rng, uint8_t pool[8][16]) {
    std::vector<NaiveRow> rows(n);
    for (NaiveRow& r : rows) {
        r.tfs = 1000 + rng() % 100;
        if (rng() % 50 == 0) r.tfs = rng() % 2 ? 0u : 0xFFFFFFFFu;
        r.src_as = rng() % 4, r.dst_as = rng() % 4;
        r.etype = rng() % 2 ? 0x800u : 0x86DDu, r.proto = (uint32_t[]){6u, 17u, 1u}[rng() % 3];
        r.src_port = PORTS[rng() % 6], r.dst_port = PORTS[rng() % 6];
        memcpy(r.src, pool[rng() % 8], 16), memcpy(r.dst, pool[rng() % 8], 16);
        if (rng() % 4 == 0) r.src[rng() % 16] ^= (uint8_t)(1u << rng() % 8);
        if (rng() % 4 == 0) r.dst[rng() % 16] ^= (uint8_t)(1u << rng() % 8);
    }
    return rows;
}
static fa_raw_filter base_filter(std::mt19937& rng, uint8_t pool[8][16]) {
    fa_raw_filter f;
    memset(&f, 0, sizeof f);
    f.t_hi = 0xFFFFFFFFu;
    f.tf_lo = 1000 + rng() % 60, f.tf_hi = rng() % 5 == 0 ? 0xFFFFFFFFu : f.tf_lo + rng() % 60;
    f.src_as = rng() % 4, f.dst_as = rng() % 4, f.etype = rng() % 2 ? 0x800u : 0x86DDu, f.proto = rng() % 2 ? 6u : 17u;
    uint32_t a = PORTS[rng() % 6], b = PORTS[rng() % 6];
    f.src_port_lo = std::min(a, b), f.src_port_hi = rng() % 2 ? f.src_port_lo : std::max(a, b);
    a = PORTS[rng() % 6], b = PORTS[rng() % 6];
    f.dst_port_lo = std::min(a, b), f.dst_port_hi = rng() % 2 ? f.dst_port_lo : std::max(a, b);
    static const uint8_t lens[] = {0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 48, 120, 24};
    f.src_prefix_len = lens[rng() % 16], f.dst_prefix_len = lens[rng() % 16];
    memcpy(f.src_addr, pool[rng() % 8], 16), memcpy(f.dst_addr, pool[rng() % 8], 16);
    // bits behind the prefix are ignored: scramble them
    for (uint32_t i = f.src_prefix_len; i < 128; i++)
        if (rng() % 2) f.src_addr[i / 8] ^= (uint8_t)(0x80 >> (i % 8));
    return f;
}
static void check_match() {
    std::mt19937 rng(20261021);
    uint8_t pool[8][16];
    for (int i = 0; i < 16; i++) pool[0][i] = (uint8_t)rng();
    for (int k = 1; k < 8; k++) {  // neighbours that share prefixes of several lengths
        memcpy(pool[k], pool[k / 2], 16);
        const uint32_t bit = (uint32_t[]){0, 127, 64, 33, 24, 9, 120, 63}[k];
        pool[k][bit / 8] ^= (uint8_t)(0x80 >> (bit % 8));
    }
    const std::vector<NaiveRow> rows = make_rows(100000, rng, pool);
    std::vector<RawSelectRow> ld;
    for (const NaiveRow& r : rows) ld.push_back(loaded(r));
    std::vector<fa_raw_filter> filters;
    for (uint32_t bit = 1; bit <= FA_RAW_F_COUNT_ONLY; bit <<= 1) {  // every bit alone
        fa_raw_filter f = base_filter(rng, pool);
        f.fields = bit;
        filters.push_back(f);
    }
    for (uint32_t p : {0u, 65535u, 65536u, 0xFFFFFFFFu})  // ports at the edges, lo == hi
        for (uint32_t bit : {FA_RAW_F_SRC_PORT, FA_RAW_F_DST_PORT}) {
            fa_raw_filter f = base_filter(rng, pool);
            f.fields = bit | (p == 65536u ? FA_RAW_F_EITHER : 0u);
            f.src_port_lo = f.src_port_hi = f.dst_port_lo = f.dst_port_hi = p;
            filters.push_back(f);
        }
    for (uint32_t bit : {FA_RAW_F_SRC_AS, FA_RAW_F_DST_AS, FA_RAW_F_SRC_PORT, FA_RAW_F_DST_PORT, FA_RAW_F_SRC_ADDR, FA_RAW_F_DST_ADDR}) {  // EITHER with one condition
        fa_raw_filter f = base_filter(rng, pool);
        f.fields = bit | FA_RAW_F_EITHER;
        if (f.src_prefix_len < 9) f.src_prefix_len = 64;
        if (f.dst_prefix_len < 9) f.dst_prefix_len = 33;
        filters.push_back(f);
    }
    while (filters.size() < 200) {
        fa_raw_filter f = base_filter(rng, pool);
        const uint32_t k = 1 + rng() % 4;  // a few conditions: filters of many select nothing
        for (uint32_t i = 0; i < k; i++) f.fields |= 1u << (rng() % 9);
        if (rng() % 2) f.fields |= FA_RAW_F_EITHER;
        if (filters.size() % 25 == 0) f.fields = FA_RAW_F_ALL;
        filters.push_back(f);
    }
    unsigned long long some = 0, either_fwd_only = 0, either_swapped_only = 0;
    for (const fa_raw_filter& f : filters) {
        CHECK(raw_select_filter_why(f) == nullptr, "a generated filter is refused: %s", raw_select_filter_why(f));
        size_t hits = 0;
        for (size_t i = 0; i < rows.size(); i++) {
            const bool want = naive_match(rows[i], f), got = raw_select_match(ld[i], f);
            CHECK(got == want, "fields 0x%x row %zu: the predicate says %d, the restatement %d", f.fields, i, (int)got, (int)want);
            hits += want;
            if (want && (f.fields & FA_RAW_F_EITHER)) {
                fa_raw_filter g = f;
                g.fields &= ~FA_RAW_F_EITHER;
                const bool fwd = naive_match(rows[i], g);
                NaiveRow sw = rows[i];
                std::swap(sw.src_as, sw.dst_as), std::swap(sw.src_port, sw.dst_port);
                for (int b = 0; b < 16; b++) std::swap(sw.src[b], sw.dst[b]);
                const bool back = naive_match(sw, g);
                CHECK(fwd || back, "EITHER matches a row neither direction matches");
                either_fwd_only += fwd && !back, either_swapped_only += back && !fwd;
            }
        }
        some += hits > 0 && hits < rows.size();
    }
    CHECK(filters.size() == 200 && some >= 100, "only %llu of 200 filters select some and not all rows", some);
    CHECK(either_fwd_only > 1000 && either_swapped_only > 1000, "EITHER with one direction alone: %llu forward, %llu swapped", either_fwd_only, either_swapped_only);
    // the columns a filter reads: exactly those the restatement's result depends on being loaded
    CHECK(raw_select_cols(0) == 0 && raw_select_cols(FA_RAW_F_EITHER | FA_RAW_F_COUNT_ONLY) == 0, "a filter without a condition reads a column");
    CHECK(raw_select_cols(FA_RAW_F_SRC_ADDR) == 1u << 6 && raw_select_cols(FA_RAW_F_SRC_ADDR | FA_RAW_F_EITHER) == (3u << 6), "the address columns of a filter");
    CHECK(raw_select_row_bytes(RAW_COLS_H, FA_RAW_F_ALL) == 7 * 4 + 2 * 16 && raw_select_row_bytes(RAW_COLS_H, FA_RAW_F_DST_PORT) == 4, "the bytes a filter reads per row");
    // refusals
    fa_raw_filter f = base_filter(rng, pool);
    auto refused = [&](fa_raw_filter g) { return raw_select_filter_why(g) != nullptr; };
    fa_raw_filter g = f;
    g.fields = 2048;
    CHECK(refused(g), "an unknown bit");
    g = f, g.t_lo = 5, g.t_hi = 4;
    CHECK(refused(g), "t_lo > t_hi");
    g = f, g.fields = FA_RAW_F_FLOW_START, g.tf_lo = 5, g.tf_hi = 4;
    CHECK(refused(g), "tf_lo > tf_hi");
    g.fields = 0;
    CHECK(!refused(g), "tf_lo > tf_hi with the bit clear is not read");
    g = f, g.fields = FA_RAW_F_SRC_PORT, g.src_port_lo = 2, g.src_port_hi = 1;
    CHECK(refused(g), "src port lo > hi");
    g = f, g.fields = FA_RAW_F_DST_PORT, g.dst_port_lo = 2, g.dst_port_hi = 1;
    CHECK(refused(g), "dst port lo > hi");
    g = f, g.fields = FA_RAW_F_SRC_ADDR, g.src_prefix_len = 129;
    CHECK(refused(g), "src prefix 129");
    g = f, g.fields = FA_RAW_F_DST_ADDR, g.dst_prefix_len = 129;
    CHECK(refused(g), "dst prefix 129");
    g = f, g.fields = 0, g._pad[1] = 1;
    CHECK(refused(g), "_pad");
}

// ---- 3: the position rule -------------------------------------------------------------------------------------------------------
static void check_positions() {
    std::mt19937_64 rng(7);
    for (int round = 0; round < 3000; round++) {
        const uint32_t nwg = 1 + round % 5;
        std::vector<uint64_t> words(nwg * RAW_SEL_WAVES);
        for (uint64_t& w : words) {
            switch (rng() % 5) {
            case 0: w = 0; break;
            case 1: w = ~0ull; break;
            case 2: w = rng() & rng() & rng(); break;
            default: w = rng();
            }
        }
        std::vector<uint32_t> set_rows, base(nwg + 1, 0);
        for (uint32_t g = 0; g < nwg; g++) {
            uint32_t n = 0;
            for (uint32_t w = 0; w < RAW_SEL_WAVES; w++)
                for (uint32_t l = 0; l < 64; l++)
                    if (words[g * RAW_SEL_WAVES + w] >> l & 1) set_rows.push_back(g * RAW_SEL_BLOCK + w * 64 + l), n++;
            base[g + 1] = base[g] + n;  // (the exclusive scan of the workgroup counts)
        }
        const uint32_t count = (uint32_t)set_rows.size();
        for (uint32_t cap : {count ? count - 1 : 0u, count, count + 1, count / 2, 1u}) {
            const uint32_t take = std::min(count, cap);
            std::vector<uint32_t> out(take, 0xFFFFFFFFu);
            std::vector<uint8_t> written(take, 0);
            for (uint32_t g = 0; g < nwg; g++)
                for (uint32_t w = 0; w < RAW_SEL_WAVES; w++)
                    for (uint32_t l = 0; l < 64; l++) {
                        if (!(words[g * RAW_SEL_WAVES + w] >> l & 1)) continue;
                        const uint32_t pos = raw_select_pos(base[g] - base[0], &words[g * RAW_SEL_WAVES], w, l);
                        if (pos >= take) continue;
                        CHECK(!written[pos], "round %d: position %u is written twice", round, pos);
                        written[pos] = 1, out[pos] = g * RAW_SEL_BLOCK + w * 64 + l;
                    }
            for (uint32_t i = 0; i < take; i++)
                CHECK(written[i] && out[i] == set_rows[i], "round %d cap %u: position %u holds row %u, the %u-th set bit is row %u", round, cap, i, out[i], i, set_rows[i]);
        }
    }
}

// ---- 4: every byte the kernels load lies in a planned block -----------------------------------------------------------------------
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
    const uint32_t all_cols = raw_select_cols(FA_RAW_F_ALL);
    CHECK(all_cols == ((1u << 2) | (3u << 6) | (63u << 8)), "the columns a filter can name");
    for (uint64_t r_lo : pts)
        for (uint64_t r_hi : pts) {
            if (r_lo >= r_hi) continue;
            std::vector<uint8_t> d2 = done;
            raw_range_load_blocks(RAW_COLS_H, rows, FIRST, nblocks, r_lo, r_hi, d2, tmp);
            // the workgroups of the slice own its rows, each once, and no other
            const uint64_t tiles = raw_select_tiles(r_hi - r_lo);
            CHECK(tiles * RAW_SEL_BLOCK >= r_hi - r_lo && (tiles - 1) * RAW_SEL_BLOCK < r_hi - r_lo, "rows %llu: %llu tiles", (unsigned long long)rows, (unsigned long long)tiles);
            for (uint64_t r = r_lo; r < r_hi; r++) {
                if (r_hi - r_lo > 700 && r > r_lo + 300 && r + 300 < r_hi && (r - r_lo) % 97) continue;  // (long slices: both ends and a stride)
                for (uint32_t c = 0; c < RAW_NCOLS; c++) {
                    if (!(all_cols >> c & 1) && c != RAW_SEL_C_TIME) continue;
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
    check_prefix();
    check_match();
    check_positions();
    for (uint64_t rows = 1; rows <= 300; rows++) check_loads(rows, true);
    // the row counts of host_raw_range.hip's grid: varuint(rows) grows at 2^7 and 2^14; a block holds 595.78 rows; a 4-, 8-, 16-byte column fills a block at 16384, 8192, 4096 rows
    std::set<uint64_t> big = {16383, 16384, 16385, 8191, 8192, 8193, 4095, 4096, 4097, 4100, 16380, 16390};
    for (uint64_t k : {1, 2, 3, 7, 11, 27}) big.insert(595 * k - 1), big.insert(595 * k), big.insert(595 * k + 1), big.insert(595 * k + k * 78 / 100), big.insert(595 * k + k * 78 / 100 + 1);
    for (uint64_t rows : big) check_loads(rows, false);
    printf("OK %llu\n", checks);
    return 0;
}
