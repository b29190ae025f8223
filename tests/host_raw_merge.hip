// host_raw_merge.hip - host instantiation of the two __host__ __device__ lookups of csrc/raw_merge.cuh (raw_merge_find: global row
// -> source; raw_merge_col / raw_merge_src_offset: (source rows, column, row) -> byte offset in the source), the text
// raw_merge_key_kernel and raw_merge_gather_kernel run, and a host model of the gather's tile walk.  TEST INFRASTRUCTURE
// (tests/test_raw_merge_cpu.py).  No GPU call.  Prints "OK <checks>" or the first failure and exits 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../flow-pipeline_amd/csrc/raw_merge.cuh"

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

// sources of the given row counts: every global row maps to the (source, row) a linear scan gives
static void check_find(const std::vector<uint32_t>& rows) {
    std::vector<RawMergeSrc> src(rows.size());
    uint32_t first = 0;
    for (size_t i = 0; i < rows.size(); i++) src[i] = RawMergeSrc{nullptr, rows[i], first}, first += rows[i];
    uint32_t p = 0;
    for (uint32_t g = 0; g < first; g++) {
        while (g >= src[p].first + src[p].rows) p++;  // the linear scan
        const uint32_t got = raw_merge_find([&](uint32_t i) { return src[i].first; }, (uint32_t)src.size(), g);
        CHECK(got == p && g - src[got].first < src[got].rows, "%zu sources: global row %u -> source %u, the scan gives %u", rows.size(), g, got, p);
    }
}

// every (rows, column, row) offset equals raw_col_offset + header + row * width and lies inside the part
static void check_offsets(uint64_t rows) {
    const uint64_t size = raw_col_offset(RAW_COLS_H, rows, RAW_NCOLS);
    for (uint32_t c = 0; c < RAW_NCOLS; c++) {
        const RawMergeCol k = raw_merge_col(RAW_COLS_H, c);
        CHECK(k.width == RAW_COLS_H[c].width, "column %u: width %u", c, k.width);
        for (uint64_t r = 0; r < rows; r++) {
            const uint64_t got = raw_merge_src_offset(k, rows, r);
            const uint64_t want = raw_col_offset(RAW_COLS_H, rows, c) + raw_col_header_len(RAW_COLS_H[c]) + r * RAW_COLS_H[c].width;
            CHECK(got == want && got + k.width <= size && got + k.width <= raw_col_offset(RAW_COLS_H, rows, c + 1), "rows %llu column %u row %llu: offset %llu, want %llu (part %llu)",
                  (unsigned long long)rows, c, (unsigned long long)r, (unsigned long long)got, (unsigned long long)want, (unsigned long long)size);
        }
    }
}

// The gather's tile walk: workgroup -> (column, tile) as the kernel finds them, lane -> its aligned 16-byte chunk, whole chunks
// as one store and a column's first and last chunk as byte stores, the headers from the column's first tile.  A part of `rows`
// rows whose first byte has the address phase `base` (mod 16): every byte is written exactly once, every wide store is aligned.
static void check_tiles(uint64_t rows, uint32_t base) {
    const uint64_t size = raw_col_offset(RAW_COLS_H, rows, RAW_NCOLS);
    std::vector<uint8_t> hits(size, 0);
    auto hit = [&](long long at, const char* what) {
        CHECK(at >= 0 && (uint64_t)at < size, "rows %llu base %u: %s outside the part at %lld", (unsigned long long)rows, base, what, at);
        hits[at]++;
    };
    uint64_t blocks = 0;
    for (uint32_t c = 0; c < RAW_NCOLS; c++)
        blocks += raw_col_tiles(base + raw_col_offset(RAW_COLS_H, rows, c) + raw_col_header_len(RAW_COLS_H[c]), rows * RAW_COLS_H[c].width);
    for (uint64_t block = 0; block < blocks; block++) {
        uint64_t tile = block, off = 1 + raw_varuint_len(rows);
        uint32_t c = 0;
        for (;; c++) {
            CHECK(c < RAW_NCOLS, "rows %llu base %u: block %llu has no column", (unsigned long long)rows, base, (unsigned long long)block);
            const RawColDef& d = RAW_COLS_H[c];
            const uint64_t data = off + raw_col_header_len(d), bytes = rows * d.width;
            const uint64_t tiles = raw_col_tiles(base + data, bytes);
            if (tile < tiles) break;
            tile -= tiles;
            off = data + bytes;
        }
        const RawColDef& d = RAW_COLS_H[c];
        const uint32_t hl = raw_col_header_len(d);
        CHECK(off == raw_col_offset(RAW_COLS_H, rows, c), "rows %llu: column %u found at %llu", (unsigned long long)rows, c, (unsigned long long)off);
        const long long col = (long long)(off + hl), bytes = (long long)(rows * d.width);
        if (tile == 0) {
            for (uint32_t t = 0; t < hl; t++) hit((long long)off + t, "a column header byte");
            if (c == 0)
                for (uint32_t t = 0; t < 1 + raw_varuint_len(rows); t++) hit(t, "a block header byte");
        }
        const long long s = (long long)tile * (RAW_TILE_CHUNKS * 16) - (long long)((base + col) & 15);
        for (uint32_t tid = 0; tid < RAW_BLOCK; tid++) {
            const long long b = s + 16ll * tid;
            if (b >= bytes || b + 16 <= 0) continue;
            if (b >= 0 && b + 16 <= bytes) {
                CHECK(((base + col + b) & 15) == 0, "rows %llu base %u column %u: a 16-byte store at phase %lld", (unsigned long long)rows, base, c, (base + col + b) & 15);
                for (int i = 0; i < 16; i++) hit(col + b + i, "a whole chunk");
            } else {
                for (int i = 0; i < 16; i++)
                    if (b + i >= 0 && b + i < bytes) hit(col + b + i, "a partial chunk");
            }
        }
    }
    for (uint64_t i = 0; i < size; i++) CHECK(hits[i] == 1, "rows %llu base %u: byte %llu written %u times", (unsigned long long)rows, base, (unsigned long long)i, hits[i]);
}

int main() {
    // ---- global row -> (source, row): source rows of 1 .. 300, 16383 and 16384; 1, 2, 17 sources and beyond the LDS table
    std::vector<uint32_t> all;
    for (uint32_t r = 1; r <= 300; r++) all.push_back(r);
    all.push_back(16383), all.push_back(16384);
    check_find({1});
    check_find({16384});
    check_find({3, 1});
    check_find({16383, 16384});
    check_find(std::vector<uint32_t>(all.begin(), all.begin() + 17));
    check_find(all);
    for (uint32_t n : {RAW_MERGE_LDS_SRCS - 1, RAW_MERGE_LDS_SRCS, RAW_MERGE_LDS_SRCS + 1, 2 * RAW_MERGE_LDS_SRCS + 2}) {
        std::vector<uint32_t> many(n);
        for (uint32_t i = 0; i < n; i++) many[i] = 1 + (i * 7) % 5;
        check_find(many);
        check_find(std::vector<uint32_t>(n, 1));
    }
    // ---- (rows, column, row) -> offset
    for (uint32_t r : all) check_offsets(r);
    // ---- the tile walk over the merged row counts of the GPU test, at every address phase of the part's first byte
    for (uint32_t rows : {1u, 2u, 127u, 128u, 129u, 255u, 256u, 257u, 1023u, 1024u, 1025u, 16383u, 16384u})
        for (uint32_t base = 0; base < 16; base++) check_tiles(rows, base);
    printf("OK %llu\n", checks);
    return 0;
}
