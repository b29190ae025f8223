// host_raw_merge.hip - host instantiation of the two __host__ __device__ lookups of csrc/raw_merge.cuh (raw_merge_find: global row
// -> source; raw_merge_col / raw_merge_src_offset: (source rows, column, row) -> byte offset in the source), the text
// raw_merge_key_kernel and raw_merge_gather_kernel run, and of the part writer's geometry of csrc/raw.cuh (the tile walk and the
// LDS staging, enumerated with the functions raw_write_tile computes them by).  TEST INFRASTRUCTURE
// (tests/test_raw_merge_cpu.py).  No GPU call.  Prints "OK <checks>" or the first failure and exits 1.
#include <hip/hip_runtime.h>

#include <algorithm>
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

// The part writer's tile walk, enumerated with the geometry functions the kernels run (csrc/raw.cuh): workgroup -> (column, tile),
// lane -> its aligned 16-byte chunk, whole chunks as one store and a column's first and last chunk as byte stores, the headers
// from the column's first tile.  A part of `rows` rows whose first byte has the address phase `base` (mod 16): every byte is
// written exactly once, every wide store is aligned.
static void check_tiles(uint64_t rows, uint32_t base) {
    const uint64_t size = raw_col_offset(RAW_COLS_H, rows, RAW_NCOLS);
    std::vector<uint8_t> hits(size, 0);
    auto hit = [&](long long at, const char* what) {
        CHECK(at >= 0 && (uint64_t)at < size, "rows %llu base %u: %s outside the part at %lld", (unsigned long long)rows, base, what, at);
        hits[at]++;
    };
    const uint64_t blocks = raw_part_tiles(RAW_COLS_H, base, rows);
    RawTile t;
    CHECK(!raw_tile_locate(RAW_COLS_H, base, rows, blocks, &t), "rows %llu base %u: a tile behind the last one", (unsigned long long)rows, base);
    for (uint64_t block = 0; block < blocks; block++) {
        CHECK(raw_tile_locate(RAW_COLS_H, base, rows, block, &t), "rows %llu base %u: block %llu has no column", (unsigned long long)rows, base, (unsigned long long)block);
        const RawColDef& d = RAW_COLS_H[t.c];
        const uint32_t hl = raw_col_header_len(d);
        CHECK(t.off == raw_col_offset(RAW_COLS_H, rows, t.c), "rows %llu: column %u found at %llu", (unsigned long long)rows, t.c, (unsigned long long)t.off);
        const long long col = (long long)(t.off + hl), bytes = (long long)(rows * d.width);
        if (t.tile == 0) {
            for (uint32_t i = 0; i < hl; i++) hit((long long)t.off + i, "a column header byte");
            if (t.c == 0)
                for (uint32_t i = 0; i < 1 + raw_varuint_len(rows); i++) hit(i, "a block header byte");
        }
        const RawTilePhase ph = raw_tile_phase(base + col, t.tile);
        for (uint32_t tid = 0; tid < RAW_BLOCK; tid++) {
            const long long b = raw_lane_byte(ph.s, tid);
            if (raw_chunk_outside(b, bytes)) continue;
            if (raw_chunk_whole(b, bytes)) {
                CHECK(((base + col + b) & 15) == 0, "rows %llu base %u column %u: a 16-byte store at phase %lld", (unsigned long long)rows, base, t.c, (base + col + b) & 15);
                for (int i = 0; i < 16; i++) hit(col + b + i, "a whole chunk");
            } else {
                for (int i = 0; i < 16; i++)
                    if (raw_chunk_byte_in(b, i, bytes)) hit(col + b + i, "a partial chunk");
            }
        }
    }
    for (uint64_t i = 0; i < size; i++) CHECK(hits[i] == 1, "rows %llu base %u: byte %llu written %u times", (unsigned long long)rows, base, (unsigned long long)i, hits[i]);
}

// The staging of every tile of every column but Date, with the functions the writer stages by: the (element, dword) pairs it
// writes to LDS slots.  Every slot that a lane with a chunk inside the column reads (4 tid .. 4 tid + 4) and that holds a byte of
// the column is written exactly once, by the (e, q) with 0 <= e < rows that the column's byte stream puts there.  (That
// nothing is staged outside the slots 0 .. RAW_TILE_DWORDS is raw_stage_holds' own bound, the writer's guard; here it is only held
// against the vectors' size.)
static void check_staging(uint64_t rows, uint32_t base) {
    const uint64_t blocks = raw_part_tiles(RAW_COLS_H, base, rows);
    std::vector<uint32_t> writes(RAW_TILE_DWORDS + 1);
    std::vector<long long> dword(RAW_TILE_DWORDS + 1);  // e * dpe + q of the slot's writer
    for (uint64_t block = 0; block < blocks; block++) {
        RawTile t;
        CHECK(raw_tile_locate(RAW_COLS_H, base, rows, block, &t), "rows %llu base %u: block %llu has no column", (unsigned long long)rows, base, (unsigned long long)block);
        const RawColDef& d = RAW_COLS_H[t.c];
        if (d.kind == RAW_K_DATE) continue;
        const uint32_t dpe = d.width >> 2;
        const long long bytes = (long long)(rows * d.width);
        const RawTilePhase ph = raw_tile_phase(base + t.off + raw_col_header_len(d), t.tile);
        std::fill(writes.begin(), writes.end(), 0u);
        const long long e0 = raw_stage_first(ph.k0, dpe);
        for (uint32_t j = 0; j < raw_stage_count(dpe); j++)
            for (uint32_t q = 0; q < dpe; q++) {
                const long long e = e0 + j, l = raw_stage_slot(e, dpe, q, ph.k0);
                if (!raw_stage_holds(l)) continue;  // (the writer's own guard: what it lets through must fit the vectors here)
                CHECK(l >= 0 && (size_t)l < writes.size(), "rows %llu base %u column %u tile %llu: slot %lld", (unsigned long long)rows, base, t.c, (unsigned long long)t.tile, l);
                writes[l]++;
                dword[l] = e >= 0 && e < (long long)rows ? e * dpe + q : -1;  // (an element outside the column stages zeroes)
            }
        for (uint32_t tid = 0; tid < RAW_BLOCK; tid++) {
            if (raw_chunk_outside(raw_lane_byte(ph.s, tid), bytes)) continue;
            for (uint32_t l = 4 * tid; l <= 4 * tid + 4; l++) {
                const long long k = ph.k0 + l;  // the column's dword the slot stands for: bytes 4 k .. 4 k + 3
                if (4 * k + 3 < 0 || 4 * k >= bytes) continue;
                CHECK(writes[l] == 1 && dword[l] == k, "rows %llu base %u column %u tile %llu: slot %u written %u times, by dword %lld, the column's is %lld", (unsigned long long)rows,
                      base, t.c, (unsigned long long)t.tile, l, writes[l], dword[l], k);
            }
        }
    }
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
    // ---- the tile walk and the staging over the merged row counts of the GPU test, at every address phase of the part's first byte
    for (uint32_t rows : {1u, 2u, 127u, 128u, 129u, 255u, 256u, 257u, 1023u, 1024u, 1025u, 16383u, 16384u})
        for (uint32_t base = 0; base < 16; base++) check_tiles(rows, base), check_staging(rows, base);
    printf("OK %llu\n", checks);
    return 0;
}
