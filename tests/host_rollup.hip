// host_rollup.hip - host instantiation of what the rollup fold decides without a GPU: the slice geometry of rollup_fold_kernel
// (csrc/rollup.cuh: rollup_rounds / rollup_first, the text the kernel runs), the chunk bound and the key-set mask check of
// csrc/rollup_plan.h.  TEST INFRASTRUCTURE (tests/test_rollup_cpu.py).  No GPU call.  Prints "OK <checks>" or the first failure
// and exits 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../flow-pipeline_amd/csrc/rollup.cuh"
#include "../flow-pipeline_amd/csrc/rollup_plan.h"

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

// every record index in [0, m) is visited exactly once; the trip count is one number for the whole grid (so all 64 lanes of a
// wave, and all waves, share it); a wave's lanes take 64 consecutive records
static void check_slices(uint32_t m, uint32_t grid) {
    std::vector<uint8_t> seen(m, 0);
    const uint32_t rounds = rollup_rounds(m, grid);
    CHECK((uint64_t)rounds * grid * ROLLUP_WAVES * 64u >= m, "m %u grid %u: %u rounds do not cover the chunk", m, grid, rounds);
    CHECK(rounds == 0 || (uint64_t)(rounds - 1) * grid * ROLLUP_WAVES * 64u < m, "m %u grid %u: %u rounds, the last one is empty", m, grid, rounds);
    CHECK((m == 0) == (rounds == 0), "m %u grid %u: %u rounds", m, grid, rounds);
    for (uint32_t g = 0; g < grid; g++)
        for (uint32_t w = 0; w < (uint32_t)ROLLUP_WAVES; w++)
            for (uint32_t r = 0; r < rounds; r++) {  // (the kernel's loop: the same bound for every (g, w, lane))
                const uint64_t first = rollup_first(g, w, r, grid);
                CHECK(first % 64u == 0, "m %u grid %u: wave (%u, %u) round %u starts at %llu", m, grid, g, w, r, (unsigned long long)first);
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint64_t at = first + lane;
                    if (at >= m) continue;  // valid = false: the lane still makes the round
                    CHECK(!seen[at], "m %u grid %u: record %llu is visited twice", m, grid, (unsigned long long)at);
                    seen[at] = 1;
                }
            }
    for (uint32_t i = 0; i < m; i++) CHECK(seen[i], "m %u grid %u: record %u is never visited", m, grid, i);
}

// the worst case one chunk can park fits both spill buffers, and a chunk is never empty
static void check_chunks() {
    const uint32_t caps[] = {4, 5, 63, 1000, (1u << 20) - 1, 1u << 20, (1u << 21), (1u << 21) + 1, (1u << 21) + 4, 3u << 20, (1u << 25), 2u * ((1u << 25) - 1) + (1u << 21), 0xFFFFFFFFu};
    const uint32_t batches[] = {0, 1, 2, 1000, 1u << 20, 1u << 24, (1u << 25) - 1};
    for (uint32_t ks = 0; ks < 64; ks++) {
        if (ks & ROLLUP_SKETCH_SETS) continue;
        for (uint32_t sc : caps)
            for (uint32_t wc : caps)
                for (uint32_t mb : batches) {
                    const size_t m = rollup_chunk_cap(sc, wc, mb, ks);
                    CHECK(m >= 1, "ks %u caps %u %u batch %u: an empty chunk", ks, sc, wc, mb);
                    CHECK(m <= (mb ? mb : 1u), "ks %u caps %u %u batch %u: chunk %zu above max_batch_records", ks, sc, wc, mb, m);
                    CHECK((uint64_t)m * rollup_as_updates(ks) <= sc, "ks %u caps %u %u batch %u: chunk %zu parks more than spill_cap", ks, sc, wc, mb, m);
                    CHECK((uint64_t)m * rollup_wide_updates(ks) <= wc, "ks %u caps %u %u batch %u: chunk %zu parks more than wspill_cap", ks, sc, wc, mb, m);
                }
    }
    // the updates per record, from the key sets: a dense-miss record with both ports >= 65536 makes four wide updates
    CHECK(rollup_wide_updates(ROLLUP_EXACT_SETS) == 4 && rollup_wide_updates(FA_KEYS_PORT_HIST) == 2 && rollup_wide_updates(FA_KEYS_AS_PAIR) == 0, "wide updates per record");
    CHECK(rollup_as_updates(FA_KEYS_AS_PAIR) == 1 && rollup_as_updates(FA_KEYS_WIDE) == 0, "flows_5m updates per record");
    // a ctx's own buffers (fa_create's sizes at the default batch): a chunk leaves the guard's 2^20 entries free
    const uint32_t mb = 1u << 24, sc = 2u * mb + (1u << 21), wc = 1u << 25;
    CHECK(rollup_chunk_cap(sc, wc, mb, FA_KEYS_AS_PAIR) == mb, "flows_5m alone: a chunk of max_batch_records");
    CHECK(rollup_chunk_cap(sc, wc, mb, ROLLUP_EXACT_SETS) * 4 + (1u << 20) <= wc, "all four: the guard's slack stays free");
}

static void check_masks() {
    for (uint32_t ctx = 0; ctx < 64; ctx++)
        for (uint32_t asked = 0; asked < 256; asked++) {
            uint32_t out = 0xdeadbeefu;
            const int rc = rollup_mask_check(ctx, asked, &out);
            const uint32_t have = ctx & ROLLUP_EXACT_SETS;
            int want = FA_OK;
            if (asked & ROLLUP_SKETCH_SETS) want = FA_ERR_UNSUPPORTED;  // (whether or not the ctx has the sketch)
            else if (asked & ~have) want = FA_ERR_ARG;                  // a foreign bit, bits above the six included
            else if (!have) want = FA_ERR_UNSUPPORTED;                  // nothing to fold into
            CHECK(rc == want, "ctx %u asked %u: %d, want %d", ctx, asked, rc, want);
            if (rc == FA_OK) CHECK(out == (asked ? asked : have) && out != 0 && !(out & ~have), "ctx %u asked %u: folds %u", ctx, asked, out);
            else CHECK(out == 0, "ctx %u asked %u: refused, but folds %u", ctx, asked, out);
        }
}

int main() {
    const uint32_t rows[] = {0, 1, 63, 64, 65, 255, 256, 257, 3 * 256 - 1, 3 * 256, 3 * 256 + 1, 2 * 3 * 256 + 65, (1u << 18) + 1};
    const uint32_t grids[] = {1, 3, 512};
    for (uint32_t m : rows)
        for (uint32_t g : grids) check_slices(m, g);
    check_slices(1u << 25, 1024);  // the largest chunk a ctx folds (max_batch_records < 2^25) on a full grid
    CHECK(rollup_rounds((1u << 25) - 1, 1) == (1u << 17), "one workgroup walks 2^25 - 1 records in 2^17 rounds");
    check_chunks();
    check_masks();
    printf("OK %llu\n", checks);
    return 0;
}
