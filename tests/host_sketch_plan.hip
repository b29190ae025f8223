// host_sketch_plan.hip - host instantiation of what the sketch fold and the restore decide without a GPU (csrc/sketch_plan.h): which
// key sets a call may ask for (sketch_mask_check, restore_mask_check) and how long a chunk may be (sketch_chunk_cap,
// restore_chunk_cap); and the LDS cache's key layout (csrc/sketch_fold.cuh: sketch_words / sketch_unwords, the text the kernel
// runs).  TEST INFRASTRUCTURE (tests/test_sketch_plan_cpu.py).  No GPU call.  Prints "OK <checks>" or the first failure and exits 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "../flow-pipeline_amd/csrc/sketch_fold.cuh"
#include "../flow-pipeline_amd/csrc/sketch_plan.h"

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

constexpr uint32_t EXACT = FA_KEYS_AS_PAIR | FA_KEYS_ADDR_PORT_PROTO | FA_KEYS_PORT_HIST | FA_KEYS_MINUTE_SERIES;
constexpr uint32_t SKETCH = FA_KEYS_SRCADDR_CMS | FA_KEYS_DSTADDR_CMS;

// the truth table of the feature's description, written out here: asked == 0 is every sketch of the ctx; an exact bit, a sketch
// the ctx lacks or a bit above the six is FA_ERR_ARG; a ctx without any sketch has nothing to fold into (FA_ERR_UNSUPPORTED)
static void check_sketch_masks() {
    for (uint32_t created = 0; created < 64; created++)
        for (uint32_t asked = 0; asked < 256; asked++) {
            uint32_t out = 0xdeadbeefu;
            const int rc = sketch_mask_check(created, asked, &out);
            const uint32_t have = created & SKETCH;
            int want = FA_OK;
            if (asked & ~have) want = FA_ERR_ARG;
            else if (!have) want = FA_ERR_UNSUPPORTED;  // (asked == 0 is all that is left here)
            CHECK(rc == want, "created %u asked %u: %d, want %d", created, asked, rc, want);
            if (rc == FA_OK) CHECK(out == (asked ? asked : have) && out != 0 && !(out & ~have), "created %u asked %u: folds %u", created, asked, out);
            else CHECK(out == 0, "created %u asked %u: refused, but folds %u", created, asked, out);
        }
}

static void check_restore_masks() {
    for (uint32_t created = 0; created < 64; created++)
        for (uint32_t asked = 0; asked < 256; asked++) {
            uint32_t ex = 0xdeadbeefu, sk = 0xdeadbeefu;
            const int rc = restore_mask_check(created, asked, &ex, &sk);
            const int want = (asked & ~created) ? FA_ERR_ARG : FA_OK;
            CHECK(rc == want, "restore: created %u asked %u: %d, want %d", created, asked, rc, want);
            const uint32_t take = rc ? 0u : (asked ? asked : created);
            CHECK(ex == (take & EXACT) && sk == (take & SKETCH), "restore: created %u asked %u: exact %u sketches %u", created, asked, ex, sk);
            CHECK((ex | sk) == take && !(ex & sk), "restore: created %u asked %u: the halves do not make the selection", created, asked);
        }
}

static void check_chunks() {
    const uint32_t batches[] = {0, 1, 2, 1000, 1u << 20, 1u << 24, (1u << 25) - 1};
    for (uint32_t mb : batches) {
        const size_t m = sketch_chunk_cap(mb);
        CHECK(m >= 1 && m == (mb ? mb : 1u), "batch %u: sketch chunk %zu", mb, m);
    }
    // the restore's chunk: the minimum over the selected destinations (0 = not selected); 0 only when none is
    const size_t caps[] = {0, 1, 2, 1000, 4096, (size_t)1 << 20, (size_t)1 << 24, ((size_t)1 << 25) - 1};
    for (size_t r : caps)
        for (size_t s : caps)
            for (size_t t : caps)
                for (size_t p : caps) {
                    const size_t m = restore_chunk_cap(r, s, t, p);
                    size_t want = 0;
                    for (size_t cap : {r, s, t, p})
                        if (cap && (!want || cap < want)) want = cap;
                    CHECK(m == want, "caps %zu %zu %zu %zu: chunk %zu, want %zu", r, s, t, p, m, want);
                    CHECK((m == 0) == (!r && !s && !t && !p), "caps %zu %zu %zu %zu: chunk %zu", r, s, t, p, m);
                    for (size_t cap : {r, s, t, p}) CHECK(!cap || m <= cap, "caps %zu %zu %zu %zu: chunk %zu above a selected cap", r, s, t, p, m);
                }
}

// the cache's key words: never 0 (0 is EMPTY), and a bijection - the all-zero address is a key like any other
static void check_words() {
    const uint64_t v[] = {0, 1, 2, 3, 1ull << 63, (1ull << 63) | 1, ~0ull, ~0ull - 1, 0x0123456789abcdefull, 0x8000000000000001ull};
    for (uint64_t lo : v)
        for (uint64_t hi : v) {
            unsigned long long k[3];
            sketch_words(lo, hi, k);
            CHECK(k[0] != 0 && k[1] != 0 && k[2] != 0, "key %llx %llx: an EMPTY word", (unsigned long long)lo, (unsigned long long)hi);
            uint64_t l2, h2;
            sketch_unwords(k, l2, h2);
            CHECK(l2 == lo && h2 == hi, "key %llx %llx comes back as %llx %llx", (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)l2, (unsigned long long)h2);
            CHECK(sketch_slot(lo, hi) < (uint32_t)SKETCH_ENTRIES, "key %llx %llx: slot out of the cache", (unsigned long long)lo, (unsigned long long)hi);
            for (uint64_t lo2 : v)
                for (uint64_t hi2 : v) {
                    unsigned long long q[3];
                    sketch_words(lo2, hi2, q);
                    const bool same = q[0] == k[0] && q[1] == k[1] && q[2] == k[2];
                    CHECK(same == (lo == lo2 && hi == hi2), "keys %llx %llx and %llx %llx share their words", (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)lo2, (unsigned long long)hi2);
                }
        }
}

int main() {
    check_sketch_masks();
    check_restore_masks();
    check_chunks();
    check_words();
    printf("OK %llu\n", checks);
    return 0;
}
