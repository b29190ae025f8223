// host_raw_query_merge.hip - host instantiation of what the queries over the whole topic decide without a GPU (csrc/raw_query.cuh,
// csrc/merge.cuh): a record's key as the fold packs it, turned into the row a read hands out and back through the merge's key
// rebuild, is the identical TKey for every kind; the two row validations (raw_query_row_ok of a merge into a held result,
// query_row_producible of fa_rows_merge_device) against naive restatements over bytes; and the key words of RowOpsQuery against a
// memcmp-based comparator of the documented order.  TEST INFRASTRUCTURE (tests/test_raw_query_group_cpu.py).  No GPU call.
// Prints "OK <checks>" or the first failure and exits 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../flow-pipeline_amd/csrc/merge.cuh"
#include "../flow-pipeline_amd/csrc/raw_query.cuh"

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

static_assert(sizeof(fa_query_row) == sizeof(TalkRow) && sizeof(fa_raw_query_merge_stats_t) == 16, "the rows and the merge's statistics");
static_assert(FA_ROWS_QUERY_WEIGHT == RK_QUERY_WEIGHT && FA_ROWS_QUERY_KEY == RK_QUERY_KEY, "the row kinds");

// what a read hands out for the slot of key k (talker_rows_kernel's unpack; raw_query_scalar_rows_kernel for a scalar kind)
static TalkRow row_of_key(uint32_t kind, const TKey& k, uint64_t weight, uint64_t count) {
    TalkRow r{};
    tkey_unpack(k.w, r.key[0], r.key[1], r.etype);
    r.pad = 0, r.weight = weight, r.count = count;
    if (!raw_query_kind_is_addr(kind)) {
        const uint32_t v = raw_query_scalar_value(r.key[0]);
        r.key[0] = 0, r.key[1] = 0, r.etype = 0, r.pad = v;
    }
    return r;
}

// ---- 1: record -> key -> row -> key ------------------------------------------------------------------------------------------------
static void check_round_trip() {
    std::mt19937_64 rng(47);
    const uint32_t etypes[] = {0x800u, 0x86DDu, 0u, 0x1234u, 0x801u};
    const uint32_t edge[] = {0u, 1u, 59u, 60u, 255u, 256u, 65535u, 65536u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    for (int round = 0; round < 300000; round++) {
        const uint32_t kind = (uint32_t)(rng() % RAW_Q_KINDS);
        TKey k;
        if (raw_query_kind_is_addr(kind)) {
            uint64_t lo = round % 5 == 0 ? 0 : rng(), hi = round % 3 == 0 ? 0 : rng();
            raw_query_key_addr(kind, lo, hi, etypes[rng() % 5], k);
        } else {
            const uint32_t v = round % 4 == 0 ? edge[rng() % 11] : (uint32_t)rng();
            raw_query_key_scalar(kind, raw_query_scalar_of(kind, v), k);
        }
        const TalkRow r = row_of_key(kind, k, rng(), rng());
        CHECK(raw_query_row_ok(kind, r), "round %d: the row of kind %u's own key is refused", round, kind);
        CHECK(query_row_producible(r), "round %d: the row of kind %u's own key is no query row", round, kind);
        TKey back;
        raw_query_row_key(kind, r, back);
        CHECK(!memcmp(&back, &k, sizeof k), "round %d: kind %u's key does not come back", round, kind);
        CHECK(tkey_bucket(back.w) == kind && tkey_hash(back) == tkey_hash(k), "round %d: the kind or the hash of the rebuilt key", round);
    }
}

// ---- 2: the validations against naive restatements ---------------------------------------------------------------------------------
static bool naive_canonical(const uint8_t key[16], uint32_t etype) {
    if (etype == 0) return true;
    if (etype != 0x800) return false;
    for (int b = 4; b < 16; b++)
        if (key[b]) return false;
    return true;
}
static bool naive_zero_key(const uint8_t key[16]) {
    for (int b = 0; b < 16; b++)
        if (key[b]) return false;
    return true;
}
static bool naive_ok(uint32_t kind, const fa_query_row& r) {
    if (kind < 2) return r.value == 0 && naive_canonical(r.key, r.etype);
    if (!naive_zero_key(r.key) || r.etype != 0) return false;
    if (kind == RAW_Q_K_MINUTE) return r.value % 60 == 0;
    if (kind == RAW_Q_K_TOTAL) return r.value == 0;
    return true;
}
static bool naive_producible(const fa_query_row& r) {
    if (!naive_canonical(r.key, r.etype)) return false;
    return r.value == 0 || (naive_zero_key(r.key) && r.etype == 0);
}
static void check_validation() {
    std::mt19937_64 rng(48);
    const uint32_t etypes[] = {0u, 0x800u, 0x86DDu, 1u, 0x801u, 0x8000800u};
    unsigned long long ok_seen = 0, bad_seen = 0;
    for (int round = 0; round < 400000; round++) {
        fa_query_row q{};
        const int shape = (int)(rng() % 6);  // zero key, four bytes, one stray byte behind them, sixteen bytes
        if (shape >= 1)
            for (int b = 0; b < 4; b++) q.key[b] = (uint8_t)rng();
        if (shape == 2) q.key[4 + rng() % 12] = (uint8_t)(1 + rng() % 255);
        if (shape >= 4)
            for (int b = 4; b < 16; b++) q.key[b] = (uint8_t)rng();
        q.etype = etypes[rng() % (shape == 0 ? 3 : 6)];
        q.value = rng() % 3 == 0 ? 0u : rng() % 2 ? (uint32_t)(60 * (rng() % 1000)) : (uint32_t)rng();
        q.weight = rng(), q.count = rng();
        TalkRow r;
        memcpy(&r, &q, sizeof r);
        for (uint32_t kind = 0; kind < RAW_Q_KINDS; kind++) {
            const bool want = naive_ok(kind, q);
            CHECK(raw_query_row_ok(kind, r) == want, "round %d: kind %u, etype 0x%x, value %u: the merge's check", round, kind, q.etype, q.value);
            want ? ok_seen++ : bad_seen++;
        }
        CHECK(query_row_producible(r) == naive_producible(q), "round %d: etype 0x%x, value %u: the row kinds' check", round, q.etype, q.value);
    }
    CHECK(ok_seen > 100000 && bad_seen > 100000, "the generator makes both kinds of rows (%llu, %llu)", ok_seen, bad_seen);
}

// ---- 3: the key words against the documented order ------------------------------------------------------------------------------------
// FA_RAW_O_KEY: value ascending (numeric), key bytes ascending (memcmp), etype ascending; FA_RAW_O_WEIGHT: weight descending above it
static int naive_cmp_key(const fa_query_row& a, const fa_query_row& b) {
    if (a.value != b.value) return a.value < b.value ? -1 : 1;
    if (const int c = memcmp(a.key, b.key, 16)) return c < 0 ? -1 : 1;
    if (a.etype != b.etype) return a.etype < b.etype ? -1 : 1;
    return 0;
}
static int naive_cmp_weight(const fa_query_row& a, const fa_query_row& b) {
    if (a.weight != b.weight) return a.weight > b.weight ? -1 : 1;
    return naive_cmp_key(a, b);
}
static int words_cmp(const TalkRow& a, const TalkRow& b, bool by_weight) {
    if (by_weight && ~a.weight != ~b.weight) return ~a.weight < ~b.weight ? -1 : 1;  // (the talkers' fourth pass above the key words)
    for (int w = RowOpsQuery::NK - 1; w >= 0; w--) {  // (the most significant word last)
        unsigned long long x = RowOpsQuery::key(a, w, 0xffffffffu), y = RowOpsQuery::key(b, w, 0xffffffffu);
        if (RowOpsQuery::bits(w) < 64) {
            const unsigned long long m = (1ull << RowOpsQuery::bits(w)) - 1ull;
            x &= m, y &= m;
        }
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}
static void check_order() {
    std::mt19937_64 rng(49);
    const uint32_t values[] = {0u, 255u, 256u, 65535u, 65536u, 0x01000000u, 0xFFFFFFFFu};
    std::vector<fa_query_row> rows;
    for (int i = 0; i < 1500; i++) {
        fa_query_row q{};
        if (i % 2) {  // a scalar row
            q.value = values[rng() % 7];
        } else {  // an address row: few distinct bytes, so that prefixes, the family and single bytes decide
            for (int b = 0; b < 4; b++) q.key[b] = (uint8_t)(rng() % 3 ? 0x0A : rng() % 2 ? 0x00 : 0xFF);
            q.etype = rng() % 2 ? 0x800u : 0u;
            if (!q.etype)
                for (int b = 4; b < 16; b++) q.key[b] = (uint8_t)(rng() % 4 ? 0 : rng() % 2 ? 1 : 0x80);
        }
        q.weight = rng() % 4 ? rng() % 5 : rng();
        q.count = rng();
        rows.push_back(q);
    }
    for (size_t i = 0; i < rows.size(); i++)
        for (size_t j = 0; j < rows.size(); j += 1 + (i + j) % 3) {
            TalkRow a, b;
            memcpy(&a, &rows[i], sizeof a), memcpy(&b, &rows[j], sizeof b);
            CHECK(query_row_producible(a), "row %zu of the order's generator is no query row", i);
            CHECK(words_cmp(a, b, false) == naive_cmp_key(rows[i], rows[j]), "rows %zu, %zu: the key order", i, j);
            CHECK(words_cmp(a, b, true) == naive_cmp_weight(rows[i], rows[j]), "rows %zu, %zu: the weight order", i, j);
        }
    // the emit order's stand-in: a scalar's value in key bytes 4..7, most significant byte first, orders under the talkers' passes
    // (bytes 0..7 as a big-endian word) as the value does
    for (uint32_t a : values)
        for (uint32_t b : values) CHECK((bytes_order(bytes_order((unsigned long long)a)) < bytes_order(bytes_order((unsigned long long)b))) == (a < b), "the stand-in of %u and %u", a, b);
}

int main() {
    check_round_trip();
    check_validation();
    check_order();
    printf("OK %llu checks\n", checks);
    return 0;
}
