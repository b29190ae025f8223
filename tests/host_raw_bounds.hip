// host_raw_bounds.hip - host instantiation of what the pending doors decide without a GPU: the step arithmetic of raw_bounds_kernel
// (csrc/raw_bounds.cuh: raw_bounds_pos, raw_bounds_narrow, raw_bounds_lower - the very text the kernel runs, here with 64 simulated
// lanes) against std::lower_bound, with every load checked against the column's bytes and the column placed at byte phases 0 .. 3
// in a heap block of exactly the part's size, so that the sanitizer sees any read outside it; the step count against the stated
// bound; and the classification of csrc/raw_pending_plan.h against a naive scan of the rows.
// TEST INFRASTRUCTURE (tests/test_raw_pending_cpu.py).  No GPU call.  Prints "OK <checks>" or the first failure and exits 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../flow-pipeline_amd/csrc/raw_bounds.cuh"
#include "../flow-pipeline_amd/csrc/raw_pending_plan.h"

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

static_assert(sizeof(fa_raw_pending_stats_t) == 72 && sizeof(fa_raw_range) == 40, "the pending doors' structures");

// ---- 1: the search ------------------------------------------------------------------------------------------------------------------
// A sorted column as a part holds it: 4 * rows bytes at byte phase `phase`, alone in a heap block of exactly that size behind
// `phase` bytes (phase 0: the block IS the column, both ends are the block's).
struct Column {
    uint8_t* block = nullptr;
    const uint8_t* col = nullptr;
    uint64_t rows = 0;
    Column(const std::vector<uint32_t>& v, uint32_t phase) : rows(v.size()) {
        block = (uint8_t*)malloc(phase + 4 * v.size() + (phase + 4 * v.size() == 0));
        col = block + phase;
        if (!v.empty()) memcpy(block + phase, v.data(), 4 * v.size());
    }
    ~Column() { free(block); }
    // an element-width read at the element's own address: bytes [4 r, 4 r + 4) of the column
    uint32_t at(uint64_t r) const {
        CHECK(r < rows, "a load at row %llu of %llu", (unsigned long long)r, (unsigned long long)rows);
        uint32_t x;
        memcpy(&x, col + 4 * r, 4);
        return x;
    }
};

// the kernel's lower(from, key), its 64 lanes run one behind the other; every step's votes are checked to be a prefix of the lanes
static uint64_t lower_sim(const Column& c, uint64_t from, uint32_t key, uint32_t* steps) {
    return raw_bounds_lower(
        from, c.rows,
        [&](const RawBoundsIv& iv) {
            uint64_t ballot = 0, last = 0;
            bool any = false;
            for (uint32_t lane = 0; lane < 64; lane++) {
                bool valid;
                const uint64_t pos = raw_bounds_pos(iv, lane, &valid);
                if (!valid) continue;
                CHECK(pos >= iv.lo && pos < iv.hi, "lane %u probes %llu outside [%llu, %llu)", lane, (unsigned long long)pos, (unsigned long long)iv.lo, (unsigned long long)iv.hi);
                CHECK(!any || pos > last, "lane %u: the positions do not ascend", lane);
                any = true, last = pos;
                if (c.at(pos) < key) ballot |= (uint64_t)1 << lane;
            }
            CHECK((ballot & (ballot + 1)) == 0, "the votes are no prefix of the lanes");
            const RawBoundsIv o = raw_bounds_narrow(iv, ballot);
            CHECK(o.lo >= iv.lo && o.hi <= iv.hi && o.lo <= o.hi && o.hi - o.lo < iv.hi - iv.lo, "a step does not narrow the interval");
            return ballot;
        },
        steps);
}

// ceil(log65(rows)) + 1, in integers
static uint32_t stated_bound(uint64_t rows) {
    uint32_t k = 0;
    for (unsigned __int128 p = 1; p < rows; p *= 65) k++;
    return k + 1;
}

static void check_keys(const std::vector<uint32_t>& v, const std::vector<uint32_t>& keys, uint32_t phase) {
    const Column c(v, phase);
    for (uint32_t key : keys) {
        uint32_t steps = 0;
        const uint64_t got = lower_sim(c, 0, key, &steps);
        const uint64_t want = (uint64_t)(std::lower_bound(v.begin(), v.end(), key) - v.begin());
        CHECK(got == want, "rows %zu phase %u key %u: lower bound %llu, not %llu", v.size(), phase, key, (unsigned long long)got, (unsigned long long)want);
        CHECK(steps <= raw_bounds_max_steps(v.size()) && steps <= stated_bound(v.size()), "rows %zu key %u: %u steps", v.size(), key, steps);
        // the second bound of the kernel starts at the first: any upper key >= key gives the same answer as a search from 0
        const uint32_t up = key > 0xFFFFFFFFu - 3 ? 0xFFFFFFFFu : key + 3;
        uint32_t s2 = 0;
        const uint64_t hi = lower_sim(c, got, up, &s2);
        CHECK(hi == (uint64_t)(std::lower_bound(v.begin(), v.end(), up) - v.begin()), "rows %zu key %u: the upper bound from r_lo differs", v.size(), up);
    }
}

// below the minimum, at every distinct value (all of them up to `every`, a sample beyond), between two values, at the maximum,
// above it, 0xFFFFFFFF
static std::vector<uint32_t> keys_of(const std::vector<uint32_t>& v, size_t every, std::mt19937_64& rng) {
    std::vector<uint32_t> k{0u, 0xFFFFFFFFu, 0xFFFFFFFEu};
    if (v.empty()) return k;
    std::vector<uint32_t> d(v);
    d.erase(std::unique(d.begin(), d.end()), d.end());
    auto add = [&](uint32_t x) {
        k.push_back(x);
        if (x > 0) k.push_back(x - 1);
        if (x < 0xFFFFFFFFu) k.push_back(x + 1);
    };
    add(d.front()), add(d.back());
    if (d.size() <= every) {
        for (uint32_t x : d) add(x);
    } else {
        for (size_t i = 0; i < every; i++) add(d[rng() % d.size()]);
    }
    return k;
}

static std::vector<uint32_t> make_col(int shape, uint64_t rows, uint32_t base, std::mt19937_64& rng) {
    std::vector<uint32_t> v(rows);
    for (uint64_t i = 0; i < rows; i++) {
        switch (shape) {
        case 0: v[i] = base; break;                          // all equal
        case 1: v[i] = base + 2 * (uint32_t)i; break;        // strictly ascending, a gap between any two
        case 2: v[i] = base + 2 * (uint32_t)(i / 3); break;  // runs of 3
        case 3: v[i] = base + 2 * (uint32_t)(i / 70); break; // runs of 70
        default: v[i] = base + (uint32_t)(rng() % (rows / 2 + 2)) * 2;
        }
    }
    if (shape > 3) std::sort(v.begin(), v.end());
    return v;
}

static void check_search() {
    std::mt19937_64 rng(65);
    for (uint64_t rows = 0; rows <= 300; rows++)
        for (int shape = 0; shape < 5; shape++) {
            const std::vector<uint32_t> v = make_col(shape, rows, 1000, rng);
            const std::vector<uint32_t> keys = keys_of(v, 400, rng);
            for (uint32_t phase = 0; phase < 4; phase++) check_keys(v, keys, phase);
        }
    const uint64_t big[] = {4095, 4096, 4097, 4098, 4224, 4225, 4226, 262143, 262144, 262145, 262146};
    for (uint64_t rows : big)
        for (int shape = 0; shape < 5; shape++) {
            const std::vector<uint32_t> v = make_col(shape, rows, 77, rng);
            const std::vector<uint32_t> keys = keys_of(v, rows < 5000 ? 5000 : 300, rng);
            for (uint32_t phase = 0; phase < 4; phase++) check_keys(v, keys, phase);
        }
    // the ends of the axis: values at 0 and at 0xFFFFFFFF
    for (uint64_t rows : {1ull, 64ull, 65ull, 130ull, 4226ull}) {
        std::vector<uint32_t> v(rows, 0xFFFFFFFFu);
        for (uint64_t i = 0; i < rows / 2; i++) v[i] = i < rows / 4 ? 0u : 0xFFFFFFFEu;
        for (uint32_t phase = 0; phase < 4; phase++) check_keys(v, {0u, 1u, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu}, phase);
    }
    // the bound itself: 2^24 rows take four steps, and the two bounds agree where the text says they do
    CHECK(raw_bounds_max_steps(1u << 24) == 4 && raw_bounds_max_steps(0) == 0 && raw_bounds_max_steps(1) == 1 && raw_bounds_max_steps(64) == 1 && raw_bounds_max_steps(65) == 2,
          "raw_bounds_max_steps");
    for (uint64_t rows = 0; rows < 300000; rows += 1 + rows / 97) CHECK(raw_bounds_max_steps(rows) <= stated_bound(rows), "the step bound at %llu rows", (unsigned long long)rows);
    CHECK(raw_bounds_max_steps(0xFFFFFFFFull) <= stated_bound(0xFFFFFFFFull), "the step bound at 2^32 - 1 rows");
}

// ---- 2: the classification ---------------------------------------------------------------------------------------------------------
static bool naive_in_range(uint32_t t, uint32_t lo, uint32_t hi) { return t >= lo && (hi == 0xFFFFFFFFu || t < hi); }

static void check_class_of(const std::vector<uint32_t>& v, uint32_t lo, uint32_t hi) {
    if (lo > hi) return;
    uint64_t in = 0;
    for (uint32_t t : v) in += naive_in_range(t, lo, hi);
    const int cls = raw_pending_class(v.size(), v.front(), v.back(), lo, hi);
    if (cls == RAW_PENDING_SKIPPED) CHECK(in == 0, "skipped, but %llu rows are in [%u, %u)", (unsigned long long)in, lo, hi);
    else if (cls == RAW_PENDING_WHOLE) CHECK(in == v.size(), "whole, but %llu of %zu rows are in [%u, %u)", (unsigned long long)in, v.size(), lo, hi);
    else CHECK(cls == RAW_PENDING_SEARCHED && in < v.size(), "searched, but every row is in [%u, %u)", lo, hi);
    // no search where the host could have known: a range that ends at or below the first value, or starts above the last
    if (hi != 0xFFFFFFFFu && hi <= v.front()) CHECK(cls == RAW_PENDING_SKIPPED, "a range below the part is not skipped");
    if (lo > v.back()) CHECK(cls == RAW_PENDING_SKIPPED, "a range above the part is not skipped");
    if (lo == hi && hi != 0xFFFFFFFFu) CHECK(cls == RAW_PENDING_SKIPPED && in == 0, "t_lo == t_hi selects a row");
    // and the two positions a search would deliver are the naive ones
    if (cls == RAW_PENDING_SEARCHED) {
        const Column c(v, 1);
        uint32_t steps = 0;
        const uint64_t r_lo = lower_sim(c, 0, lo, &steps), r_hi = hi == 0xFFFFFFFFu ? v.size() : lower_sim(c, r_lo, hi, &steps);
        CHECK(r_hi - r_lo == in, "[%u, %u): rows [%llu, %llu), %llu in range", lo, hi, (unsigned long long)r_lo, (unsigned long long)r_hi, (unsigned long long)in);
    }
}

static void check_class() {
    std::mt19937_64 rng(66);
    CHECK(raw_pending_class(0, 0, 0, 0, 0xFFFFFFFFu) == RAW_PENDING_SKIPPED, "a part without rows");
    std::vector<std::vector<uint32_t>> cols;
    cols.push_back({500});
    cols.push_back({500, 500, 500});
    cols.push_back({500, 501, 501, 504, 504, 510});
    cols.push_back({0, 0, 1, 5});
    cols.push_back({0xFFFFFFF0u, 0xFFFFFFFEu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu});
    cols.push_back({0xFFFFFFFFu, 0xFFFFFFFFu});
    cols.push_back({0xFFFFFFFEu});
    cols.push_back({0, 0xFFFFFFFFu});
    for (int i = 0; i < 20; i++) cols.push_back(make_col(4, 1 + rng() % 200, 100, rng));
    for (const std::vector<uint32_t>& v : cols) {
        std::vector<uint32_t> edges{0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu};
        for (uint32_t t : v)
            for (int d = -1; d <= 1; d++)
                if (!(t == 0 && d < 0) && !(t == 0xFFFFFFFFu && d > 0)) edges.push_back(t + d);
        std::sort(edges.begin(), edges.end());
        edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
        for (uint32_t lo : edges)
            for (uint32_t hi : edges) check_class_of(v, lo, hi);
    }
    // to the end includes the last second; one below excludes it
    CHECK(raw_pending_class(2, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFFu) == RAW_PENDING_WHOLE, "NO_UPPER over rows at the last second");
    CHECK(raw_pending_class(2, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFEu) == RAW_PENDING_SKIPPED, "t_hi below the last second");
    CHECK(raw_pending_class(3, 7, 0xFFFFFFFFu, 7, 0xFFFFFFFEu) == RAW_PENDING_SEARCHED, "a part that ends at the last second under t_hi below it");
}

int main() {
    check_search();
    check_class();
    printf("OK %llu checks\n", checks);
    return 0;
}
