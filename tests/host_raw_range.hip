// host_raw_range.hip - host instantiation of what a ranged load of flows_raw parts decides without a GPU (csrc/raw_range_plan.h): the
// three stage sets of blocks, the element predicate of raw_range_kernel and the kernel's load geometry - against every address
// raw_unpack_kernel and raw_range_kernel load (raw_unpack_kernel's arithmetic is restated here line by line from csrc/raw.cuh; the
// range kernel's is the text the kernel runs).  TEST INFRASTRUCTURE (tests/test_raw_range_cpu.py).  No GPU call.
// Prints "OK <checks>" or the first failure and exits 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

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

constexpr uint64_t IMG = 0x7f0000000000ull + 256 * 5;  // where the image lies: 256-byte aligned, as hipMalloc gives it
constexpr uint32_t FIRST = 3;                          // the part's first block of the call

struct Part {
    uint64_t rows, bytes, base;  // base: the part's first byte (a slot: 64 KiB from the image's start on)
    uint32_t nblocks;
    std::vector<uint8_t> planned;  // per block of the call: some stage decodes it
};

// the address a lies in a planned block, and inside the part
static bool in_planned(const Part& p, uint64_t a, uint64_t len) {
    if (a < p.base || a + len > p.base + p.bytes) return false;
    for (uint64_t x = a; x < a + len; x++) {  // (a 16-byte aligned word never straddles a slot: the image is 16-byte aligned)
        const uint64_t b = (x - IMG) / RAW_SLOT;
        if (b >= p.planned.size() || !p.planned[b]) return false;
    }
    return true;
}

// every address raw_unpack_kernel loads for rows [r0, r0 + m) of column c (csrc/raw.cuh, restated): `fn(address, bytes)`
template <class F>
static void unpack_loads(const Part& p, uint32_t c, uint64_t r0, uint64_t m, F fn) {
    const RawColDef& d = RAW_COLS_H[c];
    const uint32_t w = d.width;
    const bool widen = d.kind == RAW_K_KEY || d.kind == RAW_K_NARROW64;
    const uint64_t d0 = 0x7e0000000000ull;  // (the ctx's column chunk: 256-byte aligned arrays, filled from element 0)
    const uint64_t d1 = d0 + m * (widen ? 8 : w);
    const uint64_t lo = p.base, hi = p.base + p.bytes;
    const uint64_t s0 = p.base + raw_col_offset(RAW_COLS_H, p.rows, c) + raw_col_header_len(d) + r0 * w;
    for (uint64_t idx = 0;; idx++) {
        const uint64_t t = d0 - (d0 & 15) + 16 * idx;
        if (t >= d1) break;
        const bool whole = t >= d0 && t + 16 <= d1;
        const uint32_t nsrc = widen ? 8 : 16;
        const uint64_t s = s0 + (widen ? (t - d0) / 2 : (t - d0));
        const uint32_t sh = (uint32_t)(s & 15);
        const uint64_t al = s - sh;
        const bool two = sh + nsrc > 16;
        if (whole && al >= lo && al + (two ? 32 : 16) <= hi) {
            fn(al, 16);
            if (two) fn(al + 16, 16);
            continue;
        }
        if (!widen) {
            for (int i = 0; i < 16; i++)
                if (t + i >= d0 && t + i < d1) fn(s + i, 1);
        } else {
            for (int i = 0; i < 8; i++)
                if (t + 2 * (i & 4) >= d0 && t + 2 * (i & 4) < d1) fn(s + i, 1);
        }
    }
}

// every address raw_range_kernel loads over the part's TimeReceived column; -> the elements the groups own, each once
static void range_loads(const Part& p) {
    const uint64_t col = p.base + raw_col_offset(RAW_COLS_H, p.rows, RAW_COL_TIME) + raw_col_header_len(RAW_COLS_H[RAW_COL_TIME]);
    const uint64_t tiles = raw_range_tiles(p.rows);
    CHECK(tiles * RAW_RANGE_TILE >= p.rows && (tiles == 0 || (tiles - 1) * RAW_RANGE_TILE < p.rows), "rows %llu: %llu tiles", (unsigned long long)p.rows, (unsigned long long)tiles);
    uint64_t owned = 0, next_group = 0;
    for (uint64_t tile = 0; tile < tiles; tile++)
        for (uint32_t k = 0; k < RAW_RANGE_ITERS; k++)
            for (uint32_t tid = 0; tid < RAW_RANGE_BLOCK; tid++) {
                const uint64_t g = raw_range_group(tile, k, tid);
                CHECK(g == next_group, "rows %llu: group %llu follows %llu", (unsigned long long)p.rows, (unsigned long long)g, (unsigned long long)next_group);
                next_group++;
                if (4 * g >= p.rows) continue;
                const uint64_t nv = std::min<uint64_t>(4, p.rows - 4 * g);
                owned += nv;
                const RawRangeLoad l = raw_range_load(col, g, p.rows, p.base, p.base + p.bytes);
                if (l.wide) {
                    CHECK(nv == 4 && l.al % 16 == 0 && l.sh == (col & 15), "rows %llu group %llu: a wide load of a partial group or off its phase", (unsigned long long)p.rows, (unsigned long long)g);
                    for (uint32_t wd = 0; wd < l.words; wd++) {
                        const uint64_t a = l.al + 16 * wd;
                        CHECK(a + 16 > col + 16 * g && a < col + 16 * g + 16, "rows %llu group %llu: word %u holds no byte of the group", (unsigned long long)p.rows, (unsigned long long)g, wd);
                        CHECK(in_planned(p, a, 16), "rows %llu group %llu: word %u is not in a planned block of the part", (unsigned long long)p.rows, (unsigned long long)g, wd);
                    }
                } else {
                    CHECK(in_planned(p, col + 16 * g, 4 * nv), "rows %llu group %llu: byte path outside the planned blocks", (unsigned long long)p.rows, (unsigned long long)g);
                }
                if ((tid & 63) == 63 && 4 * g + 4 < p.rows)  // a wave's last lane reads its successor
                    CHECK(in_planned(p, col + 16 * g + 16, 4), "rows %llu group %llu: the successor read leaves the planned blocks", (unsigned long long)p.rows, (unsigned long long)g);
            }
    CHECK(owned == p.rows, "rows %llu: the groups own %llu elements", (unsigned long long)p.rows, (unsigned long long)owned);
}

static bool span_meets_block(const RawByteSpan* sp, uint32_t n, uint64_t b) {
    for (uint32_t i = 0; i < n; i++)
        if (sp[i].lo < sp[i].hi && sp[i].lo < (b + 1) * RAW_SLOT && sp[i].hi > b * RAW_SLOT) return true;
    return false;
}

static void check_rows(uint64_t rows, bool dense) {
    Part p;
    p.rows = rows;
    p.bytes = raw_col_offset(RAW_COLS_H, rows, RAW_NCOLS);
    uint64_t back = 0;
    CHECK(raw_rows_from_bytes(RAW_COLS_H, p.bytes, &back) && back == rows, "rows %llu: the size does not give the rows back", (unsigned long long)rows);
    p.nblocks = (uint32_t)((p.bytes + RAW_SLOT - 1) / RAW_SLOT);
    p.base = IMG + FIRST * RAW_SLOT;
    const size_t call_blocks = FIRST + p.nblocks + 2;
    std::vector<uint8_t> done(call_blocks, 0);
    std::vector<uint32_t> a, b;
    raw_range_probe_blocks(FIRST, p.nblocks, done, a);
    CHECK(a.size() == (p.nblocks > 1 ? 2u : 1u) && a[0] == FIRST && a.back() == FIRST + p.nblocks - 1, "rows %llu: stage A is not the first and last block", (unsigned long long)rows);
    raw_range_scan_blocks(RAW_COLS_H, rows, FIRST, p.nblocks, done, b);
    RawByteSpan sb[RAW_NCOLS + 2];
    const uint32_t nsb = raw_range_scan_spans(RAW_COLS_H, rows, sb);
    for (uint32_t x : b) CHECK(x >= FIRST && x < FIRST + p.nblocks && span_meets_block(sb, nsb, x - FIRST), "rows %llu: stage B plans block %u without a needed byte", (unsigned long long)rows, x);
    for (uint32_t x : b) CHECK(std::find(a.begin(), a.end(), x) == a.end(), "rows %llu: block %u in stages A and B", (unsigned long long)rows, x);
    // stages A + B: every header byte, every TimeReceived byte, every load of the range kernel
    p.planned = done;
    for (uint32_t i = 0; i < nsb; i++)
        for (uint64_t x = sb[i].lo; x < sb[i].hi; x += (sb[i].hi - sb[i].lo > 64 ? 7 : 1)) CHECK(in_planned(p, p.base + x, 1), "rows %llu: byte %llu of stage B's spans is not planned", (unsigned long long)rows, (unsigned long long)x);
    for (uint32_t i = 0; i < nsb; i++)
        if (sb[i].hi > sb[i].lo) CHECK(in_planned(p, p.base + sb[i].hi - 1, 1), "rows %llu: the last byte of span %u is not planned", (unsigned long long)rows, i);
    CHECK(sb[nsb - 1].hi - sb[nsb - 1].lo == 4 * rows, "rows %llu: the TimeReceived span", (unsigned long long)rows);
    range_loads(p);
    // stage C over a grid of slices
    std::set<uint64_t> pts = {0, rows};
    const uint64_t cand[] = {1, 3, 4, 5, 8, rows / 3, rows / 2, rows / 2 + 1, rows - 5, rows - 4, rows - 1};
    const uint64_t few[] = {1, 5, rows / 3, rows / 2 + 1, rows - 4, rows - 1};
    if (dense) {
        for (uint64_t x : cand)
            if (x <= rows) pts.insert(x);
    } else {
        for (uint64_t x : few)
            if (x <= rows) pts.insert(x);
    }
    for (uint64_t r_lo : pts)
        for (uint64_t r_hi : pts) {
            if (r_lo > r_hi) continue;
            std::vector<uint8_t> d2 = done;
            std::vector<uint32_t> cl;
            raw_range_load_blocks(RAW_COLS_H, rows, FIRST, p.nblocks, r_lo, r_hi, d2, cl);
            RawByteSpan sc[RAW_NCOLS];
            const uint32_t nsc = raw_range_load_spans(RAW_COLS_H, rows, r_lo, r_hi, sc);
            CHECK(nsc == RAW_NCOLS - 2, "14 columns behind TimeReceived");
            std::set<uint32_t> seen;
            for (uint32_t x : cl) {
                CHECK(x >= FIRST && x < FIRST + p.nblocks && span_meets_block(sc, nsc, x - FIRST), "rows %llu [%llu, %llu): stage C plans block %u without a needed byte", (unsigned long long)rows,
                      (unsigned long long)r_lo, (unsigned long long)r_hi, x);
                CHECK(!done[x], "rows %llu [%llu, %llu): block %u in stage C and in an earlier stage", (unsigned long long)rows, (unsigned long long)r_lo, (unsigned long long)r_hi, x);
                CHECK(seen.insert(x).second, "rows %llu: block %u twice in stage C", (unsigned long long)rows, x);
            }
            if (r_lo == r_hi) CHECK(cl.empty(), "rows %llu: an empty slice plans blocks", (unsigned long long)rows);
            p.planned = d2;
            for (uint32_t c = 1; c < RAW_NCOLS; c++)
                unpack_loads(p, c, r_lo, r_hi - r_lo, [&](uint64_t at, uint64_t len) {
                    CHECK(in_planned(p, at, len), "rows %llu [%llu, %llu) column %u: raw_unpack_kernel loads %llu bytes at part byte %lld outside the planned blocks", (unsigned long long)rows,
                          (unsigned long long)r_lo, (unsigned long long)r_hi, c, (unsigned long long)len, (long long)(at - p.base));
                });
        }
    for (uint8_t x : std::vector<uint8_t>(done.begin(), done.begin() + FIRST)) CHECK(!x, "a block in front of the part is planned");
    CHECK(!done[FIRST + p.nblocks] && !done[FIRST + p.nblocks + 1], "a block behind the part is planned");
}

// the kernel's sums over a column, element by element
struct Rec {
    uint64_t r_lo = 0, r_hi = 0, desc = RAW_RANGE_NONE, offd = RAW_RANGE_NONE;
    uint32_t tmin = 0xFFFFFFFFu, tmax = 0;
};
static Rec scan(const std::vector<uint32_t>& t, uint32_t t_lo, uint32_t t_hi, uint32_t date) {
    Rec r;
    for (size_t i = 0; i < t.size(); i++) {
        const RawRangeElem e = raw_range_elem(t[i], i + 1 < t.size() ? t[i + 1] : 0xdeadbeefu, i + 1 < t.size(), t_lo, t_hi, date);
        r.r_lo += e.below_lo, r.r_hi += e.below_hi;
        if (e.descends) r.desc = std::min<uint64_t>(r.desc, i);
        if (e.off_date) r.offd = std::min<uint64_t>(r.offd, i);
        if (e.selected) r.tmin = std::min(r.tmin, t[i]), r.tmax = std::max(r.tmax, t[i]);
    }
    return r;
}
static void check_predicate() {
    std::mt19937 rng(12345);
    for (int round = 0; round < 400; round++) {
        const uint32_t date = round % 7 == 0 ? 49710u : (round % 5 == 0 ? 0u : 19000u + rng() % 3);
        const uint64_t d0 = (uint64_t)date * 86400;
        const uint32_t span = date == 49710u ? 0xFFFFFFFFu - (uint32_t)d0 + 1 : 86400u;  // the last Date of the axis is cut short
        const size_t n = rng() % 200;
        std::vector<uint32_t> t(n);
        for (auto& x : t) x = (uint32_t)(d0 + rng() % std::min<uint32_t>(span, round % 3 ? 50u : span));  // runs of equal times
        std::sort(t.begin(), t.end());
        const bool sorted = round % 4 != 3;
        if (!sorted && n >= 2) std::swap(t[rng() % n], t[rng() % n]);
        uint32_t bounds[] = {0u, 0xFFFFFFFFu, (uint32_t)d0, (uint32_t)(d0 + span - 1), n ? t[0] : 5u, n ? t[n - 1] : 6u, n ? t[n / 2] : 7u, n ? t[n / 2] + 1 : 8u, n ? t[n / 2] - 1 : 9u,
                             (uint32_t)(d0 + rng() % span)};
        for (uint32_t lo : bounds)
            for (uint32_t hi : bounds) {
                if (lo > hi) continue;
                const Rec r = scan(t, lo, hi, date);
                size_t first_desc = RAW_RANGE_NONE;
                for (size_t i = 0; i + 1 < n; i++)
                    if (t[i] > t[i + 1]) {
                        first_desc = i;
                        break;
                    }
                CHECK(r.desc == first_desc, "round %d: first descent %llu, want %zu", round, (unsigned long long)r.desc, first_desc);
                CHECK(r.offd == RAW_RANGE_NONE, "round %d: a row of the part's Date is off it", round);
                if (first_desc != RAW_RANGE_NONE) continue;
                const uint64_t want_lo = std::lower_bound(t.begin(), t.end(), lo) - t.begin();
                const uint64_t want_hi = hi == 0xFFFFFFFFu ? n : std::lower_bound(t.begin(), t.end(), hi) - t.begin();
                CHECK(r.r_lo == want_lo && r.r_hi == want_hi, "round %d [%u, %u): rows [%llu, %llu), want [%llu, %llu)", round, lo, hi, (unsigned long long)r.r_lo, (unsigned long long)r.r_hi,
                      (unsigned long long)want_lo, (unsigned long long)want_hi);
                if (want_lo < want_hi) CHECK(r.tmin == t[want_lo] && r.tmax == t[want_hi - 1], "round %d: t_min / t_max of the selection", round);
                else CHECK(r.tmin == 0xFFFFFFFFu && r.tmax == 0, "round %d: an empty selection has extrema", round);
                // pruning never drops a part that holds a selected row
                if (want_lo < want_hi) CHECK(raw_range_date_meets(date, lo, hi), "round %d [%u, %u): the part's Date is pruned", round, lo, hi);
            }
        // a row of another Date is found, at its row
        if (n && date != 49710u) {
            const size_t at = rng() % n;
            std::vector<uint32_t> u = t;
            u[at] = (uint32_t)(d0 + 86400 + 5);
            const Rec r = scan(u, 0, 0xFFFFFFFFu, date);
            size_t first = 0;
            while (u[first] / 86400 == date) first++;
            CHECK(r.offd == first, "round %d: the row of another Date is %llu, want %zu", round, (unsigned long long)r.offd, first);
        }
    }
    // pruning against the definition
    for (uint32_t date : {0u, 1u, 19000u, 49709u, 49710u})
        for (uint64_t lo64 : {0ull, 86399ull, 86400ull, 19000ull * 86400 - 1, 19000ull * 86400, 19000ull * 86400 + 86399, 19000ull * 86400 + 86400, 0xFFFFFFFEull, 0xFFFFFFFFull})
            for (uint64_t hi64 : {0ull, 1ull, 86400ull, 86401ull, 19000ull * 86400, 19000ull * 86400 + 1, 19001ull * 86400, 0xFFFFFFFEull, 0xFFFFFFFFull}) {
                if (lo64 > hi64) continue;
                const uint64_t hi_ex = hi64 == 0xFFFFFFFFull ? 1ull << 32 : hi64, d0 = (uint64_t)date * 86400, d1 = d0 + 86400;
                const bool want = std::max(lo64, d0) < std::min(hi_ex, d1);
                CHECK(raw_range_date_meets(date, (uint32_t)lo64, (uint32_t)hi64) == want, "Date %u [%llu, %llu): pruning", date, (unsigned long long)lo64, (unsigned long long)hi64);
            }
}

// stage A reads Date[0] out of the part's first RAW_PROBE_BYTES bytes: at every step of varuint(rows) up to the largest part
static void check_probe_bytes() {
    for (uint64_t rows : {1ull, 127ull, 128ull, 16383ull, 16384ull, (1ull << 21) - 1, 1ull << 21, (1ull << 23), (1ull << 28) - 1, 1ull << 28, 1ull << 31}) {
        const uint32_t at = raw_range_date_at(RAW_COLS_H, rows);
        CHECK(at + 2 <= RAW_PROBE_BYTES, "rows %llu: Date[0] at byte %u leaves the %u bytes stage A reads", (unsigned long long)rows, at, RAW_PROBE_BYTES);
        CHECK(at + 2 * rows == raw_col_offset(RAW_COLS_H, rows, 1), "rows %llu: Date[0] is not where the Date column's values begin", (unsigned long long)rows);
    }
}

int main() {
    check_probe_bytes();
    for (uint64_t rows = 0; rows <= 300; rows++) check_rows(rows, true);
    // varuint(rows) grows at 2^7 and 2^14; a block holds 595.78 rows; a 4-, 8-, 16-byte column fills a block at 16384, 8192, 4096 rows
    std::set<uint64_t> big = {16383, 16384, 16385, 8191, 8192, 8193, 4095, 4096, 4097, 4100, 16380, 16390};
    for (uint64_t k : {1, 2, 3, 7, 11, 27}) big.insert(595 * k - 1), big.insert(595 * k), big.insert(595 * k + 1), big.insert(595 * k + k * 78 / 100), big.insert(595 * k + k * 78 / 100 + 1);
    for (uint64_t rows : big) check_rows(rows, false);
    check_predicate();
    printf("OK %llu\n", checks);
    return 0;
}
