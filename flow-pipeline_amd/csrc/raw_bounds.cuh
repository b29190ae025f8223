// raw_bounds.cuh - where a time range begins and ends in a SORTED flows_raw part: two positions by a 64-ary search (gfx950; host
// side: raw_pending_host.inc; the contract: include/flowagg.h "the pending flows_raw parts as input"; run on the host, the very
// text with 64 simulated lanes, by tests/host_raw_bounds.hip).
//
// WHY NOT raw_range_kernel: that one makes a full pass over the 4-byte TimeReceived column because its input is untrusted - it
// proves the order and the Date of every row.  The pending parts of a ctx are the library's own: the build's and the merge's
// stable sorts wrote them, so the order holds by construction, and after fa_raw_merge a ctx holds ONE part per Date: "the last
// five minutes" of a merged day would scan the whole column (32 MB for 2^23 rows) to find two positions.
//
// raw_bounds_kernel: ONE WAVE per searched part.  lower_bound(key) keeps an interval [lo, hi] that holds the answer.  A step's 64
// lanes probe 64 ascending positions of [lo, hi) that cut it into at most 65 pieces (raw_bounds_pos); col[pos] < key is true on
// a prefix of the lanes, so the popcount c of its __ballot names the piece (raw_bounds_narrow): behind position c - 1, up to
// position c.  An interval of n > 64 rows leaves at most ceil(n / 65); one of n <= 64 is settled by its step (lane l probes
// lo + l, the answer is lo + c).  So a search of `rows` rows takes at most ceil(log65(rows)) + 1 steps
// (raw_bounds_max_steps: four for 2^24 rows), each ONE load per lane - against 24 dependent loads of a bisection, or the full pass.
// The loop's condition and the new interval depend on the ballot alone: they are wave-uniform, no lane leaves early.
// WHY THE LOADS STAY INSIDE THE COLUMN: every probed position lies in [lo, hi) with 0 <= lo < hi <= rows, whatever the values read
// (the narrowing uses only the popcount), and a load is an element-width read at the element's own address
// (raw_load_unaligned32 at raw_merge_src_offset: the column starts at any byte phase): bytes [4 pos, 4 pos + 4) of the column,
// nothing around them.  t_min / t_max are read at r_lo and r_hi - 1, only when r_lo < r_hi.  An unsorted column would give wrong
// positions, never a read outside it, and the search still ends: every step shrinks the interval.
// The result is one 32-byte record per part, written by lane 0 with ordinary stores.  No LDS, no atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raw.cuh"
#include "raw_merge.cuh"
#include "raw_select.cuh"

namespace fa {

struct RawBoundsPart {
    uint64_t off;          // where the part starts in the image
    uint32_t rows, _pad;   // the part's rows (> 0)
};
struct RawBoundsRec {
    uint64_t r_lo, r_hi;    // the rows in range are [r_lo, r_hi)
    uint32_t t_min, t_max;  // TimeReceived of rows r_lo and r_hi - 1 (0 when r_lo == r_hi)
    uint32_t steps, _pad;   // search steps of both bounds together
};
static_assert(sizeof(RawBoundsPart) == 16 && sizeof(RawBoundsRec) == 32, "plan and record of raw_bounds_kernel");

// the interval that still holds the answer: lo <= answer <= hi
struct RawBoundsIv {
    uint64_t lo, hi;
};

// the position lane `lane` (0 .. 63) probes in this step; *valid: the lane has one.  Positions ascend with the lane and lie in
// [lo, hi).  (n < 2^32: (lane + 1) * n stays far below 2^64.)
__host__ __device__ __forceinline__ uint64_t raw_bounds_pos(const RawBoundsIv& iv, uint32_t lane, bool* valid) {
    const uint64_t n = iv.hi - iv.lo;
    if (n <= 64) {
        *valid = lane < n;
        return iv.lo + lane;
    }
    *valid = true;
    return iv.lo + (uint64_t)(lane + 1) * n / 65;  // (n >= 65: lo < pos(0) < pos(1) < ... < pos(63) < hi)
}

// the interval behind a step; ballot: bit l set iff lane l is valid and col[pos(l)] < key - a prefix of the lanes in a sorted column
__host__ __device__ __forceinline__ RawBoundsIv raw_bounds_narrow(const RawBoundsIv& iv, uint64_t ballot) {
    const uint32_t c = (uint32_t)__builtin_popcountll(ballot);
    const uint64_t n = iv.hi - iv.lo;
    if (n <= 64) return RawBoundsIv{iv.lo + c, iv.lo + c};  // (c <= n: only valid lanes vote)
    bool v;
    RawBoundsIv o = iv;
    if (c > 0) o.lo = raw_bounds_pos(iv, c - 1, &v) + 1;  // col[pos(c - 1)] < key: the answer lies behind it
    if (c < 64) o.hi = raw_bounds_pos(iv, c, &v);         // col[pos(c)] >= key: the answer is at most there
    return o;
}

// the first row of [from, rows) whose value is not below the key (rows: none); ballot(iv) -> the step's 64 votes; *steps += the
// steps taken
template <class Ballot>
__host__ __device__ __forceinline__ uint64_t raw_bounds_lower(uint64_t from, uint64_t rows, Ballot ballot, uint32_t* steps) {
    RawBoundsIv iv{from, rows};
    while (iv.lo < iv.hi) {
        iv = raw_bounds_narrow(iv, ballot(iv));
        ++*steps;
    }
    return iv.lo;
}

// the most steps a search of `rows` rows takes
__host__ __device__ inline uint32_t raw_bounds_max_steps(uint64_t rows) {
    uint32_t s = 0;
    uint64_t n = rows;
    for (; n > 64; s++) n = (n + 64) / 65;
    return s + (n ? 1u : 0u);
}

// grid: one workgroup of ONE wave per part
__global__ __launch_bounds__(64) void raw_bounds_kernel(const RawBoundsPart* __restrict__ parts, uint32_t nparts, const uint8_t* __restrict__ img, uint32_t t_lo, uint32_t t_hi,
                                                        RawBoundsRec* __restrict__ rec) {
    if (blockIdx.x >= nparts) return;
    const RawBoundsPart p = parts[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const uint8_t* const part = img + p.off;
    const RawMergeCol k = raw_merge_col(RAW_COLS_D, RAW_SEL_C_TIME);
    auto at = [&](uint64_t r) { return raw_load_unaligned32(part + raw_merge_src_offset(k, p.rows, r)); };
    uint32_t steps = 0;
    auto lower = [&](uint64_t from, uint32_t key) {
        return raw_bounds_lower(
            from, p.rows,
            [&](const RawBoundsIv& iv) {
                bool valid;
                const uint64_t pos = raw_bounds_pos(iv, lane, &valid);
                return (uint64_t)__ballot(valid && at(pos) < key);
            },
            &steps);
    };
    const uint64_t r_lo = lower(0, t_lo);
    const uint64_t r_hi = t_hi == 0xFFFFFFFFu ? (uint64_t)p.rows : lower(r_lo, t_hi);  // (t_lo <= t_hi: the answer is not in front of r_lo)
    if (lane == 0) {
        RawBoundsRec o{};
        o.r_lo = r_lo, o.r_hi = r_hi, o.steps = steps;
        if (r_lo < r_hi) o.t_min = at(r_lo), o.t_max = at(r_hi - 1);
        rec[blockIdx.x] = o;
    }
}

}  // namespace fa
