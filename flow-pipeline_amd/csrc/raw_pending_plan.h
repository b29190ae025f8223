// raw_pending_plan.h - what the host decides about a pending flows_raw part from its description alone (host only; used by
// raw_pending_host.inc; run against a naive scan of the rows by tests/host_raw_bounds.hip).
//
// A pending part is sorted by TimeReceived and the host keeps its t_min / t_max (fa_raw_part).  For a time range with the rule
// of the ranged loads - t_lo <= t32 < t_hi, t_hi == 0xFFFFFFFF: to the end, that second included - they say, without a look at
// the device, that no row can be in range (SKIPPED), that every row is (WHOLE), or neither (SEARCHED: raw_bounds_kernel of
// raw_bounds.cuh finds the two positions).  A searched part may still turn out to hold no row of the range: a range that falls
// between two values.
#pragma once
#include <stdint.h>

namespace fa {

enum { RAW_PENDING_SKIPPED = 0, RAW_PENDING_WHOLE = 1, RAW_PENDING_SEARCHED = 2 };

// the first second behind the range, in 64 bits: 0xFFFFFFFF has none on the 32-bit axis
inline uint64_t raw_pending_upper(uint32_t t_hi) { return t_hi == 0xFFFFFFFFu ? (uint64_t)1 << 32 : (uint64_t)t_hi; }

// t_min / t_max: TimeReceived of the part's first and last row (rows > 0); t_lo <= t_hi
inline int raw_pending_class(uint64_t rows, uint32_t t_min, uint32_t t_max, uint32_t t_lo, uint32_t t_hi) {
    const uint64_t upper = raw_pending_upper(t_hi);
    if (rows == 0 || (uint64_t)t_lo >= upper) return RAW_PENDING_SKIPPED;  // (t_lo == t_hi selects nothing)
    if (t_max < t_lo || (uint64_t)t_min >= upper) return RAW_PENDING_SKIPPED;
    if (t_min >= t_lo && (uint64_t)t_max < upper) return RAW_PENDING_WHOLE;
    return RAW_PENDING_SEARCHED;
}

}  // namespace fa
