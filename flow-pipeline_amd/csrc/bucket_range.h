// bucket_range.h - [t_lo, t_hi) of a bucketed table as bucket indices: THE range rule of every ranged read (the talker tables of
// talkers_host.inc, the port tables of ports_host.inc).  Plain host code with no ctx in it, so that a test can compile it alone
// (tests/host_port_buckets.hip).
#pragma once
#include <stdint.h>

namespace fa {

// bucket indices index_lo .. index_last, the last one INCLUSIVE: the last index of the axis has no successor in 32 bits
struct BucketRange {
    uint32_t index_lo = 0, index_last = 0;
    bool empty = false;  // t_lo == t_hi
};
enum { BUCKET_RANGE_OK = 0, BUCKET_RANGE_OFF_GRID = 1, BUCKET_RANGE_REVERSED = 2 };
// t_lo and t_hi lie on the grid of bucket_secs (>= 1); t_hi = 0xFFFFFFFF: no upper bound, the last bucket of the axis included.
inline int bucket_range_of(uint32_t bucket_secs, uint32_t t_lo, uint32_t t_hi, BucketRange& r) {
    const uint32_t bs = bucket_secs;
    if (t_lo % bs || (t_hi != 0xFFFFFFFFu && t_hi % bs)) return BUCKET_RANGE_OFF_GRID;
    if (t_lo > t_hi) return BUCKET_RANGE_REVERSED;
    r.empty = t_lo == t_hi;
    r.index_lo = t_lo / bs;
    r.index_last = t_hi == 0xFFFFFFFFu ? 0xFFFFFFFFu / bs : t_hi / bs - (r.empty ? 0u : 1u);
    return BUCKET_RANGE_OK;
}

}  // namespace fa
