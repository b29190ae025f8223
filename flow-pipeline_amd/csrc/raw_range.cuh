// raw_range.cuh - a time range of a flows_raw part as a row range, on the device (gfx950; host side: raw_range_host.inc; the
// geometry and the element predicate: raw_range_plan.h).
//
// flows_raw is ORDER BY TimeReceived (create.sh:36-62) and a part carries that order (raw.cuh), so the rows with
// t_lo <= t32 < t_hi are ONE run [r_lo, r_hi) of a part - if the part is sorted, which nothing has checked so far: the whole-file
// doors never needed the order.  raw_range_kernel makes ONE pass over the part's TimeReceived column, 4 of a row's 110 bytes,
// and leaves in the part's 32-byte record
//   r_lo, r_hi    the rows with t < t_lo, with t < t_hi (every row when there is no upper bound): on a sorted column the two
//                 lower bounds.  A scan, not a binary search: the same pass is the only check of the order the result rests on;
//   descends_at   the smallest row i with t[i] > t[i + 1]; off_date_at: the smallest row with t / 86400 != the part's Date
//                 (RAW_RANGE_NONE: no such row);
//   t_min, t_max  over the rows with t_lo <= t < t_hi (0xFFFFFFFF and 0 when there are none).
// The column starts at ANY byte phase of the image and the phase moves with `rows` (raw.cuh): a thread owns 4 elements - 16
// column bytes - per trip and reads them as raw_unpack_kernel does, the one or two ALIGNED 16-byte words that cover them shifted
// by the column's phase (bytes16_at_phase); the column's last, partial group and a group whose aligned words would leave the
// part's span go byte by byte.  Every word and byte read holds a byte of the column: nothing outside [part, part + bytes) is
// read, and for LZ4 input nothing outside the 64 KiB slots the column lies in (slots are 64 KiB-aligned, words 16-byte-aligned).
// An element's successor comes from the next lane (one shuffle of the lanes' first elements); a wave's last lane reads its
// own, 4 single bytes.  Counts leave a wave through __ballot + popcount, the four extrema through shuffles, a workgroup
// through LDS, and thread 0 issues at most one atomicAdd / atomicMin / atomicMax per word of the record.  The grid is
// flattened: RawRangePart::tile0 is a part's first workgroup, a workgroup finds its part by bisection over a few uniform words.
// The host initialises the records on the stream (they travel with the plan).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "align16.cuh"
#include "raw.cuh"
#include "raw_range_plan.h"

namespace fa {

struct RawRangePart {
    uint64_t off, bytes;   // where the part starts in the image, its size
    uint32_t rows, date;   // rows > 0
    uint32_t tile0, _pad;  // the part's first workgroup of the flattened grid (ascending over the list)
};
struct RawRangeRec {
    uint32_t r_lo, r_hi, descends_at, off_date_at, t_min, t_max, _pad[2];
};
static_assert(sizeof(RawRangePart) == 32 && sizeof(RawRangeRec) == 32, "plan and record of raw_range_kernel");
inline RawRangeRec raw_range_rec_init() { return RawRangeRec{0, 0, RAW_RANGE_NONE, RAW_RANGE_NONE, 0xFFFFFFFFu, 0, {0, 0}}; }

// 4 bytes at any phase (one single-byte load per trip of a loop that is NOT unrolled: raw_unpack_kernel's byte path)
__device__ __forceinline__ uint32_t raw_range_bytes4(const uint8_t* p) {
    uint32_t v = 0;
#pragma nounroll
    for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i);
    return v;
}

__global__ __launch_bounds__(RAW_RANGE_BLOCK) void raw_range_kernel(const RawRangePart* __restrict__ parts, uint32_t nparts, const uint8_t* __restrict__ img, uint32_t t_lo,
                                                                    uint32_t t_hi, RawRangeRec* __restrict__ rec) {
    __shared__ uint32_t red[RAW_RANGE_BLOCK / 64][6];
    uint32_t pa = 0, pb = nparts;  // the last part whose tile0 <= blockIdx.x (uniform)
    while (pb - pa > 1) {
        const uint32_t mid = (pa + pb) >> 1;
        if (parts[mid].tile0 <= blockIdx.x) pa = mid;
        else pb = mid;
    }
    const RawRangePart p = parts[pa];
    const uint64_t tile = blockIdx.x - p.tile0;
    if (tile >= raw_range_tiles(p.rows)) return;  // (the whole workgroup; the host launches exactly the tiles there are)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rows = p.rows;
    const uint8_t* const part = img + p.off;
    const uint8_t* const col = part + raw_col_offset(RAW_COLS_D, rows, RAW_COL_TIME) + raw_col_header_len(RAW_COLS_D[RAW_COL_TIME]);
    const uint64_t lo = (uint64_t)(uintptr_t)part, hi = lo + p.bytes;

    uint32_t c_lo = 0, c_hi = 0;                                                  // wave-uniform counts
    uint32_t desc = RAW_RANGE_NONE, offd = RAW_RANGE_NONE, tmin = 0xFFFFFFFFu, tmax = 0;  // this thread's
#pragma unroll
    for (uint32_t k = 0; k < RAW_RANGE_ITERS; k++) {
        const uint64_t g = raw_range_group(tile, k, tid);
        const uint32_t e0 = (uint32_t)(4 * g);  // (4 g < rows + RAW_RANGE_TILE <= 2^31 + 4096)
        const uint32_t nv = e0 >= rows ? 0u : min(4u, rows - e0);
        uint32_t t[4] = {0u, 0u, 0u, 0u};
        if (nv) {
            const RawRangeLoad l = raw_range_load((uint64_t)(uintptr_t)col, g, rows, lo, hi);
            if (l.wide) {
                const uint4 x = *(const uint4*)(uintptr_t)l.al;
                const uint4 y = l.sh ? *(const uint4*)(uintptr_t)(l.al + 16) : make_uint4(0, 0, 0, 0);
                const uint4 o = bytes16_at_phase(x, y, l.sh);
                t[0] = o.x, t[1] = o.y, t[2] = o.z, t[3] = o.w;
            } else {
                for (uint32_t q = 0; q < 4; q++)
                    if (q < nv) t[q] = raw_range_bytes4(col + 4 * (uint64_t)(e0 + q));
            }
        }
        // the successor of this thread's last element: the next lane's first; a wave's last lane reads its own
        uint32_t succ = __shfl_down(t[0], 1);
        if (lane == 63 && e0 + 4 < rows) succ = raw_range_bytes4(col + 4 * (uint64_t)(e0 + 4));
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const bool valid = q < nv;
            const RawRangeElem e = raw_range_elem(t[q], q < 3 ? t[q + 1] : succ, e0 + q + 1 < rows, t_lo, t_hi, p.date);
            c_lo += (uint32_t)__popcll(__ballot(valid && e.below_lo));
            c_hi += (uint32_t)__popcll(__ballot(valid && e.below_hi));
            if (valid && e.descends) desc = min(desc, e0 + q);
            if (valid && e.off_date) offd = min(offd, e0 + q);
            if (valid && e.selected) tmin = min(tmin, t[q]), tmax = max(tmax, t[q]);
        }
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        desc = min(desc, (uint32_t)__shfl_xor(desc, d));
        offd = min(offd, (uint32_t)__shfl_xor(offd, d));
        tmin = min(tmin, (uint32_t)__shfl_xor(tmin, d));
        tmax = max(tmax, (uint32_t)__shfl_xor(tmax, d));
    }
    if (lane == 0) {
        red[wave][0] = c_lo, red[wave][1] = c_hi, red[wave][2] = desc, red[wave][3] = offd;
        red[wave][4] = tmin, red[wave][5] = tmax;
    }
    __syncthreads();
    if (tid == 0) {
        // (t_min 0xFFFFFFFF with t_max 0 is "none": a selected row with t = 0xFFFFFFFF raises t_max to it)
        for (uint32_t w = 1; w < RAW_RANGE_BLOCK / 64; w++) {
            c_lo += red[w][0], c_hi += red[w][1];
            desc = min(desc, red[w][2]), offd = min(offd, red[w][3]), tmin = min(tmin, red[w][4]), tmax = max(tmax, red[w][5]);
        }
        RawRangeRec* r = rec + pa;
        if (c_lo) atomicAdd(&r->r_lo, c_lo);
        if (c_hi) atomicAdd(&r->r_hi, c_hi);
        if (desc != RAW_RANGE_NONE) atomicMin(&r->descends_at, desc);
        if (offd != RAW_RANGE_NONE) atomicMin(&r->off_date_at, offd);
        if (tmin != 0xFFFFFFFFu || tmax != 0) atomicMin(&r->t_min, tmin), atomicMax(&r->t_max, tmax);
    }
}

// The first RAW_PROBE_BYTES bytes of every part of an LZ4 input (a part starts at its first block's slot: 64 KiB-aligned, and a
// slot holds them whatever the part's size): the column count, varuint(rows), the first column's header and Date[0] lie in them.
__global__ __launch_bounds__(64) void raw_probe_kernel(const uint64_t* __restrict__ off, uint32_t n, const uint8_t* __restrict__ img, uint4* __restrict__ out) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint4* src = (const uint4*)(img + off[i]);
    for (uint32_t w = 0; w < RAW_PROBE_BYTES / 16; w++) out[i * (RAW_PROBE_BYTES / 16) + w] = src[w];
}

}  // namespace fa
