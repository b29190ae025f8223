// raw_merge.cuh - merging the pending flows_raw parts of a ctx: one sorted part per Date (gfx950; host side: raw_merge_host.inc).
//
// The SOURCES are the pending parts themselves, back to back in the image (raw.cuh: the part format).  Laid end to end in build
// order their rows have GLOBAL numbers 0 .. n - 1; source p holds the rows [first[p], first[p] + rows[p]).
//
// Order (raw_merge_key_kernel, one stable 32-bit radix sort, raw_parts_kernel of raw.cuh): the key of global row g is the
// TimeReceived value the source holds for it, the index is g.  Every source is sorted already and the sort is stable, so equal
// keys keep (source in build order, row in the source) - the order ONE chunk holding all those records would have given them.
// Date is monotone in the key: one sort serves every Date, and raw_parts_kernel lists the boundaries as it does for a chunk.
//
// Gather (raw_merge_gather_kernel), the hot part: the part writer of raw.cuh (raw_write_tile - the tiles, the LDS staging, the
// aligned stores and the headers are described there) over another load.  Sorted element e is global row g = idx[e]; a bounded
// binary search over `first` (staged in LDS when the call has at most RAW_MERGE_LDS_SRCS sources, read from global memory
// otherwise) gives the source p, and the element lies at
//   src[p].part + raw_col_offset(rows_p, c) + header_len(c) + (g - first[p]) * width.
// That address has ANY byte phase, and the phase differs from source to source: it is per lane, not wave-uniform.  The load is
// an element-width read at the element's own address (raw_load_unaligned): gfx950 serves a global load at any byte address,
// and a read of exactly the element's bytes cannot leave the source part, let alone the image.  (Aligned loads
// shifted with v_alignbyte would need two aligned 16-byte loads per 16-byte element, a per-lane dword select - every arm of
// bytes16_at_phase executed - and a byte path at the image's ends: reasoned, not measured.)
// Date is the part's constant; TimeReceived comes from the sorted keys, not from the sources.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raw.cuh"

namespace fa {

constexpr uint32_t RAW_MERGE_LDS_SRCS = 512;  // sources whose first rows fit the kernel's LDS table (2 KiB)

struct RawMergeSrc {
    const uint8_t* part;   // the source part's first byte in the old image
    uint32_t rows, first;  // its rows; the global number of its first row
};

// the source that holds global row g: the largest p with first(p) <= g (first(0) == 0, ascending, g below the total).
// The interval [lo, hi) halves every trip: at most 32 trips.
template <class First>
__host__ __device__ __forceinline__ uint32_t raw_merge_find(First first, uint32_t nsrc, uint32_t g) {
    uint32_t lo = 0, hi = nsrc;
    for (uint32_t trip = 0; trip < 32 && hi - lo > 1; trip++) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (first(mid) <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Where a column's values lie in a part of ANY row count: raw_col_offset is linear in rows but for the row count's varuint, so
// two evaluations give the column's terms once per workgroup instead of a walk over the columns per element.
struct RawMergeCol {
    uint32_t fixed, per_row, width;  // the values start at varuint_len(rows) + fixed + rows * per_row
};
__host__ __device__ inline RawMergeCol raw_merge_col(const RawColDef* cols, uint32_t c) {
    const uint64_t o0 = raw_col_offset(cols, 0, c), o1 = raw_col_offset(cols, 1, c);
    return RawMergeCol{(uint32_t)(o0 - raw_varuint_len(0) + raw_col_header_len(cols[c])), (uint32_t)(o1 - o0), cols[c].width};
}
// byte offset of row r's value inside a source part of `rows` rows
__host__ __device__ __forceinline__ uint64_t raw_merge_src_offset(const RawMergeCol& k, uint64_t rows, uint64_t r) {
    return raw_varuint_len(rows) + k.fixed + rows * k.per_row + r * k.width;
}

// 1, 2 or 4 dwords at any byte address, read through types of alignment 1: the compiler may not assume more.  gfx950 code
// objects run with unaligned access on, so no byte loads are emitted; this compiler issues a load of alignment 1 as dword
// loads at the element's own bytes (1, 2 or 4 global_load_dword), which hit the same one or two cache lines.
typedef uint32_t raw_u32x1_u __attribute__((aligned(1)));
typedef uint32_t raw_u32x2_u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t raw_u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
__device__ __forceinline__ uint32_t raw_load_unaligned32(const uint8_t* p) { return *(const raw_u32x1_u*)p; }
__device__ __forceinline__ void raw_load_unaligned(const uint8_t* p, uint32_t dwords, uint32_t v[4]) {
    if (dwords == 1) {
        v[0] = raw_load_unaligned32(p);
    } else if (dwords == 2) {
        const raw_u32x2_u q = *(const raw_u32x2_u*)p;
        v[0] = q.x, v[1] = q.y;
    } else {
        const raw_u32x4_u q = *(const raw_u32x4_u*)p;
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    }
}

// ---- order -----------------------------------------------------------------------------------------------------------------
// key[g] = the source's TimeReceived of global row g, idx[g] = g; idx[n] = n is the `pos[n]` raw_parts_kernel reads (every row
// of a part is good)
__global__ __launch_bounds__(256) void raw_merge_key_kernel(const RawMergeSrc* __restrict__ src, uint32_t nsrc, uint32_t n, uint32_t* __restrict__ key,
                                                            uint32_t* __restrict__ idx) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == n) idx[n] = n;
    if (g >= n) return;
    const RawMergeCol k = raw_merge_col(RAW_COLS_D, 1);  // TimeReceived
    const uint32_t p = raw_merge_find([&](uint32_t i) { return src[i].first; }, nsrc, g);
    const RawMergeSrc s = src[p];
    key[g] = raw_load_unaligned32(s.part + raw_merge_src_offset(k, s.rows, g - s.first));
    idx[g] = g;
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
struct RawMergeArgs {
    uint8_t* part;           // where the merged part starts in the new image
    const uint32_t* key;     // the sorted keys ...
    const uint32_t* idx;     // ... and global rows, both already advanced to the part's first row
    const RawMergeSrc* src;  // every source of the call
    uint32_t nsrc, rows, date;
};

__global__ __launch_bounds__(RAW_BLOCK) void raw_merge_gather_kernel(const RawMergeArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[RAW_TILE_DWORDS + 4];
    __shared__ uint32_t first_lds[RAW_MERGE_LDS_SRCS];
    RawTile t;
    if (!raw_tile_locate(RAW_COLS_D, (uint64_t)(uintptr_t)a.part, a.rows, blockIdx.x, &t)) return;  // (the host launches exactly the tiles there are)
    const uint32_t kind = RAW_COLS_D[t.c].kind;
    const bool in_lds = a.nsrc <= RAW_MERGE_LDS_SRCS;
    RawMergeCol mc{};
    if (kind != RAW_K_DATE && kind != RAW_K_KEY) {  // a column that comes from the sources: where it lies in them, the table of first rows
        mc = raw_merge_col(RAW_COLS_D, t.c);
        if (in_lds) {
            for (uint32_t j = threadIdx.x; j < a.nsrc; j += RAW_BLOCK) first_lds[j] = a.src[j].first;
            __syncthreads();
        }
    }
    raw_write_tile(lds, a.part, a.rows, a.date, a.key, t, [&](uint32_t e, uint32_t* v) {
        const uint32_t g = a.idx[e];
        const uint32_t p = in_lds ? raw_merge_find([&](uint32_t i) { return first_lds[i]; }, a.nsrc, g)
                                  : raw_merge_find([&](uint32_t i) { return a.src[i].first; }, a.nsrc, g);
        const RawMergeSrc sp = a.src[p];
        raw_load_unaligned(sp.part + raw_merge_src_offset(mc, sp.rows, g - sp.first), mc.width >> 2, v);
    });
}

}  // namespace fa
