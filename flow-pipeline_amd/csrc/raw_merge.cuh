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
// Gather (raw_merge_gather_kernel), the hot part: raw_gather_kernel with another source.  The store side is the same - a
// workgroup owns RAW_TILE_CHUNKS 16-byte-ALIGNED chunks of one column of the merged part, stages the dwords that cover them in
// LDS, shifts by the destination's byte phase and issues one aligned 16-byte store per lane; first and last chunk of a column
// and the headers leave as byte stores; every byte is written exactly once, by one lane.  The load side: sorted element e is
// global row g = idx[e]; a bounded binary search over `first` (staged in LDS when the call has at most RAW_MERGE_LDS_SRCS
// sources, read from global memory otherwise) gives the source p, and the element lies at
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
    const uint32_t tid = threadIdx.x;
    const uint64_t rows = a.rows;
    // which column, which tile of it: a few uniform steps over the 16 columns
    uint64_t tile = blockIdx.x, off = 1 + raw_varuint_len(rows);
    uint32_t c = 0;
    for (;; c++) {
        if (c == RAW_NCOLS) return;  // (the host launches exactly the tiles there are)
        const RawColDef& d = RAW_COLS_D[c];
        const uint64_t data = off + raw_col_header_len(d), bytes = rows * d.width;
        const uint64_t tiles = raw_col_tiles((uint64_t)(uintptr_t)(a.part + data), bytes);
        if (tile < tiles) break;
        tile -= tiles;
        off = data + bytes;
    }
    const RawColDef& d = RAW_COLS_D[c];
    const uint32_t kind = d.kind;
    const uint32_t hl = raw_col_header_len(d);
    uint8_t* const col = a.part + off + hl;  // the column's first data byte
    const long long bytes = (long long)(rows * d.width);
    const bool from_src = kind != RAW_K_DATE && kind != RAW_K_KEY;
    const bool in_lds = a.nsrc <= RAW_MERGE_LDS_SRCS;
    if (from_src && in_lds)
        for (uint32_t j = tid; j < a.nsrc; j += RAW_BLOCK) first_lds[j] = a.src[j].first;
    if (tile == 0) {  // the column's header, and in front of the first column the block's
        uint8_t* h = a.part + off;
        if (tid < hl) {
            uint8_t b;
            if (tid == 0) b = d.name_len;
            else if (tid <= d.name_len) b = (uint8_t)d.name[tid - 1];
            else if (tid == 1u + d.name_len) b = d.type_len;
            else b = (uint8_t)d.type[tid - 2 - d.name_len];
            h[tid] = b;
        }
        if (c == 0 && tid == 0) {
            a.part[0] = (uint8_t)RAW_NCOLS;
            uint64_t v = rows;
            uint8_t* p = a.part + 1;
            while (v >= 128) *p++ = (uint8_t)(v | 128), v >>= 7;
            *p = (uint8_t)v;
        }
    }
    __syncthreads();  // (the table of first rows is complete)
    // s: the column byte the tile's first aligned chunk starts at (negative in the first tile unless the column is aligned)
    const long long s = (long long)tile * (RAW_TILE_CHUNKS * 16) - (long long)((uintptr_t)col & 15);
    const long long k0 = s >> 2;            // first staged dword (floor: s may be negative)
    const uint32_t sh = (uint32_t)(s & 3);  // the byte phase, the same for every chunk of the column
    if (kind == RAW_K_DATE) {               // one Date per part: nothing to gather
        const uint32_t v = a.date | (a.date << 16);
        for (uint32_t j = tid; j < RAW_TILE_DWORDS + 4; j += RAW_BLOCK) lds[j] = v;
    } else {
        const RawMergeCol mc = raw_merge_col(RAW_COLS_D, c);
        const uint32_t dpe = d.width >> 2;      // dwords per element: 1, 2, 4
        const long long e0 = k0 >> (dpe >> 1);  // first element that touches the staged dwords (floor)
        const uint32_t nelem = (RAW_TILE_DWORDS + 1) / dpe + 2;
        for (uint32_t j = tid; j < nelem; j += RAW_BLOCK) {
            const long long e = e0 + j;
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            if (e >= 0 && e < (long long)rows) {
                if (kind == RAW_K_KEY) {
                    v[0] = a.key[e];
                } else {
                    const uint32_t g = a.idx[e];
                    const uint32_t p = in_lds ? raw_merge_find([&](uint32_t i) { return first_lds[i]; }, a.nsrc, g)
                                              : raw_merge_find([&](uint32_t i) { return a.src[i].first; }, a.nsrc, g);
                    const RawMergeSrc sp = a.src[p];
                    raw_load_unaligned(sp.part + raw_merge_src_offset(mc, sp.rows, g - sp.first), dpe, v);
                }
            }
            for (uint32_t q = 0; q < dpe; q++) {
                const long long l = e * dpe + q - k0;  // where the dword stands in the staged run
                if (l >= 0 && l <= (long long)RAW_TILE_DWORDS) lds[l] = v[q];
            }
        }
    }
    __syncthreads();
    const long long b = s + 16ll * tid;  // the column byte this lane's chunk starts at
    if (b >= bytes || b + 16 <= 0) return;
    const uint4 lo = *(const uint4*)&lds[4 * tid];
    const uint32_t hi = lds[4 * tid + 4];
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(lo.y, lo.x, sh);
    o.y = __builtin_amdgcn_alignbyte(lo.z, lo.y, sh);
    o.z = __builtin_amdgcn_alignbyte(lo.w, lo.z, sh);
    o.w = __builtin_amdgcn_alignbyte(hi, lo.w, sh);
    uint8_t* const dst = col + b;  // 16-byte aligned by construction
    if (b >= 0 && b + 16 <= bytes) {
        *(uint4*)dst = o;
    } else {  // the column's first or last chunk: only the bytes that are the column's
        const uint32_t w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (b + i >= 0 && b + i < bytes) dst[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

}  // namespace fa
