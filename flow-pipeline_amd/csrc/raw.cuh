// raw.cuh - flows_raw parts built on the device: sorted ClickHouse Native blocks, one per Date (gfx950).
//
// flows_raw (create.sh:36-68) is a MergeTree PARTITION BY Date ORDER BY TimeReceived, filled by
// "SELECT toDate(TimeReceived) AS Date, * FROM flows": one inserted block becomes one part per Date, its rows sorted by the
// DateTime-narrowed TimeReceived.  A part here is one Native block WITHOUT BlockInfo (format restated from the ClickHouse
// documentation; no server was available to load it into - the caveat of format_host.inc's RowBinary sink):
//   varuint(16) varuint(rows), then per column, in the order of create.sh:38-59:
//   varuint(len(name)) name varuint(len(type)) type, rows little-endian values.
// Every column is fixed-width (RAW_COLS below), 110 payload bytes per row.  Row rules: status != 0 is dropped
// (inserter.go:125-126); rows in STABLE ascending order of t32 = (uint32_t)TimeReceived; Date = t32 / 86400, monotone in t32,
// so one sort serves both keys; a part holds one Date.
//
// Order (raw_flag_kernel, an exclusive scan, raw_key_kernel, one 32-bit radix sort, raw_parts_kernel): the good records are
// compacted to the front in record order and the bad ones behind them with the key 0xFFFFFFFF.  The radix sort is stable, and
// every good record stands in front of every bad one before it, so after it the first `good` entries are exactly the good
// records in stable t32 order - also when a good record's own t32 is 0xFFFFFFFF.  No 33-bit key, no count on the host before
// the sort.  raw_parts_kernel marks the positions where the Date changes; the host reads that list with one small copy.
//
// Gather (raw_gather_kernel), the hot part.  Headers have odd lengths and the first column is 2 bytes wide, so a 4-, 8- or
// 16-byte column starts at ANY byte offset of the image, and the offset changes with `rows`.  The kernel never issues a store
// that is off its natural alignment: a workgroup owns RAW_TILE_CHUNKS consecutive 16-byte-ALIGNED chunks of one column's byte
// range, stages the column's dwords that cover them in LDS (natural-width, coalesced-where-sorted loads through the sort's
// index), and every lane then reads five LDS dwords, shifts them by the column's byte phase (v_alignbyte) and issues ONE aligned
// 16-byte store.  The first and last chunk of a column, which the column only partly covers, leave as byte stores; so do the
// headers.  Every byte of the part is written exactly once, by exactly one lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "align16.cuh"

namespace fa {

constexpr uint32_t RAW_NCOLS = 16;
constexpr uint32_t RAW_ROW_BYTES = 110;
constexpr uint32_t RAW_MAX_DATES = 49711;  // Dates a 32-bit time axis holds: 0 .. (2^32 - 1) / 86400
constexpr uint32_t RAW_BLOCK = 256;
constexpr uint32_t RAW_TILE_CHUNKS = RAW_BLOCK;            // 16-byte chunks a workgroup writes: 4 KiB of the image
constexpr uint32_t RAW_TILE_DWORDS = RAW_TILE_CHUNKS * 4;  // ... the dwords they hold; one more is staged for the byte phase

// how a column's dwords come into being
enum { RAW_K_DATE = 0, RAW_K_KEY = 1, RAW_K_NARROW64 = 2, RAW_K_U32 = 3, RAW_K_U64 = 4, RAW_K_B16 = 5 };

struct RawColDef {
    char name[16], type[16];
    uint8_t name_len, type_len, width, kind;
};
#define RAW_COLS_INIT                                                                                       \
    {                                                                                                       \
        {"Date", "Date", 4, 4, 2, RAW_K_DATE}, {"TimeReceived", "DateTime", 12, 8, 4, RAW_K_KEY},           \
            {"TimeFlowStart", "DateTime", 13, 8, 4, RAW_K_NARROW64}, {"SequenceNum", "UInt32", 11, 6, 4, RAW_K_U32},   \
            {"SamplingRate", "UInt64", 12, 6, 8, RAW_K_U64}, {"SamplerAddress", "FixedString(16)", 14, 15, 16, RAW_K_B16}, \
            {"SrcAddr", "FixedString(16)", 7, 15, 16, RAW_K_B16}, {"DstAddr", "FixedString(16)", 7, 15, 16, RAW_K_B16},   \
            {"SrcAS", "UInt32", 5, 6, 4, RAW_K_U32}, {"DstAS", "UInt32", 5, 6, 4, RAW_K_U32},               \
            {"EType", "UInt32", 5, 6, 4, RAW_K_U32}, {"Proto", "UInt32", 5, 6, 4, RAW_K_U32},               \
            {"SrcPort", "UInt32", 7, 6, 4, RAW_K_U32}, {"DstPort", "UInt32", 7, 6, 4, RAW_K_U32},           \
            {"Bytes", "UInt64", 5, 6, 8, RAW_K_U64}, {"Packets", "UInt64", 7, 6, 8, RAW_K_U64},             \
    }
static const RawColDef RAW_COLS_H[RAW_NCOLS] = RAW_COLS_INIT;
__constant__ RawColDef RAW_COLS_D[RAW_NCOLS] = RAW_COLS_INIT;

__host__ __device__ __forceinline__ uint32_t raw_varuint_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 128) v >>= 7, n++;
    return n;
}
__host__ __device__ __forceinline__ uint32_t raw_col_header_len(const RawColDef& d) { return 2u + d.name_len + d.type_len; }
// byte offset of column c's header inside a part of `rows` rows (c == RAW_NCOLS: the part's size)
__host__ __device__ inline uint64_t raw_col_offset(const RawColDef* cols, uint64_t rows, uint32_t c) {
    uint64_t o = 1 + raw_varuint_len(rows);
    for (uint32_t j = 0; j < c; j++) o += raw_col_header_len(cols[j]) + rows * cols[j].width;
    return o;
}
// the tiles of RAW_TILE_CHUNKS aligned 16-byte chunks that cover `bytes` bytes starting at the absolute address `at`
__host__ __device__ __forceinline__ uint64_t raw_col_tiles(uint64_t at, uint64_t bytes) {
    const uint64_t chunks = ((at & 15) + bytes + 15) >> 4;
    return (chunks + RAW_TILE_CHUNKS - 1) / RAW_TILE_CHUNKS;
}

// ---- order -----------------------------------------------------------------------------------------------------------------
// flag[i] = the record is good; flag[n] = 0, so that the exclusive scan over n + 1 words leaves the good count in pos[n]
__global__ __launch_bounds__(256) void raw_flag_kernel(const uint8_t* __restrict__ status, uint32_t n, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) flag[i] = i < n && status[i] == 0 ? 1u : 0u;
}
// good records to [0, good) in record order with key t32, bad ones to [good, n) with key 0xFFFFFFFF
__global__ __launch_bounds__(256) void raw_key_kernel(const uint8_t* __restrict__ status, const uint64_t* __restrict__ time_received, uint32_t n,
                                                      const uint32_t* __restrict__ pos, uint32_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = pos[i], good = pos[n];
    const bool ok = status[i] == 0;
    const uint32_t j = ok ? p : good + (i - p);
    key[j] = ok ? (uint32_t)time_received[i] : 0xFFFFFFFFu;
    idx[j] = i;
}

struct RawPartsHeader {
    uint32_t good, nparts, last_t_max, _pad;
};
struct RawPartEntry {
    uint32_t start, t_min, prev_t_max, _pad;  // first sorted position of a Date, its key, the key in front of it
};
// one entry per position where the Date changes (unordered: the host sorts the few entries by start); hdr is zeroed beforehand
__global__ __launch_bounds__(256) void raw_parts_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ pos, uint32_t n, RawPartsHeader* hdr,
                                                        RawPartEntry* list, uint32_t list_cap) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t good = pos[n];
    if (j == 0) hdr->good = good;
    if (j >= good) return;
    const uint32_t k = key[j], kp = j ? key[j - 1] : 0u;
    if (j == 0 || k / 86400u != kp / 86400u) {
        const uint32_t slot = atomicAdd(&hdr->nparts, 1u);
        if (slot < list_cap) list[slot] = RawPartEntry{j, k, kp, 0u};
    }
    if (j == good - 1) hdr->last_t_max = k;
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
struct RawGatherArgs {
    uint8_t* part;          // where the part starts in the image
    const uint32_t* key;    // the sorted keys ...
    const uint32_t* idx;    // ... and record indices, both already advanced to the part's first row
    const void* src[RAW_NCOLS];  // the decoded column behind each output column (nullptr: Date, TimeReceived)
    uint32_t rows, date;
};

// dwords [e * dpe, (e + 1) * dpe) of a column's byte stream: element e in sorted order (0 <= e < rows)
__device__ __forceinline__ void raw_load_element(const RawGatherArgs& a, uint32_t kind, const void* src, uint32_t e, uint32_t v[4]) {
    switch (kind) {
    case RAW_K_KEY: v[0] = a.key[e]; break;
    case RAW_K_NARROW64: v[0] = (uint32_t)((const uint64_t*)src)[a.idx[e]]; break;
    case RAW_K_U32: v[0] = ((const uint32_t*)src)[a.idx[e]]; break;
    case RAW_K_U64: {
        const uint2 q = ((const uint2*)src)[a.idx[e]];
        v[0] = q.x, v[1] = q.y;
        break;
    }
    default: {  // RAW_K_B16
        const uint4 q = ((const uint4*)src)[a.idx[e]];
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    }
    }
}

__global__ __launch_bounds__(RAW_BLOCK) void raw_gather_kernel(const RawGatherArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[RAW_TILE_DWORDS + 4];
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
    // s: the column byte the tile's first aligned chunk starts at (negative in the first tile unless the column is aligned)
    const long long s = (long long)tile * (RAW_TILE_CHUNKS * 16) - (long long)((uintptr_t)col & 15);
    const long long k0 = s >> 2;             // first staged dword (floor: s may be negative)
    const uint32_t sh = (uint32_t)(s & 3);   // the byte phase, the same for every chunk of the column
    if (kind == RAW_K_DATE) {                // one Date per part: nothing to gather
        const uint32_t v = a.date | (a.date << 16);
        for (uint32_t j = tid; j < RAW_TILE_DWORDS + 4; j += RAW_BLOCK) lds[j] = v;
    } else {
        const uint32_t dpe = d.width >> 2;  // dwords per element: 1, 2, 4
        const long long e0 = k0 >> (dpe >> 1);  // first element that touches the staged dwords (floor)
        const uint32_t nelem = (RAW_TILE_DWORDS + 1) / dpe + 2;
        for (uint32_t j = tid; j < nelem; j += RAW_BLOCK) {
            const long long e = e0 + j;
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            if (e >= 0 && e < (long long)rows) raw_load_element(a, kind, a.src[c], (uint32_t)e, v);
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

// ---- loading parts back: the header check and the unpack (host side: raw_load_host.inc) ------------------------------------------
// A part's size fixes its rows: bytes = 110 rows + 284 + len(varuint(rows)) is strictly increasing in rows.  -> false: no row
// count gives this size.
__host__ __device__ inline bool raw_rows_from_bytes(const RawColDef* cols, uint64_t bytes, uint64_t* rows) {
    const uint64_t fixed = raw_col_offset(cols, 0, RAW_NCOLS) - 1;  // the 16 column headers and the column count's byte: 284
    for (uint32_t l = 1; l <= 10; l++) {
        if (bytes < fixed + l || (bytes - fixed - l) % RAW_ROW_BYTES) continue;
        const uint64_t r = (bytes - fixed - l) / RAW_ROW_BYTES;
        if (raw_varuint_len(r) == l) {
            *rows = r;
            return true;
        }
    }
    return false;
}

// why a part was refused (RawPartVerdict::code)
enum { RAW_V_OK = 0, RAW_V_BLOCK = 1, RAW_V_SIZE = 2, RAW_V_NCOLS = 3, RAW_V_ROWS = 4, RAW_V_NAME = 5, RAW_V_TYPE = 6 };
struct RawPartPlan {
    uint64_t off, bytes;             // where the part starts in the image; its size when the host knows it (plain Native input)
    uint32_t first_block, nblocks;   // an LZ4 frame's blocks (nblocks 0xFFFFFFFF: plain input, `bytes` holds): size = (nblocks - 1) * 65536 + the last one's
};
struct RawPartVerdict {
    uint64_t rows, bytes;
    uint32_t code, at;  // RAW_V_*, and the byte of the part it was found at
};

// One workgroup of 64 threads per part: its size -> rows, then thread c compares column c's header with the expected bytes at
// their computed place and thread 0 the column count and varuint(rows).  Reads only the first bytes of the part's span that
// the header places need, all inside [off, off + bytes).  block_size[4 * b + 2]: the decoded bytes of block b, [4 * b]: its error.
__global__ __launch_bounds__(64) void raw_header_check_kernel(const RawPartPlan* __restrict__ plan, const uint32_t* __restrict__ block_status, const uint8_t* __restrict__ img,
                                                              RawPartVerdict* __restrict__ verdict) {
    __shared__ uint32_t worst;  // the smallest (byte position << 4 | code) any thread found
    const RawPartPlan p = plan[blockIdx.x];
    const uint32_t t = threadIdx.x;
    uint64_t bytes = p.bytes;
    bool blocks_ok = true;
    if (p.nblocks != 0xFFFFFFFFu) {
        bytes = 0;
        for (uint32_t j = 0; j < p.nblocks; j++) {  // (every thread walks the few words: uniform)
            blocks_ok = blocks_ok && block_status[4 * (size_t)(p.first_block + j)] == 0;
            bytes += block_status[4 * (size_t)(p.first_block + j) + 2];
        }
    }
    uint64_t rows = 0;
    const bool fits = blocks_ok && raw_rows_from_bytes(RAW_COLS_D, bytes, &rows);
    if (t == 0) worst = 0xFFFFFFFFu;
    __syncthreads();
    if (fits) {
        const uint8_t* part = img + p.off;
        auto bad = [&](uint64_t at, uint32_t code) { atomicMin(&worst, (uint32_t)(at << 4) | code); };  // (header places lie below 2^9)
        if (t == 0) {
            if (part[0] != RAW_NCOLS) bad(0, RAW_V_NCOLS);
            uint64_t v = rows;
            uint32_t i = 1;
            for (; v >= 128; v >>= 7, i++)
                if (part[i] != (uint8_t)(v | 128)) bad(i, RAW_V_ROWS);
            if (part[i] != (uint8_t)v) bad(i, RAW_V_ROWS);
        }
        if (t < RAW_NCOLS) {
            const RawColDef& d = RAW_COLS_D[t];
            const uint8_t* h = part + raw_col_offset(RAW_COLS_D, rows, t);
            // (a later column's header lies far up in the part: the COLUMN's index is reported as the place)
            if (h[0] != d.name_len) bad(t, RAW_V_NAME);
            else {
                bool ok = true;
                for (uint32_t i = 0; i < d.name_len; i++) ok = ok && h[1 + i] == (uint8_t)d.name[i];
                if (!ok) bad(t, RAW_V_NAME);
                else if (h[1 + d.name_len] != d.type_len) bad(t, RAW_V_TYPE);
                else {
                    for (uint32_t i = 0; i < d.type_len; i++) ok = ok && h[2 + d.name_len + i] == (uint8_t)d.type[i];
                    if (!ok) bad(t, RAW_V_TYPE);
                }
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        RawPartVerdict v{rows, bytes, RAW_V_OK, 0};
        if (!blocks_ok) v.code = RAW_V_BLOCK;
        else if (!fits) v.code = RAW_V_SIZE;
        else if (worst != 0xFFFFFFFFu) v.code = worst & 15, v.at = worst >> 4;
        verdict[blockIdx.x] = v;
    }
}

// raw_unpack_kernel: the inverse of raw_gather_kernel.  Rows [r0, r0 + m) of ONE part become fa_columns arrays (dst[c]: where
// the range's first element of column c goes: naturally aligned, at any element of its array).  Date is skipped (the grid's y
// runs over columns 1 .. 15), TimeReceived and TimeFlowStart widen from 4 to 8 bytes (t32 zero-extended); status is zeroed by the
// host (a memset on the same stream).
// A column's source starts at ANY byte phase of the image, and the phase changes with `rows`.  The kernel's wide accesses are all
// naturally aligned: thread k of a column owns the k-th 16-byte-ALIGNED chunk of the destination range, loads the one or two
// ALIGNED 16-byte words that cover the chunk's source bytes (16 of them; 8 for a widened column), shifts them by the source's byte
// phase - the same for every chunk of the column (bytes16_at_phase) - and issues ONE aligned 16-byte store.  Only a chunk the
// range covers partly (its first and last), and a chunk whose aligned loads would leave the part's span [lo, hi), go byte by byte:
// single-byte loads in a loop that is not unrolled, so that the compiler cannot merge them into a wider load at the bytes' phase,
// and byte stores (8-byte stores for a widened column, whose elements are 8-byte aligned).  Nothing is read outside [lo, hi),
// nothing is written outside the m elements.
struct RawUnpackArgs {
    const uint8_t* part;     // the part's first byte
    const uint8_t *lo, *hi;  // the part's span: part .. part + bytes
    void* dst[RAW_NCOLS];
    uint32_t rows, r0, m;
};
__global__ __launch_bounds__(RAW_BLOCK) void raw_unpack_kernel(const RawUnpackArgs a) {
    const uint32_t c = blockIdx.y + 1;  // (Date is skipped)
    const RawColDef& d = RAW_COLS_D[c];
    const uint32_t w = d.width;
    const bool widen = d.kind == RAW_K_KEY || d.kind == RAW_K_NARROW64;
    uint8_t* const d0 = (uint8_t*)a.dst[c];
    uint8_t* const d1 = d0 + (uint64_t)a.m * (widen ? 8 : w);  // the destination range [d0, d1)
    uint8_t* const t = d0 - ((uintptr_t)d0 & 15) + 16 * ((uint64_t)blockIdx.x * RAW_BLOCK + threadIdx.x);  // this thread's aligned chunk
    if (t >= d1) return;
    const uint8_t* const s0 = a.part + raw_col_offset(RAW_COLS_D, a.rows, c) + raw_col_header_len(d) + (uint64_t)a.r0 * w;
    const bool whole = t >= d0 && t + 16 <= d1;
    // the chunk's source bytes: 16, or the 8 of its two elements ((t - d0) is a multiple of 8 there; in front of s0 where t < d0: not read)
    const uint32_t nsrc = widen ? 8 : 16;
    const uint8_t* s = s0 + (widen ? (t - d0) / 2 : (t - d0));
    const uint32_t sh = (uint32_t)((uintptr_t)s & 15);
    const uint8_t* al = s - sh;
    const bool two = sh + nsrc > 16;  // the bytes reach into the next aligned word
    if (whole && al >= a.lo && al + (two ? 32 : 16) <= a.hi) {
        const uint4 x = *(const uint4*)al;
        const uint4 y = two ? *(const uint4*)(al + 16) : make_uint4(0, 0, 0, 0);
        const uint4 o = bytes16_at_phase(x, y, sh);
        *(uint4*)t = widen ? make_uint4(o.x, 0u, o.y, 0u) : o;
        return;
    }
    // (one single-byte load per trip of a loop that is NOT unrolled: unrolled, the compiler merges neighbouring byte loads into
    // one wider load at the bytes' phase)
    if (!widen) {
#pragma nounroll
        for (int i = 0; i < 16; i++)
            if (t + i >= d0 && t + i < d1) t[i] = s[i];
    } else {
        uint32_t v = 0;
#pragma nounroll
        for (int i = 0; i < 8; i++)
            if (t + 2 * (i & 4) >= d0 && t + 2 * (i & 4) < d1) {  // element i / 4 of the chunk lies in the range
                v |= (uint32_t)s[i] << (8 * (i & 3));
                if ((i & 3) == 3) *(uint64_t*)(t + 2 * (i & 4)) = v, v = 0;
            }
    }
}

}  // namespace fa
