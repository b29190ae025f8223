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
// The part writer (raw_write_tile), the hot part, shared by every kernel that writes a part (raw_gather_kernel here,
// raw_merge_gather_kernel of raw_merge.cuh): they differ in where an element's dwords come from, the `load` they hand in.
// Headers have odd lengths and the first column is 2 bytes wide, so a 4-, 8- or 16-byte column starts at ANY byte offset of the
// image, and the offset changes with `rows`.  The writer never issues a store that is off its natural alignment: a workgroup owns
// RAW_TILE_CHUNKS consecutive 16-byte-ALIGNED chunks of one column's byte range, stages the column's dwords that cover them in
// LDS, and every lane then reads five LDS dwords, shifts them by the column's byte phase (v_alignbyte) and issues ONE aligned
// 16-byte store.  The first and last chunk of a column, which the column only partly covers, leave as byte stores; so do the
// headers.  Every byte of the part is written exactly once, by exactly one lane.  The geometry - workgroup -> (column, tile),
// tile -> byte phase, lane -> chunk, element -> LDS slot - is plain __host__ __device__ text that the host calls too: to size the
// grid (raw_part_tiles) and to enumerate the walk (tests/host_raw_merge.hip).
// raw_gather_kernel's load: natural-width, coalesced-where-sorted reads of the decoded columns through the sort's index.
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

// ---- the part writer's geometry: a part of `rows` rows whose first byte has the address `base` (its low 4 bits matter) ---------
// the tiles of column d, whose header stands at `off`; next: where the following column's header stands
__host__ __device__ __forceinline__ uint64_t raw_col_step(const RawColDef& d, uint64_t base, uint64_t rows, uint64_t off, uint64_t* next) {
    const uint64_t data = off + raw_col_header_len(d), bytes = rows * d.width;
    *next = data + bytes;
    return raw_col_tiles(base + data, bytes);
}
// the workgroups one part takes: every column's tiles
__host__ __device__ inline uint64_t raw_part_tiles(const RawColDef* cols, uint64_t base, uint64_t rows) {
    uint64_t tiles = 0, off = 1 + raw_varuint_len(rows);
    for (uint32_t c = 0; c < RAW_NCOLS; c++) tiles += raw_col_step(cols[c], base, rows, off, &off);
    return tiles;
}
struct RawTile {
    uint32_t c;          // the column
    uint64_t tile, off;  // the tile inside the column; the column header's offset in the part (== raw_col_offset)
};
// workgroup wg -> its tile: a few uniform steps over the 16 columns.  false: the part has no such tile.  (Every workgroup runs
// this in front of 4 KiB of work.  The loop leaves from its body and has no bound in its head: the compiler unrolls that shape by
// two; written as `for (c = 0; c < RAW_NCOLS; ...)` both gathers measured 0.006 ns per row slower, 6 % of the build's.)
__host__ __device__ __forceinline__ bool raw_tile_locate(const RawColDef* cols, uint64_t base, uint64_t rows, uint64_t wg, RawTile* t) {
    uint64_t off = 1 + raw_varuint_len(rows), next;
    uint32_t c = 0;
    for (;; c++, off = next) {
        if (c == RAW_NCOLS) return false;
        const uint64_t tiles = raw_col_step(cols[c], base, rows, off, &next);
        if (wg < tiles) break;
        wg -= tiles;
    }
    *t = RawTile{c, wg, off};
    return true;
}
struct RawTilePhase {
    long long s, k0;  // the column byte the tile's first aligned chunk starts at (negative in the first tile unless the column is
                      // aligned); the first staged dword (floor: s may be negative)
    uint32_t sh;      // the byte phase, the same for every chunk of the column
};
// col: the address of the column's first data byte
__host__ __device__ __forceinline__ RawTilePhase raw_tile_phase(uint64_t col, uint64_t tile) {
    const long long s = (long long)tile * (RAW_TILE_CHUNKS * 16) - (long long)(col & 15);
    return RawTilePhase{s, s >> 2, (uint32_t)(s & 3)};
}
// the column byte lane tid's chunk starts at; what the chunk is to a column of `bytes` bytes: outside it (no store), whole (one
// aligned 16-byte store), or neither - the column's first or last chunk, partly covered: byte stores for the bytes that are the
// column's.  b > -16 always (raw_tile_phase: s >= -15), so a chunk is outside only behind the column; the byte test is ONE unsigned
// compare, 0 <= b + i < bytes.  (Spelled so, the store tail compiles to the instructions it had when it stood in the kernels: behind
// the function boundary the compiler no longer folds `b + 16 <= 0` away nor the signed pair `b + i >= 0 && b + i < bytes` into one.)
__host__ __device__ __forceinline__ long long raw_lane_byte(long long s, uint32_t tid) { return s + 16ll * tid; }
__host__ __device__ __forceinline__ bool raw_chunk_outside(long long b, long long bytes) { return b >= bytes; }
__host__ __device__ __forceinline__ bool raw_chunk_whole(long long b, long long bytes) { return b >= 0 && b + 16 <= bytes; }
__host__ __device__ __forceinline__ bool raw_chunk_byte_in(long long b, int i, long long bytes) { return (unsigned long long)(b + i) < (unsigned long long)bytes; }
// Staging, for elements of dpe = 1, 2, 4 dwords: LDS slot l holds the column's dword k0 + l, lane tid reads the slots
// 4 tid .. 4 tid + 4, so the slots 0 .. RAW_TILE_DWORDS are staged.  They belong to at most (RAW_TILE_DWORDS + 1) / dpe + 2
// consecutive elements from raw_stage_first on (the run may begin and end inside an element); an element outside [0, rows) stages
// zeroes into slots no byte of the column lies in.
__host__ __device__ __forceinline__ long long raw_stage_first(long long k0, uint32_t dpe) { return k0 >> (dpe >> 1); }  // (floor)
__host__ __device__ __forceinline__ uint32_t raw_stage_count(uint32_t dpe) { return (RAW_TILE_DWORDS + 1) / dpe + 2; }
// the slot of dword q of element e, and whether it is one of the staged ones
__host__ __device__ __forceinline__ long long raw_stage_slot(long long e, uint32_t dpe, uint32_t q, long long k0) { return e * dpe + q - k0; }
__host__ __device__ __forceinline__ bool raw_stage_holds(long long l) { return l >= 0 && l <= (long long)RAW_TILE_DWORDS; }

// ---- header bytes ------------------------------------------------------------------------------------------------------------
// varuint(v) at p -> its length
__host__ __device__ inline uint32_t raw_put_varuint(uint8_t* p, uint64_t v) {
    uint32_t n = 0;
    while (v >= 128) p[n++] = (uint8_t)(v | 128), v >>= 7;
    p[n++] = (uint8_t)v;
    return n;
}
// byte i of a column's header: varuint(name_len) name varuint(type_len) type (both lengths are below 128: one byte each)
__host__ __device__ __forceinline__ uint8_t raw_col_header_byte(const RawColDef& d, uint32_t i) {
    if (i == 0) return d.name_len;
    if (i <= d.name_len) return (uint8_t)d.name[i - 1];
    if (i == 1u + d.name_len) return d.type_len;
    return (uint8_t)d.type[i - 2 - d.name_len];
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

// dwords [e * dpe, (e + 1) * dpe) of a column's byte stream: element e in sorted order (0 <= e < rows) of a decoded column
__device__ __forceinline__ void raw_load_element(const RawGatherArgs& a, uint32_t kind, const void* src, uint32_t e, uint32_t v[4]) {
    switch (kind) {
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

// One tile of a part, by one workgroup of RAW_BLOCK threads: the headers (tile 0), the column's dwords into lds[RAW_TILE_DWORDS + 4]
// (16-byte aligned) - the Date constant, key[e] for TimeReceived, load(e, v) for every other column -, then one store per lane.
// `key`: the part's sorted keys.  load(e, v): the dwords of sorted element e (0 <= e < rows) of column t.c into v[0 .. width / 4).
template <class Load>
__device__ __forceinline__ void raw_write_tile(uint32_t* lds, uint8_t* part, uint32_t rows, uint32_t date, const uint32_t* key, const RawTile& t, Load load) {
    const uint32_t tid = threadIdx.x;
    const RawColDef& d = RAW_COLS_D[t.c];
    const uint32_t hl = raw_col_header_len(d);
    uint8_t* const col = part + t.off + hl;  // the column's first data byte
    const long long bytes = (long long)((uint64_t)rows * d.width);
    if (t.tile == 0) {  // the column's header, and in front of the first column the block's
        if (tid < hl) part[t.off + tid] = raw_col_header_byte(d, tid);
        if (t.c == 0 && tid == 0) part[0] = (uint8_t)RAW_NCOLS, raw_put_varuint(part + 1, rows);
    }
    const RawTilePhase ph = raw_tile_phase((uint64_t)(uintptr_t)col, t.tile);
    if (d.kind == RAW_K_DATE) {  // one Date per part: nothing to gather
        const uint32_t v = date | (date << 16);
        for (uint32_t j = tid; j < RAW_TILE_DWORDS + 4; j += RAW_BLOCK) lds[j] = v;
    } else {
        const uint32_t dpe = d.width >> 2;  // dwords per element: 1, 2, 4
        const long long e0 = raw_stage_first(ph.k0, dpe);
        for (uint32_t j = tid; j < raw_stage_count(dpe); j += RAW_BLOCK) {
            const long long e = e0 + j;
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            if (e >= 0 && e < (long long)rows) {
                if (d.kind == RAW_K_KEY) v[0] = key[e];
                else load((uint32_t)e, v);
            }
            for (uint32_t q = 0; q < dpe; q++) {
                const long long l = raw_stage_slot(e, dpe, q, ph.k0);
                if (raw_stage_holds(l)) lds[l] = v[q];
            }
        }
    }
    __syncthreads();
    const long long b = raw_lane_byte(ph.s, tid);
    if (raw_chunk_outside(b, bytes)) return;
    const uint4 lo = *(const uint4*)&lds[4 * tid];
    const uint32_t hi = lds[4 * tid + 4];
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(lo.y, lo.x, ph.sh);
    o.y = __builtin_amdgcn_alignbyte(lo.z, lo.y, ph.sh);
    o.z = __builtin_amdgcn_alignbyte(lo.w, lo.z, ph.sh);
    o.w = __builtin_amdgcn_alignbyte(hi, lo.w, ph.sh);
    uint8_t* const dst = col + b;  // 16-byte aligned by construction
    if (raw_chunk_whole(b, bytes)) {
        *(uint4*)dst = o;
    } else {  // the column's first or last chunk: only the bytes that are the column's
        const uint32_t w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (raw_chunk_byte_in(b, i, bytes)) dst[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

__global__ __launch_bounds__(RAW_BLOCK) void raw_gather_kernel(const RawGatherArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[RAW_TILE_DWORDS + 4];
    RawTile t;
    if (!raw_tile_locate(RAW_COLS_D, (uint64_t)(uintptr_t)a.part, a.rows, blockIdx.x, &t)) return;  // (the host launches exactly the tiles there are)
    const uint32_t kind = RAW_COLS_D[t.c].kind;
    const void* const src = a.src[t.c];
    raw_write_tile(lds, a.part, a.rows, a.date, a.key, t, [&](uint32_t e, uint32_t* v) { raw_load_element(a, kind, src, e, v); });
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
