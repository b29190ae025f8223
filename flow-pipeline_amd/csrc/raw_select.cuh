// raw_select.cuh - selecting rows of flows_raw parts on the device: a predicate over the columns where they lie in the decoded
// image, an order-preserving compaction, and the index the part writer gathers through (gfx950; host side: raw_select_host.inc;
// the contract: include/flowagg.h "selecting rows of flows_raw parts"; run on the host by tests/host_raw_select.hip).
//
// The input is what a ranged load leaves (raw_range_host.inc): of every part with a row in the time range the slice [r_lo, r_hi),
// the headers and the TimeReceived column decoded by stage B, the slice's elements of columns 2 .. 15 by stage C.
//
// raw_select_kernel, the hot part.  ONE flattened grid over the slices of all parts of the call: a workgroup owns RAW_SEL_BLOCK
// consecutive rows of ONE slice (RawSelectPart::tile0 is a slice's first workgroup, found by raw_range_kernel's uniform
// bisection), a lane owns one row, a wave 64 consecutive rows.  A value is read where it lies in the image, at the column's own
// byte phase: raw_merge_src_offset + raw_load_unaligned of raw_merge.cuh, an element-width read at the element's own address.
// WHY NO EDGE PATH: a read of exactly the element's bytes touches bytes [o, o + width) of the part with o = the offset of row r of
// column c, r_lo <= r < r_hi, c in 2 .. 15: those are bytes of raw_range_load_spans(rows, r_lo, r_hi), every block of which
// stage C planned and decoded (plain input: the part is whole).  The emit kernel reads TimeReceived of such rows: bytes of
// raw_range_scan_spans, stage B's.  Nothing else is read: no aligned word around an element, nothing of a row outside the
// slice.  (tests/host_raw_select.hip enumerates these bytes against the planned blocks.)
// Only the columns the filter names are read (raw_select_cols): `fields` is wave-uniform, a condition that is not set costs a
// scalar branch.  The 4-byte conditions come first; a 16-byte address column is loaded only while a lane of the wave is still
// alive (__ballot), only by those lanes, and with EITHER each address column at most once for both directions.  TimeReceived is
// not read: stage B proved the slice.  Output: one 64-bit mask word per wave (__ballot is 64 bits wide here; lane 0 stores it)
// and one count per workgroup (LDS, thread 0).  No atomic, no scratch.
//
// The positions: an exclusive scan over the workgroup counts (hipcub, as the build's order step), raw_select_totals_kernel turns
// it into one total per slice, which the host reads: the output's layout depends on them.
//
// raw_select_emit_kernel: the same grid; a set lane's position in its part's output is the scanned base of its workgroup minus
// that of the slice's first, plus the popcounts of the earlier words of the workgroup, plus the set bits below its lane
// (raw_select_pos).  Positions below the part's (limit-capped) count write idx[pos] = the GLOBAL row - numbered over the slices'
// parts laid end to end, RawMergeSrc::first - and key[pos] = the row's TimeReceived; the first and last position write the
// output part's t_min and t_max.  Rows keep their order: the output part is sorted.
// The gather is raw_merge_gather_kernel as it is, one launch per output part.
//
// The predicate (raw_select_eval: staged exactly as the kernel runs it; raw_select_match: the same text over a loaded row), the
// prefix comparison and the position rule are __host__ __device__ text: the CPU test runs them against naive restatements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/flowagg.h"
#include "raw.cuh"
#include "raw_merge.cuh"

namespace fa {

constexpr uint32_t RAW_SEL_BLOCK = 256;              // rows per workgroup
constexpr uint32_t RAW_SEL_WAVES = RAW_SEL_BLOCK / 64;
// the columns of RAW_COLS a filter reads
enum {
    RAW_SEL_C_TIME = 1, RAW_SEL_C_FLOW_START = 2, RAW_SEL_C_SRC_ADDR = 6, RAW_SEL_C_DST_ADDR = 7, RAW_SEL_C_SRC_AS = 8, RAW_SEL_C_DST_AS = 9,
    RAW_SEL_C_ETYPE = 10, RAW_SEL_C_PROTO = 11, RAW_SEL_C_SRC_PORT = 12, RAW_SEL_C_DST_PORT = 13
};

struct RawSelectPart {
    uint64_t off;         // where the part starts in the image
    uint32_t rows;        // the part's rows
    uint32_t r_lo, r_hi;  // the slice, r_lo < r_hi
    uint32_t tile0;       // the slice's first workgroup of the flattened grid (ascending over the list)
    uint32_t first;       // the global number of the part's row 0 (RawMergeSrc::first)
    uint32_t _pad;
};
struct RawSelectOut {
    uint32_t out0, cap;  // where the part's output starts in idx / key; the rows it delivers (its count, capped by the limit)
};
struct RawSelectSpan {
    uint32_t t_min, t_max;  // key of the first and of the last delivered row of a part
};
static_assert(sizeof(RawSelectPart) == 32 && sizeof(RawSelectOut) == 8 && sizeof(RawSelectSpan) == 8, "plans and records of the select kernels");
__host__ __device__ __forceinline__ uint64_t raw_select_tiles(uint64_t slice_rows) { return (slice_rows + RAW_SEL_BLOCK - 1) / RAW_SEL_BLOCK; }

// ---- the predicate -----------------------------------------------------------------------------------------------------------
// a row's values of the columns a filter can name; the addresses as the four little-endian dwords of the stored 16 bytes
struct RawSelectRow {
    uint32_t time_flow_start, src_as, dst_as, etype, proto, src_port, dst_port;
    uint32_t src_addr[4], dst_addr[4];
};

// lo <= t < hi; hi == 0xFFFFFFFF: to the end, that second included (raw_range_elem's rule)
__host__ __device__ __forceinline__ bool raw_select_in_range(uint32_t t, uint32_t lo, uint32_t hi) { return t >= lo && (hi == 0xFFFFFFFFu || t < hi); }

// the first `len` bits (0 .. 128) of two 16-byte strings, from byte 0 on and most significant bit first, are equal.  a, b: the
// strings' little-endian dwords, so a byte swap puts a dword's bytes in string order.
__host__ __device__ __forceinline__ bool raw_select_prefix_eq(const uint32_t a[4], const uint32_t b[4], uint32_t len) {
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
        const uint32_t bits = len > 32 * w ? (len - 32 * w < 32 ? len - 32 * w : 32u) : 0u;  // of this dword
        const uint32_t m = bits == 0 ? 0u : bits == 32 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> bits);
        diff |= (__builtin_bswap32(a[w]) ^ __builtin_bswap32(b[w])) & m;
    }
    return diff == 0;
}

// bit c set: the filter reads column c of RAW_COLS (TimeReceived is never read by the predicate)
__host__ __device__ __forceinline__ uint32_t raw_select_cols(uint32_t fields) {
    const bool e = fields & FA_RAW_F_EITHER;
    const bool s_as = fields & FA_RAW_F_SRC_AS, d_as = fields & FA_RAW_F_DST_AS, s_p = fields & FA_RAW_F_SRC_PORT, d_p = fields & FA_RAW_F_DST_PORT;
    const bool s_a = fields & FA_RAW_F_SRC_ADDR, d_a = fields & FA_RAW_F_DST_ADDR;
    uint32_t m = 0;
    if (fields & FA_RAW_F_FLOW_START) m |= 1u << RAW_SEL_C_FLOW_START;
    if (fields & FA_RAW_F_ETYPE) m |= 1u << RAW_SEL_C_ETYPE;
    if (fields & FA_RAW_F_PROTO) m |= 1u << RAW_SEL_C_PROTO;
    if (s_as || (e && d_as)) m |= 1u << RAW_SEL_C_SRC_AS;
    if (d_as || (e && s_as)) m |= 1u << RAW_SEL_C_DST_AS;
    if (s_p || (e && d_p)) m |= 1u << RAW_SEL_C_SRC_PORT;
    if (d_p || (e && s_p)) m |= 1u << RAW_SEL_C_DST_PORT;
    if (s_a || (e && d_a)) m |= 1u << RAW_SEL_C_SRC_ADDR;
    if (d_a || (e && s_a)) m |= 1u << RAW_SEL_C_DST_ADDR;
    return m;
}
// the bytes of a row the predicate reads
__host__ __device__ inline uint32_t raw_select_row_bytes(const RawColDef* cols, uint32_t fields) {
    uint32_t b = 0;
    for (uint32_t c = 0, m = raw_select_cols(fields); c < RAW_NCOLS; c++)
        if (m >> c & 1) b += cols[c].width;
    return b;
}

// The predicate in the stages the kernel runs it in.  valid: the lane has a row.  load4(c) -> the row's value of the 4-byte
// column c; load16(c, v): its 16 bytes of column c as dwords - called only where the result can still depend on it; any(x):
// whether x holds for some row evaluated together with this one (the kernel: a non-zero __ballot; one row alone: x itself).
template <class Load4, class Load16, class Any>
__host__ __device__ __forceinline__ bool raw_select_eval(const fa_raw_filter& f, bool valid, Load4 load4, Load16 load16, Any any) {
    const uint32_t fl = f.fields;
    const uint32_t cols = raw_select_cols(fl);
    const bool either = fl & FA_RAW_F_EITHER;
    bool alive = valid;
    if (fl & FA_RAW_F_FLOW_START) alive = raw_select_in_range(load4(RAW_SEL_C_FLOW_START), f.tf_lo, f.tf_hi) && alive;
    if (fl & FA_RAW_F_ETYPE) alive = load4(RAW_SEL_C_ETYPE) == f.etype && alive;
    if (fl & FA_RAW_F_PROTO) alive = load4(RAW_SEL_C_PROTO) == f.proto && alive;
    bool d0 = alive, d1 = alive && either;  // P(Src, Dst), P(Dst, Src) so far
    if (fl & (FA_RAW_F_SRC_AS | FA_RAW_F_DST_AS)) {
        const uint32_t s = cols >> RAW_SEL_C_SRC_AS & 1 ? load4(RAW_SEL_C_SRC_AS) : 0u, d = cols >> RAW_SEL_C_DST_AS & 1 ? load4(RAW_SEL_C_DST_AS) : 0u;
        if (fl & FA_RAW_F_SRC_AS) d0 = d0 && s == f.src_as, d1 = d1 && d == f.src_as;
        if (fl & FA_RAW_F_DST_AS) d0 = d0 && d == f.dst_as, d1 = d1 && s == f.dst_as;
    }
    if (fl & (FA_RAW_F_SRC_PORT | FA_RAW_F_DST_PORT)) {
        const uint32_t s = cols >> RAW_SEL_C_SRC_PORT & 1 ? load4(RAW_SEL_C_SRC_PORT) : 0u, d = cols >> RAW_SEL_C_DST_PORT & 1 ? load4(RAW_SEL_C_DST_PORT) : 0u;
        if (fl & FA_RAW_F_SRC_PORT) d0 = d0 && s >= f.src_port_lo && s <= f.src_port_hi, d1 = d1 && d >= f.src_port_lo && d <= f.src_port_hi;
        if (fl & FA_RAW_F_DST_PORT) d0 = d0 && d >= f.dst_port_lo && d <= f.dst_port_hi, d1 = d1 && s >= f.dst_port_lo && s <= f.dst_port_hi;
    }
    if ((fl & (FA_RAW_F_SRC_ADDR | FA_RAW_F_DST_ADDR)) && any(d0 || d1)) {
        uint32_t s[4] = {0u, 0u, 0u, 0u}, d[4] = {0u, 0u, 0u, 0u}, fs[4], fd[4];
        if (d0 || d1) {  // (each column at most once, for both directions)
            if (cols >> RAW_SEL_C_SRC_ADDR & 1) load16(RAW_SEL_C_SRC_ADDR, s);
            if (cols >> RAW_SEL_C_DST_ADDR & 1) load16(RAW_SEL_C_DST_ADDR, d);
        }
        memcpy(fs, f.src_addr, 16), memcpy(fd, f.dst_addr, 16);
        if (fl & FA_RAW_F_SRC_ADDR) d0 = d0 && raw_select_prefix_eq(s, fs, f.src_prefix_len), d1 = d1 && raw_select_prefix_eq(d, fs, f.src_prefix_len);
        if (fl & FA_RAW_F_DST_ADDR) d0 = d0 && raw_select_prefix_eq(d, fd, f.dst_prefix_len), d1 = d1 && raw_select_prefix_eq(s, fd, f.dst_prefix_len);
    }
    return d0 || d1;
}

// whether a row of the time range matches the filter (the time range itself is the slice: stage B's)
__host__ __device__ inline bool raw_select_match(const RawSelectRow& r, const fa_raw_filter& f) {
    return raw_select_eval(
        f, true,
        [&](uint32_t c) {
            switch (c) {
            case RAW_SEL_C_FLOW_START: return r.time_flow_start;
            case RAW_SEL_C_SRC_AS: return r.src_as;
            case RAW_SEL_C_DST_AS: return r.dst_as;
            case RAW_SEL_C_ETYPE: return r.etype;
            case RAW_SEL_C_PROTO: return r.proto;
            case RAW_SEL_C_SRC_PORT: return r.src_port;
            default: return r.dst_port;
            }
        },
        [&](uint32_t c, uint32_t* v) {
            for (int i = 0; i < 4; i++) v[i] = c == RAW_SEL_C_SRC_ADDR ? r.src_addr[i] : r.dst_addr[i];
        },
        [](bool x) { return x; });
}

// why a filter is refused (nullptr: it is not)
inline const char* raw_select_filter_why(const fa_raw_filter& f) {
    if (f.fields & ~FA_RAW_F_ALL) return "an unknown bit in fields";
    if (f._pad[0] || f._pad[1]) return "_pad is not zero";
    if (f.t_lo > f.t_hi) return "t_lo > t_hi";
    if ((f.fields & FA_RAW_F_FLOW_START) && f.tf_lo > f.tf_hi) return "tf_lo > tf_hi";
    if ((f.fields & FA_RAW_F_SRC_PORT) && f.src_port_lo > f.src_port_hi) return "src_port_lo > src_port_hi";
    if ((f.fields & FA_RAW_F_DST_PORT) && f.dst_port_lo > f.dst_port_hi) return "dst_port_lo > dst_port_hi";
    if ((f.fields & FA_RAW_F_SRC_ADDR) && f.src_prefix_len > 128) return "src_prefix_len above 128";
    if ((f.fields & FA_RAW_F_DST_ADDR) && f.dst_prefix_len > 128) return "dst_prefix_len above 128";
    return nullptr;
}

// ---- the position rule ---------------------------------------------------------------------------------------------------------
// base: the matches of the part in front of the lane's workgroup; words: the workgroup's RAW_SEL_WAVES mask words
__host__ __device__ __forceinline__ uint32_t raw_select_pos(uint32_t base, const uint64_t* words, uint32_t wave, uint32_t lane) {
    uint32_t pos = base;
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t w = 0; w < RAW_SEL_WAVES; w++) {  // (no indexing by `wave`: the words stay in registers)
        if (w < wave) pos += (uint32_t)__builtin_popcountll(words[w]);
        if (w == wave) mine = words[w];
    }
    return pos + (uint32_t)__builtin_popcountll(mine & (((uint64_t)1 << lane) - 1));
}

// the last slice whose tile0 <= wg (uniform; raw_range_kernel's bisection)
__device__ __forceinline__ uint32_t raw_select_find(const RawSelectPart* __restrict__ parts, uint32_t nparts, uint32_t wg) {
    uint32_t pa = 0, pb = nparts;
    while (pb - pa > 1) {
        const uint32_t mid = (pa + pb) >> 1;
        if (parts[mid].tile0 <= wg) pa = mid;
        else pb = mid;
    }
    return pa;
}

__global__ __launch_bounds__(RAW_SEL_BLOCK) void raw_select_kernel(const RawSelectPart* __restrict__ parts, uint32_t nparts, const uint8_t* __restrict__ img, const fa_raw_filter f,
                                                                   uint64_t* __restrict__ mask, uint32_t* __restrict__ count) {
    __shared__ uint32_t wc[RAW_SEL_WAVES];
    const RawSelectPart p = parts[raw_select_find(parts, nparts, blockIdx.x)];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t r = (uint64_t)p.r_lo + (uint64_t)(blockIdx.x - p.tile0) * RAW_SEL_BLOCK + tid;  // (the host launches exactly the tiles there are)
    const bool valid = r < p.r_hi;
    const uint8_t* const part = img + p.off;
    const bool hit = raw_select_eval(
        f, valid,
        [&](uint32_t c) { return valid ? raw_load_unaligned32(part + raw_merge_src_offset(raw_merge_col(RAW_COLS_D, c), p.rows, r)) : 0u; },
        [&](uint32_t c, uint32_t* v) { raw_load_unaligned(part + raw_merge_src_offset(raw_merge_col(RAW_COLS_D, c), p.rows, r), 4, v); },
        [](bool x) { return __ballot(x) != 0; });
    const uint64_t m = __ballot(hit);
    if (lane == 0) mask[(uint64_t)blockIdx.x * RAW_SEL_WAVES + wave] = m, wc[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (tid == 0) {
        uint32_t n = 0;
        for (uint32_t w = 0; w < RAW_SEL_WAVES; w++) n += wc[w];
        count[blockIdx.x] = n;
    }
}

// base: the exclusive scan of the workgroup counts, ntiles + 1 words -> one total per slice
__global__ __launch_bounds__(256) void raw_select_totals_kernel(const RawSelectPart* __restrict__ parts, uint32_t nparts, uint32_t ntiles, const uint32_t* __restrict__ base,
                                                                uint32_t* __restrict__ total) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nparts) return;
    total[j] = base[j + 1 < nparts ? parts[j + 1].tile0 : ntiles] - base[parts[j].tile0];
}

// idx == nullptr (COUNT_ONLY): the spans alone
__global__ __launch_bounds__(RAW_SEL_BLOCK) void raw_select_emit_kernel(const RawSelectPart* __restrict__ parts, uint32_t nparts, const uint8_t* __restrict__ img,
                                                                        const uint64_t* __restrict__ mask, const uint32_t* __restrict__ base, const RawSelectOut* __restrict__ out,
                                                                        uint32_t* __restrict__ idx, uint32_t* __restrict__ key, RawSelectSpan* __restrict__ span) {
    const uint32_t pa = raw_select_find(parts, nparts, blockIdx.x);
    const RawSelectPart p = parts[pa];
    const RawSelectOut o = out[pa];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t words[RAW_SEL_WAVES];
#pragma unroll
    for (uint32_t w = 0; w < RAW_SEL_WAVES; w++) words[w] = mask[(uint64_t)blockIdx.x * RAW_SEL_WAVES + w];
    uint64_t mine = words[0];
#pragma unroll
    for (uint32_t w = 1; w < RAW_SEL_WAVES; w++) mine = wave == w ? words[w] : mine;
    if (!(mine >> lane & 1)) return;
    const uint32_t pos = raw_select_pos(base[blockIdx.x] - base[p.tile0], words, wave, lane);
    if (pos >= o.cap) return;
    const uint32_t r = p.r_lo + (blockIdx.x - p.tile0) * RAW_SEL_BLOCK + tid;  // (a set bit: r < r_hi <= 2^31)
    const uint32_t t = raw_load_unaligned32(img + p.off + raw_merge_src_offset(raw_merge_col(RAW_COLS_D, RAW_SEL_C_TIME), p.rows, r));
    if (idx) idx[o.out0 + pos] = p.first + r, key[o.out0 + pos] = t;
    if (pos == 0) span[pa].t_min = t;
    if (pos == o.cap - 1) span[pa].t_max = t;
}

}  // namespace fa
