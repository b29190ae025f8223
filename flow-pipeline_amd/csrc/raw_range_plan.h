// raw_range_plan.h - what a ranged load of flows_raw parts decides without a GPU (host side: raw_range_host.inc; the kernel:
// raw_range.cuh; the contract: include/flowagg.h "ranged loads of flows_raw parts"; run on the host by tests/host_raw_range.hip).
//
// A part is one Native block whose columns are contiguous byte ranges (raw.cuh), and an LZ4 frame decodes block j into the
// 64 KiB slot j of the part: byte x of the part lies in block x / 65536 and nowhere else.  A call decodes a block when one of
// its three stages needs a byte of it:
//   A (probe)  the part's first and last block: the decoded size gives the rows, the first bytes the column count,
//              varuint(rows) and Date[0];
//   B (range)  every byte of the part's header, of the 16 column headers and of the TimeReceived column (4 rows bytes);
//   C (load)   every byte of elements [r_lo, r_hi) of columns 2 .. 15.  The Date VALUES are never needed.
// Everything below is over raw_col_offset / raw_col_header_len: there is no second statement of the layout.
// The element predicate of raw_range_kernel and the kernel's chunk geometry are __host__ __device__ text: the host test runs
// them against std::lower_bound and enumerates every address the kernel loads.
#pragma once
#include <stdint.h>

#include <vector>

#include "raw.cuh"

namespace fa {

constexpr uint64_t RAW_SLOT = 65536;  // decoded bytes per LZ4 block but the last (== LZ4_BLOCK_MAX)
constexpr uint32_t RAW_COL_TIME = 1;  // TimeReceived, the parts' sort key
constexpr uint32_t RAW_RANGE_NONE = 0xFFFFFFFFu;

struct RawByteSpan {
    uint64_t lo, hi;  // bytes [lo, hi) of a part
};

// ---- the byte spans a stage reads -----------------------------------------------------------------------------------------
// stage B: the part's header, the 16 column headers, the TimeReceived values -> at most 18 spans
inline uint32_t raw_range_scan_spans(const RawColDef* cols, uint64_t rows, RawByteSpan out[RAW_NCOLS + 2]) {
    uint32_t n = 0;
    out[n++] = RawByteSpan{0, 1 + (uint64_t)raw_varuint_len(rows)};
    for (uint32_t c = 0; c < RAW_NCOLS; c++) {
        const uint64_t o = raw_col_offset(cols, rows, c);
        out[n++] = RawByteSpan{o, o + raw_col_header_len(cols[c])};
    }
    const uint64_t t = raw_col_offset(cols, rows, RAW_COL_TIME) + raw_col_header_len(cols[RAW_COL_TIME]);
    out[n++] = RawByteSpan{t, t + rows * cols[RAW_COL_TIME].width};
    return n;
}
// stage C: elements [r_lo, r_hi) of the columns behind TimeReceived -> 14 spans (empty ones where r_lo == r_hi)
inline uint32_t raw_range_load_spans(const RawColDef* cols, uint64_t rows, uint64_t r_lo, uint64_t r_hi, RawByteSpan out[RAW_NCOLS]) {
    uint32_t n = 0;
    for (uint32_t c = RAW_COL_TIME + 1; c < RAW_NCOLS; c++) {
        const uint64_t d = raw_col_offset(cols, rows, c) + raw_col_header_len(cols[c]);
        out[n++] = RawByteSpan{d + r_lo * cols[c].width, d + r_hi * cols[c].width};
    }
    return n;
}

// ---- the three stage sets of one part -------------------------------------------------------------------------------------
// `done[b]` (one byte per block of the CALL): block b was planned by an earlier stage.  Each function appends, ascending per span,
// the blocks of its set that are not done yet and marks them: a block is decoded at most once per call.  The part's blocks
// are first_block .. first_block + nblocks - 1; a span never reaches behind them (rows comes from their decoded size).
inline void raw_range_take(uint32_t b, std::vector<uint8_t>& done, std::vector<uint32_t>& out) {
    if (!done[b]) done[b] = 1, out.push_back(b);
}
inline void raw_range_take_spans(const RawByteSpan* sp, uint32_t n, uint32_t first_block, uint32_t nblocks, std::vector<uint8_t>& done, std::vector<uint32_t>& out) {
    for (uint32_t i = 0; i < n; i++) {
        if (sp[i].lo >= sp[i].hi) continue;
        for (uint64_t b = sp[i].lo / RAW_SLOT; b <= (sp[i].hi - 1) / RAW_SLOT && b < nblocks; b++) raw_range_take(first_block + (uint32_t)b, done, out);
    }
}
inline void raw_range_probe_blocks(uint32_t first_block, uint32_t nblocks, std::vector<uint8_t>& done, std::vector<uint32_t>& out) {
    if (!nblocks) return;
    raw_range_take(first_block, done, out);
    raw_range_take(first_block + nblocks - 1, done, out);
}
inline void raw_range_scan_blocks(const RawColDef* cols, uint64_t rows, uint32_t first_block, uint32_t nblocks, std::vector<uint8_t>& done, std::vector<uint32_t>& out) {
    RawByteSpan sp[RAW_NCOLS + 2];
    raw_range_take_spans(sp, raw_range_scan_spans(cols, rows, sp), first_block, nblocks, done, out);
}
inline void raw_range_load_blocks(const RawColDef* cols, uint64_t rows, uint32_t first_block, uint32_t nblocks, uint64_t r_lo, uint64_t r_hi, std::vector<uint8_t>& done,
                                  std::vector<uint32_t>& out) {
    RawByteSpan sp[RAW_NCOLS];
    raw_range_take_spans(sp, raw_range_load_spans(cols, rows, r_lo, r_hi, sp), first_block, nblocks, done, out);
}

// ---- partition pruning ----------------------------------------------------------------------------------------------------
// [t_lo, t_hi) as 64-bit bounds: t_hi == 0xFFFFFFFF means "to the end" and includes that second (fa_top_talkers_range)
__host__ __device__ inline uint64_t raw_range_upper(uint32_t t_hi) { return t_hi == 0xFFFFFFFFu ? (uint64_t)1 << 32 : t_hi; }
// a part of Date `date` can hold a row of the range: [date * 86400, date * 86400 + 86400) meets [t_lo, t_hi)
inline bool raw_range_date_meets(uint32_t date, uint32_t t_lo, uint32_t t_hi) {
    const uint64_t d0 = (uint64_t)date * 86400, d1 = d0 + 86400;
    return d0 < raw_range_upper(t_hi) && (uint64_t)t_lo < d1 && (uint64_t)t_lo < raw_range_upper(t_hi);
}

// ---- stage A's look at a part's first bytes ---------------------------------------------------------------------------------
// The column count, varuint(rows), the Date column's header and Date[0] stand in the part's first RAW_PROBE_BYTES bytes for every
// row count a part may have (rows <= 2^31: 1 + 5 + 10 + 2 bytes; tests/host_raw_range.hip walks the varuint steps).
constexpr uint32_t RAW_PROBE_BYTES = 32;
inline uint32_t raw_range_date_at(const RawColDef* cols, uint64_t rows) { return 1 + raw_varuint_len(rows) + raw_col_header_len(cols[0]); }

// ---- the kernel's element predicate ---------------------------------------------------------------------------------------
// What one element t of the TimeReceived column, with its successor where it has one, adds to the part's record.
struct RawRangeElem {
    bool below_lo, below_hi;  // counted into r_lo, r_hi: on a sorted column the two counts are the lower bounds
    bool descends, off_date;  // t > t[i + 1]; t / 86400 is not the part's Date
    bool selected;            // t_lo <= t < t_hi
};
__host__ __device__ __forceinline__ RawRangeElem raw_range_elem(uint32_t t, uint32_t next, bool has_next, uint32_t t_lo, uint32_t t_hi, uint32_t date) {
    RawRangeElem e;
    e.below_lo = t < t_lo;
    e.below_hi = t_hi == 0xFFFFFFFFu || t < t_hi;
    e.descends = has_next && t > next;
    e.off_date = t / 86400u != date;
    e.selected = !e.below_lo && e.below_hi;
    return e;
}

// ---- the kernel's geometry ------------------------------------------------------------------------------------------------
// Thread-group g of a part owns elements [4 g, 4 g + 4): column bytes [16 g, 16 g + 16), wherever they lie.  Their source
// starts at the byte phase sh = (col + 16 g) & 15 = col & 15, the same for every group of the column; the group loads the aligned
// word it starts in and, where sh != 0, the next one (raw_unpack_kernel's loads).  A group goes byte by byte where it is not
// whole (the column's last, with fewer than 4 elements) or where an aligned word would leave the part's span.
constexpr uint32_t RAW_RANGE_BLOCK = 256;
constexpr uint32_t RAW_RANGE_ITERS = 4;                                       // groups per thread
constexpr uint32_t RAW_RANGE_TILE = RAW_RANGE_BLOCK * RAW_RANGE_ITERS * 4;    // elements per workgroup: 4096 (16 KiB of the column)
__host__ __device__ __forceinline__ uint64_t raw_range_tiles(uint64_t rows) { return (rows + RAW_RANGE_TILE - 1) / RAW_RANGE_TILE; }
// the group of thread tid in trip k of tile `tile`: consecutive lanes, consecutive groups
__host__ __device__ __forceinline__ uint64_t raw_range_group(uint64_t tile, uint32_t k, uint32_t tid) {
    return tile * (RAW_RANGE_BLOCK * RAW_RANGE_ITERS) + (uint64_t)k * RAW_RANGE_BLOCK + tid;
}
struct RawRangeLoad {
    bool wide;        // aligned 16-byte loads: `words` of them from address `al` on
    uint64_t al;      // (absolute address)
    uint32_t words, sh;
};
// col: the address of the column's first value; [lo, hi): the part's span
__host__ __device__ __forceinline__ RawRangeLoad raw_range_load(uint64_t col, uint64_t g, uint64_t rows, uint64_t lo, uint64_t hi) {
    const uint64_t s = col + 16 * g;
    RawRangeLoad l;
    l.sh = (uint32_t)(s & 15);
    l.al = s - l.sh;
    l.words = l.sh ? 2u : 1u;
    l.wide = 4 * g + 4 <= rows && l.al >= lo && l.al + 16 * l.words <= hi;
    return l;
}

}  // namespace fa
