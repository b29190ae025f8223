// segwalk.cuh - the tuple segments of the scatter sinks, read back: their geometry, and the walk over them that
// agg_kernel, agg8_kernel and cms_agg_kernel (agg.cuh) share.
//
// A partition's tuples lie in one SEGMENT per ingest workgroup (nwg of them, capq tuples each, 16-byte PIECES of TPL
// tuples: 1 wide or sketch tuple, 2 compact ones).  A segment has two parts, each with its own count: the FRONT part,
// tuples [0, c) (whole store units), and the BACK part (single tuples and bin leftovers, a handful), the c tuples that END
// at the segment's last slot: [capq - c, capq).  A wave reads a part LEVEL by level, one piece per lane:
//   front: level j = pieces [64j, 64j + 64) of ONE segment per 64-lane load;
//   back:  level j = pieces [first / TPL + 8j, first / TPL + 8j + 8) of EIGHT segments per load (segment = lane / 8).
// With TPL = 2 an odd `first` makes the part's first piece straddle its start: the piece is read, its first tuple is not
// valid.  THE RULE (tests/host_segwalk.hip checks it for every count): every tuple of a part is visited exactly once, by
// exactly one lane, at exactly one level below seg_levels_of(c); nothing outside the part is valid at any level.
//
// The walk goes over WORK ITEMS (group, level): a group = the SU consecutive loads of a batch (SU segments in front,
// 8 SU at the back), and a group's levels are those of its longest part (flv / blv), so that a wave never walks the
// empty levels of short segments up to the partition's longest one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fa {

constexpr int SEG_MAX_NWG = 1536;  // segments per partition: one per wave-tile workgroup (<= 2 per CU)
// loads per lane and batch (16-byte loads in flight per lane, x2 buffers) of the three kernels: build knobs
#ifndef FA_AGG_SU
#define FA_AGG_SU 4
#endif
#ifndef FA_AGG8_SU
#define FA_AGG8_SU 2
#endif
#ifndef FA_CMS_SU
#define FA_CMS_SU 4
#endif
constexpr int AGG_SU = FA_AGG_SU, AGG8_SU = FA_AGG8_SU, CMS_SU = FA_CMS_SU;
// zero counts behind the last segment: the last group of a back pass reads up to 8 SU segments from a segment below nwg on
constexpr int SEG_PAD = 8 * (AGG_SU > AGG8_SU ? (AGG_SU > CMS_SU ? AGG_SU : CMS_SU) : (AGG8_SU > CMS_SU ? AGG8_SU : CMS_SU));
constexpr int SEG_COUNTS = SEG_MAX_NWG + SEG_PAD;  // words of a staged count array (pc / pcb)

// ---- geometry: plain functions of plain values ------------------------------------------------------------------------
template <bool BACK>
__host__ __device__ constexpr uint32_t seg_per_load() { return BACK ? 8u : 1u; }  // segments a 64-lane load covers
template <bool BACK>
__host__ __device__ constexpr uint32_t seg_lanes() { return 64u / seg_per_load<BACK>(); }  // lanes = pieces per segment and level
// which of a load's segments a lane reads
template <bool BACK>
__host__ __device__ constexpr uint32_t seg_of_lane(uint32_t lane) { return BACK ? lane / seg_lanes<BACK>() : 0u; }
// levels a part of c tuples needs (back, TPL = 2: c tuples span up to c / 2 + 1 pieces)
template <bool BACK, int TPL>
__host__ __device__ constexpr uint32_t seg_levels_of(uint32_t c) {
    return BACK ? (c ? (c / TPL + (TPL > 1 ? 1u : 0u) + 7u) >> 3 : 0u) : (c + 64u * TPL - 1u) / (64u * TPL);
}
// groups of a staged count array
template <bool BACK, int SU>
__host__ __device__ constexpr uint32_t seg_groups() { return (uint32_t)SEG_COUNTS / ((uint32_t)SU * seg_per_load<BACK>()); }

struct SegPiece {
    uint32_t piece;  // index of the 16-byte piece inside the segment; 0 when no tuple of it is valid
    uint32_t valid;  // bit t: tuple piece * TPL + t belongs to the part
};
// the piece `lane` reads at level j of a part of c tuples - the only place that computes one
template <bool BACK, int TPL>
__host__ __device__ __forceinline__ SegPiece seg_piece(uint32_t capq, uint32_t c, uint32_t j, uint32_t lane) {
    constexpr uint32_t PER = seg_lanes<BACK>();
    const uint32_t first = BACK ? capq - c : 0u;  // first tuple of the part
    const uint32_t piece = first / TPL + PER * j + (BACK ? lane % PER : lane);
    static_assert(TPL == 1 || TPL == 2, "one or two tuples per 16-byte piece");
    const uint32_t q = piece * TPL;  // the piece's first tuple
    // (spelled out, not a loop over the TPL tuples: agg8_kernel sits at the SGPR limit, and the loop form made the compiler
    // spill a dozen SGPRs into a VGPR's lanes there; the same goes for the clamp of the level lookup in seg_walk)
    uint32_t valid = (q >= first && q < first + c) ? 1u : 0u;
    if (TPL > 1) valid |= (q + 1u >= first && q + 1u < first + c) ? 2u : 0u;
    return SegPiece{valid ? piece : 0u, valid};
}

// ---- the fetch ----------------------------------------------------------------------------------------------------------
// 16-byte loads a lane has in flight per batch
template <int SU>
struct SegBatch {
    uint4 t[SU];
    uint32_t v;  // bit TPL * s + t: tuple t of t[s] is a tuple of this lane (not a dummy load, not outside the part)
};

// Issue the loads of lanes [0, 64) for the work item (segments from w0 on, level j).  The counts come from LDS (pc, zero
// padded): a count read from global memory would put a full vmcnt drain between consecutive tuple loads.  Two loops - all
// indices first, then all loads - and the loads are UNCONDITIONAL (a lane without a tuple re-reads piece 0 of a valid
// segment; a segment past the end is clamped to the last one and has a zero count): with predicated loads the compiler
// cannot count what is in flight and drains everything (vmcnt(0)) before the previous batch is consumed.
template <bool BACK, int SU, int TPL>
__device__ __forceinline__ void seg_fetch(uint32_t capq, uint32_t nwg, const uint4* pbase, const uint32_t* pc, uint32_t w0, uint32_t lane, uint32_t j,
                                          SegBatch<SU>& b) {
    uint32_t idx[SU], seg[SU];
    b.v = 0;
#pragma unroll
    for (int s = 0; s < SU; s++) {
        seg[s] = w0 + (uint32_t)s * seg_per_load<BACK>() + seg_of_lane<BACK>(lane);
        const uint32_t c = pc[min(seg[s], (uint32_t)(SEG_COUNTS - 1))];  // 0 past nwg
        const SegPiece p = seg_piece<BACK, TPL>(capq, c, j, lane);
        b.v |= p.valid << (TPL * s);
        idx[s] = p.piece;
    }
#pragma unroll
    for (int s = 0; s < SU; s++) b.t[s] = pbase[(size_t)min(seg[s], nwg - 1u) * (capq / TPL) + idx[s]];
}

// ---- counts and levels (workgroup functions: every one of the NT threads calls them) -------------------------------------
// pc[] / pcb[] = the front / back counts of one partition's nwg segments, zero padded; ends with a barrier.  TOTAL: returns
// the partition's tuples (front + back) to every thread.
template <int NT, bool TOTAL>
__device__ __forceinline__ uint32_t seg_counts_stage(const uint32_t* front, const uint32_t* back, uint32_t nwg, uint32_t* pc, uint32_t* pcb) {
    uint32_t sum = 0;
    for (uint32_t i = threadIdx.x; i < (uint32_t)SEG_COUNTS; i += NT) {
        const uint32_t c = i < nwg ? front[i] : 0u, cb = i < nwg ? back[i] : 0u;
        pc[i] = c;
        pcb[i] = cb;
        sum += c + cb;
    }
    if constexpr (!TOTAL) {
        __syncthreads();
        return 0u;
    } else {
        __shared__ uint32_t total_s;
        if (threadIdx.x == 0) total_s = 0;
        __syncthreads();
        for (int o = 32; o > 0; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&total_s, sum);
        __syncthreads();
        return total_s;
    }
}
// flv[g] / blv[g] = levels the front / back group g needs, from staged counts (the caller puts a barrier behind it)
template <int NT, int SU, int TPL>
__device__ __forceinline__ void seg_levels(const uint32_t* pc, const uint32_t* pcb, uint16_t* flv, uint16_t* blv) {
    constexpr uint32_t FG = SU, BG = SU * 8;  // segments per group
    for (uint32_t g = threadIdx.x; g < seg_groups<false, SU>(); g += NT) {
        uint32_t m = 0;
        for (uint32_t s = 0; s < FG; s++) m = max(m, pc[g * FG + s]);
        flv[g] = (uint16_t)seg_levels_of<false, TPL>(m);
    }
    for (uint32_t g = threadIdx.x; g < seg_groups<true, SU>(); g += NT) {
        uint32_t m = 0;
        for (uint32_t s = 0; s < BG; s++) m = max(m, pcb[g * BG + s]);
        blv[g] = (uint16_t)seg_levels_of<true, TPL>(m);
    }
}

// ---- the walk -----------------------------------------------------------------------------------------------------------
// One wave's work items of one pass (front: pc = the front counts, lv = flv; back: pcb, blv): groups first_group,
// first_group + group_stride, ..., each at its levels.  Software pipeline over two register buffers: the loads of the next
// item fly while consume(batch) works on the current one; an item past the end reads clamped addresses with zero counts.
template <bool BACK, int SU, int TPL, class F>
__device__ __forceinline__ void seg_walk(uint32_t capq, uint32_t nwg, const uint4* pbase, const uint32_t* pc, const uint16_t* lv, uint32_t lane,
                                         uint32_t first_group, uint32_t group_stride, F&& consume) {
    constexpr uint32_t GSEGS = (uint32_t)SU * seg_per_load<BACK>();
    const uint32_t ngroups = (nwg + GSEGS - 1u) / GSEGS;
    uint32_t g = first_group, j = 0;
    auto settle_item = [&]() {  // (g, j) = the next item that exists, or g >= ngroups
        // (the lookup is clamped like every address of an item past the end, although g < ngroups already bounds it)
        while (g < ngroups && j >= (uint32_t)__builtin_amdgcn_readfirstlane((int)lv[min(g, seg_groups<BACK, SU>() - 1u)])) {
            g += group_stride;
            j = 0;
        }
    };
    settle_item();
    SegBatch<SU> b0, b1;
    seg_fetch<BACK, SU, TPL>(capq, nwg, pbase, pc, g * GSEGS, lane, j, b0);
    while (g < ngroups) {
        j++;
        settle_item();
        seg_fetch<BACK, SU, TPL>(capq, nwg, pbase, pc, g * GSEGS, lane, j, b1);
        consume(b0);
        if (g >= ngroups) break;
        j++;
        settle_item();
        seg_fetch<BACK, SU, TPL>(capq, nwg, pbase, pc, g * GSEGS, lane, j, b0);
        consume(b1);
    }
}

}  // namespace fa
