// launch_plan.h - what the host decides for ONE ingest or decode launch, as a value, and the functions of plain values behind
// those decisions, the launch guard's verdict among them (no fa_ctx, no HIP call: tests/host_launch_plan.hip and
// tests/host_ingest_feedback.hip run them on the host).
#pragma once
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <utility>

#include "ingest_feedback.h"
#include "sinks.cuh"

namespace fa {

// The instantiation a key-set mask runs - THE statement of that mapping: kernels are compiled for the masks 1..7 and 9,
// every other mask runs the KS_ALL variant (runtime mask).  A new specialised mask is added here and in with_variant.
constexpr uint32_t ks_variant(uint32_t key_sets) { return (key_sets >= 1u && key_sets <= 7u) || key_sets == 9u ? key_sets : KS_ALL; }
// ... as a compile-time constant: f(std::integral_constant<uint32_t, KS>{}) for a value ks_variant returns
template <class F>
decltype(auto) with_variant(uint32_t variant, F&& f) {
    switch (variant) {
    case 1u: return f(std::integral_constant<uint32_t, 1u>{});
    case 2u: return f(std::integral_constant<uint32_t, 2u>{});
    case 3u: return f(std::integral_constant<uint32_t, 3u>{});
    case 4u: return f(std::integral_constant<uint32_t, 4u>{});
    case 5u: return f(std::integral_constant<uint32_t, 5u>{});
    case 6u: return f(std::integral_constant<uint32_t, 6u>{});
    case 7u: return f(std::integral_constant<uint32_t, 7u>{});
    case 9u: return f(std::integral_constant<uint32_t, 9u>{});
    default: return f(std::integral_constant<uint32_t, KS_ALL>{});
    }
}

// Records per workgroup tile (tile_kernel): as many as fit one tile buffer at the batch's mean record size (one record per
// lane, at most BLOCK).  Tiles that still overflow (outliers) take the multi-pass path inside the kernel.
inline uint32_t tile_recs_for(size_t bytes, size_t n) {
    if (n == 0) return BLOCK;
    const double r = ((double)TILE_BYTES - 15.0) / ((double)bytes / (double)n + 0.5);
    return r >= (double)BLOCK ? (uint32_t)BLOCK : r < 1.0 ? 1u : (uint32_t)r;
}
// Records per wave tile (wtile_kernel<variant>): 64 (one per lane) whenever the mean record allows, otherwise as many as
// fit the buffer with about two sigma of byte headroom (sigma of a tile ~ 12 B x sqrt(records): a mix of 60- and 84-byte
// records).  A tile whose bytes still exceed the buffer is not lost to the slow path: the wave takes its rest as one more
// part (ingest.cuh) - about 1 tile in 80 on BASELINE config 2, where this fills all 64 lanes instead of 61.
inline uint32_t wtile_recs_for(size_t bytes, size_t n, uint32_t variant) {
    const double avg = (double)bytes / (double)n, cap = (double)wt_stride(variant) - 16.0 - 15.0;
    const double r = (cap - 2.0 * 12.0 * std::sqrt(std::min(cap / avg, (double)WT_RECS))) / avg;
    return r >= (double)WT_RECS ? (uint32_t)WT_RECS : r < 1.0 ? 1u : (uint32_t)r;
}
// Workgroups of a wave-tile launch: <= 64 records per wave, WBLOCK / 64 waves per workgroup, WT_WG_PER_CU workgroups per CU
// (the variants that serve a sketch run one 16-wave workgroup per CU instead of two 12-wave ones: ingest.cuh, wtile_block)
inline int wtile_grid(uint32_t n, uint32_t tile_recs, uint32_t variant, uint32_t num_cus) {
    const uint32_t waves = (uint32_t)(wt_lean(variant) ? WBLOCK : WBLOCK_CMS) / 64u;
    const uint32_t wgs = ((n + tile_recs - 1) / tile_recs + waves - 1) / waves;
    return (int)std::max(1u, std::min(wgs, num_cus * (wt_lean(variant) ? (uint32_t)WT_WG_PER_CU : 1u)));
}

// The decisions of one launch.  ingest_device_records builds one per launch and hands it to everything that prepares, queues
// and follows that launch; nothing of it is kept in the ctx.  The default is the decode path's: workgroup tiles, variant 1.
struct LaunchPlan {
    uint32_t variant = 1u;       // the instantiation (ks_variant of the ctx's mask)
    uint32_t tile_recs = BLOCK;  // records per tile
    int grid = 1;                // workgroups of the tile kernel = segments per partition of every scatter sink
    // the scatter sink, whose kernel is the wave-tile kernel (15-20 % faster than the 256-thread workgroup-tile kernel when most
    // records leave as tuples); the workgroup-tile kernel serves the decode path, the direct sink (small batches) and key
    // sets without the flows_5m rollup.  Everything below needs it.
    bool wave_tiles = false;
    bool t8 = false;             // compact 8-byte tuples (table.cuh)
    bool seq_variant = false;    // the kernel that learns a field order per wave (ingest.cuh tier 4)
    bool cms_segments = false;   // sketch updates leave as tuples (cseg), folded by cms_agg_kernel
    bool wide_segments = false;  // (SrcAddr,DstPort,Proto) updates leave as tuples (wseg) ...
    bool wlog = false;           // ... which stay where they are as a log chunk (wlog_record) instead of being folded
    bool side = false;           // candidates mode: the flows_5m aggregation runs on the side stream
};

// The plan is decided in three stages (ingest_device_records calls them in this order), each a function of plain values and
// of the feedback (ingest_feedback.h: what the earlier launches taught the ctx).
// Before the launch guard: the sink and the tuple format of a launch of n records, planned at batch count `batches`.
inline void plan_sink(LaunchPlan& p, uint32_t key_sets, int sink_mode, size_t n, uint32_t plog2, const IngestFeedback& fb, uint64_t batches) {
    p.variant = ks_variant(key_sets);
    // small batches are not worth a second pass: they go straight to the device-wide table (sink_mode, env FA_SINK: 0 auto, 1 direct, 2 scatter)
    p.wave_tiles = (key_sets & FA_KEYS_AS_PAIR) && (sink_mode == 2 || (sink_mode == 0 && n >= (1u << 15)));
    // tuple format of this launch (table.cuh): compact 8-byte tuples on the wave-tile kernel with 256 partitions,
    // unless recent launches showed that this stream's records do not fit them
    p.t8 = p.wave_tiles && plog2 == 8 && fb.compact_tuples(batches);
}
// With p.grid known: which of the other sinks' updates leave as tuples too.
inline void plan_segments(LaunchPlan& p, uint32_t key_sets, bool cms_atomic, bool cms_scatter_ok, bool wide_table, const IngestFeedback& fb) {
    p.cms_segments = p.wave_tiles && (key_sets & (FA_KEYS_SRCADDR_CMS | FA_KEYS_DSTADDR_CMS)) && !cms_atomic && cms_scatter_ok;
    p.wide_segments = p.wave_tiles && wide_table && (key_sets & FA_KEYS_ADDR_PORT_PROTO) && p.grid <= WAGG_MAX_NWG && fb.wide_scatter_sink();
}
// Behind the preparations (a settle inside them may have moved the feedback: this is what it says NOW).
inline void plan_followers(LaunchPlan& p, uint32_t key_sets, bool candidates, const IngestFeedback& fb, uint64_t batches) {
    p.wlog = p.wide_segments && fb.log_mode();
    // most records of the last launches needed the order-free parser: the kernel that learns a field order per wave
    p.seq_variant = p.wave_tiles && key_sets == FA_KEYS_AS_PAIR && fb.learnt_order(batches);
    p.side = p.cms_segments && candidates;
}

// ---- the launch guard: never lose aggregates ----
// What the newest counter snapshot says about a launch of n more records: a table above 50 % load or parked updates are
// settled (grow + replay) right away; a launch is only queued while the updates that everything in flight could park still
// fit the spill buffers - otherwise the host first waits for the newest snapshot (pre_launch_guard, maintain_host.inc).
enum GuardVerdict { GUARD_GO = 0, GUARD_WAIT = 1, GUARD_SETTLE = 2 };
struct GuardSnapshot {  // of the newest Counters the host has seen
    uint32_t spill_count, wspill_count;
    uint64_t used, wused;
};
struct GuardHost {
    uint64_t used_base, wused_base;    // groups created before the current counter epoch
    uint64_t slots, wslots;            // the two tables' sizes
    uint32_t spill_cap, wspill_cap;
    bool wide_table;
    uint32_t wide_per_record;          // wide-table updates one record can cause
    uint64_t in_flight;                // records launched behind the snapshot
};
inline GuardVerdict guard_verdict(const GuardSnapshot& h, const GuardHost& c, size_t n) {
    if (h.spill_count || h.wspill_count || (c.used_base + h.used) * 2 > c.slots || (c.wide_table && (c.wused_base + h.wused) * 2 > c.wslots)) return GUARD_SETTLE;
    const uint64_t pot = c.in_flight + n;  // records whose updates the host has not seen settle
    if (pot + (1u << 20) > c.spill_cap || (c.wide_table && pot * c.wide_per_record + (1u << 20) > c.wspill_cap)) return GUARD_WAIT;
    return GUARD_GO;
}

}  // namespace fa
