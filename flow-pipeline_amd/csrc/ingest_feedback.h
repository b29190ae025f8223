// ingest_feedback.h - the adaptive feedback of the ingest path as ONE value: the knobs it was created with, what it has learnt
// from the device counters launch after launch, and every question the host asks of it, answered by name (no fa_ctx, no HIP
// call: tests/host_ingest_feedback.hip runs it on the host).  Only speed depends on any of this, never results.
#pragma once
#include <algorithm>
#include <cstdint>

#include "sinks.cuh"

namespace fa {

// What fa_create read from the environment and the configuration; never written afterwards.
struct FeedbackKnobs {
    int wide_mode = 0;  // env FA_WIDE: 0 adaptive, 1 "atomic" (every update through memory-side atomics), 2 "scatter" (always the scatter sink),
                        // 3 "log": scatter, and the launch's tuples stay in their segments (fa_ctx::wlog) instead of being folded at once
    int t8_mode = 0;    // env FA_TUPLE: 0 adaptive, 1 always compact ("8"), 2 always wide ("16")
    int seq_mode = 0;   // env FA_SEQ: 0 by the counters, 1 always, 2 never
    uint32_t agg_passes_forced = 0;    // env FA_AGG_PASSES (tests, A/B): 1, 2, 4, 8; 0 = by the counters
    uint32_t plog2 = PART_LOG2_MAX;    // env FA_PLOG2: key partitions of the scatter sink
    bool wide_table = false;           // the ctx has a wide table (a wide key set is enabled)
    bool log_allowed = true;           // the wide log may hold chunks (FA_WIDE_LOG_CHUNKS > 0)
};

// The counter values a look reads (Counters, sinks.cuh): at least as new as the last look's.
struct FeedbackLook {
    uint64_t ok, misfit8, retried, wused, wfold_n, agg_launches, agg_groups;
};

struct IngestFeedback {
    FeedbackKnobs knobs;
    // ---- (SrcAddr,DstPort,Proto): atomics, scatter sink or log ----
    bool wide_probed = false;   // the ctx has seen its first launch (a first big launch is probed with its first 2^20 records)
    bool wide_defer = false;    // adaptive: log mode from the moment more than half of a million records opened new rows, until fewer
                                // than half of a million FOLDED tuples do (deferred launches themselves tell nothing about new rows)
    bool wide_scatter = true;   // adaptive: the scatter sink while a good share of the records open new rows (7 atomics each
                                // on the atomic path); a stream that mostly hits existing rows (one atomic line transaction
                                // each) is cheaper without the detour through the segments
    uint64_t seen_wused = 0, seen_ok_w = 0;  // Counters::wused / ok at the last verdict on the wide key set
    uint64_t seen_wfold = 0;                 // Counters::wfold_n at the last verdict in log mode
    // ---- tuple format: compact tuples while (almost) every record fits them.  A look whose misfits (records that only a wide
    // tuple holds - they took the direct path) exceed 1/16 of its records switches to wide tuples for the next 64 launches, then
    // compact is tried again ----
    uint64_t t8_wide_until = 0;              // batch count up to which wide tuples are used
    uint64_t seen_misfit8 = 0, seen_ok = 0;  // counter values at the last look
    // ---- the learnt-field-order kernel: launches before batch seq_until run it ----
    uint64_t seen_retried = 0, seq_until = 0;
    // ---- agg8_kernel's passes (1, 2, 4, 8): groups per launch / (partitions x passes) <= half the LDS table ----
    uint64_t seen_agg_groups = 0, seen_agg_launches = 0;
    uint32_t agg_passes = 1;

    // The one mutator: h = counters at least as new as the last look's, batches = launches the ctx has made so far.
    void look(const FeedbackLook& h, uint64_t batches) {
        const uint64_t d_mis = h.misfit8 - seen_misfit8, d_ok = h.ok - seen_ok;
        if (d_ok && d_mis * 16 > d_ok) t8_wide_until = batches + 64;
        // records that went through the second-chance parsers: most of them -> the kernel variant that learns the producer's field order
        if (h.retried < seen_retried) seen_retried = h.retried;
        if (d_ok && (h.retried - seen_retried) * 2 > d_ok) seq_until = batches + 64;
        seen_retried = h.retried;
        seen_misfit8 = h.misfit8;
        seen_ok = h.ok;
        if (knobs.wide_table && !wide_defer) {  // (SrcAddr,DstPort,Proto): scatter sink or atomics, by the share of records that opened a row lately
            if (h.wused < seen_wused) seen_wused = h.wused;  // (table rebuilt: the count starts over)
            if (h.ok < seen_ok_w) seen_ok_w = h.ok;
            const uint64_t dw = h.wused - seen_wused, dn = h.ok - seen_ok_w;
            if (dn >= (1u << 20)) {
                if (dw * 5 > dn) wide_scatter = true;
                else if (dw * 10 < dn) wide_scatter = false;
                // ... and no table at all for a stream that opens a row for most of its records: the log (fa_ctx::wlog)
                if (knobs.wide_mode == 0 && wide_scatter && dw * 2 > dn && knobs.log_allowed) {
                    wide_defer = true;
                    seen_wfold = h.wfold_n;
                }
                seen_wused = h.wused;
                seen_ok_w = h.ok;
            }
        }
        if (knobs.wide_table && wide_defer && knobs.wide_mode == 0) {  // log mode chosen by the library: do the chunks that ARE folded still open rows?
            const uint64_t dn = h.wfold_n - seen_wfold;
            if (h.wused < seen_wused || h.wfold_n < seen_wfold) {  // (table rebuilt / counters restarted: no verdict from this look)
                seen_wused = h.wused;
                seen_wfold = h.wfold_n;
            } else if (dn >= (1u << 20)) {
                // fewer than half of the folded tuples opened a row: this stream aggregates - back to the table (scatter sink or
                // atomics, by the feedback above); the chunks still pending are folded one per launch (ingest_device_records)
                if ((h.wused - seen_wused) * 2 < dn) {
                    wide_defer = false;
                    seen_ok_w = h.ok;
                }
                seen_wused = h.wused;
                seen_wfold = h.wfold_n;
            }
        }
        // passes of agg8_kernel: the groups a launch adds to the device table, per partition and pass, against the LDS table
        if (h.agg_launches < seen_agg_launches || h.agg_groups < seen_agg_groups) seen_agg_launches = seen_agg_groups = 0;
        const uint64_t d_l = h.agg_launches - seen_agg_launches, d_g = h.agg_groups - seen_agg_groups;
        if (d_l) {
            const uint64_t per_part = d_g / d_l >> knobs.plog2;
            uint32_t want = 1;
            while (want < 8 && per_part > (uint64_t)(AGG8_SLOTS / 2) * want) want *= 2;
            // (a launch that overflowed its table under-counts: move up one step at a time, down only when clearly below)
            if (want > agg_passes) agg_passes = std::min(want, agg_passes * 2);
            else if (want < agg_passes && per_part * 3 < (uint64_t)(AGG8_SLOTS / 2) * agg_passes) agg_passes = std::max(want, agg_passes / 2);
            seen_agg_launches = h.agg_launches;
            seen_agg_groups = h.agg_groups;
        }
    }

    // ---- what the host asks (b = the ctx's batch count when the launch is planned) ----
    bool compact_tuples(uint64_t b) const { return knobs.t8_mode != 2 && (knobs.t8_mode == 1 || b >= t8_wide_until); }
    bool learnt_order(uint64_t b) const { return knobs.seq_mode != 2 && (knobs.seq_mode == 1 || b < seq_until); }
    // the wide key set's updates leave as tuples (the scatter sink) instead of through atomics
    bool wide_scatter_sink() const { return knobs.wide_mode == 2 || knobs.wide_mode == 3 || (knobs.wide_mode == 0 && wide_scatter); }
    // ... and stay where they are as a log chunk instead of being folded behind the launch
    bool log_mode() const { return knobs.wide_mode == 3 || (knobs.wide_mode == 0 && wide_defer); }
    // the library chose the log and has left it again: chunks that are still pending drain
    bool left_log_mode() const { return knobs.wide_mode == 0 && !wide_defer; }
    // the adaptive ctx has not seen a launch yet: a first big one is probed
    bool wants_probe() const { return knobs.wide_mode == 0 && !wide_defer && !wide_probed; }
    void mark_probed() { wide_probed = true; }  // (the one write that is not a look)
    uint32_t passes() const { return knobs.agg_passes_forced ? knobs.agg_passes_forced : agg_passes; }
};

}  // namespace fa
