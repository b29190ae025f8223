// host_ingest_feedback.hip - the ingest path's adaptive feedback (csrc/ingest_feedback.h) and the plain-value functions behind a
// launch's plan and the launch guard (csrc/launch_plan.h), run on the host.
// TEST INFRASTRUCTURE (tests/test_ingest_feedback_cpu.py).  No GPU call.  Modes (argv[1]):
//   diff    the differential check: IngestFeedback against the rules as they stood BEFORE they became a value - format_feedback
//           and the conditions that were written inline, transcribed below over a plain struct of the old fa_ctx members - driven
//           with the same generated sequences of looks.  Prints "diff combos C looks L mismatches M" (and the first mismatches).
//   looks   stdin: "knobs wide_mode t8_mode seq_mode forced plog2 wide_table log_allowed" starts a fresh value,
//           "look ok misfit8 retried wused wfold_n agg_launches agg_groups batches" is one look, "probed" marks the probe;
//           every line is answered with the whole state and every named answer (at that batch count).
//   plan    stdin: "key_sets sink_mode n plog2 grid cms_atomic cms_scatter_ok wide_table candidates wide_mode t8_mode seq_mode
//           batches t8_wide_until seq_until wide_scatter wide_defer" -> the plan's nine decisions
//   guard   stdin: "spill_count wspill_count used wused used_base wused_base slots wslots spill_cap wspill_cap wide_table
//           wide_per_record in_flight n" -> "verdict guard V": 0 go, 1 wait for the newest snapshot, 2 settle
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../flow-pipeline_amd/csrc/launch_plan.h"

using namespace fa;

// ---- the rules before the refactor, verbatim -------------------------------------------------------------------------------
struct OldCtx {  // the eighteen members of fa_ctx, and what else the old text reads
    bool wtab = false;
    int wide_mode = 0;
    bool wide_probed = false;
    bool wide_defer = false;
    uint64_t seen_wfold = 0;
    size_t wlog_max = 8;
    bool wide_scatter = true;
    uint64_t seen_wused = 0, seen_ok_w = 0;
    int t8_mode = 0;
    uint64_t t8_wide_until = 0;
    uint64_t seen_misfit8 = 0, seen_ok = 0;
    uint64_t seen_retried = 0, seq_until = 0;
    int seq_mode = 0;
    uint64_t seen_agg_groups = 0, seen_agg_launches = 0;
    uint32_t agg_passes_forced = 0;
    uint32_t agg_passes = 1;
    uint32_t plog2 = PART_LOG2_MAX;
    struct {
        uint64_t batches = 0;
    } stats;
};
static void format_feedback(OldCtx* c, const Counters& h) {
    const uint64_t d_mis = h.misfit8 - c->seen_misfit8, d_ok = h.ok - c->seen_ok;
    if (d_ok && d_mis * 16 > d_ok) c->t8_wide_until = c->stats.batches + 64;
    // records that went through the second-chance parsers: most of them -> the kernel variant that learns the producer's field order
    if (h.retried < c->seen_retried) c->seen_retried = h.retried;
    if (d_ok && (h.retried - c->seen_retried) * 2 > d_ok) c->seq_until = c->stats.batches + 64;
    c->seen_retried = h.retried;
    c->seen_misfit8 = h.misfit8;
    c->seen_ok = h.ok;
    if (c->wtab && !c->wide_defer) {  // (SrcAddr,DstPort,Proto): scatter sink or atomics, by the share of records that opened a row lately
        if (h.wused < c->seen_wused) c->seen_wused = h.wused;  // (table rebuilt: the count starts over)
        if (h.ok < c->seen_ok_w) c->seen_ok_w = h.ok;
        const uint64_t dw = h.wused - c->seen_wused, dn = h.ok - c->seen_ok_w;
        if (dn >= (1u << 20)) {
            if (dw * 5 > dn) c->wide_scatter = true;
            else if (dw * 10 < dn) c->wide_scatter = false;
            // ... and no table at all for a stream that opens a row for most of its records: the log (fa_ctx::wlog)
            if (c->wide_mode == 0 && c->wide_scatter && dw * 2 > dn && c->wlog_max > 0) {
                c->wide_defer = true;
                c->seen_wfold = h.wfold_n;
            }
            c->seen_wused = h.wused;
            c->seen_ok_w = h.ok;
        }
    }
    if (c->wtab && c->wide_defer && c->wide_mode == 0) {  // log mode chosen by the library: do the chunks that ARE folded still open rows?
        const uint64_t dn = h.wfold_n - c->seen_wfold;
        if (h.wused < c->seen_wused || h.wfold_n < c->seen_wfold) {  // (table rebuilt / counters restarted: no verdict from this look)
            c->seen_wused = h.wused;
            c->seen_wfold = h.wfold_n;
        } else if (dn >= (1u << 20)) {
            // fewer than half of the folded tuples opened a row: this stream aggregates - back to the table (scatter sink or
            // atomics, by the feedback above); the chunks still pending are folded one per launch (fa_ingest_device)
            if ((h.wused - c->seen_wused) * 2 < dn) {
                c->wide_defer = false;
                c->seen_ok_w = h.ok;
            }
            c->seen_wused = h.wused;
            c->seen_wfold = h.wfold_n;
        }
    }
    // passes of agg8_kernel: the groups a launch adds to the device table, per partition and pass, against the LDS table
    if (h.agg_launches < c->seen_agg_launches || h.agg_groups < c->seen_agg_groups) c->seen_agg_launches = c->seen_agg_groups = 0;
    const uint64_t d_l = h.agg_launches - c->seen_agg_launches, d_g = h.agg_groups - c->seen_agg_groups;
    if (d_l) {
        const uint64_t per_part = d_g / d_l >> c->plog2;
        uint32_t want = 1;
        while (want < 8 && per_part > (uint64_t)(AGG8_SLOTS / 2) * want) want *= 2;
        // (a launch that overflowed its table under-counts: move up one step at a time, down only when clearly below)
        if (want > c->agg_passes) c->agg_passes = std::min(want, c->agg_passes * 2);
        else if (want < c->agg_passes && per_part * 3 < (uint64_t)(AGG8_SLOTS / 2) * c->agg_passes) c->agg_passes = std::max(want, c->agg_passes / 2);
        c->seen_agg_launches = h.agg_launches;
        c->seen_agg_groups = h.agg_groups;
    }
}
// ... and the conditions that stood inline (ingest_device_records, make_args, fa_stats), each as it was written
static bool old_t8(const OldCtx* c) { return c->t8_mode != 2 && (c->t8_mode == 1 || c->stats.batches >= c->t8_wide_until); }
static bool old_seq(const OldCtx* c) { return c->seq_mode != 2 && (c->seq_mode == 1 || c->stats.batches < c->seq_until); }
static bool old_scatter(const OldCtx* c) { return (c->wide_mode == 2 || c->wide_mode == 3 || (c->wide_mode == 0 && c->wide_scatter)); }
static bool old_log(const OldCtx* c) { return (c->wide_mode == 3 || (c->wide_mode == 0 && c->wide_defer)); }
static bool old_left(const OldCtx* c) { return c->wide_mode == 0 && !c->wide_defer; }
static bool old_probe(const OldCtx* c) { return c->wide_mode == 0 && !c->wide_defer && !c->wide_probed; }
static uint32_t old_passes(const OldCtx* c) { return c->agg_passes_forced ? c->agg_passes_forced : c->agg_passes; }

// ---- the differential check ------------------------------------------------------------------------------------------------
struct Rng {
    uint64_t s;
    uint64_t next() {  // splitmix64
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t n) { return n ? next() % n : 0; }
};
// a step on either side of `at`: at - 1, at, at + 1 (most of the time), or anything up to twice that
static uint64_t around(Rng& r, uint64_t at) {
    switch (r.below(5)) {
    case 0: return at ? at - 1 : 0;
    case 1: return at;
    case 2: return at + 1;
    case 3: return r.below(2 * at + 2);
    default: return r.below(at / 8 + 2);
    }
}
static bool same_state(const OldCtx& o, const IngestFeedback& f) {
    return o.wide_probed == f.wide_probed && o.wide_defer == f.wide_defer && o.wide_scatter == f.wide_scatter && o.seen_wfold == f.seen_wfold &&
           o.seen_wused == f.seen_wused && o.seen_ok_w == f.seen_ok_w && o.t8_wide_until == f.t8_wide_until && o.seen_misfit8 == f.seen_misfit8 &&
           o.seen_ok == f.seen_ok && o.seen_retried == f.seen_retried && o.seq_until == f.seq_until && o.seen_agg_groups == f.seen_agg_groups &&
           o.seen_agg_launches == f.seen_agg_launches && o.agg_passes == f.agg_passes && o.wide_mode == f.knobs.wide_mode &&
           o.t8_mode == f.knobs.t8_mode && o.seq_mode == f.knobs.seq_mode && o.agg_passes_forced == f.knobs.agg_passes_forced;
}
static bool same_answers(OldCtx& o, const IngestFeedback& f, uint64_t b) {
    const uint64_t keep = o.stats.batches;
    o.stats.batches = b;
    const bool same = old_t8(&o) == f.compact_tuples(b) && old_seq(&o) == f.learnt_order(b) && old_scatter(&o) == f.wide_scatter_sink() &&
                      old_log(&o) == f.log_mode() && old_left(&o) == f.left_log_mode() && old_probe(&o) == f.wants_probe() && old_passes(&o) == f.passes();
    o.stats.batches = keep;
    return same;
}
static int run_diff() {
    const uint32_t forced[5] = {0, 1, 2, 4, 8};
    unsigned long long combos = 0, looks = 0, mismatches = 0, moved[12] = {};
    for (int wide_mode = 0; wide_mode < 4; wide_mode++)
    for (int t8_mode = 0; t8_mode < 3; t8_mode++)
    for (int seq_mode = 0; seq_mode < 3; seq_mode++)
    for (uint32_t fp : forced)
    for (int wtab = 0; wtab < 2; wtab++)
    for (int log_ok = 0; log_ok < 2; log_ok++) {
        combos++;
        for (uint32_t seed = 0; seed < 3; seed++) {
            Rng r{0xFA5EEDull * (combos * 8 + seed) + 17};
            OldCtx o;
            IngestFeedback f;
            o.wtab = f.knobs.wide_table = wtab != 0;
            o.wide_mode = f.knobs.wide_mode = wide_mode;
            o.t8_mode = f.knobs.t8_mode = t8_mode;
            o.seq_mode = f.knobs.seq_mode = seq_mode;
            o.agg_passes_forced = f.knobs.agg_passes_forced = fp;
            o.wlog_max = log_ok ? 8 : 0;
            f.knobs.log_allowed = log_ok != 0;
            o.plog2 = f.knobs.plog2 = seed == 2 ? 4u : (uint32_t)PART_LOG2_MAX;
            Counters h{};
            for (int i = 0; i < 400; i++) {
                // monotone counters, every step on either side of the threshold the rules compare it with ...
                const uint64_t big = 1u << 20;
                const uint64_t d_ok = r.below(4) == 0 ? r.below(3) : around(r, r.below(3) ? big : big / 4);
                h.ok += d_ok;
                h.misfit8 += around(r, d_ok / 16);
                h.retried += around(r, d_ok / 2);
                const uint64_t dn = h.ok - f.seen_ok_w;  // (what the wide rule will compare dw with: the same value on both sides)
                const uint64_t at[3] = {dn / 5, dn / 10, dn / 2};
                if (!f.wide_defer) {
                    h.wused = std::max<uint64_t>(h.wused, f.seen_wused + around(r, at[r.below(3)]));
                    h.wfold_n += r.below(3) ? 0 : r.below(big);
                } else {
                    const uint64_t d_f = around(r, r.below(3) ? big : big / 3);
                    h.wfold_n += d_f;
                    h.wused = std::max<uint64_t>(h.wused, f.seen_wused + around(r, (h.wfold_n - f.seen_wfold) / 2));
                }
                const uint64_t d_l = r.below(4);
                const uint64_t half = AGG8_SLOTS / 2, steps[6] = {half, 2 * half, 4 * half, half / 3, 2 * half / 3, 4 * half / 3};
                h.agg_launches += d_l;
                h.agg_groups += d_l * (around(r, steps[r.below(6)] * (1 + r.below(2))) << f.knobs.plog2) + r.below(d_l + 1);
                // ... and the restarts: table rebuilt, counters starting over
                if (r.below(23) == 0) h.wused = r.below(h.wused + 1);
                if (r.below(29) == 0) h.retried = r.below(h.retried + 1);
                if (r.below(31) == 0) h.agg_launches = r.below(3), h.agg_groups = r.below(1 << 16);
                if (r.below(37) == 0) h.agg_groups = r.below(h.agg_groups + 1);
                if (r.below(41) == 0) h.wfold_n = r.below(h.wfold_n + 1);
                if (r.below(97) == 0) h.ok = r.below(h.ok + 1), h.misfit8 = r.below(h.misfit8 + 1);
                o.stats.batches += r.below(5) ? r.below(4) : r.below(70);
                if (r.below(50) == 0) o.wide_probed = true, f.mark_probed();
                const IngestFeedback was = f;
                format_feedback(&o, h);
                f.look(FeedbackLook{h.ok, h.misfit8, h.retried, h.wused, h.wfold_n, h.agg_launches, h.agg_groups}, o.stats.batches);
                looks++;
                // (what the sequences reached: every rule fired, in both directions, and every restart was met)
                moved[0] += !was.wide_defer && f.wide_defer;
                moved[1] += was.wide_defer && !f.wide_defer;
                moved[2] += !was.wide_scatter && f.wide_scatter;
                moved[3] += was.wide_scatter && !f.wide_scatter;
                moved[4] += f.t8_wide_until != was.t8_wide_until;
                moved[5] += f.seq_until != was.seq_until;
                moved[6] += f.agg_passes > was.agg_passes;
                moved[7] += f.agg_passes < was.agg_passes;
                moved[8] += h.wused < was.seen_wused;
                moved[9] += h.retried < was.seen_retried;
                moved[10] += h.agg_launches < was.seen_agg_launches || h.agg_groups < was.seen_agg_groups;
                moved[11] += was.wide_defer && h.wfold_n < was.seen_wfold;
                const uint64_t b = o.stats.batches, at_b[6] = {b, b + 1, f.t8_wide_until, f.t8_wide_until ? f.t8_wide_until - 1 : 0, f.seq_until, f.seq_until ? f.seq_until - 1 : 0};
                bool same = same_state(o, f);
                for (uint64_t q : at_b) same = same && same_answers(o, f, q);
                if (!same && mismatches++ < 5)
                    printf("mismatch: wide_mode %d t8_mode %d seq_mode %d forced %u wtab %d log %d seed %u look %d\n", wide_mode, t8_mode, seq_mode, fp, wtab, log_ok, seed, i);
            }
        }
    }
    printf("diff combos %llu looks %llu mismatches %llu\n", combos, looks, mismatches);
    printf("reached log_entered %llu log_left %llu scatter_on %llu scatter_off %llu wide_tuples %llu learnt_order %llu passes_up %llu passes_down %llu"
           " wused_restart %llu retried_restart %llu agg_restart %llu wfold_restart %llu\n",
           moved[0], moved[1], moved[2], moved[3], moved[4], moved[5], moved[6], moved[7], moved[8], moved[9], moved[10], moved[11]);
    return mismatches ? 1 : 0;
}

// ---- the modes driven from the test ----------------------------------------------------------------------------------------
static void print_feedback(const IngestFeedback& f, uint64_t b) {
    printf("state probed %d defer %d scatter %d seen_wused %" PRIu64 " seen_ok_w %" PRIu64 " seen_wfold %" PRIu64 " t8_wide_until %" PRIu64 " seen_misfit8 %" PRIu64
           " seen_ok %" PRIu64 " seen_retried %" PRIu64 " seq_until %" PRIu64 " seen_agg_groups %" PRIu64 " seen_agg_launches %" PRIu64 " agg_passes %u"
           " compact_tuples %d learnt_order %d wide_scatter_sink %d log_mode %d left_log_mode %d wants_probe %d passes %u\n",
           (int)f.wide_probed, (int)f.wide_defer, (int)f.wide_scatter, f.seen_wused, f.seen_ok_w, f.seen_wfold, f.t8_wide_until, f.seen_misfit8, f.seen_ok,
           f.seen_retried, f.seq_until, f.seen_agg_groups, f.seen_agg_launches, f.agg_passes, (int)f.compact_tuples(b), (int)f.learnt_order(b),
           (int)f.wide_scatter_sink(), (int)f.log_mode(), (int)f.left_log_mode(), (int)f.wants_probe(), f.passes());
}
static int run_looks() {
    IngestFeedback f;
    uint64_t b = 0;
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        int wm, tm, sm, wt, la;
        unsigned fp, pl;
        FeedbackLook h;
        if (sscanf(line, "knobs %d %d %d %u %u %d %d", &wm, &tm, &sm, &fp, &pl, &wt, &la) == 7) {
            f = IngestFeedback{};
            f.knobs = FeedbackKnobs{wm, tm, sm, fp, pl, wt != 0, la != 0};
            b = 0;
        } else if (sscanf(line, "look %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &h.ok, &h.misfit8, &h.retried,
                          &h.wused, &h.wfold_n, &h.agg_launches, &h.agg_groups, &b) == 8) {
            f.look(h, b);
        } else if (sscanf(line, "at %" SCNu64, &b) == 1) {  // (the answers at another batch count)
        } else if (!strncmp(line, "probed", 6)) {
            f.mark_probed();
        } else {
            return 2;
        }
        print_feedback(f, b);
    }
    return 0;
}
static int run_plan() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        unsigned ks, plog2;
        int sink_mode, grid, cms_atomic, cms_ok, wtab, cand, wm, tm, sm, scatter, defer;
        uint64_t n, batches, t8_until, seq_until;
        if (sscanf(line, "%u %d %" SCNu64 " %u %d %d %d %d %d %d %d %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %d", &ks, &sink_mode, &n, &plog2, &grid, &cms_atomic, &cms_ok, &wtab,
                   &cand, &wm, &tm, &sm, &batches, &t8_until, &seq_until, &scatter, &defer) != 17)
            return 2;
        IngestFeedback f;
        f.knobs.wide_mode = wm;
        f.knobs.t8_mode = tm;
        f.knobs.seq_mode = sm;
        f.knobs.wide_table = wtab != 0;
        f.t8_wide_until = t8_until;
        f.seq_until = seq_until;
        f.wide_scatter = scatter != 0;
        f.wide_defer = defer != 0;
        LaunchPlan p;
        plan_sink(p, ks, sink_mode, (size_t)n, plog2, f, batches);
        p.grid = grid;
        plan_segments(p, ks, cms_atomic != 0, cms_ok != 0, wtab != 0, f);
        plan_followers(p, ks, cand != 0, f, batches);
        printf("plan variant %u wave_tiles %d t8 %d seq_variant %d cms_segments %d wide_segments %d wlog %d side %d\n", p.variant, (int)p.wave_tiles, (int)p.t8,
               (int)p.seq_variant, (int)p.cms_segments, (int)p.wide_segments, (int)p.wlog, (int)p.side);
    }
    return 0;
}
static int run_guard() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        GuardSnapshot s;
        GuardHost g;
        int wtab;
        uint64_t n;
        if (sscanf(line, "%u %u %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %u %u %d %u %" SCNu64 " %" SCNu64, &s.spill_count, &s.wspill_count, &s.used,
                   &s.wused, &g.used_base, &g.wused_base, &g.slots, &g.wslots, &g.spill_cap, &g.wspill_cap, &wtab, &g.wide_per_record, &g.in_flight, &n) != 14)
            return 2;
        g.wide_table = wtab != 0;
        printf("verdict guard %d\n", (int)guard_verdict(s, g, (size_t)n));
    }
    return 0;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "diff";
    if (!strcmp(mode, "diff")) return run_diff();
    if (!strcmp(mode, "looks")) return run_looks();
    if (!strcmp(mode, "plan")) return run_plan();
    if (!strcmp(mode, "guard")) return run_guard();
    return 2;
}
