// maintain_host.inc - table growth / replay (settle), launch feedback, counter snapshots, the wide log (included by flowagg.hip: one translation unit, see kernels.cuh for the device side).

// ---- table maintenance -------------------------------------------------------------
// Builds a fresh table of 2^new_log2 slots holding every row outside [tb_lo,tb_hi).
static int rebuild_table(fa_ctx* c, uint32_t new_log2, uint32_t tb_lo, uint32_t tb_hi) {
    DevBuf<Slot> nt;
    size_t bytes = sizeof(Slot) << new_log2;
    if (!nt.grow(bytes)) return fail(c, FA_ERR_NOMEM, "rebuild_table: hipMalloc failed");
    hipError_t e;
    if ((e = hipMemsetAsync(nt, 0, bytes, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(&c->d_ctr->used, 0, sizeof(unsigned long long), c->stream)) != hipSuccess) {
        c->err = std::string("rebuild_table: ") + hipGetErrorString(e);  // (the old table stays in place)
        return FA_ERR_HIP;
    }
    DevBuf<Slot> old = std::move(c->tab);  // released on every way out of here, after the kernel that reads it
    c->tab = std::move(nt);
    uint32_t old_slots = 1u << c->cap_log2;
    c->cap_log2 = new_log2;
    KArgs a = make_args(c);
    hipLaunchKernelGGL(rebuild_kernel, dim3(1024), dim3(256), 0, c->stream, old.get(), old_slots, tb_lo, tb_hi, a);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->used_base = 0;
    c->stats.table_capacity = 1ull << c->cap_log2;
    return FA_OK;
}

// Wide table: fresh table of 2^new_log2 slots holding every row that is not selected by
// (kind_mask, [tb_lo,tb_hi)) - see wrow_selected().
static int rebuild_wide(fa_ctx* c, uint32_t new_log2, uint32_t kind_mask, uint32_t tb_lo, uint32_t tb_hi) {
    DevBuf<WSlot> nt;
    size_t bytes = sizeof(WSlot) << new_log2;
    if (!nt.grow(bytes)) return fail(c, FA_ERR_NOMEM, "rebuild_wide: hipMalloc failed");
    hipError_t e;
    if ((e = hipMemsetAsync(nt, 0, bytes, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(&c->d_ctr->wused, 0, sizeof(unsigned long long), c->stream)) != hipSuccess) {
        c->err = std::string("rebuild_wide: ") + hipGetErrorString(e);  // (the old table stays in place)
        return FA_ERR_HIP;
    }
    DevBuf<WSlot> old = std::move(c->wtab);  // released on every way out of here, after the kernel that reads it
    c->wtab = std::move(nt);
    uint32_t old_slots = 1u << c->wcap_log2;
    c->wcap_log2 = new_log2;
    KArgs a = make_args(c);
    hipLaunchKernelGGL(wrebuild_kernel, dim3(1024), dim3(256), 0, c->stream, old.get(), old_slots, kind_mask, tb_lo, tb_hi, a);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->wused_base = 0;
    c->wide_dead = 0;  // (slots without rows were not carried over)
    c->stats.wide_capacity = 1ull << c->wcap_log2;
    return FA_OK;
}

static uint32_t log2_ceil(uint64_t v) {
    uint32_t l = 0;
    while ((1ull << l) < v) l++;
    return l;
}

// grows the wide table / replays parked updates until nothing is pending (h = fresh copy of the counters)
static int settle_wide(fa_ctx* c, Counters& h) {
    if (!c->wtab) return FA_OK;
    c->stats.wide_used = c->wused_base + h.wused;
    if (h.wspill_lost) {
        c->sticky = FA_ERR_TABLE_FULL;
        return fail(c, FA_ERR_TABLE_FULL, "wide-key table and its spill buffer overflowed; aggregates were lost");
    }
    int guard = 0;
    while (h.wspill_count || c->stats.wide_used * 2 > (1ull << c->wcap_log2)) {
        // room for every group that exists plus every parked update, at <= 50 % load, in ONE step - at the SAME size when
        // the slots that closed windows left dead (wdrop_kernel) are what fills the table
        const uint64_t live = c->stats.wide_used - std::min(c->wide_dead, c->stats.wide_used);
        const uint32_t want = c->wide_dead ? std::max(c->wcap_log2, log2_ceil(2 * (live + h.wspill_count))) :
                                             std::max(c->wcap_log2 + 1, log2_ceil(2 * (c->stats.wide_used + h.wspill_count)));
        if (want > 30 || ++guard > 8) return fail(c, FA_ERR_TABLE_FULL, "wide-key table cannot grow further");
        const uint32_t nspill = h.wspill_count;
        // the parked updates move to a private copy and the buffer is emptied BEFORE the rebuild, so that anything the
        // rebuild or the replay parks again is kept for the next round of this loop
        DevBuf<WSpillEntry> tmp;
        if (nspill) {
            if (!tmp.grow(sizeof(WSpillEntry) * nspill)) return fail(c, FA_ERR_NOMEM, "hipMalloc(wide spill copy) failed");
            if (hipMemcpyAsync(tmp, c->wspill, sizeof(WSpillEntry) * nspill, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return fail(c, FA_ERR_HIP, "settle_wide: copy failed");
        }
        hipError_t e0 = hipMemsetAsync(&c->d_ctr->wspill_count, 0, sizeof(unsigned int), c->stream);
        int rc = e0 == hipSuccess ? rebuild_wide(c, want, 0, 0, 0 /* nothing selected: keep everything */) : FA_ERR_HIP;
        if (rc == FA_OK && nspill) {
            KArgs a = make_args(c);
            static_assert(sizeof(WSpillEntry) == sizeof(WRow), "spill entries replay as rows");
            hipLaunchKernelGGL(wmerge_kernel, dim3(256), dim3(256), 0, c->stream, (const WRow*)tmp.get(), nspill, a);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = FA_ERR_HIP;
        }
        if (rc) return rc == FA_ERR_HIP ? fail(c, FA_ERR_HIP, "settle_wide: replay failed") : rc;
        HIPCHK(c, hipMemcpy(c->h_ctr, c->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost));
        h = *c->h_ctr;
        c->stats.wide_used = c->wused_base + h.wused;
        if (h.wspill_lost) return fail(c, FA_ERR_TABLE_FULL, "wide spill buffer overflowed during replay");
    }
    return FA_OK;
}

static int cms_fold(fa_ctx* c);

// one look of the adaptive feedback (ingest_feedback.h: what the next LaunchPlans are decided from): h = counters at least as new as the last look's
static void feedback_look(fa_ctx* c, const Counters& h) {
    c->fb.look(FeedbackLook{h.ok, h.misfit8, h.retried, h.wused, h.wfold_n, h.agg_launches, h.agg_groups}, c->stats.batches);
}

// Waits for the stream, folds device counters into stats, replays spills after growing.
static int settle(fa_ctx* c) {
    if (c->cms_dirty) {
        int frc = cms_fold(c);
        if (frc) return frc;
    }
    HIPCHK(c, hipMemcpyAsync(c->h_ctr, c->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i + 2 < c->ev_pool.used(); i += 3) {
        uint64_t ns = 0;
        if (Events::elapsed_ns(c->ev_pool[i], c->ev_pool[i + 1], &ns)) {
            c->stats.kernel_ns = ns;
            c->stats.kernel_ns_total += ns;
            c->stats.kernel_launches += 1;
        }
        Events::elapsed_ns(c->ev_pool[i], c->ev_pool[i + 2], &c->stats.batch_ns_total);
    }
    c->ev_pool.rewind();
    for (size_t i = 0; i + 2 < c->dev_pool.used(); i += 3)
        if (Events::elapsed_ns(c->dev_pool[i], c->dev_pool[i + 2], &c->stats.decode_ns_total)) c->stats.decode_launches += 1;
    c->dev_pool.rewind();
    Counters h = *c->h_ctr;
    c->stats.records_ok = h.ok;
    c->stats.records_bad = h.bad;
    c->stats.records_slow = h.slow;
    c->stats.records_direct = h.direct;
    c->stats.records_retried = h.retried;
    c->stats.records_misfit_compact = h.misfit8;
    c->stats.records_late = h.late;
    c->stats.table_used = c->used_base + h.used;
    feedback_look(c, h);
    if (h.spill_lost) {
        c->sticky = FA_ERR_TABLE_FULL;
        return fail(c, FA_ERR_TABLE_FULL, "group-by table and spill buffer overflowed; aggregates were lost");
    }
    int guard = 0;
    while (h.spill_count || c->stats.table_used * 2 > (1ull << c->cap_log2)) {
        // room for every group that exists plus every parked update, at <= 50 % load, in ONE step
        const uint32_t want = std::max(c->cap_log2 + 1, log2_ceil(2 * (c->stats.table_used + h.spill_count)));
        if (want > 30 || ++guard > 8) return fail(c, FA_ERR_TABLE_FULL, "group-by table cannot grow further");
        const uint32_t nspill = h.spill_count;
        // the parked aggregates move to a private copy and the buffer is emptied BEFORE the rebuild, so that anything
        // the rebuild or the replay parks again is kept for the next round of this loop
        DevBuf<SpillEntry> tmp;
        if (nspill) {
            if (!tmp.grow(sizeof(SpillEntry) * nspill)) return fail(c, FA_ERR_NOMEM, "hipMalloc(spill copy) failed");
            if (hipMemcpyAsync(tmp, c->spill, sizeof(SpillEntry) * nspill, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return fail(c, FA_ERR_HIP, "settle: copy failed");
        }
        hipError_t e0 = hipMemsetAsync(&c->d_ctr->spill_count, 0, sizeof(unsigned int), c->stream);
        int rc = e0 == hipSuccess ? rebuild_table(c, want, 1, 0 /* empty range: keep everything */) : FA_ERR_HIP;
        if (rc == FA_OK && nspill) {
            KArgs a = make_args(c);
            hipLaunchKernelGGL(replay_spill_kernel, dim3(1024), dim3(256), 0, c->stream, tmp.get(), nspill, a);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = FA_ERR_HIP;
        }
        if (rc) return rc == FA_ERR_HIP ? fail(c, FA_ERR_HIP, "settle: replay failed") : rc;
        HIPCHK(c, hipMemcpy(c->h_ctr, c->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost));
        h = *c->h_ctr;
        c->stats.table_used = c->used_base + h.used;
        if (h.spill_lost) return fail(c, FA_ERR_TABLE_FULL, "spill buffer overflowed during replay");
    }
    int rc = settle_wide(c, h);
    // everything launched so far is accounted for
    c->known = h;
    c->known_records = c->launched_records;
    c->known_seq = c->launch_seq;
    c->known_wpot = c->wpot_total;
    return rc;
}

// ---- wide log (FA_WIDE=log; fa_ctx::wlog) -----------------------------------------------------------------------------
static WChunkArgs wchunk_args(const fa_ctx::WChunk& k) {
    return WChunkArgs{k.seg, k.counts, k.tail(), 1u << k.wplog2, k.nwg, k.wcapq, k.wm, k.wregion};
}
// room in the table for `more` new rows at <= 50 % load (host-side bound first; a settle - and a one-step growth - only when
// the bound says so)
static uint64_t wide_rows_bound(const fa_ctx* c) { return c->wused_base + c->known.wused + (c->wpot_total - c->known_wpot); }
static int wlog_make_room(fa_ctx* c, uint64_t more) {
    if ((wide_rows_bound(c) + more) * 2 <= (1ull << c->wcap_log2)) return FA_OK;
    int rc = settle(c);  // (exact count; grows the table by itself when it is above 50 % already)
    if (rc) return rc;
    if ((c->stats.wide_used + more) * 2 <= (1ull << c->wcap_log2)) return FA_OK;
    // (slots whose rows a window close zeroed are occupied but hold nothing: a rebuild drops them, so the new size follows the
    // LIVE rows - as settle_wide does; sized by wide_used a fold / close / fold cycle doubled a table that was mostly dead slots)
    const uint64_t live = c->stats.wide_used - std::min(c->wide_dead, c->stats.wide_used);
    const uint32_t want = c->wide_dead ? std::max(c->wcap_log2, log2_ceil(2 * (live + more))) : log2_ceil(2 * (c->stats.wide_used + more));
    if (want > 30) return fail(c, FA_ERR_TABLE_FULL, "wide-key table cannot grow further");
    return rebuild_wide(c, want, 0, 0, 0);  // (pending chunks stay pending: they are folded by the atomic replay from now on)
}
// one pending chunk into the table: wagg_kernel while the table still has the geometry the tuples were scattered for (its
// workgroups own "their" regions' tuples), the atomic replay otherwise; the buffers go to the free list
static int wlog_fold(fa_ctx* c, fa_ctx::WChunk k) {
    KArgs a = make_args(c);
    if (k.wplog2 == a.wplog2 && k.wmask == a.wmask) {
        a.wseg = k.seg;
        a.wseg_counts = k.counts;
        a.nwg = k.nwg;
        a.wcapq = k.wcapq;
        a.wregion = k.wregion;
        hipLaunchKernelGGL(wagg_kernel, dim3(1u << a.wplog2), dim3(WAGG_BLOCK), 0, c->stream, a, (const uint32_t*)k.tail(), k.wm);
        c->wlog_folded++;
    } else {
        hipLaunchKernelGGL(wlog_replay_kernel, dim3(2048), dim3(256), 0, c->stream, wchunk_args(k), a);
        c->wlog_replayed++;
    }
    HIPCHK(c, hipGetLastError());
    c->wpot_total += k.n;
    c->wlog_free.push_back(std::move(k));
    return FA_OK;
}
static int wlog_flush_oldest(fa_ctx* c) {
    int rc = wlog_make_room(c, c->wlog.front().n);
    if (rc) return rc;
    fa_ctx::WChunk k = std::move(c->wlog.front());
    c->wlog.erase(c->wlog.begin());
    return wlog_fold(c, std::move(k));
}
static int wlog_flush_all(fa_ctx* c) {
    while (!c->wlog.empty()) {
        int rc = wlog_flush_oldest(c);
        if (rc) return rc;
    }
    return FA_OK;
}
// behind a log-mode launch: its segment buffers become the newest chunk (the ctx allocates or recycles others for the next
// launch); more than wlog_max pending: the oldest is folded into the table after all
static void reserve_window_read(fa_ctx* c, uint64_t rows, uint32_t nseg);  // (rows_host.inc)
static int wlog_record(fa_ctx* c, const KArgs& a, size_t n) {
    fa_ctx::WChunk k;
    k.seg = std::move(c->wseg);
    k.counts = std::move(c->wseg_counts);
    k.nwg = a.nwg;
    k.wcapq = a.wcapq;
    k.wplog2 = a.wplog2;
    k.wmask = a.wmask;
    k.wregion = a.wregion;
    k.n = n;
    const uint32_t nseg = (1u << k.wplog2) * k.nwg;
    c->wlog.push_back(std::move(k));
    c->wlog_recorded++;
    // a window of this key set is about a chunk's worth of rows (Kafka partitions are close to time-ordered): what its read
    // will allocate is allocated here, outside the close
    reserve_window_read(c, c->stats.wide_used + n + n / 16, nseg);
    while (c->wlog.size() > c->wlog_max) {
        int rc = wlog_flush_oldest(c);
        if (rc) return rc;
    }
    return FA_OK;
}
// a drop of buckets [lo, hi) as far as the pending chunks go: when nothing older is alive in them it is their watermark
// (tuples below it are skipped by every later read and fold); anything else folds them into the table first, where the
// caller's rebuild removes the range.  "Older" is judged by the smallest bucket among a chunk's live tuples - looked for
// once per chunk (a scan of its segments, the word behind the time base) and kept: with the launch's time base instead
// (the smallest SAMPLED bucket - 2) every close of a real timeslot found "something older" and folded all chunks.
// every pending chunk's bucket range [minb, maxb]: the ingest kernel kept it while it wrote the tuples (sinks.cuh, wide_sink_wave;
// the three words behind the chunk's counts: time base, smallest bucket, ~largest bucket) - 8 bytes to fetch per chunk, once.
// (Rounds 3-4 scanned every chunk at the first close: 1.8 ms of a 27 ms read for six chunks.)  FA_WLOG_RANGE_CHECK=1 scans as well
// and compares - tests.
static int wlog_bucket_ranges(fa_ctx* c) {
    bool any = false;
    for (auto& k : c->wlog) any = any || !k.minb_known;
    if (!any) return FA_OK;
    const bool check = getenv("FA_WLOG_RANGE_CHECK") != nullptr;
    std::vector<uint32_t> mm(2 * c->wlog.size()), scan(2 * c->wlog.size());
    for (size_t i = 0; i < c->wlog.size(); i++)
        if (!c->wlog[i].minb_known) HIPCHK(c, hipMemcpyAsync(&mm[2 * i], c->wlog[i].tail() + 1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (check) {
        for (size_t i = 0; i < c->wlog.size(); i++) {
            fa_ctx::WChunk& k = c->wlog[i];
            if (k.minb_known) continue;
            uint32_t* word = k.tail() + 1;  // (scanned over the kernel's words: they are on the host by now)
            HIPCHK(c, hipMemsetAsync(word, 0xff, sizeof(uint32_t), c->stream));
            HIPCHK(c, hipMemsetAsync(word + 1, 0, sizeof(uint32_t), c->stream));
            hipLaunchKernelGGL(wlog_minbucket_kernel, dim3(2048), dim3(256), 0, c->stream, wchunk_args(k), word);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&scan[2 * i], word, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (size_t i = 0; i < c->wlog.size(); i++) {
        fa_ctx::WChunk& k = c->wlog[i];
        if (k.minb_known) continue;
        k.minb = mm[2 * i];  // (~0: no tuple at all)
        k.maxb = k.minb == 0xFFFFFFFFu ? 0u : ~mm[2 * i + 1];
        k.minb_known = true;
        if (check && k.wm == 0 && (k.minb != scan[2 * i] || k.maxb != scan[2 * i + 1]))
            return fail(c, FA_ERR_HIP, "internal: a wide-log chunk's bucket range differs from its scan");
    }
    return FA_OK;
}
static int wlog_drop(fa_ctx* c, uint32_t lo, uint32_t hi) {
    if (c->wlog.empty()) return FA_OK;
    int rc0 = wlog_bucket_ranges(c);
    if (rc0) return rc0;
    uint32_t oldest = 0xFFFFFFFFu;  // smallest bucket any pending chunk still holds
    for (size_t i = 0; i < c->wlog.size(); i++) {
        fa_ctx::WChunk& k = c->wlog[i];
        if (k.minb != 0xFFFFFFFFu && k.maxb >= k.wm) oldest = std::min(oldest, std::max(k.minb, k.wm));
    }
    if (lo > oldest) return wlog_flush_all(c);  // (a range that is not the oldest: the table's rebuild has to remove it)
    for (size_t i = 0; i < c->wlog.size();) {
        fa_ctx::WChunk& k = c->wlog[i];
        if (hi > k.wm) {
            k.wm = hi;
            c->wlog_wm_moves++;
        }
        if (k.minb == 0xFFFFFFFFu || k.maxb < k.wm) {  // nothing of this chunk is alive
            c->wlog_free.push_back(std::move(k));
            c->wlog_dropped++;
            c->wlog.erase(c->wlog.begin() + (long)i);
        } else {
            i++;
        }
    }
    return FA_OK;
}

// ---- counter snapshots: never lose aggregates ------------------------------------------------------------
// Every ingest launch is followed by an asynchronous copy of the device counters into a pinned ring slot.  Before
// the next launch the host looks at the newest snapshot that has landed (no waiting): a table above 50 % load or
// parked updates are settled (grow + replay) right away, and a launch is only queued while the updates that could
// be parked by everything in flight still fit the spill buffers - otherwise the host first waits for the newest
// snapshot.  Steady state costs one 300-byte copy per launch and no synchronisation.
static void poll_snapshots(fa_ctx* c, bool wait_newest) {
    if (c->launch_seq == c->known_seq) return;
    if (wait_newest) (void)hipEventSynchronize(c->snap_ev[(c->launch_seq - 1) % fa_ctx::NSNAP]);
    for (uint64_t q = c->launch_seq; q > c->known_seq; q--) {  // newest first
        const int k = (int)((q - 1) % fa_ctx::NSNAP);
        if (c->snap_seq[k] != q) break;  // overwritten: older ones are gone too
        if (hipEventQuery(c->snap_ev[k]) == hipSuccess) {
            c->known = c->h_snap[k];
            c->known_records = c->snap_records[k];
            c->known_seq = q;
            c->known_wpot = c->snap_wpot[k];
            feedback_look(c, c->known);
            return;
        }
    }
}
static int pre_launch_guard(fa_ctx* c, size_t n) {
    auto verdict = [&]() {  // (guard_verdict, launch_plan.h, on the newest snapshot the host has seen)
        const Counters& h = c->known;
        return guard_verdict(GuardSnapshot{h.spill_count, h.wspill_count, h.used, h.wused},
                             GuardHost{c->used_base, c->wused_base, 1ull << c->cap_log2, 1ull << c->wcap_log2, c->spill_cap, c->wspill_cap, c->wtab != nullptr,
                                       c->wide_per_record, c->launched_records - c->known_records},
                             n);
    };
    poll_snapshots(c, false);
    GuardVerdict v = verdict();
    if (v == GUARD_WAIT) {
        poll_snapshots(c, true);
        v = verdict() != GUARD_GO ? GUARD_SETTLE : GUARD_GO;
    }
    return v == GUARD_SETTLE ? settle(c) : FA_OK;
}
static int post_launch_snapshot(fa_ctx* c, size_t n) {
    c->launched_records += n;
    c->launch_seq += 1;
    const int k = (int)((c->launch_seq - 1) % fa_ctx::NSNAP);
    HIPCHK(c, hipEventSynchronize(c->snap_ev[k]));  // (the slot's previous copy, NSNAP launches ago)
    HIPCHK(c, hipMemcpyAsync(&c->h_snap[k], c->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->snap_ev[k], c->stream));
    c->snap_records[k] = c->launched_records;
    c->snap_seq[k] = c->launch_seq;
    c->snap_wpot[k] = c->wpot_total;
    return FA_OK;
}

extern "C" int fa_sync(fa_ctx* c) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    return settle(c);
}
