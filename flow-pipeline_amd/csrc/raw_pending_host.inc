// raw_pending_host.inc - the pending flows_raw parts of a live ctx as the input of the probe, select and query doors (included by
// flowagg.hip behind raw_query_host.inc: one translation unit; device side: raw_bounds.cuh; the classification: raw_pending_plan.h;
// the contract: include/flowagg.h "the pending flows_raw parts as input").
//
// The file doors bring HOST bytes to HBM, decode and validate them (range_run) and hand a RangeRun - every part's place in an
// image, its rows and its slice [r_lo, r_hi) - to select_over / query_over.  The pending parts of a ctx (RawState::img,
// RawState::pending of raw_host.inc) lie in HBM already, in the layout those bodies read, the library wrote every byte of them,
// and the host holds each part's t_min / t_max.  pending_run builds the same RangeRun from them: nothing is copied, decoded,
// validated, taken or changed; LoadState and RangeState are not touched (no load buffer is used, no load or range statistic moves).
// One call: the host classifies every pending part (raw_pending_class).  Only when a part must be SEARCHED: ONE small plan copy,
// raw_bounds_kernel (one wave per searched part), ONE small copy back, ONE wait.  A range that covers everything pending, or
// nothing, launches no bounds kernel and waits for nothing here.  Then select_over / query_over with their own waits.
// Memory (PendingState, kept until fa_raw_reset / fa_destroy): 48 bytes per searched part, and as many page-locked.

struct PendingState {
    DevBuf<> plan;      // the searched parts | their records
    PinnedBuf<> h_plan; // both on their way
    Events ev;          // 2: around the bounds launch
    fa_raw_pending_stats_t st{};
};

// fa_raw_reset: the buffers go, the counters of fa_raw_pending_stats go on counting
static void pending_release(fa_ctx* c) {
    PendingState* g = c->pending;
    if (!g) return;
    g->plan.reset(), g->h_plan.reset();
}
static int pending_state(fa_ctx* c, PendingState** out) {
    const int rc = state_with_events(c, c->pending, 2);
    *out = c->pending;
    return rc;
}

// The pending parts of the ctx, in build order, as the RangeRun of a time range.  Refusals (FA_ERR_ARG) come before any launch.
static int pending_run(fa_ctx* c, PendingState* g, const char* fn, uint32_t t_lo, uint32_t t_hi, RangeRun& run) {
    RawState* t = c->raw;
    const size_t np = t->pending.size();
    if (t_lo > t_hi) return fail(c, FA_ERR_ARG, std::string(fn) + ": t_lo > t_hi");
    for (const fa_raw_part& p : t->pending)
        if (p.rows > 0xFFFFFFFFull) return fail(c, FA_ERR_ARG, std::string(fn) + ": a pending part of more than 2^32 - 1 rows");
    // The image is read where it lies.  Its parts were written by launches on c->stream (the build's and the merge's gathers, the
    // copy of a grown image) and everything below is queued on c->stream: stream order is all the ordering there is.  The pointer
    // is read in every call: raw_reserve_image and fa_raw_merge replace the image.
    run.image = t->img.get();
    run.parts.assign(np, RangePart{});
    std::vector<uint32_t> srch;
    fa_raw_pending_stats_t d{};
    for (size_t i = 0; i < np; i++) {
        const fa_raw_part& p = t->pending[i];
        RangePart& r = run.parts[i];
        r.plan = RawPartPlan{p.offset, p.bytes, 0, 0xFFFFFFFFu};
        r.rows = p.rows, r.date = p.date;
        d.rows_seen += p.rows;
        switch (raw_pending_class(p.rows, p.t_min, p.t_max, t_lo, t_hi)) {
        case RAW_PENDING_SKIPPED: d.parts_skipped++; break;
        case RAW_PENDING_WHOLE:
            d.parts_whole++;
            r.selected = true, r.r_lo = 0, r.r_hi = p.rows, r.t_min = p.t_min, r.t_max = p.t_max;
            break;
        default:
            d.parts_searched++;
            r.selected = true;
            srch.push_back((uint32_t)i);
        }
    }
    const size_t ns = srch.size();
    if (ns) {
        const size_t o_rec = align256(ns * sizeof(RawBoundsPart)), total = o_rec + ns * sizeof(RawBoundsRec);
        int rc = ensure_dev(c, g->plan, total, "pending plan");
        if (rc) return rc;
        if (!g->h_plan.grow(total, total + total / 2)) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "hipHostMalloc(pending plan) failed; nothing was read");
        }
        uint8_t *db = (uint8_t*)g->plan.get(), *hb = (uint8_t*)g->h_plan.get();
        RawBoundsPart* h_parts = (RawBoundsPart*)hb;
        const RawBoundsRec* h_rec = (const RawBoundsRec*)(hb + o_rec);
        for (size_t j = 0; j < ns; j++) h_parts[j] = RawBoundsPart{run.parts[srch[j]].plan.off, (uint32_t)run.parts[srch[j]].rows, 0};
        HIPCHK(c, hipMemcpyAsync(db, hb, ns * sizeof(RawBoundsPart), hipMemcpyHostToDevice, c->stream));
        (void)hipEventRecord(g->ev[0], c->stream);
        hipLaunchKernelGGL(raw_bounds_kernel, dim3((unsigned)ns), dim3(64), 0, c->stream, (const RawBoundsPart*)db, (uint32_t)ns, run.image, t_lo, t_hi, (RawBoundsRec*)(db + o_rec));
        (void)hipEventRecord(g->ev[1], c->stream);
        HIPCHK(c, hipGetLastError());
        g->st.bounds_launches++;  // (counted once it is launched, as the file doors count a refused call's launches)
        HIPCHK(c, hipMemcpyAsync(hb + o_rec, db + o_rec, ns * sizeof(RawBoundsRec), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        Events::elapsed_ns(g->ev[0], g->ev[1], &g->st.bounds_ns);
        for (size_t j = 0; j < ns; j++) {
            RangePart& r = run.parts[srch[j]];
            const RawBoundsRec& b = h_rec[j];
            if (b.r_lo > b.r_hi || b.r_hi > r.rows || b.steps > 2 * raw_bounds_max_steps(r.rows)) return fail(c, FA_ERR_HIP, "internal: a pending part's row range is inconsistent");
            r.r_lo = b.r_lo, r.r_hi = b.r_hi;
            if (r.r_lo < r.r_hi) r.t_min = b.t_min, r.t_max = b.t_max;
        }
    }
    // ---- the call's input stands
    for (const RangePart& r : run.parts) d.rows_in_range += r.r_hi - r.r_lo;
    fa_raw_pending_stats_t& s = g->st;
    s.calls++, s.parts_seen += np, s.parts_skipped += d.parts_skipped, s.parts_whole += d.parts_whole, s.parts_searched += d.parts_searched;
    s.rows_seen += d.rows_seen, s.rows_in_range += d.rows_in_range;
    return FA_OK;
}

extern "C" int fa_raw_pending_probe(fa_ctx* c, uint32_t t_lo, uint32_t t_hi, fa_raw_range* out, size_t cap, size_t* n_out) {
    RAW_ENTER(c, "fa_raw_pending_probe");
    if (!n_out || (!out && cap)) return fail(c, FA_ERR_ARG, "fa_raw_pending_probe: null argument");
    *n_out = c->raw->pending.size();
    if (*n_out > cap) return fail(c, FA_ERR_CAPACITY, "fa_raw_pending_probe: the range buffer is too small (the pending parts there are is returned); nothing was launched");
    PendingState* g = nullptr;
    int rc = pending_state(c, &g);
    if (rc) return rc;
    RangeRun run;
    rc = pending_run(c, g, "fa_raw_pending_probe", t_lo, t_hi, run);
    if (rc) return rc;
    for (size_t i = 0; i < run.parts.size(); i++) {
        const RangePart& p = run.parts[i];
        out[i] = fa_raw_range{p.date, p.t_min, p.t_max, 0, p.rows, p.r_lo, p.r_hi};
    }
    return FA_OK;
}

extern "C" int fa_raw_query_pending(fa_ctx* c, const fa_raw_query_t* query) {
    RAW_ENTER(c, "fa_raw_query_pending");
    if (!query) return fail(c, FA_ERR_ARG, "fa_raw_query_pending: null argument");
    const fa_raw_query_t qa = *query;
    int rc = query_check(c, "fa_raw_query_pending", qa);
    if (rc) return rc;
    PendingState* g = nullptr;
    rc = pending_state(c, &g);
    if (rc) return rc;
    QueryState* q = nullptr;
    rc = query_start(c, &q, qa);  // (the result held ends here unless KEEP; the ctx's selection stays: no load buffer is used)
    if (rc) return rc;
    RangeRun run;
    rc = pending_run(c, g, "fa_raw_query_pending", qa.where.t_lo, qa.where.t_hi, run);
    if (rc) return rc;
    return query_over(c, q, "fa_raw_query_pending", run, qa);
}

extern "C" int fa_raw_select_pending(fa_ctx* c, const fa_raw_filter* filter, fa_raw_part* parts, size_t parts_cap, size_t* n_parts, size_t* bytes_out) {
    RAW_ENTER(c, "fa_raw_select_pending");
    if (!filter || !n_parts || !bytes_out || (!parts && parts_cap)) return fail(c, FA_ERR_ARG, "fa_raw_select_pending: null argument");
    *n_parts = 0, *bytes_out = 0;
    select_drop(c);  // (the previous selection ends when the call starts: fa_raw_select's rule)
    const fa_raw_filter f = *filter;
    if (const char* why = raw_select_filter_why(f)) {
        c->err = std::string("fa_raw_select_pending: ") + why;
        return FA_ERR_ARG;
    }
    PendingState* g = nullptr;
    int rc = pending_state(c, &g);
    if (rc) return rc;
    rc = state_with_events(c, c->select, 6);
    if (rc) return rc;
    const size_t np = c->raw->pending.size();
    if (np > parts_cap) {
        *n_parts = np;
        return fail(c, FA_ERR_CAPACITY, "fa_raw_select_pending: the parts buffer is too small (the pending parts there are is returned); nothing was launched");
    }
    RangeRun run;
    rc = pending_run(c, g, "fa_raw_select_pending", f.t_lo, f.t_hi, run);
    if (rc) return rc;
    return select_over(c, c->select, "fa_raw_select_pending", run, f, parts, n_parts, bytes_out);
}

extern "C" int fa_raw_pending_stats(fa_ctx* c, fa_raw_pending_stats_t* out) {
    RAW_ENTER(c, "fa_raw_pending_stats");
    if (!out) return fail(c, FA_ERR_ARG, "fa_raw_pending_stats: null argument");
    memset(out, 0, sizeof *out);
    if (c->pending) *out = c->pending->st;
    return FA_OK;
}
