// raw_query_host.inc - grouped queries over flows_raw parts (included by flowagg.hip behind raw_select_host.inc: one translation
// unit; device side: raw_query.cuh; the contract: include/flowagg.h "grouped queries over flows_raw parts").
//
// One call: range_run(load = true) of raw_range_host.inc - the host's walk, ONE copy of the input, stages A, B and C with their
// three waits and every validation; the query adds no decoding -, then over the slices it left:
//   fold   ONE small plan copy (the slices), raw_query_fold_kernel over the flattened grid of tiles in launches of
//          raw_query_launch_tiles tiles: before each the room rule reserves rows x kinds keys in both tables (keytab_host.inc:
//          tab_reserve, growth by tab_rehash_kernel), so no launch meets a table above half load; ONE wait behind the last
//          (tab_settle: the counters, the launches' times).
// A read: the kind's occupied slots collected by talker_rows_kernel<true> over the range [kind, kind] of table kind & 1, ordered by
// the talkers' stable radix passes (talk_order_passes: four for FA_RAW_O_WEIGHT, three for FA_RAW_O_KEY), cut at k on the
// device; a scalar kind's rows get their value back (raw_query_scalar_rows_kernel); only the rows returned are copied out.
// Another ctx's rows of one kind are added to the result held by fa_raw_query_merge_device / _rows: one check launch and one status
// word, then raw_query_merge_kernel in launches of at most the tables' chunk under the fold's room rule.
// The result lies in the tables until the next query without KEEP, fa_raw_query_reset, fa_raw_load_reset, fa_raw_reset or
// fa_destroy.  Nothing of the ctx's other state is read or written: the tables, the counters and the cursor are the query's own.

struct QueryTabs : TabPair<QueryTab> {
    DevBuf<unsigned int> cursor;  // the collect kernel's row count
    bool alloc_own() { return cursor.grow(sizeof(unsigned int)); }
};
struct QueryState {
    QueryTabs* tabs = nullptr;  // nullptr until the first query and after a release
    ~QueryState() { delete tabs; }
    uint32_t groups = 0;        // of the result held (0: none)
    DevBuf<> plan;              // the slices of the call
    PinnedBuf<> h_plan;
    DevBuf<> rows, order, top;  // a read: the kind's rows collected; the order's scratch; the rows returned
    Events ev;                  // 2: around a read's launches
    fa_raw_query_stats_t st{};  // calls, rows_scanned, updates, launches (reads), order_ns; the rest comes from the tables
    uint64_t matched0 = 0, absorbed0 = 0, grows0 = 0, launches0 = 0, fold_ns0 = 0;  // ... of tables that were released
    uint64_t matched_seen = 0;  // rows matched up to the last call's end (a call's updates = its matched rows x its kinds)
    fa_raw_query_merge_stats_t mst{};  // fa_raw_query_merge_device / _rows: calls that merged, rows they added
    uint64_t merge_launches = 0;       // their check launches (the add launches are counted by the tables, as folds)
};

// the tables' counts into the state (before the tables go)
static void query_bank(fa_ctx* c, QueryState* q) {
    QueryTabs* t = q->tabs;
    if (!t) return;
    TalkCounters h{};
    if (tab_settle(c, *t, h) == FA_OK) q->matched0 += h.folded, q->absorbed0 += h.absorbed;
    q->grows0 += t->grows, q->launches0 += t->fold_launches, q->fold_ns0 += t->fold_ns_total;
}
// fa_raw_load_reset, fa_raw_reset: the result and the buffers go, the counters of fa_raw_query_stats go on counting
static void query_release(fa_ctx* c) {
    QueryState* q = c->query;
    if (!q) return;
    query_bank(c, q);
    state_destroy(q->tabs);
    q->groups = 0;
    q->plan.reset(), q->h_plan.reset(), q->rows.reset(), q->order.reset(), q->top.reset();
}
static int query_state(fa_ctx* c, QueryState** out, bool tables) {
    int rc = state_with_events(c, c->query, 2);
    if (rc) return rc;
    if (tables && !c->query->tabs) {
        rc = tab_enable<QueryTab>(c, c->query->tabs, "fa_raw_query", 0, 0);
        if (rc) return rc;
    }
    *out = c->query;
    return FA_OK;
}
// rows_host.inc's merge of the query row kinds orders its groups in the state's scratch (no tables: any ctx, nothing enabled)
static int query_order_scratch(fa_ctx* c, DevBuf<>** order) {
    QueryState* q = nullptr;
    const int rc = query_state(c, &q, false);
    if (!rc) *order = &q->order;
    return rc;
}
// the groups of the result a ctx holds (0: none) - what the group door checks in every member before it collects
static uint32_t query_groups_held(const fa_ctx* c) { return c->query && c->query->tabs ? c->query->groups : 0u; }

// what a query door refuses in its query (the reason in fa_last_error)
static int query_check(fa_ctx* c, const char* fn, const fa_raw_query_t& qa) {
    const fa_raw_filter& f = qa.where;
    const char* why = raw_select_filter_why(f);
    if (!why && f.limit) why = "where.limit is not 0 (a query has no limit: read the first k rows)";
    if (!why && (f.fields & FA_RAW_F_COUNT_ONLY)) why = "COUNT_ONLY is set (ask for FA_RAW_G_TOTAL)";
    if (!why && !qa.groups) why = "groups is 0";
    if (!why && (qa.groups & ~FA_RAW_G_ALL)) why = "an unknown bit in groups";
    if (!why && (qa.flags & ~FA_RAW_Q_KEEP)) why = "an unknown flag";
    const bool keep = qa.flags & FA_RAW_Q_KEEP;
    if (!why && keep && c->query && c->query->groups && c->query->groups != qa.groups) why = "KEEP with groups other than those of the result held";
    if (why) {
        c->err = std::string(fn) + ": " + why;
        return FA_ERR_ARG;
    }
    return FA_OK;
}
// the state and its tables; without KEEP the result held ends here, when the call starts
static int query_start(fa_ctx* c, QueryState** out, const fa_raw_query_t& qa) {
    int rc = query_state(c, out, true);
    if (rc) return rc;
    if (!(qa.flags & FA_RAW_Q_KEEP)) {
        (*out)->groups = 0;
        rc = tab_reset(c, *(*out)->tabs);
        if (rc) return rc;
    }
    return FA_OK;
}

// The fold over the slices of a run, whatever door the run came from (fa_raw_query: a ranged load's; fa_raw_query_pending of
// raw_pending_host.inc: the ctx's pending parts): every byte the fold kernel reads is in run.image and is a flows_raw part's.
static int query_over(fa_ctx* c, QueryState* q, const char* fn, const RangeRun& run, const fa_raw_query_t& qa) {
    const fa_raw_filter& f = qa.where;
    QueryTabs& t = *q->tabs;
    int rc = FA_OK;
    const SelectSlices slices(run);
    const size_t ns = slices.sl.size();
    const uint64_t scanned = slices.scanned;
    if (slices.ntiles > 0x7FFFFFFFull) return fail(c, FA_ERR_ARG, std::string(fn) + ": more than 2^39 rows in the time range of one call; query the file in pieces with KEEP");
    const uint32_t ntiles = (uint32_t)slices.ntiles, kinds = (uint32_t)__builtin_popcount(qa.groups);
    if (ns) {
        rc = ensure_dev(c, q->plan, ns * sizeof(RawSelectPart), "query plan");
        if (rc) return rc;
        if (!q->h_plan.grow(ns * sizeof(RawSelectPart), ns * sizeof(RawSelectPart) * 3 / 2)) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "hipHostMalloc(query plan) failed; nothing was folded");
        }
        RawSelectPart* h_parts = (RawSelectPart*)q->h_plan.get();
        slices.plan(h_parts, false);
        HIPCHK(c, hipMemcpyAsync(q->plan.get(), h_parts, ns * sizeof(RawSelectPart), hipMemcpyHostToDevice, c->stream));
        for (uint32_t t0 = 0; t0 < ntiles;) {
            const uint32_t nt = std::min(ntiles - t0, raw_query_launch_tiles(t.chunk, kinds));
            const uint64_t keys = raw_query_launch_keys(nt, kinds);
            for (int d = 0; d < 2; d++) {
                rc = tab_reserve(c, t, d, keys);
                if (rc) return rc;
            }
            RawQueryArgs a{};
            a.parts = (const RawSelectPart*)q->plan.get(), a.nparts = (uint32_t)ns, a.groups = qa.groups, a.img = run.image;
            a.tile_lo = t0, a.tile_hi = t0 + nt;
            for (int d = 0; d < 2; d++) a.tab[d] = t.tab[d], a.mask[d] = t.mask(d);
            a.ctr = t.d_ctr, a.f = f;
            rc = tab_fold_launch(c, t, (size_t)nt * RAW_SEL_BLOCK, [&](dim3 grid) { hipLaunchKernelGGL(raw_query_fold_kernel, grid, dim3(RAW_SEL_BLOCK), 0, c->stream, a); });
            if (rc) return rc;
            for (int d = 0; d < 2; d++) t.used_ub[d] += keys;
            t0 += nt;
        }
    }
    TalkCounters h;
    rc = tab_settle(c, t, h);  // (the call's one wait behind the folds; the pinned plan is free again)
    if (rc) return rc;
    q->groups = qa.groups;
    const uint64_t matched = q->matched0 + h.folded;  // (of every call so far)
    q->st.updates += (matched - q->matched_seen) * kinds, q->matched_seen = matched;
    q->st.calls++, q->st.rows_scanned += scanned;
    return FA_OK;
}

extern "C" int fa_raw_query(fa_ctx* c, const uint8_t* bytes, size_t n, const fa_raw_query_t* query) {
    LOAD_ENTER(c);
    if (!query || (!bytes && n)) return fail(c, FA_ERR_ARG, "fa_raw_query: null argument");
    LoadState* s = nullptr;
    int rc = load_state(c, &s);  // (the ctx's selection is dropped here, as under any range call)
    if (rc) return rc;
    const fa_raw_query_t qa = *query;
    rc = query_check(c, "fa_raw_query", qa);
    if (rc) return rc;
    RangeState* g = nullptr;
    rc = range_state(c, &g);
    if (rc) return rc;
    QueryState* q = nullptr;
    rc = query_start(c, &q, qa);
    if (rc) return rc;
    RangeRun run;
    rc = range_run(c, s, g, "fa_raw_query", bytes, n, qa.where.t_lo, qa.where.t_hi, true, (size_t)-1, nullptr, run);
    if (rc) return rc;
    // (from here on every byte the fold kernel reads is decoded and validated)
    return query_over(c, q, "fa_raw_query", run, qa);
}

// the rows of one kind, ordered and cut, in q->top; *n_out = the rows there are to deliver (all of them when cap is too small)
static int query_rows(fa_ctx* c, const char* fn, uint32_t group, int order, size_t k, size_t cap, bool capped, const void** d_rows, size_t* n_out) {
    QueryState* q = c->query;
    if (!n_out) return fail(c, FA_ERR_ARG, std::string(fn) + ": null argument");
    *n_out = 0;
    if (!q || !q->tabs || !q->groups) return fail(c, FA_ERR_ARG, std::string(fn) + ": the ctx holds no query result");
    if (!group || (group & (group - 1)) || !(q->groups & group)) return fail(c, FA_ERR_ARG, std::string(fn) + ": group is exactly one bit of the last query's groups");
    if (order != FA_RAW_O_WEIGHT && order != FA_RAW_O_KEY) return fail(c, FA_ERR_ARG, std::string(fn) + ": order is FA_RAW_O_WEIGHT or FA_RAW_O_KEY");
    QueryTabs& t = *q->tabs;
    const uint32_t kind = (uint32_t)__builtin_ctz(group);
    const int d = (int)(kind & 1u);
    TalkCounters h;
    int rc = tab_settle(c, t, h);
    if (rc) return rc;
    const size_t used = (size_t)h.used[d];  // (every kind of the table: an upper bound of this kind's rows)
    if (!used) return FA_OK;
    rc = ensure_dev(c, q->rows, used * sizeof(TalkRow), "query rows");
    if (rc) return rc;
    (void)hipEventRecord(q->ev[0], c->stream);
    HIPCHK(c, zero_word(t.cursor.get(), c->stream));
    const uint32_t slots = 1u << t.log2[d];
    const unsigned grid = (unsigned)std::min<uint32_t>(512, (slots + TR_BLOCK * TR_U - 1) / (TR_BLOCK * TR_U));
    hipLaunchKernelGGL(talker_rows_kernel<true>, dim3(grid), dim3(TR_BLOCK), 0, c->stream, (const TSlot*)t.tab[d], slots, (TalkRow*)q->rows.get(), (uint32_t)used, t.cursor.get(), kind, kind);
    HIPCHK(c, hipGetLastError());
    q->st.launches++;
    unsigned int got = 0;
    HIPCHK(c, read_word(t.cursor.get(), got, c->stream));
    if (got > used) return fail(c, FA_ERR_HIP, "internal: a query table's rows and its count differ");
    const size_t need = k ? std::min<size_t>(k, got) : got;
    *n_out = need;
    if (capped && need > cap) return fail(c, FA_ERR_CAPACITY, std::string(fn) + ": output buffer too small (the rows needed are returned)");
    if (!need) return FA_OK;
    rc = ensure_dev(c, q->top, need * sizeof(TalkRow), "query rows");
    if (rc) return rc;
    const int passes = order == FA_RAW_O_WEIGHT ? 4 : 3;
    rc = talk_order_passes(c, c->stream, q->order, (const TalkRow*)q->rows.get(), got, need, (TalkRow*)q->top.get(), passes);
    if (rc) return rc;
    q->st.launches += 2 * passes + 1;
    if (!raw_query_kind_is_addr(kind)) {
        hipLaunchKernelGGL(raw_query_scalar_rows_kernel, dim3((unsigned)std::min<size_t>((need + 255) / 256, 1024)), dim3(256), 0, c->stream, (TalkRow*)q->top.get(), (uint32_t)need);
        HIPCHK(c, hipGetLastError());
        q->st.launches++;
    }
    (void)hipEventRecord(q->ev[1], c->stream);
    *d_rows = q->top.get();
    return FA_OK;
}
static void query_read_time(QueryState* q) {
    Events::elapsed_ns(q->ev[0], q->ev[1], &q->st.order_ns);
}

extern "C" int fa_raw_query_rows(fa_ctx* c, uint32_t group, int order, size_t k, fa_query_row* out, size_t cap, size_t* n_out) {
    LOAD_ENTER(c);
    if (!out && cap) return fail(c, FA_ERR_ARG, "fa_raw_query_rows: null argument");
    const void* d_rows = nullptr;
    int rc = query_rows(c, "fa_raw_query_rows", group, order, k, cap, true, &d_rows, n_out);
    if (rc || !d_rows) return rc;
    HIPCHK(c, hipMemcpyAsync(out, d_rows, *n_out * sizeof(fa_query_row), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    query_read_time(c->query);
    return FA_OK;
}

extern "C" int fa_raw_query_rows_device(fa_ctx* c, uint32_t group, int order, size_t k, const void** d_rows, size_t* n_out) {
    LOAD_ENTER(c);
    if (!d_rows) return fail(c, FA_ERR_ARG, "fa_raw_query_rows_device: null argument");
    *d_rows = nullptr;
    int rc = query_rows(c, "fa_raw_query_rows_device", group, order, k, 0, false, d_rows, n_out);
    if (rc || !*d_rows) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    query_read_time(c->query);
    return FA_OK;
}

extern "C" int fa_raw_query_reset(fa_ctx* c) {
    LOAD_ENTER(c);
    QueryState* q = c->query;
    if (!q) return FA_OK;
    q->groups = 0;
    return q->tabs ? tab_reset(c, *q->tabs) : FA_OK;
}

// ---- another ctx's rows into the result held ----------------------------------------------------------------------------------------
// n rows of ONE kind in HBM: every row is checked (raw_query_rows_check_kernel, one status word, one wait) before the first is added;
// then launches of at most the tables' chunk, room for that many keys reserved in table kind & 1 before each (the fold's rule).
extern "C" int fa_raw_query_merge_device(fa_ctx* c, uint32_t group, const void* d_rows, size_t n) {
    LOAD_ENTER(c);
    static const char fn[] = "fa_raw_query_merge_device";
    if (!d_rows && n) return fail(c, FA_ERR_ARG, std::string(fn) + ": null argument");
    QueryState* q = c->query;
    if (!q || !q->tabs || !q->groups) return fail(c, FA_ERR_ARG, std::string(fn) + ": the ctx holds no query result (start one with any query, such as fa_raw_query_pending over an empty range)");
    if (!group || (group & (group - 1)) || !(q->groups & group)) return fail(c, FA_ERR_ARG, std::string(fn) + ": group is exactly one bit of the groups of the result held");
    if ((uintptr_t)d_rows & 7) return fail(c, FA_ERR_ARG, std::string(fn) + ": the rows are 8-byte aligned");
    if (n >= (1ull << 31)) return fail(c, FA_ERR_ARG, std::string(fn) + ": too many rows for one call (2^31)");
    if (!n) return FA_OK;
    QueryTabs& t = *q->tabs;
    if (inside(q->rows, d_rows) || inside(q->top, d_rows)) return fail(c, FA_ERR_ARG, std::string(fn) + ": the rows are this ctx's own result (a result is not merged into itself)");
    const uint32_t kind = (uint32_t)__builtin_ctz(group);
    const int d = (int)(kind & 1u);
    HIPCHK(c, zero_word(t.cursor.get(), c->stream));
    hipLaunchKernelGGL(raw_query_rows_check_kernel, grid_n(n), dim3(256), 0, c->stream, (const TalkRow*)d_rows, (uint64_t)n, kind, t.cursor.get());
    HIPCHK(c, hipGetLastError());
    q->merge_launches++;
    unsigned int bad = 0;
    HIPCHK(c, read_word(t.cursor.get(), bad, c->stream));
    if (bad)
        return fail(c, FA_ERR_ARG, std::string(fn) + ": a row is no row of this kind (address kinds: canonical key, value 0; scalar kinds: zero key and etype; MINUTE: value % 60 == 0; TOTAL: value 0); nothing was added");
    const size_t chunk = std::max<size_t>(1, t.chunk);
    for (size_t i = 0; i < n;) {
        const size_t m = std::min(n - i, chunk);
        int rc = tab_reserve(c, t, d, m);
        if (rc) return rc;
        RawQueryMergeArgs a{(const TalkRow*)d_rows + i, (uint32_t)m, kind, t.tab[d].get(), t.mask(d), t.d_ctr.get()};
        // (timed and counted with the fold launches: fa_raw_query_stats' launches and fold_ns)
        rc = tab_fold_launch(c, t, m, [&](dim3 grid) { hipLaunchKernelGGL(raw_query_merge_kernel, grid, dim3(QueryTab::BLOCK), 0, c->stream, a); });
        if (rc) return rc;
        t.used_ub[d] += m;
        i += m;
    }
    TalkCounters h;
    int rc = tab_settle(c, t, h);  // (the caller's rows are not referenced after the call)
    if (rc) return rc;
    q->mst.merge_calls++, q->mst.rows_merged += n;
    return FA_OK;
}
extern "C" int fa_raw_query_merge_rows(fa_ctx* c, uint32_t group, const fa_query_row* rows, size_t n) {
    LOAD_ENTER(c);
    if (!rows && n) return fail(c, FA_ERR_ARG, "fa_raw_query_merge_rows: null argument");
    if (!n) return fa_raw_query_merge_device(c, group, nullptr, 0);  // (the refusals of the state and the group bit)
    DevBuf<TalkRow> d;
    if (!d.grow(n * sizeof(TalkRow))) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "fa_raw_query_merge_rows: hipMalloc failed; nothing was added");
    }
    HIPCHK(c, hipMemcpyAsync(d.get(), rows, n * sizeof(TalkRow), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's rows are not referenced after the call)
    return fa_raw_query_merge_device(c, group, d.get(), n);
}
extern "C" int fa_raw_query_merge_stats(fa_ctx* c, fa_raw_query_merge_stats_t* out) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (!out) return fail(c, FA_ERR_ARG, "fa_raw_query_merge_stats: null argument");
    memset(out, 0, sizeof *out);
    if (c->query) *out = c->query->mst;
    return FA_OK;
}

extern "C" int fa_raw_query_stats(fa_ctx* c, fa_raw_query_stats_t* out) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (!out) return fail(c, FA_ERR_ARG, "fa_raw_query_stats: null argument");
    memset(out, 0, sizeof *out);
    QueryState* q = c->query;
    if (!q) return FA_OK;
    *out = q->st;
    out->rows_matched = q->matched0, out->absorbed = q->absorbed0, out->grows = q->grows0, out->fold_ns = q->fold_ns0;
    out->launches += q->launches0 + q->merge_launches;
    if (q->tabs) {
        if (c->sticky) return c->sticky;
        TalkCounters h;
        int rc = tab_settle(c, *q->tabs, h);
        if (rc) return rc;
        out->rows_matched += h.folded, out->absorbed += h.absorbed, out->groups = h.used[0] + h.used[1];
        out->grows += q->tabs->grows, out->launches += q->tabs->fold_launches + q->tabs->grows, out->fold_ns += q->tabs->fold_ns_total;
    }
    return FA_OK;
}
