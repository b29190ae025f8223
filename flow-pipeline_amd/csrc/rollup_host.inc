// rollup_host.inc - the rollups from columns and from parts (included by flowagg.hip behind raw_load_host.inc: one translation unit;
// device side: rollup.cuh; what a call may ask for and how long a chunk may be: rollup_plan.h; the contract: include/flowagg.h
// "the rollups from columns and from parts").
//
// rollup_fold_cols is ONE launch of rollup_fold_kernel on the ctx stream - and nowhere else: a compact-tuple launch of the ingest
// owns table regions with plain stores for the duration of its aggregation kernel, and stream order is what keeps the two apart.
// The launch is bracketed like an ingest launch (pre_launch_guard / post_launch_snapshot: parked updates fit the spill buffers,
// the host sees the counters without waiting), and by wlog_make_room when the wide table takes rows.  Both doors end in settle():
// growth and spill replay have happened when they return.

struct RollupState {
    DevBuf<unsigned long long> d_bad;  // records with status != 0 the fold launches skipped, so far
    Events ev;                         // two per launch: around the kernel
    uint32_t wgpc = ROLLUP_WGPC, grid_forced = 0;  // env FA_ROLLUP_WGPC, FA_ROLLUP_GRID (tests: a small grid)
    uint64_t calls = 0, records_in = 0, records_bad = 0, launches = 0, fold_ns = 0;
};
static constexpr size_t ROLLUP_EV_MAX = 2 * 256;  // launches whose times are pending before the stream is waited for

static int rollup_state(fa_ctx* c, RollupState** out) {
    if (!c->rollup) {
        std::unique_ptr<RollupState> s(new RollupState());
        if (!s->d_bad.grow(sizeof(unsigned long long))) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "hipMalloc(rollup counter) failed");
        }
        HIPCHK(c, hipMemsetAsync(s->d_bad, 0, sizeof(unsigned long long), c->stream));
        if (const char* d = getenv("FA_ROLLUP_WGPC")) s->wgpc = (uint32_t)std::min(8, std::max(1, atoi(d)));
        if (const char* d = getenv("FA_ROLLUP_GRID")) s->grid_forced = (uint32_t)std::min<long>(ROLLUP_MAX_GRID, std::max<long>(0, atol(d)));
        c->rollup = s.release();
    }
    *out = c->rollup;
    return FA_OK;
}
// the launches' events (the stream was waited for): their times are added, the pool is free again
static void rollup_read_events(RollupState* s) {
    for (size_t i = 0; i + 1 < s->ev.used(); i += 2) Events::elapsed_ns(s->ev[i], s->ev[i + 1], &s->fold_ns);
    s->ev.rewind();
}

static size_t rollup_chunk(const fa_ctx* c, uint32_t ks) { return rollup_chunk_cap(c->spill_cap, c->wspill_cap, c->cfg.max_batch_records, ks); }

// m records (at most rollup_chunk(c, ks)) of `cols` into the key sets `ks` (checked: rollup_mask_check)
static int rollup_fold_cols(fa_ctx* c, const fa_columns& cols, size_t m, uint32_t ks) {
    RollupState* s = nullptr;
    int rc = rollup_state(c, &s);
    if (rc) return rc;
    rc = pre_launch_guard(c, m);
    if (rc) return rc;
    const uint64_t wide_rows = (uint64_t)m * rollup_wide_updates(ks);  // rows this launch may open in the wide table
    if (wide_rows && c->wtab) {
        rc = wlog_make_room(c, wide_rows);
        if (rc) return rc;
    }
    if (s->ev.used() + 2 > ROLLUP_EV_MAX) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        rollup_read_events(s);
    }
    const hipEvent_t* e = s->ev.take(2);
    if (!e) return events_failed(c);
    KArgs a = make_args(c);  // (behind the guard and the room: either may have settled and moved a table)
    a.key_sets = ks;
    RollupCols rcols{};
    rcols.time_received = cols.time_received, rcols.time_flow_start = cols.time_flow_start, rcols.sampling_rate = cols.sampling_rate;
    rcols.bytes = cols.bytes, rcols.packets = cols.packets;
    rcols.src_as = cols.src_as, rcols.dst_as = cols.dst_as, rcols.etype = cols.etype, rcols.proto = cols.proto;
    rcols.src_port = cols.src_port, rcols.dst_port = cols.dst_port;
    rcols.src_addr = (const uint4*)cols.src_addr;
    rcols.status = cols.status;
    rcols.m = (uint32_t)m;
    rcols.bad = s->d_bad;
    // persistent grid: wgpc workgroups per CU, never more than the chunk has 256-record runs
    const uint32_t want = s->grid_forced ? s->grid_forced : (uint32_t)c->num_cus * s->wgpc;
    const dim3 grid(std::max<uint32_t>(1u, std::min<uint32_t>(std::min(want, ROLLUP_MAX_GRID), (uint32_t)((m + ROLLUP_BLOCK - 1) / ROLLUP_BLOCK))));
    (void)hipEventRecord(e[0], c->stream);
    if (ks == FA_KEYS_AS_PAIR) hipLaunchKernelGGL(rollup_fold_kernel<FA_KEYS_AS_PAIR>, grid, dim3(ROLLUP_BLOCK), 0, c->stream, a, rcols);
    else hipLaunchKernelGGL(rollup_fold_kernel<KS_ALL>, grid, dim3(ROLLUP_BLOCK), 0, c->stream, a, rcols);
    (void)hipEventRecord(e[1], c->stream);
    HIPCHK(c, hipGetLastError());
    if (c->wtab) c->wpot_total += wide_rows;  // (wide_rows_bound)
    s->launches++;
    s->records_in += m;
    return post_launch_snapshot(c, m);
}

// the end of both doors: settle (growth, spill replay, fa_last_error), then the launches' times and the skipped records
static int rollup_finish(fa_ctx* c) {
    int rc = settle(c);
    if (rc) return rc;
    RollupState* s = c->rollup;
    if (!s) return FA_OK;
    rollup_read_events(s);
    unsigned long long bad = 0;
    HIPCHK(c, hipMemcpy(&bad, s->d_bad, sizeof bad, hipMemcpyDeviceToHost));
    s->records_bad = bad;
    return FA_OK;
}

static int rollup_mask(fa_ctx* c, const char* fn, uint32_t asked, uint32_t* ks) {
    const int rc = rollup_mask_check(c->cfg.key_sets, asked, ks);
    if (rc == FA_ERR_UNSUPPORTED) {
        c->err = std::string(fn) + ((asked & ROLLUP_SKETCH_SETS) ? ": this door does not feed the sketches and the distinct-address sets - they are fed from wire bytes only here; from columns and parts by fa_sketch_fold_columns_device / fa_raw_restore" :
                                                                   ": the ctx was created without an exact key set: nothing to fold into");
    } else if (rc) {
        c->err = std::string(fn) + ": key_sets names a key set the ctx was not created with";
    }
    return rc;
}

static fa_columns cols_from(const fa_columns& k, size_t i) {
    fa_columns o = k;
    auto step = [&](auto& p, size_t width) {
        if (p) p = (decltype(+p))((const uint8_t*)p + i * width);
    };
    step(o.time_received, 8), step(o.time_flow_start, 8), step(o.sampling_rate, 8), step(o.bytes, 8), step(o.packets, 8);
    step(o.sequence_num, 4), step(o.src_as, 4), step(o.dst_as, 4), step(o.etype, 4), step(o.proto, 4), step(o.src_port, 4), step(o.dst_port, 4);
    step(o.sampler_address, 16), step(o.src_addr, 16), step(o.dst_addr, 16), step(o.status, 1);
    return o;
}

extern "C" int fa_rollup_fold_columns_device(fa_ctx* c, const fa_columns* cols, size_t n, uint32_t key_sets) {
    LOAD_ENTER(c);
    uint32_t ks = 0;
    int rc = rollup_mask(c, "fa_rollup_fold_columns_device", key_sets, &ks);
    if (rc) return rc;
    if (n == 0) return FA_OK;
    if (!cols) return fail(c, FA_ERR_ARG, "fa_rollup_fold_columns_device: null argument");
    // the columns the key sets read (rollup.cuh) must be there; whatever is there must be naturally aligned
    const bool as = ks & FA_KEYS_AS_PAIR, app = ks & FA_KEYS_ADDR_PORT_PROTO, port = ks & FA_KEYS_PORT_HIST, minute = ks & FA_KEYS_MINUTE_SERIES;
    bool ok = cols->status && cols->time_received && cols->bytes && (!(as || app) || cols->packets) && (!as || (cols->src_as && cols->dst_as && cols->etype)) &&
              (!(port || minute) || cols->sampling_rate) && (!app || (cols->src_addr && cols->proto)) && (!(app || port) || cols->dst_port) &&
              (!port || cols->src_port) && (!minute || cols->time_flow_start);
    const void* p8[] = {cols->time_received, cols->time_flow_start, cols->sampling_rate, cols->bytes, cols->packets};
    const void* p4[] = {cols->sequence_num, cols->src_as, cols->dst_as, cols->etype, cols->proto, cols->src_port, cols->dst_port};
    const void* p16[] = {cols->sampler_address, cols->src_addr, cols->dst_addr};
    for (const void* p : p8) ok = ok && !((uintptr_t)p & 7);
    for (const void* p : p4) ok = ok && !((uintptr_t)p & 3);
    for (const void* p : p16) ok = ok && !((uintptr_t)p & 15);
    if (!ok) return fail(c, FA_ERR_ARG, "fa_rollup_fold_columns_device: status and every column the key sets read are needed, each naturally aligned (8 / 4 / 16 / 1 bytes)");
    const size_t cap = rollup_chunk(c, ks);
    for (size_t i = 0; i < n;) {
        const size_t m = std::min(n - i, cap);
        rc = rollup_fold_cols(c, cols_from(*cols, i), m, ks);
        if (rc) return rc;
        i += m;
    }
    rc = rollup_finish(c);
    if (rc) return rc;
    c->rollup->calls++;
    return FA_OK;
}

extern "C" int fa_raw_load_rollup(fa_ctx* c, const uint8_t* bytes, size_t n, uint32_t key_sets, int folds) {
    LOAD_ENTER(c);
    uint32_t ks = 0;
    int rc = rollup_mask(c, "fa_raw_load_rollup", key_sets, &ks);
    if (rc) return rc;
    if (folds && !c->talk && !c->ports)
        return fail(c, FA_ERR_UNSUPPORTED, "fa_raw_load_rollup: folds asked for, but neither fa_talkers_enable(_buckets) nor fa_ports_enable_buckets was called on this ctx");
    if (!bytes && n) return fail(c, FA_ERR_ARG, "fa_raw_load_rollup: null argument");
    LoadState* s = nullptr;
    rc = load_state(c, &s);
    if (rc) return rc;
    LoadPrepared pr;
    rc = load_prepare(c, s, "fa_raw_load_rollup", bytes, n, true, pr);
    if (rc) return rc;
    // (from here on the input is known to be whole: a refused call has folded nothing)
    const size_t cap = rollup_chunk(c, ks);
    for (const LoadPart& p : pr.parts)
        for (uint64_t r0 = 0; r0 < p.rows;) {
            size_t m = (size_t)std::min<uint64_t>(p.rows - r0, cap);
            if (folds && c->talk) m = std::min(m, talk_chunk_cap(c));
            if (folds && c->ports) m = std::min(m, port_chunk_cap(c));
            rc = load_chunk(c, s, p, r0, m, [&](const fa_columns& cols, size_t m) {
                const int frc = rollup_fold_cols(c, cols, m, ks);
                return frc == FA_OK && folds ? fold_chunk_cols(c, cols, m) : frc;
            });
            if (rc) return rc;
            r0 += m;
        }
    rc = rollup_finish(c);
    load_read_events(s);  // (settle has waited for the stream)
    if (rc) return rc;
    RollupState* r = nullptr;
    rc = rollup_state(c, &r);
    if (rc) return rc;
    r->calls++;
    return FA_OK;
}

extern "C" int fa_rollup_stats(fa_ctx* c, fa_rollup_stats_t* out) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (!out) return fail(c, FA_ERR_ARG, "fa_rollup_stats: null argument");
    memset(out, 0, sizeof *out);
    const RollupState* s = c->rollup;
    if (!s) return FA_OK;
    out->calls = s->calls, out->records_in = s->records_in, out->records_bad = s->records_bad;
    out->records_folded = s->records_in - s->records_bad;
    out->launches = s->launches, out->fold_ns = s->fold_ns;
    return FA_OK;
}
