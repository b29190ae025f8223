// sketch_fold_host.inc - the address sketches and the distinct-address sets from columns and from parts (included by flowagg.hip
// behind rollup_host.inc: one translation unit; device side: sketch_fold.cuh; what a call may ask for and how long a chunk may be:
// sketch_plan.h; the contract: include/flowagg.h "the sketches from columns and from parts").
//
// sketch_fold_cols is ONE launch of sketch_fold_kernel on the ctx stream - and nowhere else: cms_agg_kernel owns copy 0 of a sketch
// with plain read-modify-writes for its duration, and stream order is what keeps the two apart (the argument at the head of
// rollup_host.inc).  Behind the launch it does what ingest_device_records does behind its own: exact mode - the replica copies
// may hold counts (cms_dirty) and the merged view is stale; candidates mode - the merged view is stale and the batch's boundary
// is queued (cand_boundary, ingest_host.inc: the same three launches an ingest launch ends in).  A chunk IS a batch of the
// candidates contract.  The kernel parks nothing and opens no table row: no launch guard, no counter snapshot.
// fa_stats.records_ok / records_bad / bytes_in / batches / kernel_launches, hot_epoch, par and cms_par are not touched: they
// describe wire records and the ingest's own double buffers.

struct SketchFoldState {
    DevBuf<unsigned long long> d_bad;  // records with status != 0 the fold launches skipped, so far
    Events ev;                         // two per launch: around the kernel
    uint32_t wgpc = SKETCH_WGPC, grid_forced = 0, lds = 1;  // env FA_SKETCH_WGPC, FA_SKETCH_GRID (tests: a small grid), FA_SKETCH_LDS (0: no cache)
    uint64_t calls = 0, records_in = 0, records_bad = 0, batches = 0, launches = 0, fold_ns = 0;
};
static constexpr size_t SKETCH_EV_MAX = 2 * 256;  // launches whose times are pending before the stream is waited for

static int sketch_fold_state(fa_ctx* c, SketchFoldState** out) {
    if (!c->sketch_fold) {
        std::unique_ptr<SketchFoldState> s(new SketchFoldState());
        if (!s->d_bad.grow(sizeof(unsigned long long))) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "hipMalloc(sketch fold counter) failed");
        }
        HIPCHK(c, hipMemsetAsync(s->d_bad, 0, sizeof(unsigned long long), c->stream));
        if (const char* d = getenv("FA_SKETCH_WGPC")) s->wgpc = (uint32_t)std::min(8, std::max(1, atoi(d)));
        if (const char* d = getenv("FA_SKETCH_GRID")) s->grid_forced = (uint32_t)std::min<long>(ROLLUP_MAX_GRID, std::max<long>(0, atol(d)));
        if (const char* d = getenv("FA_SKETCH_LDS")) s->lds = atoi(d) != 0 ? 1u : 0u;
        c->sketch_fold = s.release();
    }
    *out = c->sketch_fold;
    return FA_OK;
}
// the launches' events (the stream was waited for): their times are added, the pool is free again
static void sketch_fold_read_events(SketchFoldState* s) {
    for (size_t i = 0; i + 1 < s->ev.used(); i += 2) Events::elapsed_ns(s->ev[i], s->ev[i + 1], &s->fold_ns);
    s->ev.rewind();
}

// m records (at most sketch_chunk_cap) of `cols` into the sketches `sets` (checked: sketch_mask_check) and their distinct-address sets
static int sketch_fold_cols(fa_ctx* c, const fa_columns& cols, size_t m, uint32_t sets) {
    SketchFoldState* s = nullptr;
    int rc = sketch_fold_state(c, &s);
    if (rc) return rc;
    if (s->ev.used() + 2 > SKETCH_EV_MAX) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        sketch_fold_read_events(s);
    }
    const hipEvent_t* e = s->ev.take(2);
    if (!e) return events_failed(c);
    KArgs a = make_args(c);
    a.key_sets = sets;
    SketchCols sc{};
    sc.bytes = cols.bytes, sc.sampling_rate = cols.sampling_rate;
    sc.addr[0] = (const uint4*)cols.src_addr, sc.addr[1] = (const uint4*)cols.dst_addr;
    sc.status = cols.status;
    sc.m = (uint32_t)m;
    sc.dirs = ((sets & FA_KEYS_SRCADDR_CMS) ? SKETCH_DIR_SRC : 0u) | ((sets & FA_KEYS_DSTADDR_CMS) ? SKETCH_DIR_DST : 0u);
    sc.lds = s->lds;
    sc.bad = s->d_bad;
    // persistent grid: wgpc workgroups per CU, never more than the chunk has 256-record runs
    const uint32_t want = s->grid_forced ? s->grid_forced : (uint32_t)c->num_cus * s->wgpc;
    const dim3 grid(std::max<uint32_t>(1u, std::min<uint32_t>(std::min(want, ROLLUP_MAX_GRID), (uint32_t)((m + ROLLUP_BLOCK - 1) / ROLLUP_BLOCK))));
    (void)hipEventRecord(e[0], c->stream);
    hipLaunchKernelGGL(sketch_fold_kernel, grid, dim3(ROLLUP_BLOCK), 0, c->stream, a, sc);
    (void)hipEventRecord(e[1], c->stream);
    HIPCHK(c, hipGetLastError());
    s->launches++;
    s->batches++;
    s->records_in += m;
    // (what ingest_device_records does behind its launch)
    c->cms_dirty = c->cms_dirty || c->cand_state == nullptr;  // (candidates mode: every path adds to copy 0 - nothing to fold)
    c->merged_valid = false;
    return c->cand_state ? cand_boundary(c) : FA_OK;
}

// the end of both doors, behind a settle (the replica copies are folded, the stream has drained): the launches' times and the skipped records
static int sketch_fold_finish(fa_ctx* c) {
    SketchFoldState* s = c->sketch_fold;
    if (!s) return FA_OK;
    sketch_fold_read_events(s);
    unsigned long long bad = 0;
    HIPCHK(c, hipMemcpy(&bad, s->d_bad, sizeof bad, hipMemcpyDeviceToHost));
    s->records_bad = bad;
    return FA_OK;
}

extern "C" int fa_sketch_fold_columns_device(fa_ctx* c, const fa_columns* cols, size_t n, uint32_t key_sets) {
    LOAD_ENTER(c);
    uint32_t sets = 0;
    int rc = sketch_mask_check(c->cfg.key_sets, key_sets, &sets);
    if (rc == FA_ERR_UNSUPPORTED) return fail(c, rc, "fa_sketch_fold_columns_device: the ctx was created without a sketch (FA_KEYS_SRCADDR_CMS / FA_KEYS_DSTADDR_CMS): nothing to fold into");
    if (rc) return fail(c, rc, "fa_sketch_fold_columns_device: key_sets names something that is not a sketch this ctx was created with");
    if (n == 0) return FA_OK;
    if (!cols) return fail(c, FA_ERR_ARG, "fa_sketch_fold_columns_device: null argument");
    // the columns the fold reads (sketch_fold.cuh) must be there; whatever is there must be naturally aligned
    bool ok = cols->status && cols->bytes && cols->sampling_rate && (!(sets & FA_KEYS_SRCADDR_CMS) || cols->src_addr) && (!(sets & FA_KEYS_DSTADDR_CMS) || cols->dst_addr);
    const void* p8[] = {cols->time_received, cols->time_flow_start, cols->sampling_rate, cols->bytes, cols->packets};
    const void* p4[] = {cols->sequence_num, cols->src_as, cols->dst_as, cols->etype, cols->proto, cols->src_port, cols->dst_port};
    const void* p16[] = {cols->sampler_address, cols->src_addr, cols->dst_addr};
    for (const void* p : p8) ok = ok && !((uintptr_t)p & 7);
    for (const void* p : p4) ok = ok && !((uintptr_t)p & 3);
    for (const void* p : p16) ok = ok && !((uintptr_t)p & 15);
    if (!ok)
        return fail(c, FA_ERR_ARG, "fa_sketch_fold_columns_device: status, bytes, sampling_rate and the address column of every selected sketch are needed, each naturally aligned (8 / 4 / 16 / 1 bytes)");
    const size_t cap = sketch_chunk_cap(c->cfg.max_batch_records);
    for (size_t i = 0; i < n;) {
        const size_t m = std::min(n - i, cap);
        rc = sketch_fold_cols(c, cols_from(*cols, i), m, sets);
        if (rc) return rc;
        i += m;
    }
    rc = settle(c);
    if (rc == FA_OK) rc = sketch_fold_finish(c);
    if (rc) return rc;
    c->sketch_fold->calls++;
    return FA_OK;
}

// ---- the restore's two halves, shared with the ranged door (raw_range_host.inc) -----------------------------------------------------
struct RestoreSel {
    uint32_t ks = 0, sets = 0;  // the exact key sets and the sketches selected
    bool talk = false, ports = false;
};
// rows [r_lo, r_hi) of a part
struct LoadSlice {
    LoadPart part;
    uint64_t r_lo, r_hi;
};
// what key_sets / folds select on this ctx: the mask refusals, FA_ERR_UNSUPPORTED when nothing is selected
static int restore_select(fa_ctx* c, const char* fn, uint32_t key_sets, int folds, RestoreSel* sel) {
    int rc = restore_mask_check(c->cfg.key_sets, key_sets, &sel->ks, &sel->sets);
    if (rc) {
        c->err = std::string(fn) + ": key_sets names a key set the ctx was not created with";
        return rc;
    }
    sel->talk = folds && c->talk, sel->ports = folds && c->ports;
    if (!sel->ks && !sel->sets && !sel->talk && !sel->ports) {
        c->err = std::string(fn) + ": nothing is selected to fold into (no key set of the ctx, and no enabled talker or port fold asked for)";
        return FA_ERR_UNSUPPORTED;
    }
    return FA_OK;
}
// every slice, in order, unpacked a chunk at a time and folded into everything selected; then the settle and the folds' ends
static int restore_fold_slices(fa_ctx* c, LoadState* s, const std::vector<LoadSlice>& slices, const RestoreSel& sel) {
    const uint32_t ks = sel.ks, sets = sel.sets;
    const bool talk = sel.talk, ports = sel.ports;
    int rc = FA_OK;
    const size_t cap = restore_chunk_cap(ks ? rollup_chunk(c, ks) : 0, sets ? sketch_chunk_cap(c->cfg.max_batch_records) : 0, talk ? talk_chunk_cap(c) : 0, ports ? port_chunk_cap(c) : 0);
    for (const LoadSlice& sl : slices)
        for (uint64_t r0 = sl.r_lo; r0 < sl.r_hi;) {  // (chunks end at part boundaries)
            const size_t m = (size_t)std::min<uint64_t>(sl.r_hi - r0, cap);
            rc = load_chunk(c, s, sl.part, r0, m, [&](const fa_columns& cols, size_t m) {
                int frc = ks ? rollup_fold_cols(c, cols, m, ks) : FA_OK;
                if (frc == FA_OK && sets) frc = sketch_fold_cols(c, cols, m, sets);
                if (frc == FA_OK && (talk || ports)) frc = fold_chunk_cols(c, cols, m);
                return frc;
            });
            if (rc) return rc;
            r0 += m;
        }
    rc = ks ? rollup_finish(c) : settle(c);
    load_read_events(s);  // (settle has waited for the stream)
    if (rc == FA_OK && sets) rc = sketch_fold_finish(c);
    if (rc) return rc;
    if (ks) {
        RollupState* r = nullptr;
        rc = rollup_state(c, &r);
        if (rc) return rc;
        r->calls++;
    }
    if (sets) {
        SketchFoldState* f = nullptr;
        rc = sketch_fold_state(c, &f);
        if (rc) return rc;
        f->calls++;
    }
    return FA_OK;
}

extern "C" int fa_raw_restore(fa_ctx* c, const uint8_t* bytes, size_t n, uint32_t key_sets, int folds) {
    LOAD_ENTER(c);
    RestoreSel sel;
    int rc = restore_select(c, "fa_raw_restore", key_sets, folds, &sel);
    if (rc) return rc;
    if (!bytes && n) return fail(c, FA_ERR_ARG, "fa_raw_restore: null argument");
    LoadState* s = nullptr;
    rc = load_state(c, &s);
    if (rc) return rc;
    LoadPrepared pr;
    rc = load_prepare(c, s, "fa_raw_restore", bytes, n, true, pr);
    if (rc) return rc;
    // (from here on the input is known to be whole: a refused call has folded nothing)
    std::vector<LoadSlice> slices;
    for (const LoadPart& p : pr.parts) slices.push_back({p, 0, p.rows});
    return restore_fold_slices(c, s, slices, sel);
}

extern "C" int fa_sketch_fold_stats(fa_ctx* c, fa_sketch_fold_stats_t* out) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (!out) return fail(c, FA_ERR_ARG, "fa_sketch_fold_stats: null argument");
    memset(out, 0, sizeof *out);
    const SketchFoldState* s = c->sketch_fold;
    if (!s) return FA_OK;
    out->calls = s->calls, out->records_in = s->records_in, out->records_bad = s->records_bad;
    out->records_folded = s->records_in - s->records_bad;
    out->batches = s->batches, out->launches = s->launches, out->fold_ns = s->fold_ns;
    return FA_OK;
}
