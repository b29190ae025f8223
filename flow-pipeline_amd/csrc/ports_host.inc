// ports_host.inc - host side of the bucketed port tables (included by flowagg.hip: one translation unit; device side: ports.cuh).
// The ONE second pass an ingest call runs for every enabled fold is second_pass.inc.
//
// Capacity rule: talkers_host.inc's, per table.  The host keeps an upper bound used_ub of the occupied slots (a chunk of m
// records adds at most m keys); before a launch, if (used_ub + m) * 2 > capacity, the stream is synchronised and the device's
// exact count replaces the bound; while the inequality still holds the table doubles (port_rehash_kernel re-inserts every
// slot).  So every launch finds its table at or below half full when it ends - the unbounded probe loops of ports.cuh end.
// 2^30 slots is the limit: FA_ERR_TABLE_FULL BEFORE the chunk is folded.
// Chunks: at most FA_TALK_CHUNK records (the one knob of the second pass, default 2^20), and at most max(2^16, capacity / 4).
static_assert(PORT_LARGE == PORT_DENSE, "the ranged collector's dense scratch is indexed like the dense port histograms");
static_assert(sizeof(PortRow) == sizeof(RowW) && sizeof(RowW) == sizeof(fa_port_row), "row layout");

struct PortState {
    DevBuf<PSlot> tab[2];
    uint32_t log2[2] = {16, 16};
    uint32_t bucket_secs = 60;
    uint64_t used_ub[2] = {0, 0};
    DevBuf<PortCounters> d_ctr;
    size_t chunk = (size_t)1 << 20;  // env FA_TALK_CHUNK
    uint32_t wgpc = PORT_WG_PER_CU;  // env FA_PORT_WGPC (A/B: workgroups per CU of the fold kernel)
    uint64_t grows = 0, fold_launches = 0, fold_ns_total = 0;
    struct Ev { hipEvent_t e0, e1; };
    std::vector<Ev> ev;  // one pair per fold launch that has not been read yet
    size_t ev_used = 0;
    DevBuf<ulonglong2> dense;  // the ranged collector's {weight, count} per port below 65536 (1 MiB)
    DevBuf<> rows;             // the ranged collector's rows on their way into the merge; fa_ports_buckets' scratch
};

static uint32_t port_bucket_secs(const fa_ctx* c) { return c->ports ? c->ports->bucket_secs : 0; }
static void port_destroy(fa_ctx* c) {
    PortState* t = c->ports;
    if (!t) return;
    for (auto& e : t->ev) {
        (void)hipEventDestroy(e.e0);
        (void)hipEventDestroy(e.e1);
    }
    delete t;
    c->ports = nullptr;
}

#define PORT_ENTER(c)                                                                                  \
    FA_ON_DEVICE(c);                                                                                   \
    if (!(c)) return FA_ERR_ARG;                                                                       \
    if ((c)->sticky) return (c)->sticky;                                                               \
    if (!(c)->ports) return fail((c), FA_ERR_UNSUPPORTED, PORT_OFF)

extern "C" int fa_ports_enable_buckets(fa_ctx* c, uint32_t capacity_log2, uint32_t bucket_secs) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (c->ports) return fail(c, FA_ERR_ARG, "fa_ports_enable_buckets: already enabled");
    if (bucket_secs == 0 || 86400u % bucket_secs) return fail(c, FA_ERR_ARG, "fa_ports_enable_buckets: bucket_secs must be >= 1 and divide 86400");
    if (capacity_log2 == 0) capacity_log2 = 16;
    if (capacity_log2 < 8 || capacity_log2 > 30) return fail(c, FA_ERR_ARG, "fa_ports_enable_buckets: capacity_log2 is 0 or 8..30");
    PortState* t = new PortState();
    t->bucket_secs = bucket_secs;
    if (const char* d = getenv("FA_TALK_CHUNK")) t->chunk = (size_t)std::min<long long>(1ll << 28, std::max<long long>(1, atoll(d)));
    if (const char* d = getenv("FA_PORT_WGPC")) t->wgpc = (uint32_t)std::min(8, std::max(1, atoi(d)));
    c->ports = t;
    bool ok = t->d_ctr.grow(sizeof(PortCounters)) && hipMemsetAsync(t->d_ctr, 0, sizeof(PortCounters), c->stream) == hipSuccess;
    ok = ok && t->dense.grow(sizeof(ulonglong2) * PORT_DENSE);
    for (int d = 0; d < 2 && ok; d++) {
        t->log2[d] = capacity_log2;
        ok = t->tab[d].grow(sizeof(PSlot) << capacity_log2) && hipMemsetAsync(t->tab[d], 0, sizeof(PSlot) << capacity_log2, c->stream) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        port_destroy(c);
        return fail(c, FA_ERR_NOMEM, "fa_ports_enable_buckets: allocating the tables failed");
    }
    return FA_OK;
}

// Waits for the stream; the device counters and the fold launches' times.
static int port_settle(fa_ctx* c, PortCounters& h) {
    PortState* t = c->ports;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&h, t->d_ctr, sizeof h, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < t->ev_used; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t->ev[i].e0, t->ev[i].e1) == hipSuccess) t->fold_ns_total += (uint64_t)((double)ms * 1e6);
    }
    t->ev_used = 0;
    if (h.lost) {
        c->sticky = FA_ERR_TABLE_FULL;
        return fail(c, FA_ERR_TABLE_FULL, "internal: a port table was full during a launch; updates were lost");
    }
    t->used_ub[0] = h.used[0];
    t->used_ub[1] = h.used[1];
    return FA_OK;
}

// Table d rebuilt into a fresh one of 2^nl slots: growth (nl = log2 + 1, everything kept) and fa_ports_drop_before (the same
// size, the slots of a bucket index below floor_index left behind).  The device's used[d] and large[d] are counted again.
// fresh: a table of 2^nl slots the caller allocated beforehand (fa_ports_drop_before allocates both before it rebuilds either).
static int port_rebuild(fa_ctx* c, int d, uint32_t nl, uint32_t floor_index, DevBuf<PSlot>* fresh = nullptr) {
    PortState* t = c->ports;
    DevBuf<PSlot> nt;
    if (fresh) nt = std::move(*fresh);
    else if (!nt.grow(sizeof(PSlot) << nl)) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "hipMalloc(port table) failed");
    }
    hipError_t e = hipMemsetAsync(nt, 0, sizeof(PSlot) << nl, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(&t->d_ctr->used[d], 0, sizeof(unsigned long long), c->stream);  // (the rehash counts every key again)
    if (e == hipSuccess) e = hipMemsetAsync(&t->d_ctr->large[d], 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) {
        const uint64_t slots = 1ull << t->log2[d];
        const unsigned g = (unsigned)std::min<uint64_t>((slots + 255) / 256, (uint64_t)c->num_cus * 8);
        hipLaunchKernelGGL(port_rehash_kernel, dim3(g), dim3(256), 0, c->stream, (const PSlot*)t->tab[d], slots, nt.get(), (uint32_t)((1ull << nl) - 1), t->d_ctr.get(), d, floor_index);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->sticky = FA_ERR_HIP;  // (the occupied-slot counters were reset: the state is no longer trustworthy)
        c->err = std::string("port table rebuild: ") + hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    t->tab[d] = std::move(nt);  // (frees the old table: the rehash has been synchronised)
    t->log2[d] = nl;
    return FA_OK;
}

// Room for m more keys in table d at a load of at most 1/2 (the capacity rule above).
static int port_reserve(fa_ctx* c, int d, uint64_t m) {
    PortState* t = c->ports;
    if ((t->used_ub[d] + m) * 2 <= (1ull << t->log2[d])) return FA_OK;
    PortCounters h;
    int rc = port_settle(c, h);
    if (rc) return rc;
    while ((t->used_ub[d] + m) * 2 > (1ull << t->log2[d])) {
        if (t->log2[d] >= 30) return fail(c, FA_ERR_TABLE_FULL, "a port table cannot grow further (2^30 slots)");
        rc = port_rebuild(c, d, t->log2[d] + 1, 0);
        if (rc) return rc;
        t->grows++;
    }
    return FA_OK;
}

static size_t port_chunk_cap(const fa_ctx* c) {
    const PortState* t = c->ports;
    const uint64_t cap = 1ull << std::min(t->log2[0], t->log2[1]);
    return (size_t)std::min<uint64_t>(t->chunk, std::max<uint64_t>(1ull << 16, cap / 4));
}

struct PortCols {
    const void *src_port, *dst_port, *bytes, *sampling_rate, *time_flow_start, *status;
};

static int port_fold_cols(fa_ctx* c, const PortCols& p, size_t n) {
    PortState* t = c->ports;
    for (size_t i = 0; i < n;) {
        const size_t m = std::min(n - i, port_chunk_cap(c));
        for (int d = 0; d < 2; d++) {
            int rc = port_reserve(c, d, m);
            if (rc) return rc;
        }
        if (t->ev_used == t->ev.size()) {
            if (t->ev.size() >= 1024) {  // bound the pool: read what is pending
                PortCounters h;
                int rc = port_settle(c, h);
                if (rc) return rc;  // (the exact counts replaced the bounds: no larger, so the room reserved above still holds)
            } else {
                PortState::Ev e{};
                HIPCHK(c, hipEventCreate(&e.e0));
                if (hipEventCreate(&e.e1) != hipSuccess) {
                    (void)hipEventDestroy(e.e0);
                    return fail(c, FA_ERR_HIP, "hipEventCreate failed");
                }
                t->ev.push_back(e);
            }
        }
        PortFoldArgs a{};
        a.src_port = (const uint32_t*)p.src_port + i;
        a.dst_port = (const uint32_t*)p.dst_port + i;
        a.bytes = (const uint64_t*)p.bytes + i;
        a.sampling_rate = (const uint64_t*)p.sampling_rate + i;
        a.time_flow_start = (const uint64_t*)p.time_flow_start + i;
        a.status = (const uint8_t*)p.status + i;
        a.n = (uint32_t)m;
        a.bucket_secs = t->bucket_secs;
        for (int d = 0; d < 2; d++) {
            a.tab[d] = t->tab[d];
            a.mask[d] = (uint32_t)((1ull << t->log2[d]) - 1);
        }
        a.ctr = t->d_ctr;
        // persistent grid: the workgroups that are co-resident, records grid-strided
        const uint32_t grid = (uint32_t)std::max<size_t>(1, std::min<size_t>((m + PORT_BLOCK - 1) / PORT_BLOCK, (size_t)c->num_cus * t->wgpc));
        PortState::Ev& ev = t->ev[t->ev_used++];
        (void)hipEventRecord(ev.e0, c->stream);
        hipLaunchKernelGGL(port_fold_kernel, dim3(grid), dim3(PORT_BLOCK), 0, c->stream, a);
        (void)hipEventRecord(ev.e1, c->stream);
        HIPCHK(c, hipGetLastError());
        t->fold_launches++;
        t->used_ub[0] += m;
        t->used_ub[1] += m;
        i += m;
    }
    return FA_OK;
}

extern "C" int fa_ports_fold_columns_device(fa_ctx* c, const fa_columns* cols, size_t n) {
    PORT_ENTER(c);
    if (n == 0) return FA_OK;
    if (!cols || !cols->src_port || !cols->dst_port || !cols->bytes || !cols->sampling_rate || !cols->status || !cols->time_flow_start)
        return fail(c, FA_ERR_ARG, "fa_ports_fold_columns_device: src_port, dst_port, bytes, sampling_rate, status and time_flow_start are needed");
    if ((((uintptr_t)cols->src_port | (uintptr_t)cols->dst_port) & 3) || (((uintptr_t)cols->bytes | (uintptr_t)cols->sampling_rate | (uintptr_t)cols->time_flow_start) & 7))
        return fail(c, FA_ERR_ARG, "fa_ports_fold_columns_device: the columns must be naturally aligned");
    const PortCols p{cols->src_port, cols->dst_port, cols->bytes, cols->sampling_rate, cols->time_flow_start, cols->status};
    return port_fold_cols(c, p, n);
}

// ---- ranged reads ----------------------------------------------------------------------------------------------------------
// The ranged collector of the port kinds (rows_host.inc, rows_local): the slots of the range are folded over their buckets on the
// way out - ports below 65536 in a zeroed dense scratch, the others as raw rows - and the occupied dense entries are appended
// behind the raw rows by collect_w's own port_dense_rows_kernel (one cursor for both).  The merge behind it folds the raw rows of
// equal port and orders the result; its input is at most 65536 rows plus the large-port rows.
static int collect_ports_range(fa_ctx* c, ReadClock& clk, int kind, const BucketRange& range, const void*& in, size_t& n) {
    PortState* t = c->ports;
    const int d = kind == RK_PORT_DST;
    PortCounters h;
    int rc = port_settle(c, h);
    if (rc) return rc;
    clk.mark("settle");
    if (h.large[d] >= (1ull << 31)) return fail(c, FA_ERR_ARG, "too many rows");
    const size_t cap_raw = (size_t)h.large[d];
    rc = ensure_dev(c, t->rows, (cap_raw + PORT_DENSE) * sizeof(PortRow), "port rows");
    if (rc) return rc;
    in = t->rows;
    n = 0;
    if (!h.used[d] || range.empty) return FA_OK;
    unsigned int* cursor = &c->d_ctr->rows_count;
    HIPCHK(c, zero_word(cursor, c->stream));
    HIPCHK(c, hipMemsetAsync(t->dense, 0, sizeof(ulonglong2) * PORT_DENSE, c->stream));
    const uint64_t slots = 1ull << t->log2[d];
    const unsigned grid = (unsigned)std::min<uint64_t>((slots + 255) / 256, (uint64_t)c->num_cus * 8);
    hipLaunchKernelGGL(port_range_fold_kernel, dim3(grid), dim3(256), 0, c->stream, (const PSlot*)t->tab[d], slots, range.index_lo, range.index_last, t->dense.get(),
                       (PortRow*)t->rows.get(), (uint32_t)cap_raw, cursor, t->d_ctr.get());
    hipLaunchKernelGGL(port_dense_rows_kernel, dim3(64), dim3(256), 0, c->stream, (const ulonglong2*)t->dense, (uint32_t)PORT_DENSE, (RowW*)t->rows.get(), cursor);
    HIPCHK(c, hipGetLastError());
    unsigned int got = 0;
    unsigned long long lost = 0;
    HIPCHK(c, hipMemcpyAsync(&lost, &t->d_ctr->lost, sizeof lost, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, read_word(cursor, got, c->stream));
    if (lost || got > cap_raw + PORT_DENSE) return fail(c, FA_ERR_HIP, "internal: the port table's large-port rows and their count differ");
    n = got;
    return FA_OK;
}

// Both ranged reads are fa_top_ports' read with another collector: RowOps<RK_PORT_SRC> sums the rows of equal port and leaves
// fa_top_ports' order (weight DESC, port), cut at k.
extern "C" int fa_top_ports_range(fa_ctx* c, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_port_row* out, size_t cap, size_t* n_out) {
    PORT_ENTER(c);
    if ((dst != 0 && dst != 1) || !n_out || (!out && cap)) return fail(c, FA_ERR_ARG, "fa_top_ports_range: bad argument");
    BucketRange r;
    int rc = talk_range_of(c, c->ports->bucket_secs, t_lo, t_hi, r);
    if (rc) return rc;
    return rows_read(c, dst ? RK_PORT_DST : RK_PORT_SRC, 0, k, out, cap, n_out, &r);
}
extern "C" int fa_ports_range_rows_device(fa_ctx* c, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, const void** d_rows, size_t* n_out) {
    PORT_ENTER(c);
    if ((dst != 0 && dst != 1) || !n_out || !d_rows) return fail(c, FA_ERR_ARG, "fa_ports_range_rows_device: bad argument");
    BucketRange r;
    int rc = talk_range_of(c, c->ports->bucket_secs, t_lo, t_hi, r);
    if (rc) return rc;
    const int kind = dst ? RK_PORT_DST : RK_PORT_SRC;
    ReadClock clk(c);
    rc = rows_local(c, clk, kind, 0, k, d_rows, n_out, false, nullptr, &r);
    if (rc) return rc;
    clk.done(row_kind_name(kind), clk.n_in, *n_out);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FA_OK;
}

// ---- buckets held, retention, reset, statistics --------------------------------------------------------------------------------
extern "C" int fa_ports_buckets(fa_ctx* c, uint32_t* out, size_t cap, size_t* n_out) {
    PORT_ENTER(c);
    if (!n_out || (!out && cap)) return fail(c, FA_ERR_ARG, "fa_ports_buckets: bad argument");
    PortState* t = c->ports;
    PortCounters h;
    int rc = port_settle(c, h);
    if (rc) return rc;
    auto grid = [&](int d) { return dim3((unsigned)std::min<uint64_t>(((1ull << t->log2[d]) + 255) / 256, (uint64_t)c->num_cus * 8)); };
    return bucket_starts(
        c, t->bucket_secs, (size_t)(h.used[0] + h.used[1]), t->rows,
        [&](uint32_t lo, uint32_t nbits, unsigned int* bits, unsigned int* range) {
            for (int d = 0; d < 2; d++) hipLaunchKernelGGL(port_buckets_kernel, grid(d), dim3(256), 0, c->stream, (const PSlot*)t->tab[d], 1ull << t->log2[d], lo, nbits, bits, range);
        },
        [&](uint32_t* list, uint32_t list_cap, unsigned int* cursor) {
            for (int d = 0; d < 2; d++) hipLaunchKernelGGL(port_bucket_list_kernel, grid(d), dim3(256), 0, c->stream, (const PSlot*)t->tab[d], 1ull << t->log2[d], list, list_cap, cursor);
        },
        out, cap, n_out);
}

// Removes every bucket that starts below t: fa_talkers_drop_before's contract.  The slots are write-once, so each table is rebuilt
// into a fresh one of the same size without those slots; both fresh tables are allocated before either table is touched.  No
// floor is kept: a record that arrives later with a time below t opens its bucket again.
extern "C" int fa_ports_drop_before(fa_ctx* c, uint32_t t_floor) {
    PORT_ENTER(c);
    PortState* t = c->ports;
    if (t_floor % t->bucket_secs) return fail(c, FA_ERR_ARG, "fa_ports_drop_before: t lies on the bucket grid");
    PortCounters h;
    int rc = port_settle(c, h);
    if (rc) return rc;
    if (t_floor == 0) return FA_OK;
    DevBuf<PSlot> fresh[2];  // both before either table is touched: without memory nothing is dropped, in neither table
    for (int d = 0; d < 2; d++)
        if (!fresh[d].grow(sizeof(PSlot) << t->log2[d])) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "fa_ports_drop_before: hipMalloc(port table) failed; nothing was dropped");
        }
    for (int d = 0; d < 2; d++) {
        rc = port_rebuild(c, d, t->log2[d], t_floor / t->bucket_secs, &fresh[d]);
        if (rc) return rc;  // (a failing launch or synchronisation: sticky)
    }
    return port_settle(c, h);
}

// Empties both tables (they keep their size); the counters of fa_ports_stats go on counting.
extern "C" int fa_ports_reset(fa_ctx* c) {
    PORT_ENTER(c);
    PortState* t = c->ports;
    PortCounters h;
    int rc = port_settle(c, h);
    if (rc) return rc;
    for (int d = 0; d < 2; d++) HIPCHK(c, hipMemsetAsync(t->tab[d], 0, sizeof(PSlot) << t->log2[d], c->stream));
    HIPCHK(c, hipMemsetAsync(&t->d_ctr->used[0], 0, 4 * sizeof(unsigned long long), c->stream));  // used[2], large[2]
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t->used_ub[0] = t->used_ub[1] = 0;
    return FA_OK;
}

extern "C" int fa_ports_stats(fa_ctx* c, fa_ports_stats_t* out) {
    PORT_ENTER(c);
    if (!out) return fail(c, FA_ERR_ARG, "fa_ports_stats: null argument");
    PortState* t = c->ports;
    PortCounters h;
    int rc = port_settle(c, h);
    if (rc) return rc;
    for (int d = 0; d < 2; d++) {
        out->used[d] = h.used[d];
        out->capacity[d] = 1ull << t->log2[d];
    }
    out->records_folded = h.folded;
    out->records_absorbed = h.absorbed;
    out->grows = t->grows;
    out->fold_launches = t->fold_launches;
    out->fold_ns_total = t->fold_ns_total;
    return FA_OK;
}
