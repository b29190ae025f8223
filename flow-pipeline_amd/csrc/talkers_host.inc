// talkers_host.inc - host side of the exact top talkers (included by flowagg.hip: one translation unit; device side: talkers.cuh).
//
// Capacity rule.  Per table the host keeps an upper bound used_ub of the occupied slots: a chunk of m records (or m merged
// rows) adds at most m keys.  Before a launch, if (used_ub + m) * 2 > capacity, the stream is synchronised and the device's
// exact count replaces the bound; while the inequality still holds the table doubles (talker_rehash_kernel re-inserts every
// slot).  So every launch finds its table at or below half full when it ends - the unbounded probe loops of talkers.cuh end.
// 2^30 slots is the limit: FA_ERR_TABLE_FULL BEFORE the chunk is folded.
// Chunks: at most FA_TALK_CHUNK records (default 2^20), and at most max(2^16, capacity / 4) so that a small table grows in
// steps instead of jumping to the worst case of a large chunk.

struct TalkState {
    DevBuf<TSlot> tab[2];
    uint32_t log2[2] = {16, 16};
    uint32_t bucket_secs = 0;  // fa_talkers_enable_buckets: the key carries t32 / bucket_secs; 0 = plain tables (no time axis)
    uint64_t used_ub[2] = {0, 0};
    DevBuf<TalkCounters> d_ctr;
    size_t chunk = (size_t)1 << 20;  // env FA_TALK_CHUNK
    uint32_t wgpc = TALK_WG_PER_CU;  // env FA_TALK_WGPC (A/B: workgroups per CU of the fold kernel)
    uint64_t grows = 0, fold_launches = 0, fold_ns_total = 0;
    struct Ev { hipEvent_t e0, e1; };
    std::vector<Ev> ev;   // one pair per fold launch that has not been read yet
    size_t ev_used = 0;
    DevBuf<> scratch;  // fa_top_talkers: rows, ordered rows, sort keys, permutations, hipcub storage
    DevBuf<> order;    // talk_order_rows: sort keys, permutations, hipcub storage of the row kinds' emit order
    DevBuf<> rows;     // collect_talkers: a table's rows on their way into the device-resident close (rows_host.inc)
};

static uint32_t talk_bucket_secs(const fa_ctx* c) { return c->talk ? c->talk->bucket_secs : 0; }
static void talk_destroy(fa_ctx* c) {
    TalkState* t = c->talk;
    if (!t) return;
    for (auto& e : t->ev) {
        (void)hipEventDestroy(e.e0);
        (void)hipEventDestroy(e.e1);
    }
    delete t;
    c->talk = nullptr;
}

#define TALK_ENTER(c)                                                                                  \
    FA_ON_DEVICE(c);                                                                                   \
    if (!(c)) return FA_ERR_ARG;                                                                       \
    if ((c)->sticky) return (c)->sticky;                                                               \
    if (!(c)->talk) return fail((c), FA_ERR_UNSUPPORTED, TALK_OFF)

static const char TALK_MERGE_BUCKETED[] =
    "an fa_talker_row carries no time, so rows cannot be merged into bucketed tables; partitions meet through rows in HBM (fa_talkers_range_rows_device, fa_rows_merge_device)";
#define TALK_ENTER_BUCKETED(c) \
    TALK_ENTER(c);             \
    if (!(c)->talk->bucket_secs) return fail((c), FA_ERR_UNSUPPORTED, TALK_NOT_BUCKETED)

// bucket_secs 0: plain tables
static int talk_enable(fa_ctx* c, uint32_t capacity_log2, uint32_t bucket_secs) {
    if (c->talk) return fail(c, FA_ERR_ARG, "fa_talkers_enable: already enabled (a ctx is enabled once, plain or bucketed)");
    if (capacity_log2 == 0) capacity_log2 = 16;
    if (capacity_log2 < 8 || capacity_log2 > 30) return fail(c, FA_ERR_ARG, "fa_talkers_enable: capacity_log2 is 0 or 8..30");
    TalkState* t = new TalkState();
    t->bucket_secs = bucket_secs;
    if (const char* d = getenv("FA_TALK_CHUNK")) t->chunk = (size_t)std::min<long long>(1ll << 28, std::max<long long>(1, atoll(d)));
    if (const char* d = getenv("FA_TALK_WGPC")) t->wgpc = (uint32_t)std::min(8, std::max(1, atoi(d)));
    c->talk = t;
    bool ok = t->d_ctr.grow(sizeof(TalkCounters)) && hipMemsetAsync(t->d_ctr, 0, sizeof(TalkCounters), c->stream) == hipSuccess;
    for (int d = 0; d < 2 && ok; d++) {
        t->log2[d] = capacity_log2;
        ok = t->tab[d].grow(sizeof(TSlot) << capacity_log2) && hipMemsetAsync(t->tab[d], 0, sizeof(TSlot) << capacity_log2, c->stream) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        talk_destroy(c);
        return fail(c, FA_ERR_NOMEM, "fa_talkers_enable: allocating the tables failed");
    }
    return FA_OK;
}
extern "C" int fa_talkers_enable(fa_ctx* c, uint32_t capacity_log2) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    return talk_enable(c, capacity_log2, 0);
}
extern "C" int fa_talkers_enable_buckets(fa_ctx* c, uint32_t capacity_log2, uint32_t bucket_secs) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (bucket_secs == 0 || 86400u % bucket_secs) return fail(c, FA_ERR_ARG, "fa_talkers_enable_buckets: bucket_secs must be >= 1 and divide 86400");
    return talk_enable(c, capacity_log2, bucket_secs);
}

// Waits for the stream; the device counters and the fold launches' times.
static int talk_settle(fa_ctx* c, TalkCounters& h) {
    TalkState* t = c->talk;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&h, t->d_ctr, sizeof h, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < t->ev_used; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t->ev[i].e0, t->ev[i].e1) == hipSuccess) t->fold_ns_total += (uint64_t)((double)ms * 1e6);
    }
    t->ev_used = 0;
    if (h.lost) {
        c->sticky = FA_ERR_TABLE_FULL;
        return fail(c, FA_ERR_TABLE_FULL, "internal: a talker table was full during a launch; updates were lost");
    }
    return FA_OK;
}

// Table d rebuilt into a fresh one of 2^nl slots: growth (nl = log2 + 1, everything kept) and fa_talkers_drop_before (the same
// size, the slots of a bucket index below floor_index left behind).  The device's used[d] is counted again.
// fresh: a table of 2^nl slots the caller allocated beforehand (fa_talkers_drop_before allocates both before it rebuilds either).
static int talk_rebuild(fa_ctx* c, int d, uint32_t nl, uint32_t floor_index, DevBuf<TSlot>* fresh = nullptr) {
    TalkState* t = c->talk;
    DevBuf<TSlot> nt;
    if (fresh) nt = std::move(*fresh);
    else if (!nt.grow(sizeof(TSlot) << nl)) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "hipMalloc(talker table) failed");
    }
    hipError_t e = hipMemsetAsync(nt, 0, sizeof(TSlot) << nl, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(&t->d_ctr->used[d], 0, sizeof(unsigned long long), c->stream);  // (the rehash counts every key again)
    if (e == hipSuccess) {
        const uint64_t slots = 1ull << t->log2[d];
        const unsigned g = (unsigned)std::min<uint64_t>((slots + 255) / 256, (uint64_t)c->num_cus * 8);
        hipLaunchKernelGGL(talker_rehash_kernel, dim3(g), dim3(256), 0, c->stream, (const TSlot*)t->tab[d], slots, nt.get(), (uint32_t)((1ull << nl) - 1), t->d_ctr.get(), d,
                           floor_index);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->sticky = FA_ERR_HIP;  // (the occupied-slot counter was reset: the state is no longer trustworthy)
        c->err = std::string("talker table rebuild: ") + hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    t->tab[d] = std::move(nt);  // (frees the old table: the rehash has been synchronised)
    t->log2[d] = nl;
    return FA_OK;
}
static int talk_grow(fa_ctx* c, int d) {
    const int rc = talk_rebuild(c, d, c->talk->log2[d] + 1, 0);
    if (!rc) c->talk->grows++;
    return rc;
}

// Room for m more keys in table d at a load of at most 1/2 (the capacity rule above).
static int talk_reserve(fa_ctx* c, int d, uint64_t m) {
    TalkState* t = c->talk;
    if ((t->used_ub[d] + m) * 2 <= (1ull << t->log2[d])) return FA_OK;
    TalkCounters h;
    int rc = talk_settle(c, h);
    if (rc) return rc;
    t->used_ub[0] = h.used[0];
    t->used_ub[1] = h.used[1];
    while ((t->used_ub[d] + m) * 2 > (1ull << t->log2[d])) {
        if (t->log2[d] >= 30) return fail(c, FA_ERR_TABLE_FULL, "a talker table cannot grow further (2^30 slots)");
        rc = talk_grow(c, d);
        if (rc) return rc;
    }
    return FA_OK;
}

static size_t talk_chunk_cap(const fa_ctx* c) {
    const TalkState* t = c->talk;
    const uint64_t cap = 1ull << std::min(t->log2[0], t->log2[1]);
    return (size_t)std::min<uint64_t>(t->chunk, std::max<uint64_t>(1ull << 16, cap / 4));
}

struct TalkCols {
    const void *src_addr, *dst_addr, *etype, *bytes, *sampling_rate, *status;
    const void* time_flow_start;  // read on a bucketed ctx only
};

static int talk_fold_cols(fa_ctx* c, const TalkCols& p, size_t n) {
    TalkState* t = c->talk;
    for (size_t i = 0; i < n;) {
        const size_t m = std::min(n - i, talk_chunk_cap(c));
        for (int d = 0; d < 2; d++) {
            int rc = talk_reserve(c, d, m);
            if (rc) return rc;
        }
        if (t->ev_used == t->ev.size()) {
            if (t->ev.size() >= 1024) {  // bound the pool: read what is pending
                TalkCounters h;
                int rc = talk_settle(c, h);
                if (rc) return rc;
            } else {
                TalkState::Ev e{};
                HIPCHK(c, hipEventCreate(&e.e0));
                if (hipEventCreate(&e.e1) != hipSuccess) {
                    (void)hipEventDestroy(e.e0);
                    return fail(c, FA_ERR_HIP, "hipEventCreate failed");
                }
                t->ev.push_back(e);
            }
        }
        TalkFoldArgs a{};
        a.src_addr = (const uint4*)p.src_addr + i;
        a.dst_addr = (const uint4*)p.dst_addr + i;
        a.etype = (const uint32_t*)p.etype + i;
        a.bytes = (const uint64_t*)p.bytes + i;
        a.sampling_rate = (const uint64_t*)p.sampling_rate + i;
        a.status = (const uint8_t*)p.status + i;
        a.time_flow_start = t->bucket_secs ? (const uint64_t*)p.time_flow_start + i : nullptr;
        a.bucket_secs = t->bucket_secs;
        a.n = (uint32_t)m;
        for (int d = 0; d < 2; d++) {
            a.tab[d] = t->tab[d];
            a.mask[d] = (uint32_t)((1ull << t->log2[d]) - 1);
        }
        a.ctr = t->d_ctr;
        // persistent grid: the workgroups that are co-resident, records grid-strided
        const uint32_t grid = (uint32_t)std::max<size_t>(1, std::min<size_t>((m + TALK_BLOCK - 1) / TALK_BLOCK, (size_t)c->num_cus * t->wgpc));
        TalkState::Ev& ev = t->ev[t->ev_used++];
        (void)hipEventRecord(ev.e0, c->stream);
        if (t->bucket_secs) hipLaunchKernelGGL(talker_fold_kernel<true>, dim3(grid), dim3(TALK_BLOCK), 0, c->stream, a);
        else hipLaunchKernelGGL(talker_fold_kernel<false>, dim3(grid), dim3(TALK_BLOCK), 0, c->stream, a);
        (void)hipEventRecord(ev.e1, c->stream);
        HIPCHK(c, hipGetLastError());
        t->fold_launches++;
        t->used_ub[0] += m;
        t->used_ub[1] += m;
        i += m;
    }
    return FA_OK;
}

extern "C" int fa_talkers_fold_columns_device(fa_ctx* c, const fa_columns* cols, size_t n) {
    TALK_ENTER(c);
    if (n == 0) return FA_OK;
    if (!cols || !cols->src_addr || !cols->dst_addr || !cols->etype || !cols->bytes || !cols->sampling_rate || !cols->status)
        return fail(c, FA_ERR_ARG, "fa_talkers_fold_columns_device: src_addr, dst_addr, etype, bytes, sampling_rate and status are needed");
    if ((((uintptr_t)cols->src_addr | (uintptr_t)cols->dst_addr) & 15) || (((uintptr_t)cols->bytes | (uintptr_t)cols->sampling_rate) & 7) || ((uintptr_t)cols->etype & 3))
        return fail(c, FA_ERR_ARG, "fa_talkers_fold_columns_device: the address columns must be 16-byte aligned (the others naturally)");
    if (c->talk->bucket_secs && (!cols->time_flow_start || ((uintptr_t)cols->time_flow_start & 7)))
        return fail(c, FA_ERR_ARG, "fa_talkers_fold_columns_device: a bucketed ctx also needs time_flow_start, 8-byte aligned");
    const TalkCols p{cols->src_addr, cols->dst_addr, cols->etype, cols->bytes, cols->sampling_rate, cols->status, cols->time_flow_start};
    return talk_fold_cols(c, p, n);
}

extern "C" int fa_merge_talkers(fa_ctx* c, int dst, const fa_talker_row* rows, size_t n) {
    TALK_ENTER(c);
    if (c->talk->bucket_secs) return fail(c, FA_ERR_UNSUPPORTED, TALK_MERGE_BUCKETED);
    if ((!rows && n) || (dst != 0 && dst != 1)) return fail(c, FA_ERR_ARG, "fa_merge_talkers: bad argument");
    static_assert(sizeof(fa_talker_row) == sizeof(TalkRow), "row layout");
    for (size_t i = 0; i < n; i++) {  // all rows are looked at before the first is merged
        bool ok = rows[i].etype == 0 || rows[i].etype == TALK_FAMILY_V4;
        if (ok && rows[i].etype == TALK_FAMILY_V4)
            for (int b = 4; b < 16; b++) ok = ok && rows[i].key[b] == 0;
        if (!ok) return fail(c, FA_ERR_ARG, TALK_NOT_CANONICAL);
    }
    TalkState* t = c->talk;
    for (size_t i = 0; i < n;) {
        const size_t m = std::min(n - i, talk_chunk_cap(c));
        int rc = talk_reserve(c, dst, m);
        if (rc) return rc;
        DevBuf<TalkRow> d;
        if (!d.grow(m * sizeof(TalkRow))) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "hipMalloc failed");
        }
        hipError_t e = hipMemcpyAsync(d, rows + i, m * sizeof(TalkRow), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(talker_merge_kernel, dim3((unsigned)std::min<size_t>((m + 255) / 256, 1024)), dim3(256), 0, c->stream, (const TalkRow*)d, (uint32_t)m,
                               t->tab[dst].get(), (uint32_t)((1ull << t->log2[dst]) - 1), t->d_ctr.get(), dst);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (the caller's rows are not referenced after the call)
        if (e != hipSuccess) {
            c->err = std::string("fa_merge_talkers: ") + hipGetErrorString(e);
            return FA_ERR_HIP;
        }
        t->used_ub[dst] += m;
        i += m;
    }
    return FA_OK;
}

// fa_merge_talkers for rows that sit in HBM already (another ctx's fa_rows_device result, a share an exchange delivered): the
// merge kernel reads the caller's rows where they are.
extern "C" int fa_merge_talkers_device(fa_ctx* c, int dst, const void* d_rows, size_t n) {
    TALK_ENTER(c);
    if (c->talk->bucket_secs) return fail(c, FA_ERR_UNSUPPORTED, TALK_MERGE_BUCKETED);
    if ((!d_rows && n) || (dst != 0 && dst != 1)) return fail(c, FA_ERR_ARG, "fa_merge_talkers_device: bad argument");
    int rc = talker_rows_canonical(c, d_rows, n);
    if (rc) return rc;
    TalkState* t = c->talk;
    for (size_t i = 0; i < n;) {
        const size_t m = std::min(n - i, talk_chunk_cap(c));
        rc = talk_reserve(c, dst, m);
        if (rc) return rc;
        hipLaunchKernelGGL(talker_merge_kernel, dim3((unsigned)std::min<size_t>((m + 255) / 256, 1024)), dim3(256), 0, c->stream, (const TalkRow*)d_rows + i, (uint32_t)m,
                           t->tab[dst].get(), (uint32_t)((1ull << t->log2[dst]) - 1), t->d_ctr.get(), dst);
        HIPCHK(c, hipGetLastError());
        t->used_ub[dst] += m;
        i += m;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's rows are not referenced after the call)
    return FA_OK;
}

// ---- the talker row kinds of the device-resident close (rows_host.inc: rows_local, fa_rows_merge_device) ---------------------
static bool talk_rows_hold(const fa_ctx* c, const void* p) { return c->talk && inside(c->talk->rows, p); }
// [t_lo, t_hi) on the grid of bucket_secs as bucket indices (bucket_range.h states the rule): the talker tables' ranged reads
// and the port tables' (ports_host.inc) share it.
static int talk_range_of(fa_ctx* c, uint32_t bucket_secs, uint32_t t_lo, uint32_t t_hi, BucketRange& r) {
    switch (bucket_range_of(bucket_secs, t_lo, t_hi, r)) {
    case BUCKET_RANGE_OFF_GRID: return fail(c, FA_ERR_ARG, "range: t_lo and t_hi lie on the bucket grid (t_hi = 0xFFFFFFFF: no upper bound)");
    case BUCKET_RANGE_REVERSED: return fail(c, FA_ERR_ARG, "range: t_lo > t_hi");
    default: return FA_OK;
    }
}
// Table d's occupied slots as fa_talker_row, unordered, in the state's row buffer: the exact count first (it sizes the buffer
// and reports lost updates), then one scan of the table.  range: only the slots of those buckets (their count is not known
// beforehand: the table's count bounds it, and the cursor says how many there were).
static int collect_talkers(fa_ctx* c, ReadClock& clk, int kind, const BucketRange* range, const void*& in, size_t& n) {
    TalkState* t = c->talk;
    const int d = kind == RK_TALKERS_DST;
    TalkCounters h;
    int rc = talk_settle(c, h);
    if (rc) return rc;
    t->used_ub[0] = h.used[0];
    t->used_ub[1] = h.used[1];
    clk.mark("settle");
    const size_t used = (size_t)h.used[d];  // (<= 2^29: the load is at most 1/2)
    rc = ensure_dev(c, t->rows, std::max<size_t>(used, 1) * sizeof(TalkRow), "talker rows");
    if (rc) return rc;
    in = t->rows;
    n = 0;
    if (!used || (range && range->empty)) return FA_OK;
    unsigned int* cursor = &c->d_ctr->rows_count;
    HIPCHK(c, zero_word(cursor, c->stream));
    const uint32_t slots = 1u << t->log2[d];
    const unsigned grid = (unsigned)std::min<uint32_t>(512, (slots + TR_BLOCK * TR_U - 1) / (TR_BLOCK * TR_U));
    if (range)
        hipLaunchKernelGGL(talker_rows_kernel<true>, dim3(grid), dim3(TR_BLOCK), 0, c->stream, (const TSlot*)t->tab[d], slots, (TalkRow*)t->rows.get(), (uint32_t)used, cursor,
                           range->index_lo, range->index_last);
    else
        hipLaunchKernelGGL(talker_rows_kernel<false>, dim3(grid), dim3(TR_BLOCK), 0, c->stream, (const TSlot*)t->tab[d], slots, (TalkRow*)t->rows.get(), (uint32_t)used, cursor, 0u,
                           0xFFFFFFFFu);
    HIPCHK(c, hipGetLastError());
    unsigned int got = 0;
    HIPCHK(c, read_word(cursor, got, c->stream));
    if (range ? got > used : got != used) return fail(c, FA_ERR_HIP, "internal: the talker table's rows and its count differ");
    n = got;
    return FA_OK;
}

extern "C" int fa_talkers_reset(fa_ctx* c) {
    TALK_ENTER(c);
    TalkState* t = c->talk;
    TalkCounters h;
    int rc = talk_settle(c, h);
    if (rc) return rc;
    for (int d = 0; d < 2; d++) HIPCHK(c, hipMemsetAsync(t->tab[d], 0, sizeof(TSlot) << t->log2[d], c->stream));
    HIPCHK(c, hipMemsetAsync(&t->d_ctr->used[0], 0, 2 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t->used_ub[0] = t->used_ub[1] = 0;
    return FA_OK;
}

extern "C" int fa_talkers_stats(fa_ctx* c, fa_talkers_stats_t* out) {
    TALK_ENTER(c);
    if (!out) return fail(c, FA_ERR_ARG, "fa_talkers_stats: null argument");
    TalkState* t = c->talk;
    TalkCounters h;
    int rc = talk_settle(c, h);
    if (rc) return rc;
    for (int d = 0; d < 2; d++) {
        t->used_ub[d] = h.used[d];
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

// Every group, or the first k, in emit order: the occupied slots are compacted into rows, ordered ON THE DEVICE by four stable
// radix sorts over (key word, index) - least significant criterion first - and only the rows returned are copied out.
extern "C" int fa_top_talkers(fa_ctx* c, int dst, size_t k, fa_talker_row* out, size_t cap, size_t* n_out) {
    TALK_ENTER(c);
    if ((dst != 0 && dst != 1) || !n_out || (!out && cap)) return fail(c, FA_ERR_ARG, "fa_top_talkers: bad argument");
    TalkState* t = c->talk;
    // (bucketed tables hold a key once per bucket: every bucket held, summed and ordered by the row merge of the close)
    if (t->bucket_secs) return rows_read(c, dst ? RK_TALKERS_DST : RK_TALKERS_SRC, 0, k, out, cap, n_out);
    TalkCounters h;
    int rc = talk_settle(c, h);
    if (rc) return rc;
    t->used_ub[0] = h.used[0];
    t->used_ub[1] = h.used[1];
    const size_t used = (size_t)h.used[dst];
    const size_t need = k ? std::min(k, used) : used;
    *n_out = need;
    if (need > cap) return fail(c, FA_ERR_CAPACITY, "fa_top_talkers: output buffer too small");
    if (need == 0) return FA_OK;
    const uint32_t n = (uint32_t)used;  // (<= 2^29: the load is at most 1/2)
    size_t tmp_bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0,
                                           64, c->stream) != hipSuccess)
        return fail(c, FA_ERR_HIP, "fa_top_talkers: sort sizing failed");
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t rows_b = al((size_t)n * sizeof(TalkRow)), out_b = al(need * sizeof(TalkRow)), key_b = al((size_t)n * 8), perm_b = al((size_t)n * 4);
    rc = ensure_dev(c, t->scratch, rows_b + out_b + 2 * key_b + 2 * perm_b + 256 + al(tmp_bytes), "talker rows");
    if (rc) return rc;
    uint8_t* p = (uint8_t*)t->scratch;
    TalkRow* rows = (TalkRow*)p;
    TalkRow* ordered = (TalkRow*)(p + rows_b);
    unsigned long long* keys[2] = {(unsigned long long*)(p + rows_b + out_b), (unsigned long long*)(p + rows_b + out_b + key_b)};
    uint32_t* perm[2] = {(uint32_t*)(p + rows_b + out_b + 2 * key_b), (uint32_t*)(p + rows_b + out_b + 2 * key_b + perm_b)};
    unsigned int* cursor = (unsigned int*)(p + rows_b + out_b + 2 * key_b + 2 * perm_b);
    void* tmp = p + rows_b + out_b + 2 * key_b + 2 * perm_b + 256;
    HIPCHK(c, hipMemsetAsync(cursor, 0, sizeof(unsigned int), c->stream));
    const uint64_t slots = 1ull << t->log2[dst];
    const unsigned gs = (unsigned)std::min<uint64_t>((slots + 255) / 256, (uint64_t)c->num_cus * 8);
    const unsigned gn = (unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, (uint64_t)c->num_cus * 8);
    hipLaunchKernelGGL(talker_collect_kernel, dim3(gs), dim3(256), 0, c->stream, (const TSlot*)t->tab[dst], slots, rows, n, cursor);
    int cur = 0;
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(talker_sortkey_kernel, dim3(gn), dim3(256), 0, c->stream, (const TalkRow*)rows, pass ? (const uint32_t*)perm[cur] : (const uint32_t*)nullptr, n, pass, keys[0],
                           perm[cur]);
        size_t tb = tmp_bytes;
        if (hipcub::DeviceRadixSort::SortPairs(tmp, tb, (const unsigned long long*)keys[0], keys[1], (const uint32_t*)perm[cur], perm[cur ^ 1], (int)n, 0, pass == 0 ? 16 : 64,
                                               c->stream) != hipSuccess)
            return fail(c, FA_ERR_HIP, "fa_top_talkers: sort failed");
        cur ^= 1;
    }
    hipLaunchKernelGGL(talker_emit_kernel, dim3((unsigned)std::min<uint64_t>(((uint64_t)need + 255) / 256, (uint64_t)c->num_cus * 8)), dim3(256), 0, c->stream, (const TalkRow*)rows,
                       (const uint32_t*)perm[cur], (uint32_t)need, ordered);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, ordered, need * sizeof(TalkRow), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FA_OK;
}

// The row kinds' emit order (rows_host.inc, rows_merge_t): talker_sortkey_kernel's four passes, least significant criterion
// first, each a stable full-width radix sort over (key word, index) - what fa_top_talkers runs over a plain table's slots.
static int talk_order_rows(fa_ctx* c, hipStream_t stream, const TalkRow* rows, uint32_t n, size_t need, TalkRow* out) {
    TalkState* t = c->talk;
    if (!t) return fail(c, FA_ERR_UNSUPPORTED, TALK_OFF);
    if (!n || !need) return FA_OK;
    size_t tmp_bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0,
                                           64, stream) != hipSuccess)
        return fail(c, FA_ERR_HIP, "talker rows: sort sizing failed");
    const size_t key_b = align256((size_t)n * 8), perm_b = align256((size_t)n * 4);
    int rc = ensure_dev(c, t->order, 2 * key_b + 2 * perm_b + align256(tmp_bytes), "talker row order");
    if (rc) return rc;
    uint8_t* p = (uint8_t*)t->order;
    unsigned long long* keys[2] = {(unsigned long long*)p, (unsigned long long*)(p + key_b)};
    uint32_t* perm[2] = {(uint32_t*)(p + 2 * key_b), (uint32_t*)(p + 2 * key_b + perm_b)};
    void* tmp = p + 2 * key_b + 2 * perm_b;
    const unsigned gn = (unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, (uint64_t)c->num_cus * 8);
    int cur = 0;
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(talker_sortkey_kernel, dim3(gn), dim3(256), 0, stream, rows, pass ? (const uint32_t*)perm[cur] : (const uint32_t*)nullptr, n, pass, keys[0], perm[cur]);
        size_t tb = tmp_bytes;
        if (hipcub::DeviceRadixSort::SortPairs(tmp, tb, (const unsigned long long*)keys[0], keys[1], (const uint32_t*)perm[cur], perm[cur ^ 1], (int)n, 0, pass == 0 ? 16 : 64, stream) !=
            hipSuccess)
            return fail(c, FA_ERR_HIP, "talker rows: sort failed");
        cur ^= 1;
    }
    hipLaunchKernelGGL(talker_emit_kernel, dim3((unsigned)std::min<uint64_t>(((uint64_t)need + 255) / 256, (uint64_t)c->num_cus * 8)), dim3(256), 0, stream, rows,
                       (const uint32_t*)perm[cur], (uint32_t)need, out);
    HIPCHK(c, hipGetLastError());
    return FA_OK;
}

// ---- bucketed tables: ranged reads and retention ------------------------------------------------------------------------------
// Both ranged reads are the un-ranged ones with another collector: talker_rows_kernel<true> keeps the slots of the range and
// drops the bucket, and the RowOps<RK_TALKERS_*> merge sums the rows of equal key and leaves fa_top_talkers' order, cut at k.
extern "C" int fa_top_talkers_range(fa_ctx* c, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_talker_row* out, size_t cap, size_t* n_out) {
    TALK_ENTER_BUCKETED(c);
    if ((dst != 0 && dst != 1) || !n_out || (!out && cap)) return fail(c, FA_ERR_ARG, "fa_top_talkers_range: bad argument");
    BucketRange r;
    int rc = talk_range_of(c, c->talk->bucket_secs, t_lo, t_hi, r);
    if (rc) return rc;
    return rows_read(c, dst ? RK_TALKERS_DST : RK_TALKERS_SRC, 0, k, out, cap, n_out, &r);
}
extern "C" int fa_talkers_range_rows_device(fa_ctx* c, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, const void** d_rows, size_t* n_out) {
    TALK_ENTER_BUCKETED(c);
    if ((dst != 0 && dst != 1) || !n_out || !d_rows) return fail(c, FA_ERR_ARG, "fa_talkers_range_rows_device: bad argument");
    BucketRange r;
    int rc = talk_range_of(c, c->talk->bucket_secs, t_lo, t_hi, r);
    if (rc) return rc;
    const int kind = dst ? RK_TALKERS_DST : RK_TALKERS_SRC;
    ReadClock clk(c);
    rc = rows_local(c, clk, kind, 0, k, d_rows, n_out, false, nullptr, &r);
    if (rc) return rc;
    clk.done(row_kind_name(kind), clk.n_in, *n_out);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FA_OK;
}

// The bucket starts held in a pair of bucketed tables, ascending (fa_open_timeslots' contract): what fa_talkers_buckets and
// fa_ports_buckets (ports_host.inc) answer.  Min and max index first; a span of up to 2^16 indices is answered from one bit per
// index, a wider one (bucket_secs = 1 over days, stray times) from the slots' own indices.
//   held: the occupied slots of both tables; scratch: a buffer of the state, dead otherwise;
//   scan(lo, nbits, bits, range): launches the tables' buckets kernel over both tables (bits == nullptr: min / max into range);
//   list(out, cap, cursor): launches their bucket-list kernel over both.
template <class Scan, class List>
static int bucket_starts(fa_ctx* c, uint32_t bucket_secs, size_t held, DevBuf<>& scratch, Scan&& scan, List&& list, uint32_t* out, size_t cap, size_t* n_out) {
    constexpr uint32_t MAXBITS = 1u << 16;
    int rc = ensure_dev(c, scratch, std::max<size_t>(MAXBITS / 8 + 64, held * sizeof(uint32_t) + 64), "buckets");
    if (rc) return rc;
    unsigned int* range = (unsigned int*)scratch.get();  // {min, max, any, cursor}
    unsigned int* bits = range + 16;
    const unsigned int init[4] = {0xffffffffu, 0u, 0u, 0u};
    HIPCHK(c, hipMemcpyAsync(range, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    scan(0u, 0u, (unsigned int*)nullptr, range);
    HIPCHK(c, hipGetLastError());
    unsigned int r[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(r, range, sizeof r, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (init is read by the copy above until here)
    std::vector<uint32_t> idx;
    if (r[2]) {
        if (r[1] - r[0] < MAXBITS) {
            const uint32_t nbits = r[1] - r[0] + 1u, nwords = (nbits + 31u) / 32u;
            HIPCHK(c, hipMemsetAsync(bits, 0, nwords * sizeof(unsigned int), c->stream));
            scan(r[0], nbits, bits, range);
            HIPCHK(c, hipGetLastError());
            std::vector<unsigned int> hb(nwords);
            HIPCHK(c, hipMemcpyAsync(hb.data(), bits, nwords * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (uint32_t i = 0; i < nbits; i++)
                if (hb[i >> 5] >> (i & 31u) & 1u) idx.push_back(r[0] + i);
        } else {
            list((uint32_t*)(range + 16), (uint32_t)held, range + 3);
            HIPCHK(c, hipGetLastError());
            unsigned int got = 0;
            HIPCHK(c, read_word(range + 3, got, c->stream));
            if (got != held) return fail(c, FA_ERR_HIP, "internal: the bucketed tables' slots and their counts differ");
            idx.resize(got);
            if (got) HIPCHK(c, hipMemcpy(idx.data(), range + 16, (size_t)got * sizeof(uint32_t), hipMemcpyDeviceToHost));
            std::sort(idx.begin(), idx.end());
            idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
        }
    }
    *n_out = idx.size();
    if (idx.size() > cap) return fail(c, FA_ERR_CAPACITY, "output buffer too small");
    for (size_t i = 0; i < idx.size(); i++) out[i] = idx[i] * bucket_secs;
    return FA_OK;
}
extern "C" int fa_talkers_buckets(fa_ctx* c, uint32_t* out, size_t cap, size_t* n_out) {
    TALK_ENTER_BUCKETED(c);
    if (!n_out || (!out && cap)) return fail(c, FA_ERR_ARG, "fa_talkers_buckets: bad argument");
    TalkState* t = c->talk;
    TalkCounters h;
    int rc = talk_settle(c, h);
    if (rc) return rc;
    t->used_ub[0] = h.used[0];
    t->used_ub[1] = h.used[1];
    auto grid = [&](int d) { return dim3((unsigned)std::min<uint64_t>(((1ull << t->log2[d]) + 255) / 256, (uint64_t)c->num_cus * 8)); };
    return bucket_starts(
        c, t->bucket_secs, (size_t)(h.used[0] + h.used[1]), t->rows,
        [&](uint32_t lo, uint32_t nbits, unsigned int* bits, unsigned int* range) {
            for (int d = 0; d < 2; d++) hipLaunchKernelGGL(talker_buckets_kernel, grid(d), dim3(256), 0, c->stream, (const TSlot*)t->tab[d], 1ull << t->log2[d], lo, nbits, bits, range);
        },
        [&](uint32_t* list, uint32_t list_cap, unsigned int* cursor) {
            for (int d = 0; d < 2; d++) hipLaunchKernelGGL(talker_bucket_list_kernel, grid(d), dim3(256), 0, c->stream, (const TSlot*)t->tab[d], 1ull << t->log2[d], list, list_cap, cursor);
        },
        out, cap, n_out);
}

// Removes every bucket that starts below t.  The slots are write-once, so nothing is deleted in place: each table is rebuilt into
// a fresh one of the same size without those slots (talk_rebuild), used[] and the host's bounds counted again.  No floor is kept:
// a record that arrives later with a time below t opens its bucket again (what a late INSERT does to flows_5m).
extern "C" int fa_talkers_drop_before(fa_ctx* c, uint32_t t_floor) {
    TALK_ENTER_BUCKETED(c);
    TalkState* t = c->talk;
    if (t_floor % t->bucket_secs) return fail(c, FA_ERR_ARG, "fa_talkers_drop_before: t lies on the bucket grid");
    TalkCounters h;
    int rc = talk_settle(c, h);
    if (rc) return rc;
    if (t_floor == 0) return FA_OK;
    DevBuf<TSlot> fresh[2];  // both before either table is touched: without memory nothing is dropped, in neither table
    for (int d = 0; d < 2; d++)
        if (!fresh[d].grow(sizeof(TSlot) << t->log2[d])) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "fa_talkers_drop_before: hipMalloc(talker table) failed; nothing was dropped");
        }
    for (int d = 0; d < 2; d++) {
        rc = talk_rebuild(c, d, t->log2[d], t_floor / t->bucket_secs, &fresh[d]);
        if (rc) return rc;  // (a failing launch or synchronisation: sticky)
    }
    rc = talk_settle(c, h);
    if (rc) return rc;
    t->used_ub[0] = h.used[0];
    t->used_ub[1] = h.used[1];
    return FA_OK;
}
