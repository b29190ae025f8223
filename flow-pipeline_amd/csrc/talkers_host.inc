// talkers_host.inc - host side of the exact top talkers (included by flowagg.hip: one translation unit; device side: talkers.cuh).
// The tables, their capacity rule, chunks, growth, retention and statistics are keytab_host.inc's under the traits TalkTab; here
// are the talkers' own doors, their fold and merge launches, and the read side.

struct TalkState : TabPair<TalkTab> {
    DevBuf<> top;    // fa_top_talkers: the rows it returns, ordered
    DevBuf<> order;  // talk_order_rows: sort keys, permutations, hipcub storage of the row kinds' emit order
    DevBuf<> rows;   // collect_talkers: a table's rows on their way into the device-resident close (rows_host.inc)
    bool alloc_own() { return true; }
};

static uint32_t talk_bucket_secs(const fa_ctx* c) { return c->talk ? c->talk->bucket_secs : 0; }

#define TALK_ENTER(c) TAB_ENTER(c, talk, TALK_OFF)

static const char TALK_MERGE_BUCKETED[] =
    "an fa_talker_row carries no time, so rows cannot be merged into bucketed tables; partitions meet through rows in HBM (fa_talkers_range_rows_device, fa_rows_merge_device)";
#define TALK_ENTER_BUCKETED(c) \
    TALK_ENTER(c);             \
    if (!(c)->talk->bucket_secs) return fail((c), FA_ERR_UNSUPPORTED, TALK_NOT_BUCKETED)

// bucket_secs 0: plain tables
static int talk_enable(fa_ctx* c, uint32_t capacity_log2, uint32_t bucket_secs) {
    if (c->talk) return fail(c, FA_ERR_ARG, "fa_talkers_enable: already enabled (a ctx is enabled once, plain or bucketed)");
    return tab_enable<TalkTab>(c, c->talk, "fa_talkers_enable", capacity_log2, bucket_secs);
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

static size_t talk_chunk_cap(const fa_ctx* c) { return tab_chunk_cap(*c->talk); }

struct TalkCols {
    const void *src_addr, *dst_addr, *etype, *bytes, *sampling_rate, *status;
    const void* time_flow_start;  // read on a bucketed ctx only
};

static int talk_fold_cols(fa_ctx* c, const TalkCols& p, size_t n) {
    TalkState& t = *c->talk;
    return tab_chunks(c, t, 3, n, [&](size_t i, size_t m) -> int {
        TalkFoldArgs a{};
        a.src_addr = (const uint4*)p.src_addr + i;
        a.dst_addr = (const uint4*)p.dst_addr + i;
        a.etype = (const uint32_t*)p.etype + i;
        a.bytes = (const uint64_t*)p.bytes + i;
        a.sampling_rate = (const uint64_t*)p.sampling_rate + i;
        a.status = (const uint8_t*)p.status + i;
        a.time_flow_start = t.bucket_secs ? (const uint64_t*)p.time_flow_start + i : nullptr;
        a.bucket_secs = t.bucket_secs;
        a.n = (uint32_t)m;
        for (int d = 0; d < 2; d++) {
            a.tab[d] = t.tab[d];
            a.mask[d] = t.mask(d);
        }
        a.ctr = t.d_ctr;
        return tab_fold_launch(c, t, m, [&](dim3 grid) {
            if (t.bucket_secs) hipLaunchKernelGGL(talker_fold_kernel<true>, grid, dim3(TALK_BLOCK), 0, c->stream, a);
            else hipLaunchKernelGGL(talker_fold_kernel<false>, grid, dim3(TALK_BLOCK), 0, c->stream, a);
        });
    });
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

// m canonical rows in HBM into table dst (room reserved by the chunk loop)
static void talk_merge_launch(fa_ctx* c, int dst, const TalkRow* d_rows, size_t m) {
    TalkState& t = *c->talk;
    hipLaunchKernelGGL(talker_merge_kernel, dim3((unsigned)std::min<size_t>((m + 255) / 256, 1024)), dim3(256), 0, c->stream, d_rows, (uint32_t)m, t.tab[dst].get(), t.mask(dst),
                       t.d_ctr.get(), dst);
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
    return tab_chunks(c, *c->talk, 1 << dst, n, [&](size_t i, size_t m) -> int {
        DevBuf<TalkRow> d;
        if (!d.grow(m * sizeof(TalkRow))) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "hipMalloc failed");
        }
        hipError_t e = hipMemcpyAsync(d, rows + i, m * sizeof(TalkRow), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            talk_merge_launch(c, dst, d, m);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (the caller's rows are not referenced after the call)
        if (e != hipSuccess) {
            c->err = std::string("fa_merge_talkers: ") + hipGetErrorString(e);
            return FA_ERR_HIP;
        }
        return FA_OK;
    });
}

// fa_merge_talkers for rows that sit in HBM already (another ctx's fa_rows_device result, a share an exchange delivered): the
// merge kernel reads the caller's rows where they are.
extern "C" int fa_merge_talkers_device(fa_ctx* c, int dst, const void* d_rows, size_t n) {
    TALK_ENTER(c);
    if (c->talk->bucket_secs) return fail(c, FA_ERR_UNSUPPORTED, TALK_MERGE_BUCKETED);
    if ((!d_rows && n) || (dst != 0 && dst != 1)) return fail(c, FA_ERR_ARG, "fa_merge_talkers_device: bad argument");
    int rc = talker_rows_canonical(c, d_rows, n);
    if (rc) return rc;
    rc = tab_chunks(c, *c->talk, 1 << dst, n, [&](size_t i, size_t m) -> int {
        talk_merge_launch(c, dst, (const TalkRow*)d_rows + i, m);
        HIPCHK(c, hipGetLastError());
        return FA_OK;
    });
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's rows are not referenced after the call)
    return FA_OK;
}

// ---- the talker row kinds of the device-resident close (rows_host.inc: rows_local, fa_rows_merge_device) ---------------------
static bool talk_rows_hold(const fa_ctx* c, const void* p) { return c->talk && inside(c->talk->rows, p); }
// Table d's occupied slots as fa_talker_row, unordered, in the state's row buffer: the exact count first (it sizes the buffer
// and reports lost updates), then one scan of the table.  range: only the slots of those buckets (their count is not known
// beforehand: the table's count bounds it, and the cursor says how many there were).
static int collect_talkers(fa_ctx* c, ReadClock& clk, int kind, const BucketRange* range, const void*& in, size_t& n) {
    TalkState* t = c->talk;
    const int d = kind == RK_TALKERS_DST;
    TalkCounters h;
    int rc = tab_settle(c, *t, h);
    if (rc) return rc;
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
    return tab_reset(c, *c->talk);
}
extern "C" int fa_talkers_stats(fa_ctx* c, fa_talkers_stats_t* out) {
    TALK_ENTER(c);
    return tab_stats(c, *c->talk, out);
}

// Every group, or the first k, in emit order: a plain table holds a key once, so its rows (collect_talkers) only have to be
// ordered ON THE DEVICE (talk_order_rows), and only the rows returned are copied out.
extern "C" int fa_top_talkers(fa_ctx* c, int dst, size_t k, fa_talker_row* out, size_t cap, size_t* n_out) {
    TALK_ENTER(c);
    if ((dst != 0 && dst != 1) || !n_out || (!out && cap)) return fail(c, FA_ERR_ARG, "fa_top_talkers: bad argument");
    TalkState* t = c->talk;
    const int kind = dst ? RK_TALKERS_DST : RK_TALKERS_SRC;
    // (bucketed tables hold a key once per bucket: every bucket held, summed and ordered by the row merge of the close)
    if (t->bucket_secs) return rows_read(c, kind, 0, k, out, cap, n_out);
    ReadClock clk(c, false);
    const void* rows = nullptr;
    size_t used = 0;
    int rc = collect_talkers(c, clk, kind, nullptr, rows, used);
    if (rc) return rc;
    const size_t need = k ? std::min(k, used) : used;
    *n_out = need;
    if (need > cap) return fail(c, FA_ERR_CAPACITY, "fa_top_talkers: output buffer too small");
    if (need == 0) return FA_OK;
    rc = ensure_dev(c, t->top, need * sizeof(TalkRow), "talker rows");
    if (rc) return rc;
    rc = talk_order_rows(c, c->stream, (const TalkRow*)rows, (uint32_t)used, need, (TalkRow*)t->top.get());
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out, t->top, need * sizeof(TalkRow), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FA_OK;
}

// The row kinds' emit order (rows_host.inc, rows_merge_t) and fa_top_talkers': talker_sortkey_kernel's four passes, least
// significant criterion first, each a stable full-width radix sort over (key word, index).
static int talk_order_rows(fa_ctx* c, hipStream_t stream, const TalkRow* rows, uint32_t n, size_t need, TalkRow* out) {
    TalkState* t = c->talk;
    if (!t) return fail(c, FA_ERR_UNSUPPORTED, TALK_OFF);
    return talk_order_passes(c, stream, t->order, rows, n, need, out, 4);
}
// The scheme itself, for any owner of 40-byte talker rows (the grouped queries, raw_query_host.inc): `order` is the owner's scratch;
// passes = 4: the order above; 3: without the weight - key bytes ascending, etype ascending.
static int talk_order_passes(fa_ctx* c, hipStream_t stream, DevBuf<>& order, const TalkRow* rows, uint32_t n, size_t need, TalkRow* out, int passes) {
    if (!n || !need) return FA_OK;
    size_t tmp_bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0,
                                           64, stream) != hipSuccess)
        return fail(c, FA_ERR_HIP, "talker rows: sort sizing failed");
    const size_t key_b = align256((size_t)n * 8), perm_b = align256((size_t)n * 4);
    int rc = ensure_dev(c, order, 2 * key_b + 2 * perm_b + align256(tmp_bytes), "talker row order");
    if (rc) return rc;
    uint8_t* p = (uint8_t*)order;
    unsigned long long* keys[2] = {(unsigned long long*)p, (unsigned long long*)(p + key_b)};
    uint32_t* perm[2] = {(uint32_t*)(p + 2 * key_b), (uint32_t*)(p + 2 * key_b + perm_b)};
    void* tmp = p + 2 * key_b + 2 * perm_b;
    const unsigned gn = (unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, (uint64_t)c->num_cus * 8);
    int cur = 0;
    for (int pass = 0; pass < passes; pass++) {
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
// The ranged collector: talker_rows_kernel<true> keeps the slots of the range and drops the bucket.
extern "C" int fa_top_talkers_range(fa_ctx* c, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_talker_row* out, size_t cap, size_t* n_out) {
    TALK_ENTER_BUCKETED(c);
    return tab_range_read(c, "fa_top_talkers_range", c->talk->bucket_secs, dst ? RK_TALKERS_DST : RK_TALKERS_SRC, dst, t_lo, t_hi, k, out, cap, n_out);
}
extern "C" int fa_talkers_range_rows_device(fa_ctx* c, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, const void** d_rows, size_t* n_out) {
    TALK_ENTER_BUCKETED(c);
    return tab_range_rows_device(c, "fa_talkers_range_rows_device", c->talk->bucket_secs, dst ? RK_TALKERS_DST : RK_TALKERS_SRC, dst, t_lo, t_hi, k, d_rows, n_out);
}
extern "C" int fa_talkers_buckets(fa_ctx* c, uint32_t* out, size_t cap, size_t* n_out) {
    TALK_ENTER_BUCKETED(c);
    return tab_buckets(c, *c->talk, c->talk->rows, out, cap, n_out);
}
extern "C" int fa_talkers_drop_before(fa_ctx* c, uint32_t t_floor) {
    TALK_ENTER_BUCKETED(c);
    return tab_drop_before(c, *c->talk, t_floor);
}
