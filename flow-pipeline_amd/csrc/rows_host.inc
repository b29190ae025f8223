// rows_host.inc - host side of the device-resident window close (included by flowagg.hip; kernels: merge.cuh).
//
// Every read of aggregated state - fa_read_window / fa_close_window, the (SrcAddr,DstPort,Proto) rows, GROUP BY port,
// the minute series, fa_topk - is "collect the rows out of the device state, merge + order them in HBM, copy the
// result out".  The same two steps are exported (fa_rows_device, fa_rows_merge_device) so that a multi-GPU window
// close exchanges device buffers over RCCL and merges them without a host sort (flow-pipeline_amd/dist.py).

// The RowOps<K> a row kind runs - THE statement of that mapping: both port kinds share one instantiation, both top-k kinds
// another, both talker kinds a third; the two query kinds differ in their emit passes.  f(std::integral_constant<int, K>{}); false for a
// kind that is none (7, 10 and 11 are none).
template <class F>
static bool with_row_kind(int kind, F&& f) {
    switch (kind) {
    case RK_5M: f(std::integral_constant<int, RK_5M>{}); return true;
    case RK_APP: f(std::integral_constant<int, RK_APP>{}); return true;
    case RK_PORT_SRC: case RK_PORT_DST: f(std::integral_constant<int, RK_PORT_SRC>{}); return true;
    case RK_MINUTE: f(std::integral_constant<int, RK_MINUTE>{}); return true;
    case RK_TOPK_SRC: case RK_TOPK_DST: f(std::integral_constant<int, RK_TOPK_SRC>{}); return true;
    case RK_TALKERS_SRC: case RK_TALKERS_DST: f(std::integral_constant<int, RK_TALKERS_SRC>{}); return true;
    case RK_QUERY_WEIGHT: f(std::integral_constant<int, RK_QUERY_WEIGHT>{}); return true;
    case RK_QUERY_KEY: f(std::integral_constant<int, RK_QUERY_KEY>{}); return true;
    default: return false;
    }
}
static size_t row_bytes_of(int kind) {
    size_t bytes = 0;
    (void)with_row_kind(kind, [&](auto rk) { bytes = sizeof(typename RowOps<decltype(rk)::value>::Row); });
    return bytes;
}
static_assert(sizeof(RowOps<RK_5M>::Row) == sizeof(Row5m) && sizeof(Row5m) == 48, "row layout");
static_assert(sizeof(RowOps<RK_APP>::Row) == sizeof(RowApp) && sizeof(RowApp) == 56, "row layout");
static_assert(sizeof(RowOps<RK_PORT_SRC>::Row) == sizeof(RowW) && sizeof(RowOps<RK_MINUTE>::Row) == sizeof(RowW) && sizeof(RowW) == 24, "row layout");
static_assert(sizeof(RowOps<RK_TOPK_SRC>::Row) == sizeof(TopkRow) && sizeof(TopkRow) == 24, "row layout");
static_assert(sizeof(RowOps<RK_TALKERS_SRC>::Row) == sizeof(TalkRow) && sizeof(TalkRow) == sizeof(fa_talker_row) && sizeof(TalkRow) == 40, "row layout");
static_assert(RowOps<RK_TALKERS_SRC>::NK2 <= RP_MAX_WORDS, "emit words");
static_assert(sizeof(RowOps<RK_QUERY_WEIGHT>::Row) == sizeof(fa_query_row) && sizeof(RowOps<RK_QUERY_KEY>::Row) == sizeof(fa_query_row) && sizeof(fa_query_row) == 40, "row layout");
static_assert(RK_QUERY_WEIGHT == FA_ROWS_QUERY_WEIGHT && RK_QUERY_KEY == FA_ROWS_QUERY_KEY, "row kinds");
// The talker kinds' emit order, and fa_top_talkers': the first `need` of n rows (device memory) by four full-width sorts, in the
// talker state's scratch (talkers_host.inc).  The packed emit sort below returned rows out of order on sets of a million talker
// rows (DESIGN.md 3.7); these four sorts never did.
static int talk_order_rows(fa_ctx* c, hipStream_t stream, const TalkRow* rows, uint32_t n, size_t need, TalkRow* out);
static int talk_order_passes(fa_ctx* c, hipStream_t stream, DevBuf<>& order, const TalkRow* rows, uint32_t n, size_t need, TalkRow* out, int passes);
// The query kinds' emit order runs the same passes in the query state's scratch (raw_query_host.inc): the state comes into being
// without tables on a ctx that never queried.
static bool is_query_kind(int kind) { return kind == RK_QUERY_WEIGHT || kind == RK_QUERY_KEY; }
static int query_order_scratch(fa_ctx* c, DevBuf<>** order);
static const char QUERY_NOT_PRODUCIBLE[] =
    "fa_rows_merge_device: a query row no query produces (etype 0 or 0x800; bytes 4..15 zero under 0x800; value != 0 only with a zero key and etype 0)";
extern "C" size_t fa_row_bytes(int kind) { return row_bytes_of(kind); }

static int ensure_dev(fa_ctx* c, DevBuf<>& b, size_t bytes, const char* what) {
    if (b.grow(bytes, bytes + bytes / 8 + 4096)) return FA_OK;
    c->err = std::string("hipMalloc(") + what + ") failed";
    return FA_ERR_NOMEM;
}
// ---- the small steps every read is made of --------------------------------------------------------------------------
// one device word: zeroed in stream order / read back (copy, then synchronise).  Callers wrap them in HIPCHK.
static hipError_t zero_word(unsigned int* d_word, hipStream_t s) { return hipMemsetAsync(d_word, 0, sizeof(unsigned int), s); }
static hipError_t read_word(const unsigned int* d_word, unsigned int& v, hipStream_t s) {
    const hipError_t e = hipMemcpyAsync(&v, d_word, sizeof v, hipMemcpyDeviceToHost, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
}
// does p point into buf?
template <class B>
static bool inside(const B& buf, const void* p) {
    const uint8_t *b = (const uint8_t*)buf.get(), *q = (const uint8_t*)p;
    return b && q >= b && q < b + buf.bytes();
}
static size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// hipcub's temporary storage for an exclusive scan of n words
static size_t scan_tmp_bytes(fa_ctx* c, size_t n) {
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, c->stream);
    return bytes;
}
static dim3 grid_n(size_t n) { return dim3((unsigned)std::min<size_t>(2048, std::max<size_t>(1, (n + 255) / 256))); }
// The buckets a read of `timeslot` covers and the timeslot its rows fold to: the sub-buckets of a sliding window sum into one
// row per key (0xFFFFFFFF: no fold - tumbling windows, every timeslot).  false: not a bucket boundary - no rows.
struct Window { uint32_t lo = 0, hi = 0, fold = 0xFFFFFFFFu; };
static bool window_of(const fa_ctx* c, uint32_t timeslot, Window& w) {
    w = Window{};
    if (!bucket_range(c, timeslot, w.lo, w.hi)) return false;
    if (timeslot != 0xFFFFFFFFu && c->gran != c->cfg.window_secs) w.fold = timeslot;
    return true;
}

// ---- phase times of a read (FA_VERBOSE): collect / key bits / sort / heads + scan / reduce / emit order / copy out ----------
// A read makes one and hands it by reference to everything that works for it; off, a mark is one branch.
struct ReadClock {
    hipStream_t stream;  // what a mark waits for (unless it names another)
    bool on;
    double t_last;
    size_t n_in = 0;
    std::string line;
    static double now() {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
    }
    explicit ReadClock(fa_ctx* c, bool enable = true) : stream(c->stream), on(enable && getenv("FA_VERBOSE") != nullptr), t_last(0) {
        if (on) {
            (void)hipStreamSynchronize(stream);
            t_last = now();
        }
    }
    void mark(const char* what, hipStream_t s = nullptr) {  // (the syncs cost a few us each: verbose runs only)
        if (!on) return;
        (void)hipStreamSynchronize(s ? s : stream);
        const double t = now();
        char buf[64];
        snprintf(buf, sizeof buf, " %s %.2f", what, t - t_last);
        line += buf;
        t_last = t;
    }
    void done(const char* tag, size_t n_in, size_t n_out) {  // (no phase marked - a timeslot off the grid: nothing to say)
        if (on && !line.empty()) fprintf(stderr, "[flowagg read] %s: %zu rows in, %zu out; ms:%s\n", tag, n_in, n_out, line.c_str());
        line.clear();
    }
};

// ---- collect: rows of the device state, public format, unsorted, in a buffer of the ctx (`in`, `n`) -------------------
static int collect_5m(fa_ctx* c, ReadClock&, uint32_t tb_lo, uint32_t tb_hi, const void*& in, size_t& n) {
    int rc = settle(c);
    if (rc) return rc;
    const size_t need = std::max<uint64_t>(c->stats.table_used, 1024);
    rc = ensure_dev(c, c->rc_buf, need * sizeof(Row5m), "rows");
    if (rc) return rc;
    HIPCHK(c, zero_word(&c->d_ctr->rows_count, c->stream));
    hipLaunchKernelGGL(extract_kernel, dim3(1024), dim3(256), 0, c->stream, c->tab, 1u << c->cap_log2, c->gran, tb_lo, tb_hi,
                       (Row5m*)c->rc_buf, (uint32_t)need, c->d_ctr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_ctr, c->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    in = c->rc_buf;
    n = c->h_ctr->rows_count;
    if (n > need) return fail(c, FA_ERR_HIP, "internal: row buffer too small");
    return FA_OK;
}
// The scratch collect_wide_raw wants for a window that lives in pending chunks: the tuple count (256 bytes), then per chunk
// the live tuples of each of its nseg segments and their exclusive scan (wl_arr bytes each), then hipcub's temporary storage
static size_t wl_arr(uint32_t nseg) { return align256((size_t)nseg * 4); }
static size_t wl_scratch_bytes(size_t arrays_end, size_t tmp_scan) { return arrays_end + tmp_scan + 256; }
// selected rows of the wide table (packed keys) into c->rc_buf
static int collect_wide_raw(fa_ctx* c, ReadClock& clk, uint32_t kind_mask, uint32_t tb_lo, uint32_t tb_hi, size_t& n) {
    if (!c->wtab) return fail(c, FA_ERR_ARG, "key set not enabled");
    int rc = settle(c);
    if (rc) return rc;
    clk.mark("settle");
    const size_t need = std::max<uint64_t>(c->stats.wide_used, 1024);
    // log mode: the pending chunks' tuples are rows of this key set as well (one per record; the merge behind this sums them).
    // Kafka partitions are close to time-ordered, so a window lives in one or two chunks: the others are not even scanned
    // (their bucket ranges are looked for once and kept: wlog_bucket_ranges).
    // The live tuples of those chunks are COUNTED first (per segment, then an exclusive scan: maintenance.cuh, wlog_rows_pass)
    // and the row buffer is sized by that count: a window that straddles two chunks holds one chunk's worth of tuples, not
    // two (sized by the chunks' records the buffer doubled to 2.2 GB at the first such window: 90 ms of hipMalloc in a 26 ms read).
    uint64_t pending = 0;
    auto chunk_in_range = [&](const fa_ctx::WChunk& k) {
        return k.minb != 0xFFFFFFFFu && k.maxb >= k.wm && std::max(k.minb, k.wm) < tb_hi && k.maxb >= tb_lo;
    };
    struct Sel {
        const fa_ctx::WChunk* k;
        uint32_t nseg;
        size_t sel_at, pos_at;  // byte offsets into wl_scratch
    };
    std::vector<Sel> sel;
    size_t at = 256, tmp_max = 0;
    if ((kind_mask & (1u << WK_APP)) && !c->wlog.empty()) {
        rc = wlog_bucket_ranges(c);
        if (rc) return rc;
        clk.mark("chunk ranges");
        for (const auto& k : c->wlog) {
            if (!chunk_in_range(k)) continue;
            const uint32_t nseg = (1u << k.wplog2) * k.nwg;
            sel.push_back(Sel{&k, nseg, at, at + wl_arr(nseg)});
            at += 2 * wl_arr(nseg);
            tmp_max = std::max(tmp_max, scan_tmp_bytes(c, nseg));
        }
        if (!sel.empty()) {
            rc = ensure_dev(c, c->wl_scratch, wl_scratch_bytes(at, tmp_max), "log row scratch");
            if (rc) return rc;
            uint8_t* sb = (uint8_t*)c->wl_scratch;
            unsigned int* total = (unsigned int*)sb;
            HIPCHK(c, zero_word(total, c->stream));
            for (const Sel& q : sel) {
                uint32_t* seg_sel = (uint32_t*)(sb + q.sel_at);
                uint32_t* seg_pos = (uint32_t*)(sb + q.pos_at);
                size_t tb = tmp_max;
                hipLaunchKernelGGL(wlog_count_kernel, dim3(2048), dim3(256), 0, c->stream, wchunk_args(*q.k), tb_lo, tb_hi, seg_sel);
                if (hipcub::DeviceScan::ExclusiveSum(sb + at, tb, seg_sel, seg_pos, (int)q.nseg, c->stream) != hipSuccess) return fail(c, FA_ERR_HIP, "scan failed");
                hipLaunchKernelGGL(wlog_bump_kernel, dim3(1), dim3(64), 0, c->stream, (const uint32_t*)seg_sel, (const uint32_t*)seg_pos, q.nseg, total);
            }
            HIPCHK(c, hipGetLastError());
            unsigned int h_total = 0;
            HIPCHK(c, read_word(total, h_total, c->stream));
            pending = h_total;
            clk.mark("count");
        }
    }
    if (need + pending >= (1ull << 32)) return fail(c, FA_ERR_CAPACITY, "too many wide rows for one read");
    rc = ensure_dev(c, c->rc_buf, (need + pending) * sizeof(WRow), "wide rows");
    if (rc) return rc;
    HIPCHK(c, zero_word(&c->d_ctr->wrows_count, c->stream));
    hipLaunchKernelGGL(wextract_kernel, dim3(512), dim3(WX_BLOCK), 0, c->stream, c->wtab, 1u << c->wcap_log2, kind_mask, tb_lo, tb_hi,
                       (WRow*)c->rc_buf, (uint32_t)need, c->d_ctr);
    for (const Sel& q : sel) {  // the selected tuples behind the table's rows, every segment at its place (no atomics, no holes)
        uint8_t* sb = (uint8_t*)c->wl_scratch;
        const uint32_t* seg_sel = (const uint32_t*)(sb + q.sel_at);
        const uint32_t* seg_pos = (const uint32_t*)(sb + q.pos_at);
        hipLaunchKernelGGL(wlog_rows_kernel, dim3(2048), dim3(256), 0, c->stream, wchunk_args(*q.k), tb_lo, tb_hi, seg_pos, (WRow*)c->rc_buf,
                           (uint32_t)(need + pending), (const unsigned int*)&c->d_ctr->wrows_count);
        hipLaunchKernelGGL(wlog_bump_kernel, dim3(1), dim3(64), 0, c->stream, seg_sel, seg_pos, q.nseg, &c->d_ctr->wrows_count);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_ctr, c->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    n = c->h_ctr->wrows_count;
    if (n > need + pending) return fail(c, FA_ERR_HIP, "internal: wide row buffer too small");
    clk.mark("extract");
    return FA_OK;
}
static int ensure_pinned(fa_ctx* c, size_t result_bytes);

// ---- merge: sort, sum equal keys, emit order; result in c->m_out[*] (or the pinned host buffer) -------------------
struct SortScratch {
    unsigned long long *ka, *kb;
    uint32_t *ia, *ib;
    void* tmp;
    size_t tmp_bytes;
    unsigned long long* bits;  // 2 x RP_MAX_WORDS words
};
// the permutation that puts n rows into the kind's merge order (EMIT: emit order): varying bits only (merge.cuh, RowPlan)
template <int KIND, bool EMIT>
static int rows_sort_order(fa_ctx* c, hipStream_t stream, const typename RowOps<KIND>::Row* rows, uint32_t n, uint32_t fold, const SortScratch& s, uint32_t** perm, uint32_t* bits_sorted) {
    typedef RowOps<KIND> Ops;
    constexpr int NW = EMIT ? Ops::NK2 : Ops::NK;
    static_assert(NW >= 1 && NW <= RP_MAX_WORDS, "key words");
    const dim3 g = grid_n(n), b(256);
    HIPCHK(c, hipMemsetAsync(s.bits, 0, NW * sizeof(unsigned long long), stream));
    HIPCHK(c, hipMemsetAsync(s.bits + NW, 0xff, NW * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL((row_bits_kernel<KIND, EMIT>), g, b, 0, stream, rows, n, fold, s.bits);
    unsigned long long h[2 * RP_MAX_WORDS];
    HIPCHK(c, hipMemcpyAsync(h, s.bits, 2 * NW * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    int wbits[RP_MAX_WORDS];
    for (int w = 0; w < NW; w++) {
        if constexpr (EMIT) wbits[w] = Ops::bits2(w);
        else wbits[w] = Ops::bits(w);
    }
    RowPlan plan;
    row_plan_build(h, h + NW, wbits, NW, plan);
    *bits_sorted = 0;
    uint32_t* cur = nullptr;  // permutation so far (nullptr: identity)
    for (uint32_t p = 0; p < plan.nwords; p++) {
        uint32_t* src = cur ? cur : s.ia;  // (identity is written into ia by the first pass)
        uint32_t* dst = src == s.ia ? s.ib : s.ia;
        hipLaunchKernelGGL((row_pack_kernel<KIND, EMIT>), g, b, 0, stream, rows, (const uint32_t*)cur, n, fold, plan, p, s.ka, s.ia);
        size_t tb = s.tmp_bytes;
        if (hipcub::DeviceRadixSort::SortPairs(s.tmp, tb, s.ka, s.kb, src, dst, (int)n, 0, (int)plan.bits[p], stream) != hipSuccess)
            return fail(c, FA_ERR_HIP, "radix sort failed");
        cur = dst;
        *bits_sorted += plan.bits[p];
    }
    if (!cur) {  // every key equal (or one row): any order is the order
        hipLaunchKernelGGL(iota_kernel, g, b, 0, stream, s.ia, n);
        cur = s.ia;
    }
    HIPCHK(c, hipGetLastError());
    *perm = cur;
    return FA_OK;
}

// the sort / scan scratch of a merge of n rows: 2 key arrays, 4 index arrays, hipcub's temporary storage, the key-bit words
static size_t merge_scratch_bytes(fa_ctx* c, uint32_t n, size_t& karr, size_t& iarr, size_t& tmp_bytes) {
    size_t tmp_sort = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                             (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 64, c->stream);
    tmp_bytes = align256(std::max(tmp_sort, scan_tmp_bytes(c, n)));
    karr = align256((size_t)n * 8);
    iarr = align256((size_t)n * 4);
    return 2 * karr + 4 * iarr + tmp_bytes + 256;
}
// The buffers a window read of `rows` (SrcAddr,DstPort,Proto) rows will want - collected rows, sort scratch, merged rows, the
// pinned relay - allocated NOW: called when a launch's tuples are kept in the wide log (maintain_host.inc, wlog_record), so that
// the first window close does not pay for a gigabyte of hipMalloc and 64 MiB of page-locking (round 4: first read 30.9 ms, the
// median 26.3; one read with a 28 ms "collect").  Best effort: a failed allocation is the read's problem, not the ingest's.
static constexpr size_t APP48_SPLIT_MIN = (size_t)1 << 22;  // rows of a window from which fa_read_window_app48 leaves in two halves (below)
static void reserve_window_read(fa_ctx* c, uint64_t rows, uint32_t nseg) {
    if (rows == 0 || rows >= (1ull << 31) - 1024) return;
    // (a member of a group merges the share it RECEIVES: one share of every member - as many rows as its own window in the mean)
    if (c->group_members > 1) rows = std::min<uint64_t>(rows + rows / 8, (1ull << 31) - 2048);
    const std::string keep = c->err;
    // (a window lives in one or two chunks; three when a close lags)
    if (nseg) (void)ensure_dev(c, c->wl_scratch, wl_scratch_bytes(256 + 3 * 2 * wl_arr(nseg), scan_tmp_bytes(c, nseg)), "log row scratch");
    size_t karr, iarr, tmp_bytes;
    const size_t scratch_bytes = merge_scratch_bytes(c, (uint32_t)rows, karr, iarr, tmp_bytes);
    const bool grow = c->rc_buf.bytes() < rows * sizeof(WRow) || c->m_scratch.bytes() < scratch_bytes || c->m_out[0].bytes() < rows * sizeof(RowApp);
    if (grow) (void)hipStreamSynchronize(c->stream);  // (ensure_dev frees what it replaces)
    (void)ensure_dev(c, c->rc_buf, rows * sizeof(WRow), "wide rows");
    (void)ensure_dev(c, c->m_scratch, scratch_bytes, "merge scratch");
    (void)ensure_dev(c, c->m_out[0], rows * sizeof(RowApp), "merged rows");
    if (rows >= APP48_SPLIT_MIN) {  // (fa_read_window_app48 in two halves: the cut rows and the packed ones)
        (void)ensure_dev(c, c->cut_buf, rows * sizeof(RowApp), "cut rows");
        (void)ensure_dev(c, c->m_out[1], rows * sizeof(RowApp48), "packed rows");
    }
    (void)ensure_pinned(c, rows * sizeof(RowApp));
    if (c->group_members > 1) {
        // a member of a group (fa_group_*): its window leaves hash-partitioned - the rows regrouped by owner, and about as many
        // rows again received from the other members
        (void)ensure_dev(c, c->part_buf, rows * sizeof(RowApp), "partitioned rows");
        (void)ensure_dev(c, c->xch_buf, rows * sizeof(RowApp), "group exchange buffer");
        if (!c->part_cnt.grow(3 * RPART_MAX_WORLD * sizeof(unsigned int))) (void)hipGetLastError();
    }
    if (rows >= APP48_SPLIT_MIN && !c->copy_stream && hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) == hipSuccess && c->h_rows && c->m_out[1]) {
        // (a stream's first copy sets its engine up: 3 ms inside the first window read otherwise)
        (void)hipMemcpyAsync(c->h_rows, c->m_out[1], 4096, hipMemcpyDeviceToHost, c->copy_stream);
        (void)hipStreamSynchronize(c->copy_stream);
    }
    c->err = keep;
}
template <int KIND>
static int rows_merge_t(fa_ctx* c, hipStream_t stream, ReadClock& clk, const void* d_rows, size_t n_in, uint32_t fold, size_t k, const void** out, size_t* n_out,
                        bool to_host = false, bool* in_host = nullptr) {
    typedef typename RowOps<KIND>::Row Row;
    typedef RowOps<KIND> Ops;
    if (in_host) *in_host = false;
    *out = nullptr;
    *n_out = 0;
    if (n_in == 0) return FA_OK;
    if (n_in >= (1ull << 31) - 1024) return fail(c, FA_ERR_ARG, "too many rows for one merge (2^31)");
    const uint32_t n = (uint32_t)n_in;
    const Row* rows = (const Row*)d_rows;
    // (the caller's rows may be this ctx's own result of an earlier call - one rank feeding fa_rows_device's pointer back
    // in: the buffers below are about to be reused)
    if (inside(c->m_out[0], d_rows) || inside(c->m_out[1], d_rows)) return fail(c, FA_ERR_ARG, "rows to merge alias the ctx's result buffer (copy them first)");
    size_t karr, iarr, tmp_bytes;
    const size_t scratch_bytes = merge_scratch_bytes(c, n, karr, iarr, tmp_bytes);
    int rc = ensure_dev(c, c->m_scratch, scratch_bytes, "merge scratch");
    if (rc) return rc;
    uint8_t* base = (uint8_t*)c->m_scratch;
    SortScratch ss;
    ss.ka = (unsigned long long*)base;
    ss.kb = (unsigned long long*)(base + karr);
    ss.ia = (uint32_t*)(base + 2 * karr);
    ss.ib = (uint32_t*)(base + 2 * karr + iarr);
    uint32_t* flags = (uint32_t*)(base + 2 * karr + 2 * iarr);
    uint32_t* pos = (uint32_t*)(base + 2 * karr + 3 * iarr);
    ss.tmp = base + 2 * karr + 4 * iarr;
    ss.tmp_bytes = tmp_bytes;
    ss.bits = (unsigned long long*)(base + 2 * karr + 4 * iarr + tmp_bytes);
    void* tmp = ss.tmp;
    const dim3 g = grid_n(n), b(256);
    uint32_t* cur = nullptr;
    uint32_t sorted_bits = 0;
    rc = rows_sort_order<KIND, false>(c, stream, rows, n, fold, ss, &cur, &sorted_bits);
    if (rc) return rc;
    if (clk.on) {
        char what[32];
        snprintf(what, sizeof what, "sort(%u bits)", sorted_bits);
        clk.mark(what, stream);
    }
    hipLaunchKernelGGL((row_heads_kernel<KIND>), g, b, 0, stream, rows, (const uint32_t*)cur, n, fold, flags);
    {
        size_t tb = tmp_bytes;
        if (hipcub::DeviceScan::ExclusiveSum(tmp, tb, flags, pos, (int)n, stream) != hipSuccess) return fail(c, FA_ERR_HIP, "scan failed");
    }
    uint32_t last[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&last[0], flags + (n - 1), 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipMemcpyAsync(&last[1], pos + (n - 1), 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    clk.mark("heads+scan", stream);
    const uint32_t m = last[0] + last[1];  // groups
    const size_t m_emit = (k && k < m) ? k : m;
    const bool host = to_host && c->h_rows && m_emit * sizeof(Row) <= c->h_rows.bytes();
    rc = ensure_dev(c, c->m_out[0], (size_t)m * sizeof(Row), "merged rows");
    if (rc) return rc;
    // the groups' rows: heads sum the first RUN_SERIAL rows of their run; longer runs (a caller's degenerate input, or a talker
    // key held in more than RUN_SERIAL buckets of a range) are finished with atomics by a second kernel, which needs the rows in
    // device memory and costs one more read of a device word
    unsigned int* long_runs = &c->d_ctr->rows_count;
    HIPCHK(c, zero_word(long_runs, stream));
    auto reduce_into = [&](Row* dst) -> int {
        hipLaunchKernelGGL((row_reduce_kernel<KIND>), g, b, 0, stream, rows, (const uint32_t*)cur, (const uint32_t*)flags, (const uint32_t*)pos, n, fold, dst, long_runs);
        HIPCHK(c, hipGetLastError());
        return FA_OK;
    };
    auto finish_long_runs = [&](Row* dst) -> int {  // dst: device memory
        unsigned int lr = 0;
        HIPCHK(c, read_word(long_runs, lr, stream));
        if (lr) {
            hipLaunchKernelGGL((row_tail_kernel<KIND>), g, b, 0, stream, rows, (const uint32_t*)cur, (const uint32_t*)flags, (const uint32_t*)pos, n, dst);
            HIPCHK(c, hipGetLastError());
        }
        return FA_OK;
    };
    const bool may_be_long = n > m && (uint64_t)n >= (uint64_t)RUN_SERIAL;  // (a run of RUN_SERIAL rows needs at least that many rows)
    // a kind without an emit order is done with the reduce: straight into the pinned host buffer when no run can be long (the
    // atomics of row_tail_kernel want device memory)
    constexpr bool QUERY = KIND == RK_QUERY_WEIGHT || KIND == RK_QUERY_KEY;  // (NK2 == 0, yet ordered behind the reduce)
    Row* red = (Ops::NK2 == 0 && !QUERY && host && m_emit == m && !may_be_long) ? (Row*)c->h_rows : (Row*)c->m_out[0];
    rc = reduce_into(red);
    if (rc) return rc;
    if (may_be_long) {
        rc = finish_long_runs(red);
        if (rc) return rc;
    }
    clk.mark("reduce", stream);
    Row* dst = red;
    if constexpr (KIND == RK_TALKERS_SRC || KIND == RK_TALKERS_DST) {  // emit order by the talkers' own sorts (talk_order_rows)
        rc = ensure_dev(c, c->m_out[1], m_emit * sizeof(Row), "ordered rows");
        if (rc) return rc;
        dst = host ? (Row*)c->h_rows : (Row*)c->m_out[1];
        rc = talk_order_rows(c, stream, (const Row*)red, m, m_emit, dst);
        if (rc) return rc;
        clk.mark("emit order", stream);
    } else if constexpr (KIND == RK_QUERY_WEIGHT || KIND == RK_QUERY_KEY) {  // fa_raw_query_rows' order by fa_raw_query_rows' passes (merge.cuh, RowOpsQuery)
        DevBuf<>* order = nullptr;
        rc = query_order_scratch(c, &order);
        if (!rc) rc = ensure_dev(c, c->m_out[1], m_emit * sizeof(Row), "ordered rows");
        if (rc) return rc;
        dst = (Row*)c->m_out[1];  // (never the pinned buffer: a kernel rewrites the rows behind the order)
        hipLaunchKernelGGL(query_rows_key_kernel<true>, grid_n(m), b, 0, stream, red, m);
        rc = talk_order_passes(c, stream, *order, (const Row*)red, m, m_emit, dst, KIND == RK_QUERY_WEIGHT ? 4 : 3);
        if (rc) return rc;
        hipLaunchKernelGGL(query_rows_key_kernel<false>, grid_n(m_emit), b, 0, stream, dst, (uint32_t)m_emit);
        HIPCHK(c, hipGetLastError());
        clk.mark("emit order", stream);
    } else if constexpr (Ops::NK2 > 0) {  // emit order: a second sort over the groups
        uint32_t* cur2 = nullptr;
        rc = rows_sort_order<KIND, true>(c, stream, (const Row*)red, m, fold, ss, &cur2, &sorted_bits);
        if (rc) return rc;
        rc = ensure_dev(c, c->m_out[1], m_emit * sizeof(Row), "ordered rows");
        if (rc) return rc;
        dst = host ? (Row*)c->h_rows : (Row*)c->m_out[1];
        hipLaunchKernelGGL((row_gather_kernel<Row>), grid_n(m_emit), b, 0, stream, (const Row*)red, (const uint32_t*)cur2, (uint32_t)m_emit, dst);
        HIPCHK(c, hipGetLastError());
        clk.mark("emit order", stream);
    }
    if (in_host) *in_host = dst == (Row*)c->h_rows;
    *out = dst;
    *n_out = m_emit;
    return FA_OK;
}

static int rows_merge(fa_ctx* c, hipStream_t stream, ReadClock& clk, int kind, const void* d_rows, size_t n, uint32_t fold, size_t k, const void** out, size_t* n_out,
                      bool to_host = false, bool* in_host = nullptr) {
    int rc = FA_OK;
    const bool known = with_row_kind(kind, [&](auto rk) { rc = rows_merge_t<decltype(rk)::value>(c, stream, clk, d_rows, n, fold, k, out, n_out, to_host, in_host); });
    return known ? rc : fail(c, FA_ERR_ARG, "unknown row kind");
}

// the talker kinds live in talkers_host.inc (TalkState, a TabPair of keytab_host.inc): is the state there, its collector, and its
// row buffer
static bool is_talker_kind(int kind) { return kind == RK_TALKERS_SRC || kind == RK_TALKERS_DST; }
static const char TALK_OFF[] = "top talkers are not enabled on this ctx (fa_talkers_enable)";
static const char TALK_NOT_CANONICAL[] = "fa_merge_talkers: a row is not canonical (etype 0 or 0x800; bytes 4..15 zero under 0x800)";
static int collect_talkers(fa_ctx* c, ReadClock& clk, int kind, const BucketRange* range, const void*& in, size_t& n);
static bool talk_rows_hold(const fa_ctx* c, const void* p);
static const char TALK_NOT_BUCKETED[] = "the ctx's top talkers have no time axis (fa_talkers_enable_buckets)";
static uint32_t talk_bucket_secs(const fa_ctx* c);  // 0: not enabled, or plain tables
// the bucketed port tables live in ports_host.inc (PortState): the port kinds' RANGED reads collect from them - and from nothing
// else; the un-ranged reads never look at them
static const char PORT_OFF[] = "bucketed port tables are not enabled on this ctx (fa_ports_enable_buckets)";
static int collect_ports_range(fa_ctx* c, ReadClock& clk, int kind, const BucketRange& range, const void*& in, size_t& n);
static uint32_t port_bucket_secs(const fa_ctx* c);  // 0: not enabled

static int kind_enabled(fa_ctx* c, int kind) {
    switch (kind) {
    case RK_5M: return FA_OK;
    case RK_APP: return (c->cfg.key_sets & FA_KEYS_ADDR_PORT_PROTO) ? FA_OK : fail(c, FA_ERR_ARG, "FA_KEYS_ADDR_PORT_PROTO not enabled");
    case RK_PORT_SRC: case RK_PORT_DST: return c->port_hist ? FA_OK : fail(c, FA_ERR_ARG, "FA_KEYS_PORT_HIST not enabled");
    case RK_MINUTE: return (c->cfg.key_sets & FA_KEYS_MINUTE_SERIES) ? FA_OK : fail(c, FA_ERR_ARG, "FA_KEYS_MINUTE_SERIES not enabled");
    case RK_TOPK_SRC: return c->ks_src ? FA_OK : fail(c, FA_ERR_ARG, "fa_topk: key set not enabled");
    case RK_TOPK_DST: return c->ks_dst ? FA_OK : fail(c, FA_ERR_ARG, "fa_topk: key set not enabled");
    case RK_TALKERS_SRC: case RK_TALKERS_DST: return c->talk ? FA_OK : fail(c, FA_ERR_UNSUPPORTED, TALK_OFF);
    case RK_QUERY_WEIGHT: case RK_QUERY_KEY:
        return fail(c, FA_ERR_UNSUPPORTED, "fa_rows_device: query rows come from fa_raw_query_rows_device (a row kind names no GROUP BY: the call has no place for the group bit)");
    default: return fail(c, FA_ERR_ARG, "unknown row kind");
    }
}

static const char* row_kind_name(int kind) {
    switch (kind) {
    case RK_5M: return "flows_5m";
    case RK_APP: return "(SrcAddr,DstPort,Proto)";
    case RK_PORT_SRC: return "SrcPort";
    case RK_PORT_DST: return "DstPort";
    case RK_MINUTE: return "minutes";
    case RK_TOPK_SRC: return "top-k SrcAddr";
    case RK_TOPK_DST: return "top-k DstAddr";
    case RK_TALKERS_SRC: return "talkers SrcAddr";
    case RK_TALKERS_DST: return "talkers DstAddr";
    case RK_QUERY_WEIGHT: return "query rows by weight";
    case RK_QUERY_KEY: return "query rows by key";
    default: return "unknown";
    }
}

// (SrcAddr,DstPort,Proto) rows of the buckets [lo, hi): the wide table's (and the pending chunks') rows, unpacked in place
static int collect_app(fa_ctx* c, ReadClock& clk, uint32_t lo, uint32_t hi, const void*& in, size_t& n) {
    int rc = collect_wide_raw(c, clk, 1u << WK_APP, lo, hi, n);
    if (rc) return rc;
    if (n) hipLaunchKernelGGL(wrows_to_app_kernel, grid_n(n), dim3(256), 0, c->stream, (WRow*)c->rc_buf, (uint32_t)n, c->gran);
    in = c->rc_buf;
    return FA_OK;
}
// GROUP BY port / the minute series: the wide table's rows as RowW in c->rw_buf, the dense ports' rows behind them
static int collect_w(fa_ctx* c, ReadClock& clk, int kind, const void*& in, size_t& n) {
    const bool port = kind != RK_MINUTE;
    const int dst = kind == RK_PORT_DST;
    int rc = collect_wide_raw(c, clk, 1u << (kind == RK_MINUTE ? WK_MINUTE : dst ? WK_DSTPORT : WK_SRCPORT), 0, 0, n);
    if (rc) return rc;
    const size_t cap_rows = n + (port ? PORT_DENSE : 0) + 16;
    rc = ensure_dev(c, c->rw_buf, cap_rows * sizeof(RowW), "port / minute rows");
    if (rc) return rc;
    if (n) hipLaunchKernelGGL(wrows_to_w_kernel, grid_n(n), dim3(256), 0, c->stream, (const WRow*)c->rc_buf, (uint32_t)n, port ? 1u : 60u, (RowW*)c->rw_buf);
    if (port) {
        HIPCHK(c, zero_word(&c->d_ctr->rows_count, c->stream));
        hipLaunchKernelGGL(port_dense_rows_kernel, dim3(64), dim3(256), 0, c->stream, c->port_hist + (size_t)dst * PORT_DENSE, (uint32_t)PORT_DENSE,
                           (RowW*)c->rw_buf + n, &c->d_ctr->rows_count);
        unsigned int nd = 0;
        HIPCHK(c, read_word(&c->d_ctr->rows_count, nd, c->stream));
        n += nd;
    }
    in = c->rw_buf;
    return FA_OK;
}

// ---- fa_topk's collection: k rows out of millions - only the rows that can be among the first k leave the set ----------
struct TopkSet {  // one direction's distinct-address set and the sketch its estimates come from
    KeySlot* ks;
    const unsigned long long* cms;
    uint32_t nslots;
};
// ONE scan of the whole set: the rows whose estimate reaches lb_bin (0: every row) into c->rc_buf, room for cap_rows of them
// (almost every key stops at its row-0 counter) -> how many there were (more than cap_rows: the caller's call)
static int topk_scan_rows(fa_ctx* c, const TopkSet& t, uint32_t lb_bin, size_t cap_rows, unsigned int& nr) {
    int rc = ensure_dev(c, c->rc_buf, cap_rows * sizeof(TopkRow), "top-k rows");
    if (rc) return rc;
    HIPCHK(c, zero_word(&c->d_ctr->ks_rows, c->stream));
    hipLaunchKernelGGL(topk_scan_kernel<TK_ONE>, dim3(1024), dim3(256), 0, c->stream, t.ks, t.nslots, t.cms, c->cfg.cms_depth, c->cfg.cms_width_log2, c->cfg.cms_seed, lb_bin,
                       (unsigned int*)nullptr, (unsigned short*)nullptr, (TopkRow*)c->rc_buf, (uint32_t)cap_rows, c->d_ctr);
    HIPCHK(c, read_word(&c->d_ctr->ks_rows, nr, c->stream));
    return FA_OK;
}
// histogram of the estimates' bins over the first ns slots (grid workgroups), then the bin that holds rank sel_k:
// sel[0] that bin, sel[1] the rows in the bins >= it, sel[2] the rows held; the chunks' largest bins are left in c->rw_buf
static int topk_threshold(fa_ctx* c, const TopkSet& t, uint32_t ns, unsigned grid, size_t sel_k, unsigned int (&sel)[3], const unsigned short** chunkmax) {
    const size_t cm_bytes = align256((size_t)(ns >> 6) * sizeof(unsigned short));
    int rc = ensure_dev(c, c->rw_buf, (TK_BINS + 4) * sizeof(unsigned int) + cm_bytes, "top-k histogram");
    if (rc) return rc;
    unsigned int* hist = (unsigned int*)c->rw_buf;
    unsigned short* cmax = (unsigned short*)(hist + TK_BINS + 4);
    HIPCHK(c, hipMemsetAsync(hist, 0, (TK_BINS + 4) * sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(topk_scan_kernel<TK_HIST>, dim3(grid), dim3(256), 0, c->stream, t.ks, ns, t.cms, c->cfg.cms_depth, c->cfg.cms_width_log2, c->cfg.cms_seed, 0u, hist, cmax,
                       (TopkRow*)nullptr, 0u, c->d_ctr);
    hipLaunchKernelGGL(topk_thresh_kernel, dim3(1), dim3(256), 0, c->stream, (const unsigned int*)hist, (uint32_t)sel_k, hist + TK_BINS);
    HIPCHK(c, hipMemcpyAsync(sel, hist + TK_BINS, sizeof sel, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *chunkmax = cmax;
    return FA_OK;
}
// The rows that can be among the first sel_k (k: what the caller asked for; sel_k > k: a retry, see rows_local), tried in
// this order - each arm that does not settle it falls through to the next:
//  1. a bin the k-th estimate is known to reach (the k-th row of an earlier read of this sketch and view: estimates and sets
//     only grow): ONE scan;
//  2. no such bin (a first read, a new view, a larger k) and a set of 2^18 slots or more: the k-th estimate of a SAMPLE is a
//     lower bound of the k-th estimate of the set - the first 1 / 64 of the slots hold a hash-uniform 1 / 64 of the keys - and
//     one scan of the whole set with that bin replaces the full-depth scan (40 M random sketch reads on BASELINE config 3's sets);
//  3. histogram of the estimates' bins -> the bin that holds rank k -> the rows of that bin and above, found through the
//     chunks' largest bins;
//  4. every row (k = 0, k >= the slots).
// partial: rows were left behind.
static int collect_topk(fa_ctx* c, ReadClock& clk, int kind, size_t k, size_t sel_k, bool& partial, const void*& in, size_t& n) {
    const int d = kind == RK_TOPK_DST;
    int rc = settle(c);
    if (rc) return rc;
    if (c->h_ctr->ks_overflow) return fail(c, FA_ERR_TABLE_FULL, "fa_topk: distinct-address set overflowed (raise topk_capacity_log2)");
    const TopkSet t{d ? c->ks_dst : c->ks_src, cms_of(c, d ? FA_KEYS_DSTADDR_CMS : FA_KEYS_SRCADDR_CMS), 1u << c->ks_log2};
    const bool merged_now = c->merged_valid && (d ? c->cms_dst_m : c->cms_src_m) != nullptr;
    const bool lb_ok = c->tk_lb_k[d] != 0 && sel_k != 0 && sel_k <= c->tk_lb_k[d] && c->tk_lb_merged[d] == merged_now && sel_k == k;
    partial = false;
    unsigned int nr = 0, sel[3] = {0, 0, 0};
    const unsigned short* chunkmax = nullptr;
    bool done = false;
    if (lb_ok) {
        const size_t cap_rows = std::max<size_t>(8 * sel_k, 1u << 16);
        rc = topk_scan_rows(c, t, c->tk_lb_bin[d], cap_rows, nr);
        if (rc) return rc;
        done = nr <= cap_rows && nr >= sel_k;  // (more rows than room, or fewer than k - a reset nobody told us about: the long way)
        partial = true;
        if (!done) c->tk_lb_k[d] = 0;
        clk.mark("one pass");
    }
    if (!done && sel_k && sel_k == k && sel_k <= 4096 && t.nslots >= (1u << 18)) {
        rc = topk_threshold(c, t, t.nslots >> 6, 256, sel_k, sel, &chunkmax);
        if (rc) return rc;
        clk.mark("sample");
        if (sel[2] >= sel_k && sel[0] > 0) {
            const size_t cap_rows = std::max<size_t>(256 * sel_k, 1u << 16);
            rc = topk_scan_rows(c, t, sel[0], cap_rows, nr);
            if (rc) return rc;
            done = nr <= cap_rows;  // (a stream whose estimates crowd one bin: the histogram of the whole set decides)
            partial = true;
            clk.mark("one pass");
        }
    }
    if (!done && sel_k && sel_k < t.nslots) {
        rc = topk_threshold(c, t, t.nslots, 1024, sel_k, sel, &chunkmax);
        if (rc) return rc;
        clk.mark("estimates");
        const size_t cap_rows = std::max<size_t>(sel[1], 1);
        partial = sel[1] < sel[2];
        rc = ensure_dev(c, c->rc_buf, cap_rows * sizeof(TopkRow), "top-k rows");
        if (rc) return rc;
        HIPCHK(c, zero_word(&c->d_ctr->ks_rows, c->stream));
        hipLaunchKernelGGL(topk_pick_kernel, dim3(256), dim3(256), 0, c->stream, (const KeySlot*)t.ks, t.nslots, chunkmax, sel[0], (TopkRow*)c->rc_buf, (uint32_t)cap_rows, c->d_ctr);
        HIPCHK(c, read_word(&c->d_ctr->ks_rows, nr, c->stream));
        if (nr > cap_rows) return fail(c, FA_ERR_HIP, "internal: top-k row buffer too small");
        done = true;
    }
    if (!done) {  // every row
        rc = topk_scan_rows(c, t, 0u, t.nslots, nr);
        if (rc) return rc;
    }
    in = c->rc_buf;
    n = nr;
    return FA_OK;
}

// The ctx's own result for (kind, timeslot): what the matching read call returns, left in HBM (or, to_host, written
// straight into the pinned host buffer when it fits): the window, then collect, then merge.
// (range: the ranged reads of the talker kinds and of the port kinds - where the rows come from is the only difference: a
// bucketed table of talkers_host.inc / ports_host.inc instead of the kind's un-ranged state)
static int rows_local(fa_ctx* c, ReadClock& clk, int kind, uint32_t timeslot, size_t k, const void** out, size_t* n_out, bool to_host = false, bool* in_host = nullptr,
                      const BucketRange* range = nullptr) {
    *out = nullptr;
    *n_out = 0;
    if (in_host) *in_host = false;
    const bool ports_ranged = range && (kind == RK_PORT_SRC || kind == RK_PORT_DST);
    int rc = ports_ranged ? (c->ports ? FA_OK : fail(c, FA_ERR_UNSUPPORTED, PORT_OFF)) : kind_enabled(c, kind);
    if (rc) return rc;
    Window w;
    if ((kind == RK_5M || kind == RK_APP) && !window_of(c, timeslot, w)) return FA_OK;  // not a bucket boundary: no rows
    const bool topk = kind == RK_TOPK_SRC || kind == RK_TOPK_DST;
    const int d = kind == RK_TOPK_DST;
    const void* in = nullptr;
    size_t n = 0;
    // top-k kinds: sel_k rows the collection has to keep, and whether it left rows behind.  The distinct-address set may (rarely)
    // hold a key twice (sinks.cuh, keyset_step): the merge keeps it once, and when that leaves fewer than k rows although the
    // collection cut some off, it collects again with more room.
    size_t sel_k = k;
    bool sel_partial = false, again;
    do {
        switch (kind) {
        case RK_5M: rc = collect_5m(c, clk, w.lo, w.hi, in, n); break;
        case RK_APP: rc = collect_app(c, clk, w.lo, w.hi, in, n); break;
        case RK_PORT_SRC: case RK_PORT_DST: case RK_MINUTE: rc = ports_ranged ? collect_ports_range(c, clk, kind, *range, in, n) : collect_w(c, clk, kind, in, n); break;
        case RK_TOPK_SRC: case RK_TOPK_DST: rc = collect_topk(c, clk, kind, k, sel_k, sel_partial, in, n); break;
        case RK_TALKERS_SRC: case RK_TALKERS_DST: rc = collect_talkers(c, clk, kind, range, in, n); break;  // (a plain table holds a key once and k only cuts; a bucketed one once per bucket: the merge sums)
        default: return fail(c, FA_ERR_ARG, "unknown row kind");
        }
        if (rc) return rc;
        HIPCHK(c, hipGetLastError());
        clk.mark("collect");
        rc = rows_merge(c, c->stream, clk, kind, in, n, w.fold, k, out, n_out, to_host, in_host);
        again = !rc && topk && k && *n_out < k && sel_partial;
        if (again) {
            sel_k = std::max<size_t>(2 * sel_k, sel_k + 64);
            c->tk_lb_k[d] = 0;
        }
    } while (again);
    if (!rc && topk && k && *n_out == k) {
        // the k-th row's estimate: a bin every later read of this sketch and view (for k' <= k) knows its k'-th estimate reaches
        unsigned long long weight = 0;
        HIPCHK(c, hipMemcpyAsync(&weight, (const uint8_t*)*out + (k - 1) * sizeof(TopkRow) + offsetof(TopkRow, weight), sizeof weight, hipMemcpyDefault, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->tk_lb_bin[d] = topk_bin(weight);
        c->tk_lb_k[d] = k;
        c->tk_lb_merged[d] = c->merged_valid && (d ? c->cms_dst_m : c->cms_src_m) != nullptr;
    }
    clk.n_in = n;
    return rc;
}

// host copy on a few threads (one thread moves ~10 GB/s; the destination is the caller's pageable memory, often untouched)
static std::atomic<int> g_copyout_active{0};  // threads of this process inside a host-side row copy (a group's members fetch at the same time)
static void copy_threads(fa_ctx* c, void* dst, const void* src, size_t bytes) {
    struct Active {
        int n;
        Active() : n(g_copyout_active.fetch_add(1, std::memory_order_relaxed) + 1) {}
        ~Active() { g_copyout_active.fetch_sub(1, std::memory_order_relaxed); }
    } active;
    // (the team shrinks with the callers: 8 members x 8 threads on a 16-CPU cgroup only get throttled)
    const unsigned team = std::max(1u, std::min(c->stage_threads, usable_cpus() / (unsigned)active.n));
    unsigned nthr = bytes < ((size_t)4 << 20) ? 1u : std::min<unsigned>(team, (unsigned)(bytes >> 20));
    if (nthr <= 1) {
        memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> pool;
    auto work = [&](unsigned t) {
        const size_t b0 = (bytes * t / nthr) & ~(size_t)63, b1 = t + 1 == nthr ? bytes : (bytes * (t + 1) / nthr) & ~(size_t)63;
        if (b1 > b0) memcpy((uint8_t*)dst + b0, (const uint8_t*)src + b0, b1 - b0);
    };
    for (unsigned t = 1; t < nthr; t++) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
}
// `bytes` from HBM into the caller's (pageable) buffer.  A plain hipMemcpy into pageable memory runs at ~9 GB/s - a 930 MB
// window of (SrcAddr,DstPort,Proto) rows spent 100 of its 112-149 ms there (round 3).  Large results go through the ctx's
// pinned buffer in two halves: the copy engine fills one half (57 GB/s) while the host threads empty the other.
// is [p, p + bytes) host memory the copy engine can write directly (hipHostMalloc'd or hipHostRegister'ed by the caller)?
static bool host_pinned(const void* p, size_t bytes) {
    hipPointerAttribute_t at{};
    const bool yes = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost;
    bool end_too = yes;
    if (yes && bytes > 1) {  // (a registration may end inside the buffer: both ends have to be pinned)
        hipPointerAttribute_t ae{};
        end_too = hipPointerGetAttributes(&ae, (const uint8_t*)p + bytes - 1) == hipSuccess && ae.type == hipMemoryTypeHost;
    }
    (void)hipGetLastError();  // (pageable memory is reported as an error by some runtimes: not ours to keep)
    return yes && end_too;
}
static int copy_out_pipelined(fa_ctx* c, void* out, const void* d, size_t bytes) {
    // A caller that pinned its buffer gets ONE copy by the copy engine, no staging and no host threads: the link's 57 GB/s
    // instead of the 54 GB/s the two-slot relay below reaches into pageable memory (a 928 MB window of config 5: 16.3 ms
    // instead of 17.1) - and none of the host's cores.
    if (bytes >= ((size_t)1 << 20) && host_pinned(out, bytes)) {
        HIPCHK(c, hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return FA_OK;
    }
    const size_t half = (c->h_rows.bytes() / 2) & ~(size_t)4095;
    if (!c->h_rows || bytes < ((size_t)8 << 20) || half < ((size_t)4 << 20)) {
        HIPCHK(c, hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
        return FA_OK;
    }
    uint8_t* slot[2] = {(uint8_t*)c->h_rows, (uint8_t*)c->h_rows + half};
    const size_t npieces = (bytes + half - 1) / half;
    auto piece_bytes = [&](size_t i) { return std::min(half, bytes - i * half); };
    HIPCHK(c, hipMemcpyAsync(slot[0], d, piece_bytes(0), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->copy_ev[0], c->stream));
    for (size_t i = 0; i < npieces; i++) {
        if (i + 1 < npieces) {  // (slot (i + 1) & 1 was emptied by the host in the previous round)
            HIPCHK(c, hipMemcpyAsync(slot[(i + 1) & 1], (const uint8_t*)d + (i + 1) * half, piece_bytes(i + 1), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipEventRecord(c->copy_ev[(i + 1) & 1], c->stream));
        }
        HIPCHK(c, hipEventSynchronize(c->copy_ev[i & 1]));
        copy_threads(c, (uint8_t*)out + i * half, slot[i & 1], piece_bytes(i));
    }
    return FA_OK;
}
// the pinned buffer grows with the results up to 64 MiB (the last kernel of a read then writes straight into it); larger
// results stay in HBM and leave through it in pieces (copy_out_pipelined) - pinning a gigabyte costs more than the copy
static int ensure_pinned(fa_ctx* c, size_t result_bytes) {
    constexpr size_t PIN_MAX = (size_t)64 << 20;
    const size_t want = std::min(PIN_MAX, result_bytes + result_bytes / 4 + 4096);
    if (c->h_rows.bytes() >= want) return FA_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)c->h_rows.grow(want);  // (a failure is not an error: the copy falls back to a plain hipMemcpy)
    return FA_OK;
}
// the rows behind `d` (device, or the pinned host buffer) into the caller's buffer
static int rows_copy_out(fa_ctx* c, const void* d, size_t n, size_t row_bytes, bool in_host, void* out, size_t cap, size_t* n_out) {
    *n_out = n;
    if (n > cap) return fail(c, FA_ERR_CAPACITY, "output buffer too small");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!n) return FA_OK;
    if (in_host) {
        copy_threads(c, out, d, n * row_bytes);
        return FA_OK;
    }
    return copy_out_pipelined(c, out, d, n * row_bytes);
}
static int rows_read(fa_ctx* c, int kind, uint32_t timeslot, size_t k, void* out, size_t cap, size_t* n_out, const BucketRange* range = nullptr) {
    const void* d = nullptr;
    size_t n = 0;
    bool in_host = false;
    ReadClock clk(c);
    int rc = rows_local(c, clk, kind, timeslot, k, &d, &n, true, &in_host, range);
    if (rc) return rc;
    if (n > cap) {  // (the caller asks again with room for *n_out rows; nothing was removed)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *n_out = n;
        return fail(c, FA_ERR_CAPACITY, "output buffer too small");
    }
    if (n && !in_host) {
        rc = ensure_pinned(c, n * row_bytes_of(kind));
        if (rc) return rc;
    }
    rc = rows_copy_out(c, d, n, row_bytes_of(kind), in_host, out, cap, n_out);
    clk.mark("copy out");
    clk.done(row_kind_name(kind), clk.n_in, n);
    return rc;
}

// one window's (SrcAddr,DstPort,Proto) rows as 48-byte rows (fa_row_app48): the merged rows are repacked in HBM - into the buffer
// the read collected its input in, dead by now - and leave like any other result
static int rows_read_app48_whole(fa_ctx* c, const void* d, size_t n, void* out, size_t cap, size_t* n_out, ReadClock& clk) {
    int rc = ensure_dev(c, c->rc_buf, n * sizeof(RowApp48), "packed rows");
    if (rc) return rc;
    hipLaunchKernelGGL(row_app48_kernel, grid_n(n), dim3(256), 0, c->stream, (const RowApp*)d, (uint32_t)n, (RowApp48*)c->rc_buf);
    HIPCHK(c, hipGetLastError());
    clk.mark("pack");
    rc = ensure_pinned(c, n * sizeof(RowApp48));
    if (rc) return rc;
    rc = rows_copy_out(c, c->rc_buf, n, sizeof(RowApp48), false, out, cap, n_out);
    clk.mark("copy out");
    return rc;
}
// A large window into PAGE-LOCKED memory: the copy over PCIe (14 ms for 16.6 M rows) is as long as everything in front of it, so the
// rows are cut in two by key - below / not below the median of a sample of their most significant key word - and the first half's
// sorted, summed, packed rows leave on a second stream while the second half is sorted: both halves are in emit order and every key
// of the first lies below every key of the second, so back to back they are what the one-piece read returns.  (A caller's pageable
// buffer goes through the pinned relay and host threads instead: rows_read_app48_whole.)  FA_APP48_SPLIT=0: never.
static int rows_read_app48_split(fa_ctx* c, size_t n, uint32_t fold, void* out, size_t cap, size_t* n_out, ReadClock& clk) {
    const RowApp* rows = (const RowApp*)c->rc_buf;
    // the pivot: median of 2048 sampled keys (a window of one address block, or of fewer rows than samples, still works - one half is
    // then small or empty)
    constexpr uint32_t NS = 2048;
    size_t karr, iarr, tmp_bytes;
    const size_t scratch_bytes = merge_scratch_bytes(c, (uint32_t)n, karr, iarr, tmp_bytes);
    int rc = ensure_dev(c, c->m_scratch, scratch_bytes, "merge scratch");
    if (rc) return rc;
    unsigned long long* d_keys = (unsigned long long*)c->m_scratch;
    hipLaunchKernelGGL(app_key_sample_kernel, dim3(NS / 256), dim3(256), 0, c->stream, rows, (uint32_t)n, (uint32_t)(n / NS), d_keys, NS);
    std::vector<unsigned long long> keys(NS);
    HIPCHK(c, hipMemcpyAsync(keys.data(), d_keys, NS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::nth_element(keys.begin(), keys.begin() + NS / 2, keys.end());
    const unsigned long long pivot = keys[NS / 2];
    rc = ensure_dev(c, c->cut_buf, n * sizeof(RowApp), "cut rows");
    if (rc) return rc;
    unsigned int* d_cnt = (unsigned int*)c->m_scratch;  // (two words; the sample has been read)
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(app_cut_kernel, dim3(1024), dim3(APP_CUT_BLOCK), 0, c->stream, rows, (uint32_t)n, pivot, (RowApp*)c->cut_buf, d_cnt);
    HIPCHK(c, hipGetLastError());
    unsigned int na = 0;
    HIPCHK(c, read_word(d_cnt, na, c->stream));
    clk.mark("cut");
    rc = ensure_dev(c, c->m_out[1], n * sizeof(RowApp48), "packed rows");  // (at most n rows come out)
    if (rc) return rc;
    if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    RowApp48* packed = (RowApp48*)c->m_out[1];
    size_t done = 0;
    const size_t part_n[2] = {na, n - na};
    // The copies stay on the ctx's own stream (its copy engine knows the caller's pages: on a second stream the first window's copy
    // took 3 ms longer); the SECOND half's kernels run on the other stream, behind the first half's (they share the merge scratch).
    hipStream_t const main_stream = c->stream;
    for (int h = 0; h < 2; h++) {
        if (!part_n[h]) continue;
        const void* d = nullptr;
        size_t m = 0;
        hipStream_t const on = h ? c->copy_stream : main_stream;
        if (h) HIPCHK(c, hipStreamWaitEvent(on, c->copy_ev[0], 0));  // (behind the first half's pack; recorded below, or never: no first half)
        rc = rows_merge(c, on, clk, RK_APP, (const RowApp*)c->cut_buf + (h ? na : 0), part_n[h], fold, 0, &d, &m);
        if (!rc && done + m <= cap) {
            hipLaunchKernelGGL(row_app48_kernel, grid_n(m), dim3(256), 0, on, (const RowApp*)d, (uint32_t)m, packed + done);
            if (hipGetLastError() != hipSuccess || hipEventRecord(c->copy_ev[h], on) != hipSuccess) rc = fail(c, FA_ERR_HIP, "pack of a half failed");
        }
        if (rc) break;
        if (done + m > cap) {  // (what has left already is the front of the result; the caller asks again with room for every row)
            (void)hipStreamSynchronize(main_stream);
            *n_out = done + m + (h == 0 ? part_n[1] : 0);  // (an upper bound is all the caller needs)
            return fail(c, FA_ERR_CAPACITY, "output buffer too small");
        }
        if (h) HIPCHK(c, hipStreamWaitEvent(main_stream, c->copy_ev[1], 0));
        HIPCHK(c, hipMemcpyAsync((RowApp48*)out + done, packed + done, m * sizeof(RowApp48), hipMemcpyDeviceToHost, main_stream));
        done += m;
    }
    const hipError_t e = hipStreamSynchronize(main_stream);
    (void)hipStreamSynchronize(c->copy_stream);
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, FA_ERR_HIP, "copy of the packed rows failed");
    clk.mark("pack + copy out");
    *n_out = done;
    return FA_OK;
}
static int rows_read_app48(fa_ctx* c, uint32_t timeslot, void* out, size_t cap, size_t* n_out, uint32_t* date_out) {
    if (timeslot == 0xFFFFFFFFu) return fail(c, FA_ERR_ARG, "fa_read_window_app48: one window at a time (its rows share date and timeslot)");
    int rc = kind_enabled(c, RK_APP);
    if (rc) return rc;
    *n_out = 0;
    if (date_out) *date_out = timeslot / 86400u;
    Window w;
    if (!window_of(c, timeslot, w)) return FA_OK;  // not a bucket boundary: no rows
    ReadClock clk(c);
    const void* in = nullptr;
    size_t n = 0;
    rc = collect_app(c, clk, w.lo, w.hi, in, n);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    clk.mark("collect");
    clk.n_in = n;
    // FA_APP48_SPLIT=0: never in two halves; =<rows>: from that many rows on (tests; default 2^22)
    size_t split_min = APP48_SPLIT_MIN;
    if (const char* e = getenv("FA_APP48_SPLIT")) split_min = !strcmp(e, "0") ? ~(size_t)0 : std::max<size_t>(4096, strtoull(e, nullptr, 0));
    if (n >= split_min && n < ((size_t)1 << 31) - 1024 && cap && host_pinned(out, cap * sizeof(RowApp48))) {
        rc = rows_read_app48_split(c, n, w.fold, out, cap, n_out, clk);
        clk.done("(SrcAddr,DstPort,Proto) 48-byte rows, in two halves", clk.n_in, *n_out);
        return rc;
    }
    const void* d = nullptr;
    size_t m = 0;
    rc = rows_merge(c, c->stream, clk, RK_APP, in, n, w.fold, 0, &d, &m);
    if (rc) return rc;
    *n_out = m;
    if (m > cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return fail(c, FA_ERR_CAPACITY, "output buffer too small");
    }
    if (!m) return FA_OK;
    rc = rows_read_app48_whole(c, d, m, out, cap, n_out, clk);
    clk.done("(SrcAddr,DstPort,Proto) 48-byte rows", clk.n_in, m);
    return rc;
}

// ---- C-ABI: window close ----------------------------------------------------------------------------------------------
extern "C" int fa_read_window(fa_ctx* c, uint32_t timeslot, fa_row5m* out, size_t cap, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out || (!out && cap)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    static_assert(sizeof(Row5m) == sizeof(fa_row5m), "row layout");
    return rows_read(c, RK_5M, timeslot, 0, out, cap, n_out);
}

// what a close removes: everything for tumbling windows / close-all, only the oldest sub-bucket when windows slide
static int drop_buckets(fa_ctx* c, int kind, uint32_t lo, uint32_t rm_hi, bool time_watermark);
static int drop_window(fa_ctx* c, int kind, uint32_t timeslot) {
    Window w;
    if (!window_of(c, timeslot, w) || w.lo == w.hi) return FA_OK;
    const uint32_t rm_hi = w.fold != 0xFFFFFFFFu ? w.lo + 1 : w.hi;  // (a sliding window's rows are folded: so is what its close removes)
    return drop_buckets(c, kind, w.lo, rm_hi, timeslot != 0xFFFFFFFFu);
}
// removes the buckets [lo, rm_hi) of a windowed row kind
static int drop_buckets(fa_ctx* c, int kind, uint32_t lo, uint32_t rm_hi, bool time_watermark) {
    if (kind == RK_5M) {
        if (time_watermark) c->late_below = std::max(c->late_below, rm_hi);  // (records that still arrive for it are late: stats.records_late)
        return rebuild_table(c, c->cap_log2, lo, rm_hi);
    }
    if (kind == RK_APP) {
        if (!c->wtab) return fail(c, FA_ERR_ARG, "key set not enabled");
        const bool had_log = !c->wlog.empty();
        int rc = wlog_drop(c, lo, rm_hi);  // (log mode: the pending chunks' share of the drop)
        if (rc) return rc;
        if (had_log) {  // the table may hold nothing at all: no scan then
            rc = settle(c);
            if (rc) return rc;
            if (c->stats.wide_used == 0) return FA_OK;
        }
        // the table's share of the drop: the rows' sums are zeroed in place (wdrop_kernel) - no rebuild
        HIPCHK(c, hipMemsetAsync(&c->d_ctr->wrows_count, 0, sizeof(unsigned int), c->stream));
        hipLaunchKernelGGL(wdrop_kernel, dim3(2048), dim3(256), 0, c->stream, c->wtab, 1u << c->wcap_log2, 1u << WK_APP, lo, rm_hi, &c->d_ctr->wrows_count);
        HIPCHK(c, hipGetLastError());
        unsigned int dropped = 0;
        HIPCHK(c, hipMemcpyAsync(&dropped, &c->d_ctr->wrows_count, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        // (a heuristic, upper bound: a dead slot that a late record revives still counts, and a second close of its bucket counts it
        // again - settle_wide / wlog_make_room then see fewer live rows than there are and may rebuild once at the same size before
        // they grow; never more dead slots than occupied ones)
        c->wide_dead = std::min<uint64_t>(c->wide_dead + dropped, c->wused_base + c->known.wused);
        return FA_OK;
    }
    return fail(c, FA_ERR_ARG, "fa_drop_window: not a windowed row kind");
}

extern "C" int fa_close_window(fa_ctx* c, uint32_t timeslot, fa_row5m* out, size_t cap, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out || (!out && cap)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    int rc = rows_read(c, RK_5M, timeslot, 0, out, cap, n_out);
    if (rc) return rc;
    return drop_window(c, RK_5M, timeslot);
}

extern "C" int fa_drop_window(fa_ctx* c, int kind, uint32_t timeslot) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    int rc = settle(c);
    if (rc) return rc;
    return drop_window(c, kind, timeslot);
}

extern "C" int fa_drop_range(fa_ctx* c, int kind, uint32_t timeslot_lo, uint32_t timeslot_hi) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (timeslot_lo % c->gran || timeslot_hi % c->gran || timeslot_hi <= timeslot_lo) return fail(c, FA_ERR_ARG, "fa_drop_range: bounds must lie on the bucket grid, hi > lo");
    int rc = settle(c);
    if (rc) return rc;
    return drop_buckets(c, kind, timeslot_lo / c->gran, timeslot_hi / c->gran, true);
}

extern "C" int fa_rows_device(fa_ctx* c, int kind, uint32_t timeslot, size_t k, const void** d_rows, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !d_rows || !n_out) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    ReadClock clk(c);
    int rc = rows_local(c, clk, kind, timeslot, k, d_rows, n_out);
    if (rc) return rc;
    clk.done(row_kind_name(kind), clk.n_in, *n_out);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FA_OK;
}

// rows from elsewhere: are all n timeslots on this ctx's bucket grid?  (`who`: the entry point, for the message)
static int rows5m_on_grid(fa_ctx* c, const void* d_rows, size_t n, const char* who) {
    HIPCHK(c, zero_word(&c->d_ctr->rows_count, c->stream));
    hipLaunchKernelGGL(rows5m_check_kernel, grid_n(n), dim3(256), 0, c->stream, (const Row5m*)d_rows, (uint32_t)n, c->gran, &c->d_ctr->rows_count);
    unsigned int bad = 0;
    HIPCHK(c, read_word(&c->d_ctr->rows_count, bad, c->stream));
    if (!bad) return FA_OK;
    return fail(c, FA_ERR_ARG, (std::string(who) + ": timeslot not on this ctx's bucket grid").c_str());
}

// talker rows from elsewhere: all n are looked at before the first is merged
static int talker_rows_canonical(fa_ctx* c, const void* d_rows, size_t n) {
    if (!n) return FA_OK;
    HIPCHK(c, zero_word(&c->d_ctr->rows_count, c->stream));
    hipLaunchKernelGGL(talker_rows_check_kernel, grid_n(n), dim3(256), 0, c->stream, (const TalkRow*)d_rows, (uint64_t)n, &c->d_ctr->rows_count);
    unsigned int bad = 0;
    HIPCHK(c, read_word(&c->d_ctr->rows_count, bad, c->stream));
    return bad ? fail(c, FA_ERR_ARG, TALK_NOT_CANONICAL) : FA_OK;
}
// query rows from elsewhere, likewise
static int query_rows_producible(fa_ctx* c, const void* d_rows, size_t n) {
    if (!n) return FA_OK;
    HIPCHK(c, zero_word(&c->d_ctr->rows_count, c->stream));
    hipLaunchKernelGGL(query_rows_check_kernel, grid_n(n), dim3(256), 0, c->stream, (const TalkRow*)d_rows, (uint64_t)n, &c->d_ctr->rows_count);
    unsigned int bad = 0;
    HIPCHK(c, read_word(&c->d_ctr->rows_count, bad, c->stream));
    return bad ? fail(c, FA_ERR_ARG, QUERY_NOT_PRODUCIBLE) : FA_OK;
}

extern "C" int fa_rows_merge_device(fa_ctx* c, int kind, const void* d_rows, size_t n, size_t k, const void** d_out, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !d_out || !n_out || (!d_rows && n)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!row_bytes_of(kind)) return fail(c, FA_ERR_ARG, "unknown row kind");
    int rc = FA_OK;
    if (kind == RK_5M && n) {
        if (n >= (1ull << 31)) return fail(c, FA_ERR_ARG, "too many rows");
        rc = rows5m_on_grid(c, d_rows, n, "fa_rows_merge_device");
        if (rc) return rc;
    }
    if (is_talker_kind(kind)) {
        rc = kind_enabled(c, kind);
        if (rc) return rc;
        if (talk_rows_hold(c, d_rows)) return fail(c, FA_ERR_ARG, "rows to merge alias the ctx's result buffer (copy them first)");
        rc = talker_rows_canonical(c, d_rows, n);
        if (rc) return rc;
    }
    if (is_query_kind(kind)) {
        rc = query_rows_producible(c, d_rows, n);
        if (rc) return rc;
    }
    ReadClock clk(c, false);
    rc = rows_merge(c, c->stream, clk, kind, d_rows, n, 0xFFFFFFFFu, k, d_out, n_out);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FA_OK;
}

template <int KIND>
static int rows_partition_t(fa_ctx* c, const void* d_rows, uint32_t n, uint32_t world, size_t* counts) {
    typedef typename RowOps<KIND>::Row Row;
    unsigned int *cnt = c->part_cnt, *starts = c->part_cnt + RPART_MAX_WORLD, *cursor = c->part_cnt + 2 * RPART_MAX_WORLD;
    HIPCHK(c, hipMemsetAsync(c->part_cnt, 0, 3 * RPART_MAX_WORLD * sizeof(unsigned int), c->stream));
    const dim3 g((unsigned)std::min<size_t>(2048, ((size_t)n + RPART_BLOCK * RPART_U - 1) / (RPART_BLOCK * RPART_U))), b(RPART_BLOCK);
    hipLaunchKernelGGL((row_partition_kernel<KIND, false>), g, b, 0, c->stream, (const Row*)d_rows, n, world, cnt, (const unsigned int*)starts, cursor, (Row*)nullptr);
    std::vector<unsigned int> h(world), hs(world);
    HIPCHK(c, hipMemcpyAsync(h.data(), cnt, world * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned int run = 0;
    for (uint32_t d = 0; d < world; d++) {
        hs[d] = run;
        run += h[d];
        counts[d] = h[d];
    }
    if (run != n) return fail(c, FA_ERR_HIP, "internal: partition counts do not add up");
    HIPCHK(c, hipMemcpyAsync(starts, hs.data(), world * sizeof(unsigned int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL((row_partition_kernel<KIND, true>), g, b, 0, c->stream, (const Row*)d_rows, n, world, cnt, (const unsigned int*)starts, cursor, (Row*)c->part_buf);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (hs is read by the copy above until here)
    return FA_OK;
}

extern "C" int fa_rows_partition_device(fa_ctx* c, int kind, const void* d_rows, size_t n, uint32_t world, const void** d_out, size_t* counts) {
    FA_ON_DEVICE(c);
    if (!c || !d_out || !counts || (!d_rows && n) || world == 0 || world > RPART_MAX_WORLD) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    const size_t rb = row_bytes_of(kind);
    if (!rb) return fail(c, FA_ERR_ARG, "unknown row kind");
    if (is_talker_kind(kind) && !c->talk) return kind_enabled(c, kind);
    if (n >= (1ull << 31) - 1024) return fail(c, FA_ERR_ARG, "too many rows for one partition (2^31)");
    *d_out = nullptr;
    for (uint32_t d = 0; d < world; d++) counts[d] = 0;
    if (!n) return FA_OK;
    int rc = ensure_dev(c, c->part_buf, n * rb, "partitioned rows");
    if (rc) return rc;
    if (!c->part_cnt.grow(3 * RPART_MAX_WORLD * sizeof(unsigned int))) return fail(c, FA_ERR_NOMEM, "hipMalloc(partition counters) failed");
    if (inside(c->part_buf, d_rows)) return fail(c, FA_ERR_ARG, "rows to partition alias the ctx's partition buffer");
    (void)with_row_kind(kind, [&](auto rk) { rc = rows_partition_t<decltype(rk)::value>(c, d_rows, (uint32_t)n, world, counts); });  // (a known kind: it has a row size)
    if (rc) return rc;
    *d_out = c->part_buf;
    return FA_OK;
}

extern "C" int fa_rows_fetch(fa_ctx* c, int kind, const void* d_rows, size_t n, void* out, size_t cap) {
    FA_ON_DEVICE(c);
    if (!c || (!d_rows && n) || (!out && n)) return FA_ERR_ARG;
    const size_t rb = row_bytes_of(kind);
    if (!rb) return fail(c, FA_ERR_ARG, "unknown row kind");
    if (is_talker_kind(kind) && !c->talk) return kind_enabled(c, kind);
    if (n > cap) return fail(c, FA_ERR_CAPACITY, "output buffer too small");
    ReadClock clk(c);
    struct Done {
        ReadClock& k;
        int kind;
        size_t n;
        ~Done() {
            k.mark("copy out");
            k.done(row_kind_name(kind), n, n);
        }
    } done{clk, kind, n};
    if (n) {
        if (inside(c->h_rows, d_rows)) {
            copy_threads(c, out, d_rows, n * rb);  // (host memory: a result the last kernel wrote into the pinned buffer)
            return FA_OK;
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        int rc = ensure_pinned(c, n * rb);
        if (rc) return rc;
        return copy_out_pipelined(c, out, d_rows, n * rb);
    }
    return FA_OK;
}

// (kept from ABI 4: the window's flows_5m rows, sorted, in HBM - not folded; fa_rows_device folds sliding windows)
extern "C" int fa_window_rows_device(fa_ctx* c, uint32_t timeslot, const void** d_rows, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !d_rows || !n_out) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    *d_rows = nullptr;
    *n_out = 0;
    uint32_t lo, hi;
    if (!bucket_range(c, timeslot, lo, hi)) return FA_OK;
    ReadClock clk(c, false);  // (not a read with phases to report)
    const void* in = nullptr;
    size_t n = 0;
    int rc = collect_5m(c, clk, lo, hi, in, n);
    if (rc) return rc;
    rc = rows_merge(c, c->stream, clk, RK_5M, in, n, 0xFFFFFFFFu, 0, d_rows, n_out);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FA_OK;
}

extern "C" int fa_merge_rows_device(fa_ctx* c, const void* d_rows, size_t n) {
    FA_ON_DEVICE(c);
    if (!c || (!d_rows && n)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!n) return FA_OK;
    if (n >= (1ull << 31)) return fail(c, FA_ERR_ARG, "fa_merge_rows_device: too many rows");
    int rc = rows5m_on_grid(c, d_rows, n, "fa_merge_rows_device");
    if (rc) return rc;
    KArgs a = make_args(c);
    hipLaunchKernelGGL(merge_rows_kernel, dim3(1024), dim3(256), 0, c->stream, (const Row5m*)d_rows, (uint32_t)n, a);
    HIPCHK(c, hipGetLastError());
    return settle(c);
}

extern "C" int fa_open_timeslots(fa_ctx* c, uint32_t* out, size_t cap, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    {   // the buckets the table holds, found on the device: min / max, then one bit per bucket of that range (a consumer asks
        // before every flush - inserter_gpu: markEmitted -; round 3 copied every row to the host and sorted the timeslots)
        int rc0 = settle(c);
        if (rc0) return rc0;
        constexpr uint32_t MAXBITS = 1u << 16;
        rc0 = ensure_dev(c, c->rw_buf, MAXBITS / 8 + 64, "timeslot bits");
        if (rc0) return rc0;
        unsigned int* range = (unsigned int*)c->rw_buf;
        unsigned int* bits = range + 16;
        HIPCHK(c, hipMemsetAsync(range, 0xff, sizeof(unsigned int), c->stream));
        HIPCHK(c, hipMemsetAsync(range + 1, 0, sizeof(unsigned int), c->stream));
        hipLaunchKernelGGL(timeslots_kernel, dim3(1024), dim3(256), 0, c->stream, (const Slot*)c->tab, 1u << c->cap_log2, 0u, 0u, (unsigned int*)nullptr, range);
        unsigned int r[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(r, range, sizeof r, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (r[0] == 0xffffffffu) {  // no live group
            *n_out = 0;
            return FA_OK;
        }
        if (r[1] - r[0] < MAXBITS) {
            const uint32_t nbits = r[1] - r[0] + 1u, nwords = (nbits + 31u) / 32u;
            HIPCHK(c, hipMemsetAsync(bits, 0, nwords * sizeof(unsigned int), c->stream));
            hipLaunchKernelGGL(timeslots_kernel, dim3(1024), dim3(256), 0, c->stream, (const Slot*)c->tab, 1u << c->cap_log2, r[0], nbits, bits, range);
            std::vector<unsigned int> h(nwords);
            HIPCHK(c, hipMemcpyAsync(h.data(), bits, nwords * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::vector<uint32_t> ts;
            for (uint32_t i = 0; i < nbits; i++)
                if (h[i >> 5] >> (i & 31u) & 1u) ts.push_back((r[0] + i) * c->gran);
            *n_out = ts.size();
            if (ts.size() > cap) return fail(c, FA_ERR_CAPACITY, "output buffer too small");
            if (!ts.empty()) memcpy(out, ts.data(), ts.size() * 4);
            return FA_OK;
        }
        // (buckets spread over more than 65 536 granules: the rows' own timeslots, below)
    }
    ReadClock clk(c, false);
    const void* in = nullptr;
    size_t nr = 0;
    int rc = collect_5m(c, clk, 0, 0xFFFFFFFFu, in, nr);
    if (rc) return rc;
    std::vector<fa_row5m> rows(nr);
    if (nr) HIPCHK(c, hipMemcpy(rows.data(), in, nr * sizeof(Row5m), hipMemcpyDeviceToHost));
    std::vector<uint32_t> ts;
    ts.reserve(rows.size());
    for (auto& r : rows) ts.push_back(r.timeslot);
    std::sort(ts.begin(), ts.end());
    ts.erase(std::unique(ts.begin(), ts.end()), ts.end());
    *n_out = ts.size();
    if (ts.size() > cap) return fail(c, FA_ERR_CAPACITY, "output buffer too small");
    if (!ts.empty()) memcpy(out, ts.data(), ts.size() * 4);
    return FA_OK;
}

extern "C" int fa_merge_rows(fa_ctx* c, const fa_row5m* rows, size_t n) {
    FA_ON_DEVICE(c);
    if (!c || (!rows && n)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!n) return FA_OK;
    for (size_t i = 0; i < n; i++)
        if (rows[i].timeslot % c->gran) return fail(c, FA_ERR_ARG, "fa_merge_rows: timeslot not on this ctx's bucket grid");
    DevBuf<Row5m> d;
    if (!d.grow(n * sizeof(Row5m))) return fail(c, FA_ERR_NOMEM, "hipMalloc failed");
    auto hip_failed = [&](hipError_t e) {
        c->err = std::string("fa_merge_rows: ") + hipGetErrorString(e);
        return FA_ERR_HIP;
    };
    hipError_t e = hipMemcpyAsync(d, rows, n * sizeof(Row5m), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_failed(e);
    KArgs a = make_args(c);
    hipLaunchKernelGGL(merge_rows_kernel, dim3(256), dim3(256), 0, c->stream, d.get(), (uint32_t)n, a);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_failed(e);
    return settle(c);
}

// ---- C-ABI: the wide key sets and the dashboard reads --------------------------------------------------------------
extern "C" int fa_read_window_app(fa_ctx* c, uint32_t timeslot, fa_row_app* out, size_t cap, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out || (!out && cap)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    static_assert(sizeof(RowApp) == sizeof(fa_row_app), "row layout");
    return rows_read(c, RK_APP, timeslot, 0, out, cap, n_out);
}

extern "C" int fa_close_window_app(fa_ctx* c, uint32_t timeslot, fa_row_app* out, size_t cap, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out || (!out && cap)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    int rc = rows_read(c, RK_APP, timeslot, 0, out, cap, n_out);
    if (rc) return rc;
    return drop_window(c, RK_APP, timeslot);
}

extern "C" int fa_read_window_app48(fa_ctx* c, uint32_t timeslot, fa_row_app48* out, size_t cap, size_t* n_out, uint32_t* date_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out || (!out && cap)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    static_assert(sizeof(RowApp48) == sizeof(fa_row_app48), "row layout");
    return rows_read_app48(c, timeslot, out, cap, n_out, date_out);
}

extern "C" int fa_close_window_app48(fa_ctx* c, uint32_t timeslot, fa_row_app48* out, size_t cap, size_t* n_out, uint32_t* date_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out || (!out && cap)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    int rc = rows_read_app48(c, timeslot, out, cap, n_out, date_out);
    if (rc) return rc;
    return drop_window(c, RK_APP, timeslot);
}

extern "C" int fa_top_ports(fa_ctx* c, int dst, size_t k, fa_port_row* out, size_t cap, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out || (!out && cap) || (dst != 0 && dst != 1)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    static_assert(sizeof(RowW) == sizeof(fa_port_row) && sizeof(RowW) == sizeof(fa_minute_row), "row layout");
    if (k == 0) {
        *n_out = 0;
        return FA_OK;
    }
    return rows_read(c, dst ? RK_PORT_DST : RK_PORT_SRC, 0, k, out, cap, n_out);
}

extern "C" int fa_minute_series(fa_ctx* c, fa_minute_row* out, size_t cap, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out || (!out && cap)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    return rows_read(c, RK_MINUTE, 0, 0, out, cap, n_out);
}

extern "C" int fa_topk(fa_ctx* c, uint32_t key_set, size_t k, fa_topk_row* out, size_t cap, size_t* n_out) {
    FA_ON_DEVICE(c);
    if (!c || !n_out || (!out && cap)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (key_set != FA_KEYS_SRCADDR_CMS && key_set != FA_KEYS_DSTADDR_CMS) return fail(c, FA_ERR_ARG, "fa_topk: key set not enabled");
    static_assert(sizeof(TopkRow) == sizeof(fa_topk_row), "row layout");
    if (k == 0) {
        *n_out = 0;
        return FA_OK;
    }
    return rows_read(c, key_set == FA_KEYS_SRCADDR_CMS ? RK_TOPK_SRC : RK_TOPK_DST, 0, k, out, cap, n_out);
}
