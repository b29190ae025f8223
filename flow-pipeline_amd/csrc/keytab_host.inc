// keytab_host.inc - host side of the keyed tables (included by flowagg.hip before talkers_host.inc and ports_host.inc: one
// translation unit; device side: keytab.cuh).  TabPair<T> is what the talker and the port state share; everything that keeps the
// capacity rule (table_room.h) is here and nowhere else: settle, reserve, rebuild and the chunk loop.
// The traits T (talkers.cuh TalkTab, ports.cuh PortTab) also supply NOUN ("talker"), FN ("fa_talkers"), WG_PER_CU and WGPC_ENV.

static int fail(fa_ctx* c, int code, const std::string& msg) { return fail(c, code, msg.c_str()); }

template <class T>
struct TabPair {
    DevBuf<typename T::Slot> tab[2];
    uint32_t log2[2] = {16, 16};
    uint32_t bucket_secs = 0;  // the key carries t32 / bucket_secs; 0 = plain tables (no time axis)
    uint64_t used_ub[2] = {0, 0};
    DevBuf<typename T::Counters> d_ctr;
    size_t chunk = (size_t)1 << 20;  // env FA_TALK_CHUNK (the one knob of the second pass)
    uint32_t wgpc = T::WG_PER_CU;    // env T::WGPC_ENV (A/B: workgroups per CU of the fold kernel)
    uint64_t grows = 0, fold_launches = 0, fold_ns_total = 0;
    Events ev;  // one pair per fold launch that has not been read yet

    uint64_t slots(int d) const { return 1ull << log2[d]; }
    uint32_t mask(int d) const { return (uint32_t)(slots(d) - 1); }
    dim3 scan_grid(const fa_ctx* c, int d) const { return dim3((unsigned)std::min<uint64_t>((slots(d) + 255) / 256, (uint64_t)c->num_cus * 8)); }
};
static constexpr size_t TAB_EV_MAX = 2 * 1024;  // fold launches whose times are pending before the tables are settled

#define TAB_ENTER(c, state, off)                                                                       \
    FA_ON_DEVICE(c);                                                                                   \
    if (!(c)) return FA_ERR_ARG;                                                                       \
    if ((c)->sticky) return (c)->sticky;                                                               \
    if (!(c)->state) return fail((c), FA_ERR_UNSUPPORTED, off)

// A state S (a TabPair plus S::alloc_own() for what else it owns) behind `slot`, both tables empty at 2^capacity_log2 slots.
template <class T, class S>
static int tab_enable(fa_ctx* c, S*& slot, const char* fn, uint32_t capacity_log2, uint32_t bucket_secs) {
    if (capacity_log2 == 0) capacity_log2 = 16;
    if (capacity_log2 < 8 || capacity_log2 > 30) return fail(c, FA_ERR_ARG, std::string(fn) + ": capacity_log2 is 0 or 8..30");
    S* t = new S();
    t->bucket_secs = bucket_secs;
    if (const char* d = getenv("FA_TALK_CHUNK")) t->chunk = (size_t)std::min<long long>(1ll << 28, std::max<long long>(1, atoll(d)));
    if (const char* d = getenv(T::WGPC_ENV)) t->wgpc = (uint32_t)std::min(8, std::max(1, atoi(d)));
    slot = t;
    bool ok = t->d_ctr.grow(sizeof(typename T::Counters)) && hipMemsetAsync(t->d_ctr, 0, sizeof(typename T::Counters), c->stream) == hipSuccess;
    ok = ok && t->alloc_own();
    for (int d = 0; d < 2 && ok; d++) {
        t->log2[d] = capacity_log2;
        ok = t->tab[d].grow(sizeof(typename T::Slot) << capacity_log2) && hipMemsetAsync(t->tab[d], 0, sizeof(typename T::Slot) << capacity_log2, c->stream) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        state_destroy(slot);
        return fail(c, FA_ERR_NOMEM, std::string(fn) + ": allocating the tables failed");
    }
    return FA_OK;
}

// Waits for the stream; the device counters and the fold launches' times.  The exact counts replace the host's bounds.
template <class T>
static int tab_settle(fa_ctx* c, TabPair<T>& t, typename T::Counters& h) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&h, t.d_ctr, sizeof h, hipMemcpyDeviceToHost));
    for (size_t i = 0; i + 1 < t.ev.used(); i += 2) Events::elapsed_ns(t.ev[i], t.ev[i + 1], &t.fold_ns_total);
    t.ev.rewind();
    if (h.lost) {
        c->sticky = FA_ERR_TABLE_FULL;
        return fail(c, FA_ERR_TABLE_FULL, std::string("internal: a ") + T::NOUN + " table was full during a launch; updates were lost");
    }
    t.used_ub[0] = h.used[0];
    t.used_ub[1] = h.used[1];
    return FA_OK;
}

// Table d rebuilt into a fresh one of 2^nl slots: growth (nl above log2, everything kept) and drop_before (the same size, the
// slots of a bucket index below floor_index left behind).  The device's counters of direction d are counted again.
// fresh: a table of 2^nl slots the caller allocated beforehand (tab_drop_before allocates both before it rebuilds either).
template <class T>
static int tab_rebuild(fa_ctx* c, TabPair<T>& t, int d, uint32_t nl, uint32_t floor_index, DevBuf<typename T::Slot>* fresh = nullptr) {
    using Slot = typename T::Slot;
    DevBuf<Slot> nt;
    if (fresh) nt = std::move(*fresh);
    else if (!nt.grow(sizeof(Slot) << nl)) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, std::string("hipMalloc(") + T::NOUN + " table) failed");
    }
    hipError_t e = hipMemsetAsync(nt, 0, sizeof(Slot) << nl, c->stream);
    for (int w = 0; w < T::NT && e == hipSuccess; w++)  // (the rehash counts every key again)
        e = hipMemsetAsync(&t.d_ctr->used[0] + 2 * w + d, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tab_rehash_kernel<T>, t.scan_grid(c, d), dim3(256), 0, c->stream, (const Slot*)t.tab[d], t.slots(d), nt.get(), (uint32_t)((1ull << nl) - 1), t.d_ctr.get(), d,
                           floor_index);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->sticky = FA_ERR_HIP;  // (the occupied-slot counters were reset: the state is no longer trustworthy)
        c->err = std::string(T::NOUN) + " table rebuild: " + hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    t.tab[d] = std::move(nt);  // (frees the old table: the rehash has been synchronised)
    t.log2[d] = nl;
    return FA_OK;
}

// Room for m more keys in table d at a load of at most 1/2: growth is decided on the exact counts, right after a settle.
template <class T>
static int tab_reserve(fa_ctx* c, TabPair<T>& t, int d, uint64_t m) {
    if (table_room_fits(t.used_ub[d], m, t.log2[d])) return FA_OK;
    typename T::Counters h;
    int rc = tab_settle(c, t, h);
    if (rc) return rc;
    const uint32_t nl = table_room_grow_to(t.used_ub[d], m, t.log2[d]);
    if (nl == TABLE_ROOM_FULL) return fail(c, FA_ERR_TABLE_FULL, std::string("a ") + T::NOUN + " table cannot grow further (2^30 slots)");
    if (nl == t.log2[d]) return FA_OK;
    const uint32_t doublings = nl - t.log2[d];
    rc = tab_rebuild(c, t, d, nl, 0);
    if (!rc) t.grows += doublings;
    return rc;
}

template <class T>
static size_t tab_chunk_cap(const TabPair<T>& t) {
    return table_room_chunk_cap(t.chunk, t.log2[0], t.log2[1]);
}

// n records (or rows) in chunks: room reserved in the tables of `dirs` (bit d = table d), launch(i, m) for the chunk
// [i, i + m), the bounds raised by what it may have added.
template <class T, class Launch>
static int tab_chunks(fa_ctx* c, TabPair<T>& t, int dirs, size_t n, Launch&& launch) {
    for (size_t i = 0; i < n;) {
        const size_t m = std::min(n - i, tab_chunk_cap(t));
        for (int d = 0; d < 2; d++)
            if (dirs >> d & 1) {
                int rc = tab_reserve(c, t, d, m);
                if (rc) return rc;
            }
        int rc = launch(i, m);
        if (rc) return rc;
        for (int d = 0; d < 2; d++)
            if (dirs >> d & 1) t.used_ub[d] += m;
        i += m;
    }
    return FA_OK;
}

// One fold launch over m records, timed: kernel(grid) launches it on the ctx stream.  The pool of event pairs is bounded: a
// full one is read first (the exact counts replace the bounds - no larger, so room reserved before still holds).
// persistent grid: the workgroups that are co-resident, records grid-strided
template <class T, class Kernel>
static int tab_fold_launch(fa_ctx* c, TabPair<T>& t, size_t m, Kernel&& kernel) {
    if (t.ev.used() + 2 > TAB_EV_MAX) {
        typename T::Counters h;
        int rc = tab_settle(c, t, h);
        if (rc) return rc;
    }
    const hipEvent_t* ev = t.ev.take(2);
    if (!ev) return events_failed(c);
    const uint32_t grid = (uint32_t)std::max<size_t>(1, std::min<size_t>((m + T::BLOCK - 1) / T::BLOCK, (size_t)c->num_cus * t.wgpc));
    (void)hipEventRecord(ev[0], c->stream);
    kernel(dim3(grid));
    (void)hipEventRecord(ev[1], c->stream);
    HIPCHK(c, hipGetLastError());
    t.fold_launches++;
    return FA_OK;
}

// Empties both tables (they keep their size); the other counters of the statistics go on counting.
template <class T>
static int tab_reset(fa_ctx* c, TabPair<T>& t) {
    typename T::Counters h;
    int rc = tab_settle(c, t, h);
    if (rc) return rc;
    for (int d = 0; d < 2; d++) HIPCHK(c, hipMemsetAsync(t.tab[d], 0, sizeof(typename T::Slot) << t.log2[d], c->stream));
    HIPCHK(c, hipMemsetAsync(&t.d_ctr->used[0], 0, 2 * T::NT * sizeof(unsigned long long), c->stream));  // (the tally words)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t.used_ub[0] = t.used_ub[1] = 0;
    return FA_OK;
}

template <class T, class Stats>
static int tab_stats(fa_ctx* c, TabPair<T>& t, Stats* out) {
    if (!out) return fail(c, FA_ERR_ARG, std::string(T::FN) + "_stats: null argument");
    typename T::Counters h;
    int rc = tab_settle(c, t, h);
    if (rc) return rc;
    for (int d = 0; d < 2; d++) {
        out->used[d] = h.used[d];
        out->capacity[d] = t.slots(d);
    }
    out->records_folded = h.folded;
    out->records_absorbed = h.absorbed;
    out->grows = t.grows;
    out->fold_launches = t.fold_launches;
    out->fold_ns_total = t.fold_ns_total;
    return FA_OK;
}

// Removes every bucket that starts below t_floor.  The slots are write-once, so nothing is deleted in place: each table is
// rebuilt into a fresh one of the same size without those slots (tab_rebuild), the counters and the host's bounds counted again.
// No floor is kept: a record that arrives later with a time below t_floor opens its bucket again (what a late INSERT does to
// flows_5m).
template <class T>
static int tab_drop_before(fa_ctx* c, TabPair<T>& t, uint32_t t_floor) {
    using Slot = typename T::Slot;
    if (t_floor % t.bucket_secs) return fail(c, FA_ERR_ARG, std::string(T::FN) + "_drop_before: t lies on the bucket grid");
    typename T::Counters h;
    int rc = tab_settle(c, t, h);
    if (rc) return rc;
    if (t_floor == 0) return FA_OK;
    DevBuf<Slot> fresh[2];  // both before either table is touched: without memory nothing is dropped, in neither table
    for (int d = 0; d < 2; d++)
        if (!fresh[d].grow(sizeof(Slot) << t.log2[d])) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, std::string(T::FN) + "_drop_before: hipMalloc(" + T::NOUN + " table) failed; nothing was dropped");
        }
    for (int d = 0; d < 2; d++) {
        rc = tab_rebuild(c, t, d, t.log2[d], t_floor / t.bucket_secs, &fresh[d]);
        if (rc) return rc;  // (a failing launch or synchronisation: sticky)
    }
    return tab_settle(c, t, h);
}

// ---- ranged reads ---------------------------------------------------------------------------------------------------------
// [t_lo, t_hi) on the grid of bucket_secs as bucket indices (bucket_range.h states the rule).
static int tab_range_of(fa_ctx* c, uint32_t bucket_secs, uint32_t t_lo, uint32_t t_hi, BucketRange& r) {
    switch (bucket_range_of(bucket_secs, t_lo, t_hi, r)) {
    case BUCKET_RANGE_OFF_GRID: return fail(c, FA_ERR_ARG, "range: t_lo and t_hi lie on the bucket grid (t_hi = 0xFFFFFFFF: no upper bound)");
    case BUCKET_RANGE_REVERSED: return fail(c, FA_ERR_ARG, "range: t_lo > t_hi");
    default: return FA_OK;
    }
}
// The two doors of a ranged read are the un-ranged read of row kind `kind` with the tables' ranged collector (rows_local): the
// merge behind it sums the rows of equal key and leaves the un-ranged read's order, cut at k.  fn: the door's name.
static int tab_range_read(fa_ctx* c, const char* fn, uint32_t bucket_secs, int kind, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, void* out, size_t cap, size_t* n_out) {
    if ((dst != 0 && dst != 1) || !n_out || (!out && cap)) return fail(c, FA_ERR_ARG, std::string(fn) + ": bad argument");
    BucketRange r;
    int rc = tab_range_of(c, bucket_secs, t_lo, t_hi, r);
    if (rc) return rc;
    return rows_read(c, kind, 0, k, out, cap, n_out, &r);
}
static int tab_range_rows_device(fa_ctx* c, const char* fn, uint32_t bucket_secs, int kind, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, const void** d_rows, size_t* n_out) {
    if ((dst != 0 && dst != 1) || !n_out || !d_rows) return fail(c, FA_ERR_ARG, std::string(fn) + ": bad argument");
    BucketRange r;
    int rc = tab_range_of(c, bucket_secs, t_lo, t_hi, r);
    if (rc) return rc;
    ReadClock clk(c);
    rc = rows_local(c, clk, kind, 0, k, d_rows, n_out, false, nullptr, &r);
    if (rc) return rc;
    clk.done(row_kind_name(kind), clk.n_in, *n_out);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FA_OK;
}

// The bucket starts held in a pair of bucketed tables, ascending (fa_open_timeslots' contract).  Min and max index first; a span
// of up to 2^16 indices is answered from one bit per index, a wider one (bucket_secs = 1 over days, stray times) from the slots'
// own indices.
//   held: the occupied slots of both tables; scratch: a buffer of the state, dead otherwise;
//   scan(lo, nbits, bits, range): launches tab_buckets_kernel over both tables (bits == nullptr: min / max into range);
//   list(out, cap, cursor): launches tab_bucket_list_kernel over both.
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
template <class T>
static int tab_buckets(fa_ctx* c, TabPair<T>& t, DevBuf<>& scratch, uint32_t* out, size_t cap, size_t* n_out) {
    using Slot = typename T::Slot;
    if (!n_out || (!out && cap)) return fail(c, FA_ERR_ARG, std::string(T::FN) + "_buckets: bad argument");
    typename T::Counters h;
    int rc = tab_settle(c, t, h);
    if (rc) return rc;
    return bucket_starts(
        c, t.bucket_secs, (size_t)(h.used[0] + h.used[1]), scratch,
        [&](uint32_t lo, uint32_t nbits, unsigned int* bits, unsigned int* range) {
            for (int d = 0; d < 2; d++) hipLaunchKernelGGL(tab_buckets_kernel<T>, t.scan_grid(c, d), dim3(256), 0, c->stream, (const Slot*)t.tab[d], t.slots(d), lo, nbits, bits, range);
        },
        [&](uint32_t* list, uint32_t list_cap, unsigned int* cursor) {
            for (int d = 0; d < 2; d++) hipLaunchKernelGGL(tab_bucket_list_kernel<T>, t.scan_grid(c, d), dim3(256), 0, c->stream, (const Slot*)t.tab[d], t.slots(d), list, list_cap, cursor);
        },
        out, cap, n_out);
}
