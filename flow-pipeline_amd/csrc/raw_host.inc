// raw_host.inc - host side of the flows_raw parts (included by flowagg.hip: one translation unit; device side and the part format:
// raw.cuh).  A ctx with fa_raw_enable hands every decoded chunk of the second pass (second_pass.inc) to raw_build_cols, which
// appends the chunk's parts - one Native block per Date, rows in stable t32 order - to ONE device image; fa_raw_take delivers
// the image with one copy.
//
// Memory: the image holds header + 110 bytes per row that was built and not yet taken, and grows by doubling (at least to
// what is needed; the old image is copied inside HBM).  Scratch: 24 bytes per record of the largest chunk plus hipcub's
// temporary storage.  Both are kept until fa_raw_reset / fa_destroy.
// One host synchronisation per chunk: the part list (a few entries) is read before the gather is launched, because the
// image's layout depends on the rows per Date.

struct RawState {
    size_t chunk = (size_t)1 << 20;
    DevBuf<uint8_t> img;   // the pending parts, back to back
    size_t used = 0;       // bytes of img that hold pending parts
    std::vector<fa_raw_part> pending;
    DevBuf<> scratch;      // flags, positions, 2 x keys, 2 x indices, the part list, hipcub storage
    PinnedBuf<uint8_t> h_list;  // the part list's first RAW_LIST_FIRST bytes on their way to the host
    Events ev;             // 4: build start, order done, first gather launch, gather done
    bool ev_pending = false;
    uint64_t records_in = 0, records_bad = 0, rows_out = 0, parts_out = 0, bytes_out = 0, chunks = 0;
    uint64_t order_ns = 0, gather_ns = 0, launches = 0;
    uint64_t takes = 0;    // times the pending parts were cleared (a take, a reset) or replaced (a merge): frames made of them before are stale (lz4_host.inc)
};
static constexpr size_t RAW_LIST_FIRST = 4096;  // header + 255 entries: what one small copy brings

static void raw_destroy(fa_ctx* c) {
    RawState* t = c->raw;
    if (!t) return;
    if (getenv("FA_VERBOSE"))
        fprintf(stderr, "[flowagg] raw parts: %llu records in %llu chunks, order %llu ns, gather %llu ns\n", (unsigned long long)t->records_in, (unsigned long long)t->chunks,
                (unsigned long long)t->order_ns, (unsigned long long)t->gather_ns);
    state_destroy(c->raw);
}

#define RAW_ENTER(c, fn)                                                                                   \
    FA_ON_DEVICE(c);                                                                                       \
    if (!(c)) return FA_ERR_ARG;                                                                           \
    if ((c)->sticky) return (c)->sticky;                                                                   \
    if (!(c)->raw) return fail((c), FA_ERR_ARG, fn ": fa_raw_enable was not called on this ctx")

// ---- host only: the part's size and the encoder the CPU tests and a consumer without a GPU sink use ---------------------------
extern "C" size_t fa_raw_part_bytes(uint64_t rows) { return (size_t)raw_col_offset(RAW_COLS_H, rows, RAW_NCOLS); }

extern "C" int fa_flow_rows_to_native(const fa_flow_row* rows, size_t n, uint8_t* out, size_t cap, size_t* bytes_out) {
    if ((!rows && n) || !bytes_out) return FA_ERR_ARG;
    for (size_t i = 0; i < n; i++) {  // one Date, status 0, ascending t32
        const uint32_t t = (uint32_t)rows[i].time_received;
        if (rows[i].status != 0) return FA_ERR_ARG;
        if (i && (t < (uint32_t)rows[i - 1].time_received || t / 86400u != (uint32_t)rows[0].time_received / 86400u)) return FA_ERR_ARG;
    }
    const size_t need = fa_raw_part_bytes(n);
    *bytes_out = need;
    if (need > cap || !out) return FA_ERR_CAPACITY;
    uint8_t* p = out;
    auto put = [&](uint64_t v, int bytes) {
        for (int i = 0; i < bytes; i++) *p++ = (uint8_t)(v >> (8 * i));
    };
    p += raw_put_varuint(p, RAW_NCOLS);
    p += raw_put_varuint(p, n);
    for (uint32_t c = 0; c < RAW_NCOLS; c++) {
        const RawColDef& d = RAW_COLS_H[c];
        for (uint32_t i = 0; i < raw_col_header_len(d); i++) *p++ = raw_col_header_byte(d, i);
        for (size_t i = 0; i < n; i++) {
            const fa_flow_row& r = rows[i];
            switch (c) {
            case 0: put((uint32_t)r.time_received / 86400u, 2); break;
            case 1: put((uint32_t)r.time_received, 4); break;
            case 2: put((uint32_t)r.time_flow_start, 4); break;
            case 3: put(r.sequence_num, 4); break;
            case 4: put(r.sampling_rate, 8); break;
            case 5: memcpy(p, r.sampler_address, 16), p += 16; break;
            case 6: memcpy(p, r.src_addr, 16), p += 16; break;
            case 7: memcpy(p, r.dst_addr, 16), p += 16; break;
            case 8: put(r.src_as, 4); break;
            case 9: put(r.dst_as, 4); break;
            case 10: put(r.etype, 4); break;
            case 11: put(r.proto, 4); break;
            case 12: put(r.src_port, 4); break;
            case 13: put(r.dst_port, 4); break;
            case 14: put(r.bytes, 8); break;
            default: put(r.packets, 8);
            }
        }
    }
    return FA_OK;
}

// ---- enable -------------------------------------------------------------------------------------------------------------------
extern "C" int fa_raw_enable(fa_ctx* c, uint32_t chunk_records) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (c->raw) return fail(c, FA_ERR_ARG, "fa_raw_enable: already enabled");
    if (chunk_records > (1u << 24)) return fail(c, FA_ERR_ARG, "fa_raw_enable: chunk_records is 0 (default 2^20) or 1..2^24");
    RawState* t = new RawState();
    if (chunk_records) t->chunk = chunk_records;
    c->raw = t;
    if (!t->h_list.grow(RAW_LIST_FIRST) || !t->ev.ensure(4)) {
        (void)hipGetLastError();
        raw_destroy(c);
        return fail(c, FA_ERR_NOMEM, "fa_raw_enable: allocating the part list's staging failed");
    }
    return FA_OK;
}

static size_t raw_chunk_cap(const fa_ctx* c) { return c->raw->chunk; }

// the gather of the last build has finished (the caller synchronised, or does so here): its time is added
static void raw_read_events(RawState* t) {
    if (!t->ev_pending) return;
    if (hipEventSynchronize(t->ev[3]) == hipSuccess) Events::elapsed_ns(t->ev[2], t->ev[3], &t->gather_ns);
    t->ev_pending = false;
}

// Room for `more` bytes behind the pending parts.  A larger image is allocated first and the pending bytes are copied inside
// HBM: when the allocation fails nothing has changed.
static int raw_reserve_image(fa_ctx* c, size_t more) {
    RawState* t = c->raw;
    const size_t need = t->used + more;
    if (t->img.bytes() >= need) return FA_OK;
    DevBuf<uint8_t> bigger;
    if (!bigger.grow(std::max<size_t>(need, std::max<size_t>(2 * t->img.bytes(), (size_t)1 << 20)))) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "hipMalloc(raw part image) failed; the chunk's parts were not built");
    }
    if (t->used) HIPCHK(c, hipMemcpyAsync(bigger, t->img, t->used, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t->img = std::move(bigger);
    return FA_OK;
}

// ---- order and layout, shared by the build of a chunk and the merge (raw_merge_host.inc) ------------------------------------------
// The scratch of one order step over n keys, behind whatever the caller keeps in front of it: keys and indices in and out
// (n + 1 words each), the part list, hipcub's storage (tmp_min: what the caller's own hipcub calls need of it).
struct RawOrder {
    uint32_t n = 0;
    size_t words = 0, list_bytes = 0, tmp_bytes = 0;
    uint32_t *key_in = nullptr, *key = nullptr, *idx_in = nullptr, *idx = nullptr;
    RawPartsHeader* hdr = nullptr;
    RawPartEntry* list = nullptr;
    void* tmp = nullptr;
    RawOrder(fa_ctx* c, uint32_t n_, size_t tmp_min = 0) : n(n_) {
        size_t tmp_sort = 0;
        (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 32, c->stream);
        words = align256(((size_t)n + 1) * 4), tmp_bytes = align256(std::max(tmp_min, tmp_sort));
        list_bytes = align256(sizeof(RawPartsHeader) + (size_t)RAW_MAX_DATES * sizeof(RawPartEntry));
    }
    size_t bytes() const { return 4 * words + list_bytes + tmp_bytes; }
    void carve(uint8_t* sb) {
        key_in = (uint32_t*)sb, key = (uint32_t*)(sb + words), idx_in = (uint32_t*)(sb + 2 * words), idx = (uint32_t*)(sb + 3 * words);
        hdr = (RawPartsHeader*)(sb + 4 * words), list = (RawPartEntry*)(hdr + 1);
        tmp = sb + 4 * words + list_bytes;
    }
};

// key_in / idx_in -> key / idx in stable key order, the positions where the Date changes (pos[n]: the count of good rows in
// front), `done` recorded behind the last kernel and *launches += launched, then ONE small copy and one synchronisation: the
// list's header and its entries in ascending `start`.  A header whose nparts exceeds the list comes back without entries: the
// caller's consistency check fails.
static int raw_order_and_list(fa_ctx* c, const RawOrder& o, const uint32_t* pos, hipEvent_t done, uint64_t* launches, uint64_t launched, RawPartsHeader* h,
                              std::vector<RawPartEntry>* ent) {
    RawState* t = c->raw;
    HIPCHK(c, hipMemsetAsync(o.hdr, 0, sizeof(RawPartsHeader), c->stream));
    size_t tb = o.tmp_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(o.tmp, tb, (const uint32_t*)o.key_in, o.key, (const uint32_t*)o.idx_in, o.idx, (int)o.n, 0, 32, c->stream) != hipSuccess)
        return fail(c, FA_ERR_HIP, "sort failed");
    hipLaunchKernelGGL(raw_parts_kernel, dim3((o.n + 1 + 255) / 256), dim3(256), 0, c->stream, (const uint32_t*)o.key, pos, o.n, o.hdr, o.list, RAW_MAX_DATES);
    (void)hipEventRecord(done, c->stream);
    HIPCHK(c, hipGetLastError());
    *launches += launched;  // (the caller's kernels in front and the two here: counted once they are launched, before the readback)
    HIPCHK(c, hipMemcpyAsync(t->h_list, o.hdr, RAW_LIST_FIRST, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *h = *(const RawPartsHeader*)t->h_list.get();
    ent->assign(h->nparts <= RAW_MAX_DATES ? h->nparts : 0, RawPartEntry{});
    const size_t first = std::min<size_t>(ent->size(), (RAW_LIST_FIRST - sizeof(RawPartsHeader)) / sizeof(RawPartEntry));
    if (first) memcpy(ent->data(), t->h_list.get() + sizeof(RawPartsHeader), first * sizeof(RawPartEntry));
    if (ent->size() > first) HIPCHK(c, hipMemcpy(ent->data() + first, o.list + first, (ent->size() - first) * sizeof(RawPartEntry), hipMemcpyDeviceToHost));
    std::sort(ent->begin(), ent->end(), [](const RawPartEntry& x, const RawPartEntry& y) { return x.start < y.start; });
    return FA_OK;
}

// the sorted entries -> the parts' descriptions, laid back to back from `offset` on
static std::vector<fa_raw_part> raw_lay_out(const RawPartsHeader& h, const std::vector<RawPartEntry>& ent, size_t offset) {
    std::vector<fa_raw_part> parts(ent.size());
    for (size_t i = 0; i < ent.size(); i++) {
        const bool last = i + 1 == ent.size();
        fa_raw_part& p = parts[i];
        p.date = ent[i].t_min / 86400u;
        p.t_min = ent[i].t_min;
        p.t_max = last ? h.last_t_max : ent[i + 1].prev_t_max;
        p.rows = (last ? h.good : ent[i + 1].start) - ent[i].start;
        p.offset = offset;
        p.bytes = fa_raw_part_bytes(p.rows);
        offset += p.bytes;
    }
    return parts;
}
// the workgroups that write a part of `rows` rows at `part`
static dim3 raw_part_grid(const uint8_t* part, uint64_t rows) { return dim3((unsigned)raw_part_tiles(RAW_COLS_H, (uint64_t)(uintptr_t)part, rows)); }

// One chunk of m <= raw_chunk_cap decoded records -> its parts appended to the image.
static int raw_build_chunk(fa_ctx* c, const fa_columns& cols, size_t m) {
    RawState* t = c->raw;
    if (m == 0) return FA_OK;
    raw_read_events(t);
    // scratch: flags and positions (m + 1 words each) in front of the order step's
    const uint32_t n = (uint32_t)m;
    size_t tmp_scan = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_scan, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(n + 1), c->stream);
    RawOrder o(c, n, tmp_scan);
    int rc = ensure_dev(c, t->scratch, 2 * o.words + o.bytes(), "raw part scratch");
    if (rc) return rc;
    uint8_t* sb = (uint8_t*)t->scratch.get();
    uint32_t *flag = (uint32_t*)sb, *pos = (uint32_t*)(sb + o.words);
    o.carve(sb + 2 * o.words);

    // ---- order
    const dim3 grid((n + 1 + 255) / 256), block(256);
    (void)hipEventRecord(t->ev[0], c->stream);
    hipLaunchKernelGGL(raw_flag_kernel, grid, block, 0, c->stream, cols.status, n, flag);
    size_t tb = o.tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(o.tmp, tb, (const uint32_t*)flag, pos, (int)(n + 1), c->stream) != hipSuccess) return fail(c, FA_ERR_HIP, "scan failed");
    hipLaunchKernelGGL(raw_key_kernel, grid, block, 0, c->stream, cols.status, cols.time_received, n, (const uint32_t*)pos, o.key_in, o.idx_in);
    RawPartsHeader h;
    std::vector<RawPartEntry> ent;
    rc = raw_order_and_list(c, o, pos, t->ev[1], &t->launches, 5, &h, &ent);
    if (rc) return rc;
    Events::elapsed_ns(t->ev[0], t->ev[1], &t->order_ns);
    if (h.good > n || h.nparts > RAW_MAX_DATES || (h.good != 0) != (h.nparts != 0)) return fail(c, FA_ERR_HIP, "internal: the raw part list is inconsistent");
    // (the counters move only once the chunk's parts are certain to be built: rows_out + records_bad == records_in always holds)
    auto count_chunk = [&] {
        t->records_in += n;
        t->records_bad += n - h.good;
        t->chunks++;
    };
    if (!h.nparts) {
        count_chunk();
        return FA_OK;
    }
    // ---- the image's layout, then the gather: one launch per part
    const std::vector<fa_raw_part> parts = raw_lay_out(h, ent, t->used);
    rc = raw_reserve_image(c, parts.back().offset + parts.back().bytes - t->used);
    if (rc) return rc;
    count_chunk();
    (void)hipEventRecord(t->ev[2], c->stream);  // (behind the part list's round trip and the image's growth: the gather launches alone)
    for (size_t i = 0; i < parts.size(); i++) {
        const fa_raw_part& p = parts[i];
        RawGatherArgs a{};
        a.part = t->img + p.offset;
        a.key = o.key + ent[i].start;
        a.idx = o.idx + ent[i].start;
        const void* src[RAW_NCOLS] = {nullptr, nullptr, cols.time_flow_start, cols.sequence_num, cols.sampling_rate, cols.sampler_address, cols.src_addr, cols.dst_addr,
                                      cols.src_as, cols.dst_as, cols.etype, cols.proto, cols.src_port, cols.dst_port, cols.bytes, cols.packets};
        memcpy(a.src, src, sizeof src);
        a.rows = (uint32_t)p.rows;
        a.date = p.date;
        hipLaunchKernelGGL(raw_gather_kernel, raw_part_grid(a.part, p.rows), dim3(RAW_BLOCK), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        t->launches++;
        t->used += p.bytes;
        t->pending.push_back(p);
        t->rows_out += p.rows;
        t->parts_out++;
        t->bytes_out += p.bytes;
    }
    (void)hipEventRecord(t->ev[3], c->stream);
    t->ev_pending = true;
    return FA_OK;
}

static fa_columns raw_cols_at(const fa_columns& s, size_t i) {
    fa_columns o = s;
    o.time_received += i, o.time_flow_start += i, o.sampling_rate += i, o.bytes += i, o.packets += i;
    o.sequence_num += i, o.src_as += i, o.dst_as += i, o.etype += i, o.proto += i, o.src_port += i, o.dst_port += i;
    o.sampler_address += 16 * i, o.src_addr += 16 * i, o.dst_addr += 16 * i;
    o.status += i;
    return o;
}

// n decoded records -> parts, a chunk at a time
static int raw_build_cols(fa_ctx* c, const fa_columns& cols, size_t n) {
    for (size_t i = 0; i < n;) {
        const size_t m = std::min(n - i, raw_chunk_cap(c));
        int rc = raw_build_chunk(c, raw_cols_at(cols, i), m);
        if (rc) return rc;
        i += m;
    }
    return FA_OK;
}

extern "C" int fa_raw_build_columns_device(fa_ctx* c, const fa_columns* cols, size_t n) {
    RAW_ENTER(c, "fa_raw_build_columns_device");
    if (n == 0) return FA_OK;
    if (!cols) return fail(c, FA_ERR_ARG, "fa_raw_build_columns_device: null argument");
    const void* p8[] = {cols->time_received, cols->time_flow_start, cols->sampling_rate, cols->bytes, cols->packets};
    const void* p4[] = {cols->sequence_num, cols->src_as, cols->dst_as, cols->etype, cols->proto, cols->src_port, cols->dst_port};
    const void* p16[] = {cols->sampler_address, cols->src_addr, cols->dst_addr};
    bool ok = cols->status != nullptr;
    for (const void* p : p8) ok = ok && p && !((uintptr_t)p & 7);
    for (const void* p : p4) ok = ok && p && !((uintptr_t)p & 3);
    for (const void* p : p16) ok = ok && p && !((uintptr_t)p & 15);
    if (!ok) return fail(c, FA_ERR_ARG, "fa_raw_build_columns_device: all 15 columns and status are needed, each naturally aligned (8 / 4 / 16 / 1 bytes)");
    const int rc = raw_build_cols(c, *cols, n);
    // the gather launches of the last chunk still read the caller's columns: they are done before the call returns
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    HIPCHK(c, e);
    return FA_OK;
}

// ---- take, reset, statistics -----------------------------------------------------------------------------------------------------
static int raw_take_check(fa_ctx* c, size_t cap, bool have_out, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts) {
    RawState* t = c->raw;
    *bytes_out = t->used;
    *n_parts = t->pending.size();
    if (t->used > cap || (t->used && !have_out) || t->pending.size() > parts_cap || (!parts && !t->pending.empty()))
        return fail(c, FA_ERR_CAPACITY, "fa_raw_take: a buffer is too small (bytes and parts needed are returned); nothing was taken");
    return FA_OK;
}
static void raw_clear(RawState* t, fa_raw_part* parts) {
    if (parts && !t->pending.empty()) memcpy(parts, t->pending.data(), t->pending.size() * sizeof(fa_raw_part));
    t->pending.clear();
    t->used = 0;
    t->takes++;
}

extern "C" int fa_raw_take(fa_ctx* c, uint8_t* out, size_t cap, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts) {
    RAW_ENTER(c, "fa_raw_take");
    if (!bytes_out || !n_parts) return fail(c, FA_ERR_ARG, "fa_raw_take: null argument");
    RawState* t = c->raw;
    int rc = raw_take_check(c, cap, out != nullptr, bytes_out, parts, parts_cap, n_parts);
    if (rc) return rc;
    if (t->used) HIPCHK(c, hipMemcpyAsync(out, t->img, t->used, hipMemcpyDeviceToHost, c->stream));  // (page-locked `out`: one copy-engine transfer)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    raw_read_events(t);
    raw_clear(t, parts);
    return FA_OK;
}

extern "C" int fa_raw_take_device(fa_ctx* c, const void** d_bytes, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts) {
    RAW_ENTER(c, "fa_raw_take_device");
    if (!d_bytes || !bytes_out || !n_parts) return fail(c, FA_ERR_ARG, "fa_raw_take_device: null argument");
    RawState* t = c->raw;
    *d_bytes = nullptr;
    int rc = raw_take_check(c, t->used, true, bytes_out, parts, parts_cap, n_parts);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    raw_read_events(t);
    *d_bytes = t->used ? t->img.get() : nullptr;
    raw_clear(t, parts);
    return FA_OK;
}

// Drops the pending parts and releases the image and the scratch; the counters of fa_raw_stats go on counting.
extern "C" int fa_raw_reset(fa_ctx* c) {
    RAW_ENTER(c, "fa_raw_reset");
    RawState* t = c->raw;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    raw_read_events(t);
    raw_clear(t, nullptr);
    t->img.reset();
    t->scratch.reset();
    raw_merge_release(c);
    lz4_release(c);
    load_release(c);
    pending_release(c);
    return FA_OK;
}

extern "C" int fa_raw_stats(fa_ctx* c, fa_raw_stats_t* out) {
    RAW_ENTER(c, "fa_raw_stats");
    if (!out) return fail(c, FA_ERR_ARG, "fa_raw_stats: null argument");
    RawState* t = c->raw;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    raw_read_events(t);
    out->records_in = t->records_in;
    out->records_bad = t->records_bad;
    out->rows_out = t->rows_out;
    out->parts_out = t->parts_out;
    out->bytes_out = t->bytes_out;
    out->chunks = t->chunks;
    out->pending_parts = t->pending.size();
    out->pending_bytes = t->used;
    out->build_ns_total = t->order_ns + t->gather_ns;
    out->build_launches = t->launches;
    return FA_OK;
}
