// raw_load_host.inc - loading flows_raw parts back (included by flowagg.hip behind second_pass.inc: one translation unit;
// device side: lz4_decode.cuh, raw.cuh "loading parts back"; the contract: include/flowagg.h "loading flows_raw parts").
//
// One call (load_prepare): the host walks the frames - or the plain parts' row counts - and builds the block and part plans; ONE
// copy brings the input to HBM; lz4_decode_kernel fills a 64 KiB slot per block; raw_header_check_kernel gives every part's
// rows and verdict; ONE copy brings every block's status and every part's verdict back and the stream is waited for ONCE.
// Everything is validated there, before the first unpack or fold launch: a refused call folds nothing.  Then, per part and in
// chunks of at most the enabled folds' caps: raw_unpack_kernel into the ctx's column chunk, fold_chunk_cols (second_pass.inc).
// raw_build_cols is never called: loading parts does not produce parts.  fa_raw_load touches neither flows_5m nor the wide table;
// the door that feeds them from the same front half (load_prepare, load_columns, load_unpack) is fa_raw_load_rollup
// (rollup_host.inc); fa_raw_restore (sketch_fold_host.inc) feeds those, the sketches and the folds from it in one pass.
// Memory (LoadState, kept until fa_raw_reset / fa_destroy): the input's copy, 64 KiB per block of decoded image, 40 bytes per
// block and 48 per part of plan and verdicts, one chunk of columns.

struct LoadState {
    DevBuf<uint8_t> in;   // the call's input bytes
    DevBuf<uint8_t> img;  // the decoded image: a 64 KiB slot per block (LZ4 input; plain input is read where `in` holds it)
    DevBuf<> meta;        // block plan, part plan | block status, part verdicts (the second half comes back in one copy)
    PinnedBuf<> h_meta;   // both halves on their way
    DevBuf<> cols;        // one chunk of columns (fa_raw_columns_device: every row of the call)
    Events ev;            // [0], [1]: around the decode kernel; then per chunk: before unpack, behind unpack, behind the folds
    uint64_t calls = 0, frames = 0, blocks = 0, stored = 0, bytes_in = 0, bytes_decoded = 0, parts = 0, rows_loaded = 0, launches = 0;
    uint64_t decode_ns = 0, unpack_ns = 0, fold_ns = 0;
};
static constexpr size_t LOAD_EV_MAX = 2 + 3 * 256;  // chunks whose times are pending before the stream is waited for

// fa_raw_load_reset, fa_raw_reset: the buffers go, the counters of fa_raw_load_stats go on counting
static void load_release(fa_ctx* c) {
    LoadState* s = c->load;
    if (!s) return;
    s->in.reset(), s->img.reset(), s->meta.reset(), s->h_meta.reset(), s->cols.reset();
    select_release(c);
    query_release(c);
}
static int load_state(fa_ctx* c, LoadState** out) {
    select_drop(c);  // (every decode, load, restore, range and select door starts here: a selection lives until the next of them)
    const int rc = state_with_events(c, c->load, 2);
    if (rc == FA_OK) c->load->ev.rewind(2);  // (the decode's pair stays; chunk events of a call that failed half-way are dropped unread)
    *out = c->load;
    return rc;
}
// the chunks' events (the stream was waited for): their times are added, the pool is free again
static void load_read_events(LoadState* s) {
    for (size_t i = 2; i + 2 < s->ev.used(); i += 3) {
        Events::elapsed_ns(s->ev[i], s->ev[i + 1], &s->unpack_ns);
        Events::elapsed_ns(s->ev[i + 1], s->ev[i + 2], &s->fold_ns);
    }
    s->ev.rewind(2);
}

// ---- host only: the twin (the frame walk and the decoder over lz4_seq_parse: lz4_decode.cuh) ---------------------------------------
extern "C" int fa_lz4_decode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* bytes_out) {
    if ((!in && n) || !bytes_out) return FA_ERR_ARG;
    std::vector<uint8_t> dec;
    std::string err;
    if (!lz4_frames_decode_host(in, n, dec, &err)) return FA_ERR_FRAMING;
    *bytes_out = dec.size();
    if (dec.size() > cap || (!dec.empty() && !out)) return FA_ERR_CAPACITY;
    if (!dec.empty()) memcpy(out, dec.data(), dec.size());
    return FA_OK;
}

// ---- one call's preparation: decode, header check, ONE copy back, ONE wait --------------------------------------------------------
struct LoadPart {
    const uint8_t* d;  // the part's first byte in HBM
    uint64_t bytes, rows;
};
struct LoadPrepared {
    size_t frames_cap = (size_t)-1;  // in: more frames than this is FA_ERR_CAPACITY, found by the host's walk before anything is copied or counted
    Lz4Walk walk;                    // (empty for plain Native input)
    std::vector<uint64_t> frame_bytes;
    std::vector<LoadPart> parts;  // (want_parts only)
};

// why raw_header_check_kernel refused a part (empty: no such code)
static std::string load_verdict_why(const RawPartVerdict& v) {
    switch (v.code) {
    case RAW_V_SIZE: return std::to_string(v.bytes) + " bytes fit no row count of a flows_raw part (a truncated part or trailing bytes)";
    case RAW_V_NCOLS: return "a flows_raw block has 16 columns, not this column count";
    case RAW_V_ROWS: return "the row count at byte " + std::to_string(v.at) + " is not the one the part's size gives (a size that fits no row count, or trailing bytes)";
    case RAW_V_NAME: return "column " + std::to_string(v.at) + " has a wrong name (" + RAW_COLS_H[v.at & 15].name + " is expected)";
    case RAW_V_TYPE: return "column " + std::to_string(v.at) + " has a wrong type (" + RAW_COLS_H[v.at & 15].type + " is expected)";
    default: return std::string();
    }
}

// The host's half: the frames walked (or the plain parts' row counts read) -> pr.walk and one RawPartPlan per part.  Nothing is
// copied or counted.  (Shared with the ranged doors, raw_range_host.inc.)
static int load_walk(fa_ctx* c, const char* fn, const uint8_t* in, size_t n, bool want_parts, LoadPrepared& pr, std::vector<RawPartPlan>& pplan, bool* is_lz4) {
    auto framing = [&](const std::string& why) {
        c->err = std::string(fn) + ": " + why;
        return FA_ERR_FRAMING;
    };
    const bool lz4 = !want_parts || (n >= 4 && (lz4_read32(in) == 0x184D2204u || (lz4_read32(in) >= 0x184D2A50u && lz4_read32(in) <= 0x184D2A5Fu)));
    std::string err;
    if (lz4) {
        if (!lz4_walk_frames(in, n, pr.walk, &err)) return framing(err);
        if (pr.walk.first.size() - 1 > pr.frames_cap) return fail(c, FA_ERR_CAPACITY, "the span buffer is too small (the frames needed are returned); nothing was decoded");
        if (want_parts)
            for (uint32_t f = 0; f + 1 < pr.walk.first.size(); f++)
                pplan.push_back({(uint64_t)pr.walk.first[f] * LZ4_BLOCK_MAX, 0, pr.walk.first[f], pr.walk.first[f + 1] - pr.walk.first[f]});
    } else {  // plain Native parts: the row count at a part's head gives its size; everything else is checked on the device
        for (size_t p = 0; p < n;) {
            if (in[p] != RAW_NCOLS) return framing(lz4_at_byte(p ? "a flows_raw block has 16 columns: no such block starts" : "neither an LZ4 frame nor a flows_raw Native block (16 columns) starts", p));
            uint64_t rows = 0;
            size_t q = p + 1;
            for (uint32_t shift = 0;; shift += 7) {
                if (q >= n || shift > 63) return framing(lz4_at_byte("truncated or overlong row count", q));
                const uint8_t x = in[q++];
                rows |= (uint64_t)(x & 127) << shift;
                if (x < 128) break;
            }
            if (rows > ((uint64_t)1 << 31) || fa_raw_part_bytes(rows) > n - p)
                return framing(lz4_at_byte("a part of " + std::to_string(rows) + " rows does not fit the bytes that are left (a size that fits no row count, or trailing bytes)", p));
            pplan.push_back({(uint64_t)p, (uint64_t)fa_raw_part_bytes(rows), 0, 0xFFFFFFFFu});
            p += fa_raw_part_bytes(rows);
        }
    }
    *is_lz4 = lz4;
    return FA_OK;
}

// in[0, n) -> the decoded image in HBM.  want_parts: the input is LZ4 frames or plain Native parts, told apart by its first four
// bytes, and every frame (or plain block) is also checked as a flows_raw part; otherwise it is LZ4 frames.
// FA_ERR_FRAMING (text in fa_last_error) on the first violation in input order; nothing was unpacked or folded then.
static int load_prepare(fa_ctx* c, LoadState* s, const char* fn, const uint8_t* in, size_t n, bool want_parts, LoadPrepared& pr) {
    auto framing = [&](const std::string& why) {
        c->err = std::string(fn) + ": " + why;
        return FA_ERR_FRAMING;
    };
    std::string err;
    std::vector<RawPartPlan> pplan;
    bool lz4 = false;
    int rc = load_walk(c, fn, in, n, want_parts, pr, pplan, &lz4);
    if (rc) return rc;
    const size_t nb = pr.walk.blocks.size(), np = pplan.size();
    if (n == 0) return FA_OK;
    // ---- buffers
    const size_t plan_b = align256(nb * sizeof(Lz4DBlock)), pplan_b = align256(np * sizeof(RawPartPlan));
    const size_t st_b = align256(nb * sizeof(Lz4DecStatus)), ver_b = align256(np * sizeof(RawPartVerdict));
    rc = ensure_dev(c, s->meta, plan_b + pplan_b + st_b + ver_b + 256, "load plan");
    if (rc) return rc;
    bool ok = s->h_meta.grow(std::max(plan_b + pplan_b, st_b + ver_b) + 256) && s->in.grow(n + 16) && s->img.grow(std::max<size_t>(nb, 1) * LZ4_BLOCK_MAX);
    if (!ok) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "hipMalloc(load: input copy / decoded image) failed; nothing was loaded (load the file in pieces cut at frame boundaries)");
    }
    uint8_t *mb = (uint8_t*)s->meta.get(), *hb = (uint8_t*)s->h_meta.get();
    Lz4DBlock *d_plan = (Lz4DBlock*)mb, *h_plan = (Lz4DBlock*)hb;
    RawPartPlan* d_pplan = (RawPartPlan*)(mb + plan_b);
    Lz4DecStatus* d_st = (Lz4DecStatus*)(mb + plan_b + pplan_b);
    RawPartVerdict* d_ver = (RawPartVerdict*)(mb + plan_b + pplan_b + st_b);
    for (size_t b = 0; b < nb; b++) h_plan[b] = Lz4DBlock{pr.walk.blocks[b].at, (uint64_t)b * LZ4_BLOCK_MAX, pr.walk.blocks[b].n, pr.walk.blocks[b].stored ? (uint32_t)LZ4D_F_STORED : 0u};
    if (np) memcpy(hb + plan_b, pplan.data(), np * sizeof(RawPartPlan));
    // ---- copy in, decode, check the headers
    HIPCHK(c, hipMemcpyAsync(s->in, in, n, hipMemcpyHostToDevice, c->stream));
    if (nb + np) HIPCHK(c, hipMemcpyAsync(mb, hb, plan_b + pplan_b, hipMemcpyHostToDevice, c->stream));
    uint64_t launches = 0;
    if (nb) {
        (void)hipEventRecord(s->ev[0], c->stream);
        hipLaunchKernelGGL(lz4_decode_kernel, dim3((unsigned)((nb + LZ4D_WAVES - 1) / LZ4D_WAVES)), dim3(64 * LZ4D_WAVES), 0, c->stream, (const Lz4DBlock*)d_plan, (uint32_t)nb,
                           (const uint8_t*)s->in.get(), s->img.get(), d_st);
        (void)hipEventRecord(s->ev[1], c->stream);
        launches++;
    }
    const uint8_t* image = lz4 ? s->img.get() : s->in.get();
    if (np) {
        hipLaunchKernelGGL(raw_header_check_kernel, dim3((unsigned)np), dim3(64), 0, c->stream, (const RawPartPlan*)d_pplan, (const uint32_t*)d_st, image, d_ver);
        launches++;
    }
    HIPCHK(c, hipGetLastError());
    // ---- every block's status and every part's verdict: one copy, one wait (the plans' staging is free again: the stream is in order)
    if (nb + np) HIPCHK(c, hipMemcpyAsync(hb, d_st, st_b + ver_b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s->launches += launches;
    if (nb) Events::elapsed_ns(s->ev[0], s->ev[1], &s->decode_ns);
    const Lz4DecStatus* st = (const Lz4DecStatus*)hb;
    const RawPartVerdict* ver = (const RawPartVerdict*)(hb + st_b);
    // ---- validation, in input order
    const size_t nf = lz4 ? pr.walk.first.size() - 1 : 0;
    pr.frame_bytes.resize(nf);
    for (size_t i = 0; i < std::max(nf, np); i++) {
        if (i < nf && !lz4_frame_verdict(pr.walk, (uint32_t)i, st, &pr.frame_bytes[i], &err)) return framing(err);
        if (i < np && ver[i].code) {
            const std::string where = lz4 ? "frame " + std::to_string(i) : "the part at byte " + std::to_string(pplan[i].off);
            const std::string v = load_verdict_why(ver[i]);
            if (v.empty()) return fail(c, FA_ERR_HIP, "internal: a part's verdict is inconsistent");
            return framing(where + ": " + v);
        }
        if (i < np) {
            if (ver[i].rows > ((uint64_t)1 << 31)) return fail(c, FA_ERR_ARG, "a part of more than 2^31 rows");
            pr.parts.push_back({image + pplan[i].off, ver[i].bytes, ver[i].rows});
        }
    }
    uint64_t dec = 0, stored = 0;
    for (size_t b = 0; b < nb; b++) dec += st[b].size, stored += pr.walk.blocks[b].stored;
    s->calls++, s->frames += nf, s->blocks += nb, s->stored += stored, s->bytes_in += n, s->bytes_decoded += dec, s->parts += np;
    return FA_OK;
}

#define LOAD_ENTER(c)                        \
    FA_ON_DEVICE(c);                         \
    if (!(c)) return FA_ERR_ARG;             \
    if ((c)->sticky) return (c)->sticky

extern "C" int fa_lz4_decode_device(fa_ctx* c, const uint8_t* in, size_t n, const void** d_out, fa_lz4_span* spans, size_t spans_cap, size_t* n_frames) {
    LOAD_ENTER(c);
    if ((!in && n) || !d_out || !n_frames) return fail(c, FA_ERR_ARG, "fa_lz4_decode_device: null argument");
    *d_out = nullptr, *n_frames = 0;
    LoadState* s = nullptr;
    int rc = load_state(c, &s);
    if (rc) return rc;
    LoadPrepared pr;
    pr.frames_cap = spans ? spans_cap : 0;
    rc = load_prepare(c, s, "fa_lz4_decode_device", in, n, false, pr);
    if (rc == FA_ERR_CAPACITY) *n_frames = pr.walk.first.size() - 1;
    if (rc) return rc;
    const size_t nf = pr.frame_bytes.size();
    *n_frames = nf;
    for (size_t f = 0; f < nf; f++) spans[f] = fa_lz4_span{(uint64_t)pr.walk.first[f] * LZ4_BLOCK_MAX, pr.frame_bytes[f]};
    *d_out = n ? s->img.get() : nullptr;
    return FA_OK;
}

// the ctx's column chunk for `cap` rows: every array 256-byte aligned
static int load_columns(fa_ctx* c, LoadState* s, size_t cap, fa_columns* out, void* dst[RAW_NCOLS]) {
    const size_t a8 = align256(cap * 8), a4 = align256(cap * 4), a16 = align256(cap * 16), a1 = align256(cap);
    int rc = ensure_dev(c, s->cols, 5 * a8 + 7 * a4 + 3 * a16 + a1, "load columns");
    if (rc) return rc;
    uint8_t* p = (uint8_t*)s->cols.get();
    auto take = [&](size_t b) {
        uint8_t* r = p;
        p += b;
        return r;
    };
    fa_columns o{};
    o.time_received = (const uint64_t*)take(a8), o.time_flow_start = (const uint64_t*)take(a8), o.sampling_rate = (const uint64_t*)take(a8);
    o.bytes = (const uint64_t*)take(a8), o.packets = (const uint64_t*)take(a8);
    o.sampler_address = take(a16), o.src_addr = take(a16), o.dst_addr = take(a16);
    o.sequence_num = (const uint32_t*)take(a4), o.src_as = (const uint32_t*)take(a4), o.dst_as = (const uint32_t*)take(a4), o.etype = (const uint32_t*)take(a4);
    o.proto = (const uint32_t*)take(a4), o.src_port = (const uint32_t*)take(a4), o.dst_port = (const uint32_t*)take(a4);
    o.status = take(a1);
    *out = o;
    // (in the order of RAW_COLS; Date has no array)
    const void* d[RAW_NCOLS] = {nullptr, o.time_received, o.time_flow_start, o.sequence_num, o.sampling_rate, o.sampler_address, o.src_addr, o.dst_addr,
                                o.src_as, o.dst_as, o.etype, o.proto, o.src_port, o.dst_port, o.bytes, o.packets};
    for (uint32_t i = 0; i < RAW_NCOLS; i++) dst[i] = const_cast<void*>(d[i]);
    return FA_OK;
}
// rows [r0, r0 + m) of a part -> the column arrays from element `at` on (any element: the kernel's chunks follow the destination's alignment)
static int load_unpack(fa_ctx* c, LoadState* s, const LoadPart& part, uint32_t r0, uint32_t m, void* const dst[RAW_NCOLS], size_t at) {
    if (!m) return FA_OK;
    RawUnpackArgs a{};
    a.part = part.d, a.lo = part.d, a.hi = part.d + part.bytes;
    a.rows = (uint32_t)part.rows, a.r0 = r0, a.m = m;
    for (uint32_t i = 1; i < RAW_NCOLS; i++) a.dst[i] = (uint8_t*)dst[i] + at * (RAW_COLS_H[i].kind == RAW_K_KEY || RAW_COLS_H[i].kind == RAW_K_NARROW64 ? 8 : RAW_COLS_H[i].width);
    hipLaunchKernelGGL(raw_unpack_kernel, dim3((unsigned)(((size_t)m * 16 + 16 * RAW_BLOCK - 1) / (16 * RAW_BLOCK)), RAW_NCOLS - 1), dim3(RAW_BLOCK), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    s->launches++;
    return FA_OK;
}
// One chunk of a load door, timed: rows [r0, r0 + m) of a part unpacked into the ctx's column chunk and handed to fold(cols, m).
// A failed unpack returns before the chunk's three events count; a failed fold after they do (the next call drops them unread).
template <class Fold>
static int load_chunk(fa_ctx* c, LoadState* s, const LoadPart& part, uint64_t r0, size_t m, Fold&& fold) {
    fa_columns cols;
    void* dst[RAW_NCOLS];
    int rc = load_columns(c, s, m, &cols, dst);
    if (rc) return rc;
    if (s->ev.used() + 3 > LOAD_EV_MAX) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        load_read_events(s);
    }
    const size_t at = s->ev.used();
    if (!s->ev.ensure(at + 3)) return events_failed(c);
    (void)hipEventRecord(s->ev[at], c->stream);
    HIPCHK(c, hipMemsetAsync(const_cast<uint8_t*>(cols.status), 0, m, c->stream));
    rc = load_unpack(c, s, part, (uint32_t)r0, (uint32_t)m, dst, 0);
    if (rc) return rc;
    (void)hipEventRecord(s->ev[at + 1], c->stream);
    rc = fold(cols, m);
    (void)hipEventRecord(s->ev[at + 2], c->stream);
    s->ev.take(3);  // (the chunk's events count from here on: they exist, nothing is created)
    if (rc) return rc;
    s->rows_loaded += m;
    return FA_OK;
}

extern "C" int fa_raw_columns_device(fa_ctx* c, const uint8_t* bytes, size_t n, fa_columns* out, size_t* rows_out) {
    LOAD_ENTER(c);
    if ((!bytes && n) || !out || !rows_out) return fail(c, FA_ERR_ARG, "fa_raw_columns_device: null argument");
    memset(out, 0, sizeof *out);
    *rows_out = 0;
    LoadState* s = nullptr;
    int rc = load_state(c, &s);
    if (rc) return rc;
    LoadPrepared pr;
    rc = load_prepare(c, s, "fa_raw_columns_device", bytes, n, true, pr);
    if (rc) return rc;
    uint64_t total = 0;
    for (const LoadPart& p : pr.parts) total += p.rows;
    if (total > ((uint64_t)1 << 24)) return fail(c, FA_ERR_ARG, "fa_raw_columns_device: more than 2^24 rows in one call");
    if (!total) return FA_OK;
    void* dst[RAW_NCOLS];
    rc = load_columns(c, s, (size_t)total, out, dst);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(const_cast<uint8_t*>(out->status), 0, (size_t)total, c->stream));
    size_t at = 0;
    for (const LoadPart& p : pr.parts) {  // parts stand in input order, back to back
        rc = load_unpack(c, s, p, 0, (uint32_t)p.rows, dst, at);
        if (rc) return rc;
        at += p.rows;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *rows_out = (size_t)total;
    return FA_OK;
}

extern "C" int fa_raw_load(fa_ctx* c, const uint8_t* bytes, size_t n) {
    LOAD_ENTER(c);
    if (!c->talk && !c->ports) return fail(c, FA_ERR_UNSUPPORTED, "fa_raw_load: neither fa_talkers_enable(_buckets) nor fa_ports_enable_buckets was called on this ctx: nothing to load into");
    if (!bytes && n) return fail(c, FA_ERR_ARG, "fa_raw_load: null argument");
    LoadState* s = nullptr;
    int rc = load_state(c, &s);
    if (rc) return rc;
    LoadPrepared pr;
    rc = load_prepare(c, s, "fa_raw_load", bytes, n, true, pr);
    if (rc) return rc;
    // (from here on the input is known to be whole: every frame, block and header was validated at load_prepare's one wait)
    for (const LoadPart& p : pr.parts)
        for (uint64_t r0 = 0; r0 < p.rows;) {
            size_t m = (size_t)std::min<uint64_t>(p.rows - r0, (uint64_t)1 << 24);
            if (c->talk) m = std::min(m, talk_chunk_cap(c));
            if (c->ports) m = std::min(m, port_chunk_cap(c));
            rc = load_chunk(c, s, p, r0, m, [&](const fa_columns& cols, size_t m) { return fold_chunk_cols(c, cols, m); });
            if (rc) return rc;
            r0 += m;
        }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    load_read_events(s);
    return FA_OK;
}

// Releases the buffers of the decode / load doors and of the LZ4 compressions, on any ctx (fa_raw_reset, which needs
// fa_raw_enable, does the same beside the parts' image); the counters go on counting.
extern "C" int fa_raw_load_reset(fa_ctx* c) {
    LOAD_ENTER(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    load_release(c);
    lz4_release(c);
    return FA_OK;
}

extern "C" int fa_raw_load_stats(fa_ctx* c, fa_raw_load_stats_t* out) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (!out) return fail(c, FA_ERR_ARG, "fa_raw_load_stats: null argument");
    memset(out, 0, sizeof *out);
    const LoadState* s = c->load;
    if (!s) return FA_OK;
    out->calls = s->calls, out->frames = s->frames, out->blocks = s->blocks, out->stored_blocks = s->stored;
    out->bytes_in = s->bytes_in, out->bytes_decoded = s->bytes_decoded, out->parts = s->parts, out->rows_loaded = s->rows_loaded;
    out->launches = s->launches, out->decode_ns = s->decode_ns, out->unpack_ns = s->unpack_ns, out->fold_ns = s->fold_ns;
    return FA_OK;
}
