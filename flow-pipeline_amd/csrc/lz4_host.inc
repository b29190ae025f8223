// lz4_host.inc - host side of the LZ4 frames (included by flowagg.hip: one translation unit; device side and the format: lz4.cuh).
// fa_raw_take_lz4 compresses the pending flows_raw parts where they lie (RawState::img) - one frame per part, one wave per
// 64 KiB block - and delivers the frames with one copy of about a quarter of the bytes; fa_lz4_frame_device does the same for
// any bytes in HBM; fa_lz4_frame is the host twin (a plain greedy encoder over the same helpers).
//
// One compression (lz4_compress): the host knows every input's size, so the block plan - block -> (input offset, bytes,
// first / last of its frame, frame index) - is built on the host and copied in; lz4_block_kernel fills a slot per block and
// writes the bytes each block will take; an exclusive scan (hipcub) turns those into positions; lz4_pack_kernel moves every
// block, its size word, the frame headers and the EndMarks into place; one small copy brings the frames' starts, the total and
// the number of stored blocks back, and the stream is waited for once.
// Memory, kept until fa_raw_reset / fa_destroy: a 64 KiB slot per block of the largest compression (= its input's size), the
// frames (allocated to the bound: input + 4 bytes per block + 11 per frame), 40 bytes per block of plan and sizes.

struct Lz4Src {  // one frame's input in HBM
    const uint8_t* d;
    size_t bytes;
};

struct Lz4State {
    DevBuf<uint8_t> slots;  // LZ4_BLOCK_MAX bytes per block
    DevBuf<> meta;          // plan, val, off, frame_off, sizes, hipcub storage
    PinnedBuf<> h_meta;     // the plan on its way in; the frames' starts, the total and the stored blocks on their way back
    // the frames of the first starts.size() pending parts of the ctx's RawState, made while its take counter stood at raw_takes:
    // kept across a take that failed for capacity, so that the retry compresses only what was built in between
    DevBuf<uint8_t> frames;
    size_t frames_used = 0;
    std::vector<uint64_t> starts;
    uint64_t raw_takes = 0;
    DevBuf<uint8_t> one;  // fa_lz4_frame_device's result
    Events ev;            // 3: before / behind the block kernel, behind the pack kernel
    uint64_t n_frames = 0, n_blocks = 0, n_stored = 0, bytes_in = 0, bytes_out = 0, launches = 0, block_ns = 0, pack_ns = 0;
};

// fa_raw_reset: the buffers go, the counters of fa_raw_lz4_stats go on counting
static void lz4_release(fa_ctx* c) {
    Lz4State* z = c->lz4;
    if (!z) return;
    z->slots.reset(), z->meta.reset(), z->h_meta.reset(), z->frames.reset(), z->one.reset();
    z->frames_used = 0;
    z->starts.clear();
}
static int lz4_state(fa_ctx* c, Lz4State** out) {
    const int rc = state_with_events(c, c->lz4, 3);
    *out = c->lz4;
    return rc;
}

// ---- host only: the bound, the twin ------------------------------------------------------------------------------------------------
extern "C" size_t fa_lz4_frame_bound(size_t n) { return LZ4_HEADER_BYTES + LZ4_ENDMARK_BYTES + n + 4 * ((n + LZ4_BLOCK_MAX - 1) / LZ4_BLOCK_MAX); }

// one block, greedy: -> its compressed bytes in out (room for n - 1), or 0: it does not shrink and is stored
static uint32_t lz4_block_host(const uint8_t* src, uint32_t n, uint8_t* out, std::vector<int32_t>& tab) {
    tab.assign(LZ4_HASH_SIZE, -1);
    const uint32_t cap = n ? n - 1 : 0, mstarts = lz4_match_starts(n), mend = lz4_match_end(n);
    uint32_t anchor = 0, p = 0, o = 0;
    while (p < mstarts) {
        const uint32_t v = lz4_read32(src + p), h = lz4_hash(v);
        const int32_t cand = tab[h];
        tab[h] = (int32_t)p;
        if (cand < 0 || lz4_read32(src + cand) != v) {
            p++;
            continue;
        }
        uint32_t mlen = LZ4_MIN_MATCH;
        while (p + mlen < mend && src[p + mlen] == src[(uint32_t)cand + mlen]) mlen++;
        const uint32_t lit = p - anchor;
        if (o + lz4_seq_bytes(lit, mlen) > cap) return 0;
        o += lz4_put_head(out + o, lit, mlen, 0, 1);
        memcpy(out + o, src + anchor, lit), o += lit;
        o += lz4_put_match(out + o, p - (uint32_t)cand, mlen, 0, 1);
        anchor = p = p + mlen;
    }
    const uint32_t lit = n - anchor;
    if (o + lz4_seq_bytes(lit, 0) > cap) return 0;
    o += lz4_put_head(out + o, lit, 0, 0, 1);
    memcpy(out + o, src + anchor, lit);
    return o + lit;
}

extern "C" int fa_lz4_frame(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* bytes_out) {
    if ((!in && n) || !bytes_out) return FA_ERR_ARG;
    std::vector<uint8_t> f(fa_lz4_frame_bound(n));
    std::vector<int32_t> tab;
    lz4_frame_header(f.data());
    size_t o = LZ4_HEADER_BYTES;
    for (size_t at = 0; at < n; at += LZ4_BLOCK_MAX) {
        const uint32_t bn = (uint32_t)std::min<size_t>(LZ4_BLOCK_MAX, n - at);
        uint32_t word = lz4_block_host(in + at, bn, f.data() + o + 4, tab);
        if (!word) {
            memcpy(f.data() + o + 4, in + at, bn);
            word = bn | LZ4_STORED;
        }
        for (int i = 0; i < 4; i++) f[o + i] = (uint8_t)(word >> (8 * i));
        o += 4 + (word & ~LZ4_STORED);
    }
    memset(f.data() + o, 0, LZ4_ENDMARK_BYTES);
    o += LZ4_ENDMARK_BYTES;
    *bytes_out = o;
    if (o > cap || !out) return FA_ERR_CAPACITY;
    memcpy(out, f.data(), o);
    return FA_OK;
}

// ---- one compression -------------------------------------------------------------------------------------------------------------
// Room for `more` bytes behind out[0, used): a larger buffer is allocated first and the bytes are copied inside HBM.
static int lz4_reserve(fa_ctx* c, DevBuf<uint8_t>& out, size_t used, size_t more) {
    if (out.bytes() >= used + more) return FA_OK;
    DevBuf<uint8_t> bigger;
    if (!bigger.grow(used + more)) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "hipMalloc(LZ4 frames) failed; nothing was compressed");
    }
    if (used) HIPCHK(c, hipMemcpyAsync(bigger, out, used, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out = std::move(bigger);
    return FA_OK;
}

// Every input (none empty) becomes one frame, appended to out at *used; the frames' starts are appended to `starts`.  Synchronous.
static int lz4_compress(fa_ctx* c, Lz4State* z, const std::vector<Lz4Src>& in, DevBuf<uint8_t>& out, size_t* used, std::vector<uint64_t>& starts) {
    if (in.empty()) return FA_OK;
    size_t nb = 0, bytes = 0, bound = 0;
    for (const Lz4Src& s : in) nb += (s.bytes + LZ4_BLOCK_MAX - 1) / LZ4_BLOCK_MAX, bytes += s.bytes, bound += fa_lz4_frame_bound(s.bytes);
    const size_t nf = in.size();
    if (nb >= ((size_t)1 << 30) || nf >= ((size_t)1 << 30)) return fail(c, FA_ERR_ARG, "LZ4: more than 2^30 blocks or frames in one compression");
    int rc = lz4_reserve(c, out, *used, bound);
    if (rc) return rc;
    if (!z->slots.grow(nb * LZ4_BLOCK_MAX)) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "hipMalloc(LZ4 block slots) failed; nothing was compressed");
    }
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(nb + 1), c->stream);
    const size_t plan_b = align256(nb * sizeof(Lz4Block)), arr_b = align256((nb + 1) * 8), fo_b = align256((nf + 2) * 8), size_b = align256(nb * 4);
    rc = ensure_dev(c, z->meta, plan_b + 2 * arr_b + fo_b + size_b + align256(tmp_bytes), "LZ4 plan");
    if (rc) return rc;
    if (!z->h_meta.grow(std::max(plan_b, fo_b))) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "hipHostMalloc(LZ4 plan staging) failed; nothing was compressed");
    }
    uint8_t* mb = (uint8_t*)z->meta.get();
    Lz4Block* d_plan = (Lz4Block*)mb;
    unsigned long long *val = (unsigned long long*)(mb + plan_b), *off = (unsigned long long*)(mb + plan_b + arr_b), *fo = (unsigned long long*)(mb + plan_b + 2 * arr_b);
    uint32_t* sizes = (uint32_t*)(mb + plan_b + 2 * arr_b + fo_b);
    void* tmp = mb + plan_b + 2 * arr_b + fo_b + size_b;
    // ---- the block plan
    Lz4Block* h_plan = (Lz4Block*)z->h_meta.get();
    size_t b = 0;
    for (size_t f = 0; f < nf; f++)
        for (size_t at = 0; at < in[f].bytes; at += LZ4_BLOCK_MAX, b++) {
            h_plan[b].off = (uint64_t)(in[f].d - in[0].d) + at;  // (relative to the first input: two's complement if an input lies below it)
            h_plan[b].n = (uint32_t)std::min<size_t>(LZ4_BLOCK_MAX, in[f].bytes - at);
            h_plan[b].flags = (uint32_t)(f << 2) | (at == 0 ? LZ4_F_FIRST : 0) | (at + LZ4_BLOCK_MAX >= in[f].bytes ? LZ4_F_LAST : 0);
        }
    HIPCHK(c, hipMemcpyAsync(d_plan, h_plan, nb * sizeof(Lz4Block), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(val + nb, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(fo, 0, (nf + 2) * 8, c->stream));
    // ---- blocks, positions, pack
    (void)hipEventRecord(z->ev[0], c->stream);
    hipLaunchKernelGGL(lz4_block_kernel, dim3((unsigned)((nb + LZ4_WAVES - 1) / LZ4_WAVES)), dim3(64 * LZ4_WAVES), 0, c->stream, (const Lz4Block*)d_plan, (uint32_t)nb, in[0].d,
                       z->slots.get(), sizes, val);
    (void)hipEventRecord(z->ev[1], c->stream);
    size_t tb = tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(tmp, tb, (const unsigned long long*)val, off, (int)(nb + 1), c->stream) != hipSuccess) return fail(c, FA_ERR_HIP, "scan failed");
    hipLaunchKernelGGL(lz4_pack_kernel, dim3((unsigned)nb), dim3(LZ4_PACK_BLOCK), 0, c->stream, (const Lz4Block*)d_plan, (uint32_t)nb, in[0].d, (const uint8_t*)z->slots.get(),
                       (const uint32_t*)sizes, (const unsigned long long*)off, (uint32_t)nf, out.get(), (unsigned long long)*used, fo);
    (void)hipEventRecord(z->ev[2], c->stream);
    HIPCHK(c, hipGetLastError());
    // ---- the frames' starts, the total, the stored blocks: one small copy, one wait (the plan's staging is free again: the stream is in order)
    HIPCHK(c, hipMemcpyAsync(z->h_meta.get(), fo, (nf + 2) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned long long* h_fo = (const unsigned long long*)z->h_meta.get();
    const size_t end = h_fo[nf];
    bool ok = end > *used && end <= *used + bound && h_fo[nf + 1] <= nb;
    for (size_t f = 0; f < nf && ok; f++) ok = h_fo[f] >= *used && h_fo[f] < end && (f == 0 ? h_fo[f] == *used : h_fo[f] > h_fo[f - 1]);
    if (!ok) return fail(c, FA_ERR_HIP, "internal: the LZ4 frame offsets are inconsistent");
    Events::elapsed_ns(z->ev[0], z->ev[1], &z->block_ns);
    Events::elapsed_ns(z->ev[1], z->ev[2], &z->pack_ns);
    for (size_t f = 0; f < nf; f++) starts.push_back(h_fo[f]);
    z->n_frames += nf, z->n_blocks += nb, z->n_stored += h_fo[nf + 1], z->bytes_in += bytes, z->bytes_out += end - *used, z->launches += 3;
    *used = end;
    return FA_OK;
}

// ---- the takes -------------------------------------------------------------------------------------------------------------------
// Frames for every pending part that has none yet; -> what a take needs.  FA_ERR_CAPACITY leaves parts and frames as they are.
static int lz4_take_prepare(fa_ctx* c, Lz4State** zp, size_t cap, bool have_out, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts) {
    RawState* t = c->raw;
    Lz4State* z = nullptr;
    int rc = lz4_state(c, &z);
    if (rc) return rc;
    *zp = z;
    if (z->raw_takes != t->takes) z->frames_used = 0, z->starts.clear(), z->raw_takes = t->takes;  // (a plain take or a reset took the parts these frames were of)
    if (z->starts.size() < t->pending.size()) {
        std::vector<Lz4Src> in;
        for (size_t i = z->starts.size(); i < t->pending.size(); i++) in.push_back({t->img.get() + t->pending[i].offset, (size_t)t->pending[i].bytes});
        rc = lz4_compress(c, z, in, z->frames, &z->frames_used, z->starts);
        if (rc) return rc;
        raw_read_events(t);
    }
    *bytes_out = z->frames_used;
    *n_parts = t->pending.size();
    if (z->frames_used > cap || (z->frames_used && !have_out) || t->pending.size() > parts_cap || (!parts && !t->pending.empty()))
        return fail(c, FA_ERR_CAPACITY, "fa_raw_take_lz4: a buffer is too small (bytes and parts needed are returned); nothing was taken, the frames are kept");
    return FA_OK;
}
static void lz4_take_finish(RawState* t, Lz4State* z, fa_raw_part* parts) {
    for (size_t i = 0; i < t->pending.size(); i++) {
        parts[i] = t->pending[i];
        parts[i].offset = z->starts[i];
        parts[i].bytes = (i + 1 < z->starts.size() ? z->starts[i + 1] : z->frames_used) - z->starts[i];
    }
    raw_clear(t, nullptr);
    z->frames_used = 0, z->starts.clear(), z->raw_takes = t->takes;
}

extern "C" int fa_raw_take_lz4(fa_ctx* c, uint8_t* out, size_t cap, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts) {
    RAW_ENTER(c, "fa_raw_take_lz4");
    if (!bytes_out || !n_parts) return fail(c, FA_ERR_ARG, "fa_raw_take_lz4: null argument");
    Lz4State* z = nullptr;
    int rc = lz4_take_prepare(c, &z, cap, out != nullptr, bytes_out, parts, parts_cap, n_parts);
    if (rc) return rc;
    if (z->frames_used) HIPCHK(c, hipMemcpyAsync(out, z->frames, z->frames_used, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    raw_read_events(c->raw);
    lz4_take_finish(c->raw, z, parts);
    return FA_OK;
}

extern "C" int fa_raw_take_lz4_device(fa_ctx* c, const void** d_bytes, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts) {
    RAW_ENTER(c, "fa_raw_take_lz4_device");
    if (!d_bytes || !bytes_out || !n_parts) return fail(c, FA_ERR_ARG, "fa_raw_take_lz4_device: null argument");
    *d_bytes = nullptr;
    Lz4State* z = nullptr;
    int rc = lz4_take_prepare(c, &z, (size_t)-1, true, bytes_out, parts, parts_cap, n_parts);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    raw_read_events(c->raw);
    *d_bytes = z->frames_used ? z->frames.get() : nullptr;
    lz4_take_finish(c->raw, z, parts);
    return FA_OK;
}

extern "C" int fa_lz4_frame_device(fa_ctx* c, const void* d_in, size_t n, const void** d_out, size_t* bytes_out) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if ((!d_in && n) || !d_out || !bytes_out) return fail(c, FA_ERR_ARG, "fa_lz4_frame_device: null argument");
    *d_out = nullptr;
    *bytes_out = 0;
    Lz4State* z = nullptr;
    int rc = lz4_state(c, &z);
    if (rc) return rc;
    size_t used = 0;
    if (n == 0) {  // header and EndMark
        uint8_t f[LZ4_HEADER_BYTES + LZ4_ENDMARK_BYTES] = {};
        lz4_frame_header(f);
        rc = lz4_reserve(c, z->one, 0, sizeof f);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(z->one, f, sizeof f, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        used = sizeof f;
        z->n_frames++, z->bytes_out += used;
    } else {
        std::vector<uint64_t> starts;
        rc = lz4_compress(c, z, {{(const uint8_t*)d_in, n}}, z->one, &used, starts);
        if (rc) return rc;
    }
    *d_out = z->one.get();
    *bytes_out = used;
    return FA_OK;
}

extern "C" int fa_raw_lz4_stats(fa_ctx* c, fa_raw_lz4_stats_t* out) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (!out) return fail(c, FA_ERR_ARG, "fa_raw_lz4_stats: null argument");
    memset(out, 0, sizeof *out);
    const Lz4State* z = c->lz4;
    if (!z) return FA_OK;
    out->frames = z->n_frames, out->blocks = z->n_blocks, out->stored_blocks = z->n_stored;
    out->bytes_in = z->bytes_in, out->bytes_out = z->bytes_out;
    out->compress_launches = z->launches;
    out->device_ns = z->block_ns + z->pack_ns, out->block_ns = z->block_ns, out->pack_ns = z->pack_ns;
    return FA_OK;
}
