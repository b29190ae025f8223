// decode_host.inc - decode + project: the 15 SoA columns (included by flowagg.hip: one translation unit, see kernels.cuh for the device side).

// ---- decode + project ---------------------------------------------------------------------
static int ensure_columns(fa_ctx* c, size_t n) {
    const size_t rec = 5 * 8 + 7 * 4 + 3 * 16 + 1;  // bytes of one record's columns
    if (c->col_block.bytes() >= n * rec) return FA_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cols = ColumnPtrs{};  // (they point into the block that goes)
    size_t cap = std::max<size_t>(n, 1 << 16);
    cap = (cap + 63) & ~(size_t)63;
    if (!c->col_block.grow(n * rec, cap * rec)) return fail(c, FA_ERR_NOMEM, "hipMalloc(columns) failed");
    uint8_t* p = (uint8_t*)c->col_block.get();
    auto take = [&](size_t elem) {
        uint8_t* r = p;
        p += cap * elem;
        return r;
    };
    c->cols.sampler_address = (uint4*)take(16);
    c->cols.src_addr = (uint4*)take(16);
    c->cols.dst_addr = (uint4*)take(16);
    c->cols.time_received = (uint64_t*)take(8);
    c->cols.time_flow_start = (uint64_t*)take(8);
    c->cols.sampling_rate = (uint64_t*)take(8);
    c->cols.bytes = (uint64_t*)take(8);
    c->cols.packets = (uint64_t*)take(8);
    c->cols.sequence_num = (uint32_t*)take(4);
    c->cols.src_as = (uint32_t*)take(4);
    c->cols.dst_as = (uint32_t*)take(4);
    c->cols.etype = (uint32_t*)take(4);
    c->cols.proto = (uint32_t*)take(4);
    c->cols.src_port = (uint32_t*)take(4);
    c->cols.dst_port = (uint32_t*)take(4);
    c->cols.status = (uint8_t*)take(1);
    return FA_OK;
}

// len = bytes of the whole buffer the offsets point into (the bound the kernel clamps to); bytes = wire bytes of THESE n
// records (exact or estimated: tile sizing only) - the sub-range convention of ingest_device_records.
static int decode_device_records(fa_ctx* c, const void* d_buf, size_t len, size_t bytes, const void* d_off, size_t n, fa_columns* out);
extern "C" int fa_decode_device(fa_ctx* c, const void* d_buf, size_t len, const void* d_off, size_t n,
                                fa_columns* out) {
    FA_ON_DEVICE(c);
    if (!c || !out) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    return decode_device_records(c, d_buf, len, len, d_off, n, out);
}
static int decode_device_records(fa_ctx* c, const void* d_buf, size_t len, size_t bytes, const void* d_off, size_t n, fa_columns* out) {
    if (!d_buf || !d_off || len >= (1ull << 32) || n > c->cfg.max_batch_records || ((uintptr_t)d_buf & 15))
        return fail(c, FA_ERR_ARG, "fa_decode_device: bad buffer");
    int rc = ensure_columns(c, std::max<size_t>(n, 1));
    if (rc) return rc;
    rc = ensure_exotic(c, std::max<size_t>(n, 1));
    if (rc) return rc;
    if (n) {
        KArgs a = make_args(c);
        a.buf = (const uint8_t*)d_buf;
        a.off = (const uint32_t*)d_off;
        a.n = (uint32_t)n;
        a.len = (uint32_t)len;
        LaunchPlan p;  // (the default: workgroup tiles, the flows_5m variant)
        p.tile_recs = a.tile_recs = tile_recs_for(bytes, n);
        p.grid = grid_for(c, tile_kernel<MODE_DECODE, 1u>, a.n, p.tile_recs);
        rc = acquire_events(c, c->dev_pool, 1024);
        if (rc) return rc;
        rc = launch_tiles<MODE_DECODE>(c, a, p, c->dev_pool.take(3));
        if (rc) return rc;
    }
    out->time_received = c->cols.time_received;
    out->time_flow_start = c->cols.time_flow_start;
    out->sampling_rate = c->cols.sampling_rate;
    out->bytes = c->cols.bytes;
    out->packets = c->cols.packets;
    out->sequence_num = c->cols.sequence_num;
    out->src_as = c->cols.src_as;
    out->dst_as = c->cols.dst_as;
    out->etype = c->cols.etype;
    out->proto = c->cols.proto;
    out->src_port = c->cols.src_port;
    out->dst_port = c->cols.dst_port;
    out->sampler_address = (const uint8_t*)c->cols.sampler_address;
    out->src_addr = (const uint8_t*)c->cols.src_addr;
    out->dst_addr = (const uint8_t*)c->cols.dst_addr;
    out->status = c->cols.status;
    return FA_OK;
}

extern "C" int fa_decode(fa_ctx* c, const uint8_t* buf, size_t len, const uint64_t* offsets, size_t n,
                         fa_flow_row* out) {
    FA_ON_DEVICE(c);
    if (!c || (!out && n)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!offsets) return fail(c, FA_ERR_ARG, "fa_decode: offsets required");
    size_t done = 0;
    while (done < n) {
        size_t j = std::min(n, done + (size_t)std::min<uint32_t>(c->cfg.max_batch_records, 1u << 22));
        while (j > done + 1 && offsets[j] - offsets[done] > (1ull << 30)) j = done + (j - done) / 2;
        size_t m = j - done;
        uint64_t base = offsets[done];
        std::vector<uint64_t> rel(m + 1);
        for (size_t k = 0; k <= m; k++) {
            if (offsets[done + k] < base || offsets[done + k] > len) return fail(c, FA_ERR_ARG, "bad offsets");
            rel[k] = offsets[done + k] - base;
        }
        const uint8_t* d_buf;
        const uint32_t* d_off;
        int slot = 0;
        int rc = stage_and_upload(c, buf + base, (size_t)rel[m], rel.data(), m, &d_buf, &d_off, &slot);
        if (rc) return rc;
        fa_columns cols;
        rc = fa_decode_device(c, d_buf, (size_t)rel[m], d_off, m, &cols);
        if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        // gather SoA -> AoS on the host
        std::vector<uint64_t> u64(m);
        std::vector<uint32_t> u32(m);
        std::vector<uint8_t> b16(m * 16), st(m);
        fa_flow_row* o = out + done;
        memset(o, 0, m * sizeof(fa_flow_row));
#define GET64(member, src)                                                                  \
    HIPCHK(c, hipMemcpy(u64.data(), src, m * 8, hipMemcpyDeviceToHost));                    \
    for (size_t k = 0; k < m; k++) o[k].member = u64[k];
#define GET32(member, src)                                                                  \
    HIPCHK(c, hipMemcpy(u32.data(), src, m * 4, hipMemcpyDeviceToHost));                    \
    for (size_t k = 0; k < m; k++) o[k].member = u32[k];
#define GET16(member, src)                                                                  \
    HIPCHK(c, hipMemcpy(b16.data(), src, m * 16, hipMemcpyDeviceToHost));                   \
    for (size_t k = 0; k < m; k++) memcpy(o[k].member, &b16[k * 16], 16);
        GET64(time_received, cols.time_received)
        GET64(time_flow_start, cols.time_flow_start)
        GET64(sampling_rate, cols.sampling_rate)
        GET64(bytes, cols.bytes)
        GET64(packets, cols.packets)
        GET32(sequence_num, cols.sequence_num)
        GET32(src_as, cols.src_as)
        GET32(dst_as, cols.dst_as)
        GET32(etype, cols.etype)
        GET32(proto, cols.proto)
        GET32(src_port, cols.src_port)
        GET32(dst_port, cols.dst_port)
        GET16(sampler_address, cols.sampler_address)
        GET16(src_addr, cols.src_addr)
        GET16(dst_addr, cols.dst_addr)
#undef GET64
#undef GET32
#undef GET16
        HIPCHK(c, hipMemcpy(st.data(), cols.status, m, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < m; k++) o[k].status = st[k];
        done = j;
    }
    return FA_OK;
}
