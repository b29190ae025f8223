// ports_host.inc - host side of the bucketed port tables (included by flowagg.hip: one translation unit; device side: ports.cuh).
// The ONE second pass an ingest call runs for every enabled fold is second_pass.inc.  The tables, their capacity rule, chunks,
// growth, retention and statistics are keytab_host.inc's under the traits PortTab; here are the ports' own doors, their fold
// launch and the ranged collector.
static_assert(PORT_LARGE == PORT_DENSE, "the ranged collector's dense scratch is indexed like the dense port histograms");
static_assert(sizeof(PortRow) == sizeof(RowW) && sizeof(RowW) == sizeof(fa_port_row), "row layout");

struct PortState : TabPair<PortTab> {
    DevBuf<ulonglong2> dense;  // the ranged collector's {weight, count} per port below 65536 (1 MiB)
    DevBuf<> rows;             // the ranged collector's rows on their way into the merge; fa_ports_buckets' scratch
    bool alloc_own() { return dense.grow(sizeof(ulonglong2) * PORT_DENSE); }
};

static uint32_t port_bucket_secs(const fa_ctx* c) { return c->ports ? c->ports->bucket_secs : 0; }

#define PORT_ENTER(c) TAB_ENTER(c, ports, PORT_OFF)

extern "C" int fa_ports_enable_buckets(fa_ctx* c, uint32_t capacity_log2, uint32_t bucket_secs) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (c->ports) return fail(c, FA_ERR_ARG, "fa_ports_enable_buckets: already enabled");
    if (bucket_secs == 0 || 86400u % bucket_secs) return fail(c, FA_ERR_ARG, "fa_ports_enable_buckets: bucket_secs must be >= 1 and divide 86400");
    return tab_enable<PortTab>(c, c->ports, "fa_ports_enable_buckets", capacity_log2, bucket_secs);
}

static size_t port_chunk_cap(const fa_ctx* c) { return tab_chunk_cap(*c->ports); }

struct PortCols {
    const void *src_port, *dst_port, *bytes, *sampling_rate, *time_flow_start, *status;
};

static int port_fold_cols(fa_ctx* c, const PortCols& p, size_t n) {
    PortState& t = *c->ports;
    return tab_chunks(c, t, 3, n, [&](size_t i, size_t m) -> int {
        PortFoldArgs a{};
        a.src_port = (const uint32_t*)p.src_port + i;
        a.dst_port = (const uint32_t*)p.dst_port + i;
        a.bytes = (const uint64_t*)p.bytes + i;
        a.sampling_rate = (const uint64_t*)p.sampling_rate + i;
        a.time_flow_start = (const uint64_t*)p.time_flow_start + i;
        a.status = (const uint8_t*)p.status + i;
        a.n = (uint32_t)m;
        a.bucket_secs = t.bucket_secs;
        for (int d = 0; d < 2; d++) {
            a.tab[d] = t.tab[d];
            a.mask[d] = t.mask(d);
        }
        a.ctr = t.d_ctr;
        return tab_fold_launch(c, t, m, [&](dim3 grid) { hipLaunchKernelGGL(port_fold_kernel, grid, dim3(PORT_BLOCK), 0, c->stream, a); });
    });
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
    int rc = tab_settle(c, *t, h);
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
    hipLaunchKernelGGL(port_range_fold_kernel, t->scan_grid(c, d), dim3(256), 0, c->stream, (const PSlot*)t->tab[d], t->slots(d), range.index_lo, range.index_last, t->dense.get(),
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

// (the merge of the port kinds, RowOps<RK_PORT_SRC>, leaves fa_top_ports' order: weight DESC, port)
extern "C" int fa_top_ports_range(fa_ctx* c, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_port_row* out, size_t cap, size_t* n_out) {
    PORT_ENTER(c);
    return tab_range_read(c, "fa_top_ports_range", c->ports->bucket_secs, dst ? RK_PORT_DST : RK_PORT_SRC, dst, t_lo, t_hi, k, out, cap, n_out);
}
extern "C" int fa_ports_range_rows_device(fa_ctx* c, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, const void** d_rows, size_t* n_out) {
    PORT_ENTER(c);
    return tab_range_rows_device(c, "fa_ports_range_rows_device", c->ports->bucket_secs, dst ? RK_PORT_DST : RK_PORT_SRC, dst, t_lo, t_hi, k, d_rows, n_out);
}

// ---- buckets held, retention, reset, statistics --------------------------------------------------------------------------------
extern "C" int fa_ports_buckets(fa_ctx* c, uint32_t* out, size_t cap, size_t* n_out) {
    PORT_ENTER(c);
    return tab_buckets(c, *c->ports, c->ports->rows, out, cap, n_out);
}
extern "C" int fa_ports_drop_before(fa_ctx* c, uint32_t t_floor) {
    PORT_ENTER(c);
    return tab_drop_before(c, *c->ports, t_floor);
}
extern "C" int fa_ports_reset(fa_ctx* c) {
    PORT_ENTER(c);
    return tab_reset(c, *c->ports);
}
extern "C" int fa_ports_stats(fa_ctx* c, fa_ports_stats_t* out) {
    PORT_ENTER(c);
    return tab_stats(c, *c->ports, out);
}
