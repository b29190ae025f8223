// raw_merge_host.inc - host side of fa_raw_merge (included by flowagg.hip: one translation unit; device side: raw_merge.cuh).
// The pending parts of a ctx (RawState of raw_host.inc) are replaced by one part per Date, rows in stable t32 order over the
// parts laid end to end: bit for bit what ONE chunk holding all those records would have built.
//
// One merge: everything it needs is allocated first - the second image (as large as the pending bytes: a merged part is never
// larger than its sources, it has fewer headers and a row count's varuint is no longer than its terms' together), the scratch and
// the descriptors' staging; a failure there is FA_ERR_NOMEM with nothing changed.  Then the sources' descriptors are copied in,
// raw_merge_key_kernel reads the keys, the build's order step (raw_order_and_list of raw_host.inc: one radix sort, raw_parts_kernel,
// ONE synchronisation that brings the Date list) orders them, the host lays the merged parts out and launches one gather per Date (a Date with a single source part is that part:
// a device copy), and ONE synchronisation ends the call.  Only then the images change places and the pending list is replaced.
// Memory, kept until fa_raw_reset / fa_destroy: the image that is NOT in use (the old image is KEPT as the next merge's spare,
// not released), 16 bytes per pending row of keys and indices in and out, 16 bytes per source, the Date list and hipcub's storage.

struct RawMergeState {
    DevBuf<uint8_t> spare;     // the image the next merge writes: the one the last merge read
    DevBuf<> scratch;          // 2 x keys, 2 x indices (+ the word raw_parts_kernel reads as pos[n]), descriptors, the Date list, hipcub storage
    PinnedBuf<uint8_t> h_src;  // the descriptors on their way in
    Events ev;                 // 4: order start / done, gather start / done
    uint64_t merges = 0, parts_in = 0, parts_out = 0, rows = 0, bytes_in = 0, bytes_out = 0, launches = 0, order_ns = 0, gather_ns = 0;
};

// fa_raw_reset: the buffers go, the counters of fa_raw_merge_stats go on counting
static void raw_merge_release(fa_ctx* c) {
    RawMergeState* m = c->raw_merge;
    if (!m) return;
    m->spare.reset(), m->scratch.reset(), m->h_src.reset();
}

extern "C" int fa_raw_merge(fa_ctx* c) {
    RAW_ENTER(c, "fa_raw_merge");
    RawState* t = c->raw;
    const size_t nsrc = t->pending.size();
    // ---- nothing to do: no part, or one part per Date in ascending Date already
    bool merged = true;
    for (size_t i = 1; i < nsrc; i++) merged = merged && t->pending[i - 1].date < t->pending[i].date;
    if (merged) return FA_OK;
    uint64_t n64 = 0;
    for (const fa_raw_part& p : t->pending) n64 += p.rows;
    if (n64 > (uint64_t)INT32_MAX)
        return fail(c, FA_ERR_ARG, "fa_raw_merge: " + std::to_string(n64) + " pending rows are more than one sort takes (2^31 - 1); take the parts first");
    const uint32_t n = (uint32_t)n64;
    // what the merge will give is known from the descriptions: rows per Date, and which Dates have a single source
    struct DateSum {
        uint64_t rows = 0;
        size_t sources = 0, only = 0;
        uint32_t t_min = 0xFFFFFFFFu, t_max = 0;
    };
    std::map<uint32_t, DateSum> dates;
    for (size_t i = 0; i < nsrc; i++) {
        DateSum& d = dates[t->pending[i].date];
        d.rows += t->pending[i].rows, d.sources++, d.only = i;
        d.t_min = std::min(d.t_min, t->pending[i].t_min), d.t_max = std::max(d.t_max, t->pending[i].t_max);
    }
    size_t bytes_out = 0;
    for (const auto& d : dates) bytes_out += fa_raw_part_bytes(d.second.rows);
    if (bytes_out > t->used) return fail(c, FA_ERR_HIP, "internal: the merged parts are larger than their sources");

    // ---- everything the merge needs, before anything changes
    int rc = state_with_events(c, c->raw_merge, 4);
    if (rc) return rc;
    RawMergeState* m = c->raw_merge;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the last build's gather has written the image)
    raw_read_events(t);
    RawOrder o(c, n);
    const size_t src_bytes = align256(nsrc * sizeof(RawMergeSrc));
    if (m->spare.bytes() < t->used) {
        DevBuf<uint8_t> image;
        if (!image.grow(std::max(t->used, t->img.bytes()))) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "hipMalloc(merged raw part image) failed; the pending parts are unchanged");
        }
        m->spare = std::move(image);
    }
    rc = ensure_dev(c, m->scratch, src_bytes + o.bytes(), "raw merge scratch");
    if (rc) return rc;
    if (!m->h_src.grow(src_bytes, src_bytes + src_bytes / 2)) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "hipHostMalloc(raw merge descriptors) failed; the pending parts are unchanged");
    }
    RawMergeSrc* d_src = (RawMergeSrc*)m->scratch.get();  // the descriptors, in front of the order step's scratch
    o.carve((uint8_t*)m->scratch.get() + src_bytes);

    // ---- order
    RawMergeSrc* h_src = (RawMergeSrc*)m->h_src.get();
    uint32_t first = 0;
    for (size_t i = 0; i < nsrc; i++) {
        h_src[i] = RawMergeSrc{t->img.get() + t->pending[i].offset, (uint32_t)t->pending[i].rows, first};
        first += (uint32_t)t->pending[i].rows;
    }
    (void)hipEventRecord(m->ev[0], c->stream);
    HIPCHK(c, hipMemcpyAsync(d_src, h_src, nsrc * sizeof(RawMergeSrc), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(raw_merge_key_kernel, dim3((n + 1 + 255) / 256), dim3(256), 0, c->stream, (const RawMergeSrc*)d_src, (uint32_t)nsrc, n, o.key_in, o.idx_in);
    // (raw_parts_kernel reads pos[n] alone, the count of good rows: idx_in[n] holds n, every row of a part is good)
    RawPartsHeader h;
    std::vector<RawPartEntry> ent;
    uint64_t launches = 0;
    rc = raw_order_and_list(c, o, o.idx_in, m->ev[1], &launches, 3, &h, &ent);
    if (rc) return rc;
    if (h.good != n || h.nparts != dates.size()) return fail(c, FA_ERR_HIP, "internal: the merged Date list does not match the pending parts");
    // ---- the merged image's layout, then one gather (or one copy) per Date
    std::vector<fa_raw_part> out = raw_lay_out(h, ent, 0);
    size_t used = 0, i = 0;
    for (const auto& d : dates) {  // (ascending Date, as the sorted list is)
        const fa_raw_part& p = out[i++];
        if (p.date != d.first || p.rows != d.second.rows || p.t_min != d.second.t_min || p.t_max != d.second.t_max)
            return fail(c, FA_ERR_HIP, "internal: the merged Date list does not match the pending parts");
        used += p.bytes;
    }
    (void)hipEventRecord(m->ev[2], c->stream);
    for (i = 0; i < out.size(); i++) {
        const fa_raw_part& p = out[i];
        const DateSum& d = dates[p.date];
        if (d.sources == 1) {  // the Date's only part, sorted as it is
            HIPCHK(c, hipMemcpyAsync(m->spare.get() + p.offset, t->img.get() + t->pending[d.only].offset, p.bytes, hipMemcpyDeviceToDevice, c->stream));
            continue;
        }
        RawMergeArgs a{};
        a.part = m->spare.get() + p.offset;
        a.key = o.key + ent[i].start;
        a.idx = o.idx + ent[i].start;
        a.src = d_src;
        a.nsrc = (uint32_t)nsrc, a.rows = (uint32_t)p.rows, a.date = p.date;
        hipLaunchKernelGGL(raw_merge_gather_kernel, raw_part_grid(a.part, p.rows), dim3(RAW_BLOCK), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        launches++;
    }
    (void)hipEventRecord(m->ev[3], c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // ---- the gather has finished: the images change places (the old one is the next spare), the pending list is the merged one
    Events::elapsed_ns(m->ev[0], m->ev[1], &m->order_ns);
    Events::elapsed_ns(m->ev[2], m->ev[3], &m->gather_ns);
    m->merges++, m->parts_in += nsrc, m->parts_out += out.size(), m->rows += n, m->bytes_in += t->used, m->bytes_out += used, m->launches += launches;
    std::swap(t->img, m->spare);
    t->used = used;
    t->pending = std::move(out);
    t->takes++;  // frames kept from a refused fa_raw_take_lz4 were made of the old parts (lz4_host.inc)
    return FA_OK;
}

extern "C" int fa_raw_merge_stats(fa_ctx* c, fa_raw_merge_stats_t* out) {
    RAW_ENTER(c, "fa_raw_merge_stats");
    if (!out) return fail(c, FA_ERR_ARG, "fa_raw_merge_stats: null argument");
    *out = fa_raw_merge_stats_t{};
    if (const RawMergeState* m = c->raw_merge) {
        out->merges = m->merges, out->parts_in = m->parts_in, out->parts_out = m->parts_out;
        out->rows = m->rows, out->bytes_in = m->bytes_in, out->bytes_out = m->bytes_out;
        out->launches = m->launches, out->order_ns = m->order_ns, out->gather_ns = m->gather_ns;
    }
    return FA_OK;
}
