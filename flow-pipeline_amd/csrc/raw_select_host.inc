// raw_select_host.inc - selecting rows of flows_raw parts (included by flowagg.hip behind raw_range_host.inc: one translation unit;
// device side: raw_select.cuh; the contract: include/flowagg.h "selecting rows of flows_raw parts").
//
// One call: range_run(load = true) of raw_range_host.inc - the host's walk, ONE copy of the input, stages A, B and C with their
// three waits and every validation; the select adds no decoding -, then over the slices it left:
//   select  ONE small plan copy (the slices, and the same parts as the gather's sources), raw_select_kernel over one flattened
//           grid, hipcub's exclusive scan of the workgroup counts, raw_select_totals_kernel, the per-slice totals back, ONE wait:
//           the output's layout depends on them (raw_lay_out / raw_part_grid of raw_host.inc);
//   emit    ONE small copy (where each part's output starts, the rows it delivers under the limit), raw_select_emit_kernel:
//           idx / key of the delivered rows, t_min / t_max of every output part;
//   gather  raw_merge_gather_kernel as it is, one launch per output part; the spans back, ONE wait.
// The selection lies in SelectState::sel until the ctx's next select, decode, load, restore or range call (load_state of
// raw_load_host.inc drops it: every such door goes through it), fa_raw_load_reset, fa_raw_reset or fa_destroy.

struct SelectState {
    DevBuf<uint8_t> sel;   // the selection: the output parts back to back
    size_t sel_bytes = 0;  // bytes of sel that hold a selection (0: none)
    DevBuf<> work;         // slices, sources | masks, counts, bases | totals, spans | outs | hipcub's storage
    DevBuf<> order;        // idx, key of the delivered rows
    PinnedBuf<> h_work;    // slices, sources, outs on their way in; totals, spans on their way back
    Events ev;             // 6: pairs around the select kernel with the scan, the emit kernel, the gathers
    fa_raw_select_stats_t st{};
};

// the next select, decode, load, restore or range call: the selection is gone (its memory is kept)
static void select_drop(fa_ctx* c) {
    if (c->select) c->select->sel_bytes = 0;
}
// fa_raw_load_reset, fa_raw_reset: the buffers go, the counters of fa_raw_select_stats go on counting
static void select_release(fa_ctx* c) {
    SelectState* q = c->select;
    if (!q) return;
    q->sel_bytes = 0;
    q->sel.reset(), q->work.reset(), q->order.reset(), q->h_work.reset();
}

// The slices a range run left - the parts that hold a row of the time range, in input order - and what the select and the
// query door (raw_query_host.inc) both plan over them.
struct SelectSlices {
    std::vector<const RangePart*> sl;
    uint64_t scanned = 0, src_rows = 0, ntiles = 0;  // rows of the slices, rows of their parts, workgroups of the flattened grid
    explicit SelectSlices(const RangeRun& run) {
        for (const RangePart& p : run.parts)
            if (p.r_lo < p.r_hi) sl.push_back(&p), scanned += p.r_hi - p.r_lo, src_rows += p.rows, ntiles += raw_select_tiles(p.r_hi - p.r_lo);
    }
    // the plan entries: tile0 running; first running (the gather numbers the source rows) or 0
    void plan(RawSelectPart* h_parts, bool number_rows) const {
        uint32_t tile0 = 0, first = 0;
        for (size_t j = 0; j < sl.size(); j++) {
            const RangePart& p = *sl[j];
            h_parts[j] = RawSelectPart{p.plan.off, (uint32_t)p.rows, (uint32_t)p.r_lo, (uint32_t)p.r_hi, tile0, number_rows ? first : 0u, 0};
            tile0 += (uint32_t)raw_select_tiles(p.r_hi - p.r_lo), first += (uint32_t)p.rows;
        }
    }
};

// The select, emit and gather steps over the slices of a run, whatever door the run came from (fa_raw_select: a ranged load's;
// fa_raw_select_pending of raw_pending_host.inc: the ctx's pending parts): every byte the kernels read is in run.image and is a
// flows_raw part's.  parts has room for one description per part of the run.
static int select_over(fa_ctx* c, SelectState* q, const char* fn, const RangeRun& run, const fa_raw_filter& f, fa_raw_part* parts, size_t* n_parts, size_t* bytes_out) {
    int rc = FA_OK;
    const SelectSlices slices(run);
    const std::vector<const RangePart*>& sl = slices.sl;
    const uint64_t scanned = slices.scanned, src_rows = slices.src_rows;
    const size_t ns = sl.size();
    const bool count_only = f.fields & FA_RAW_F_COUNT_ONLY;
    fa_raw_select_stats_t& st = q->st;
    if (!ns) {
        st.calls++;
        return FA_OK;
    }
    if (src_rows > (uint64_t)INT32_MAX)
        return fail(c, FA_ERR_ARG, std::string(fn) + ": " + std::to_string(src_rows) + " rows in the parts that hold a row of the time range are more than one gather indexes (2^31 - 1); select the file in pieces");
    const uint32_t ntiles = (uint32_t)slices.ntiles;

    // ---- buffers: the device's work area and its pinned mirror share one layout
    const size_t o_parts = 0, o_src = o_parts + align256(ns * sizeof(RawSelectPart)), o_out = o_src + align256(ns * sizeof(RawMergeSrc));
    const size_t o_tot = o_out + align256(ns * sizeof(RawSelectOut)), o_span = o_tot + align256(ns * sizeof(uint32_t)), o_small = o_span + align256(ns * sizeof(RawSelectSpan));
    const size_t o_mask = o_small, o_count = o_mask + align256((size_t)ntiles * RAW_SEL_WAVES * sizeof(uint64_t)), o_base = o_count + align256(((size_t)ntiles + 1) * 4);
    const size_t o_tmp = o_base + align256(((size_t)ntiles + 1) * 4), tmp_bytes = align256(scan_tmp_bytes(c, (size_t)ntiles + 1));
    rc = ensure_dev(c, q->work, o_tmp + tmp_bytes, "select work area");
    if (rc) return rc;
    if (!q->h_work.grow(o_small, o_small + o_small / 2)) {
        (void)hipGetLastError();
        return fail(c, FA_ERR_NOMEM, "hipHostMalloc(select plan) failed; nothing was selected");
    }
    uint8_t *wb = (uint8_t*)q->work.get(), *hb = (uint8_t*)q->h_work.get();
    RawSelectPart* h_parts = (RawSelectPart*)(hb + o_parts);
    RawMergeSrc* h_src = (RawMergeSrc*)(hb + o_src);
    RawSelectOut* h_out = (RawSelectOut*)(hb + o_out);
    const uint32_t* h_tot = (const uint32_t*)(hb + o_tot);
    const RawSelectSpan* h_span = (const RawSelectSpan*)(hb + o_span);
    const RawSelectPart* d_parts = (const RawSelectPart*)(wb + o_parts);
    uint64_t* d_mask = (uint64_t*)(wb + o_mask);
    uint32_t *d_count = (uint32_t*)(wb + o_count), *d_base = (uint32_t*)(wb + o_base);
    slices.plan(h_parts, true);
    for (size_t j = 0; j < ns; j++) h_src[j] = RawMergeSrc{run.image + h_parts[j].off, h_parts[j].rows, h_parts[j].first};

    // ---- select: the masks, the scanned bases, the totals
    HIPCHK(c, hipMemcpyAsync(wb + o_parts, hb + o_parts, o_out - o_parts, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_count + ntiles, 0, 4, c->stream));
    (void)hipEventRecord(q->ev[0], c->stream);
    hipLaunchKernelGGL(raw_select_kernel, dim3(ntiles), dim3(RAW_SEL_BLOCK), 0, c->stream, d_parts, (uint32_t)ns, run.image, f, d_mask, d_count);
    size_t tb = tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(wb + o_tmp, tb, (const uint32_t*)d_count, d_base, (int)(ntiles + 1), c->stream) != hipSuccess) return fail(c, FA_ERR_HIP, "scan failed");
    hipLaunchKernelGGL(raw_select_totals_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, d_parts, (uint32_t)ns, ntiles, (const uint32_t*)d_base, (uint32_t*)(wb + o_tot));
    (void)hipEventRecord(q->ev[1], c->stream);
    HIPCHK(c, hipGetLastError());
    st.launches += 3;
    HIPCHK(c, hipMemcpyAsync(hb + o_tot, wb + o_tot, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    Events::elapsed_ns(q->ev[0], q->ev[1], &st.select_ns);

    // ---- the output's layout: the rows every part delivers under the limit, in input order
    uint64_t matched = 0, left = f.limit ? f.limit : ~(uint64_t)0, total = 0;
    RawPartsHeader h{};
    std::vector<RawPartEntry> ent;
    std::vector<size_t> from;  // the slice an output part comes from
    for (size_t j = 0; j < ns; j++) {
        if (h_tot[j] > sl[j]->r_hi - sl[j]->r_lo) return fail(c, FA_ERR_HIP, "internal: a slice's match count is inconsistent");
        matched += h_tot[j];
        const uint32_t take = (uint32_t)std::min<uint64_t>(h_tot[j], left);
        h_out[j] = RawSelectOut{(uint32_t)total, take};
        if (!take) continue;
        ent.push_back(RawPartEntry{(uint32_t)total, sl[j]->date * 86400u, 0, 0});  // (the Date; the keys come back behind the emit)
        from.push_back(j);
        total += take, left -= take;
    }
    h.good = (uint32_t)total, h.nparts = (uint32_t)ent.size();
    std::vector<fa_raw_part> out = raw_lay_out(h, ent, 0);
    const size_t sel_bytes = out.empty() ? 0 : out.back().offset + out.back().bytes;
    if (total) {
        if (!count_only) {
            rc = ensure_dev(c, q->order, 2 * align256(total * 4), "select order");
            if (rc) return rc;
            if (!q->sel.grow(sel_bytes, sel_bytes + sel_bytes / 8 + 4096)) {
                (void)hipGetLastError();
                return fail(c, FA_ERR_NOMEM, "hipMalloc(selection) failed; nothing was selected (select a shorter range, or set a limit)");
            }
        }
        uint32_t* d_idx = count_only ? nullptr : (uint32_t*)q->order.get();
        uint32_t* d_key = count_only ? nullptr : (uint32_t*)((uint8_t*)q->order.get() + align256(total * 4));
        // ---- emit
        HIPCHK(c, hipMemcpyAsync(wb + o_out, hb + o_out, ns * sizeof(RawSelectOut), hipMemcpyHostToDevice, c->stream));
        (void)hipEventRecord(q->ev[2], c->stream);
        hipLaunchKernelGGL(raw_select_emit_kernel, dim3(ntiles), dim3(RAW_SEL_BLOCK), 0, c->stream, d_parts, (uint32_t)ns, run.image, (const uint64_t*)d_mask, (const uint32_t*)d_base,
                           (const RawSelectOut*)(wb + o_out), d_idx, d_key, (RawSelectSpan*)(wb + o_span));
        (void)hipEventRecord(q->ev[3], c->stream);
        HIPCHK(c, hipGetLastError());
        st.launches++;
        // ---- gather: one launch per output part
        (void)hipEventRecord(q->ev[4], c->stream);
        for (size_t i = 0; i < out.size() && !count_only; i++) {
            RawMergeArgs a{};
            a.part = q->sel.get() + out[i].offset;
            a.key = d_key + ent[i].start, a.idx = d_idx + ent[i].start;
            a.src = (const RawMergeSrc*)(wb + o_src);
            a.nsrc = (uint32_t)ns, a.rows = (uint32_t)out[i].rows, a.date = out[i].date;
            hipLaunchKernelGGL(raw_merge_gather_kernel, raw_part_grid(a.part, out[i].rows), dim3(RAW_BLOCK), 0, c->stream, a);
            HIPCHK(c, hipGetLastError());
            st.launches++;
        }
        (void)hipEventRecord(q->ev[5], c->stream);
        HIPCHK(c, hipMemcpyAsync(hb + o_span, wb + o_span, ns * sizeof(RawSelectSpan), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        Events::elapsed_ns(q->ev[2], q->ev[3], &st.emit_ns);
        if (!count_only) Events::elapsed_ns(q->ev[4], q->ev[5], &st.gather_ns);
        for (size_t i = 0; i < out.size(); i++) {
            out[i].t_min = h_span[from[i]].t_min, out[i].t_max = h_span[from[i]].t_max;
            if (out[i].t_min > out[i].t_max || out[i].t_min / 86400u != out[i].date) return fail(c, FA_ERR_HIP, "internal: an output part's keys are inconsistent");
        }
    }
    // ---- the call is done
    if (!out.empty()) memcpy(parts, out.data(), out.size() * sizeof(fa_raw_part));
    *n_parts = out.size(), *bytes_out = sel_bytes;
    if (!count_only) q->sel_bytes = sel_bytes;
    st.calls++, st.rows_scanned += scanned, st.rows_matched += matched, st.rows_out += total, st.parts_out += out.size(), st.bytes_out += sel_bytes;
    return FA_OK;
}

extern "C" int fa_raw_select(fa_ctx* c, const uint8_t* bytes, size_t n, const fa_raw_filter* filter, fa_raw_part* parts, size_t parts_cap, size_t* n_parts, size_t* bytes_out) {
    LOAD_ENTER(c);
    if (!filter || !n_parts || !bytes_out || (!parts && parts_cap) || (!bytes && n)) return fail(c, FA_ERR_ARG, "fa_raw_select: null argument");
    *n_parts = 0, *bytes_out = 0;
    LoadState* s = nullptr;
    int rc = load_state(c, &s);  // (the previous selection is dropped here)
    if (rc) return rc;
    const fa_raw_filter f = *filter;
    if (const char* why = raw_select_filter_why(f)) {
        c->err = std::string("fa_raw_select: ") + why;
        return FA_ERR_ARG;
    }
    RangeState* g = nullptr;
    rc = range_state(c, &g);
    if (rc) return rc;
    rc = state_with_events(c, c->select, 6);
    if (rc) return rc;
    RangeRun run;
    size_t np_in = 0;
    rc = range_run(c, s, g, "fa_raw_select", bytes, n, f.t_lo, f.t_hi, true, parts_cap, &np_in, run);
    if (rc == FA_ERR_CAPACITY) *n_parts = np_in;
    if (rc) return rc;
    // (from here on every byte the select, emit and gather kernels read is decoded and validated)
    return select_over(c, c->select, "fa_raw_select", run, f, parts, n_parts, bytes_out);
}

extern "C" int fa_raw_selection_device(fa_ctx* c, const void** d_bytes, size_t* bytes_out) {
    LOAD_ENTER(c);
    if (!d_bytes || !bytes_out) return fail(c, FA_ERR_ARG, "fa_raw_selection_device: null argument");
    const SelectState* q = c->select;
    *bytes_out = q ? q->sel_bytes : 0;
    *d_bytes = *bytes_out ? q->sel.get() : nullptr;
    return FA_OK;
}

extern "C" int fa_raw_selection_fetch(fa_ctx* c, uint8_t* out, size_t cap, size_t* bytes_out) {
    LOAD_ENTER(c);
    if (!bytes_out) return fail(c, FA_ERR_ARG, "fa_raw_selection_fetch: null argument");
    const SelectState* q = c->select;
    const size_t nb = q ? q->sel_bytes : 0;
    *bytes_out = nb;
    if (nb > cap || (nb && !out)) return fail(c, FA_ERR_CAPACITY, "fa_raw_selection_fetch: the buffer is too small (the bytes needed are returned); the selection stays");
    if (nb) HIPCHK(c, hipMemcpyAsync(out, q->sel.get(), nb, hipMemcpyDeviceToHost, c->stream));  // (page-locked `out`: one copy-engine transfer)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FA_OK;
}

extern "C" int fa_raw_select_stats(fa_ctx* c, fa_raw_select_stats_t* out) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (!out) return fail(c, FA_ERR_ARG, "fa_raw_select_stats: null argument");
    memset(out, 0, sizeof *out);
    if (c->select) *out = c->select->st;
    return FA_OK;
}
