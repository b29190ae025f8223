// raw_range_host.inc - ranged loads of flows_raw parts (included by flowagg.hip behind sketch_fold_host.inc: one translation unit;
// device side: raw_range.cuh; the block sets: raw_range_plan.h; the contract: include/flowagg.h "ranged loads of flows_raw parts").
//
// One call (range_run): the host walks the input as every load door does (load_walk), ONE copy brings it to HBM, and then three
// stages run, each ONE small plan copy, its launches, its verdicts' copies back and ONE wait:
//   A probe  lz4_decode_kernel over the first and last block of every frame, raw_probe_kernel -> rows, Date[0]; the selection;
//   B range  lz4_decode_kernel over the header and TimeReceived blocks of the selected parts, raw_header_check_kernel (the part's
//            size is known by now and travels in RawPartPlan::bytes: no status word of an undecoded block is ever read),
//            raw_range_kernel -> [r_lo, r_hi), the order and Date verdicts;
//   C load   lz4_decode_kernel over the blocks rows [r_lo, r_hi) of columns 2 .. 15 lie in; then restore_fold_slices.
// The decode plans of the three stages stand one behind the other in ONE plan array (a block is planned at most once per call, so
// nb entries suffice) and so do their status words: plan entry k belongs to block order[k].  Plain Native input has no blocks:
// stage A reads the host's bytes, stage B runs its two kernels on the input's copy, stage C is the slice alone.
// Everything is validated before the first unpack or fold launch: a refused call folds nothing.  The buffers are LoadState's
// (raw_load_host.inc): the input's copy, a 64 KiB slot per block - decoded or not; slots of blocks this call does not decode
// keep what an earlier call left and are never read (DESIGN 3.9) -, the plans, one chunk of columns.

struct RangeState {
    Events ev;  // 8: pairs around stage A's kernels, stage B's decode, raw_range_kernel, stage C's decode
    fa_raw_range_stats_t st{};
};

static int range_state(fa_ctx* c, RangeState** out) {
    const int rc = state_with_events(c, c->range, 8);
    *out = c->range;
    return rc;
}

struct RangePart {
    RawPartPlan plan;  // off, bytes (known behind stage A), first_block, nblocks (0xFFFFFFFF: plain input)
    uint64_t rows = 0, r_lo = 0, r_hi = 0;
    uint32_t date = 0, t_min = 0, t_max = 0;
    bool selected = false;
};
struct RangeRun {
    std::vector<RangePart> parts;
    const uint8_t* image = nullptr;
};

// Stages A and B, and with `load` the decode of stage C: afterwards run.parts holds every part's rows and [r_lo, r_hi), and every
// byte the slices' unpack will read is decoded and validated.  parts_cap: more parts than this is FA_ERR_CAPACITY, found by the
// host's walk before anything is copied; *n_parts = the parts there are.
static int range_run(fa_ctx* c, LoadState* s, RangeState* g, const char* fn, const uint8_t* in, size_t n, uint32_t t_lo, uint32_t t_hi, bool load, size_t parts_cap,
                     size_t* n_parts, RangeRun& run) {
    auto framing = [&](const std::string& why) {
        c->err = std::string(fn) + ": " + why;
        return FA_ERR_FRAMING;
    };
    LoadPrepared pr;
    std::vector<RawPartPlan> pplan;
    bool lz4 = false;
    int rc = load_walk(c, fn, in, n, true, pr, pplan, &lz4);
    if (rc) return rc;
    const size_t nb = pr.walk.blocks.size(), np = pplan.size();
    if (n_parts) *n_parts = np;
    if (np > parts_cap) return fail(c, FA_ERR_CAPACITY, "the range buffer is too small (the parts there are is returned); nothing was copied or decoded");
    if (np > ((size_t)1 << 30)) return fail(c, FA_ERR_ARG, "more than 2^30 parts in one call");
    // a frame without blocks decodes to 0 bytes, which is no part: refused here, before anything is copied, planned or launched (its
    // slot would begin where the image ends)
    if (lz4)
        for (size_t i = 0; i < np; i++)
            if (pplan[i].nblocks == 0) return framing("frame " + std::to_string(i) + ": 0 bytes fit no row count of a flows_raw part (a truncated part or trailing bytes)");
    run.parts.resize(np);
    for (size_t i = 0; i < np; i++) run.parts[i].plan = pplan[i];
    uint64_t launches = 0, blocks_decoded = 0, stored = 0, bytes_decoded = 0;
    auto commit_launches = [&] { s->launches += launches, g->st.launches += launches, launches = 0; };
    auto add_ns = [&](uint64_t* a, uint64_t* b, hipEvent_t e0, hipEvent_t e1) {
        uint64_t ns = 0;
        Events::elapsed_ns(e0, e1, &ns);
        *a += ns;
        if (b) *b += ns;
    };
    if (n) {
        // ---- buffers: the device's plan area and its pinned mirror share one layout
        const size_t o_plan = 0, o_st = o_plan + align256(nb * sizeof(Lz4DBlock)), o_poff = o_st + align256(nb * sizeof(Lz4DecStatus));
        const size_t o_pout = o_poff + align256(np * sizeof(uint64_t)), o_b = o_pout + align256(np * RAW_PROBE_BYTES);
        const size_t total = o_b + align256(np * sizeof(RawPartPlan)) + align256(np * sizeof(RawRangePart)) + align256(np * sizeof(RawRangeRec)) + align256(np * sizeof(RawPartVerdict)) + 256;
        rc = ensure_dev(c, s->meta, total, "range plan");
        if (rc) return rc;
        const bool ok = s->h_meta.grow(total) && s->in.grow(n + 16) && s->img.grow(std::max<size_t>(nb, 1) * LZ4_BLOCK_MAX);
        if (!ok) {
            (void)hipGetLastError();
            return fail(c, FA_ERR_NOMEM, "hipMalloc(load: input copy / decoded image) failed; nothing was loaded (load the file in pieces cut at frame boundaries)");
        }
        uint8_t *mb = (uint8_t*)s->meta.get(), *hb = (uint8_t*)s->h_meta.get();
        Lz4DBlock* const h_plan = (Lz4DBlock*)(hb + o_plan);
        const Lz4DecStatus* const h_st = (const Lz4DecStatus*)(hb + o_st);
        const uint8_t* const image = lz4 ? s->img.get() : s->in.get();
        run.image = image;
        std::vector<uint8_t> done(nb, 0);
        std::vector<uint32_t> order;  // plan entry k decodes block order[k]
        order.reserve(nb);
        // plan entries [k0, order.size()) -> the device, one decode launch between the events e, e + 1, their status words back
        auto decode = [&](size_t k0, size_t e) -> int {
            const size_t k1 = order.size();
            (void)hipEventRecord(g->ev[e], c->stream);
            if (k1 > k0) {
                for (size_t k = k0; k < k1; k++) {
                    const Lz4WalkBlock& w = pr.walk.blocks[order[k]];
                    h_plan[k] = Lz4DBlock{w.at, (uint64_t)order[k] * LZ4_BLOCK_MAX, w.n, w.stored ? (uint32_t)LZ4D_F_STORED : 0u};
                    stored += w.stored;
                }
                HIPCHK(c, hipMemcpyAsync(mb + o_plan + k0 * sizeof(Lz4DBlock), h_plan + k0, (k1 - k0) * sizeof(Lz4DBlock), hipMemcpyHostToDevice, c->stream));
                hipLaunchKernelGGL(lz4_decode_kernel, dim3((unsigned)((k1 - k0 + LZ4D_WAVES - 1) / LZ4D_WAVES)), dim3(64 * LZ4D_WAVES), 0, c->stream,
                                   (const Lz4DBlock*)(mb + o_plan) + k0, (uint32_t)(k1 - k0), (const uint8_t*)s->in.get(), s->img.get(), (Lz4DecStatus*)(mb + o_st) + k0);
                HIPCHK(c, hipGetLastError());
                launches++;
                HIPCHK(c, hipMemcpyAsync(hb + o_st + k0 * sizeof(Lz4DecStatus), mb + o_st + k0 * sizeof(Lz4DecStatus), (k1 - k0) * sizeof(Lz4DecStatus), hipMemcpyDeviceToHost, c->stream));
                blocks_decoded += k1 - k0;
            }
            (void)hipEventRecord(g->ev[e + 1], c->stream);
            return FA_OK;
        };
        // the verdict on plan entry k (behind the stage's wait)
        auto block_ok = [&](size_t k, std::string* why) {
            const uint32_t b = order[k];
            const Lz4WalkBlock& w = pr.walk.blocks[b];
            if (h_st[k].code) return *why = lz4_at_byte(std::string("LZ4 block: ") + lz4d_reason(h_st[k].code), w.at + h_st[k].at), false;
            if (b + 1 < pr.walk.first[w.frame + 1] && h_st[k].size != LZ4_BLOCK_MAX)
                return *why = lz4_at_byte("LZ4 frame: a block of " + std::to_string(h_st[k].size) + " decoded bytes that is not the last of its frame (every block but the last holds 65536)", w.at), false;
            bytes_decoded += h_st[k].size;
            return true;
        };
        auto where = [&](size_t i) { return lz4 ? "frame " + std::to_string(i) : "the part at byte " + std::to_string(pplan[i].off); };
        std::string why;

        HIPCHK(c, hipMemcpyAsync(s->in, in, n, hipMemcpyHostToDevice, c->stream));
        // ---- A. probe
        std::vector<size_t> k_first(np, 0), k_last(np, 0);
        uint8_t head[RAW_PROBE_BYTES];
        if (lz4) {
            uint64_t* h_poff = (uint64_t*)(hb + o_poff);
            for (size_t i = 0; i < np; i++) {
                const RawPartPlan& p = pplan[i];
                k_first[i] = order.size();
                raw_range_probe_blocks(p.first_block, p.nblocks, done, order);
                k_last[i] = order.size() - 1;  // (nblocks >= 1, checked above; a frame of one block: both are its entry)
                h_poff[i] = p.off;
            }
            HIPCHK(c, hipMemcpyAsync(mb + o_poff, h_poff, np * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
            rc = decode(0, 0);
            if (rc) return rc;
            hipLaunchKernelGGL(raw_probe_kernel, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, c->stream, (const uint64_t*)(mb + o_poff), (uint32_t)np, image, (uint4*)(mb + o_pout));
            (void)hipEventRecord(g->ev[1], c->stream);
            HIPCHK(c, hipGetLastError());
            launches++;
            HIPCHK(c, hipMemcpyAsync(hb + o_pout, mb + o_pout, np * RAW_PROBE_BYTES, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (plain input: the input's copy alone)
        commit_launches();
        if (lz4) add_ns(&g->st.probe_ns, nullptr, g->ev[0], g->ev[1]);
        for (size_t i = 0; i < np; i++) {
            RangePart& p = run.parts[i];
            const uint8_t* first = lz4 ? hb + o_pout + RAW_PROBE_BYTES * i : head;
            if (lz4) {
                if (!block_ok(k_first[i], &why)) return framing(why);
                if (k_last[i] != k_first[i] && !block_ok(k_last[i], &why)) return framing(why);
                p.plan.bytes = (uint64_t)(p.plan.nblocks - 1) * LZ4_BLOCK_MAX + h_st[k_last[i]].size;
            } else {
                memcpy(head, in + p.plan.off, RAW_PROBE_BYTES);  // (a part holds at least its 285 header bytes: load_walk)
            }
            if (!raw_rows_from_bytes(RAW_COLS_H, p.plan.bytes, &p.rows))
                return framing(where(i) + ": " + std::to_string(p.plan.bytes) + " bytes fit no row count of a flows_raw part (a truncated part or trailing bytes)");
            if (first[0] != RAW_NCOLS) return framing(where(i) + ": a flows_raw block has 16 columns, not this column count");
            uint8_t vu[10];
            const uint32_t vl = raw_put_varuint(vu, p.rows);
            for (uint32_t j = 0; j < vl; j++)
                if (first[1 + j] != vu[j])
                    return framing(where(i) + ": the row count at byte " + std::to_string(1 + j) + " is not the one the part's size gives (a size that fits no row count, or trailing bytes)");
            if (p.rows > ((uint64_t)1 << 31)) return fail(c, FA_ERR_ARG, "a part of more than 2^31 rows");
            if (p.rows) {
                const uint32_t at = raw_range_date_at(RAW_COLS_H, p.rows);  // (at + 2 <= RAW_PROBE_BYTES: rows <= 2^31)
                p.date = (uint32_t)first[at] | ((uint32_t)first[at + 1] << 8);
                p.selected = raw_range_date_meets(p.date, t_lo, t_hi);
            }
        }
        // ---- B. range
        std::vector<uint32_t> sel;
        for (size_t i = 0; i < np; i++)
            if (run.parts[i].selected) sel.push_back((uint32_t)i);
        const size_t ns = sel.size();
        std::vector<size_t> kb(ns + 1, order.size());
        if (ns) {
            const size_t b_pplan = o_b, b_rparts = b_pplan + align256(ns * sizeof(RawPartPlan)), b_recs = b_rparts + align256(ns * sizeof(RawRangePart));
            const size_t b_ver = b_recs + align256(ns * sizeof(RawRangeRec)), b_end = b_ver + align256(ns * sizeof(RawPartVerdict));
            RawPartPlan* h_pp = (RawPartPlan*)(hb + b_pplan);
            RawRangePart* h_rp = (RawRangePart*)(hb + b_rparts);
            RawRangeRec* h_rec = (RawRangeRec*)(hb + b_recs);
            const RawPartVerdict* h_ver = (const RawPartVerdict*)(hb + b_ver);
            uint64_t tiles = 0;
            const size_t k0 = order.size();
            for (size_t j = 0; j < ns; j++) {
                const RangePart& p = run.parts[sel[j]];
                kb[j] = order.size();
                if (lz4) raw_range_scan_blocks(RAW_COLS_H, p.rows, p.plan.first_block, p.plan.nblocks, done, order);
                h_pp[j] = RawPartPlan{p.plan.off, p.plan.bytes, 0, 0xFFFFFFFFu};  // (the size is known: no block status is read)
                h_rp[j] = RawRangePart{p.plan.off, p.plan.bytes, (uint32_t)p.rows, p.date, (uint32_t)tiles, 0};
                h_rec[j] = raw_range_rec_init();
                tiles += raw_range_tiles(p.rows);
            }
            kb[ns] = order.size();
            if (tiles > 0x7FFFFFFFu) return fail(c, FA_ERR_ARG, "more than 2^43 rows in the selected parts of one call");
            HIPCHK(c, hipMemcpyAsync(mb + b_pplan, hb + b_pplan, b_ver - b_pplan, hipMemcpyHostToDevice, c->stream));
            rc = decode(k0, 2);
            if (rc) return rc;
            hipLaunchKernelGGL(raw_header_check_kernel, dim3((unsigned)ns), dim3(64), 0, c->stream, (const RawPartPlan*)(mb + b_pplan), (const uint32_t*)(mb + o_st), image,
                               (RawPartVerdict*)(mb + b_ver));
            (void)hipEventRecord(g->ev[4], c->stream);
            hipLaunchKernelGGL(raw_range_kernel, dim3((unsigned)tiles), dim3(RAW_RANGE_BLOCK), 0, c->stream, (const RawRangePart*)(mb + b_rparts), (uint32_t)ns, image, t_lo, t_hi,
                               (RawRangeRec*)(mb + b_recs));
            (void)hipEventRecord(g->ev[5], c->stream);
            HIPCHK(c, hipGetLastError());
            launches += 2;
            HIPCHK(c, hipMemcpyAsync(hb + b_recs, mb + b_recs, b_end - b_recs, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            commit_launches();
            add_ns(&g->st.decode_ns, &s->decode_ns, g->ev[2], g->ev[3]);
            add_ns(&g->st.range_ns, nullptr, g->ev[4], g->ev[5]);
            for (size_t j = 0; j < ns; j++) {  // (input order)
                RangePart& p = run.parts[sel[j]];
                for (size_t k = kb[j]; k < kb[j + 1]; k++)
                    if (!block_ok(k, &why)) return framing(why);
                if (h_ver[j].code) {
                    const std::string v = load_verdict_why(h_ver[j]);
                    if (v.empty()) return fail(c, FA_ERR_HIP, "internal: a part's verdict is inconsistent");
                    return framing(where(sel[j]) + ": " + v);
                }
                const RawRangeRec& r = h_rec[j];
                if (r.descends_at != RAW_RANGE_NONE && r.descends_at <= r.off_date_at)
                    return framing(where(sel[j]) + " (part " + std::to_string(sel[j]) + "): TimeReceived descends behind row " + std::to_string(r.descends_at) +
                                   ": a flows_raw part is sorted by it, and the range rests on that order");
                if (r.off_date_at != RAW_RANGE_NONE)
                    return framing(where(sel[j]) + " (part " + std::to_string(sel[j]) + "): the TimeReceived of row " + std::to_string(r.off_date_at) + " does not lie in the part's Date " +
                                   std::to_string(p.date) + ": a flows_raw part holds one Date");
                if (r.r_lo > r.r_hi || r.r_hi > p.rows) return fail(c, FA_ERR_HIP, "internal: a part's row range is inconsistent");
                p.r_lo = r.r_lo, p.r_hi = r.r_hi;
                if (p.r_lo < p.r_hi) p.t_min = r.t_min, p.t_max = r.t_max;
            }
        }
        // ---- C. load: the blocks of the slices
        if (load && lz4) {
            const size_t k0 = order.size();
            for (const RangePart& p : run.parts)
                if (p.r_lo < p.r_hi) raw_range_load_blocks(RAW_COLS_H, p.rows, p.plan.first_block, p.plan.nblocks, p.r_lo, p.r_hi, done, order);
            if (order.size() > k0) {
                rc = decode(k0, 6);
                if (rc) return rc;
                HIPCHK(c, hipStreamSynchronize(c->stream));
                commit_launches();
                add_ns(&g->st.decode_ns, &s->decode_ns, g->ev[6], g->ev[7]);
                for (size_t k = k0; k < order.size(); k++)
                    if (!block_ok(k, &why)) return framing(why);
            }
        }
    }
    // ---- the call's input is accepted
    fa_raw_range_stats_t& t = g->st;
    uint64_t unpacked = 0;
    for (const RangePart& p : run.parts) {
        t.rows_seen += p.rows;
        if (p.rows && !p.selected) t.parts_skipped_date++;
        else if (p.r_lo == p.r_hi) t.parts_empty++;
        else unpacked++;
    }
    t.calls++, t.parts_seen += np, t.blocks_seen += nb, t.blocks_decoded += blocks_decoded;
    s->calls++, s->frames += lz4 ? pr.walk.first.size() - 1 : 0, s->blocks += blocks_decoded, s->stored += stored, s->bytes_in += n, s->bytes_decoded += bytes_decoded;
    if (load) s->parts += unpacked;
    return FA_OK;
}

static int range_args(fa_ctx* c, const char* fn, const uint8_t* bytes, size_t n, uint32_t t_lo, uint32_t t_hi) {
    if (!bytes && n) {
        c->err = std::string(fn) + ": null argument";
        return FA_ERR_ARG;
    }
    if (t_lo > t_hi) {
        c->err = std::string(fn) + ": t_lo > t_hi";
        return FA_ERR_ARG;
    }
    return FA_OK;
}

extern "C" int fa_raw_range_probe(fa_ctx* c, const uint8_t* bytes, size_t n, uint32_t t_lo, uint32_t t_hi, fa_raw_range* out, size_t cap, size_t* n_out) {
    LOAD_ENTER(c);
    if (!n_out || (!out && cap)) return fail(c, FA_ERR_ARG, "fa_raw_range_probe: null argument");
    *n_out = 0;
    int rc = range_args(c, "fa_raw_range_probe", bytes, n, t_lo, t_hi);
    if (rc) return rc;
    LoadState* s = nullptr;
    rc = load_state(c, &s);
    if (rc) return rc;
    RangeState* g = nullptr;
    rc = range_state(c, &g);
    if (rc) return rc;
    RangeRun run;
    rc = range_run(c, s, g, "fa_raw_range_probe", bytes, n, t_lo, t_hi, false, cap, n_out, run);
    if (rc) return rc;
    for (size_t i = 0; i < run.parts.size(); i++) {
        const RangePart& p = run.parts[i];
        out[i] = fa_raw_range{p.date, p.t_min, p.t_max, 0, p.rows, p.r_lo, p.r_hi};
    }
    return FA_OK;
}

extern "C" int fa_raw_restore_range(fa_ctx* c, const uint8_t* bytes, size_t n, uint32_t t_lo, uint32_t t_hi, uint32_t key_sets, int folds) {
    LOAD_ENTER(c);
    RestoreSel sel;
    int rc = restore_select(c, "fa_raw_restore_range", key_sets, folds, &sel);
    if (rc) return rc;
    rc = range_args(c, "fa_raw_restore_range", bytes, n, t_lo, t_hi);
    if (rc) return rc;
    LoadState* s = nullptr;
    rc = load_state(c, &s);
    if (rc) return rc;
    RangeState* g = nullptr;
    rc = range_state(c, &g);
    if (rc) return rc;
    RangeRun run;
    rc = range_run(c, s, g, "fa_raw_restore_range", bytes, n, t_lo, t_hi, true, (size_t)-1, nullptr, run);
    if (rc) return rc;
    // (from here on every byte the slices' unpack reads is decoded and validated: a refused call has folded nothing)
    std::vector<LoadSlice> slices;
    uint64_t rows = 0;
    for (const RangePart& p : run.parts)
        if (p.r_lo < p.r_hi) slices.push_back({LoadPart{run.image + p.plan.off, p.plan.bytes, p.rows}, p.r_lo, p.r_hi}), rows += p.r_hi - p.r_lo;
    const uint64_t launches0 = s->launches;
    rc = restore_fold_slices(c, s, slices, sel);
    g->st.launches += s->launches - launches0;  // (the unpack launches)
    if (rc) return rc;
    g->st.rows_loaded += rows;
    return FA_OK;
}

extern "C" int fa_raw_range_stats(fa_ctx* c, fa_raw_range_stats_t* out) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (!out) return fail(c, FA_ERR_ARG, "fa_raw_range_stats: null argument");
    memset(out, 0, sizeof *out);
    if (c->range) *out = c->range->st;
    return FA_OK;
}
