// ingest_host.inc - the ingest path: tuple segments, device-side framing, launches, host staging (included by flowagg.hip: one translation unit, see kernels.cuh for the device side).

// ---- ingest ---------------------------------------------------------------------------
template <uint32_t KS, bool SEQ = false, int CANDM = -1>
static void launch_wtile(fa_ctx* c, const KArgs& a, const LaunchPlan& p) {
    const dim3 g(p.grid), b(wtile_block<KS>());
    if (p.t8) hipLaunchKernelGGL((wtile_kernel<KS, true, SEQ, CANDM>), g, b, 0, c->stream, a);
    else hipLaunchKernelGGL((wtile_kernel<KS, false, SEQ, CANDM>), g, b, 0, c->stream, a);
}
// The wave-tile kernel of a plan, for a variant with the flows_5m rollup.  The sketch variants exist once per top-k contract
// (the contract as a template argument: the exact mode's kernel carries no candidate test, the candidates mode's no probe of
// the big sets in its tile loop - config 3: 1.15 -> 1.08 ms and 1.115 -> 1.055 ms per launch, same box); without sketch
// segments, and in KS_ALL: the kernel that reads the contract from its arguments.  The learnt-order kernel: flows_5m alone.
template <uint32_t KS>
static void launch_wave_tiles(fa_ctx* c, const KArgs& a, const LaunchPlan& p) {
    if constexpr ((KS & (FA_KEYS_SRCADDR_CMS | FA_KEYS_DSTADDR_CMS)) != 0u && KS != KS_ALL)
        if (p.cms_segments) return c->cand_state ? launch_wtile<KS, false, 1>(c, a, p) : launch_wtile<KS, false, 0>(c, a, p);
    if constexpr (KS == 1u)
        if (p.seq_variant) return launch_wtile<1u, true>(c, a, p);
    launch_wtile<KS>(c, a, p);
}
// candidates mode: the boundary behind a batch - an ingest launch or a chunk of a sketch fold from columns (sketch_fold_host.inc) -
// on the ctx stream, behind every kernel of the batch that adds to a sketch: theta of this boundary and the bits the NEXT batch
// tests its addresses against.
static int cand_boundary(fa_ctx* c) {
    HIPCHK(c, hipMemsetAsync(c->cand_state, 0, 2 * sizeof(CandState), c->stream));
    const dim3 gs(CAND_SCAN_BLOCKS, 2), gb(256, 2);
    hipLaunchKernelGGL(cand_scan_kernel, gs, dim3(256), 0, c->stream, c->ks_src, c->ks_dst, 1u << c->ks_log2, (const unsigned long long*)c->cms_src,
                       (const unsigned long long*)c->cms_dst, c->cfg.cms_depth, c->cfg.cms_width_log2, c->cfg.cms_seed, c->cand_state, c->cand_chunkmax);
    hipLaunchKernelGGL(cand_bits_kernel, gb, dim3(256), 0, c->stream, (const KeySlot*)c->ks_src, (const KeySlot*)c->ks_dst, (const unsigned long long*)c->cms_src,
                       (const unsigned long long*)c->cms_dst, c->cfg.cms_depth, c->cfg.cms_width_log2, c->cfg.topk_track, std::max(c->ks_log2, 8u) - 2u, c->cand_state,
                       c->cand_bits[0], c->cand_bits[1]);
    return FA_OK;
}
// Launch order on the ctx stream: tile -> deferred -> [agg]   (the wave-tile kernel finds the batch's time base itself).
template <int MODE>
static int launch_tiles(fa_ctx* c, KArgs& a, const LaunchPlan& p, const hipEvent_t* ev) {
    // (wave tiles only with tuple segments, which only an ingest with the flows_5m rollup has)
    if (p.wave_tiles && (MODE != MODE_INGEST || !(p.variant & FA_KEYS_AS_PAIR) || !a.seg)) return fail(c, FA_ERR_ARG, "internal: wave tiles without tuple segments");
    const dim3 b(BLOCK), ge(std::min(256u, (a.n + BLOCK - 1) / BLOCK));
    a.par = c->par;
    c->par ^= 1u;
    if (ev) (void)hipEventRecord(ev[0], c->stream);
    if (p.seq_variant) c->stats.learnt_order_launches += 1;
    if (p.wave_tiles) c->stats.wave_tile_launches += 1;
    if (p.t8) c->stats.compact_tuple_launches += 1;
    // the bucket range of the wide tuples this launch leaves in its segments starts empty (Counters::wtb_min, wtb_nmax)
    if (p.wide_segments) HIPCHK(c, hipMemsetAsync(&c->d_ctr->wtb_min, 0xff, 2 * sizeof(unsigned int), c->stream));
    auto launch = [&](auto variant) {
        constexpr uint32_t KS = decltype(variant)::value;
        if (!p.wave_tiles) {
            hipLaunchKernelGGL((tile_kernel<MODE, KS>), dim3(p.grid), b, 0, c->stream, a);
        } else if constexpr (MODE == MODE_INGEST && (KS & FA_KEYS_AS_PAIR) != 0u) {  // (no other variant has a wave-tile kernel compiled)
            launch_wave_tiles<KS>(c, a, p);
        }
        if (ev) (void)hipEventRecord(ev[1], c->stream);
        // (the second-chance kernel runs in line: on a side stream beside the aggregation it cost MORE - 66 vs 58 us for
        // deferred + aggregation per launch, the cross-stream hand-over being slower than the 4.5 us kernel - and its atomic
        // upserts would race with the region-owned plain stores of agg8_kernel / cms_agg_kernel)
        hipLaunchKernelGGL((deferred_kernel<MODE, KS>), ge, b, 0, c->stream, a);
    };
    if constexpr (MODE == MODE_DECODE) launch(std::integral_constant<uint32_t, 1u>{});  // (the one decode kernel that is compiled)
    else with_variant(p.variant, launch);
    // Behind the ingest and second-chance kernels two chains that share nothing run side by side in the candidates mode:
    //   ctx stream   [fold the sketch tuples: cms_agg_kernel] -> [candidates mode: the launch boundary] -> [(SrcAddr,DstPort,Proto) tuples]
    //   side stream  [flows_5m tuple aggregation: agg8_kernel / agg_kernel]
    // The boundary's two small kernels (52 us of BASELINE config 3's 1.03 ms) and the tails of the two big ones - each one LDS-filling
    // workgroup per CU - overlap: 1.017-1.034 -> 0.966-0.983 ms per launch, same box (profiles/r06_exp_agg_side_stream.jsonl).
    // (candidates mode only: in the exact mode the two big kernels gain nothing from each other - measured 0 .. +1 % - and stay in line)
    hipStream_t agg_stream = c->stream;
    if (p.side) {
        HIPCHK(c, hipEventRecord(c->cand_ev[0], c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->cand_stream, c->cand_ev[0], 0));
        agg_stream = c->cand_stream;
    }
    if (p.wave_tiles) {
        const dim3 ga(1u << a.plog2);
        if (p.t8) hipLaunchKernelGGL(agg8_kernel, ga, dim3(AGG_BLOCK), 0, agg_stream, a);
        else hipLaunchKernelGGL(agg_kernel, ga, dim3(AGG_BLOCK), 0, agg_stream, a);
    }
    // Nothing returns between the fork and the join: the ctx stream's part is a lambda, whose early returns (HIPCHK) end that
    // part only - on every way out of this launch the ctx stream waits for the side stream.
    const hipError_t side_done = p.side ? hipEventRecord(c->cand_ev[1], c->cand_stream) : hipSuccess;
    const int rc = [&]() -> int {
        if (p.cms_segments) {  // fold the sketch tuples (Count-Min scatter sink)
            const uint32_t set_mask = (c->cfg.key_sets >> 1) & 3u;
            const uint32_t nlog = CMS_NPART * (set_mask == 3u ? 2u : 1u);
            hipLaunchKernelGGL(cms_agg_kernel, dim3(std::min<uint32_t>((uint32_t)c->num_cus, nlog)), dim3(AGG_BLOCK), 0, c->stream, a, set_mask, c->cms_par);  // persistent: one per CU
            c->cms_par ^= 1u;
        }
        // candidates mode: the launch boundary - theta of this boundary and the bits the NEXT launch tests its addresses against
        // (behind every kernel of the launch that adds to a sketch: hot-address flushes, the atomic paths, cms_agg_kernel)
        if (MODE == MODE_INGEST && c->cand_state) {
            const int brc = cand_boundary(c);
            if (brc) return brc;
        }
        // fold the (SrcAddr,DstPort,Proto) tuples: one workgroup per table region, plain loads and stores - behind every
        // dispatch of this launch that updates the wide table with atomics (wagg.cuh)
        if (p.wide_segments) {
            if (p.wlog) {  // log mode: the tuples stay where they are (the chunk is taken over behind the launch: wlog_record)
                // (the time base and the tuples' bucket range, three words: Counters::tb_base, wtb_min, wtb_nmax)
                HIPCHK(c, hipMemcpyAsync(c->wseg_counts + fa_ctx::wcounts_cap(c->wseg_counts), &c->d_ctr->tb_base, 3 * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
            } else {
                hipLaunchKernelGGL(wagg_kernel, dim3(1u << a.wplog2), dim3(WAGG_BLOCK), 0, c->stream, a, (const uint32_t*)nullptr, 0u);
            }
        }
        return FA_OK;
    }();
    // the join: everything behind this launch sees the aggregated table (on the host if the stream cannot wait for it)
    if (p.side && (side_done != hipSuccess || hipStreamWaitEvent(c->stream, c->cand_ev[1], 0) != hipSuccess)) {
        (void)hipStreamSynchronize(c->cand_stream);
        if (rc == FA_OK) return fail(c, FA_ERR_HIP, "joining the side stream failed");
    }
    if (rc) return rc;
    if (ev) (void)hipEventRecord(ev[2], c->stream);
    HIPCHK(c, hipGetLastError());
    return FA_OK;
}

// deferral lists for n records: exotic [0,cap) and retry [cap,2cap)
static int ensure_exotic(fa_ctx* c, size_t n) {
    if (c->exotic_cap() >= n) return FA_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t cap = std::max<size_t>(n, 1 << 16);
    if (!c->d_exotic.grow(2 * n * sizeof(uint32_t), 2 * cap * sizeof(uint32_t))) return fail(c, FA_ERR_NOMEM, "hipMalloc(deferral lists) failed");
    return FA_OK;
}

// Tuple segments for a batch of n records processed by p.grid workgroups: capacity per (partition,
// workgroup) = 2x the mean + 32 (a Poisson mean of m never reaches 2m+32; skewed batches overflow into
// the direct path), in whole 128-byte lines (8 wide / 16 compact tuples).  The region stride gets a skew of
// three lines so that consecutive partitions do not alias in L2.
static int ensure_segments(fa_ctx* c, size_t n, const LaunchPlan& p, KArgs& a) {
    const uint32_t nwg = (uint32_t)p.grid;
    const bool t8 = p.t8;
    const size_t NPART = (size_t)1 << c->plog2;
    const size_t avg = n / ((size_t)nwg * NPART);
    const uint32_t tpl = (t8 ? 2u : 1u) * bin_line(c->cfg.key_sets);  // tuples per store unit (a 128-byte line; flows_5m alone: half a line)
    uint32_t capq = (uint32_t)((2 * avg + 32 + tpl - 1) & ~(size_t)(tpl - 1));
    if (c->seg_cap_limit) capq = std::max<uint32_t>(std::min(capq, c->seg_cap_limit) & ~(tpl - 1), 2 * tpl);  // (tests: force the segment-overflow fallbacks)
    const size_t region = (size_t)nwg * capq + 3 * tpl;
    const size_t bytes = region * NPART * (t8 ? 8 : 16);
    if (c->seg.bytes() < bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!c->seg.grow(bytes)) return fail(c, FA_ERR_NOMEM, "hipMalloc(tuple segments) failed");
    }
    const size_t ncnt = (size_t)nwg * NPART_MAX * 2;  // front and back counts
    if (c->seg_counts.bytes() < ncnt * sizeof(uint32_t)) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!c->seg_counts.grow(ncnt * sizeof(uint32_t))) return fail(c, FA_ERR_NOMEM, "hipMalloc(segment counts) failed");
    }
    a.seg = c->seg;
    a.seg_counts = c->seg_counts;
    a.capq = capq;
    // (the LDS position counters are 16-bit halves of one word: caps leave room for the few increments that are in
    // flight before a full segment's overflow is taken back - sinks.cuh)
    a.capb = std::min<uint32_t>(std::max<uint32_t>(2 * tpl, (capq / 4) & ~(tpl - 1)), 0xff00u - tpl);  // back part: single tuples, bin leftovers
    a.capb = std::min(a.capb, capq - tpl);
    a.capf = std::min<uint32_t>(capq - a.capb, 0xff00u * tpl);                                           // front part: full lines
    a.nwg = nwg;  // (of every scatter sink's segments: the sketch and wide sinks exist only beside this one)
    a.region = region;
    a.plog2 = c->plog2;
    c->last_nwg = nwg;
    return FA_OK;
}

// Segments of the Count-Min scatter sink for a batch of n records processed by p.grid workgroups: per (sketch partition,
// workgroup) 3x the mean + 32 tuples of 16 bytes (a heavy hitter adds up to one tuple per wave-tile to its partition after
// the wave-level fold: about as much again as the partition's mean; what still overflows is added with atomics).
static int ensure_csegments(fa_ctx* c, size_t n, const LaunchPlan& p, KArgs& a) {
    const uint32_t nwg = (uint32_t)p.grid;
    const size_t nparts = (size_t)CMS_SETS * CMS_NPART;
    const size_t mean = n / ((size_t)CMS_NPART * nwg);
    uint32_t capq = (uint32_t)((3 * mean + 32 + 3) & ~(size_t)3);
    if (c->seg_cap_limit) capq = std::max<uint32_t>(std::min(capq, c->seg_cap_limit) & ~3u, 32u);  // (tests: force the overflow fallbacks)
    const size_t region = (size_t)nwg * capq + 12;
    const size_t bytes = region * nparts * sizeof(uint4);
    if (c->cseg.bytes() < bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!c->cseg.grow(bytes)) return fail(c, FA_ERR_NOMEM, "hipMalloc(sketch tuple segments) failed");
    }
    const size_t ncnt = (size_t)nwg * nparts * 2;
    if (c->cseg_counts.bytes() < ncnt * sizeof(uint32_t)) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!c->cseg_counts.grow(ncnt * sizeof(uint32_t))) return fail(c, FA_ERR_NOMEM, "hipMalloc(sketch segment counts) failed");
    }
    if (c->hot_seed_wgs < nwg) {  // the hot-address caches' surviving entries, one set per workgroup (sinks.cuh, HotAddrs)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->hot_seed_wgs = 0;
        const size_t ne = (size_t)nwg * CMS_SETS * HOT_SLOTS;
        if (!c->hot_seed.grow(ne * sizeof(HotSeed)) || !c->hot_seed_tag.grow(ne * sizeof(uint32_t))) return fail(c, FA_ERR_NOMEM, "hipMalloc(hot-address seeds) failed");
        HIPCHK(c, hipMemsetAsync(c->hot_seed_tag, 0, ne * sizeof(uint32_t), c->stream));
        c->hot_seed_wgs = nwg;
    }
    a.hot_seed = c->hot_seed;
    a.hot_seed_tag = c->hot_seed_tag;
    a.hot_epoch = c->hot_epoch++;
    if (!c->cms_psize) {
        const size_t bytes = (2 * (size_t)CMS_SETS * CMS_NPART + 2) * sizeof(uint32_t);  // (+ the two unit counters)
        if (!c->cms_psize.grow(bytes)) return fail(c, FA_ERR_NOMEM, "hipMalloc(sketch partition sizes) failed");
        HIPCHK(c, hipMemsetAsync(c->cms_psize, 0, bytes, c->stream));
    }
    a.cms_psize = c->cms_psize;
    a.cseg = c->cseg;
    a.cseg_counts = c->cseg_counts;
    a.ccapq = capq;
    a.ccapb = std::min<uint32_t>(std::max<uint32_t>(8u, (capq / 8) & ~3u), 0xff00u);
    a.ccapf = std::min<uint32_t>(capq - a.ccapb, 0xff00u * CMS_BIN);
    a.cregion = region;
    a.cms_sub = c->cfg.cms_width_log2 - 8u;
    return FA_OK;
}

// Segments of the wide scatter sink for a batch of n records processed by p.grid workgroups: per (table region, workgroup)
// 2x the mean + 32 tuples of 32 bytes (what overflows - a heavy key's region - takes the atomic path).
static int ensure_wsegments(fa_ctx* c, size_t n, const LaunchPlan& p, KArgs& a) {
    const uint32_t nwg = (uint32_t)p.grid;
    const size_t nparts = (size_t)1 << a.wplog2;
    const size_t mean = n / (nparts * nwg);
    uint32_t capq = (uint32_t)(2 * mean + 32);
    if (c->seg_cap_limit) capq = std::max<uint32_t>(std::min(capq, c->seg_cap_limit), 4u);  // (tests: force the overflow fallback)
    const size_t region = (size_t)nwg * capq + 6;  // (skew against power-of-two strides)
    const size_t bytes = region * nparts * 2 * sizeof(uint4);
    const size_t ncnt = (size_t)nwg * nparts;
    // Log mode keeps up to wlog_max + 1 pairs of buffers alive (the pending chunks and the one being filled; recycled through
    // wlog_free).  When another pair cannot be had - hipMalloc fails (FA_WSEG_BUDGET: the tests' stand-in for that) - the
    // ingest does not fail: buffers on the free list that are too small are released, then the OLDEST pending chunk is folded
    // into the table after all and its buffers are taken over; only a ctx that holds no chunk at all reports FA_ERR_NOMEM.
    auto held = [&]() { return (uint32_t)((c->wseg || c->wseg_counts ? 1 : 0) + c->wlog.size() + c->wlog_free.size()); };
    for (;;) {
        if (!c->wseg && !c->wseg_counts && !c->wlog_free.empty()) {  // the buffers of a chunk that has been folded or dropped
            c->wseg = std::move(c->wlog_free.back().seg);
            c->wseg_counts = std::move(c->wlog_free.back().counts);
            c->wlog_free.pop_back();
        }
        bool ok = true;
        if (c->wseg.bytes() < bytes || fa_ctx::wcounts_cap(c->wseg_counts) < ncnt) {
            HIPCHK(c, hipStreamSynchronize(c->stream));  // (a recycled pair may still be read by its chunk's fold)
            c->wseg.reset();  // (both go, so that the pair no longer counts as held)
            c->wseg_counts.reset();
            ok = !(c->wseg_budget && held() + 1u > c->wseg_budget) && c->wseg.grow(bytes) &&
                 c->wseg_counts.grow((ncnt + 4) * sizeof(uint32_t));  // (+ the time base and minimum bucket words of a log chunk)
            if (!ok) {
                (void)hipGetLastError();
                c->wseg.reset();
            }
        }
        if (ok) break;
        if (!c->wlog_free.empty()) continue;  // (the next pair of the free list - released if it is too small as well)
        if (c->wlog.empty()) return fail(c, FA_ERR_NOMEM, "hipMalloc(wide tuple segments) failed");
        int rc = wlog_flush_oldest(c);  // its buffers land on the free list
        if (rc) return rc;
        c->wlog_nomem_folds++;
    }
    a.wseg = c->wseg;
    a.wseg_counts = c->wseg_counts;
    a.wcapq = capq;
    a.wregion = region;
    return FA_OK;
}

static int ensure_dev(fa_ctx* c, DevBuf<>& b, size_t bytes, const char* what);
static int frame_split_host(const uint8_t* buf, size_t len, std::vector<uint64_t>& off);
// Device-side framing (framing.cuh): d_buf[0, len) is a chain of varint(len)-framed records -> *d_off = n + 1 offsets in HBM
// (owned by the ctx, valid until the next split), *n_out = records.  FA_ERR_FRAMING when it is not such a chain.
// h_buf: the same bytes in host memory when the caller has them (fa_ingest) - an unsettled stream is then walked there instead of
// being copied back.
static int frame_split_device(fa_ctx* c, const uint8_t* d_buf, size_t len, const uint32_t** d_off, size_t* n_out, const uint8_t* h_buf = nullptr) {
    *d_off = nullptr;
    *n_out = 0;
    if (len == 0) return FA_OK;
    const uint32_t nb = (uint32_t)((len + FS_BLOCK - 1) / FS_BLOCK);
    size_t tmp_scan = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_scan, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)nb, c->stream);
    const size_t arr = ((size_t)nb * 4 + 255) & ~(size_t)255;
    const size_t ent_bytes = ((size_t)nb * FS_NSUB + 255) & ~(size_t)255;
    int rc = ensure_dev(c, c->fs_scratch, 11 * arr + ent_bytes + tmp_scan + 512, "framing scratch");
    if (rc) return rc;
    uint8_t* base = (uint8_t*)c->fs_scratch;
    uint32_t* start = (uint32_t*)base;
    uint32_t* exits = (uint32_t*)(base + arr);
    uint32_t* cnt = (uint32_t*)(base + 2 * arr);
    uint32_t* bases = (uint32_t*)(base + 3 * arr);
    uint8_t* err = base + 4 * arr;             // (nb bytes)
    uint8_t* trust[2] = {base + 5 * arr, base + 6 * arr};  // (nb bytes each)
    uint32_t* list = (uint32_t*)(base + 7 * arr);          // (nb x 8 bytes) blocks whose start a round replaced, and the start they had: walked again
    unsigned long long* present = (unsigned long long*)(base + 9 * arr);  // (nb x 8 bytes) sub-blocks of a block in which a frame starts
    uint8_t* ent8 = base + 11 * arr;                       // ... and where the first one does (64 bytes per block)
    unsigned int* flag = (unsigned int*)(base + 11 * arr + ent_bytes);  // [0] blocks that differ, [1] blocks listed
    void* tmp = base + 11 * arr + ent_bytes + 256;
    const dim3 gl((nb + 255) / 256), bl(256);
    HIPCHK(c, hipMemsetAsync(start, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL((fs_guess_kernel_t<FS_PREFILTER, FS_PLAUSIBLE, FS_TIERS>), dim3((nb + 3) / 4), bl, 0, c->stream, d_buf, (uint32_t)len, nb, start);
    HIPCHK(c, hipGetLastError());
    bool settled = false;
    int rounds = 0;
    for (int round = 0; round < FS_MAX_ROUNDS && !settled; round++, rounds++) {
        const uint8_t* tin = round ? trust[(round - 1) & 1] : nullptr;
        HIPCHK(c, hipMemsetAsync(flag, 0, 2 * sizeof(unsigned int), c->stream));
        if (round == 0) {
            hipLaunchKernelGGL(fs_walk_kernel, gl, bl, 0, c->stream, d_buf, (uint32_t)len, nb, (const uint32_t*)start, cnt, err, exits, ent8, present);
        } else {
            hipLaunchKernelGGL(fs_apply_kernel, gl, bl, 0, c->stream, nb, start, (const uint32_t*)exits, tin, list, flag + 1);
            hipLaunchKernelGGL(fs_rewalk_kernel, dim3(std::min<uint32_t>(FS_REWALK_WGS, (nb + 255) / 256)), bl, 0, c->stream, d_buf, (uint32_t)len, nb, (const uint32_t*)start,
                               (const uint32_t*)list, (const unsigned int*)(flag + 1), cnt, err, exits, ent8, present);
        }
        hipLaunchKernelGGL(fs_round_kernel, gl, bl, 0, c->stream, nb, (const uint32_t*)start, (const uint32_t*)exits, tin, trust[round & 1], flag);
        HIPCHK(c, hipGetLastError());
        unsigned int differ = 0;
        HIPCHK(c, hipMemcpyAsync(&differ, flag, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        settled = differ == 0;
    }
    if (getenv("FA_VERBOSE")) fprintf(stderr, "[flowagg framing] %zu bytes, %u blocks: %s after %d round(s)\n", len, nb, settled ? "settled" : "NOT settled (host walk)", rounds);
    std::vector<uint32_t> h_off;
    if (settled) {
        HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(unsigned int), c->stream));
        hipLaunchKernelGGL(fs_err_kernel, dim3(64), dim3(256), 0, c->stream, (const uint8_t*)err, nb, flag);
        size_t tb = tmp_scan;
        if (hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, bases, (int)nb, c->stream) != hipSuccess) return fail(c, FA_ERR_HIP, "scan failed");
        unsigned int bad = 0;
        uint32_t last[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(&bad, flag, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&last[0], bases + (nb - 1), 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&last[1], cnt + (nb - 1), 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (bad) return fail(c, FA_ERR_FRAMING, "stream is not a chain of varint-framed records");
        const size_t n = (size_t)last[0] + last[1];
        rc = ensure_dev(c, c->fs_off, (n + 1) * sizeof(uint32_t), "frame offsets");
        if (rc) return rc;
        hipLaunchKernelGGL(fs_emit_kernel, dim3((nb + 3) / 4), dim3(256), 0, c->stream, d_buf, (uint32_t)len, nb, (const uint8_t*)ent8, (const unsigned long long*)present,
                           (const uint32_t*)bases, (uint32_t*)c->fs_off, (uint32_t)n);
        HIPCHK(c, hipGetLastError());
        *d_off = (const uint32_t*)c->fs_off;
        *n_out = n;
        return FA_OK;
    }
    // the guesses did not settle (records longer than several blocks, adversarial bytes): the host walks the stream
    std::vector<uint8_t> h;
    if (!h_buf) {
        h.resize(len);
        HIPCHK(c, hipMemcpy(h.data(), d_buf, len, hipMemcpyDeviceToHost));
        h_buf = h.data();
    }
    std::vector<uint64_t> off64;
    rc = frame_split_host(h_buf, len, off64);
    if (rc) return fail(c, rc, "stream is not a chain of varint-framed records");
    h_off.assign(off64.begin(), off64.end());
    rc = ensure_dev(c, c->fs_off, h_off.size() * sizeof(uint32_t), "frame offsets");
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(c->fs_off, h_off.data(), h_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    *d_off = (const uint32_t*)c->fs_off;
    *n_out = h_off.size() - 1;
    return FA_OK;
}

// One call's records -> launches.  len = bytes of the whole buffer the offsets point into (the bound the kernels clamp
// to); bytes = wire bytes of THESE n records (exact or estimated: tile sizing and the bytes_in statistic).
static int ingest_device_records(fa_ctx* c, const void* d_buf, size_t len, size_t bytes, const void* d_off, size_t n);

static int ingest_device_any(fa_ctx* c, const void* d_buf, size_t len, const void* d_off, size_t n, const uint8_t* h_buf);
extern "C" int fa_ingest_device(fa_ctx* c, const void* d_buf, size_t len, const void* d_off, size_t n) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    return ingest_device_any(c, d_buf, len, d_off, n, nullptr);
}
static int ingest_device_any(fa_ctx* c, const void* d_buf, size_t len, const void* d_off, size_t n, const uint8_t* h_buf) {
    if (!d_off) {  // offsets == NULL: the stream is split on the device (framing.cuh); n is ignored
        if (!c->cfg.framed) return fail(c, FA_ERR_ARG, "fa_ingest_device: offsets are required for bare (unframed) records");
        if (len == 0) return FA_OK;
        // (< 4 GiB - 1: 0xFFFFFFFF is the device split's "no such position")
        if (!d_buf || len >= 0xFFFFFFFFull || ((uintptr_t)d_buf & 15)) return fail(c, FA_ERR_ARG, "fa_ingest_device: bad buffer (16-byte aligned, < 4 GiB)");
        const uint32_t* off = nullptr;
        size_t total = 0;
        int rc = frame_split_device(c, (const uint8_t*)d_buf, len, &off, &total, h_buf);
        if (rc) return rc;
        size_t used = 0;
        for (size_t i = 0; i < total;) {
            const size_t m = std::min<size_t>(c->cfg.max_batch_records, total - i);
            const size_t bytes = i + m == total ? len - used : (size_t)((double)len * (double)m / (double)total);  // (an estimate per launch; exact in sum)
            rc = ingest_device_records(c, d_buf, len, bytes, off + i, m);
            if (rc) return rc;
            used += bytes;
            i += m;
        }
        // exact top talkers / bucketed ports / flows_raw parts: the second pass, once per call, behind everything the call queued (the offsets of the split above)
        return c->talk || c->ports || c->raw ? second_pass_records(c, d_buf, len, off, total) : FA_OK;
    }
    if (n == 0) return FA_OK;
    if (!d_buf || len >= (1ull << 32) || n > c->cfg.max_batch_records || ((uintptr_t)d_buf & 15) || ((uintptr_t)d_off & 3))
        return fail(c, FA_ERR_ARG, "fa_ingest_device: bad buffer (16-byte aligned, < 4 GiB, n <= max_batch_records)");
    const int rc = ingest_device_records(c, d_buf, len, len, d_off, n);
    if (rc || !(c->talk || c->ports || c->raw)) return rc;
    return second_pass_records(c, d_buf, len, (const uint32_t*)d_off, n);
}

// Room for one more launch's three events in a pool that settle hands back whole: afterwards the launch's take(3) creates
// nothing (a settle in between starts the pool over; the launch then takes its first triple).  A pool at its limit of `limit`
// launches is settled instead of grown; no event is destroyed before the ctx goes.
static int acquire_events(fa_ctx* c, Events& pool, size_t limit) {
    if (pool.used() + 3 <= pool.size()) return FA_OK;
    if (pool.size() >= 3 * limit) return settle(c);  // bound the pool: fold what is pending
    return pool.ensure(pool.used() + 3) ? FA_OK : events_failed(c);
}

// the launch arguments that name a table (settle / rebuild_* replace them)
static bool table_args_stale(const fa_ctx* c, const KArgs& a) {
    return a.tab != c->tab || a.mask != (1u << c->cap_log2) - 1 || a.wtab != c->wtab || a.wmask != (1u << c->wcap_log2) - 1;
}
static void refresh_table_args(fa_ctx* c, KArgs& a) {
    const KArgs f = make_args(c);
    a.tab = f.tab;
    a.mask = f.mask;
    a.rlog2 = f.rlog2;
    a.wtab = f.wtab;
    a.wmask = f.wmask;
    a.wplog2 = f.wplog2;
    a.agg_passes = f.agg_passes;
}
static int ingest_device_records(fa_ctx* c, const void* d_buf, size_t len, size_t bytes, const void* d_off, size_t n) {
    if (n == 0) return FA_OK;
    // The first big launch of a ctx with the (SrcAddr,DstPort,Proto) key set teaches it what the stream looks like: its first 2^20 (and
    // a margin) records go ahead as a launch of their own and the host looks at the counters before the rest follows - a stream that
    // opens a row per record (BASELINE config 5) keeps the rest of that launch in the log instead of folding 16 M rows into the
    // hash table first (one extra launch and one synchronisation in a ctx's life).
    if (c->wtab && (c->cfg.key_sets & FA_KEYS_ADDR_PORT_PROTO) && c->fb.wants_probe() && n >= (1u << 22)) {
        c->fb.mark_probed();
        const size_t m = ((size_t)1 << 20) + ((size_t)1 << 17);  // (the feedback's look wants 2^20 decoded records; some may be refused)
        const size_t b0 = (size_t)((double)bytes * (double)m / (double)n);
        int rc0 = ingest_device_records(c, d_buf, len, b0, d_off, m);
        if (rc0) return rc0;
        rc0 = settle(c);  // (the counters of those records: the feedback's look decides between table, scatter sink and log)
        if (rc0) return rc0;
        return ingest_device_records(c, d_buf, len, bytes - b0, (const uint32_t*)d_off + m, n - m);
    }
    c->fb.mark_probed();
    if (c->wide_per_record) {
        // a launch may not be able to park more wide-table updates than the spill buffer holds: split it
        const size_t lim = (c->wspill_cap - (1u << 20)) / c->wide_per_record;
        if (n > lim) {
            for (size_t i = 0; i < n; i += lim) {
                const size_t m = std::min(lim, n - i);
                int rc1 = ingest_device_records(c, d_buf, len, (size_t)((double)bytes * (double)m / (double)n), (const uint32_t*)d_off + i, m);
                if (rc1) return rc1;
            }
            return FA_OK;
        }
    }
    LaunchPlan p;  // (decided in three stages, launch_plan.h: here, with the grid known, and behind the preparations)
    plan_sink(p, c->cfg.key_sets, c->sink_mode, n, c->plog2, c->fb, c->stats.batches);
    if (n > AGG_MAX_BATCH && !p.t8) {  // the packed LDS sums of the wide-tuple aggregation hold 2^24 records per launch
        const size_t h = n / 2;
        int rc1 = ingest_device_records(c, d_buf, len, bytes / 2, d_off, h);
        if (rc1) return rc1;
        return ingest_device_records(c, d_buf, len, bytes - bytes / 2, (const uint32_t*)d_off + h, n - h);
    }
    int rc = pre_launch_guard(c, n);
    if (rc) return rc;
    rc = ensure_exotic(c, n);
    if (rc) return rc;
    rc = acquire_events(c, c->ev_pool, 4096);
    if (rc) return rc;
    KArgs a = make_args(c);
    a.buf = (const uint8_t*)d_buf;
    a.off = (const uint32_t*)d_off;
    a.n = (uint32_t)n;
    a.len = (uint32_t)len;
    if (p.wave_tiles) {  // wave-private tiles, sized by RECORDS
        p.tile_recs = wtile_recs_for(bytes, n, p.variant);
        p.grid = wtile_grid(a.n, p.tile_recs, p.variant, (uint32_t)c->num_cus);
    } else {
        p.tile_recs = tile_recs_for(bytes, n);
        p.grid = with_variant(p.variant, [&](auto v) { return grid_for(c, tile_kernel<MODE_INGEST, decltype(v)::value>, a.n, p.tile_recs); });
    }
    a.tile_recs = p.tile_recs;
    plan_segments(p, c->cfg.key_sets, c->cms_atomic, c->cms_scatter_ok, c->wtab != nullptr, c->fb);
    if (p.wave_tiles) {
        rc = ensure_segments(c, n, p, a);
        if (rc) return rc;
    }
    if (p.cms_segments) {
        rc = ensure_csegments(c, n, p, a);
        if (rc) return rc;
    }
    // (a segment-buffer pair that cannot be had folds the oldest log chunk - and that fold may settle, grow or rebuild a
    // table: the launch arguments built above would then point at freed memory.  Rebuilt, and the segments sized again
    // for the new region count, until nothing moved.)
    for (int guard = 0; p.wide_segments; guard++) {
        rc = ensure_wsegments(c, n, p, a);
        if (rc) return rc;
        if (!table_args_stale(c, a)) break;
        if (guard >= 4) return fail(c, FA_ERR_HIP, "internal: tables keep moving while a launch is prepared");
        refresh_table_args(c, a);
    }
    // (what the feedback rules say NOW: a settle inside the preparations above may have moved them)
    plan_followers(p, c->cfg.key_sets, c->cand_stream && c->cand_state, c->fb, c->stats.batches);
    if (c->wtab) c->wpot_total += (uint64_t)n * c->wide_per_record;  // (rows this launch may open in the wide table: wide_rows_bound)
    rc = launch_tiles<MODE_INGEST>(c, a, p, c->ev_pool.take(3));
    if (rc) return rc;
    if (p.wlog) {
        rc = wlog_record(c, a, n);
        if (rc) return rc;
    } else if (c->fb.left_log_mode() && !c->wlog.empty()) {
        // the library left the log mode: what is pending drains - a chunk per launch while wagg_kernel can take it (1.2 ms), one
        // in eight launches when the table has grown since and it is the atomic replay (13 ms for 16.67 M tuples)
        const fa_ctx::WChunk& k = c->wlog.front();
        if ((k.wplog2 == a.wplog2 && k.wmask == a.wmask) || c->stats.batches % 8 == 0) {
            rc = wlog_flush_oldest(c);
            if (rc) return rc;
        }
    }
    rc = post_launch_snapshot(c, n);
    if (rc) return rc;
    c->stats.bytes_in += bytes;
    c->stats.batches += 1;
    if (c->cfg.key_sets & (FA_KEYS_SRCADDR_CMS | FA_KEYS_DSTADDR_CMS)) {
        c->cms_dirty = c->cand_state == nullptr;  // (candidates mode: every path adds to copy 0 - nothing to fold)
        c->merged_valid = false;
    }
    return FA_OK;
}

static constexpr size_t FRAME_DEVICE_MIN = (size_t)1 << 20;  // fa_ingest(offsets == NULL): streams below it are walked on the host
// Splits a chain of framed records on the host (offsets == NULL).
static int frame_split_host(const uint8_t* buf, size_t len, std::vector<uint64_t>& off) {
    size_t p = 0;
    off.clear();
    while (p < len) {
        off.push_back(p);
        uint64_t v = 0;
        int i = 0;
        for (;; i++) {
            if (i >= 10 || p >= len) return FA_ERR_FRAMING;
            uint8_t b = buf[p++];
            if (i < 9)
                v |= (uint64_t)(b & 0x7f) << (7 * i);
            else
                v |= (uint64_t)(b & 1) << 63;
            if (!(b & 0x80)) break;
        }
        if (v > len - p) return FA_ERR_FRAMING;
        p += v;
    }
    off.push_back(len);
    return FA_OK;
}

static int ensure_stage(fa_ctx* c, int s, size_t bytes) {
    const size_t cap = std::max<size_t>(bytes + bytes / 4, 1 << 20);
    if (!c->h_stage[s].grow(bytes, cap)) return fail(c, FA_ERR_NOMEM, "hipHostMalloc(staging) failed");
    if (!c->d_in[s].grow(bytes, cap)) return fail(c, FA_ERR_NOMEM, "hipMalloc(input) failed");
    return FA_OK;
}

// Copies [buf,len) + offsets into pinned staging slot and uploads.  On return the
// caller's memory is no longer referenced.  Layout in the slot: bytes, pad to 16,
// 32 B slack, then n+1 uint32 offsets.
// threads of this process that are inside fa_ingest right now (the partition threads of a consumer call it concurrently,
// one ctx each - inserter.go:176), and the CPUs the process may really use (affinity mask cut by a cgroup CPU quota)
static std::atomic<int> g_ingest_active{0};
static unsigned usable_cpus() {
    static const unsigned n = [] {
        unsigned aff = std::max(1u, std::thread::hardware_concurrency());
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) aff = std::max(1, CPU_COUNT(&set));
        double quota = 0;
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
            char q[32] = {0};
            double per = 0;
            if (fscanf(f, "%31s %lf", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) quota = atof(q) / per;
            fclose(f);
        } else {
            long q = -1, per = 0;
            if (FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
                if (fscanf(fq, "%ld", &q) != 1) q = -1;
                fclose(fq);
            }
            if (FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (fscanf(fp, "%ld", &per) != 1) per = 0;
                fclose(fp);
            }
            if (q > 0 && per > 0) quota = (double)q / (double)per;
        }
        if (quota >= 1.0) aff = std::min(aff, (unsigned)quota);
        return std::max(1u, aff);
    }();
    return n;
}
static inline uint64_t host_ns() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static int stage_and_upload(fa_ctx* c, const uint8_t* buf, size_t len, const uint64_t* off, size_t n,
                            const uint8_t** d_buf, const uint32_t** d_off, int* slot) {
    if (len >= (1ull << 32) - 64) return fail(c, FA_ERR_ARG, "batch larger than 4 GiB; split it");
    int s = c->stage_cur;
    c->stage_cur ^= 1;
    size_t off_pos = ((len + 15) & ~(size_t)15) + 32;
    size_t total = off_pos + (n + 1) * sizeof(uint32_t);
    const uint64_t t_wait = host_ns();
    HIPCHK(c, hipEventSynchronize(c->stage_ev[s]));  // slot free again?
    int rc = ensure_stage(c, s, total);
    if (rc) return rc;
    const uint64_t t_copy = host_ns();
    c->stats.host_stage_wait_ns += t_copy - t_wait;

    uint8_t* hs = c->h_stage[s];
    uint32_t* ho = reinterpret_cast<uint32_t*>(hs + off_pos);
    // the copy into pinned memory and the u64 -> u32 narrowing of the offsets run on a few host threads: one thread
    // moves ~10 GB/s, the PCIe Gen5 link behind it 63 GB/s (env FA_STAGE_THREADS, default 8; small batches: inline)
    // ... shared with the other threads that are inside fa_ingest: 8 partition threads with 8 copy threads each on a host
    // whose cgroup grants 16 CPUs only take turns and get throttled (round 5's consumer: 64 M records/s through a library
    // that moves 670 M/s for one caller)
    const unsigned callers = (unsigned)std::max(1, g_ingest_active.load(std::memory_order_relaxed));
    unsigned nthr = std::max(1u, std::min(c->stage_threads, usable_cpus() / callers));
    if (len + n * 12 < (8u << 20)) nthr = 1;
    std::atomic<int> bad{0};
    auto work = [&](unsigned t) {
        const size_t b0 = len * t / nthr, b1 = len * (t + 1) / nthr;
        if (b1 > b0) memcpy(hs + b0, buf + b0, b1 - b0);
        const size_t i0 = (n + 1) * t / nthr, i1 = (n + 1) * (t + 1) / nthr;
        uint64_t prev = i0 ? off[i0 - 1] : 0;
        for (size_t i = i0; i < i1; i++) {
            const uint64_t o = off[i];
            if (o < prev || o > len) {
                bad.store(1);
                return;
            }
            prev = o;
            ho[i] = (uint32_t)o;
        }
    };
    if (nthr <= 1) {
        nthr = 1;
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nthr; t++) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
    }
    if (bad.load()) return fail(c, FA_ERR_ARG, "offsets must be non-decreasing and <= len");
    memset(hs + len, 0, off_pos - len);
    c->stats.host_stage_copy_ns += host_ns() - t_copy;
    HIPCHK(c, hipMemcpyAsync(c->d_in[s], hs, total, hipMemcpyHostToDevice, c->stream));
    *slot = s;  // caller records stage_ev[s] once the kernels reading d_in[s] are enqueued
    *d_buf = c->d_in[s];
    *d_off = reinterpret_cast<const uint32_t*>(c->d_in[s] + off_pos);
    return FA_OK;
}

static int ingest_host(fa_ctx* c, const uint8_t* buf, size_t len, const uint64_t* offsets, size_t n);
extern "C" int fa_ingest(fa_ctx* c, const uint8_t* buf, size_t len, const uint64_t* offsets, size_t n) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!buf && len) return fail(c, FA_ERR_ARG, "fa_ingest: null buffer");
    const uint64_t t0 = host_ns();
    g_ingest_active.fetch_add(1, std::memory_order_relaxed);
    const int rc = ingest_host(c, buf, len, offsets, n);
    g_ingest_active.fetch_sub(1, std::memory_order_relaxed);
    c->stats.host_ingest_ns += host_ns() - t0;
    return rc;
}
// What the first fa_ingest calls of a ctx would allocate inside the consumer's hot loop - both page-locked staging slots and
// their device twins (page-locking 2 x 64 MiB: tens of milliseconds), the deferral lists - for batches of up to `bytes` wire
// bytes in `records` records.  Optional: fa_ingest sizes everything on demand.
extern "C" int fa_reserve_ingest(fa_ctx* c, size_t bytes, size_t records) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (bytes >= (1ull << 32) - 64 || records > c->cfg.max_batch_records) return fail(c, FA_ERR_ARG, "fa_reserve_ingest: a batch is < 4 GiB and <= max_batch_records");
    const size_t total = ((bytes + 15) & ~(size_t)15) + 32 + (records + 1) * sizeof(uint32_t);
    for (int s = 0; s < 2; s++) {
        HIPCHK(c, hipEventSynchronize(c->stage_ev[s]));
        int rc = ensure_stage(c, s, total);
        if (rc) return rc;
        memset(c->h_stage[s], 0, std::min<size_t>(total, c->h_stage[s].bytes()));  // (first touch of the pinned pages: here, not in the loop)
    }
    return records ? ensure_exotic(c, records) : FA_OK;
}
static int ingest_host(fa_ctx* c, const uint8_t* buf, size_t len, const uint64_t* offsets, size_t n) {
    std::vector<uint64_t> split;
    if (!offsets && c->cfg.framed && len >= FRAME_DEVICE_MIN && len <= (1ull << 30)) {
        // a framed stream without offsets: the bytes are uploaded as they are and cut into records on the device (framing.cuh);
        // the host walk below - 1 GB/s - serves streams beyond one staging buffer and SMALL ones: the device split costs a guess
        // kernel and four or five stream synchronisations (~0.3 ms) whatever the size, the host walk of 1 MiB about 1 ms, and a
        // small call stays asynchronous on the host walk
        const uint64_t whole[2] = {0, len};
        const uint8_t* d_buf;
        const uint32_t* d_off;
        int slot = 0;
        int rc = stage_and_upload(c, buf, len, whole, 1, &d_buf, &d_off, &slot);
        if (rc) return rc;
        rc = ingest_device_any(c, d_buf, len, nullptr, 0, buf);  // (an unsettled chain is walked in the caller's memory)
        HIPCHK(c, hipEventRecord(c->stage_ev[slot], c->stream));
        return rc;
    }
    if (!offsets) {
        if (!c->cfg.framed) return fail(c, FA_ERR_ARG, "fa_ingest: offsets are required for bare (unframed) records");
        int rc = frame_split_host(buf, len, split);
        if (rc) return fail(c, rc, "fa_ingest: stream is not a chain of varint-framed records");
        offsets = split.data();
        n = split.size() - 1;
    }
    if (n == 0) return FA_OK;
    // chunk so that each launch stays under max_batch_records and 1 GiB of wire bytes
    size_t i = 0;
    while (i < n) {
        size_t j = std::min(n, i + (size_t)c->cfg.max_batch_records);
        while (j > i + 1 && offsets[j] - offsets[i] > (1ull << 30)) j = i + (j - i) / 2;
        std::vector<uint64_t> rel;
        const uint64_t* o = offsets + i;
        uint64_t base = offsets[i];
        if (base) {
            rel.resize(j - i + 1);
            for (size_t k = 0; k <= j - i; k++) {
                if (offsets[i + k] < base) return fail(c, FA_ERR_ARG, "offsets must be non-decreasing");
                rel[k] = offsets[i + k] - base;
            }
            o = rel.data();
        }
        if (offsets[j] > len || offsets[j] < base) return fail(c, FA_ERR_ARG, "offsets exceed len");
        const uint8_t* d_buf;
        const uint32_t* d_off;
        int slot = 0;
        int rc = stage_and_upload(c, buf + base, (size_t)(offsets[j] - base), o, j - i, &d_buf, &d_off, &slot);
        if (rc) return rc;
        rc = fa_ingest_device(c, d_buf, (size_t)(offsets[j] - base), d_off, j - i);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(c->stage_ev[slot], c->stream));
        i = j;
    }
    return FA_OK;
}
