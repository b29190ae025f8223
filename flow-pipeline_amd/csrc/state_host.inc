// state_host.inc - rows merged into the wide table, dashboard reset, sketches and distinct-address sets (included by flowagg.hip: one translation unit, see kernels.cuh for the device side).

// ---- wide key sets: window close and dashboard reads -----------------------------------------------
// rows (already packed keys) -> device -> wmerge_kernel
static int merge_wide(fa_ctx* c, const std::vector<WRow>& rows) {
    if (!c->wtab) return fail(c, FA_ERR_ARG, "key set not enabled");
    if (rows.empty()) return FA_OK;
    DevBuf<WRow> d;
    if (!d.grow(rows.size() * sizeof(WRow))) return fail(c, FA_ERR_NOMEM, "hipMalloc failed");
    auto hip_failed = [&](hipError_t e) {
        c->err = std::string("merge_wide: ") + hipGetErrorString(e);
        return FA_ERR_HIP;
    };
    hipError_t e = hipMemcpyAsync(d, rows.data(), rows.size() * sizeof(WRow), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_failed(e);
    KArgs a = make_args(c);
    hipLaunchKernelGGL(wmerge_kernel, dim3(256), dim3(256), 0, c->stream, d.get(), (uint32_t)rows.size(), a);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_failed(e);
    return settle(c);
}

extern "C" int fa_merge_rows_app(fa_ctx* c, const fa_row_app* rows, size_t n) {
    FA_ON_DEVICE(c);
    if (!c || (!rows && n)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!(c->cfg.key_sets & FA_KEYS_ADDR_PORT_PROTO)) return fail(c, FA_ERR_ARG, "FA_KEYS_ADDR_PORT_PROTO not enabled");
    std::vector<WRow> w(n);
    for (size_t i = 0; i < n; i++) {
        if (rows[i].timeslot % c->gran) return fail(c, FA_ERR_ARG, "fa_merge_rows_app: timeslot not on this ctx's bucket grid");
        uint64_t lo, hi;
        memcpy(&lo, rows[i].src_addr, 8);
        memcpy(&hi, rows[i].src_addr + 8, 8);
        WKey k;
        wkey_pack(WK_APP, rows[i].timeslot / c->gran, lo, hi, rows[i].dst_port, rows[i].proto, k);
        w[i] = WRow{{k.w[0], k.w[1], k.w[2], k.w[3]}, rows[i].bytes, rows[i].packets, rows[i].count};
    }
    return merge_wide(c, w);
}

__global__ void port_merge_kernel(const fa_port_row* rows, uint32_t n, ulonglong2* hist) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        unsigned long long* e = reinterpret_cast<unsigned long long*>(&hist[rows[i].port]);
        if (rows[i].weight) atomicAdd(e, (unsigned long long)rows[i].weight);
        atomicAdd(e + 1, (unsigned long long)rows[i].count);
    }
}

extern "C" int fa_merge_ports(fa_ctx* c, int dst, const fa_port_row* rows, size_t n) {
    FA_ON_DEVICE(c);
    if (!c || (!rows && n) || (dst != 0 && dst != 1)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->port_hist) return fail(c, FA_ERR_ARG, "FA_KEYS_PORT_HIST not enabled");
    std::vector<fa_port_row> small;
    std::vector<WRow> big;
    for (size_t i = 0; i < n; i++) {
        if (rows[i].port < PORT_DENSE) {
            small.push_back(rows[i]);
        } else {
            WKey k;
            wkey_pack(dst ? WK_DSTPORT : WK_SRCPORT, 0, 0, 0, rows[i].port, 0, k);
            big.push_back(WRow{{k.w[0], k.w[1], k.w[2], k.w[3]}, rows[i].weight, 0, rows[i].count});
        }
    }
    if (!small.empty()) {
        DevBuf<fa_port_row> d;
        if (!d.grow(small.size() * sizeof(fa_port_row))) return fail(c, FA_ERR_NOMEM, "hipMalloc failed");
        auto hip_failed = [&](hipError_t e) {
            c->err = std::string("fa_merge_ports: ") + hipGetErrorString(e);
            return FA_ERR_HIP;
        };
        hipError_t e = hipMemcpyAsync(d, small.data(), small.size() * sizeof(fa_port_row), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return hip_failed(e);
        hipLaunchKernelGGL(port_merge_kernel, dim3(64), dim3(256), 0, c->stream, d.get(), (uint32_t)small.size(),
                           c->port_hist + (size_t)dst * PORT_DENSE);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_failed(e);
    }
    return merge_wide(c, big);
}

extern "C" int fa_merge_minutes(fa_ctx* c, const fa_minute_row* rows, size_t n) {
    FA_ON_DEVICE(c);
    if (!c || (!rows && n)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!(c->cfg.key_sets & FA_KEYS_MINUTE_SERIES)) return fail(c, FA_ERR_ARG, "FA_KEYS_MINUTE_SERIES not enabled");
    std::vector<WRow> w(n);
    for (size_t i = 0; i < n; i++) {
        if (rows[i].minute % 60u) return fail(c, FA_ERR_ARG, "fa_merge_minutes: not a minute boundary");
        WKey k;
        wkey_pack(WK_MINUTE, 0, 0, 0, rows[i].minute / 60u, 0, k);
        w[i] = WRow{{k.w[0], k.w[1], k.w[2], k.w[3]}, rows[i].weight, 0, rows[i].count};
    }
    return merge_wide(c, w);
}

extern "C" int fa_dashboard_reset(fa_ctx* c) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    int rc = settle(c);
    if (rc) return rc;
    if (c->port_hist) HIPCHK(c, hipMemsetAsync(c->port_hist, 0, sizeof(ulonglong2) * 2 * PORT_DENSE, c->stream));
    if (c->wtab && (c->cfg.key_sets & (FA_KEYS_PORT_HIST | FA_KEYS_MINUTE_SERIES)))
        return rebuild_wide(c, c->wcap_log2, (1u << WK_SRCPORT) | (1u << WK_DSTPORT) | (1u << WK_MINUTE), 0, 0);
    return FA_OK;
}

// ---- sketches -----------------------------------------------------------------------------------
// Sums the sketch copies into copy 0 (sinks.cuh, cms_add).  Every reader of a sketch calls this first.
static int cms_fold(fa_ctx* c) {
    if (!c->cms_dirty) return FA_OK;
    for (unsigned long long* p : {c->cms_src.get(), c->cms_dst.get()})
        if (p) hipLaunchKernelGGL(cms_fold_kernel, dim3(2048), dim3(256), 0, c->stream, p, c->cms_words);
    HIPCHK(c, hipGetLastError());
    c->cms_dirty = false;
    return FA_OK;
}

// the sketch readers answer from: the merged (all-rank) view while it is valid, the ctx's own sketch otherwise
static unsigned long long* cms_of(fa_ctx* c, uint32_t key_set) {
    if (key_set == FA_KEYS_SRCADDR_CMS) return c->merged_valid && c->cms_src_m ? c->cms_src_m : c->cms_src;
    if (key_set == FA_KEYS_DSTADDR_CMS) return c->merged_valid && c->cms_dst_m ? c->cms_dst_m : c->cms_dst;
    return nullptr;
}
static int ensure_merged_view(fa_ctx* c) {
    for (int d = 0; d < 2; d++) {
        unsigned long long* own = d ? c->cms_dst : c->cms_src;
        DevBuf<unsigned long long>& m = d ? c->cms_dst_m : c->cms_src_m;
        if (own && !m.grow(c->cms_words * 8)) return fail(c, FA_ERR_NOMEM, "hipMalloc(merged sketch view) failed");
    }
    return FA_OK;
}

extern "C" int fa_cms_read(fa_ctx* c, uint32_t key_set, uint64_t* out, size_t cap_words) {
    FA_ON_DEVICE(c);
    if (!c || !out) return FA_ERR_ARG;
    unsigned long long* p = cms_of(c, key_set);
    if (!p) return fail(c, FA_ERR_ARG, "key set not enabled");
    if (cap_words < c->cms_words) return fail(c, FA_ERR_CAPACITY, "sketch buffer too small");
    int rc = settle(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(out, p, c->cms_words * 8, hipMemcpyDeviceToHost));
    return FA_OK;
}

extern "C" int fa_cms_reset(fa_ctx* c, uint32_t key_set) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    unsigned long long* p = key_set == FA_KEYS_SRCADDR_CMS ? c->cms_src : key_set == FA_KEYS_DSTADDR_CMS ? c->cms_dst : nullptr;
    if (!p) return fail(c, FA_ERR_ARG, "key set not enabled");
    c->merged_valid = false;
    HIPCHK(c, hipMemsetAsync(p, 0, c->cms_words * 8 * CMS_REPLICAS, c->stream));
    KeySlot* ks = key_set == FA_KEYS_SRCADDR_CMS ? c->ks_src : c->ks_dst;
    if (ks) HIPCHK(c, hipMemsetAsync(ks, 0, sizeof(KeySlot) << c->ks_log2, c->stream));
    c->tk_lb_k[key_set == FA_KEYS_SRCADDR_CMS ? 0 : 1] = 0;  // (estimates start over: nothing is known about the k-th one)
    uint32_t* bits = c->cand_bits[key_set == FA_KEYS_SRCADDR_CMS ? 0 : 1];  // candidates mode: back to "nothing admitted yet"
    if (bits) HIPCHK(c, hipMemsetAsync(bits, 0, c->cand_bits_bytes, c->stream));
    return FA_OK;
}

static uint32_t cms_column_host(const uint8_t key[16], uint64_t seed, uint32_t wl2, uint32_t row) {
    uint64_t lo, hi, h1, h2;
    memcpy(&lo, key, 8);
    memcpy(&hi, key + 8, 8);
    cms_hash2(lo, hi, seed, h1, h2);  // (sinks.cuh: the one definition, host and device)
    return cms_column(cms_key(h1, h2, wl2), row, wl2);
}

extern "C" int fa_cms_query(fa_ctx* c, uint32_t key_set, const uint8_t key[16], uint64_t* weight) {
    FA_ON_DEVICE(c);
    if (!c || !key || !weight) return FA_ERR_ARG;
    unsigned long long* p = cms_of(c, key_set);
    if (!p) return fail(c, FA_ERR_ARG, "key set not enabled");
    int rc = settle(c);
    if (rc) return rc;
    uint64_t best = ~0ull;
    for (uint32_t r = 0; r < c->cfg.cms_depth; r++) {
        size_t idx = ((size_t)r << c->cfg.cms_width_log2) + cms_column_host(key, c->cfg.cms_seed, c->cfg.cms_width_log2, r);
        unsigned long long v;
        HIPCHK(c, hipMemcpy(&v, p + idx, 8, hipMemcpyDeviceToHost));
        best = std::min<uint64_t>(best, v);
    }
    *weight = best;
    return FA_OK;
}

extern "C" int fa_topk_merge_keys(fa_ctx* c, uint32_t key_set, const uint8_t* keys, size_t n) {
    FA_ON_DEVICE(c);
    if (!c || (!keys && n)) return FA_ERR_ARG;
    if (c->sticky) return c->sticky;
    KeySlot* ks = key_set == FA_KEYS_SRCADDR_CMS ? c->ks_src : key_set == FA_KEYS_DSTADDR_CMS ? c->ks_dst : nullptr;
    if (!ks) return fail(c, FA_ERR_ARG, "fa_topk_merge_keys: key set not enabled");
    if (!n) return FA_OK;
    DevBuf<uint4> d;
    if (!d.grow(n * 16)) return fail(c, FA_ERR_NOMEM, "hipMalloc failed");
    auto hip_failed = [&](hipError_t e) {
        c->err = std::string("fa_topk_merge_keys: ") + hipGetErrorString(e);
        return FA_ERR_HIP;
    };
    hipError_t e = hipMemcpyAsync(d, keys, n * 16, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_failed(e);
    KArgs a = make_args(c);
    hipLaunchKernelGGL(keyset_merge_kernel, dim3(256), dim3(256), 0, c->stream, d.get(), (uint32_t)n, ks, a);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_failed(e);
    return FA_OK;
}
