// group_host.inc - the merged sketch view, the RCCL binding, and the window close of a GROUP of contexts inside one process
// (included by flowagg.hip: one translation unit, see kernels.cuh for the device side).
//
// The reference's consumer is ONE process with one goroutine per claimed Kafka partition (inserter/inserter.go:167-196, :176;
// the topic has --partitions 2, compose/docker-compose-clickhouse-mock.yml:18; the north star shards 8 partitions over 8 GPUs).
// Ingest needs nothing from a group - a ctx per (partition, GPU), no data-path collective.  The window close does: flows_5m rows
// could be left to SummingMergeTree (create.sh:70-90 sums partial rows downstream), but the sketches, the top-k and the
// (SrcAddr,DstPort,Proto) rows have no such downstream.  fa_group_* is that close behind the C-ABI: every step stays in HBM
// and is the composition of the ABI 5/6 steps (fa_rows_device -> [fa_rows_partition_device] -> exchange -> fa_rows_merge_device)
// that flow-pipeline_amd/dist.py drives across PROCESSES over torch.distributed; here the exchange is a peer copy
// (hipMemcpyPeerAsync over xGMI: inside one process no communicator is needed) and the members work in parallel on host threads.

extern "C" int fa_device_state_get(fa_ctx* c, fa_device_state* out) {
    FA_ON_DEVICE(c);
    if (!c || !out) return FA_ERR_ARG;
    int rc = settle(c);
    if (rc) return rc;
    out->cms_src = c->cms_src;
    out->cms_dst = c->cms_dst;
    out->cms_words = c->cms_words;
    out->port_hist = c->port_hist;
    out->port_hist_words = c->port_hist ? (size_t)4 * PORT_DENSE : 0;
    rc = ensure_merged_view(c);
    if (rc) return rc;
    out->cms_src_merged = c->cms_src_m;
    out->cms_dst_merged = c->cms_dst_m;
    return FA_OK;
}

extern "C" int fa_merged_view_set(fa_ctx* c, int valid) {
    FA_ON_DEVICE(c);
    if (!c) return FA_ERR_ARG;
    if (valid && ((c->cms_src && !c->cms_src_m) || (c->cms_dst && !c->cms_dst_m))) return fail(c, FA_ERR_ARG, "fa_merged_view_set: no merged view (call fa_device_state_get first)");
    c->merged_valid = valid != 0;
    return FA_OK;
}

// ---- RCCL, bound lazily so that libflowagg.so loads on hosts without librccl ----------------------------------------------
#include <dlfcn.h>
struct RcclApi {
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    bool tried = false;
};
static const RcclApi* rccl_api() {
    static RcclApi api;
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    if (!api.tried) {
        api.tried = true;
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            api.AllReduce = (decltype(api.AllReduce))dlsym(h, "ncclAllReduce");
            api.CommInitAll = (decltype(api.CommInitAll))dlsym(h, "ncclCommInitAll");
            api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
            api.GroupStart = (decltype(api.GroupStart))dlsym(h, "ncclGroupStart");
            api.GroupEnd = (decltype(api.GroupEnd))dlsym(h, "ncclGroupEnd");
        }
    }
    return api.AllReduce ? &api : nullptr;
}
// ncclAllReduce(sum, u64) of the ctx's sketches INTO its merged view, queued on the ctx stream (no wait): the caller settles
// the ctx first and synchronises behind it - one call per rank (fa_merge_allreduce), or one per member between ncclGroupStart /
// ncclGroupEnd when several communicators live in one process (fa_group_allreduce_sketches: RCCL deadlocks otherwise)
static int allreduce_enqueue(fa_ctx* c, const RcclApi* api, void* comm) {
    const int ncclUint64 = 5, ncclSum = 0;  // rccl.h: ncclDataType_t / ncclRedOp_t
    c->merged_valid = false;
    if (c->cms_src && api->AllReduce(c->cms_src, c->cms_src_m, c->cms_words, ncclUint64, ncclSum, comm, c->stream) != 0)
        return fail(c, FA_ERR_HIP, "ncclAllReduce(cms_src) failed");
    if (c->cms_dst && api->AllReduce(c->cms_dst, c->cms_dst_m, c->cms_words, ncclUint64, ncclSum, comm, c->stream) != 0)
        return fail(c, FA_ERR_HIP, "ncclAllReduce(cms_dst) failed");
    return FA_OK;
}
extern "C" int fa_merge_allreduce(fa_ctx* c, void* comm) {
    FA_ON_DEVICE(c);
    if (!c || !comm) return FA_ERR_ARG;
    const RcclApi* api = rccl_api();
    if (!api) return fail(c, FA_ERR_UNSUPPORTED, "librccl.so / ncclAllReduce not found");
    int rc = settle(c);  // (folds the sketch copies into copy 0)
    if (rc) return rc;
    rc = ensure_merged_view(c);
    if (rc) return rc;
    rc = allreduce_enqueue(c, api, comm);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->merged_valid = true;
    return FA_OK;
}

// ---- the group -------------------------------------------------------------------------------------------------------------
// One host thread per member beyond the first, alive as long as the group: a close runs four or five parallel steps, and round 5
// spawned and joined n - 1 threads for every one of them.
struct GroupPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    std::function<void(size_t)> job;  // the step every worker runs for its member (set under mu)
    uint64_t gen = 0;                 // step counter: a worker runs the job once per generation
    size_t pending = 0;               // workers that have not finished the current generation
    bool stop = false;
    void start(size_t workers, const std::vector<int>& device_of) {
        for (size_t w = 0; w < workers; w++)
            th.emplace_back([this, w, dev = device_of[w + 1]] {
                (void)hipSetDevice(dev);
                uint64_t seen = 0;
                for (;;) {
                    std::function<void(size_t)> f;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv_go.wait(lk, [&] { return stop || gen != seen; });
                        if (stop) return;
                        seen = gen;
                        f = job;
                    }
                    f(w + 1);
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        if (--pending == 0) cv_done.notify_one();
                    }
                }
            });
    }
    // f(i) on worker i - 1 for i = 1..workers, f(0) on the caller; returns when all are done
    void run(const std::function<void(size_t)>& f) {
        {
            std::lock_guard<std::mutex> lk(mu);
            job = f;
            pending = th.size();
            gen++;
        }
        cv_go.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
    }
    ~GroupPool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_go.notify_all();
        for (auto& t : th) t.join();
    }
};
struct fa_group {
    std::vector<fa_ctx*> m;          // members, in the caller's order (member i = Kafka partition i's ctx)
    // (the device buffer the exchange writes into is the MEMBER's: fa_ctx::xch_buf - reserved when its rows come into being)
    std::vector<void*> comms;        // ncclComm_t per member (transport FA_GROUP_RCCL)
    int transport = FA_GROUP_PEER;
    uint32_t next_root = 0;          // merged reads rotate their root over the members (the merge's HBM and PCIe work with it)
    std::unique_ptr<GroupPool> pool; // n - 1 host threads (none for a group of one)
    std::string err;
};
static thread_local std::string g_group_error;

static int gfail(fa_group* g, int code, const std::string& msg) {
    g->err = msg;
    return code;
}
// a member's failure is the group's - and every member reports it (a caller that only looks at "its" ctx still sees it)
static int gfail_member(fa_group* g, size_t i, int code, const char* what) {
    const std::string text = std::string(what) + ": member " + std::to_string(i) + ": " + g->m[i]->err;
    for (size_t j = 0; j < g->m.size(); j++)
        if (j != i) g->m[j]->err = "group: " + text;
    g->err = text;
    return code;
}
// f(i) for every member, on host threads (each GPU collects / sorts / copies on its own; the calls block on their stream):
// returns the first failing member's code
template <class F>
static int group_each(fa_group* g, const char* what, F f) {
    const size_t n = g->m.size();
    std::vector<int> rc(n, FA_OK);
    if (n == 1 || !g->pool) {
        for (size_t i = 0; i < n; i++) {
            (void)hipSetDevice(g->m[i]->cfg.device);
            rc[i] = f(i);
        }
    } else {
        (void)hipSetDevice(g->m[0]->cfg.device);
        g->pool->run([&](size_t i) { rc[i] = f(i); });  // (every worker selected its member's device when it started)
    }
    for (size_t i = 0; i < n; i++)
        if (rc[i]) return gfail_member(g, i, rc[i], what);
    return FA_OK;
}
static int group_recv(fa_group* g, size_t r, size_t bytes) {
    fa_ctx* c = g->m[r];
    (void)hipSetDevice(c->cfg.device);
    return ensure_dev(c, c->xch_buf, std::max<size_t>(bytes, 256), "group exchange buffer");
}
// `bytes` from member p's HBM into member r's, queued on r's stream: a plain device copy when both live on one GPU, a peer
// copy otherwise (xGMI when the peers can reach each other - enabled at fa_group_create -, staged by the runtime when not)
static hipError_t group_copy(fa_group* g, size_t r, void* dst, size_t p, const void* src, size_t bytes) {
    if (!bytes) return hipSuccess;
    fa_ctx *cr = g->m[r], *cp = g->m[p];
    (void)hipSetDevice(cr->cfg.device);
    if (cr->cfg.device == cp->cfg.device) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, cr->stream);
    return hipMemcpyPeerAsync(dst, cr->cfg.device, src, cp->cfg.device, bytes, cr->stream);
}
// waits for what is queued on member i's stream
static int member_sync(fa_group* g, size_t i, const char* what) {
    (void)hipSetDevice(g->m[i]->cfg.device);
    const hipError_t e = hipStreamSynchronize(g->m[i]->stream);
    if (e == hipSuccess) return FA_OK;
    g->m[i]->err = std::string(what) + ": " + hipGetErrorString(e);
    return gfail_member(g, i, FA_ERR_HIP, what);
}
static int group_sync(fa_group* g, const char* what) {
    for (size_t i = 0; i < g->m.size(); i++)
        if (int rc = member_sync(g, i, what)) return rc;
    return FA_OK;
}
// what a call that works with the members' state refuses up front
static int group_sticky(fa_group* g) {
    for (fa_ctx* c : g->m)
        if (c->sticky) return gfail(g, c->sticky, "a member context holds a sticky error");
    return FA_OK;
}
// words of a sketch one member sums in the peer all-reduce (even: 16-byte loads); fa_group_create reserves what it receives
static size_t sketch_slice_words(size_t words, size_t n) { return ((words + n - 1) / n + 1) & ~(size_t)1; }

extern "C" int fa_group_create(fa_ctx* const* ctxs, size_t n, uint32_t flags, fa_group** out) {
    if (!ctxs || !out || n == 0 || n > RPART_MAX_WORLD || (flags & ~1u)) {
        g_group_error = "fa_group_create: bad argument (1 <= n <= 1024 contexts, flags: FA_GROUP_PEER / FA_GROUP_RCCL)";
        return FA_ERR_ARG;
    }
    *out = nullptr;
    for (size_t i = 0; i < n; i++) {
        if (!ctxs[i]) {
            g_group_error = "fa_group_create: null context";
            return FA_ERR_ARG;
        }
        for (size_t j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) {
                g_group_error = "fa_group_create: a context appears twice";
                return FA_ERR_ARG;
            }
        // one merge, one result: every member has to aggregate the same thing on the same grid
        const fa_config &a = ctxs[0]->cfg, &b = ctxs[i]->cfg;
        if (a.window_secs != b.window_secs || a.subwindow_secs != b.subwindow_secs || a.key_sets != b.key_sets || a.cms_depth != b.cms_depth ||
            a.cms_width_log2 != b.cms_width_log2 || a.cms_seed != b.cms_seed) {
            g_group_error = "fa_group_create: members differ in window / key-set / sketch configuration";
            return FA_ERR_ARG;
        }
        // ... and rank by the same top-k contract (a mixed group would rank the union of an exact member's universe and a
        // candidates member's admitted keys - neither contract)
        // (the capacity of the sets is part of the candidates contract - theta's weight term - and only a size in the exact mode)
        if ((a.key_sets & (FA_KEYS_SRCADDR_CMS | FA_KEYS_DSTADDR_CMS)) &&
            (a.topk_mode != b.topk_mode || (a.topk_mode == FA_TOPK_CANDIDATES && (a.topk_track != b.topk_track || a.topk_capacity_log2 != b.topk_capacity_log2)))) {
            g_group_error = "fa_group_create: members differ in top-k configuration (topk_mode; candidates mode: topk_track / topk_capacity_log2)";
            return FA_ERR_ARG;
        }
        if (ctxs[i]->group_members) {
            g_group_error = "fa_group_create: a context is already a member of a group";
            return FA_ERR_ARG;
        }
    }
    std::unique_ptr<fa_group> g(new fa_group());
    g->m.assign(ctxs, ctxs + n);
    std::vector<int> dev(n);  // the members' devices
    for (size_t i = 0; i < n; i++) dev[i] = ctxs[i]->cfg.device;
    // peers that can reach each other exchange over xGMI without a bounce through host memory
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) {
            const int di = dev[i], dj = dev[j];
            int can = 0;
            if (di == dj || hipDeviceCanAccessPeer(&can, di, dj) != hipSuccess || !can) continue;
            (void)hipSetDevice(di);
            (void)hipDeviceEnablePeerAccess(dj, 0);  // (hipErrorPeerAccessAlreadyEnabled is fine)
            (void)hipGetLastError();
        }
    if (flags & FA_GROUP_RCCL) {
        // one communicator per member, made in one call (ncclCommInitAll): needs a GPU per member
        const RcclApi* api = rccl_api();
        bool distinct = true;
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < i; j++) distinct = distinct && dev[j] != dev[i];
        if (!api || !api->CommInitAll || !api->CommDestroy || !api->GroupStart || !api->GroupEnd) {
            g_group_error = "fa_group_create: FA_GROUP_RCCL, but librccl.so could not be loaded";
            return FA_ERR_UNSUPPORTED;
        }
        if (!distinct) {
            g_group_error = "fa_group_create: FA_GROUP_RCCL needs every member on its own GPU (use FA_GROUP_PEER)";
            return FA_ERR_UNSUPPORTED;
        }
        g->comms.assign(n, nullptr);
        if (api->CommInitAll(g->comms.data(), (int)n, dev.data()) != 0) {
            g_group_error = "fa_group_create: ncclCommInitAll failed";
            return FA_ERR_HIP;
        }
        g->transport = FA_GROUP_RCCL;
    }
    if (n > 1) {
        g->pool.reset(new GroupPool());
        g->pool->start(n - 1, dev);
    }
    // What the first close would allocate is allocated here (round 5: the first partitioned close of 8 members took 120 ms, the
    // median 62 - 24 hipMallocs of a gigabyte inside it): the merged sketch views and the slices the reduce-scatter receives,
    // and - for members that already hold (SrcAddr,DstPort,Proto) rows - the partition, exchange and merge buffers of a window;
    // members that ingest AFTER this call reserve theirs when a launch's tuples enter the log (reserve_window_read).  Best
    // effort: a failed reservation is the close's error, not the create's.
    for (size_t i = 0; i < n; i++) ctxs[i]->group_members = (uint32_t)n;
    (void)group_each(g.get(), "reserve", [&](size_t i) {
        fa_ctx* c = g->m[i];
        const std::string keep = c->err;
        if ((c->cms_src || c->cms_dst) && n > 1) {
            (void)ensure_merged_view(c);
            if (g->transport == FA_GROUP_PEER) (void)ensure_dev(c, c->xch_buf, (n - 1) * sketch_slice_words(c->cms_words, n) * 8, "group exchange buffer");
        }
        if (n > 1 && c->wtab && (c->cfg.key_sets & FA_KEYS_ADDR_PORT_PROTO)) {
            uint64_t rows = c->stats.wide_used;
            uint32_t nseg = 0;
            for (const fa_ctx::WChunk& k : c->wlog) {
                rows += k.n;
                nseg = std::max(nseg, (1u << k.wplog2) * k.nwg);
            }
            // (a window is a fraction of what a member holds; what it holds bounds it - capped at 2^25 rows: 1.9 GB per buffer)
            if (rows) reserve_window_read(c, std::min<uint64_t>(rows, 1u << 25), nseg);
        }
        c->err = keep;
        return (int)FA_OK;
    });
    g->err.clear();
    *out = g.release();
    return FA_OK;
}

extern "C" void fa_group_destroy(fa_group* g) {
    if (!g) return;
    g->pool.reset();  // (joins the workers)
    for (size_t i = 0; i < g->m.size(); i++) {
        (void)hipSetDevice(g->m[i]->cfg.device);
        (void)hipStreamSynchronize(g->m[i]->stream);
        g->m[i]->group_members = 0;  // (the exchange buffer stays the ctx's: freed by fa_destroy, reused by a later group)
    }
    if (!g->comms.empty())
        if (const RcclApi* api = rccl_api())
            for (void* c : g->comms)
                if (c) (void)api->CommDestroy(c);
    delete g;  // (the contexts stay the caller's)
}

extern "C" const char* fa_group_last_error(const fa_group* g) { return g ? g->err.c_str() : g_group_error.c_str(); }
extern "C" size_t fa_group_size(const fa_group* g) { return g ? g->m.size() : 0; }
extern "C" int fa_group_transport(const fa_group* g) { return g ? g->transport : FA_ERR_ARG; }

// ---- sketches: every member's merged view = the sum over the members -------------------------------------------------------
// FA_GROUP_RCCL: one ncclAllReduce per member and sketch between ncclGroupStart / ncclGroupEnd.
// FA_GROUP_PEER: reduce-scatter + all-gather by peer copies - member r owns slice r of the sketch: it pulls that slice of every
// other member's sketch into its exchange buffer (n - 1 copies of words / n, one per xGMI link), sums them with its own slice
// (group_sum_kernel, plain coalesced loads and stores), and pushes the summed slice into every member's merged view.
// Out of place like fa_merge_allreduce: the members' own sketches are not touched, repeating the call recomputes the views.
static int group_allreduce(fa_group* g) {
    const size_t n = g->m.size();
    fa_ctx* c0 = g->m[0];
    if (!c0->cms_src && !c0->cms_dst) return gfail(g, FA_ERR_ARG, "fa_group_allreduce_sketches: no sketch key set enabled");
    int rc = group_each(g, "settle", [&](size_t i) {
        int r = settle(g->m[i]);  // (folds the sketch copies into copy 0)
        if (r) return r;
        g->m[i]->merged_valid = false;
        return ensure_merged_view(g->m[i]);
    });
    if (rc) return rc;
    const size_t words = c0->cms_words;
    if (g->transport == FA_GROUP_RCCL) {
        const RcclApi* api = rccl_api();
        if (api->GroupStart() != 0) return gfail(g, FA_ERR_HIP, "ncclGroupStart failed");
        int bad = -1;
        for (size_t i = 0; i < n && bad < 0; i++) {
            (void)hipSetDevice(g->m[i]->cfg.device);
            if (allreduce_enqueue(g->m[i], api, g->comms[i])) bad = (int)i;
        }
        // (the group is ALWAYS closed and every member's stream drained before the call returns: a member that failed inside
        // ncclGroupStart / End leaves the other members' all-reduces enqueued - returning with them in flight would let the
        // caller reuse or destroy buffers a collective still writes, and on eight devices an unmatched collective is a hang that
        // the NEXT call would meet)
        const bool end_failed = api->GroupEnd() != 0;
        const int src = group_sync(g, "sketch all-reduce");
        if (bad >= 0) return gfail_member(g, (size_t)bad, FA_ERR_HIP, "sketch all-reduce");
        if (end_failed) return gfail(g, FA_ERR_HIP, "ncclGroupEnd failed");
        if (src) return src;
    } else if (n == 1) {
        for (int d = 0; d < 2; d++) {
            unsigned long long *own = d ? c0->cms_dst : c0->cms_src, *mv = d ? c0->cms_dst_m : c0->cms_src_m;
            if (own && group_copy(g, 0, mv, 0, own, words * 8) != hipSuccess) return gfail(g, FA_ERR_HIP, "sketch copy failed");
        }
        rc = group_sync(g, "sketch all-reduce");
        if (rc) return rc;
    } else {
        const size_t slice = sketch_slice_words(words, n);
        for (size_t r = 0; r < n; r++) {
            rc = group_recv(g, r, (n - 1) * slice * 8);
            if (rc) return gfail_member(g, r, rc, "sketch all-reduce");
        }
        for (int d = 0; d < 2; d++) {
            if (!(d ? c0->cms_dst : c0->cms_src)) continue;
            auto own = [&](size_t i) -> unsigned long long* { return d ? g->m[i]->cms_dst : g->m[i]->cms_src; };
            auto mv = [&](size_t i) -> unsigned long long* { return d ? g->m[i]->cms_dst_m : g->m[i]->cms_src_m; };
            for (size_t r = 0; r < n; r++) {  // reduce-scatter: member r sums slice r
                const size_t lo = std::min(words, r * slice), w = std::min(words, lo + slice) - lo;
                if (!w) continue;
                size_t q = 0;
                for (size_t p = 0; p < n; p++)
                    if (p != r && group_copy(g, r, (unsigned long long*)g->m[r]->xch_buf + (q++) * slice, p, own(p) + lo, w * 8) != hipSuccess)
                        return gfail(g, FA_ERR_HIP, "sketch slice copy failed");
                (void)hipSetDevice(g->m[r]->cfg.device);
                hipLaunchKernelGGL(group_sum_kernel, dim3((unsigned)std::min<size_t>(1024, (w / 2 + 255) / 256 + 1)), dim3(256), 0, g->m[r]->stream,
                                   (const unsigned long long*)(own(r) + lo), (const unsigned long long*)g->m[r]->xch_buf, (uint32_t)(n - 1), slice, w, mv(r) + lo);
                if (hipGetLastError() != hipSuccess) return gfail(g, FA_ERR_HIP, "group_sum_kernel launch failed");
            }
            rc = group_sync(g, "sketch reduce-scatter");
            if (rc) return rc;
            for (size_t r = 0; r < n; r++) {  // all-gather: member r pulls every summed slice it does not own
                for (size_t p = 0; p < n; p++) {
                    const size_t lo = std::min(words, p * slice), w = std::min(words, lo + slice) - lo;
                    if (p != r && w && group_copy(g, r, mv(r) + lo, p, mv(p) + lo, w * 8) != hipSuccess) return gfail(g, FA_ERR_HIP, "sketch slice copy failed");
                }
            }
            rc = group_sync(g, "sketch all-gather");
            if (rc) return rc;
        }
    }
    for (fa_ctx* c : g->m) c->merged_valid = true;
    return FA_OK;
}
extern "C" int fa_group_allreduce_sketches(fa_group* g) {
    if (!g) return FA_ERR_ARG;
    int rc = group_sticky(g);
    return rc ? rc : group_allreduce(g);
}

// ---- rows ------------------------------------------------------------------------------------------------------------------
// Every read is three steps: the members leave rows in their HBM (fa_rows_device; group_shares), an exchange - a gather on one
// root (group_gather_merge) or a hash-partitioned all-to-all (inside group_shares) -, and the receiver merges and fetches
// (group_emit; a partitioned read fetches every share through its own member).  The result is what a single ctx that had
// ingested every partition returns (sum is a commutative monoid; SummingMergeTree collapse, create.sh:70-90).
// FA_VERBOSE: wall time of a close's steps (every step ends with its members synchronised)
struct StepClock {
    bool on = getenv("FA_VERBOSE") != nullptr;
    double t = ReadClock::now();
    std::string head, line;  // head: which call, set by the caller when `on`
    void mark(const char* what) {
        if (!on) return;
        const double u = ReadClock::now();
        char b[64];
        snprintf(b, sizeof b, " %s %.2f", what, u - t);
        line += b;
        t = u;
    }
    void done(size_t rows) const {
        if (on) fprintf(stderr, "[flowagg group] %s %zu rows out; ms:%s\n", head.c_str(), rows, line.c_str());
    }
};
static void mark(StepClock* clk, const char* what) {
    if (clk) clk->mark(what);
}

// where member i's rows come from: fa_rows_device of the read's (kind, timeslot) unless a caller says otherwise
typedef std::function<int(size_t i, const void** d_rows, size_t* n)> GroupRowsSource;
struct RootRows {  // m rows at d, in member `root`'s HBM
    size_t root = 0, m = 0;
    const void* d = nullptr;
};
// rows[p] / cnt[p] in member p's HBM -> peer copies into ONE member's exchange buffer -> fa_rows_merge_device there, cut after k
// rows (0: all).  The root rotates, one step per call that gathers: a group of one has nothing to gather (its rows, cut, are the
// result), and neither have members without a single row (m = 0).  (A root's exchange buffer may have held the input of its own
// share's merge: dead, that result sits in the merge's buffers.)
static int group_gather_merge(fa_group* g, int kind, const std::vector<const void*>& rows, const std::vector<size_t>& cnt, size_t k, StepClock* clk, RootRows& res) {
    const size_t n = g->m.size(), rb = row_bytes_of(kind);
    size_t total = 0;
    for (size_t p = 0; p < n; p++) total += cnt[p];
    res = RootRows();
    if (n == 1) res.d = rows[0], res.m = k && total > k ? k : total;
    if (n == 1 || !total) return FA_OK;
    const size_t root = res.root = g->next_root++ % n;
    fa_ctx* c = g->m[root];
    int rc = group_recv(g, root, total * rb);
    if (rc) return gfail_member(g, root, rc, "rows");
    size_t at = 0;
    for (size_t p = 0; p < n; p++) {
        if (group_copy(g, root, (uint8_t*)c->xch_buf + at * rb, p, rows[p], cnt[p] * rb) != hipSuccess) return gfail(g, FA_ERR_HIP, "group_gather_merge: copy failed");
        at += cnt[p];
    }
    rc = member_sync(g, root, "group_gather_merge");
    if (rc) return rc;
    mark(clk, "gather");
    rc = fa_rows_merge_device(c, kind, c->xch_buf, total, k, &res.d, &res.m);
    if (rc) return gfail_member(g, root, rc, "merge");
    mark(clk, "merge of the shares");
    return FA_OK;
}
// -> the caller's buffer (FA_ERR_CAPACITY: *n_out says what is needed, nothing was fetched); a clocked read's line ends here
static int group_emit(fa_group* g, int kind, const RootRows& res, void* out, size_t cap, size_t* n_out, StepClock* clk) {
    *n_out = res.m;
    if (res.m > cap) return gfail(g, FA_ERR_CAPACITY, "output buffer too small");
    const int rc = fa_rows_fetch(g->m[res.root], kind, res.d, res.m, out, cap);
    mark(clk, "fetch");
    if (clk) clk->done(res.m);
    return rc ? gfail_member(g, res.root, rc, "fetch") : FA_OK;
}
// gathered (small sets): every member's own result (collected, sub-buckets folded, sorted, cut at k_local) -> one root -> the
// caller's buffer.  An empty result returns with *n_out = 0 and no fetch - unless the read is clocked (the talkers of a group of
// one), whose line has always reported the fetch of no rows too.
static int group_rows_merged(fa_group* g, int kind, uint32_t timeslot, size_t k_local, size_t k, void* out, size_t cap, size_t* n_out, StepClock* clk = nullptr,
                             const GroupRowsSource& rows_of = nullptr) {
    const size_t n = g->m.size();
    if (!row_bytes_of(kind)) return gfail(g, FA_ERR_ARG, "unknown row kind");
    *n_out = 0;
    std::vector<const void*> ptr(n, nullptr);
    std::vector<size_t> cnt(n, 0);
    int rc = group_each(g, "rows", [&](size_t i) { return rows_of ? rows_of(i, &ptr[i], &cnt[i]) : fa_rows_device(g->m[i], kind, timeslot, k_local, &ptr[i], &cnt[i]); });
    if (rc) return rc;
    mark(clk, "rows");
    RootRows res;
    rc = group_gather_merge(g, kind, ptr, cnt, k, clk, res);
    if (rc || (!res.m && !clk)) return rc;
    return group_emit(g, kind, res, out, cap, n_out, clk);
}
static int group_drop(fa_group* g, int kind, uint32_t timeslot) {
    return group_each(g, "drop", [&](size_t i) { return fa_drop_window(g->m[i], kind, timeslot); });
}
static int group_args(fa_group* g, const void* out, size_t cap, const size_t* n_out) {
    if (!g || !n_out || (!out && cap)) return FA_ERR_ARG;
    return group_sticky(g);
}
// the kinds a close removes a window of
static int group_windowed(fa_group* g, int kind, const char* who) {
    return kind == RK_5M || kind == RK_APP ? FA_OK : gfail(g, FA_ERR_ARG, std::string(who) + ": not a windowed row kind");
}

extern "C" int fa_group_read_window(fa_group* g, int kind, uint32_t timeslot, size_t k, void* out, size_t cap, size_t* n_out) {
    if (is_talker_kind(kind)) return fa_group_top_talkers(g, kind == RK_TALKERS_DST, k, (fa_talker_row*)out, cap, n_out);  // (no timeslot: the tables span the stream)
    int rc = group_args(g, out, cap, n_out);
    if (rc) return rc;
    if (kind == RK_TOPK_SRC || kind == RK_TOPK_DST) {
        // exact with respect to the merged sketch: every member ranks ITS distinct addresses by the merged estimate and hands
        // over its first k rows - a key of the global top k ranks at least as high among the keys of any member that saw it
        if (!k) return gfail(g, FA_ERR_ARG, "top-k rows need k > 0");
        rc = group_allreduce(g);
        if (rc) return rc;
        return group_rows_merged(g, kind, 0, k, k, out, cap, n_out);
    }
    // (ports: every member's rows travel - a port just below the cut everywhere can lead overall)
    return group_rows_merged(g, kind, timeslot, 0, k, out, cap, n_out);
}
extern "C" int fa_group_close_window(fa_group* g, int kind, uint32_t timeslot, void* out, size_t cap, size_t* n_out) {
    int rc = group_args(g, out, cap, n_out);
    if (!rc) rc = group_windowed(g, kind, "fa_group_close_window");
    if (!rc) rc = group_rows_merged(g, kind, timeslot, 0, 0, out, cap, n_out);
    return rc ? rc : group_drop(g, kind, timeslot);  // (FA_ERR_CAPACITY included: nothing is removed before the rows have left)
}
extern "C" int fa_group_topk(fa_group* g, uint32_t key_set, size_t k, fa_topk_row* out, size_t cap, size_t* n_out) {
    if (key_set != FA_KEYS_SRCADDR_CMS && key_set != FA_KEYS_DSTADDR_CMS) return g ? gfail(g, FA_ERR_ARG, "fa_group_topk: key set") : FA_ERR_ARG;
    if (g && n_out && k == 0) {
        *n_out = 0;
        return FA_OK;
    }
    return fa_group_read_window(g, key_set == FA_KEYS_SRCADDR_CMS ? RK_TOPK_SRC : RK_TOPK_DST, 0, k, out, cap, n_out);
}

// ---- rows: hash-partitioned (large sets) -----------------------------------------------------------------------------------
// (SrcAddr,DstPort,Proto): a window of BASELINE config 5 is 16.6 M rows x 56 B PER MEMBER - gathered, one GPU would receive
// and sort all of it.  Every member cuts its rows by owner (fa_rows_partition_device, owner = hash(key) scaled to the group),
// member r pulls group r of every member (one peer copy per pair: every xGMI link carries 1 / n of a member's rows), merges
// its share - 1 / n of the keys, complete - and the shares leave through the members' own PCIe links in parallel, back to
// back in the caller's buffer: share 0 first, each in the kind's emit order, a key in exactly one share.
// The shares: member r's merged rows (res[r], m[r] of them, in r's HBM) of the keys it owns, cut after k rows (0: all).
// rows_of: where member i's rows come from (all of them, uncut) - fa_rows_device of (kind, timeslot) unless the caller says otherwise.
static int group_shares(fa_group* g, int kind, uint32_t timeslot, size_t k, StepClock& clk, std::vector<const void*>& res, std::vector<size_t>& m,
                        const GroupRowsSource& rows_of = nullptr) {
    const size_t n = g->m.size(), rb = row_bytes_of(kind);
    std::vector<const void*> part(n, nullptr);
    std::vector<size_t> counts(n * n, 0);  // counts[p * n + r]: rows member p holds for member r
    int rc = group_each(g, "rows", [&](size_t i) {
        const void* d = nullptr;
        size_t m = 0;
        int r = rows_of ? rows_of(i, &d, &m) : fa_rows_device(g->m[i], kind, timeslot, 0, &d, &m);
        if (r) return r;
        return fa_rows_partition_device(g->m[i], kind, d, m, (uint32_t)n, &part[i], &counts[i * n]);
    });
    if (rc) return rc;
    clk.mark("rows + partition");
    std::vector<size_t> got(n, 0);
    for (size_t r = 0; r < n; r++) {
        for (size_t p = 0; p < n; p++) got[r] += counts[p * n + r];
        rc = group_recv(g, r, got[r] * rb);
        if (rc) return gfail_member(g, r, rc, "rows");
    }
    clk.mark("exchange buffers");
    for (size_t r = 0; r < n; r++) {
        size_t at = 0;
        for (size_t p = 0; p < n; p++) {
            size_t from = 0;
            for (size_t q = 0; q < r; q++) from += counts[p * n + q];
            if (group_copy(g, r, (uint8_t*)g->m[r]->xch_buf + at * rb, p, (const uint8_t*)part[p] + from * rb, counts[p * n + r] * rb) != hipSuccess)
                return gfail(g, FA_ERR_HIP, "row exchange copy failed");
            at += counts[p * n + r];
        }
    }
    rc = group_sync(g, "row exchange");
    if (rc) return rc;
    clk.mark("exchange");
    res.assign(n, nullptr);
    m.assign(n, 0);
    rc = group_each(g, "merge", [&](size_t r) { return got[r] ? fa_rows_merge_device(g->m[r], kind, g->m[r]->xch_buf, got[r], k, &res[r], &m[r]) : FA_OK; });
    clk.mark("merge");
    return rc;
}
static int group_rows_partitioned(fa_group* g, int kind, uint32_t timeslot, void* out, size_t cap, size_t* share_rows, size_t* n_out) {
    const size_t n = g->m.size(), rb = row_bytes_of(kind);
    if (!rb) return gfail(g, FA_ERR_ARG, "unknown row kind");
    *n_out = 0;
    StepClock clk;
    if (clk.on) clk.head = "partitioned read of kind " + std::to_string(kind) + ", " + std::to_string(n) + " members,";
    std::vector<const void*> res;
    std::vector<size_t> m;
    int rc = group_shares(g, kind, timeslot, 0, clk, res, m);
    if (rc) return rc;
    size_t total = 0;
    std::vector<size_t> at(n, 0);
    for (size_t r = 0; r < n; r++) {
        at[r] = total;
        total += m[r];
        if (share_rows) share_rows[r] = m[r];
    }
    *n_out = total;
    if (total > cap) return gfail(g, FA_ERR_CAPACITY, "output buffer too small");
    rc = group_each(g, "fetch", [&](size_t r) { return m[r] ? fa_rows_fetch(g->m[r], kind, res[r], m[r], (uint8_t*)out + at[r] * rb, m[r]) : FA_OK; });
    clk.mark("fetch");
    clk.done(total);
    return rc;
}
extern "C" int fa_group_read_window_partitioned(fa_group* g, int kind, uint32_t timeslot, void* out, size_t cap, size_t* share_rows, size_t* n_out) {
    int rc = group_args(g, out, cap, n_out);
    return rc ? rc : group_rows_partitioned(g, kind, timeslot, out, cap, share_rows, n_out);
}
extern "C" int fa_group_close_window_partitioned(fa_group* g, int kind, uint32_t timeslot, void* out, size_t cap, size_t* share_rows, size_t* n_out) {
    int rc = group_args(g, out, cap, n_out);
    if (!rc) rc = group_windowed(g, kind, "fa_group_close_window_partitioned");
    if (!rc) rc = group_rows_partitioned(g, kind, timeslot, out, cap, share_rows, n_out);
    return rc ? rc : group_drop(g, kind, timeslot);
}

// ---- exact top talkers over the members' tables -------------------------------------------------------------------------------
// An exact top k over partitions cannot be built from each partition's top k (a key that is tenth everywhere can lead overall):
// every member's WHOLE table leaves as rows, hash-partitioned.  Stage 1 is group_shares with the merge cut at k: member r holds
// the first k rows of the keys it owns - each key in exactly one share, with its complete sums, so under the total order (weight
// DESC, key bytes, etype) the global first k are among the shares' first k.  Stage 2 gathers those n x k rows on one root and
// merges them with the same cut.  The result is fa_top_talkers of ONE ctx that folded every partition, byte for byte.
// range (fa_group_top_talkers_range): every member's rows come from fa_talkers_range_rows_device instead of fa_rows_device - the
// members are bucketed, with one bucket_secs.
static int group_top_talkers(fa_group* g, int dst, const uint32_t* range, size_t k, fa_talker_row* out, size_t cap, size_t* n_out) {
    int rc = group_args(g, out, cap, n_out);
    if (rc) return rc;
    if (dst != 0 && dst != 1) return gfail(g, FA_ERR_ARG, "fa_group_top_talkers: bad argument");
    const int kind = dst ? RK_TALKERS_DST : RK_TALKERS_SRC;
    const size_t n = g->m.size();
    *n_out = 0;
    for (size_t i = 0; i < n; i++) {  // (before anything is collected or exchanged; gfail_member names member i in every member's error)
        if (!g->m[i]->talk) {
            rc = gfail_member(g, i, kind_enabled(g->m[i], kind), "top talkers");
            g->m[i]->err = "group: " + g->err;
            return rc;
        }
        if (!range) continue;
        const char* why = !talk_bucket_secs(g->m[i]) ? TALK_NOT_BUCKETED : talk_bucket_secs(g->m[i]) != talk_bucket_secs(g->m[0]) ? "bucket_secs differs from member 0's" : nullptr;
        if (!why) continue;
        rc = gfail_member(g, i, fail(g->m[i], why == TALK_NOT_BUCKETED ? FA_ERR_UNSUPPORTED : FA_ERR_ARG, why), "top talkers of a range");
        g->m[i]->err = "group: " + g->err;
        return rc;
    }
    StepClock clk;
    if (clk.on) clk.head = std::string("top talkers (") + (dst ? "DstAddr" : "SrcAddr") + (range ? ", ranged" : "") + "), " + std::to_string(n) + " members, k " + std::to_string(k) + ",";
    GroupRowsSource all_rows, first_k;  // (empty: fa_rows_device)
    if (range) {
        all_rows = [=](size_t i, const void** d, size_t* m) { return fa_talkers_range_rows_device(g->m[i], dst, range[0], range[1], 0, d, m); };
        first_k = [=](size_t i, const void** d, size_t* m) { return fa_talkers_range_rows_device(g->m[i], dst, range[0], range[1], k, d, m); };
    }
    if (n == 1) return group_rows_merged(g, kind, 0, k, k, out, cap, n_out, &clk, first_k);  // (the one member's first k rows are the result)
    std::vector<const void*> res;
    std::vector<size_t> cnt;
    RootRows top;
    rc = group_shares(g, kind, 0, k, clk, res, cnt, all_rows);
    if (!rc) rc = group_gather_merge(g, kind, res, cnt, k, &clk, top);
    if (rc || !top.m) return rc;
    return group_emit(g, kind, top, out, cap, n_out, &clk);
}
extern "C" int fa_group_top_talkers(fa_group* g, int dst, size_t k, fa_talker_row* out, size_t cap, size_t* n_out) {
    return group_top_talkers(g, dst, nullptr, k, out, cap, n_out);
}
// fa_top_talkers_range of ONE ctx that folded every partition.  Checked before anything is exchanged: a member that is not
// bucketed -> FA_ERR_UNSUPPORTED, members with different bucket_secs -> FA_ERR_ARG (the member is named in fa_group_last_error
// and in every member's last error); the range itself is checked by the members, which share one grid by then.
extern "C" int fa_group_top_talkers_range(fa_group* g, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_talker_row* out, size_t cap, size_t* n_out) {
    const uint32_t range[2] = {t_lo, t_hi};
    return group_top_talkers(g, dst, range, k, out, cap, n_out);
}

// ---- exact top ports of a range over the members' bucketed port tables -----------------------------------------------------------
// fa_top_ports_range of ONE ctx that folded every partition.  Port rows are a small set (at most 65536 rows per member plus its
// large ports), so nothing is partitioned: every member's WHOLE ranged result (fa_ports_range_rows_device, k = 0 - a port that
// no member ranks first can lead overall) is gathered on one root and merged there, cut at k.  Checked before anything is
// collected or exchanged: a member that is not enabled -> FA_ERR_UNSUPPORTED, members with different bucket_secs -> FA_ERR_ARG.
extern "C" int fa_group_top_ports_range(fa_group* g, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_port_row* out, size_t cap, size_t* n_out) {
    int rc = group_args(g, out, cap, n_out);
    if (rc) return rc;
    if (dst != 0 && dst != 1) return gfail(g, FA_ERR_ARG, "fa_group_top_ports_range: bad argument");
    *n_out = 0;
    for (size_t i = 0; i < g->m.size(); i++) {  // (gfail_member names member i in every member's error)
        const uint32_t bs = port_bucket_secs(g->m[i]);
        if (bs && bs == port_bucket_secs(g->m[0])) continue;
        rc = gfail_member(g, i, bs ? fail(g->m[i], FA_ERR_ARG, "bucket_secs differs from member 0's") : fail(g->m[i], FA_ERR_UNSUPPORTED, PORT_OFF), "top ports of a range");
        g->m[i]->err = "group: " + g->err;
        return rc;
    }
    const GroupRowsSource all_rows = [=](size_t i, const void** d, size_t* m) { return fa_ports_range_rows_device(g->m[i], dst, t_lo, t_hi, 0, d, m); };
    return group_rows_merged(g, dst ? RK_PORT_DST : RK_PORT_SRC, 0, 0, k, out, cap, n_out, nullptr, all_rows);
}

// ---- grouped queries over the whole topic ---------------------------------------------------------------------------------------
// The members stay the caller's: fa_group_raw_query_pending runs fa_raw_query_pending on every member (KEEP passed through, so a
// caller adds stored files member by member with fa_raw_query first), and fa_group_raw_query_rows merges WHAT THE MEMBERS HOLD - it
// reads their results (fa_raw_query_rows_device, k = 0) and changes none.  An exact first k cannot be built from the members' first
// k, so the address kinds go the top talkers' two stages (group_shares with the merge cut at k, group_gather_merge with the same
// cut: the argument above group_top_talkers, with the total order of fa_raw_query_rows) and the scalar kinds - small sets - are
// gathered whole on one root (fa_group_top_ports_range's way).  Rows of ONE kind meet in a call: the row kinds' duty.
static uint32_t query_groups_held(const fa_ctx* c);  // raw_query_host.inc
static int group_query_refuse(fa_group* g, size_t i, int code, const char* what, const std::string& why) {
    const int rc = gfail_member(g, i, fail(g->m[i], code, why.c_str()), what);
    g->m[i]->err = "group: " + g->err;
    return rc;
}
extern "C" int fa_group_raw_query_pending(fa_group* g, const fa_raw_query_t* q) {
    if (!g) return FA_ERR_ARG;
    if (!q) return gfail(g, FA_ERR_ARG, "fa_group_raw_query_pending: null argument");
    int rc = group_sticky(g);
    if (rc) return rc;
    for (size_t i = 0; i < g->m.size(); i++)  // (before any member runs)
        if (!g->m[i]->raw) return group_query_refuse(g, i, FA_ERR_UNSUPPORTED, "query of the pending parts", "flows_raw parts are not enabled on this ctx (fa_raw_enable)");
    const fa_raw_query_t qa = *q;
    return group_each(g, "query of the pending parts", [&](size_t i) { return fa_raw_query_pending(g->m[i], &qa); });
}
extern "C" int fa_group_raw_query_reset(fa_group* g) {
    if (!g) return FA_ERR_ARG;
    return group_each(g, "query reset", [&](size_t i) { return fa_raw_query_reset(g->m[i]); });
}
extern "C" int fa_group_raw_query_rows(fa_group* g, uint32_t group, int order, size_t k, fa_query_row* out, size_t cap, size_t* n_out) {
    int rc = group_args(g, out, cap, n_out);
    if (rc) return rc;
    *n_out = 0;
    if (!group || (group & (group - 1)) || (group & ~FA_RAW_G_ALL)) return gfail(g, FA_ERR_ARG, "fa_group_raw_query_rows: group is exactly one FA_RAW_G_* bit");
    if (order != FA_RAW_O_WEIGHT && order != FA_RAW_O_KEY) return gfail(g, FA_ERR_ARG, "fa_group_raw_query_rows: order is FA_RAW_O_WEIGHT or FA_RAW_O_KEY");
    const size_t n = g->m.size();
    for (size_t i = 0; i < n; i++) {  // (before anything is collected or exchanged)
        const uint32_t held = query_groups_held(g->m[i]);
        if (!held) return group_query_refuse(g, i, FA_ERR_ARG, "query rows", "the ctx holds no query result");
        if (!(held & group)) return group_query_refuse(g, i, FA_ERR_ARG, "query rows", "group is not among the groups of the result the ctx holds");
    }
    const int kind = order == FA_RAW_O_WEIGHT ? RK_QUERY_WEIGHT : RK_QUERY_KEY;
    const bool addr = group & (FA_RAW_G_SRC_ADDR | FA_RAW_G_DST_ADDR);
    StepClock clk;
    if (clk.on) clk.head = "query rows (group bit " + std::to_string(group) + ", order " + std::to_string(order) + "), " + std::to_string(n) + " members, k " + std::to_string(k) + ",";
    const GroupRowsSource all_rows = [=](size_t i, const void** d, size_t* m) { return fa_raw_query_rows_device(g->m[i], group, order, 0, d, m); };
    const GroupRowsSource first_k = [=](size_t i, const void** d, size_t* m) { return fa_raw_query_rows_device(g->m[i], group, order, k, d, m); };
    std::vector<const void*> res(n, nullptr);
    std::vector<size_t> cnt(n, 0);
    RootRows top;
    if (n == 1 || !addr) {  // a group of one: its member's first k rows are the result; a scalar kind: every member's whole set on one root
        const GroupRowsSource& src = n == 1 ? first_k : all_rows;
        rc = group_each(g, "rows", [&](size_t i) { return src(i, &res[i], &cnt[i]); });
        clk.mark("rows");
    } else {
        rc = group_shares(g, kind, 0, k, clk, res, cnt, all_rows);
    }
    if (!rc) rc = group_gather_merge(g, kind, res, cnt, k, &clk, top);
    if (rc || !top.m) return rc;
    return group_emit(g, kind, top, out, cap, n_out, &clk);
}

// ---- what a consumer asks before a flush, and at exit ----------------------------------------------------------------------
extern "C" int fa_group_open_timeslots(fa_group* g, uint32_t* out, size_t cap, size_t* n_out) {
    int rc = group_args(g, out, cap, n_out);
    if (rc) return rc;
    const size_t n = g->m.size();
    std::vector<std::vector<uint32_t>> ts(n);
    rc = group_each(g, "open timeslots", [&](size_t i) {
        ts[i].resize(256);
        size_t k = 0;
        int r = fa_open_timeslots(g->m[i], ts[i].data(), ts[i].size(), &k);
        if (r == FA_ERR_CAPACITY) {
            ts[i].resize(k);
            r = fa_open_timeslots(g->m[i], ts[i].data(), ts[i].size(), &k);
        }
        ts[i].resize(r ? 0 : k);
        return r;
    });
    if (rc) return rc;
    std::vector<uint32_t> all;
    for (auto& v : ts) all.insert(all.end(), v.begin(), v.end());
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    *n_out = all.size();
    if (all.size() > cap) return gfail(g, FA_ERR_CAPACITY, "output buffer too small");
    if (!all.empty()) memcpy(out, all.data(), all.size() * sizeof(uint32_t));
    return FA_OK;
}
extern "C" int fa_group_stats(fa_group* g, fa_stats_t* out) {
    if (!g || !out) return FA_ERR_ARG;
    const size_t n = g->m.size();
    std::vector<fa_stats_t> st(n);
    int rc = group_each(g, "stats", [&](size_t i) { return fa_stats(g->m[i], &st[i]); });
    if (rc) return rc;
    // every member of fa_stats_t is a uint64 counter or gauge: the group's figure is the sum (kernel_ns: the slowest member's
    // last launch; wide_log_mode: members in log mode)
    static_assert(sizeof(fa_stats_t) % sizeof(uint64_t) == 0, "fa_stats_t is an array of uint64");
    memset(out, 0, sizeof *out);
    for (size_t i = 0; i < n; i++)
        for (size_t w = 0; w < sizeof(fa_stats_t) / sizeof(uint64_t); w++) ((uint64_t*)out)[w] += ((const uint64_t*)&st[i])[w];
    out->kernel_ns = out->topk_theta[0] = out->topk_theta[1] = 0;  // (not additive: the slowest member's last launch; the highest threshold)
    for (size_t i = 0; i < n; i++) {
        out->kernel_ns = std::max(out->kernel_ns, st[i].kernel_ns);
        for (int d = 0; d < 2; d++) out->topk_theta[d] = std::max(out->topk_theta[d], st[i].topk_theta[d]);
    }
    return FA_OK;
}
