// ports.cuh - exact GROUP BY SrcPort / DstPort for a time range: bucketed port tables (gfx950).
//
// The two port panels (viz-ch.json:358 SrcPort, :604 DstPort) read "... WHERE $timeFilter GROUP BY port".  The group key here is
// (bucket index, port): bucket index = t32 / bucket_secs with t32 = (uint32_t)TimeFlowStart (the DateTime narrowing of
// create.sh:40, the rule of the minute series and of the talker buckets); port = the whole UInt32 column value - 65536 and above
// are keys like any other.  value = sum(Bytes * SamplingRate) mod 2^64 and count(); a group of weight 0 is still a row.
//
// State: two open-addressed tables of their own (SrcPort, DstPort) - never the ctx's wide table or its dense port histograms.
// Slot = 32 bytes: two key words + weight + count.  w0 = bit 63 | bucket index, w1 = bit 63 | port: both words are never 0, so 0
// is EMPTY for each, and the keys (0, 0) and (0xFFFFFFFF, 0xFFFFFFFF) are words like any other.  A slot is claimed word by word
// with 64-bit CAS in the order w0, w1 (the argument of wide.cuh and talkers.cuh: a word is written once, a contender that loses
// a word leaves the slot, so the lane that wins w1 matched w0).  Probing is linear over the WHOLE table and has no limit: the
// host keeps the load at or below 1/2 before every launch (ports_host.inc), so a probe sequence ends and no update is lost.
//
// port_fold_kernel, the hot part: one lane per record of the decoded columns (six of them, 33 bytes per record), both tables in
// one pass, one 32-bit division per record for the bucket index.  Real port streams are far more skewed than address streams - a
// handful of service ports carries most records - so a workgroup-private LDS cache of (bucket, port) -> (weight, count) per
// direction is part of the design, not an option: without it millions of same-key atomics land on a few L2 lines.  An entry's
// key is the slot's two words, claimed in order with LDS CAS; a lane that loses a word tries the next entry (PORT_LDS_PROBES of
// them), then goes straight to the global table.  The cache is cleared at the start of the launch and flushed at its end, one
// global upsert per occupied entry.
//
// Invariants (those of talkers.cuh):
//   - an LDS entry or a global slot only ever holds ONE key (write-once words, claimed in order);
//   - every (record, direction) update is applied exactly once: to the cache (and from there once by the flush) or to the
//     global table, never both;
//   - u64 wrap-around adds commute: any order of updates, chunks, growths and rebuilds gives bit-identical sums;
//   - creations are summed per wave, then per workgroup, before they touch the device counters (one word for every creation of
//     the chip serialises: the talkers measured 0.99 -> 0.31 ns per record for exactly this).
//
// Sizes - chosen by the reasoning below, BEFORE anything was measured.  tools/port_buckets_run.py has since measured this ONE
// geometry on one stream (uniform 16-bit ports: 0.24 ns per record); no other block size, cache size or
// workgroup count has been tried, so none of them is known to be the best:
//   - 512 threads per workgroup, two workgroups per CU (FA_PORT_WGPC): 16 waves per CU behind the latency of the random global
//     upserts, the geometry the talker fold was measured with.  A record is 33 bytes and a lane holds one key per direction,
//     so registers do not limit the residency; the 32-waves-per-CU cap would allow four workgroups, but every workgroup flushes
//     its own copy of the hot keys, so more workgroups per chunk mean more flush upserts for the same records.
//   - 512 cache entries per direction x 32 bytes = 32 KiB of LDS per workgroup, 64 KiB of the CU's 160 KiB for two workgroups.
//     What the cache has to hold is the HOT set of one workgroup's share of a chunk (2048 records of a 2^20 chunk on 256 CUs):
//     service ports times the one or two buckets a chunk of a time-ordered stream touches - tens of keys.  Ephemeral client
//     ports do not repeat inside a share; an entry they take costs one flush upsert in place of one direct upsert, nothing
//     more, so a larger cache only holds more keys seen once.  A launch flushes at most 2 x 512 entries per workgroup.
//   - PORT_LDS_PROBES = 4: a hot key claims its entry the first time it is seen and is found at probe 0..3 ever after; a cold
//     key that finds four foreign entries goes global after four LDS reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "table.cuh"

namespace fa {

struct PKey {
    unsigned long long w[2];
};
constexpr unsigned long long PKEY_B63 = 1ull << 63;
__host__ __device__ __forceinline__ void pkey_pack(uint32_t bucket_index, uint32_t port, PKey& k) {
    k.w[0] = PKEY_B63 | bucket_index;
    k.w[1] = PKEY_B63 | port;
}
__host__ __device__ __forceinline__ uint32_t pkey_bucket(const unsigned long long w[2]) { return (uint32_t)w[0]; }
__host__ __device__ __forceinline__ uint32_t pkey_port(const unsigned long long w[2]) { return (uint32_t)w[1]; }
__host__ __device__ __forceinline__ bool pkey_empty(unsigned long long word) { return word == 0ull; }
__host__ __device__ __forceinline__ uint32_t pkey_hash(const PKey& k) { return key_hash(k.w[0], k.w[1]); }
// the bucket index of a record: the DateTime narrowing, then one 32-bit division
__host__ __device__ __forceinline__ uint32_t port_bucket_index(uint64_t time_flow_start, uint32_t bucket_secs) { return (uint32_t)time_flow_start / bucket_secs; }

struct __attribute__((aligned(32))) PSlot {
    unsigned long long w[2];
    unsigned long long weight, count;
};
static_assert(sizeof(PSlot) == 32, "two port slots per 64-byte line");

struct PortCounters {
    unsigned long long used[2];   // occupied slots per direction (summed per wave / workgroup before they are added)
    unsigned long long large[2];  // ... of them, slots whose port is 65536 or above: the room the ranged collector's raw rows need
    unsigned long long folded;    // status == 0 records folded
    unsigned long long absorbed;  // (record, direction) updates that ended in an LDS cache
    unsigned long long lost;      // updates that met a full table, rows the ranged collector had no room for: the host's capacity rule or
                                  // large[] was broken (never on a correct host)
};

constexpr uint32_t PORT_LARGE = 65536;  // ports from here on have no entry in a dense {weight, count} array (== sinks.cuh's PORT_DENSE)

// Adds (w, cnt) to k's slot, claiming one if the key is new.  Stale plain reads (per-XCD L2s are not coherent) can only show
// EMPTY or the final word - never a false match; an EMPTY that is stale is settled by the CAS.
// created / created_large: the lane's counts of the keys it created.
__device__ __forceinline__ void port_upsert(PSlot* tab, uint32_t mask, const PKey& k, uint32_t h, uint64_t w, uint64_t cnt, PortCounters* ctr, uint32_t& created,
                                            uint32_t& created_large) {
    uint32_t i = h & mask;
    // (the bound is the table itself: with the load at or below 1/2 an EMPTY slot is met long before it)
    for (uint32_t probe = 0; probe <= mask; probe++, i = (i + 1u) & mask) {
        PSlot* s = &tab[i];
        const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(&s->w[0]);
        unsigned long long c[2] = {k01.x, k01.y};
        bool mine = true;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            if (!mine) break;
            if (c[j] == 0) {
                c[j] = atomicCAS(&s->w[j], 0ull, k.w[j]);
                if (c[j] == 0) {
                    c[j] = k.w[j];
                    if (j == 1) {  // this lane created the group
                        created++;
                        if (pkey_port(k.w) >= PORT_LARGE) created_large++;
                    }
                }
            }
            mine = c[j] == k.w[j];
        }
        if (mine) {
            if (w) atomicAdd(&s->weight, (unsigned long long)w);
            atomicAdd(&s->count, (unsigned long long)cnt);
            return;
        }
    }
    atomicAdd(&ctr->lost, 1ull);
}

constexpr int PORT_BLOCK = 512;
#ifndef FA_PORT_LDS_ENTRIES
#define FA_PORT_LDS_ENTRIES 512
#endif
constexpr int PORT_LDS_ENTRIES = FA_PORT_LDS_ENTRIES;  // per direction, a power of two
constexpr int PORT_LDS_PROBES = 4;
constexpr int PORT_WG_PER_CU = 2;
static_assert((PORT_LDS_ENTRIES & (PORT_LDS_ENTRIES - 1)) == 0, "the cache is indexed by hash bits");

struct PortLds {
    unsigned long long k0[2][PORT_LDS_ENTRIES], k1[2][PORT_LDS_ENTRIES];
    unsigned long long w[2][PORT_LDS_ENTRIES], c[2][PORT_LDS_ENTRIES];
    unsigned long long absorbed, folded, created[2], large[2];
};

// one key word of an entry: EMPTY is claimed, then it must be ours.  (A plain read that shows a word is final.)
__device__ __forceinline__ bool port_lds_word(unsigned long long* p, unsigned long long want) {
    unsigned long long cur = *p;
    if (cur == 0) {
        cur = atomicCAS(p, 0ull, want);
        if (cur == 0) cur = want;
    }
    return cur == want;
}
// true = absorbed by the workgroup's cache
__device__ __forceinline__ bool port_lds_add(PortLds& L, int d, const PKey& k, uint32_t h, uint64_t w) {
    uint32_t i = (h >> 9) & (PORT_LDS_ENTRIES - 1);
#pragma unroll 1
    for (int probe = 0; probe < PORT_LDS_PROBES; probe++, i = (i + 1u) & (PORT_LDS_ENTRIES - 1)) {
        if (!port_lds_word(&L.k0[d][i], k.w[0])) continue;
        if (!port_lds_word(&L.k1[d][i], k.w[1])) continue;
        if (w) atomicAdd(&L.w[d][i], (unsigned long long)w);
        atomicAdd(&L.c[d][i], 1ull);  // (count even when the weight is 0)
        return true;
    }
    return false;
}

struct PortFoldArgs {
    const uint32_t* src_port;
    const uint32_t* dst_port;
    const uint64_t* bytes;
    const uint64_t* sampling_rate;
    const uint64_t* time_flow_start;
    const uint8_t* status;
    uint32_t n;
    uint32_t bucket_secs;
    PSlot* tab[2];
    uint32_t mask[2];
    PortCounters* ctr;
};

__global__ __launch_bounds__(PORT_BLOCK) void port_fold_kernel(PortFoldArgs a) {
    __shared__ PortLds L;
    for (int i = threadIdx.x; i < 2 * PORT_LDS_ENTRIES; i += PORT_BLOCK) {
        (&L.k0[0][0])[i] = 0;
        (&L.k1[0][0])[i] = 0;
        (&L.w[0][0])[i] = 0;
        (&L.c[0][0])[i] = 0;
    }
    if (threadIdx.x == 0) L.absorbed = L.folded = L.created[0] = L.created[1] = L.large[0] = L.large[1] = 0;
    __syncthreads();
    uint32_t absorbed = 0, folded = 0, created[2] = {0, 0}, large[2] = {0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * PORT_BLOCK + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * PORT_BLOCK) {
        if (a.status[i]) continue;  // malformed: dropped, whatever the other columns hold
        folded++;
        const uint64_t w = a.bytes[i] * a.sampling_rate[i];
        const uint32_t bidx = port_bucket_index(a.time_flow_start[i], a.bucket_secs);
#pragma unroll
        for (int d = 0; d < 2; d++) {
            PKey k;
            pkey_pack(bidx, (d ? a.dst_port : a.src_port)[i], k);
            const uint32_t h = pkey_hash(k);
            if (port_lds_add(L, d, k, h, w)) absorbed++;
            else port_upsert(a.tab[d], a.mask[d], k, h, w, 1, a.ctr, created[d], large[d]);
        }
    }
    const uint64_t wa = wave_sum_u64(absorbed), wf = wave_sum_u64(folded);
    if (__lane_id() == 0) {
        if (wa) atomicAdd(&L.absorbed, (unsigned long long)wa);
        if (wf) atomicAdd(&L.folded, (unsigned long long)wf);
    }
    __syncthreads();
    // flush: every occupied entry is complete by now (the lane that claimed k0 went on to k1, or met it claimed)
    for (int e = threadIdx.x; e < 2 * PORT_LDS_ENTRIES; e += PORT_BLOCK) {
        const int d = e / PORT_LDS_ENTRIES, j = e % PORT_LDS_ENTRIES;
        if (L.k0[d][j] == 0) continue;
        PKey k;
        k.w[0] = L.k0[d][j];
        k.w[1] = L.k1[d][j];
        port_upsert(a.tab[d], a.mask[d], k, pkey_hash(k), L.w[d][j], L.c[d][j], a.ctr, created[d], large[d]);
    }
#pragma unroll
    for (int d = 0; d < 2; d++) {
        const uint64_t wc = wave_sum_u64(created[d]), wl = wave_sum_u64(large[d]);
        if (__lane_id() == 0) {
            if (wc) atomicAdd(&L.created[d], (unsigned long long)wc);
            if (wl) atomicAdd(&L.large[d], (unsigned long long)wl);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one atomic per workgroup and counter
        if (L.absorbed) atomicAdd(&a.ctr->absorbed, L.absorbed);
        if (L.folded) atomicAdd(&a.ctr->folded, L.folded);
#pragma unroll
        for (int d = 0; d < 2; d++) {
            if (L.created[d]) atomicAdd(&a.ctr->used[d], L.created[d]);
            if (L.large[d]) atomicAdd(&a.ctr->large[d], L.large[d]);
        }
    }
}

// Growth: every occupied slot of the old table is inserted again (key, weight, count) - the sums stay exact; used[d] and
// large[d] are counted again (the host zeroes them before the launch).
// floor_index (fa_ports_drop_before; 0 = keep everything): slots of a bucket index below it are left behind.
__global__ __launch_bounds__(256) void port_rehash_kernel(const PSlot* old_tab, uint64_t old_slots, PSlot* tab, uint32_t mask, PortCounters* ctr, int d, uint32_t floor_index) {
    uint32_t created = 0, large = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * blockDim.x) {
        const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(&old_tab[i].w[0]);
        if (k01.x == 0) continue;
        PKey k;
        k.w[0] = k01.x;
        k.w[1] = k01.y;
        if (pkey_bucket(k.w) < floor_index) continue;
        port_upsert(tab, mask, k, pkey_hash(k), old_tab[i].weight, old_tab[i].count, ctr, created, large);
    }
    const uint64_t wc = wave_sum_u64(created), wl = wave_sum_u64(large);
    if (__lane_id() == 0) {
        if (wc) atomicAdd(&ctr->used[d], (unsigned long long)wc);
        if (wl) atomicAdd(&ctr->large[d], (unsigned long long)wl);
    }
}

// ---- read side ---------------------------------------------------------------------------------------------------------
// One public row (include/flowagg.h: fa_port_row; merge.cuh: RowW), 24 bytes.
struct PortRow {
    uint32_t port, pad;
    unsigned long long weight, count;
};
static_assert(sizeof(PortRow) == 24, "fa_port_row");

// The ranged collector.  The slots whose bucket index lies in [index_lo, index_last] (both inclusive) lose their bucket here, not
// in the merge behind the read: a port below PORT_LARGE is added into dense[port] = {weight, count} (zeroed by the host, 1 MiB),
// a port from PORT_LARGE on leaves as a raw row behind *cursor.  So the merge is handed at most 65536 rows (the occupied dense
// entries, port_dense_rows_kernel) plus the large-port rows - never one row per (bucket, port).
// cap = the table's count of large-port slots (PortCounters::large), an upper bound of the raw rows of any range.  *cursor never
// ends above cap - port_dense_rows_kernel appends behind it: a row that finds no room (never, while the count is right) takes its
// place back and is counted in ctr->lost, which the host reads with the cursor.
__global__ __launch_bounds__(256) void port_range_fold_kernel(const PSlot* tab, uint64_t nslots, uint32_t index_lo, uint32_t index_last, ulonglong2* dense, PortRow* raw, uint32_t cap,
                                                              unsigned int* cursor, PortCounters* ctr) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
        const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(&tab[i].w[0]);
        if (k01.x == 0) continue;
        const uint32_t b = (uint32_t)k01.x, port = (uint32_t)k01.y;
        if (b < index_lo || b > index_last) continue;
        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(&tab[i].weight);
        if (port < PORT_LARGE) {
            unsigned long long* e = reinterpret_cast<unsigned long long*>(&dense[port]);
            if (v.x) atomicAdd(e, v.x);
            atomicAdd(e + 1, v.y);
        } else {
            const unsigned int j = atomicAdd(cursor, 1u);
            if (j < cap) {  // (always: cap counts the large-port slots of every bucket)
                raw[j] = PortRow{port, 0u, v.x, v.y};
            } else {
                atomicSub(cursor, 1u);
                atomicAdd(&ctr->lost, 1ull);
            }
        }
    }
}

// fa_ports_buckets, the shape of talker_buckets_kernel.  bits == nullptr: the smallest and largest bucket index of the occupied
// slots into range[0..1], range[2] = a bucket was seen; else one bit per index of [lo, lo + nbits).
__global__ __launch_bounds__(256) void port_buckets_kernel(const PSlot* tab, uint64_t nslots, uint32_t lo, uint32_t nbits, unsigned int* bits, unsigned int* range) {
    uint32_t mn = 0xffffffffu, mx = 0u;
    bool any = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
        const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(&tab[i].w[0]);
        if (k01.y == 0) continue;  // (w1 is the last word claimed: a slot whose w1 is set holds a whole key)
        const uint32_t b = (uint32_t)k01.x;
        if (bits) {
            if (b - lo < nbits) atomicOr(&bits[(b - lo) >> 5], 1u << ((b - lo) & 31u));
        } else {
            any = true;
            mn = min(mn, b);
            mx = max(mx, b);
        }
    }
    if (!bits) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
            mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        }
        const bool wave_any = __builtin_amdgcn_ballot_w64(any) != 0ull;
        if (__lane_id() == 0 && wave_any) {
            atomicMin(&range[0], mn);
            atomicMax(&range[1], mx);
            range[2] = 1u;  // (a bucket was seen: index 0xFFFFFFFF is a bucket like any other)
        }
    }
}
// The bucket index of every occupied slot, compacted (fa_ports_buckets when the indices span more than its bitmap).
__global__ __launch_bounds__(256) void port_bucket_list_kernel(const PSlot* tab, uint64_t nslots, uint32_t* out, uint32_t cap, unsigned int* cursor) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
        const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(&tab[i].w[0]);
        if (k01.y == 0) continue;
        const unsigned int j = atomicAdd(cursor, 1u);
        if (j < cap) out[j] = (uint32_t)k01.x;
    }
}

}  // namespace fa
