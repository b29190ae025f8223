// ports.cuh - exact GROUP BY SrcPort / DstPort for a time range: bucketed port tables (gfx950).
//
// The two port panels (viz-ch.json:358 SrcPort, :604 DstPort) read "... WHERE $timeFilter GROUP BY port".  The group key here is
// (bucket index, port): bucket index = t32 / bucket_secs with t32 = (uint32_t)TimeFlowStart (the DateTime narrowing of
// create.sh:40, the rule of the minute series and of the talker buckets); port = the whole UInt32 column value - 65536 and above
// are keys like any other.  value = sum(Bytes * SamplingRate) mod 2^64 and count(); a group of weight 0 is still a row.
//
// State: two keyed tables of their own (SrcPort, DstPort) - never the ctx's wide table or its dense port histograms - under the
// traits PortTab: the slot claim, the LDS cache, growth, the buckets held and every invariant are keytab.cuh's, the capacity rule
// is table_room.h's.  Slot = 32 bytes: two key words + weight + count.  w0 = bit 63 | bucket index, w1 = bit 63 | port: both
// words are never 0, so 0 is EMPTY for each, and the keys (0, 0) and (0xFFFFFFFF, 0xFFFFFFFF) are words like any other.
//
// port_fold_kernel, the hot part: one lane per record of the decoded columns (six of them, 33 bytes per record), both tables in
// one pass, one 32-bit division per record for the bucket index.  Real port streams are far more skewed than address streams - a
// handful of service ports carries most records - so the LDS cache of (bucket, port) -> (weight, count) per direction is part
// of the design, not an option.
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
#include <stddef.h>
#include <stdint.h>

#include "keytab.cuh"
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

constexpr int PORT_BLOCK = 512;
#ifndef FA_PORT_LDS_ENTRIES
#define FA_PORT_LDS_ENTRIES 512
#endif
constexpr int PORT_LDS_ENTRIES = FA_PORT_LDS_ENTRIES;  // per direction, a power of two
constexpr int PORT_LDS_PROBES = 4;
constexpr int PORT_WG_PER_CU = 2;
static_assert((PORT_LDS_ENTRIES & (PORT_LDS_ENTRIES - 1)) == 0, "the cache is indexed by hash bits");

// (the tally of a created key: n[0] every key, n[1] the large ports - PortCounters' used[] and large[])
struct PortTab {
    using Slot = PSlot;
    using Key = PKey;
    using Counters = PortCounters;
    static constexpr int NW = 2, NT = 2;
    static constexpr int BLOCK = PORT_BLOCK, LDS_ENTRIES = PORT_LDS_ENTRIES, LDS_PROBES = PORT_LDS_PROBES;
    static constexpr int WG_PER_CU = PORT_WG_PER_CU;
    static constexpr char NOUN[] = "port", FN[] = "fa_ports", WGPC_ENV[] = "FA_PORT_WGPC";
    __host__ __device__ static uint32_t hash(const PKey& k) { return pkey_hash(k); }
    __host__ __device__ static uint32_t bucket(const unsigned long long w[2]) { return pkey_bucket(w); }
    __device__ static void tally(const PKey& k, uint32_t (&n)[2]) {
        n[0]++;
        if (pkey_port(k.w) >= PORT_LARGE) n[1]++;
    }
};
static_assert(offsetof(PortCounters, large) == 2 * sizeof(unsigned long long), "tab_counter: large[] lies behind used[]");

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
    __shared__ TabLds<PortTab> L;
    tab_lds_clear(L);
    uint32_t absorbed = 0, folded = 0, created[2][2] = {};
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
            if (tab_lds_add(L, d, k, h, w)) absorbed++;
            else tab_upsert<PortTab>(a.tab[d], a.mask[d], k, h, w, 1, a.ctr, created[d]);
        }
    }
    tab_lds_flush(L, a.tab, a.mask, a.ctr, absorbed, folded, created);
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

}  // namespace fa
