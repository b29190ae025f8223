// talkers.cuh - exact GROUP BY SrcAddr / DstAddr "top talkers", grouped as the dashboards do (gfx950).
//
// The two top-talker panels (viz-ch.json:233 SrcAddr, :479 DstAddr) group by the RENDERED string
//   if(EType = 0x800, IPv4NumToString(first four bytes), IPv6NumToString(Addr))
// so the group key is the string's preimage (talker_canon below):
//   EType == 0x800   family 0x800, key = bytes 0..3 followed by twelve zero bytes (fa_format_addr ignores bytes 4..15);
//   any other EType  family 0,     key = all 16 bytes (0x86dd, 0, 0x1234 ... fall into one group).
// The same 16 bytes under the two families are two groups: a dotted quad is never an IPv6NumToString output.
// value = sum(Bytes * SamplingRate) mod 2^64 and count(); a group of weight 0 is still a row.
//
// State: two keyed tables of their own (SrcAddr, DstAddr) - never the ctx's wide table - under the traits TalkTab: the slot claim,
// the LDS cache, growth, the buckets held and every invariant are keytab.cuh's, the capacity rule is table_room.h's.  Slot = one
// 64-byte line: three key words + weight + count; every key word has bit 63 set, so 0 is EMPTY for each.
//
// talker_fold_kernel, the hot part: one lane per record of the decoded columns (six of them, 53 bytes per record), both
// tables in one pass; mocker-shaped and Zipf streams are what the LDS cache is for (why the ingest kernel has its
// hot-address cache and LdsMinutes).
//
// Sizes (reasoned, not yet measured on hardware - DESIGN.md 3.7): 512 threads and 512 entries per direction = 40 KiB of LDS per
// workgroup, two workgroups per CU = 16 waves per CU behind the random-access latency of the global upserts, half of
// the CU's 160 KiB of LDS.  A launch flushes at most 2 x 512 entries per workgroup: 2^19 upserts for a chunk of 2^20
// records whose 2^21 updates would otherwise all be global.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "keytab.cuh"
#include "table.cuh"

namespace fa {

constexpr uint32_t TALK_FAMILY_V4 = 0x800u;

// (lo, hi) = the FixedString(16) as two little-endian u64 (lo = bytes 0..7).  Returns the family.
__host__ __device__ __forceinline__ uint32_t talker_canon_words(uint64_t& lo, uint64_t& hi, uint32_t etype) {
    if (etype != TALK_FAMILY_V4) return 0u;
    lo &= 0xffffffffull;  // bytes 0..3
    hi = 0;
    return TALK_FAMILY_V4;
}
__host__ __device__ __forceinline__ void talker_canon(const uint8_t addr[16], uint32_t etype, uint64_t* lo, uint64_t* hi, uint32_t* family) {
    uint64_t l = 0, h = 0;
    for (int i = 0; i < 8; i++) {
        l |= (uint64_t)addr[i] << (8 * i);
        h |= (uint64_t)addr[8 + i] << (8 * i);
    }
    *family = talker_canon_words(l, h, etype);
    *lo = l;
    *hi = h;
}

struct TKey {
    unsigned long long w[3];
};
// 128 key bits + the family bit in three words that are never 0
__host__ __device__ __forceinline__ void tkey_pack(uint64_t lo, uint64_t hi, uint32_t family, TKey& k) {
    constexpr unsigned long long B63 = 1ull << 63, M63 = B63 - 1;
    k.w[0] = B63 | (lo & M63);
    k.w[1] = B63 | (((lo >> 63) | (hi << 1)) & M63);
    k.w[2] = B63 | (hi >> 62) | (family ? 4ull : 0ull);
}
__host__ __device__ __forceinline__ void tkey_unpack(const unsigned long long w[3], unsigned long long& lo, unsigned long long& hi, uint32_t& family) {
    constexpr unsigned long long M63 = (1ull << 63) - 1;
    const unsigned long long a = w[0] & M63, b = w[1] & M63;
    lo = a | (b << 63);
    hi = (b >> 1) | ((w[2] & 3ull) << 62);
    family = (w[2] & 4ull) ? TALK_FAMILY_V4 : 0u;
}
// Bucketed tables (fa_talkers_enable_buckets): the group key is (bucket, address, family).  The bucket INDEX (t32 / bucket_secs,
// 32 bits) lives in bits 8..39 of w[2], beside the 3 payload bits tkey_pack uses - index 0 packs to tkey_pack's words, and
// tkey_unpack (which masks bits 0..2) reads the address and family of either kind of key.
constexpr int TKEY_BUCKET_SHIFT = 8;
__host__ __device__ __forceinline__ void tkey_pack_bucket(uint64_t lo, uint64_t hi, uint32_t family, uint32_t bucket_index, TKey& k) {
    tkey_pack(lo, hi, family, k);
    k.w[2] |= (unsigned long long)bucket_index << TKEY_BUCKET_SHIFT;
}
__host__ __device__ __forceinline__ uint32_t tkey_bucket(const unsigned long long w[3]) { return (uint32_t)(w[2] >> TKEY_BUCKET_SHIFT); }
__host__ __device__ __forceinline__ uint32_t tkey_hash(const TKey& k) {
    return key_hash(k.w[0] ^ (k.w[2] * 0x9E3779B97F4A7C15ull), k.w[1]);
}

struct __attribute__((aligned(64))) TSlot {
    unsigned long long w[3], pad0;
    unsigned long long weight, count, pad1, pad2;
};
static_assert(sizeof(TSlot) == 64, "one talker slot per 64-byte line");

struct TalkCounters {
    unsigned long long used[2];   // occupied slots: the lane that wins the last key word counts the key, the counts are summed per wave /
                                  // workgroup and added once at the end of the kernel (one word for every creation of the chip serialises)
    unsigned long long folded;    // status == 0 records folded
    unsigned long long absorbed;  // (record, direction) updates that ended in an LDS cache
    unsigned long long lost;      // updates that met a full table: the host's capacity rule was broken (never on a correct host)
};

// One public row (include/flowagg.h: fa_talker_row), 40 bytes.
struct TalkRow {
    unsigned long long key[2];  // the 16 canonical bytes
    uint32_t etype, pad;
    unsigned long long weight, count;
};
static_assert(sizeof(TalkRow) == 40, "fa_talker_row");

constexpr int TALK_BLOCK = 512;
#ifndef FA_TALK_LDS_ENTRIES
#define FA_TALK_LDS_ENTRIES 512
#endif
constexpr int TALK_LDS_ENTRIES = FA_TALK_LDS_ENTRIES;  // per direction, a power of two
constexpr int TALK_LDS_PROBES = 4;
constexpr int TALK_WG_PER_CU = 2;
static_assert((TALK_LDS_ENTRIES & (TALK_LDS_ENTRIES - 1)) == 0, "the cache is indexed by hash bits");

struct TalkTab {
    using Slot = TSlot;
    using Key = TKey;
    using Counters = TalkCounters;
    static constexpr int NW = 3, NT = 1;
    static constexpr int BLOCK = TALK_BLOCK, LDS_ENTRIES = TALK_LDS_ENTRIES, LDS_PROBES = TALK_LDS_PROBES;
    static constexpr int WG_PER_CU = TALK_WG_PER_CU;
    static constexpr char NOUN[] = "talker", FN[] = "fa_talkers", WGPC_ENV[] = "FA_TALK_WGPC";
    __host__ __device__ static uint32_t hash(const TKey& k) { return tkey_hash(k); }
    __host__ __device__ static uint32_t bucket(const unsigned long long w[3]) { return tkey_bucket(w); }
    __device__ static void tally(const TKey&, uint32_t (&n)[1]) { n[0]++; }
};

struct TalkFoldArgs {
    const uint4* src_addr;
    const uint4* dst_addr;
    const uint32_t* etype;
    const uint64_t* bytes;
    const uint64_t* sampling_rate;
    const uint8_t* status;
    uint32_t n;
    TSlot* tab[2];
    uint32_t mask[2];
    TalkCounters* ctr;
    // bucketed tables only (last: the plain instantiation's arguments stay where they were)
    const uint64_t* time_flow_start;
    uint32_t bucket_secs;  // (0 on a plain ctx)
};

// BUCKETED: the seventh column (TimeFlowStart, 61 bytes per record) gives the key its bucket index - t32 / bucket_secs with
// t32 = (uint32_t)TimeFlowStart, the DateTime narrowing of create.sh:40.  One 32-bit division per record, plain `/`: the random
// upserts bound this kernel, not its ALU.  Everything behind the pack works on the three key words and is shared.
template <bool BUCKETED>
__global__ __launch_bounds__(TALK_BLOCK) void talker_fold_kernel(TalkFoldArgs a) {
    __shared__ TabLds<TalkTab> L;
    tab_lds_clear(L);
    uint32_t absorbed = 0, folded = 0, created[2][1] = {};
    for (uint64_t i = (uint64_t)blockIdx.x * TALK_BLOCK + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * TALK_BLOCK) {
        if (a.status[i]) continue;  // malformed: dropped, whatever the other columns hold
        folded++;
        const uint32_t et = a.etype[i];
        const uint64_t w = a.bytes[i] * a.sampling_rate[i];
        uint32_t bidx = 0;
        if (BUCKETED) bidx = (uint32_t)a.time_flow_start[i] / a.bucket_secs;
#pragma unroll
        for (int d = 0; d < 2; d++) {
            const uint4 q = (d ? a.dst_addr : a.src_addr)[i];
            uint64_t lo = (uint64_t)q.y << 32 | q.x, hi = (uint64_t)q.w << 32 | q.z;
            const uint32_t fam = talker_canon_words(lo, hi, et);
            TKey k;
            if (BUCKETED) tkey_pack_bucket(lo, hi, fam, bidx, k);
            else tkey_pack(lo, hi, fam, k);
            const uint32_t h = tkey_hash(k);
            if (tab_lds_add(L, d, k, h, w)) absorbed++;
            else tab_upsert<TalkTab>(a.tab[d], a.mask[d], k, h, w, 1, a.ctr, created[d]);
        }
    }
    tab_lds_flush(L, a.tab, a.mask, a.ctr, absorbed, folded, created);
}

// fa_merge_talkers: canonical rows of another ctx.
__global__ __launch_bounds__(256) void talker_merge_kernel(const TalkRow* rows, uint32_t n, TSlot* tab, uint32_t mask, TalkCounters* ctr, int d) {
    uint32_t created[1] = {0};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        TKey k;
        tkey_pack(rows[i].key[0], rows[i].key[1], rows[i].etype, k);
        tab_upsert<TalkTab>(tab, mask, k, tkey_hash(k), rows[i].weight, rows[i].count, ctr, created);
    }
    tab_count_created<TalkTab>(ctr, d, created);
}

// ---- read side: compaction, sort keys, emit ---------------------------------------------------------------------
// The occupied slots as rows for the device-resident close (rows_host.inc, collect_talkers), unordered.  Shaped like
// wextract_kernel (maintenance.cuh): a workgroup of 16 waves looks at TR_U x 1024 slots per round - every lane its own 64-byte
// slot, three 16-byte loads, so a wave reads 64 whole lines - ballot and popcount give each row its place among the wave's,
// and the workgroup takes the places of the round's rows with ONE returning atomic.  cap = the table's own count of occupied
// slots; *cursor ends at the rows there were.
// RANGED (fa_talkers_range_rows_device, bucketed tables): only the slots whose bucket index lies in [index_lo, index_last]
// (both inclusive: the last index of the axis has no successor in 32 bits) are kept; the row carries no bucket, so a key
// held in several buckets leaves as several rows, which the merge behind the read folds.  cap = the table's count of
// occupied slots, an upper bound there.
constexpr int TR_U = 4;
constexpr int TR_BLOCK = 1024;
template <bool RANGED>
__global__ __launch_bounds__(TR_BLOCK) void talker_rows_kernel(const TSlot* tab, uint32_t nslots, TalkRow* rows, uint32_t cap, unsigned int* cursor, uint32_t index_lo, uint32_t index_last) {
    __shared__ uint32_t wave_total[TR_BLOCK / 64];
    __shared__ uint32_t wg_rows;
    const uint32_t nthr = gridDim.x * blockDim.x, lane = __lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t b0 = blockIdx.x * blockDim.x; b0 < nslots; b0 += TR_U * nthr) {  // (the trip count is the workgroup's: barriers inside)
        const uint32_t i0 = b0 + threadIdx.x;
        ulonglong2 q[TR_U][3];  // {w0, w1}, {w2, -}, {weight, count}
        bool sel[TR_U];
        unsigned long long m[TR_U];
        uint32_t total = 0;
#pragma unroll
        for (int u = 0; u < TR_U; u++) {
            // (i0 + u * nthr < 2^32: nslots <= 2^30 and a round overshoots by less than TR_U * nthr <= 2^21)
            const ulonglong2* p = reinterpret_cast<const ulonglong2*>(&tab[min(i0 + (uint32_t)u * nthr, nslots - 1u)]);
            q[u][0] = p[0];
            q[u][1] = p[1];
            q[u][2] = p[2];
        }
#pragma unroll
        for (int u = 0; u < TR_U; u++) {
            sel[u] = i0 + (uint32_t)u * nthr < nslots && q[u][0].x != 0ull;
            if (RANGED) {
                const uint32_t b = (uint32_t)(q[u][1].x >> TKEY_BUCKET_SHIFT);
                sel[u] = sel[u] && b >= index_lo && b <= index_last;
            }
            m[u] = __builtin_amdgcn_ballot_w64(sel[u]);
            total += (uint32_t)__builtin_popcountll(m[u]);
        }
        if (lane == 0) wave_total[wave] = total;
        __syncthreads();
        if (threadIdx.x < 64) {  // wave 0: the workgroup's rows of this round, one atomic
            const uint32_t t = lane < TR_BLOCK / 64 ? wave_total[lane] : 0u;
            uint32_t incl = t;
#pragma unroll
            for (int o = 1; o < TR_BLOCK / 64; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                if (lane >= (uint32_t)o) incl += up;
            }
            const uint32_t wg_total = (uint32_t)__builtin_amdgcn_readlane((int)incl, TR_BLOCK / 64 - 1);
            uint32_t base = 0;
            if (lane == 0 && wg_total != 0u) base = atomicAdd(cursor, wg_total);
            base = (uint32_t)__builtin_amdgcn_readlane((int)base, 0);
            if (lane < TR_BLOCK / 64) wave_total[lane] = base + incl - t;  // (exclusive: where this wave's rows start)
            if (lane == 0) wg_rows = wg_total;
        }
        __syncthreads();
        if (wg_rows != 0u && total != 0u) {  // (wave-uniform)
            unsigned int base = wave_total[wave];
#pragma unroll
            for (int u = 0; u < TR_U; u++) {
                const unsigned int j = base + (unsigned int)__builtin_popcountll(m[u] & ((1ull << lane) - 1ull));
                base += (unsigned int)__builtin_popcountll(m[u]);
                if (sel[u] && j < cap) {  // (j < cap always: cap counts the same slots)
                    const unsigned long long w[3] = {q[u][0].x, q[u][0].y, q[u][1].x};
                    TalkRow r;
                    tkey_unpack(w, r.key[0], r.key[1], r.etype);
                    r.pad = 0;
                    r.weight = q[u][2].x;
                    r.count = q[u][2].y;
                    rows[j] = r;
                }
            }
        }
        __syncthreads();  // (wave_total and wg_rows are rewritten by the next round)
    }
}
__device__ __forceinline__ unsigned long long talk_bswap64(unsigned long long v) { return __builtin_bswap64(v); }
// Sort key of pass p over the rows in their current order (perm == nullptr: the identity, which is written to perm_out).
// Emit order = weight DESC, key bytes ascending (memcmp), etype ascending - least significant criterion first, stable passes:
//   0 etype   1 bytes 8..15 as a big-endian word   2 bytes 0..7 as a big-endian word   3 the inverted weight
__global__ __launch_bounds__(256) void talker_sortkey_kernel(const TalkRow* rows, const uint32_t* perm, uint32_t n, int pass, unsigned long long* keys, uint32_t* perm_out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t j = perm ? perm[i] : i;
        if (!perm) perm_out[i] = i;
        const TalkRow& r = rows[j];
        keys[i] = pass == 0 ? (unsigned long long)r.etype : pass == 1 ? talk_bswap64(r.key[1]) : pass == 2 ? talk_bswap64(r.key[0]) : ~r.weight;
    }
}
__global__ __launch_bounds__(256) void talker_emit_kernel(const TalkRow* rows, const uint32_t* perm, uint32_t n, TalkRow* out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = rows[perm[i]];
}

}  // namespace fa
