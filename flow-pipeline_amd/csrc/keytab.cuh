// keytab.cuh - the device core of the keyed tables: the exact talker tables (talkers.cuh) and the bucketed port tables
// (ports.cuh) are this code under two traits types (gfx950).  Host side: keytab_host.inc.
//
// A pair of open-addressed tables (one per direction), slot = key words + weight + count.  Every key word is never 0, so 0 is
// EMPTY for each; a slot is claimed word by word with 64-bit CAS in the order w0, w1, ... (the argument of wide.cuh: a word is
// written once, a contender that loses word j leaves the slot, so the lane that wins the last word matched the ones before).
// Probing is linear over the WHOLE table and has no limit: the host keeps the load at or below 1/2 before every launch
// (table_room.h), so a probe sequence ends and no update is ever parked or lost.
//
// A fold kernel runs one lane per record, both tables in one pass, between tab_lds_clear and tab_lds_flush: a
// workgroup-private LDS cache of key -> (weight, count) per direction absorbs repeats, which would otherwise put millions of
// same-key atomics on a handful of L2 lines.  An entry's key is the slot's words, claimed in order with LDS CAS; a lane that
// loses a word tries the next entry (T::LDS_PROBES of them), then goes straight to the global table.  The cache is cleared at
// the start of the launch and flushed at its end, one global upsert per occupied entry.
//
// Invariants:
//   - an LDS entry or a global slot only ever holds ONE key (write-once words, claimed in order);
//   - every (record, direction) update is applied exactly once: to the cache (and from there once by the flush) or to the
//     global table, never both;
//   - u64 wrap-around adds commute: any order of updates, chunks, growths, rebuilds and merges gives bit-identical sums;
//   - creations are summed per wave, then per workgroup, before they touch the device counters (one word for every creation of
//     the chip serialises: the talkers measured 0.99 -> 0.31 ns per record for exactly this).
//
// The traits type T:
//   Slot, Key, Counters     w[NW] first in Slot and Key; Slot goes on with weight, count; Counters starts with NT pairs of
//                           words [tally][direction] (used[2], then what else T::tally counts) and has folded, absorbed, lost
//   NW, NT                  key words; words of the per-lane tally of the keys a lane created (n[0] = all of them)
//   BLOCK, LDS_ENTRIES, LDS_PROBES   the fold kernel's geometry
//   hash(k), bucket(w), tally(k, n)  the key's hash, its bucket index (floor tests, bucket listings), n[] counted up for a new key
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "table.cuh"

namespace fa {

// Adds (w, cnt) to k's slot, claiming one if the key is new.  Stale plain reads (per-XCD L2s are not coherent) can only show
// EMPTY or the final word - never a false match; an EMPTY that is stale is settled by the CAS.
// n: the lane's tally of the keys it created (tab_count_created and tab_lds_flush add the sums to the counters).
template <class T>
__device__ __forceinline__ void tab_upsert(typename T::Slot* tab, uint32_t mask, const typename T::Key& k, uint32_t h, uint64_t w, uint64_t cnt, typename T::Counters* ctr,
                                           uint32_t (&n)[T::NT]) {
    uint32_t i = h & mask;
    // (the bound is the table itself: with the load at or below 1/2 an EMPTY slot is met long before it)
    for (uint32_t probe = 0; probe <= mask; probe++, i = (i + 1u) & mask) {
        typename T::Slot* s = &tab[i];
        const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(&s->w[0]);
        unsigned long long c[T::NW];
        c[0] = k01.x;
        c[1] = k01.y;
        if constexpr (T::NW == 3) c[2] = s->w[2];
        bool mine = true;
#pragma unroll
        for (int j = 0; j < T::NW; j++) {
            if (!mine) break;
            if (c[j] == 0) {
                c[j] = atomicCAS(&s->w[j], 0ull, k.w[j]);
                if (c[j] == 0) {
                    c[j] = k.w[j];
                    if (j == T::NW - 1) T::tally(k, n);  // this lane created the group
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

// the counter word of tally word t and direction d
template <class T>
__device__ __forceinline__ unsigned long long* tab_counter(typename T::Counters* ctr, int t, int d) {
    return &ctr->used[0] + 2 * t + d;
}
// (all lanes of the wave: after a kernel's loop over one table)
template <class T>
__device__ __forceinline__ void tab_count_created(typename T::Counters* ctr, int d, const uint32_t (&n)[T::NT]) {
#pragma unroll
    for (int t = 0; t < T::NT; t++) {
        const uint64_t s = wave_sum_u64(n[t]);
        if (__lane_id() == 0 && s) atomicAdd(tab_counter<T>(ctr, t, d), (unsigned long long)s);
    }
}

template <class T>
struct TabLds {
    unsigned long long k[T::NW][2][T::LDS_ENTRIES];
    unsigned long long w[2][T::LDS_ENTRIES], c[2][T::LDS_ENTRIES];
    unsigned long long absorbed, folded, created[T::NT][2];
};

// one key word of an entry: EMPTY is claimed, then it must be ours.  (A plain read that shows a word is final.)
__device__ __forceinline__ bool tab_lds_word(unsigned long long* p, unsigned long long want) {
    unsigned long long cur = *p;
    if (cur == 0) {
        cur = atomicCAS(p, 0ull, want);
        if (cur == 0) cur = want;
    }
    return cur == want;
}
// true = absorbed by the workgroup's cache
template <class T>
__device__ __forceinline__ bool tab_lds_add(TabLds<T>& L, int d, const typename T::Key& k, uint32_t h, uint64_t w) {
    uint32_t i = (h >> 9) & (T::LDS_ENTRIES - 1);
#pragma unroll 1
    for (int probe = 0; probe < T::LDS_PROBES; probe++, i = (i + 1u) & (T::LDS_ENTRIES - 1)) {
        if (!tab_lds_word(&L.k[0][d][i], k.w[0])) continue;
        if (!tab_lds_word(&L.k[1][d][i], k.w[1])) continue;
        if constexpr (T::NW == 3)
            if (!tab_lds_word(&L.k[2][d][i], k.w[2])) continue;
        if (w) atomicAdd(&L.w[d][i], (unsigned long long)w);
        atomicAdd(&L.c[d][i], 1ull);  // (count even when the weight is 0)
        return true;
    }
    return false;
}

// (the whole workgroup: before the fold kernel's record loop)
template <class T>
__device__ __forceinline__ void tab_lds_clear(TabLds<T>& L) {
    for (int i = threadIdx.x; i < 2 * T::LDS_ENTRIES; i += T::BLOCK) {
#pragma unroll
        for (int j = 0; j < T::NW; j++) (&L.k[j][0][0])[i] = 0;
        (&L.w[0][0])[i] = 0;
        (&L.c[0][0])[i] = 0;
    }
    if (threadIdx.x == 0) {
        L.absorbed = L.folded = 0;
#pragma unroll
        for (int t = 0; t < T::NT; t++) L.created[t][0] = L.created[t][1] = 0;
    }
    __syncthreads();
}

// (the whole workgroup: after the record loop)  The cache's entries into the tables, then the lanes' counts - records folded,
// updates absorbed, keys created per direction - summed per wave, per workgroup, and added with one atomic per workgroup and counter.
template <class T>
__device__ __forceinline__ void tab_lds_flush(TabLds<T>& L, typename T::Slot* const (&tab)[2], const uint32_t (&mask)[2], typename T::Counters* ctr, uint32_t absorbed,
                                              uint32_t folded, uint32_t (&n)[2][T::NT]) {
    const uint64_t wa = wave_sum_u64(absorbed), wf = wave_sum_u64(folded);
    if (__lane_id() == 0) {
        if (wa) atomicAdd(&L.absorbed, (unsigned long long)wa);
        if (wf) atomicAdd(&L.folded, (unsigned long long)wf);
    }
    __syncthreads();
    // every occupied entry is complete by now (the lane that claimed w0 went on to the words behind it, or met them claimed)
    for (int e = threadIdx.x; e < 2 * T::LDS_ENTRIES; e += T::BLOCK) {
        const int d = e / T::LDS_ENTRIES, j = e % T::LDS_ENTRIES;
        if (L.k[0][d][j] == 0) continue;
        typename T::Key k;
#pragma unroll
        for (int x = 0; x < T::NW; x++) k.w[x] = L.k[x][d][j];
        tab_upsert<T>(tab[d], mask[d], k, T::hash(k), L.w[d][j], L.c[d][j], ctr, n[d]);
    }
#pragma unroll
    for (int d = 0; d < 2; d++)
#pragma unroll
        for (int t = 0; t < T::NT; t++) {
            const uint64_t wc = wave_sum_u64(n[d][t]);
            if (__lane_id() == 0 && wc) atomicAdd(&L.created[t][d], (unsigned long long)wc);
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (L.absorbed) atomicAdd(&ctr->absorbed, L.absorbed);
        if (L.folded) atomicAdd(&ctr->folded, L.folded);
#pragma unroll
        for (int t = 0; t < T::NT; t++)
#pragma unroll
            for (int d = 0; d < 2; d++)
                if (L.created[t][d]) atomicAdd(tab_counter<T>(ctr, t, d), L.created[t][d]);
    }
}

// Growth and retention: every occupied slot of the old table is inserted again (key, weight, count) - the sums stay exact; the
// counters of direction d are counted again (the host zeroes them before the launch).
// floor_index (drop_before; 0 = keep everything): slots of a bucket index below it are left behind.
template <class T>
__global__ __launch_bounds__(256) void tab_rehash_kernel(const typename T::Slot* old_tab, uint64_t old_slots, typename T::Slot* tab, uint32_t mask, typename T::Counters* ctr, int d,
                                                         uint32_t floor_index) {
    uint32_t n[T::NT] = {};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * blockDim.x) {
        const typename T::Slot* s = &old_tab[i];
        if (s->w[0] == 0) continue;
        typename T::Key k;
#pragma unroll
        for (int j = 0; j < T::NW; j++) k.w[j] = s->w[j];
        if (T::bucket(k.w) < floor_index) continue;
        tab_upsert<T>(tab, mask, k, T::hash(k), s->weight, s->count, ctr, n);
    }
    tab_count_created<T>(ctr, d, n);
}

// The buckets held, shaped like timeslots_kernel (maintenance.cuh).  bits == nullptr: the smallest and largest bucket index of the
// occupied slots into range[0..1] (one atomic pair per wave), range[2] = a bucket was seen; else one bit per index of
// [lo, lo + nbits).
template <class T>
__global__ __launch_bounds__(256) void tab_buckets_kernel(const typename T::Slot* tab, uint64_t nslots, uint32_t lo, uint32_t nbits, unsigned int* bits, unsigned int* range) {
    uint32_t mn = 0xffffffffu, mx = 0u;
    bool any = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
        if (tab[i].w[T::NW - 1] == 0) continue;  // (the last word claimed: a slot whose last word is set holds a whole key)
        const uint32_t b = T::bucket(tab[i].w);
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
// The bucket index of every occupied slot, compacted (the buckets held when the indices span more than the bitmap).
template <class T>
__global__ __launch_bounds__(256) void tab_bucket_list_kernel(const typename T::Slot* tab, uint64_t nslots, uint32_t* out, uint32_t cap, unsigned int* cursor) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
        if (tab[i].w[T::NW - 1] == 0) continue;
        const unsigned int j = atomicAdd(cursor, 1u);
        if (j < cap) out[j] = T::bucket(tab[i].w);
    }
}

}  // namespace fa
