// sketch_fold.cuh - the address sketches and the distinct-address sets from decoded columns (gfx950): one chunk of fa_columns -> the
// ctx's two Count-Min sketches (FA_KEYS_SRCADDR_CMS, FA_KEYS_DSTADDR_CMS) and the sets behind fa_topk.
//
// rollup.cuh rebuilds flows_5m and the exact dashboard key sets from columns; this is the same step for the state fa_topk ranks
// from, through the helpers every ingest path ends in: cms_add (with the replica copies) and keyset_offer (exact: every address;
// candidates: the addresses that pass the bits of the last boundary) - sinks.cuh.  u64 sums commute and the sets are sets, so the
// state is what an ingest of the same records leaves, bit for bit.
//
// Shape: rollup_fold_kernel's - a persistent grid of 256-thread workgroups over the record geometry rollup_rounds / rollup_first
// (rollup.cuh): one trip count for every wave, tail lanes carried as valid = false.  Read per record: status, Bytes, SamplingRate
// and the 16 address bytes of every selected direction (49 bytes for both).  status != 0: skipped and counted, one atomic per
// workgroup.  Weight = Bytes * SamplingRate (u64, wrapping); key = the raw 16 bytes as (lo, hi), as keyset_offer forms them from
// Rec::src / Rec::dst - the EType plays no part.
//
// Per workgroup and direction: an LDS cache (lo, hi) -> wrapping weight sum.  In the candidates mode cms_nrep is 1, and every
// update of a heavy hitter would be `depth` memory-side atomics on the same `depth` words; summed on chip, an address leaves the
// workgroup as ONE cms_add and ONE keyset_offer at the end of the kernel.  A record that finds no room in SKETCH_PROBES entries
// goes straight to cms_add + keyset_offer.  An entry is three write-once words claimed in order with tab_lds_word (keytab.cuh;
// the argument is wide.cuh's: a contender that loses word j leaves the entry, so whoever wins the last word matched the ones
// before).  EMPTY is a word that is 0 - and no key makes one: the 128 key bits are laid out over the three words beside a set
// top bit each (sketch_words), a bijection, so the all-zero address is a key like any other, and neither the key nor the weight
// says "occupied".  An entry whose weights sum to 0 (mod 2^64, or because every record had Bytes = 0) is still offered to the
// set: zero-weight addresses are rows of the ranking (cms_add adds nothing for them, as on the ingest paths).
// SKETCH_ENTRIES = 256 per direction (16 KiB per workgroup, 64 KiB per CU at 4 workgroups) is a GUESS: one size was measured,
// against no cache at all (env FA_SKETCH_LDS=0); what another size gains is not.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keytab.cuh"
#include "rollup.cuh"
#include "sinks.cuh"

namespace fa {

constexpr int SKETCH_ENTRIES = 256, SKETCH_PROBES = 4;
constexpr uint32_t SKETCH_WGPC = 4;  // workgroups per CU (env FA_SKETCH_WGPC)
constexpr uint32_t SKETCH_DIR_SRC = 1u, SKETCH_DIR_DST = 2u;

// the columns a fold reads (device pointers, naturally aligned; the address column of a direction that is not selected may be null)
struct SketchCols {
    const uint64_t *bytes, *sampling_rate;
    const uint4* addr[2];  // SrcAddr, DstAddr
    const uint8_t* status;
    uint32_t m;
    uint32_t dirs;  // SKETCH_DIR_*: wave-uniform
    uint32_t lds;   // 0: no cache, every record goes straight to the sketch and the set (FA_SKETCH_LDS=0)
    unsigned long long* bad;  // records with status != 0 (skipped): one atomic per workgroup
};

struct SketchLds {
    unsigned long long k[3][2][SKETCH_ENTRIES];
    unsigned long long w[2][SKETCH_ENTRIES];
};

// (lo, hi) <-> three words that are never 0: bits 63..1 of lo, bits 63..1 of hi, the two low bits - each beside a set bit 63
__host__ __device__ __forceinline__ void sketch_words(uint64_t lo, uint64_t hi, unsigned long long (&k)[3]) {
    k[0] = (1ull << 63) | (lo >> 1);
    k[1] = (1ull << 63) | (hi >> 1);
    k[2] = (1ull << 63) | ((lo & 1ull) << 1) | (hi & 1ull);
}
__host__ __device__ __forceinline__ void sketch_unwords(const unsigned long long (&k)[3], uint64_t& lo, uint64_t& hi) {
    lo = (k[0] << 1) | ((k[2] >> 1) & 1ull);
    hi = (k[1] << 1) | (k[2] & 1ull);
}
__host__ __device__ __forceinline__ uint32_t sketch_slot(uint64_t lo, uint64_t hi) {
    uint32_t h = (uint32_t)lo * 0x9E3779B1u ^ (uint32_t)(lo >> 32) * 0x85EBCA6Bu ^ (uint32_t)hi * 0xC2B2AE35u ^ (uint32_t)(hi >> 32) * 0x27D4EB2Fu;
    h ^= h >> 15;
    return (h * 0x2545F491u) >> 24;
}
static_assert(SKETCH_ENTRIES == 256, "sketch_slot gives 8 bits");

// true = absorbed by the workgroup's cache
__device__ __forceinline__ bool sketch_lds_add(SketchLds& L, int d, uint64_t lo, uint64_t hi, uint64_t w) {
    unsigned long long k[3];
    sketch_words(lo, hi, k);
    uint32_t i = sketch_slot(lo, hi);
#pragma unroll 1
    for (int probe = 0; probe < SKETCH_PROBES; probe++, i = (i + 1u) & (SKETCH_ENTRIES - 1)) {
        if (!tab_lds_word(&L.k[0][d][i], k[0])) continue;
        if (!tab_lds_word(&L.k[1][d][i], k[1])) continue;
        if (!tab_lds_word(&L.k[2][d][i], k[2])) continue;
        if (w) atomicAdd(&L.w[d][i], (unsigned long long)w);  // (an entry of zero weights is claimed all the same: it is offered at the end)
        return true;
    }
    return false;
}

// one address with a weight into the sketch and the set of its direction: what every ingest path does per record
__device__ __forceinline__ void sketch_sink(const KArgs& a, uint32_t d, uint64_t lo, uint64_t hi, uint64_t w) {
    const uint32_t key[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    cms_add(d ? a.cms_dst : a.cms_src, a.cms_depth, a.cms_wl2, a.cms_seed, key, w, a.cms_nrep);
    keyset_offer(a, d, key);
}

__global__ __launch_bounds__(ROLLUP_BLOCK) void sketch_fold_kernel(KArgs a, SketchCols sc) {
    __shared__ SketchLds L;
    __shared__ uint32_t wg_bad;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (sc.lds) {
        for (uint32_t e = tid; e < 2u * SKETCH_ENTRIES; e += ROLLUP_BLOCK) {
            (&L.k[0][0][0])[e] = 0, (&L.k[1][0][0])[e] = 0, (&L.k[2][0][0])[e] = 0;
            (&L.w[0][0])[e] = 0;
        }
    }
    if (tid == 0) wg_bad = 0;
    __syncthreads();
    const uint32_t rounds = rollup_rounds(sc.m, gridDim.x);
    uint32_t bad = 0;
    for (uint32_t r = 0; r < rounds; r++) {  // (the same trip count in every wave of the grid)
        const uint64_t at = rollup_first(blockIdx.x, wave, r, gridDim.x) + lane;
        const bool in = at < (uint64_t)sc.m;
        const uint32_t i = in ? (uint32_t)at : 0u;
        const bool sure = in && sc.status[i] == 0;
        bad += (in && !sure) ? 1u : 0u;
        uint64_t w = 0;
        if (sure) w = sc.bytes[i] * sc.sampling_rate[i];
#pragma unroll
        for (uint32_t d = 0; d < 2; d++) {
            if (!((sc.dirs >> d) & 1u)) continue;
            if (sure) {
                const uint4 q = sc.addr[d][i];
                const uint64_t lo = (uint64_t)q.y << 32 | q.x, hi = (uint64_t)q.w << 32 | q.z;
                if (!(sc.lds && sketch_lds_add(L, (int)d, lo, hi, w))) sketch_sink(a, d, lo, hi, w);
            }
        }
    }
    // every occupied entry is complete by now (the lane that claimed a word went on to the ones behind it, or met them claimed)
    __syncthreads();
    if (sc.lds) {
        for (uint32_t e = tid; e < 2u * SKETCH_ENTRIES; e += ROLLUP_BLOCK) {
            const uint32_t d = e / SKETCH_ENTRIES, j = e % SKETCH_ENTRIES;
            const unsigned long long k[3] = {L.k[0][d][j], L.k[1][d][j], L.k[2][d][j]};
            if (k[0] == 0) continue;
            uint64_t lo, hi;
            sketch_unwords(k, lo, hi);
            sketch_sink(a, d, lo, hi, L.w[d][j]);
        }
    }
    const uint32_t wb = wave_sum_u32(bad);
    if (lane == 0 && wb) atomicAdd(&wg_bad, wb);
    __syncthreads();
    if (tid == 0 && wg_bad) atomicAdd(sc.bad, (unsigned long long)wg_bad);
}

}  // namespace fa
