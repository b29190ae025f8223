// rollup.cuh - the rollups from decoded columns (gfx950): one chunk of fa_columns -> flows_5m and the dashboard key sets.
//
// The reference's flows_5m is a materialized view that fires on every block inserted into flows_raw
// (compose/clickhouse/create.sh:92-110), so whoever holds flows_raw can rebuild the rollup (INSERT INTO flows_5m SELECT ... FROM
// flows_raw), and the first panel and both port panels read flows_raw itself (viz-ch.json:74,358,604).  rollup_fold_kernel is that
// step for columns in HBM - a loaded part (raw_load_host.inc) or a decode - into the SAME device-wide tables the ingest kernels
// feed, through the same helpers: pack_key / key_hash / as_home (table.cuh), table_find_or_claim + quad_atomic_update, and
// wide_sink_wave's atomic form for the wide key sets (sinks.cuh).  u64 sums commute, so the state is what an ingest of the same
// records leaves, bit for bit.  No tuple segments, no wide log; the sketches and the distinct-address sets have a fold of their own
// (sketch_fold.cuh).
//
// Shape: a persistent grid of 256-thread workgroups.  In round r, wave w of the grid (w = workgroup * 4 + wave of the workgroup)
// takes the 64 records from (r * waves + w) * 64 on: consecutive waves read consecutive 64-record runs of every column, and the
// trip count is the same for EVERY wave - the lane-cooperative helpers (wave_combine, the quad rounds) need whole waves, so tail
// lanes carry valid = false / null pointers through them instead of branching around them.  rollup_rounds / rollup_first are
// that geometry, __host__ __device__: tests/host_rollup.hip enumerates it.
// Per workgroup: an LdsTable<ROLLUP_SLOTS> in front of the flows_5m table (the mocker's 9 groups, mocker.go:61-62, become 9 LDS
// adds per wave instead of 9 hot memory-side atomics) and LdsMinutes in front of the minute series; both are flushed once at the
// end.  ROLLUP_SLOTS = 256 (10 KiB, 10.3 KiB with LdsMinutes): the registers allow 8 waves per SIMD for the flows_5m variant
// (38 VGPRs) and 6 for the runtime-mask one (78), i.e. 8 / 6 workgroups per CU, and eight tables are 82 KiB of the CU's 160 KiB
// - the table does not limit occupancy until it is twice as large.  The size is a GUESS: what a larger table would gain in hit
// rate on mid-cardinality streams (a few thousand groups) is not measured; 256 slots hold every group of the mocker shape and
// cost ROLLUP_PROBES LDS probes per record on a stream of distinct groups.  ROLLUP_WGPC = 4 was chosen before it was measured; on
// one stream (config 2, chunks of 2^20 rows) 2 / 4 / 6 / 8 workgroups per CU read 0.153 / 0.167 / 0.185 / 0.203 ns
// per record for flows_5m alone and 0.822 / 0.841 / 0.849 / 0.859 for all four key sets: flat within 4 % where the wide table's
// atomics dominate, and every workgroup more is one more LDS-table flush.  Longer chunks and other streams are not measured.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sinks.cuh"

namespace fa {

constexpr int ROLLUP_BLOCK = 256, ROLLUP_WAVES = ROLLUP_BLOCK / 64;
constexpr int ROLLUP_SLOTS = 256, ROLLUP_PROBES = 4;
constexpr uint32_t ROLLUP_WGPC = 4;             // workgroups per CU (env FA_ROLLUP_WGPC)
constexpr uint32_t ROLLUP_MAX_GRID = 1u << 16;  // (m <= 2^25 records: (rounds * grid * 4 + 2^18) * 64 stays below 2^64 by far)

// rounds every wave of a grid of `grid` workgroups makes over m records
__host__ __device__ __forceinline__ uint32_t rollup_rounds(uint32_t m, uint32_t grid) {
    const uint64_t per_round = (uint64_t)grid * ROLLUP_WAVES * 64u;
    return (uint32_t)(((uint64_t)m + per_round - 1u) / per_round);
}
// first record of wave `wave` (0..3) of workgroup g in round r; its lane l takes record first + l when that is below m
__host__ __device__ __forceinline__ uint64_t rollup_first(uint32_t g, uint32_t wave, uint32_t r, uint32_t grid) {
    return (((uint64_t)r * grid + g) * ROLLUP_WAVES + wave) * 64u;
}

// the columns a fold reads (device pointers, naturally aligned; the ones the launch's key sets do not read may be null)
struct RollupCols {
    const uint64_t *time_received, *time_flow_start, *sampling_rate, *bytes, *packets;
    const uint32_t *src_as, *dst_as, *etype, *proto, *src_port, *dst_port;
    const uint4* src_addr;
    const uint8_t* status;
    uint32_t m;
    unsigned long long* bad;  // records with status != 0 (skipped, inserter.go:125-126): one atomic per workgroup
};

// KEYSETS: the compile-time key-set mask (FA_KEYS_AS_PAIR: flows_5m alone; KS_ALL: the runtime mask a.key_sets decides, ks_on)
template <uint32_t KEYSETS>
__global__ __launch_bounds__(ROLLUP_BLOCK) void rollup_fold_kernel(KArgs a, RollupCols rc) {
    __shared__ LdsTable<ROLLUP_SLOTS> lt;
    __shared__ LdsMinutes lm;
    __shared__ uint32_t wg_tally[2];  // late, bad
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool on_as = ks_on<KEYSETS>(a, FA_KEYS_AS_PAIR), on_app = ks_on<KEYSETS>(a, FA_KEYS_ADDR_PORT_PROTO);
    const bool on_port = ks_on<KEYSETS>(a, FA_KEYS_PORT_HIST), on_min = ks_on<KEYSETS>(a, FA_KEYS_MINUTE_SERIES);
    if (KEYSETS & FA_KEYS_AS_PAIR) lds_table_clear(lt);
    if (KEYSETS & FA_KEYS_MINUTE_SERIES) lds_minutes_clear(lm);
    if (tid < 2) wg_tally[tid] = 0;
    __syncthreads();
    const uint32_t rounds = rollup_rounds(rc.m, gridDim.x);
    uint32_t late = 0, bad = 0;
    for (uint32_t r = 0; r < rounds; r++) {  // (the same trip count in every wave of the grid)
        const uint64_t at = rollup_first(blockIdx.x, wave, r, gridDim.x) + lane;
        const bool in = at < (uint64_t)rc.m;
        const uint32_t i = in ? (uint32_t)at : 0u;
        const bool sure = in && rc.status[i] == 0;
        bad += (in && !sure) ? 1u : 0u;
        Rec rec;
        rec_clear(rec);
        if (sure) {  // only the columns of the launch's key sets
            rec.time_received = rc.time_received[i];
            if (on_as | on_app | on_port | on_min) rec.bytes = rc.bytes[i];
            if (on_as | on_app) rec.packets = rc.packets[i];
            if (on_as) {
                rec.src_as = rc.src_as[i];
                rec.dst_as = rc.dst_as[i];
                rec.etype = rc.etype[i];
            }
            if (on_port | on_min) rec.sampling_rate = rc.sampling_rate[i];
            if (on_app) {
                const uint4 s = rc.src_addr[i];
                rec.src[0] = s.x, rec.src[1] = s.y, rec.src[2] = s.z, rec.src[3] = s.w;
                rec.proto = rc.proto[i];
            }
            if (on_app | on_port) rec.dst_port = rc.dst_port[i];
            if (on_port) rec.src_port = rc.src_port[i];
            if (on_min) rec.time_flow_start = rc.time_flow_start[i];
        }
        const uint32_t tb = time_bucket(a, (uint32_t)rec.time_received);  // UInt64 -> DateTime (create.sh:39), the ingest's granule
        late += (sure && tb < a.late_below) ? 1u : 0u;
        if (on_as) {
            uint64_t k0, k1;
            pack_key(tb, rec.src_as, rec.dst_as, rec.etype, k0, k1);
            uint64_t b = rec.bytes, p = rec.packets, c = 1;
            bool valid = sure;
            wave_combine<16, 2>(valid, k0, k1, b, p, c);
            const uint32_t h = key_hash(k0, k1);
            const bool pending = valid && !lds_table_add<ROLLUP_SLOTS, ROLLUP_PROBES>(lt, k0, k1, h, b, p, c);
            if (__builtin_amdgcn_ballot_w64(pending) != 0ull) {  // wave-uniform: one atomic line transaction per record that missed
                Slot* sp = nullptr;
                if (pending) {
                    sp = table_find_or_claim(a, k0, k1, h);
                    if (!sp) spill_park(a, k0, k1, b, p, c);
                }
                quad_atomic_update(sp, b, p, c);
            }
        }
        // the wide key sets: wide_sink_wave's atomic form (no segment counters: nothing leaves as a tuple, nothing is logged)
        if (KEYSETS & FA_KEYS_WIDE) wide_sink_wave<KEYSETS>(a, lm, rec, sure, tb);
    }
    if (KEYSETS & FA_KEYS_MINUTE_SERIES) {
        __syncthreads();
        if (tid < LDS_MINUTES && lm.key[tid] != 0 && lm.c[tid] != 0) {
            WKey k;
            wkey_pack(WK_MINUTE, 0, 0, 0, lm.key[tid] - 1u, 0, k);
            wagg_global(wargs(a), k, lm.w[tid], 0, lm.c[tid]);
        }
    }
    if (KEYSETS & FA_KEYS_AS_PAIR) {
        __syncthreads();
        for (uint32_t s = tid; s < (uint32_t)ROLLUP_SLOTS; s += ROLLUP_BLOCK) {
            const unsigned long long k0 = lt.k0[s], k1 = lt.k1[s], c = lt.count[s];
            if (k0 != 0 && k1 != 0 && c != 0) agg_global(a, k0, k1, key_hash(k0, k1), lt.bytes[s], lt.packets[s], c);
        }
    }
    // late and skipped records: one atomic per workgroup and counter
    const uint32_t wl = wave_sum_u32(late), wb = wave_sum_u32(bad);
    if (lane == 0) {
        if (wl) atomicAdd(&wg_tally[0], wl);
        if (wb) atomicAdd(&wg_tally[1], wb);
    }
    __syncthreads();
    if (tid == 0) {
        if (wg_tally[0]) atomicAdd(&a.ctr->late, (unsigned long long)wg_tally[0]);
        if (wg_tally[1]) atomicAdd(rc.bad, (unsigned long long)wg_tally[1]);
    }
}

}  // namespace fa
