// host_port_buckets.hip - host instantiation of the bucketed port key (ports.cuh: pkey_pack / pkey_bucket / pkey_port / pkey_empty /
// port_bucket_index) and of the range rule every ranged read shares (bucket_range.h: bucket_range_of).
// TEST INFRASTRUCTURE (tests/test_port_buckets_cpu.py).  No GPU call.
//   host_port_buckets keys IN OUT: IN holds records of {bucket index, port, bucket_secs, pad: uint32; TimeFlowStart: uint64}
//   (little-endian, 24 bytes); OUT receives, per record, what the packed key words give back - {bucket index, port} - and
//   {the index port_bucket_index computes from TimeFlowStart, 0} (uint32 each).  On the way: both key words keep bit 63, so
//   neither is EMPTY for any key - (0, 0) and (0xFFFFFFFF, 0xFFFFFFFF) included - and the hash is a function of the words.
//   host_port_buckets ranges IN OUT: IN holds {bucket_secs, t_lo, t_hi: uint32}; OUT {status, index_lo, index_last, empty}.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../flow-pipeline_amd/csrc/bucket_range.h"
#include "../flow-pipeline_amd/csrc/ports.cuh"

using namespace fa;

int main(int argc, char** argv) {
    if (argc != 4 || (strcmp(argv[1], "keys") && strcmp(argv[1], "ranges"))) {
        fprintf(stderr, "usage: host_port_buckets keys|ranges IN OUT\n");
        return 2;
    }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open files\n");
        return 2;
    }
    unsigned long long fails = 0, n = 0;
    if (!strcmp(argv[1], "keys")) {
        uint8_t rec[24];
        while (fread(rec, 1, 24, in) == 24) {
            uint32_t index, port, bs;
            uint64_t tfs;
            memcpy(&index, rec, 4);
            memcpy(&port, rec + 4, 4);
            memcpy(&bs, rec + 8, 4);
            memcpy(&tfs, rec + 16, 8);
            PKey k, again;
            pkey_pack(index, port, k);
            pkey_pack(index, port, again);
            if (!(k.w[0] >> 63) || !(k.w[1] >> 63) || pkey_empty(k.w[0]) || pkey_empty(k.w[1])) fails++;
            if (pkey_hash(k) != pkey_hash(again)) fails++;
            if ((k.w[0] & ~PKEY_B63) != index || (k.w[1] & ~PKEY_B63) != port) fails++;  // nothing but the flag beside the value
            const uint32_t o[4] = {pkey_bucket(k.w), pkey_port(k.w), port_bucket_index(tfs, bs), 0u};
            if (o[0] != index || o[1] != port) fails++;
            fwrite(o, 4, 4, out);
            n++;
        }
        PSlot zeroed;
        memset(&zeroed, 0, sizeof zeroed);  // what hipMemset leaves: EMPTY in both words
        if (!pkey_empty(zeroed.w[0]) || !pkey_empty(zeroed.w[1])) fails++;
    } else {
        uint32_t rec[3];
        while (fread(rec, 4, 3, in) == 3) {
            BucketRange r;
            const int rc = bucket_range_of(rec[0], rec[1], rec[2], r);
            const uint32_t o[4] = {(uint32_t)rc, r.index_lo, r.index_last, r.empty ? 1u : 0u};
            fwrite(o, 4, 4, out);
            n++;
        }
    }
    fclose(in);
    fclose(out);
    printf(fails ? "FAILED (%llu of %llu)\n" : "OK %llu\n", fails ? fails : n, n);
    return fails ? 1 : 0;
}
