// host_talker_buckets.hip - host instantiation of the bucketed talker key (talkers.cuh: tkey_pack_bucket / tkey_bucket / tkey_unpack).
// TEST INFRASTRUCTURE (tests/test_talker_buckets_cpu.py).  No GPU call.
//   host_talker_buckets IN OUT: IN holds records of 16 address bytes + a little-endian uint32 EType + a little-endian uint32
//   bucket index; OUT receives, per record, what the packed key words give back: the canonical key's 16 bytes, the family and
//   the bucket index (little-endian uint32 each).  On the way: every key word keeps bit 63 (never 0 = EMPTY), the bucket
//   changes no bit outside its field, and index 0 packs to exactly the words of the plain tkey_pack.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../flow-pipeline_amd/csrc/talkers.cuh"

using namespace fa;

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: host_talker_buckets IN OUT\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open files\n");
        return 2;
    }
    uint8_t rec[24];
    unsigned long long fails = 0, n = 0;
    while (fread(rec, 1, 24, in) == 24) {
        uint32_t etype, index;
        memcpy(&etype, rec + 16, 4);
        memcpy(&index, rec + 20, 4);
        uint64_t lo, hi;
        uint32_t fam;
        talker_canon(rec, etype, &lo, &hi, &fam);
        TKey plain, k, zero;
        tkey_pack(lo, hi, fam, plain);
        tkey_pack_bucket(lo, hi, fam, index, k);
        tkey_pack_bucket(lo, hi, fam, 0u, zero);
        for (int j = 0; j < 3; j++) {
            if (!(k.w[j] >> 63)) fails++;
            if (zero.w[j] != plain.w[j]) fails++;
        }
        const unsigned long long field = 0xFFFFFFFFull << TKEY_BUCKET_SHIFT;
        if (k.w[0] != plain.w[0] || k.w[1] != plain.w[1] || (k.w[2] & ~field) != plain.w[2] || (plain.w[2] & field)) fails++;
        unsigned long long lo2, hi2;
        uint32_t fam2;
        tkey_unpack(k.w, lo2, hi2, fam2);
        const uint32_t index2 = tkey_bucket(k.w);
        if (lo2 != lo || hi2 != hi || fam2 != fam || index2 != index) fails++;
        uint8_t o[24];
        memcpy(o, &lo2, 8);
        memcpy(o + 8, &hi2, 8);
        memcpy(o + 16, &fam2, 4);
        memcpy(o + 20, &index2, 4);
        fwrite(o, 1, 24, out);
        n++;
    }
    fclose(in);
    fclose(out);
    printf(fails ? "FAILED (%llu of %llu)\n" : "OK %llu\n", fails ? fails : n, n);
    return fails ? 1 : 0;
}
