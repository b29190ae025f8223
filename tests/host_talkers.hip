// host_talkers.hip - host instantiation of the top talkers' group key (talkers.cuh: talker_canon, tkey_pack / tkey_unpack).
// TEST INFRASTRUCTURE (tests/test_talkers_cpu.py).  No GPU call.
//   host_talkers IN OUT: IN holds records of 16 address bytes + a little-endian uint32 EType; OUT receives, per record, the
//   canonical key's 16 bytes + a little-endian uint32 family.  The key words of the table are packed and unpacked on the
//   way (a round trip that must not change anything, and words that must never be 0 = EMPTY).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../flow-pipeline_amd/csrc/talkers.cuh"

using namespace fa;

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: host_talkers IN OUT\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open files\n");
        return 2;
    }
    uint8_t rec[20];
    unsigned long long fails = 0, n = 0;
    while (fread(rec, 1, 20, in) == 20) {
        uint32_t etype;
        memcpy(&etype, rec + 16, 4);
        uint64_t lo, hi;
        uint32_t fam;
        talker_canon(rec, etype, &lo, &hi, &fam);
        TKey k;
        tkey_pack(lo, hi, fam, k);
        if (!k.w[0] || !k.w[1] || !k.w[2]) fails++;
        unsigned long long lo2, hi2;
        uint32_t fam2;
        tkey_unpack(k.w, lo2, hi2, fam2);
        if (lo2 != lo || hi2 != hi || fam2 != fam) fails++;
        uint8_t o[20];
        memcpy(o, &lo2, 8);
        memcpy(o + 8, &hi2, 8);
        memcpy(o + 16, &fam2, 4);
        fwrite(o, 1, 20, out);
        n++;
    }
    fclose(in);
    fclose(out);
    printf(fails ? "FAILED (%llu of %llu)\n" : "OK %llu\n", fails ? fails : n, n);
    return fails ? 1 : 0;
}
