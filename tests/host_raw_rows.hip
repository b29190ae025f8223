// host_raw_rows.hip - host instantiation of raw_rows_from_bytes (csrc/raw.cuh), the size -> rows rule that
// raw_header_check_kernel runs on the device for every part it is given.  TEST INFRASTRUCTURE (tests/test_raw_load_cpu.py).
// No GPU call.
//   host_raw_rows IN OUT: IN holds sizes (uint64); OUT receives per size {fits: uint64 (0 / 1), rows: uint64 (0 when it does not)}.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../flow-pipeline_amd/csrc/raw.cuh"

using namespace fa;

int main(int argc, char** argv) {
    FILE* in = argc == 3 ? fopen(argv[1], "rb") : nullptr;
    FILE* out = argc == 3 ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) {
        fprintf(stderr, "usage: host_raw_rows IN OUT\n");
        return 2;
    }
    unsigned long long n = 0;
    uint64_t size;
    while (fread(&size, 8, 1, in) == 1) {
        uint64_t o[2] = {0, 0};
        o[0] = raw_rows_from_bytes(RAW_COLS_H, size, &o[1]) ? 1 : 0;
        if (!o[0]) o[1] = 0;
        fwrite(o, 8, 2, out);
        n++;
    }
    fclose(in);
    fclose(out);
    printf("OK %llu\n", n);
    return 0;
}
