// host_lz4.hip - host instantiation of what lz4_block_kernel and the host encoder share (csrc/lz4.cuh): token, length bytes,
// offset (lz4_put_head / lz4_put_match / lz4_seq_bytes), the end rules (lz4_match_starts / lz4_match_end) and the frame header.
// TEST INFRASTRUCTURE (tests/test_raw_lz4_cpu.py).  No GPU call.
//   host_lz4 emit IN OUT: IN holds records of {literals, match length (0: the last sequence, no match), offset: uint32}; OUT
//   receives per record {bytes: uint32} and the sequence - token, literal length bytes, the literals (byte i = (7 i + 3) & 255),
//   offset, match length bytes - written once by one thread (0 of 1) and once by 64 "lanes" in reverse order, which must agree
//   with each other and with lz4_seq_bytes (checked here; the bytes are compared with a statement in the test).
//   host_lz4 rules IN OUT: IN holds block sizes (uint32); OUT {lz4_match_starts, lz4_match_end: uint32}.
//   host_lz4 header OUT: the 7 header bytes.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../flow-pipeline_amd/csrc/lz4.cuh"

using namespace fa;

static uint32_t sequence(uint8_t* out, uint32_t lit, uint32_t mlen, uint32_t offset, uint32_t lanes, bool reverse) {
    uint32_t o = 0, head = 0, tail = 0;
    for (uint32_t k = 0; k < lanes; k++) head = lz4_put_head(out + o, lit, mlen, reverse ? lanes - 1 - k : k, lanes);
    o += head;
    for (uint32_t i = 0; i < lit; i++) out[o + i] = (uint8_t)(7 * i + 3);
    o += lit;
    if (mlen) {
        for (uint32_t k = 0; k < lanes; k++) tail = lz4_put_match(out + o, offset, mlen, reverse ? lanes - 1 - k : k, lanes);
        o += tail;
    }
    return o;
}

int main(int argc, char** argv) {
    const bool emit = argc == 4 && !strcmp(argv[1], "emit"), rules = argc == 4 && !strcmp(argv[1], "rules"), header = argc == 3 && !strcmp(argv[1], "header");
    if (!emit && !rules && !header) {
        fprintf(stderr, "usage: host_lz4 emit|rules IN OUT | header OUT\n");
        return 2;
    }
    FILE* in = header ? nullptr : fopen(argv[2], "rb");
    FILE* out = fopen(argv[header ? 2 : 3], "wb");
    if ((!header && !in) || !out) {
        fprintf(stderr, "cannot open files\n");
        return 2;
    }
    unsigned long long fails = 0, n = 0;
    if (emit) {
        uint32_t rec[3];
        while (fread(rec, 4, 3, in) == 3) {
            const uint32_t need = lz4_seq_bytes(rec[0], rec[1]);
            std::vector<uint8_t> a(need, 0xEE), b(need, 0xDD);  // exactly the room the kernel checks for
            const uint32_t na = sequence(a.data(), rec[0], rec[1], rec[2], 1, false), nb = sequence(b.data(), rec[0], rec[1], rec[2], 64, true);
            if (na != need || nb != need || a != b) fails++;
            fwrite(&na, 4, 1, out);
            fwrite(a.data(), 1, na, out);
            n++;
        }
    } else if (rules) {
        uint32_t size;
        while (fread(&size, 4, 1, in) == 1) {
            const uint32_t o[2] = {lz4_match_starts(size), lz4_match_end(size)};
            fwrite(o, 4, 2, out);
            n++;
        }
    } else {
        uint8_t h[LZ4_HEADER_BYTES];
        lz4_frame_header(h);
        fwrite(h, 1, sizeof h, out);
        n = 1;
    }
    if (in) fclose(in);
    fclose(out);
    printf(fails ? "FAILED (%llu of %llu)\n" : "OK %llu\n", fails ? fails : n, n);
    return fails ? 1 : 0;
}
