// host_lz4_decode.hip - host instantiation of what lz4_decode_kernel and the host twin fa_lz4_decode share (csrc/lz4_decode.cuh):
// the per-sequence step function lz4_seq_parse, the frame walk and the twin over them.  TEST INFRASTRUCTURE
// (tests/test_raw_load_cpu.py), built once plain and once with the host's AddressSanitizer and UBSan.  No GPU call.
// Every input is copied into a heap block of exactly its size and every block decodes into a heap block of exactly 65536 bytes
// (lz4_frames_decode_host), so a read or write outside either is a sanitizer report.
//   host_lz4_decode cases IN: IN holds records {frame bytes: uint32, expected bytes: uint32 (0xFFFFFFFF: the frames must be
//   refused), the frames, the expected bytes}.  Each is decoded by the twin AND, block by block, by a second loop over
//   lz4_seq_parse that copies nothing and only adds up the sizes; both must agree with the record and with each other.
//   host_lz4_decode mutate IN SEED COUNT: IN holds records of valid frames (expected bytes ignored); COUNT seeded mutations -
//   byte flips, truncations, size-word edits - of them are decoded: each is refused or decodes to at most 65536 bytes per block.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../flow-pipeline_amd/csrc/lz4_decode.cuh"

using namespace fa;

struct Record {
    std::vector<uint8_t> frames, expect;
    bool refuse;
};

static bool read_records(const char* path, std::vector<Record>& out) {
    FILE* in = fopen(path, "rb");
    if (!in) return false;
    uint32_t h[2];
    while (fread(h, 4, 2, in) == 2) {
        Record r;
        r.refuse = h[1] == 0xFFFFFFFFu;
        r.frames.resize(h[0]);
        r.expect.resize(r.refuse ? 0 : h[1]);
        if ((h[0] && fread(r.frames.data(), 1, h[0], in) != h[0]) || (!r.expect.empty() && fread(r.expect.data(), 1, r.expect.size(), in) != r.expect.size())) {
            fclose(in);
            return false;
        }
        out.push_back(std::move(r));
    }
    fclose(in);
    return true;
}

// the sizes alone, by the step function: -> false when a block is refused; *total = the decoded bytes of all blocks
static bool sizes_by_steps(const std::vector<uint8_t>& f, uint64_t* total, uint32_t* largest) {
    Lz4Walk w;
    std::string err;
    *total = 0, *largest = 0;
    if (!lz4_walk_frames(f.data(), f.size(), w, &err)) return false;
    for (size_t b = 0; b < w.blocks.size(); b++) {
        const Lz4WalkBlock& k = w.blocks[b];
        uint32_t o = k.n;
        if (!k.stored) {
            std::vector<uint8_t> src(f.begin() + k.at, f.begin() + k.at + k.n);  // exactly the block's input
            uint32_t p = 0;
            o = 0;
            for (;;) {
                const Lz4Seq q = lz4_seq_parse(src.data(), k.n, p, o);
                if (q.err) return false;
                if (q.next <= p || q.next > k.n || (uint64_t)q.lit_at + q.lit > k.n) abort();  // the step function's own promises
                if (q.mlen && (q.offset == 0 || q.offset > o + q.lit)) abort();
                o += q.lit + q.mlen;
                if (o > LZ4_BLOCK_MAX) abort();
                p = q.next;
                if (!q.mlen) break;
            }
            if (p != k.n) abort();  // the last sequence ends exactly at the input's end
        }
        const bool last = b + 1 == w.blocks.size() || w.blocks[b + 1].frame != k.frame;
        if (!last && o != LZ4_BLOCK_MAX) return false;
        *total += o;
        if (o > *largest) *largest = o;
    }
    return true;
}

static uint64_t rng_state;
static uint32_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 2685821657736338717ull) >> 32);
}

int main(int argc, char** argv) {
    const bool cases = argc == 3 && !strcmp(argv[1], "cases"), mutate = argc == 5 && !strcmp(argv[1], "mutate");
    std::vector<Record> recs;
    if ((!cases && !mutate) || !read_records(argv[2], recs) || recs.empty()) {
        fprintf(stderr, "usage: host_lz4_decode cases IN | mutate IN SEED COUNT\n");
        return 2;
    }
    unsigned long long fails = 0, n = 0, refused = 0;
    std::string err;
    std::vector<uint8_t> got;
    if (cases) {
        for (size_t i = 0; i < recs.size(); i++, n++) {
            const Record& r = recs[i];
            const bool ok = lz4_frames_decode_host(r.frames.data(), r.frames.size(), got, &err);
            uint64_t total;
            uint32_t largest;
            const bool ok2 = sizes_by_steps(r.frames, &total, &largest);
            bool good = ok == ok2 && ok != r.refuse;
            if (ok && good) good = got == r.expect && total == got.size();
            if (!ok) refused++;
            if (!good) {
                fails++;
                fprintf(stderr, "case %zu: twin %d (%s), steps %d, refusal expected %d, %zu bytes for %zu\n", i, (int)ok, err.c_str(), (int)ok2, (int)r.refuse, got.size(), r.expect.size());
            }
        }
    } else {
        rng_state = strtoull(argv[3], nullptr, 0) * 0x9E3779B97F4A7C15ull + 1;
        const unsigned long long count = strtoull(argv[4], nullptr, 0);
        for (; n < count; n++) {
            const Record& r = recs[rng() % recs.size()];
            std::vector<uint8_t> f = r.frames;
            const uint32_t kind = rng() % 4;
            if (kind == 0 && !f.empty()) {  // a few byte flips
                for (uint32_t k = 1 + rng() % 4; k; k--) f[rng() % f.size()] ^= (uint8_t)(1u << (rng() % 8));
            } else if (kind == 1 && !f.empty()) {  // a random byte
                f[rng() % f.size()] = (uint8_t)rng();
            } else if (kind == 2) {  // a truncation
                f.resize(rng() % (f.size() + 1));
            } else if (f.size() >= 11) {  // the first block's size word
                const uint32_t edits[] = {0, 1, 65535, 65536, 65537, 0x80000000u, 0x80000001u, 0x80010001u, 0xFFFFFFFFu, rng(), rng() % 70000};
                const uint32_t v = edits[rng() % (sizeof edits / sizeof *edits)];
                memcpy(f.data() + 7, &v, 4);
            }
            std::vector<uint8_t> exact(f);  // a heap block of exactly the mutated size
            exact.shrink_to_fit();
            const bool ok = lz4_frames_decode_host(exact.data(), exact.size(), got, &err);
            uint64_t total;
            uint32_t largest;
            const bool ok2 = sizes_by_steps(exact, &total, &largest);
            if (!ok) refused++;
            if (ok != ok2 || (ok && (total != got.size() || largest > LZ4_BLOCK_MAX))) fails++;
        }
    }
    printf(fails ? "FAILED (%llu of %llu)\n" : "OK %llu refused %llu\n", fails ? fails : n, fails ? n : refused);
    return fails ? 1 : 0;
}
