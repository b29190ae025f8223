// host_framing_positions.hip - device framing's position arithmetic (framing.cuh) compiled for the host, at stream lengths up to
// the top of the 32-bit offset range.  TEST INFRASTRUCTURE: built and run by tests/test_host_parsers.py.
//
// fa_ingest_device without offsets takes len < 2^32 - 1: the last block of such a stream may end above 2^32 - FS_BLOCK, where
// begin + FS_BLOCK and the stage's slack wrap past 2^32.  Checked for every len in (2^32 - FS_BLOCK - 300, 2^32 - 2]:
//   - the emit pass's sub-block ranges (fs_sub_end) of the last two blocks tile [begin, end) exactly;
//   - the stage's "inside the stream" test (fs_in_stream) never admits a position >= len and admits every one below;
//   - a chain of frames ending at len, walked block by block through fs_walk_block and emitted sub-block by sub-block the way
//     fs_emit_kernel does, gives the frames of the same chain at base 0 (fewer lens: every one near the ends, every 256-byte step).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../flow-pipeline_amd/csrc/framing.cuh"

using namespace fa;

static uint64_t rng_state = 0xf4a3e;
static uint64_t rnd() {
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = rng_state;
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull; z ^= z >> 27; z *= 0x94d049bb133111ebull; z ^= z >> 31;
    return z;
}

static uint64_t fails = 0;
#define FAIL(...) do { if (fails++ < 20) { printf(__VA_ARGS__); printf("\n"); } } while (0)

// the chain's bytes at [base, base + n), zeros elsewhere
struct OffBytes {
    const uint8_t* p;
    uint64_t base, n;
    FA_HD uint8_t operator[](uint32_t q) const { return q >= base && q < base + n ? p[q - base] : 0; }
};

// frame starts of the chain as the device finds them: walk every block the chain touches from the previous block's exit, then
// emit each present sub-block's frames up to its end
static bool device_split(const OffBytes& b, uint32_t len, std::vector<uint64_t>& starts, uint32_t& frames) {
    starts.clear();
    frames = 0;
    const uint64_t nb = ((uint64_t)len + FS_BLOCK - 1) / FS_BLOCK;
    uint32_t from = (uint32_t)b.base;
    for (uint64_t blk = b.base / FS_BLOCK; blk < nb; blk++) {
        const uint32_t begin = (uint32_t)(blk * FS_BLOCK), end = blk + 1 == nb ? len : (uint32_t)((blk + 1) * FS_BLOCK);
        uint32_t cnt = 0, exit_ = 0;
        uint8_t err = 0;
        alignas(8) uint8_t ent8[FS_NSUB];
        unsigned long long present = 0;
        memset(ent8, 0, sizeof ent8);
        fs_walk_block(b, len, begin, end, from, &cnt, &err, &exit_, ent8, &present);
        if (err) { FAIL("len %#x block %#x: the walk met a malformed frame", len, begin); return false; }
        frames += cnt;
        uint32_t emitted = 0;
        for (uint32_t j = 0; j < FS_NSUB; j++) {
            if (!((present >> j) & 1ull)) continue;
            const uint32_t sub_end = fs_sub_end(begin, j, end);
            for (uint32_t p = begin + j * FS_SUB + ent8[j]; p < sub_end; p = fs_next(b, p, len)) {
                starts.push_back(p);
                emitted++;
            }
        }
        if (emitted != cnt) { FAIL("len %#x block %#x: the walk counted %u frames, the emit pass finds %u", len, begin, cnt, emitted); return false; }
        from = exit_;
    }
    if (from != len) { FAIL("len %#x: the chain's walk exits at %#x", len, from); return false; }
    return true;
}

int main() {
    const uint64_t top = 0xFFFFFFFEull;  // the largest len the offsets-free path accepts
    const uint64_t lo = (1ull << 32) - FS_BLOCK - 300;
    // 1. sub-block ranges and the stage predicate, every len
    uint64_t lens = 0;
    for (uint64_t len = lo + 1; len <= top; len++, lens++) {
        const uint64_t nb = (len + FS_BLOCK - 1) / FS_BLOCK;
        for (uint64_t blk = nb >= 2 ? nb - 2 : 0; blk < nb; blk++) {
            const uint64_t begin = blk * FS_BLOCK, end = blk + 1 == nb ? len : (blk + 1) * FS_BLOCK;
            uint64_t prev = begin;
            for (uint32_t j = 0; j < FS_NSUB; j++) {
                const uint64_t want = begin + (uint64_t)(j + 1) * FS_SUB < end ? begin + (uint64_t)(j + 1) * FS_SUB : end;
                const uint32_t got = fs_sub_end((uint32_t)begin, j, (uint32_t)end);
                if (got != want || got < prev) { FAIL("fs_sub_end: len %#llx block %#llx sub-block %u ends at %#x, not %#llx", (unsigned long long)len, (unsigned long long)begin, j, got, (unsigned long long)want); break; }
                prev = got;
            }
            if (prev != end) FAIL("fs_sub_end: len %#llx block %#llx: the sub-blocks end at %#llx, not at the block's end", (unsigned long long)len, (unsigned long long)begin, (unsigned long long)prev);
            // the emit pass stages FS_BLOCK + FS_SLACK bytes, the guess FS_STAGE + FS_STAGE_PAD, in pieces of 16
            const bool dense = len - lo < 600 || top - len < 600 || len % 256 < 2;
            for (uint32_t i = 0; i < FS_BLOCK + FS_SLACK; i += dense ? 1u : 16u) {
                const bool in = fs_in_stream((uint32_t)begin, i, (uint32_t)len);
                if (in != (begin + i < len)) { FAIL("fs_in_stream: len %#llx lo %#llx i %u says %d", (unsigned long long)len, (unsigned long long)begin, i, in); break; }
            }
        }
    }
    // 2. a chain of frames (prefix of 1..3 bytes, payloads of 0..700 bytes - some longer than a sub-block) ending at len
    std::vector<uint8_t> chain;
    std::vector<uint64_t> truth;
    while (chain.size() < 3 * FS_BLOCK) {
        truth.push_back(chain.size());
        const uint32_t pl = (rnd() & 7) == 0 ? (uint32_t)(rnd() % 700) : (uint32_t)(rnd() % 200);
        uint32_t v = pl;
        while (v >= 0x80) { chain.push_back((uint8_t)(v | 0x80)); v >>= 7; }
        chain.push_back((uint8_t)v);
        for (uint32_t k = 0; k < pl; k++) chain.push_back((uint8_t)rnd());
    }
    const uint64_t n = chain.size();
    std::vector<uint64_t> starts;
    uint32_t frames = 0;
    {
        const OffBytes b0{chain.data(), 0, n};
        if (!device_split(b0, (uint32_t)n, starts, frames) || frames != truth.size() || starts != truth) FAIL("the chain at base 0: %u frames, %zu expected", frames, truth.size());
    }
    uint64_t walked = 0;
    for (uint64_t len = lo + 1; len <= top; len++) {
        const bool dense = len - lo < 300 || top - len < 300 || len % 256 < 2 || len % 256 > 253;
        if (!dense && (rnd() & 63) != 0) continue;
        const OffBytes b{chain.data(), len - n, n};
        if (!device_split(b, (uint32_t)len, starts, frames)) continue;
        walked++;
        bool same = frames == truth.size() && starts.size() == truth.size();
        for (size_t i = 0; same && i < truth.size(); i++) same = starts[i] == truth[i] + (len - n);
        if (!same) FAIL("the chain ending at len %#llx: %u frames (%zu emitted), %zu at base 0", (unsigned long long)len, frames, starts.size(), truth.size());
    }
    printf("lens=%llu chains_walked=%llu frames_per_chain=%zu FAIL=%llu\n", (unsigned long long)lens, (unsigned long long)walked, truth.size(), (unsigned long long)fails);
    printf(fails ? "FAILED\n" : "OK\n");
    return fails ? 1 : 0;
}
