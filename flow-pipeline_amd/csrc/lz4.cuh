// lz4.cuh - LZ4 frames compressed on the device (gfx950): one frame per flows_raw part, one wave per 64 KiB block.
//
// The format, restated from the LZ4 frame format and LZ4 block format specifications:
//   frame  = magic 04 22 4D 18 | FLG 0x60 (version 01, independent blocks, no checksums, no content size, no dictionary) |
//            BD 0x40 (64 KiB blocks) | HC = (xxHash32(FLG BD, seed 0) >> 8) & 0xFF | data blocks | EndMark 00 00 00 00
//   block  = 4-byte little-endian size, then the data; bit 31 of the size set: the data is the input itself ("stored")
//   data   = sequences: token (literal length << 4 | match length - 4, each nibble 15 = "more follows": bytes of 255 and a last
//            one below 255), literals, 2-byte little-endian offset (1 .. 65535), match length bytes.  The last sequence ends
//            behind its literals.  End rules: the last 5 bytes of a block are literals, no match starts within the last 12
//            bytes, so a block under 13 bytes is all literals - and therefore stored here, because it would not shrink.
// Blocks never refer to one another: each decodes alone.
//
// lz4_block_kernel: ONE WAVE compresses one block; LZ4_WAVES waves share a workgroup and nothing else (no barrier in the kernel).
// Search: a table of LZ4_HASH_SIZE 16-bit entries per wave in LDS (8 KiB), entry = position + 1, 0 = empty - so position 0 is
// a candidate like any other.  Each step lane i takes position s + i: loads its 4 bytes, hashes them and reads the table's
// candidate.  A candidate counts only when it is not empty, lies below the lane's position - which puts it inside this block
// and, a block being 64 KiB, at a distance of at most 65535 - and its 4 bytes, read from the block itself, equal the lane's: a
// stale or raced entry can cost ratio, never correctness.  The table of a step holds nothing of that step, so a repetition
// would be seen only 64 positions late - and the parts are columns of 2-, 4-, 8- and 16-byte values whose repetitions are
// short: a lane without a table candidate therefore also compares its 4 bytes with those 1, 2, 4, 8 and 16 positions in
// front of it (the same rule: below the position, inside the block, equal in the block).  __ballot picks the first matching
// lane; then the lanes UP TO it write their positions into the table - every read of a step comes before every write of that
// step, and positions inside a match are not entered, which keeps the 4096 entries for positions a later match can start at.
// (Measured on the mock-shaped part of the tests, on the host: 1.85 without the near candidates, 3.35 with them and every lane
// writing, 3.82 as described - the greedy host encoder gives 3.80.)  The wave extends the match 64 bytes per step (compare,
// ballot, first set bit), emits token, literal length bytes, literals, offset and match length bytes with the lanes sharing the
// bytes, and goes on behind the match.  Without a match all 64 positions are entered and the step moves on by 64.
// Output: the block's slot in scratch (LZ4_BLOCK_MAX bytes).  The room is checked before every sequence against n - 1 bytes -
// a block must SHRINK - and a block that does not fit is marked stored and left.  Nothing is written outside the slot, nothing
// is read outside the block.  Literals and length bytes leave as byte stores (the store form of the measured point).
// INVARIANT (termination): every loop of the kernel advances a wave-uniform position that is bounded by the block's size by at
// least 1 per iteration - the search position `s` (by 64, or to the end of a match of >= 4 bytes that starts at or behind it),
// the match length (by 64 or out of the loop), the per-lane copy indices (by 64).  No loop waits on another wave or on memory.
//
// lz4_pack_kernel: one workgroup per block moves it to its final place (an exclusive scan over the blocks' sizes gave it),
// in front of it the block's size word and, for the first block of a frame, the 7 header bytes; behind the last one the EndMark.
// Stored blocks are copied from the input.
//
// The token / length / end-rule helpers are __host__ __device__: the host encoder (fa_lz4_frame, lz4_host.inc) and the host test
// program (tests/host_lz4.hip) run the code the kernel runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace fa {

constexpr uint32_t LZ4_BLOCK_MAX = 65536;  // input bytes of a block (BD 0x40)
constexpr uint32_t LZ4_HASH_LOG = 12, LZ4_HASH_SIZE = 1u << LZ4_HASH_LOG;
constexpr uint32_t LZ4_WAVES = 4;          // waves (= blocks) per workgroup of lz4_block_kernel
constexpr uint32_t LZ4_NEAR_MAX = 16;      // largest of the near distances 1, 2, 4, 8, 16 a lane tries beside the table
constexpr uint32_t LZ4_MIN_MATCH = 4, LZ4_LAST_LITERALS = 5, LZ4_MF_LIMIT = 12;
constexpr uint32_t LZ4_HEADER_BYTES = 7, LZ4_ENDMARK_BYTES = 4;
constexpr uint32_t LZ4_STORED = 0x80000000u;  // bit 31 of a block's size word
enum { LZ4_F_FIRST = 1, LZ4_F_LAST = 2 };     // Lz4Block::flags: first / last block of its frame; flags >> 2 = the frame's index

// The block plan, built on the host: where a block's input lies and what stands around it in the frame.  The input is given
// as an offset from ONE base pointer that the kernels receive as an argument: a pointer read from memory would make every load
// of the block a flat load (which also occupies the LDS counter), an offset from a kernel argument gives global loads.
struct Lz4Block {
    uint64_t off;
    uint32_t n, flags;
};

// ---- shared with the host ---------------------------------------------------------------------------------------------------------
// a length nibble of 15 is followed by bytes of 255 and a last byte below 255: how many, and the i-th of them
__host__ __device__ inline uint32_t lz4_len_extra(uint32_t x) { return x >= 15 ? 1 + (x - 15) / 255 : 0; }
__host__ __device__ inline uint8_t lz4_len_byte(uint32_t x, uint32_t i) { return i + 1 < lz4_len_extra(x) ? (uint8_t)255 : (uint8_t)((x - 15) % 255); }
// mlen: the match's length (>= 4), or 0 for the last sequence of a block, which has no match
__host__ __device__ inline uint8_t lz4_token(uint32_t lit, uint32_t mlen) {
    const uint32_t m = mlen ? mlen - LZ4_MIN_MATCH : 0;
    return (uint8_t)(((lit < 15 ? lit : 15) << 4) | (m < 15 ? m : 15));
}
__host__ __device__ inline uint32_t lz4_seq_bytes(uint32_t lit, uint32_t mlen) {
    return 1 + lz4_len_extra(lit) + lit + (mlen ? 2 + lz4_len_extra(mlen - LZ4_MIN_MATCH) : 0);
}
// end rules of a block of n bytes: positions 0 .. lz4_match_starts(n) - 1 may start a match (none within the last 12 bytes; 0:
// the block is all literals), and a match ends at or before lz4_match_end(n) (the last 5 bytes are literals)
__host__ __device__ inline uint32_t lz4_match_starts(uint32_t n) { return n > LZ4_MF_LIMIT ? n - LZ4_MF_LIMIT + 1 : 0; }
__host__ __device__ inline uint32_t lz4_match_end(uint32_t n) { return n > LZ4_MF_LIMIT ? n - LZ4_LAST_LITERALS : 0; }
__host__ __device__ inline uint32_t lz4_read32(const uint8_t* p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
__host__ __device__ inline uint32_t lz4_hash(uint32_t v) { return (v * 2654435761u) >> (32 - LZ4_HASH_LOG); }
// Token and literal length bytes at out[0 ..], offset and match length bytes at out[0 ..]: thread `lane` of `lanes` writes its
// share (the host: 0 of 1).  -> bytes written by all of them together.
__host__ __device__ inline uint32_t lz4_put_head(uint8_t* out, uint32_t lit, uint32_t mlen, uint32_t lane, uint32_t lanes) {
    if (lane == 0) out[0] = lz4_token(lit, mlen);
    const uint32_t e = lz4_len_extra(lit);
    for (uint32_t i = lane; i < e; i += lanes) out[1 + i] = lz4_len_byte(lit, i);
    return 1 + e;
}
__host__ __device__ inline uint32_t lz4_put_match(uint8_t* out, uint32_t offset, uint32_t mlen, uint32_t lane, uint32_t lanes) {
    if (lane == 0) out[0] = (uint8_t)offset, out[1] = (uint8_t)(offset >> 8);
    const uint32_t e = lz4_len_extra(mlen - LZ4_MIN_MATCH);
    for (uint32_t i = lane; i < e; i += lanes) out[2 + i] = lz4_len_byte(mlen - LZ4_MIN_MATCH, i);
    return 2 + e;
}
// xxHash32 (restated from the xxHash specification), for the frame header's checksum byte
__host__ __device__ inline uint32_t lz4_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__host__ __device__ inline uint32_t lz4_xxh32(const uint8_t* p, size_t len, uint32_t seed) {
    const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    const uint8_t* end = p + len;
    uint32_t h;
    if (len >= 16) {
        uint32_t v[4] = {seed + P1 + P2, seed + P2, seed, seed - P1};
        for (; p + 16 <= end; p += 16)
            for (int i = 0; i < 4; i++) v[i] = lz4_rotl(v[i] + lz4_read32(p + 4 * i) * P2, 13) * P1;
        h = lz4_rotl(v[0], 1) + lz4_rotl(v[1], 7) + lz4_rotl(v[2], 12) + lz4_rotl(v[3], 18);
    } else
        h = seed + P5;
    h += (uint32_t)len;
    for (; p + 4 <= end; p += 4) h = lz4_rotl(h + lz4_read32(p) * P3, 17) * P4;
    for (; p < end; p++) h = lz4_rotl(h + *p * P5, 11) * P1;
    h ^= h >> 15, h *= P2, h ^= h >> 13, h *= P3, h ^= h >> 16;
    return h;
}
__host__ __device__ inline void lz4_frame_header(uint8_t h[LZ4_HEADER_BYTES]) {
    h[0] = 0x04, h[1] = 0x22, h[2] = 0x4D, h[3] = 0x18, h[4] = 0x60, h[5] = 0x40;
    h[6] = (uint8_t)(lz4_xxh32(h + 4, 2, 0) >> 8);
}

// ---- the block kernel ---------------------------------------------------------------------------------------------------------
// sizes[b]: the block's size word (compressed bytes, or n | LZ4_STORED); val[b]: the bytes the block takes in the output, the
// size word, the frame header in front of a first block and the EndMark behind a last one included (the scan's input).
__global__ __launch_bounds__(64 * LZ4_WAVES) void lz4_block_kernel(const Lz4Block* __restrict__ plan, uint32_t nblocks, const uint8_t* __restrict__ in, uint8_t* __restrict__ slots,
                                                                   uint32_t* __restrict__ sizes, unsigned long long* __restrict__ val) {
    __shared__ __attribute__((aligned(16))) uint16_t tabs[LZ4_WAVES][LZ4_HASH_SIZE];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * LZ4_WAVES + wave;
    if (b >= nblocks) return;  // (the whole wave: b is wave-uniform, and no barrier follows)
    uint16_t* tab = tabs[wave];
    const Lz4Block pb = plan[b];
    const uint8_t* __restrict__ src = in + pb.off;
    const uint32_t n = pb.n;
    uint8_t* out = slots + (size_t)b * LZ4_BLOCK_MAX;
    const uint32_t cap = n ? n - 1 : 0;  // a block that does not shrink is stored
    for (uint32_t i = lane; i < LZ4_HASH_SIZE * 2 / 16; i += 64) ((uint4*)tab)[i] = make_uint4(0, 0, 0, 0);
    __builtin_amdgcn_wave_barrier();

    const uint32_t mstarts = lz4_match_starts(n), mend = lz4_match_end(n);
    uint32_t anchor = 0, s = 0, o = 0;  // first pending literal, search position, bytes written: all wave-uniform
    bool stored = false;
    while (s < mstarts) {  // (s strictly increases: by 64 without a match, to the end of the match otherwise)
        const uint32_t p = s + lane;
        bool hit = false;
        uint32_t ref = 0, h = 0;
        if (p < mstarts) {  // p + 4 <= n - 8: the load stays inside the block
            const uint32_t v = lz4_read32(src + p);
            // the positions the table cannot know yet (comment at the top): the smallest near distance whose 4 bytes equal the
            // lane's, 0 = none.  Branch-free - a distance that would leave the block reads the lane's own position instead - so
            // that the five loads leave together with the first one instead of one memory round trip later.
            uint32_t near = 0;
#pragma unroll
            for (uint32_t d = LZ4_NEAR_MAX; d >= 1; d /= 2) near = (p >= d && lz4_read32(src + (p >= d ? p - d : p)) == v) ? d : near;
            h = lz4_hash(v);
            const uint32_t c = tab[h];
            if (c) {
                ref = c - 1;
                hit = ref < p && lz4_read32(src + ref) == v;
            }
            if (!hit && near) hit = true, ref = p - near;
        }
        const unsigned long long hits = __ballot(hit);
        const uint32_t first = hits ? (uint32_t)__ffsll((long long)hits) - 1 : 63;
        if (p < mstarts && lane <= first) tab[h] = (uint16_t)(p + 1);  // p + 1 <= n - 11 fits 16 bits
        if (!hits) {
            s += 64;
            continue;
        }
        const uint32_t mp = s + first, mref = (uint32_t)__shfl((int)ref, (int)first);
        uint32_t mlen = LZ4_MIN_MATCH;  // mp + 4 <= n - 8 < mend
        for (;;) {                      // (mlen strictly increases and mp + mlen <= mend)
            const uint32_t q = mp + mlen + lane;
            const bool differs = q >= mend || src[q] != src[mref + mlen + lane];
            const unsigned long long d = __ballot(differs);
            if (d) {
                mlen += (uint32_t)__ffsll((long long)d) - 1;
                break;
            }
            mlen += 64;
        }
        const uint32_t lit = mp - anchor;
        if (o + lz4_seq_bytes(lit, mlen) > cap) {
            stored = true;
            break;
        }
        o += lz4_put_head(out + o, lit, mlen, lane, 64);
        for (uint32_t i = lane; i < lit; i += 64) out[o + i] = src[anchor + i];
        o += lit;
        o += lz4_put_match(out + o, mp - mref, mlen, lane, 64);
        anchor = s = mp + mlen;  // > the old s: mp >= s and mlen >= 4
    }
    if (!stored) {  // the last sequence: literals only (at least 5 of them when the block had a match)
        const uint32_t lit = n - anchor;
        if (o + lz4_seq_bytes(lit, 0) > cap)
            stored = true;
        else {
            o += lz4_put_head(out + o, lit, 0, lane, 64);
            for (uint32_t i = lane; i < lit; i += 64) out[o + i] = src[anchor + i];
            o += lit;
        }
    }
    if (lane == 0) {
        sizes[b] = stored ? (n | LZ4_STORED) : o;
        val[b] = 4ull + (stored ? n : o) + ((pb.flags & LZ4_F_FIRST) ? LZ4_HEADER_BYTES : 0) + ((pb.flags & LZ4_F_LAST) ? LZ4_ENDMARK_BYTES : 0);
    }
}

// ---- the pack kernel ---------------------------------------------------------------------------------------------------------
// off[b]: where block b's bytes (header, size word, data, EndMark) start in dst - the exclusive scan of val, off[nblocks] = the
// total.  frame_off[f] receives the start of frame f (its first block writes it), frame_off[nframes] the total and
// frame_off[nframes + 1] the number of stored blocks (zeroed by the host before the launch).
constexpr uint32_t LZ4_PACK_BLOCK = 256;
__global__ __launch_bounds__(LZ4_PACK_BLOCK) void lz4_pack_kernel(const Lz4Block* __restrict__ plan, uint32_t nblocks, const uint8_t* __restrict__ in, const uint8_t* __restrict__ slots,
                                                                  const uint32_t* __restrict__ sizes, const unsigned long long* __restrict__ off,
                                                                  uint32_t nframes, uint8_t* __restrict__ dst,
                                                                  unsigned long long base, unsigned long long* __restrict__ frame_off) {
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= nblocks) return;
    const Lz4Block pb = plan[b];
    const uint32_t word = sizes[b], bytes = word & ~LZ4_STORED;
    const uint8_t* __restrict__ from = (word & LZ4_STORED) ? in + pb.off : slots + (size_t)b * LZ4_BLOCK_MAX;
    uint8_t* to = dst + base + off[b];
    if (pb.flags & LZ4_F_FIRST) {
        if (t == 0) {
            uint8_t h[LZ4_HEADER_BYTES];
            lz4_frame_header(h);
            for (uint32_t i = 0; i < LZ4_HEADER_BYTES; i++) to[i] = h[i];
            frame_off[pb.flags >> 2] = base + off[b];
        }
        to += LZ4_HEADER_BYTES;
    }
    if (t < 4) to[t] = (uint8_t)(word >> (8 * t));
    to += 4;
    // bytes until `to` is 4-byte aligned, then dwords (the source at whatever phase it has), then the rest as bytes
    const uint32_t head = min(bytes, (uint32_t)((4 - ((uintptr_t)to & 3)) & 3));
    if (t < head) to[t] = from[t];
    const uint32_t words = (bytes - head) / 4;
    for (uint32_t i = t; i < words; i += LZ4_PACK_BLOCK) *(uint32_t*)(to + head + 4 * (size_t)i) = lz4_read32(from + head + 4 * (size_t)i);
    const uint32_t done = head + 4 * words;
    if (t < bytes - done) to[done + t] = from[done + t];
    if ((pb.flags & LZ4_F_LAST) && t < LZ4_ENDMARK_BYTES) to[bytes + t] = 0;
    if (t == 0) {
        if (word & LZ4_STORED) atomicAdd(&frame_off[nframes + 1], 1ull);
        if (b == nblocks - 1) frame_off[nframes] = base + off[nblocks];
    }
}

}  // namespace fa
