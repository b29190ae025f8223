// lz4_decode.cuh - LZ4 frames decoded on the device (gfx950): the inverse of lz4.cuh, one wave per block of at most 64 KiB.
//
// The format is restated at the top of lz4.cuh.  The host walks the frames (lz4_walk_frames, raw_load_host.inc: one size word
// per block) and builds the plan: where a block's bytes lie - an offset from ONE base pointer passed as a kernel argument, so the
// loads are global loads (lz4.cuh, at Lz4Block) - and where its 64 KiB slot lies.  Block j of frame f decodes into the slot at
// base_f + j * 65536, base_f a multiple of 65536; every block of a frame but the last must decode to exactly 65536 bytes (the
// host checks the sizes the kernel reports), so a frame's decoded bytes are contiguous without a pack pass.
//
// lz4_decode_kernel: ONE WAVE decodes one block; LZ4D_WAVES waves share a workgroup and nothing else - no LDS, no barrier, no
// wave waits on another.  Per sequence every lane runs lz4_seq_parse (the SAME function the host twin fa_lz4_decode and
// tests/host_lz4_decode.hip run) on wave-uniform arguments: token, length bytes, offset, and every bound below.  Then the lanes
// share the literals (lane i copies bytes i, i + 64, ...) and the match: byte j of the match is out[pos - offset + (j % offset)],
// which for EVERY offset - overlapping (offset < match length) or not - lies in front of the match, in bytes that were stored
// before the match began.  A lane keeps j % offset as a running remainder (+ 64 % offset per step, one conditional subtraction).
// A stored block is copied with aligned 16-byte stores (the slot is 64 KiB-aligned) and ALIGNED 16-byte loads: the two aligned
// words that cover a chunk's source bytes, shifted by the source's byte phase (bytes16_at_phase; one word when the source is
// 16-byte aligned); the first and last chunk, which aligned loads would overshoot, leave as single-byte copies.  The sequence
// parser and the literal and match copies issue single-byte loads and stores only (checked in the ISA).
//
// BOUNDS (the contract: nothing is read outside the block's n input bytes or its slot, nothing is written outside its slot,
// whatever the input holds).  lz4_seq_parse refuses, before anything of the sequence is copied: a token or a length byte behind
// the input's end; literals > input left; decoded + literals > 65536; a missing 2-byte offset; offset == 0 or offset > decoded;
// decoded + match > 65536; a last sequence (the one whose literals end the input) whose token carries a match length.  An input
// that ends behind a match has no last sequence: the next parse finds no token.  On a refusal lane 0 records the reason code
// and the input position in the block's status word and the wave leaves: no trap, no assert.
// INVARIANT (termination): every loop advances a wave-uniform position that is bounded by the block's input size or by 65536 by
// at least 1 per iteration - the input position (a sequence is at least its token), the length chains (one input byte each),
// the copy indices (by 64).  No loop waits on another wave or on memory.
// VISIBILITY: the match source is the slot the wave has just written, and lanes are separate threads: a byte stored by lane a
// is read by lane b.  What makes the read see the store is the HARDWARE's order, not a wait: outside threadgroup-split mode (the
// library is not built with -mtgsplit) the waves of a workgroup share one L1, and the vector memory operations of one wave are
// performed at it in the order the wave issued them, so a load issued behind a store of the same wave to the same address
// returns the stored byte (the rule the LLVM AMDGPU memory model for gfx90a / gfx942 / gfx950 relies on when it asks nothing
// for vector memory at workgroup scope outside tgsplit mode).  Between the stores of a sequence's literals (and of the sequences
// before it) and the loads of its match stands a workgroup-scope acq_rel fence: it keeps the COMPILER from moving the loads in
// front of the stores or reusing a value it loaded earlier, and it compiles to NO instruction for these accesses - checked in
// the ISA built with the library's flags: no s_waitcnt vmcnt stands between the literals' global_store_byte and the match's
// first global_load_ubyte.  The match itself needs no fence between its steps: it reads only bytes in front of the match
// (above).  The slot is reached through a plain uint8_t* - no __restrict__, no const - so the compiler may not keep its values
// across the fence.  The input is never written and is __restrict__.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "align16.cuh"
#include "lz4.cuh"

namespace fa {

constexpr uint32_t LZ4D_WAVES = 4;  // waves (= blocks) per workgroup of lz4_decode_kernel

// why a block was refused (Lz4DecStatus::code; the texts: lz4d_reason)
enum {
    LZ4D_OK = 0,
    LZ4D_E_TOKEN = 1,      // the input ends where a sequence's token is expected (also: the input ends behind a match)
    LZ4D_E_LENGTH = 2,     // a length chain runs past the input's end
    LZ4D_E_LITERALS = 3,   // literals run past the input's end
    LZ4D_E_SIZE = 4,       // the block decodes to more than 65536 bytes
    LZ4D_E_NO_OFFSET = 5,  // the input ends inside a 2-byte offset
    LZ4D_E_OFFSET = 6,     // offset 0, or an offset larger than the bytes decoded in this block
    LZ4D_E_LAST_MATCH = 7, // the last sequence carries a match length
};
__host__ __device__ inline const char* lz4d_reason(uint32_t code) {
    switch (code) {
    case LZ4D_E_TOKEN: return "truncated (a sequence's token is missing)";
    case LZ4D_E_LENGTH: return "a length chain runs past the block's end";
    case LZ4D_E_LITERALS: return "literals run past the block's end";
    case LZ4D_E_SIZE: return "decodes to more than 65536 bytes";
    case LZ4D_E_NO_OFFSET: return "truncated offset";
    case LZ4D_E_OFFSET: return "offset 0 or an offset larger than the bytes decoded (blocks must decode alone)";
    case LZ4D_E_LAST_MATCH: return "the last sequence carries a match length";
    default: return "ok";
    }
}

// One sequence of a block of n input bytes, starting at input position p with `decoded` bytes out: what to copy, or why not.
struct Lz4Seq {
    uint32_t lit, lit_at;   // literals: how many, where in the input
    uint32_t offset, mlen;  // the match (mlen 0: the last sequence, which has none)
    uint32_t next;          // input position behind the sequence
    uint32_t err, err_at;   // LZ4D_E_*, and the input position it was found at
};
__host__ __device__ inline Lz4Seq lz4_seq_fail(uint32_t code, uint32_t at) { return Lz4Seq{0, 0, 0, 0, 0, code, at}; }
__host__ __device__ inline Lz4Seq lz4_seq_parse(const uint8_t* src, uint32_t n, uint32_t p, uint32_t decoded) {
    if (p >= n) return lz4_seq_fail(LZ4D_E_TOKEN, p);
    const uint32_t token = src[p++];
    uint32_t lit = token >> 4;
    if (lit == 15)
        for (;;) {  // (p strictly increases and stays below n)
            if (p >= n) return lz4_seq_fail(LZ4D_E_LENGTH, p);
            const uint32_t b = src[p++];
            lit += b;
            if (b != 255) break;
        }
    if (lit > n - p) return lz4_seq_fail(LZ4D_E_LITERALS, p);
    if (lit > LZ4_BLOCK_MAX - decoded) return lz4_seq_fail(LZ4D_E_SIZE, p);
    Lz4Seq q{lit, p, 0, 0, p + lit, LZ4D_OK, 0};
    p += lit;
    if (p == n) {  // the last sequence ends exactly at the input's end and has no match
        if (token & 15) return lz4_seq_fail(LZ4D_E_LAST_MATCH, q.lit_at - 1);
        return q;
    }
    if (n - p < 2) return lz4_seq_fail(LZ4D_E_NO_OFFSET, p);
    q.offset = (uint32_t)src[p] | ((uint32_t)src[p + 1] << 8);
    const uint32_t off_at = p;
    p += 2;
    uint32_t mlen = (token & 15) + LZ4_MIN_MATCH;
    if ((token & 15) == 15)
        for (;;) {
            if (p >= n) return lz4_seq_fail(LZ4D_E_LENGTH, p);
            const uint32_t b = src[p++];
            mlen += b;
            if (b != 255) break;
        }
    if (q.offset == 0 || q.offset > decoded + lit) return lz4_seq_fail(LZ4D_E_OFFSET, off_at);
    if (mlen > LZ4_BLOCK_MAX - decoded - lit) return lz4_seq_fail(LZ4D_E_SIZE, off_at);
    q.mlen = mlen;
    q.next = p;
    return q;
}

// The host's copy of one sequence (fa_lz4_decode, tests/host_lz4_decode.hip): out[decoded ..] receives literals and match.
inline void lz4_seq_copy_host(const uint8_t* src, const Lz4Seq& q, uint8_t* out, uint32_t decoded) {
    for (uint32_t i = 0; i < q.lit; i++) out[decoded + i] = src[q.lit_at + i];
    const uint32_t at = decoded + q.lit;
    for (uint32_t j = 0; j < q.mlen; j++) out[at + j] = out[at - q.offset + j];  // (byte by byte: an overlapping match repeats itself)
}
// One compressed block -> out (LZ4_BLOCK_MAX bytes of room); -> LZ4D_E_*, *size = the decoded bytes, *at = the error's position.
inline uint32_t lz4_block_decode_host(const uint8_t* src, uint32_t n, uint8_t* out, uint32_t* size, uint32_t* at) {
    uint32_t p = 0, o = 0;
    for (;;) {
        const Lz4Seq q = lz4_seq_parse(src, n, p, o);
        if (q.err) {
            *size = o, *at = q.err_at;
            return q.err;
        }
        lz4_seq_copy_host(src, q, out, o);
        o += q.lit + q.mlen;
        p = q.next;
        if (!q.mlen) break;
    }
    *size = o, *at = p;
    return LZ4D_OK;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------
enum { LZ4D_F_STORED = 1 };
struct Lz4DBlock {
    uint64_t in_off;   // the block's data (behind its size word), from the kernel's `in`
    uint64_t out_off;  // its slot, from the kernel's `out`: a multiple of LZ4_BLOCK_MAX
    uint32_t n, flags;
};
struct Lz4DecStatus {
    uint32_t code, at, size, _pad;  // LZ4D_E_* and the input position it was found at; the bytes decoded
};

// ---- host only: the frame walk and the twin (fa_lz4_decode, the device doors' plan, tests/host_lz4_decode.hip) -----------------
struct Lz4WalkBlock {
    size_t at;  // the block's data in the input (behind its size word)
    uint32_t n, frame;
    bool stored;
};
struct Lz4Walk {
    std::vector<Lz4WalkBlock> blocks;
    std::vector<uint32_t> first;  // first[f]: frame f's first block; first[frames]: the number of blocks
};
inline std::string lz4_at_byte(const std::string& what, size_t p) { return what + " at byte " + std::to_string(p); }
// A concatenation of frames -> its blocks.  Refuses what spill.lz4_frames_decode refuses, and a block of more than 65536 bytes
// (the slot a block decodes into).  false: *err names the reason and the byte.
inline bool lz4_walk_frames(const uint8_t* b, size_t n, Lz4Walk& w, std::string* err) {
    size_t p = 0;
    auto no = [&](const char* what, size_t at) {
        *err = lz4_at_byte(what, at);
        return false;
    };
    while (p < n) {
        if (n - p >= 4) {
            const uint32_t magic = lz4_read32(b + p);
            if (magic >= 0x184D2A50u && magic <= 0x184D2A5Fu) return no("LZ4 stream: a skippable frame (the library writes none)", p);
        }
        if (n - p < 4 || memcmp(b + p, "\x04\x22\x4d\x18", 4)) return no("LZ4 stream: no frame magic", p);
        if (n - p < LZ4_HEADER_BYTES) return no("LZ4 stream: truncated frame header", p);
        const uint8_t flg = b[p + 4], bd = b[p + 5], hc = b[p + 6];
        if (flg >> 6 != 1) return no("LZ4 frame: a version other than 01", p + 4);
        if (!(flg & 0x20)) return no("LZ4 frame: linked blocks (the library writes independent blocks, each decodes alone)", p + 4);
        if (flg & 0x10) return no("LZ4 frame: block checksums (the library writes none)", p + 4);
        if (flg & 0x08) return no("LZ4 frame: a content size (the library writes none)", p + 4);
        if (flg & 0x04) return no("LZ4 frame: a content checksum (the library writes none)", p + 4);
        if (flg & 0x01) return no("LZ4 frame: a dictionary id (the library writes none)", p + 4);
        if ((flg & 0x02) || (bd & 0x8F) || (bd >> 4) < 4) return no("LZ4 frame: reserved bits set or an invalid block size id", p + 4);
        if ((uint8_t)(lz4_xxh32(b + p + 4, 2, 0) >> 8) != hc) return no("LZ4 frame: the header checksum does not match FLG / BD", p + 6);
        p += LZ4_HEADER_BYTES;
        const uint32_t f = (uint32_t)w.first.size();
        w.first.push_back((uint32_t)w.blocks.size());
        for (;;) {
            if (n - p < 4) return no("LZ4 stream: truncated (no EndMark)", p);
            const uint32_t word = lz4_read32(b + p);
            p += 4;
            if (word == 0) break;
            const uint32_t size = word & ~LZ4_STORED;
            if (size > LZ4_BLOCK_MAX) return no(("LZ4 frame: a block of " + std::to_string(size) + " bytes, the maximum is 65536").c_str(), p - 4);
            if (size > n - p) return no("LZ4 stream: truncated block", p);
            if (w.blocks.size() >= ((size_t)1 << 30)) return no("LZ4 stream: more than 2^30 blocks in one call", p);
            w.blocks.push_back({p, size, f, (word & LZ4_STORED) != 0});
            p += size;
        }
    }
    w.first.push_back((uint32_t)w.blocks.size());
    return true;
}
// what the blocks' statuses - the kernel's or the twin's - say about frame f: every block decoded, every block but the last to
// exactly 65536 bytes.  -> *bytes: the frame's decoded size
inline bool lz4_frame_verdict(const Lz4Walk& w, uint32_t f, const Lz4DecStatus* st, uint64_t* bytes, std::string* err) {
    *bytes = 0;
    for (uint32_t b = w.first[f]; b < w.first[f + 1]; b++) {
        if (st[b].code) return *err = lz4_at_byte(std::string("LZ4 block: ") + lz4d_reason(st[b].code), w.blocks[b].at + st[b].at), false;
        if (b + 1 < w.first[f + 1] && st[b].size != LZ4_BLOCK_MAX)
            return *err = lz4_at_byte("LZ4 frame: a block of " + std::to_string(st[b].size) + " decoded bytes that is not the last of its frame (every block but the last holds 65536)",
                                      w.blocks[b].at),
                   false;
        *bytes += st[b].size;
    }
    return true;
}
// The twin: a concatenation of frames -> their decoded bytes.  Every block is decoded into a buffer of exactly 65536 bytes.
inline bool lz4_frames_decode_host(const uint8_t* in, size_t n, std::vector<uint8_t>& out, std::string* err) {
    Lz4Walk w;
    out.clear();
    if (!lz4_walk_frames(in, n, w, err)) return false;
    std::vector<std::vector<uint8_t>> slot(w.blocks.size());
    std::vector<Lz4DecStatus> st(w.blocks.size());
    for (size_t b = 0; b < w.blocks.size(); b++) {
        const Lz4WalkBlock& k = w.blocks[b];
        slot[b].resize(LZ4_BLOCK_MAX);
        st[b] = Lz4DecStatus{LZ4D_OK, k.n, k.n, 0};
        if (k.stored) memcpy(slot[b].data(), in + k.at, k.n);
        else st[b].code = lz4_block_decode_host(in + k.at, k.n, slot[b].data(), &st[b].size, &st[b].at);
    }
    for (uint32_t f = 0; f + 1 < w.first.size(); f++) {
        uint64_t bytes;
        if (!lz4_frame_verdict(w, f, st.data(), &bytes, err)) return false;
        for (uint32_t b = w.first[f]; b < w.first[f + 1]; b++) out.insert(out.end(), slot[b].begin(), slot[b].begin() + st[b].size);
    }
    return true;
}

// ---- the kernel ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64 * LZ4D_WAVES) void lz4_decode_kernel(const Lz4DBlock* __restrict__ plan, uint32_t nblocks, const uint8_t* __restrict__ in, uint8_t* out_base,
                                                                     Lz4DecStatus* __restrict__ status) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * LZ4D_WAVES + wave;
    if (b >= nblocks) return;  // (the whole wave: b is wave-uniform, and no barrier follows)
    const Lz4DBlock pb = plan[b];
    const uint8_t* __restrict__ src = in + pb.in_off;
    uint8_t* out = out_base + pb.out_off;  // 64 KiB-aligned (the host lays the slots out)
    const uint32_t n = pb.n;
    if (pb.flags & LZ4D_F_STORED) {  // n <= LZ4_BLOCK_MAX: the host refused anything larger
        const uint32_t sh = (uint32_t)((uintptr_t)src & 15);
        // chunk k = bytes [16 k, 16 k + 16): its aligned words - one at src + 16 k when sh == 0, else the two from src + 16 k - sh
        // on - lie inside [src, src + n) when first <= k < last
        const uint32_t first = sh ? 1 : 0, last = sh ? (n + sh >= 32 ? (n + sh - 16) / 16 : 0) : n / 16;
        for (uint32_t k = first + lane; k < last; k += 64) {
            const uint8_t* al = src + 16 * k - sh;  // 16-byte aligned; >= src: k >= 1 where sh != 0; al + 32 <= src + n: k < last
            const uint4 x = *(const uint4*)al;
            const uint4 y = sh ? *(const uint4*)(al + 16) : make_uint4(0, 0, 0, 0);
            *(uint4*)(out + 16 * k) = bytes16_at_phase(x, y, sh);
        }
        const uint32_t head = min(n, first * 16), tail = max(head, last * 16);
        for (uint32_t i = lane; i < head; i += 64) out[i] = src[i];
        for (uint32_t i = tail + lane; i < n; i += 64) out[i] = src[i];
        if (lane == 0) status[b] = Lz4DecStatus{LZ4D_OK, n, n, 0};
        return;
    }
    uint32_t p = 0, o = 0;  // input position, bytes decoded: wave-uniform
    for (;;) {              // (p strictly increases: a sequence is at least its token)
        const Lz4Seq q = lz4_seq_parse(src, n, p, o);
        if (q.err) {
            if (lane == 0) status[b] = Lz4DecStatus{q.err, q.err_at, o, 0};
            return;
        }
        for (uint32_t i = lane; i < q.lit; i += 64) out[o + i] = src[q.lit_at + i];
        o += q.lit;
        p = q.next;
        if (!q.mlen) break;
        // the match reads what this wave has stored, other lanes' bytes included (VISIBILITY at the top)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const uint8_t* from = out + (o - q.offset);
        const uint32_t step = 64 % q.offset;
        uint32_t r = q.offset >= 64 ? lane : lane % q.offset;  // (j % offset) of this lane's byte j = lane, lane + 64, ...
        for (uint32_t j = lane; j < q.mlen; j += 64) {
            out[o + j] = from[r];  // from + r < out + o: in front of the match
            r += step;
            if (r >= q.offset) r -= q.offset;
        }
        o += q.mlen;
    }
    if (lane == 0) status[b] = Lz4DecStatus{LZ4D_OK, p, o, 0};
}

}  // namespace fa
