// host_positions.hip - the device parsers' HOST instantiations (wire.cuh) at absolute positions up to the top of the 32-bit offset
// range.  TEST INFRASTRUCTURE: built and run by tests/test_host_parsers.py (and, before any byte reaches the GPU, by
// tests/test_positions_4gib_gpu.py); links oracle/liboracle.so for the generator only.
//
// The deferred kernel and the ingest kernel's probe run parse_fast through GlobalSrc on positions of the caller's whole batch, which
// may end at 2^32 - 1.  A record is a record wherever it sits, so every tier that takes a Src must give the same verdict and the same
// 15 columns (sure or not) at base 0 and near 2^31 / 2^32, and must read a bounded number of dwords: a cursor step that wraps past
// 2^32 moves the walk back to the start of the batch (parse_fast then walks the whole buffer).  OffSrc serves the record at
// [base, base + n) and zeros elsewhere, counts its reads and ends the program (status 3) past a small cap.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../flow-pipeline_amd/csrc/wire.cuh"
#include "../oracle/flow_oracle.h"

using namespace fa;

static uint64_t rng_state = 0x5eed0b5;
static uint64_t rnd() {
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = rng_state;
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull; z ^= z >> 27; z *= 0x94d049bb133111ebull; z ^= z >> 31;
    return z;
}

static void hexdump(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n && i < 160; i++) printf("%02x", p[i]);
    printf(n > 160 ? "...\n" : "\n");
}

static const char* g_tier = "";  // the tier being run (named when the read cap ends the program)
static uint64_t g_max_reads = 0;

template <bool IS_ABS>
struct OffSrc {
    static constexpr bool ABS = IS_ABS;
    const uint8_t* rec;
    uint64_t base;
    uint32_t n;
    uint64_t* reads;
    uint64_t cap;
    FA_HD uint32_t dw(uint32_t i) const {
        if (++*reads > cap) {
            printf("READ CAP: %s read more than %llu dwords for a record of %u bytes at [%#llx, %#llx) - the cursor wrapped past 2^32\n", g_tier,
                   (unsigned long long)cap, n, (unsigned long long)base, (unsigned long long)(base + n));
            hexdump(rec, n);
            fflush(stdout);
            exit(3);
        }
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; k++) {
            const uint64_t p = (uint64_t)i * 4u + k;
            const uint32_t b = p >= base && p < base + n ? rec[p - base] : 0u;
            v |= b << (8u * k);
        }
        return v;
    }
};

static bool rec_eq(const Rec& a, const Rec& b) {
    return a.time_received == b.time_received && a.time_flow_start == b.time_flow_start && a.sampling_rate == b.sampling_rate &&
           a.bytes == b.bytes && a.packets == b.packets && a.sequence_num == b.sequence_num && a.src_as == b.src_as && a.dst_as == b.dst_as &&
           a.etype == b.etype && a.proto == b.proto && a.src_port == b.src_port && a.dst_port == b.dst_port &&
           memcmp(a.sampler, b.sampler, 16) == 0 && memcmp(a.src, b.src, 16) == 0 && memcmp(a.dst, b.dst, 16) == 0;
}

// every tier's answer for one placement of a record
constexpr int NT = 12;
static const char* TIER_NAMES[NT] = {"parse_canon<ALL>", "parse_canon<ALL,FULL>", "parse_canon<AS_ROLLUP>", "parse_canon<AS_ROLLUP,FULL>",
                                     "parse_tmpl<ALL,MOCKER>", "parse_tmpl<ALL,GOFLOW>", "parse_tmpl<AS_ROLLUP,GOFLOW>", "parse_seq<ALL>",
                                     "parse_fast<ALL>", "parse_fast<AS_ROLLUP>", "seq_learn", "frame_fast+window64"};
struct Answer {
    bool sure[NT];
    Rec r[NT];
    uint32_t learnt, steps[SEQ_MAX], prefix;
};

static uint32_t g_steps[SEQ_MAX];
static uint32_t g_nsteps = 0;

// rec[0, n) at absolute byte position base (base + n <= 2^32 - 1)
template <bool IS_ABS>
static void run_all(const uint8_t* rec, uint32_t n, uint64_t base, Answer& a) {
    uint64_t reads = 0;
    const OffSrc<IS_ABS> s{rec, base, n, &reads, 1024u + 8ull * n};
    const uint32_t pos = (uint32_t)base, end = (uint32_t)(base + n);
    memset(&a, 0, sizeof a);
    auto go = [&](int t, auto fn) {
        g_tier = TIER_NAMES[t];
        reads = 0;
        rec_clear(a.r[t]);
        a.sure[t] = fn(a.r[t]);
        if (reads > g_max_reads) g_max_reads = reads;
    };
    go(0, [&](Rec& r) { return parse_canon<COL_ALL>(s, pos, end, r); });
    go(1, [&](Rec& r) { return parse_canon<COL_ALL, true>(s, pos, end, r); });
    go(2, [&](Rec& r) { return parse_canon<COLS_AS_ROLLUP>(s, pos, end, r); });
    go(3, [&](Rec& r) { return parse_canon<COLS_AS_ROLLUP, true>(s, pos, end, r); });
    go(4, [&](Rec& r) { return parse_tmpl<COL_ALL, SHAPE_MOCKER>(s, pos, end, r); });
    go(5, [&](Rec& r) { return parse_tmpl<COL_ALL, SHAPE_GOFLOW>(s, pos, end, r); });
    go(6, [&](Rec& r) { return parse_tmpl<COLS_AS_ROLLUP, SHAPE_GOFLOW>(s, pos, end, r); });
    go(7, [&](Rec& r) { return g_nsteps ? parse_seq<COL_ALL>(s, pos, end, r, g_steps, g_nsteps) : false; });
    go(8, [&](Rec& r) { return parse_fast<COL_ALL>(s, pos, end, r); });
    go(9, [&](Rec& r) { return parse_fast<COLS_AS_ROLLUP>(s, pos, end, r); });
    go(10, [&](Rec&) {
        a.learnt = seq_learn(s, pos, end, a.steps);
        return a.learnt != 0;
    });
    go(11, [&](Rec&) { return frame_fast(window64(s, pos), end - pos, a.prefix); });
}

struct Stats {
    uint64_t records = 0, placements = 0, fail = 0, fast_sure = 0;
};

static bool same_answer(const Answer& x, const Answer& y, int& tier) {
    for (int t = 0; t < NT; t++) {
        tier = t;
        if (x.sure[t] != y.sure[t] || !rec_eq(x.r[t], y.r[t])) return false;
    }
    tier = 10;
    if (x.learnt != y.learnt || memcmp(x.steps, y.steps, sizeof x.steps) != 0) return false;
    tier = 11;
    return !x.sure[11] || x.prefix == y.prefix;
}

// the record at base 0 (both source kinds) and at the top of the offset range: the same answers everywhere
static void check(const uint8_t* rec, uint32_t n, Stats& st) {
    Answer ref, abs0, at;
    run_all<false>(rec, n, 0, ref);
    run_all<true>(rec, n, 0, abs0);
    st.records++;
    st.fast_sure += ref.sure[8];
    int tier = 0;
    if (!same_answer(ref, abs0, tier)) {
        if (st.fail++ < 20) { printf("MISMATCH %s: ABS source at base 0 differs (n=%u): ", TIER_NAMES[tier], n); hexdump(rec, n); }
    }
    const uint64_t top = 0xFFFFFFFFull;
    const uint64_t k = rnd() % 64;
    const uint64_t bases[] = {(1ull << 31) - k, (1ull << 31) - n / 2, (1ull << 31), (1ull << 32) - (1ull << 20) - k, (1ull << 32) - (1ull << 20) - n,
                              (1ull << 32) - 4096, (1ull << 32) - 4096 - k, top - n - (rnd() % 9), top - n};
    for (uint64_t b : bases) {
        run_all<true>(rec, n, b, at);
        st.placements++;
        if (!same_answer(ref, at, tier)) {
            if (st.fail++ < 20) {
                printf("MISMATCH %s at pos %#llx end %#llx (n=%u): sure %d vs %d at base 0: ", TIER_NAMES[tier], (unsigned long long)b,
                       (unsigned long long)(b + n), n, at.sure[tier], ref.sure[tier]);
                hexdump(rec, n);
            }
        }
    }
}

static size_t put_varint(uint8_t* p, uint64_t v) {
    size_t k = 0;
    while (v >= 0x80) { p[k++] = (uint8_t)(v | 0x80); v >>= 7; }
    p[k++] = (uint8_t)v;
    return k;
}

int main(int argc, char** argv) {
    const uint64_t iters = argc > 1 ? strtoull(argv[1], 0, 0) : 3000;
    Stats gen, mut, trunc, wrap;
    // 1. generator output of every mode (MOCKER, ASPAIRS, ZIPF, GOFLOW, DISTINCT, REVERSED), framed and bare; byte mutations;
    //    truncations at every length of a few records
    for (uint32_t mode = 0; mode < 6; mode++) {
        fo_gen_params gp;
        memset(&gp, 0, sizeof gp);
        gp.mode = mode; gp.framed = mode & 1; gp.seed = 21 + mode; gp.n_total = iters; gp.t0 = 1600000200; gp.span_secs = 900; gp.per_sec = 4;
        gp.zipf_log2_universe = 20; gp.zipf_s_x100 = 110;
        std::vector<uint8_t> buf(iters * 220 + 1024);
        std::vector<uint64_t> off(iters + 1);
        if (fo_gen_records(&gp, 0, iters, buf.data(), buf.size(), off.data()) == (size_t)-1) { printf("generator overflow\n"); return 2; }
        g_nsteps = 0;
        for (uint64_t i = 0; i < iters; i++) {
            const uint8_t* r = buf.data() + off[i];
            const uint32_t n = (uint32_t)(off[i + 1] - off[i]);
            if (i == 0) {  // the learnt order of this stream (parse_seq's steps): learnt at base 0, walked everywhere
                uint64_t reads = 0;
                const OffSrc<false> s{r, 0, n, &reads, ~0ull};
                uint32_t pl = 0;
                const uint32_t p0 = gp.framed && frame_fast(window64(s, 0), n, pl) ? pl : 0u;
                g_nsteps = seq_learn(s, p0, n, g_steps);
            }
            check(r, n, gen);
            uint8_t tmp[512];
            uint32_t m = n;
            memcpy(tmp, r, n);
            const uint32_t kind = (uint32_t)(rnd() % 5);
            if (kind == 0) tmp[rnd() % m] = (uint8_t)rnd();
            if (kind == 1) tmp[rnd() % m] ^= (uint8_t)(1u << (rnd() & 7));
            if (kind == 2) m = (uint32_t)(rnd() % (m + 1));
            if (kind == 3) { const uint32_t e = (uint32_t)(rnd() % 8 + 1); for (uint32_t j = 0; j < e; j++) tmp[m++] = (uint8_t)rnd(); }
            if (kind == 4) { const uint32_t x = (uint32_t)(rnd() % m), y = (uint32_t)(rnd() % m); std::swap(tmp[x], tmp[y]); }
            check(tmp, m, mut);
            if (i < 4)
                for (uint32_t t = 0; t < n; t++) check(r, t, trunc);
        }
    }
    // 2. records built to wrap: a truncated LEN field claiming up to 2^20 - 1 bytes behind a valid prefix (field 100, above every
    //    schema field, and the projected bytes fields), and varints with no stop byte in their window in every walk's step shapes
    {
        fo_gen_params gp;
        memset(&gp, 0, sizeof gp);
        gp.mode = 3; gp.framed = 0; gp.seed = 99; gp.n_total = 64; gp.t0 = 1600000200; gp.span_secs = 900; gp.per_sec = 4;
        std::vector<uint8_t> buf(64 * 220 + 1024);
        std::vector<uint64_t> off(65);
        fo_gen_records(&gp, 0, 64, buf.data(), buf.size(), off.data());
        const uint32_t claims[] = {0xFFFF0u, 0xFFFFFu, 0xFFF00u, 0x80000u, 4096u, 4097u, 40000u, 17u, 0xFFFFFu - 7u};
        const uint32_t len_tags[] = {(100u << 3) | 2u, (6u << 3) | 2u, (11u << 3) | 2u, (2047u << 3) | 2u, (1000u << 3) | 2u};
        // varint fields of every step shape (1- and 2-byte tags, projected or not, 4- and 8-byte windows)
        const uint32_t var_tags[] = {1u << 3, 2u << 3, 3u << 3, 4u << 3, 9u << 3, 14u << 3, 15u << 3, 20u << 3, 21u << 3, 27u << 3, 30u << 3,
                                     38u << 3, 42u << 3, 50u << 3, 100u << 3, 2047u << 3};
        for (uint64_t i = 0; i < iters; i++) {
            const uint8_t* r = buf.data() + off[i % 64];
            const uint32_t rn = (uint32_t)(off[i % 64 + 1] - off[i % 64]);
            uint8_t tmp[512];
            uint32_t pre = (uint32_t)(rnd() % (rn + 1));
            if ((rnd() & 3) == 0) pre = rn;
            memcpy(tmp, r, pre);
            uint32_t m = pre;
            if (i & 1) {
                m += (uint32_t)put_varint(tmp + m, len_tags[rnd() % 5]);
                const uint32_t claim = (rnd() & 1) ? claims[rnd() % 9] : (uint32_t)(rnd() % (1u << 20));
                m += (uint32_t)put_varint(tmp + m, claim);
                const uint32_t have = (uint32_t)(rnd() % 24);
                for (uint32_t j = 0; j < have && j < claim; j++) tmp[m++] = (uint8_t)rnd();
            } else {
                m += (uint32_t)put_varint(tmp + m, var_tags[rnd() % 16] | ((rnd() & 7) == 0 ? 1u : 0u));
                const uint32_t cont = 1 + (uint32_t)(rnd() % 12);
                for (uint32_t j = 0; j < cont; j++) tmp[m++] = (uint8_t)(0x80u | rnd());
                if (rnd() & 1) { for (uint32_t j = 0; j < 4; j++) tmp[m++] = (uint8_t)(rnd() & 0x7f); }  // garbage behind it, then the end
            }
            check(tmp, m, wrap);
        }
        // the case that wrapped parse_fast on the way here: 48 bytes, field 100 claiming 0xFFFF0 bytes
        uint8_t t48[64];
        uint32_t m = 0;
        m += (uint32_t)put_varint(t48 + m, 2u << 3);
        m += (uint32_t)put_varint(t48 + m, 1600000300u);
        while (m < 40) { t48[m++] = 0x48; t48[m++] = 0x05; }
        m += (uint32_t)put_varint(t48 + m, (100u << 3) | 2u);
        m += (uint32_t)put_varint(t48 + m, 0xFFFF0u);
        while (m < 48) t48[m++] = 0xab;
        check(t48, m, wrap);
    }
    auto pr = [](const char* name, const Stats& s) {
        printf("%-24s records=%llu placements=%llu fast_sure=%llu FAIL=%llu\n", name, (unsigned long long)s.records, (unsigned long long)s.placements,
               (unsigned long long)s.fast_sure, (unsigned long long)s.fail);
    };
    pr("generator (6 modes)", gen);
    pr("mutated", mut);
    pr("truncated", trunc);
    pr("built to wrap", wrap);
    printf("max dwords read by one call: %llu\n", (unsigned long long)g_max_reads);
    const uint64_t fails = gen.fail + mut.fail + trunc.fail + wrap.fail;
    printf(fails ? "FAILED\n" : "OK\n");
    return fails ? 1 : 0;
}
