// host_segwalk.hip - the segment geometry of the scatter sinks' tuples (csrc/segwalk.cuh), run on the host.
// TEST INFRASTRUCTURE (tests/test_segwalk_cpu.py).  No GPU call.  For BACK in {0, 1}, TPL in {1, 2}, capq in
// {2 TPL, 8, 40, 64, 130} and every count c in [0, capq] it enumerates lanes 0..63 at levels 0..seg_levels_of(c) - 1 and
// checks THE RULE: every tuple of the part [first, first + c), first = BACK ? capq - c : 0, is valid exactly once (per
// segment of the load: a back load covers eight), nothing outside the part is, every piece lies inside the segment, and
// the three levels from seg_levels_of(c) on mark nothing.  Prints, one line each:
//   levels BACK TPL C L                      seg_levels_of<BACK, TPL>(C), C in [0, 130]
//   piece BACK TPL CAPQ C J LANE PIECE VALID seg_piece<BACK, TPL>(CAPQ, C, J, LANE) (capq <= 40 only)
//   geom BACK TPL CAPQ CASES TUPLES FAILS    counts checked, tuples marked valid, violations of the rule
// and exits 1 when any rule is violated (the first violations go to stderr).
#include <cstdio>
#include <vector>

#include "../flow-pipeline_amd/csrc/segwalk.cuh"

using namespace fa;

static unsigned long long g_fails = 0;
static void fail(const char* what, bool back, int tpl, uint32_t capq, uint32_t c, uint32_t j, uint32_t lane, uint32_t q) {
    if (g_fails++ < 20) fprintf(stderr, "%s: back %d tpl %d capq %u c %u level %u lane %u tuple %u\n", what, (int)back, tpl, capq, c, j, lane, q);
}

template <bool BACK, int TPL>
static void check(uint32_t capq) {
    constexpr uint32_t SEGS = seg_per_load<BACK>();
    const unsigned long long fails0 = g_fails;
    unsigned long long tuples = 0;
    for (uint32_t c = 0; c <= capq; c++) {
        const uint32_t first = BACK ? capq - c : 0u, levels = seg_levels_of<BACK, TPL>(c);
        std::vector<uint32_t> seen((size_t)SEGS * capq, 0u);  // times tuple q of the load's segment k was valid
        for (uint32_t j = 0; j < levels + 3u; j++)
            for (uint32_t lane = 0; lane < 64u; lane++) {
                const SegPiece p = seg_piece<BACK, TPL>(capq, c, j, lane);
                const uint32_t k = seg_of_lane<BACK>(lane);
                if (capq <= 40u) printf("piece %d %d %u %u %u %u %u %u\n", (int)BACK, TPL, capq, c, j, lane, p.piece, p.valid);
                if (k >= SEGS) fail("segment of the lane outside the load", BACK, TPL, capq, c, j, lane, k);
                if (p.piece >= capq / TPL) fail("piece outside the segment", BACK, TPL, capq, c, j, lane, p.piece * TPL);
                if (p.valid >> TPL) fail("valid bit beyond the piece", BACK, TPL, capq, c, j, lane, p.valid);
                if (!p.valid && p.piece) fail("dummy load not at piece 0", BACK, TPL, capq, c, j, lane, p.piece * TPL);
                if (j >= levels && p.valid) fail("tuple at a level the count does not have", BACK, TPL, capq, c, j, lane, p.piece * TPL);
                for (uint32_t t = 0; t < (uint32_t)TPL; t++) {
                    if (!((p.valid >> t) & 1u)) continue;
                    const uint32_t q = p.piece * TPL + t;
                    if (q >= capq || k >= SEGS) fail("tuple outside the segment", BACK, TPL, capq, c, j, lane, q);
                    else seen[(size_t)k * capq + q]++;
                }
            }
        for (uint32_t k = 0; k < SEGS; k++)
            for (uint32_t q = 0; q < capq; q++) {
                const uint32_t want = q >= first && q < first + c ? 1u : 0u, got = seen[(size_t)k * capq + q];
                tuples += got;
                if (got != want) fail(want ? (got ? "tuple visited more than once" : "tuple never visited") : "tuple outside the part visited", BACK, TPL, capq, c, k, 0, q);
            }
    }
    printf("geom %d %d %u %u %llu %llu\n", (int)BACK, TPL, capq, capq + 1u, tuples, g_fails - fails0);
}

template <bool BACK, int TPL>
static void all() {
    for (uint32_t c = 0; c <= 130u; c++) printf("levels %d %d %u %u\n", (int)BACK, TPL, c, seg_levels_of<BACK, TPL>(c));
    const uint32_t capqs[5] = {2u * TPL, 8u, 40u, 64u, 130u};
    for (uint32_t capq : capqs) check<BACK, TPL>(capq);
}

int main() {
    all<false, 1>();
    all<false, 2>();
    all<true, 1>();
    all<true, 2>();
    return g_fails ? 1 : 0;
}
