// host_launch_plan.hip - the plain-value functions behind a launch's plan (csrc/launch_plan.h), run on the host.
// TEST INFRASTRUCTURE (tests/test_launch_plan_cpu.py).  No GPU call.  Prints, one line each:
//   variant M V            ks_variant(M) for every mask 0..63 - and with_variant's constant for that value
//   stride M S             wt_stride(ks_variant(M)) for M = 1, 9, 7, 63
//   wg N v1 v2 ...         tile_recs_for(mean * N, N) for mean = 1..6000
//   wt M N v1 v2 ...       wtile_recs_for(mean * N, N, ks_variant(M)) for mean = 1..6000
#include <cstdio>

#include "../flow-pipeline_amd/csrc/launch_plan.h"

using namespace fa;

int main() {
    const uint32_t masks[4] = {1u, 9u, 7u, 63u};
    const size_t ns[6] = {1, 63, 64, 65, 256, 4096};
    for (uint32_t m = 0; m < 64; m++) {
        const uint32_t v = ks_variant(m);
        if (with_variant(v, [](auto k) { return (uint32_t) decltype(k)::value; }) != v) return 1;
        printf("variant %u %u\n", m, v);
    }
    for (uint32_t m : masks) printf("stride %u %d\n", m, wt_stride(ks_variant(m)));
    for (size_t n : ns) {
        printf("wg %zu", n);
        for (size_t mean = 1; mean <= 6000; mean++) printf(" %u", tile_recs_for(mean * n, n));
        printf("\n");
    }
    for (uint32_t m : masks)
        for (size_t n : ns) {
            printf("wt %u %zu", m, n);
            for (size_t mean = 1; mean <= 6000; mean++) printf(" %u", wtile_recs_for(mean * n, n, ks_variant(m)));
            printf("\n");
        }
    return 0;
}
