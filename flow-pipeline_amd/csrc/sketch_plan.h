// sketch_plan.h - what the host decides for a sketch fold from columns and for a restore from parts (sketch_fold_host.inc; device
// side: sketch_fold.cuh): which key sets a call may ask for, and how many records one chunk may take.  Host only, no HIP:
// tests/host_sketch_plan.hip runs all of it without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/flowagg.h"
#include "rollup_plan.h"

namespace fa {

// The sketches a call folds into: `asked` == 0 means every sketch the ctx was created with (`created` = fa_config.key_sets);
// otherwise a subset of those.  FA_OK and *sets, or: FA_ERR_ARG for any bit that is not a sketch of this ctx - an exact key set,
// a sketch the ctx was created without, a bit above the six -, FA_ERR_UNSUPPORTED for asked == 0 on a ctx without any sketch.
inline int sketch_mask_check(uint32_t created, uint32_t asked, uint32_t* sets) {
    *sets = 0;
    const uint32_t have = created & ROLLUP_SKETCH_SETS;
    if (asked & ~have) return FA_ERR_ARG;
    if (!have) return FA_ERR_UNSUPPORTED;
    *sets = asked ? asked : have;
    return FA_OK;
}

// fa_raw_restore: `asked` == 0 means everything the ctx was created with, exact key sets and sketches alike; otherwise a subset.
// FA_OK with the two halves (either may be 0: the caller knows whether a fold is selected beside them), or FA_ERR_ARG for a bit
// the ctx was not created with.
inline int restore_mask_check(uint32_t created, uint32_t asked, uint32_t* exact, uint32_t* sets) {
    *exact = *sets = 0;
    const uint32_t have = created & (ROLLUP_EXACT_SETS | ROLLUP_SKETCH_SETS);
    if (asked & ~have) return FA_ERR_ARG;
    const uint32_t take = asked ? asked : have;
    *exact = take & ROLLUP_EXACT_SETS;
    *sets = take & ROLLUP_SKETCH_SETS;
    return FA_OK;
}

// Records of one sketch-fold launch.  A chunk IS a batch of the candidates contract (include/flowagg.h, fa_config.topk_mode): at
// most max_batch_records, as an ingest launch; the kernel parks nothing, so no spill buffer has a say.  Never 0.
inline size_t sketch_chunk_cap(uint32_t max_batch_records) { return std::max<uint32_t>(max_batch_records, 1u); }

// The chunk of fa_raw_restore: the smallest cap among the selected destinations (0 = that destination is not selected); 0 only
// when none is.
inline size_t restore_chunk_cap(size_t rollup_cap, size_t sketch_cap, size_t talk_cap, size_t port_cap) {
    size_t m = 0;
    for (size_t cap : {rollup_cap, sketch_cap, talk_cap, port_cap})
        if (cap) m = m ? std::min(m, cap) : cap;
    return m;
}

}  // namespace fa
