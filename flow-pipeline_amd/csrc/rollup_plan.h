// rollup_plan.h - what the host decides for a rollup fold from columns (rollup_host.inc; device side: rollup.cuh): which key sets a
// call may ask for, and how many records one launch may take.  Host only, no HIP: tests/host_rollup.hip runs both without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/flowagg.h"

namespace fa {

constexpr uint32_t ROLLUP_EXACT_SETS = FA_KEYS_AS_PAIR | FA_KEYS_ADDR_PORT_PROTO | FA_KEYS_PORT_HIST | FA_KEYS_MINUTE_SERIES;
constexpr uint32_t ROLLUP_SKETCH_SETS = FA_KEYS_SRCADDR_CMS | FA_KEYS_DSTADDR_CMS;

// The key sets a call folds: `asked` == 0 means every exact key set the ctx was created with (`ctx_sets` = fa_config.key_sets);
// otherwise a subset of those.  FA_OK and *out, or: FA_ERR_UNSUPPORTED for a sketch bit (the rollup doors do not feed the sketches:
// sketch_plan.h, fa_sketch_fold_columns_device / fa_raw_restore) and for a ctx without any exact key set, FA_ERR_ARG for any other
// bit the ctx was not created with.
inline int rollup_mask_check(uint32_t ctx_sets, uint32_t asked, uint32_t* out) {
    *out = 0;
    if (asked & ROLLUP_SKETCH_SETS) return FA_ERR_UNSUPPORTED;
    const uint32_t have = ctx_sets & ROLLUP_EXACT_SETS;
    if (asked & ~have) return FA_ERR_ARG;
    if (!have) return FA_ERR_UNSUPPORTED;
    *out = asked ? asked : have;
    return FA_OK;
}

// Updates ONE record can park when every upsert meets a full table.  flows_5m: one - a record either leaves on its own or as part
// of a group of the workgroup's LDS table, and a group holds at least one record that parked nothing else.  Wide table: one
// (SrcAddr,DstPort,Proto) row, one hashed key per port >= 65536 (both directions), one minute (on its own or through LdsMinutes).
inline uint32_t rollup_as_updates(uint32_t ks) { return (ks & FA_KEYS_AS_PAIR) ? 1u : 0u; }
inline uint32_t rollup_wide_updates(uint32_t ks) {
    return ((ks & FA_KEYS_ADDR_PORT_PROTO) ? 1u : 0u) + ((ks & FA_KEYS_PORT_HIST) ? 2u : 0u) + ((ks & FA_KEYS_MINUTE_SERIES) ? 1u : 0u);
}

// Records of one launch: if every upsert of the chunk parks, both spill buffers still hold them - with the 2^20 entries the
// launch guard (pre_launch_guard) keeps free left free while the buffer is large enough to spare them: a call that folds every
// exact key set of its ctx then passes the guard without a settle per chunk (the guard counts the ctx's key sets, not the
// call's).  At most max_batch_records; never 0.
constexpr uint32_t ROLLUP_GUARD_SLACK = 1u << 20;
inline size_t rollup_chunk_cap(uint32_t spill_cap, uint32_t wspill_cap, uint32_t max_batch_records, uint32_t ks) {
    auto room = [](uint32_t cap) { return cap > 2u * ROLLUP_GUARD_SLACK ? cap - ROLLUP_GUARD_SLACK : cap; };
    size_t m = std::max<uint32_t>(max_batch_records, 1u);
    if (rollup_as_updates(ks)) m = std::min<size_t>(m, room(spill_cap) / rollup_as_updates(ks));
    if (rollup_wide_updates(ks)) m = std::min<size_t>(m, room(wspill_cap) / rollup_wide_updates(ks));
    return std::max<size_t>(m, 1);
}

}  // namespace fa
