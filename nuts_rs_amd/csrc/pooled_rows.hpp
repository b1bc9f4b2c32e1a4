// pooled_rows.hpp — what the units of the pooled adaptation share (pooled_reduce.hip, pooled_scatter.hip): the ONE rule by which a
// recorded row counts, and the error text behind nm_pooled_last_error.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "../../include/nuts_amd.h"

namespace nm {
namespace pooled {
// The reference's DrawGradCollector (src/transform/adapt/diagonal.rs:57-84): the chain is healthy and the draw `is_good`
// (index_in_trajectory != 0, or |index| > 4 for a divergent draw).  Rows of chains that stopped are never written by the engine and carry
// all-zero statistics in a zero-initialised buffer, which this rule rejects.  No statistics: every row counts.
__device__ inline bool row_ok(const nm_draw_stats* st, uint64_t row) {
    if (!st) return true;
    const nm_draw_stats& s = st[row];
    if (s.chain_status != NM_CHAIN_OK) return false;
    const int64_t idx = s.index_in_trajectory;
    return s.diverging ? ((idx < 0 ? -idx : idx) > 4) : (idx != 0);
}
// the calling thread's message for nm_pooled_last_error (defined in pooled_reduce.hip)
void set_error(const std::string& msg);
}  // namespace pooled
}  // namespace nm
