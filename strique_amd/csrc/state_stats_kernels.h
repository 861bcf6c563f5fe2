// Internal: state statistics of traced windows (not part of the C ABI; strq_set_state_stats and strq_viterbi_state_stats in
// strique_hip.h, strique_amd/state_stats.py states the rule).  The decode itself is the back-pointer decode of the Viterbi kernels and
// launch_vit_traceback;
//   state_stats_kernel -- per emitting state the count, the sum and the sum of squares of the observations the best path assigns to it,
//                         accumulated in ascending observation order, one addition each, no contraction: defined to the bit
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "viterbi_kernels.h"

namespace strq {

// One traced window, beside its VitTask (same index): `path` = the emitting state of every observation (launch_vit_traceback), `result`
// the VitResult of the back-pointer decode (device).  n / sum / sumsq: the window's three rows of n_emit entries; every entry is written
// (a state the path never visits: 0, +0.0, +0.0).  *bad is set to 1, and the rows are zero, when the decode found no path or the path
// names a state outside [0, n_emit).
struct StateStatsTask {
    const int32_t* path;
    const void* result;
    int64_t* n; double* sum; double* sumsq;
    int32_t n_emit, pad_;
    int32_t* bad;
};
#define STATE_STATS_MAX_EMIT 4096      // VIT_CSR_MAX_STATES: 24 B per emitting state, 96 KB of LDS with one wave per workgroup
// One wave (and one workgroup) per window, the accumulators of `max_emit` states in LDS.  0 ok, 1 launch failed, 2 max_emit out of range.
int launch_state_stats(hipStream_t s, const VitTask* vit, const StateStatsTask* tasks, int n, int max_emit);

}  // namespace strq
