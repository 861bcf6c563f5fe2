// Internal: tract pass of the detect pipeline (not part of the C ABI; strq_set_tracts in strique_hip.h, strique_amd/tracts.py states
// the rule).  The decode itself is the count decode of the Viterbi kernels with the wide payload (launch_viterbi's `tracts`);
//   tract_task_kernel -- the Viterbi tasks of the eligible reads of a sub-batch, once the host has grouped them by kernel shape:
//                        the window [prefix_begin, suffix_end) of the count decode on the slot's filtered signal, from the read's
//                        geometry and conditioning record
//   tract_scan_kernel -- the unit positions of every tract (strq_set_tract_positions) from the state path of a back-pointer decode
//                        of the same window: one ballot per tract and 64 observations
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cond_kernels.h"
#include "scan_kernels.h"
#include "viterbi_kernels.h"

namespace strq {

// task k of the pass: read[k] of the sub-batch, decoded with model[k] (the compound model of its target); written to vit[k]
struct TractTaskArgs {
    const ReadGeom* geom; const ReadCond* rc;
    const int32_t* read; const VitModel* const* model;
    const void* flt; int is_f64;
    PoreStats ps;
    VitTask* vit;
    int n_tasks, n_reads;
};
int launch_tract_tasks(hipStream_t s, const TractTaskArgs& a);

// One traced window: the observations t of the best path that emit from a counted state of tract j, written as base + t (ascending)
// to out[off[j] .. off[j] + n[j]).  `path` = the emitting state of every observation (launch_vit_traceback), `tract_inc` the model's
// increments (VitModel::tract_inc: tract of a state = ctz(inc) / VIT_TRACT_BITS, 0 = none; n_states + 1 entries), n[j] the visits the
// count decode of the same window found.  *bad is set to 1 when the back-pointer decode found no path or a tract does not give exactly
// n[j]; nothing is stored beyond n[j].
struct TractScanTask {
    const int32_t* path;
    const uint64_t* tract_inc;
    const void* result;      // VitResult of the back-pointer decode (device)
    int64_t* out;
    int64_t T, base;
    int64_t off[VIT_TRACTS_MAX], n[VIT_TRACTS_MAX];
    int32_t n_tracts, n_states;
    int32_t* bad;
};
int launch_tract_scan(hipStream_t s, const TractScanTask* tasks, int n);      // one wave per window

}  // namespace strq
