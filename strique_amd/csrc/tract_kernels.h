// Internal: tract pass of the detect pipeline (not part of the C ABI; strq_set_tracts in strique_hip.h, strique_amd/tracts.py states
// the rule).  The decode itself is the count decode of the Viterbi kernels with the wide payload (launch_viterbi's `tracts`);
//   tract_task_kernel -- the Viterbi tasks of the eligible reads of a sub-batch, once the host has grouped them by kernel shape:
//                        the window [prefix_begin, suffix_end) of the count decode on the slot's filtered signal, from the read's
//                        geometry and conditioning record
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

}  // namespace strq
