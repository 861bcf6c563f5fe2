// Internal: anchored counting -- reads that hold one flank only (not part of the C ABI; strq_set_anchored in strique_hip.h states
// the rule, strique_amd/anchored.py restates it for the tests).
//   anchored_classify_kernel -- the kind and the window of every read of a sub-batch from its ReadGeom / ReadCond: the only place
//                               on the device that knows the rule
//   anchored_task_kernel     -- the Viterbi tasks of the reads of kind 2 / 3, once the host has grouped them by kernel shape
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cond_kernels.h"
#include "scan_kernels.h"
#include "viterbi_kernels.h"

namespace strq {

enum { ANCH_NONE = 0, ANCH_SPANNING = 1, ANCH_ENDS = 2, ANCH_STARTS = 3 };

struct AnchoredClass { int32_t kind, pad_; int64_t begin, end; };      // per read: kind and window [begin, end) of the filtered signal (0, 0 for kind 0)

struct AnchoredClassifyArgs {
    const ReadGeom* geom; const ReadCond* rc;
    double min_score;
    AnchoredClass* out;
    int n_reads;
};
int launch_anchored_classify(hipStream_t s, const AnchoredClassifyArgs& a);

// task k of the pass: read[k] of the sub-batch, decoded with model[k]; written to vit[k]
struct AnchoredTaskArgs {
    const AnchoredClass* cls; const ReadCond* rc;
    const int32_t* read; const VitModel* const* model;
    const void* flt; int is_f64;
    PoreStats ps;
    VitTask* vit;
    int n_tasks, n_reads;
};
int launch_anchored_tasks(hipStream_t s, const AnchoredTaskArgs& a);

}  // namespace strq
