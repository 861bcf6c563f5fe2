// Internal: anchored counting -- reads that hold one flank only (not part of the C ABI; strq_set_anchored in strique_hip.h states
// the rule, strique_amd/anchored.py restates it for the tests).
//   anchored_classify_kernel -- the kind and the window of every read of a sub-batch from its ReadGeom / ReadCond: the only place
//                               on the device that knows the rule
//   anchored_task_kernel     -- the Viterbi tasks of the reads of kind 2 / 3, once the host has grouped them by kernel shape
//   anchored_mod_task_kernel -- behind their decode: the tasks of the modification pass on the stretch it put into the repeat
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cond_kernels.h"
#include "mod_kernels.h"
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

// Methylation calls of anchored reads (strq_set_anchored_mod): item k is one read of kind 2 / 3 whose target has a dual model.  Its
// stretch -- the raw samples [begin, end) its MARK decode put into the repeat section, as anchored_record reads them off
// VitResult::dbg[0 .. 1] -- is known on the device only; the host has sized `out` (compacted samples) and `bp` (hub records) from
// the window, `cap` observations, which the stretch never exceeds.
struct AnchoredModItem {
    int32_t read, res, slot, pad_;      // read of the sub-batch, its task in the MARK launch, the position of its HUB task
    const VitModel* model;              // the dual model
    double* out; uint16_t* bp;
    double mod_lo, mod_hi;
    int64_t cap;
};
//   anchored_mod_task_kernel -- the ModTask (mod[k]) and the HUB VitTask (vit[slot]) of every item; T = 0 for a record that does not
//                               qualify (no path, marks that describe no stretch, a window outside its read)
struct AnchoredModTaskArgs {
    const AnchoredClass* cls; const ReadCond* rc; const VitResult* res;
    const AnchoredModItem* item;
    const void* raw; int is_f64;        // the raw samples of the sub-batch (ReadCond::off counts from here)
    double clip_lo, clip_hi;
    ModTask* mod; VitTask* vit;
    int n_items, n_reads, n_res;
};
int launch_anchored_mod_tasks(hipStream_t s, const AnchoredModTaskArgs& a);

}  // namespace strq
