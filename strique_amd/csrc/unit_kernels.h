// Internal: repeat-unit positions of the detect pipeline (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace strq {

// One decoded window: the observations t of the best path that emit from a counted state, written as base + t (ascending) to
// out[0 .. n).  Record route: `rec` = the 2 x T unit records of a VIT_UNIT decode (VIT_UNIT_T_MAX) and the end payload in
// result->dbg[0]; back-pointer route: `path` = the emitting state of every observation (launch_vit_traceback) and `count_inc`
// of the model.  n comes from the count decode of the same window; *bad is set to 1 when the window does not give exactly n.
struct UnitTask {
    const uint32_t* rec;
    const int32_t* path;
    const int32_t* count_inc;
    const void* result;      // VitResult of the window (device)
    int64_t* out;
    int64_t T, base, n;
    int32_t* bad;
};
int launch_unit_hop(hipStream_t s, const UnitTask* tasks, int n);        // record route: one lane per window
int launch_unit_scan(hipStream_t s, const UnitTask* tasks, int n);       // back-pointer route: one wave per window

}  // namespace strq
