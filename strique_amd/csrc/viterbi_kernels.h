// Internal: profile-HMM Viterbi kernels (not part of the C ABI).  Model and task images, decode modes, kernel shapes: vit_model.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vit_model.h"

namespace strq {

int vit_shape_for(const VitModel& model_host, VitMode mode);      // vit_shape_for(.., allow_g2) with the STRQ_VIT_NO_G2 switch read
// `shape` as vit_shape_of / vit_shape_for give it; `max_cells` = largest n_cells among the launch's models (checked against the
// shape's LDS buffers).  Returns 0, 1 (launch failed), 2 (the shape has no such mode: vit_mode_ok), 3 (max_cells).
// waves_hint 4: the launch shares the GPU with other kernels (register-resident shape: four waves per workgroup instead of eight)
// tracts (with VIT_COUNT, lane rows and the general kernel; 2 otherwise): VitResult::counted holds the tract counters of the models'
// tract_inc (VIT_TRACT_BITS) instead of the count; windows of VIT_MARK_T_MAX observations or more are not decoded and get status 2
int launch_viterbi(hipStream_t stream, int shape, int max_cells, const VitTask* tasks, VitResult* results,
                   int n_tasks, int* queue, int n_cu, VitMode mode, const int* order = nullptr, int waves_hint = 0, bool tracts = false);
int launch_vit_sort(hipStream_t stream, const VitTask* tasks, int n, int* order);   // order by descending T (n <= 8192)
int launch_vit_traceback(hipStream_t stream, const VitTask* tasks, const VitResult* results,
                         int32_t* const* paths, int n_tasks);

}  // namespace strq
