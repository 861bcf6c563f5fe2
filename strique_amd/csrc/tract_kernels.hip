// Tract pass: the windows of the compound-model decode.  The flank geometry and the conditioning rows are on the device already
// (finalize_kernel, scan_kernels.h); the decode runs on the Viterbi kernels with the wide count payload (viterbi_kernels.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tract_kernels.h"

namespace strq {

// One thread per task.  The window is that of the count decode, checked once more against the read it is cut from: a task never
// leaves the read's samples (an empty task -- T = 0 -- decodes to "no path").
__global__ void __launch_bounds__(128) tract_task_kernel(TractTaskArgs a)
{
    const int k = blockIdx.x * 128 + threadIdx.x;
    if (k >= a.n_tasks) return;
    const int r = a.read[k];
    VitTask vt = {};
    vt.model = a.model[k];
    if (r >= 0 && r < a.n_reads) {
        const ReadGeom g = a.geom[r];
        const ReadCond rc = a.rc[r];
        const int open = g.gate && rc.status == COND_OK && g.prefix_begin >= 0 && g.prefix_begin < g.suffix_end && g.suffix_end <= (int64_t)rc.n;
        vt = window_task(open, g.prefix_begin, g.suffix_end, rc, a.model[k], a.flt, a.is_f64, a.ps);
    }
    a.vit[k] = vt;
}

int launch_tract_tasks(hipStream_t s, const TractTaskArgs& a)
{
    if (a.n_tasks <= 0) return 0;
    hipLaunchKernelGGL(tract_task_kernel, dim3((a.n_tasks + 127) / 128), dim3(128), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace strq
