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

// One wave per window: 64 observations per round, the counted ones of every tract compacted with a ballot (ascending order).
__global__ void __launch_bounds__(256) tract_scan_kernel(const TractScanTask* __restrict__ tasks, int n_tasks)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_tasks) return;
    const TractScanTask tk = tasks[i];
    const VitResult* r = static_cast<const VitResult*>(tk.result);
    if (r->status != 0) { if (lane == 0) *tk.bad = 1; return; }
    const int K = tk.n_tracts < VIT_TRACTS_MAX ? tk.n_tracts : VIT_TRACTS_MAX;
    int64_t k[VIT_TRACTS_MAX] = {0, 0, 0};
    const uint64_t below = ((uint64_t)1 << lane) - 1ull;
    for (int64_t t0 = 0; t0 < tk.T; t0 += 64) {
        const int64_t t = t0 + lane;
        int tract = -1;
        if (t < tk.T) {
            const int32_t s = tk.path[t];
            const uint64_t inc = s >= 0 && s <= tk.n_states ? tk.tract_inc[s] : 0;
            if (inc) tract = (int)(__builtin_ctzll(inc) / VIT_TRACT_BITS);
        }
#pragma unroll
        for (int j = 0; j < VIT_TRACTS_MAX; ++j) {
            if (j >= K) break;
            const bool hit = tract == j;
            const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
            const int64_t at = k[j] + __builtin_popcountll(m & below);
            if (hit && at < tk.n[j]) tk.out[tk.off[j] + at] = tk.base + t;
            k[j] += __builtin_popcountll(m);
        }
    }
    if (lane == 0) {
        bool ok = true;
        for (int j = 0; j < K; ++j) ok = ok && k[j] == tk.n[j];
        if (!ok) *tk.bad = 1;
    }
}

int launch_tract_scan(hipStream_t s, const TractScanTask* tasks, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(tract_scan_kernel, dim3((n + 3) / 4), dim3(256), 0, s, tasks, n);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace strq
