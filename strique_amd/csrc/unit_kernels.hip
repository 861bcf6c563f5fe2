// Repeat-unit positions from a flanked-model decode (repeatHMM's path, STRique.py:374-378,433-441): the observations of the best
// path that emit from the two counted (dummy) states.  Two routes, same positions:
//   unit_hop_kernel   -- from the unit records of a VIT_UNIT decode: one hop per repeat unit, back from the end state's payload;
//   unit_scan_kernel  -- from the state path that the back-pointer traceback wrote (models and windows without a unit decode).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "unit_kernels.h"
#include "viterbi_kernels.h"

namespace strq {

// The chains are short (one hop per repeat unit, a few thousand at most) and independent: a lane per window.
__global__ void __launch_bounds__(64) unit_hop_kernel(const UnitTask* __restrict__ tasks, int n_tasks)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_tasks) return;
    const UnitTask tk = tasks[i];
    const VitResult* r = static_cast<const VitResult*>(tk.result);
    if (r->status != 0) { *tk.bad = 1; return; }
    uint32_t p = r->dbg[0];
    int64_t j = tk.n;
    while (p != 0 && j > 0) {
        const int64_t t = (int64_t)(p >> 1) - 1;
        if (t < 0 || t >= tk.T) break;
        tk.out[--j] = tk.base + t;
        p = tk.rec[2 * t + (p & 1u)];
    }
    if (p != 0 || j != 0) *tk.bad = 1;          // the chain and the count decode disagree
}

// One wave per window: 64 observations per round, the counted ones compacted with a ballot (ascending order).
__global__ void __launch_bounds__(256) unit_scan_kernel(const UnitTask* __restrict__ tasks, int n_tasks)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_tasks) return;
    const UnitTask tk = tasks[i];
    const VitResult* r = static_cast<const VitResult*>(tk.result);
    if (r->status != 0) { if (lane == 0) *tk.bad = 1; return; }
    int64_t k = 0;
    for (int64_t t0 = 0; t0 < tk.T; t0 += 64) {
        const int64_t t = t0 + lane;
        const bool hit = t < tk.T && tk.count_inc[tk.path[t]] != 0;
        const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
        const int64_t at = k + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (hit && at < tk.n) tk.out[at] = tk.base + t;
        k += __builtin_popcountll(m);
    }
    if (lane == 0 && k != tk.n) *tk.bad = 1;
}

int launch_unit_hop(hipStream_t s, const UnitTask* tasks, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(unit_hop_kernel, dim3((n + 63) / 64), dim3(64), 0, s, tasks, n);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_unit_scan(hipStream_t s, const UnitTask* tasks, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(unit_scan_kernel, dim3((n + 3) / 4), dim3(256), 0, s, tasks, n);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace strq
