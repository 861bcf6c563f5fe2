// Methylation calls for the CpG groups of the flanks (flank_mod_kernels.h).
//   flank_mod_bounds_kernel -- one wave per flank stretch.  The lanes stride over the path, 64 observations per round: every lane
//                              looks up the column of its observation once, then one ballot per group says which of the 64
//                              observations the group's columns emitted.  Lane g keeps the minimum and the maximum of group g, so
//                              the reduction over the path is the ballot and nothing is exchanged through LDS.
// A stretch is ~10^3 observations and a flank has ~10 groups: the launch is a few thousand waves of a few microseconds, bound by
// the latency of the two dependent loads (path, column_of); four waves per workgroup and no LDS keep the occupancy at the wave limit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flank_mod_kernels.h"

namespace strq {

// the score task of one group: a passage x[u .. w] as a read of one unit that starts at u, or no passage
static __device__ __forceinline__ void flank_score_task(const FlankBoundTask& tk, int g, const FlankGroupBounds& b)
{
    if (!tk.score) return;
    const FlankScoreSlot s = tk.score[g];
    const bool scored = b.status == FMOD_SCORED;
    LlrRead rd;
    rd.model = s.model; rd.x = tk.x + (scored ? b.u : 0); rd.w = tk.wloc + s.slot; rd.out = tk.scores + 2 * (size_t)s.slot; rd.T = scored ? (int64_t)(b.w - b.u + 1) : 0;
    tk.wloc[s.slot] = scored ? b.w - b.u : -1;
    tk.reads[s.slot] = rd;
}

__global__ void __launch_bounds__(256) flank_mod_bounds_kernel(const FlankBoundTask* __restrict__ tasks, int n_tasks)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_tasks) return;
    const FlankBoundTask tk = tasks[i];
    const int G = tk.n_groups < FMOD_MAX_GROUPS ? tk.n_groups : FMOD_MAX_GROUPS;
    const bool mine = lane < G;
    if (tk.vit_status && *tk.vit_status != 0) {
        if (mine) { const FlankGroupBounds b = {FMOD_NO_PATH, -1, -1}; tk.out[lane] = b; flank_score_task(tk, lane, b); }
        return;
    }
    FlankGroupRange r = {0, -1};
    if (mine) r = tk.groups[lane];
    int64_t first = -1, last = -1;          // of group `lane`
    for (int64_t t0 = 0; t0 < tk.T; t0 += 64) {
        const int64_t t = t0 + lane;
        int col = -1;
        if (t < tk.T) {
            const int32_t s = tk.path[t];
            if (s >= 0 && s < tk.n_emit) col = tk.column_of[s];
        }
        if (__builtin_amdgcn_ballot_w64(col >= 0) == 0) continue;          // a round outside every column (the ballot is wave-uniform)
        for (int g = 0; g < G; ++g) {
            const int c0 = __shfl(r.c0, g), c1 = __shfl(r.c1, g);
            const uint64_t hit = __builtin_amdgcn_ballot_w64(col >= c0 && col <= c1);
            if (hit != 0 && lane == g) {
                if (first < 0) first = t0 + __builtin_ctzll(hit);
                last = t0 + 63 - __builtin_clzll(hit);
            }
        }
    }
    if (!mine) return;
    FlankGroupBounds b = {FMOD_SKIPPED, -1, -1};
    if (first >= 0) {
        if (first == 0 || last == tk.T - 1) b.status = FMOD_EDGE;
        else { b.status = FMOD_SCORED; b.u = (int32_t)(first - 1); b.w = (int32_t)(last + 1); }
    }
    tk.out[lane] = b;
    flank_score_task(tk, lane, b);
}

int launch_flank_mod_bounds(hipStream_t s, const FlankBoundTask* tasks, int n_tasks)
{
    if (n_tasks <= 0) return 0;
    hipLaunchKernelGGL(flank_mod_bounds_kernel, dim3((n_tasks + 3) / 4), dim3(256), 0, s, tasks, n_tasks);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace strq
