// State statistics of traced windows (state_stats_kernels.h; strique_amd/state_stats.py states the rule): what the best path assigns to
// every emitting state, summed in the order of the observations.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "state_stats_kernels.h"
#include "hmm_wave.h"

namespace strq {

// One wave per window, one window per workgroup.  A round takes 64 observations (coalesced loads of the path and, through
// vit_observation, of the window), finds the distinct states among them with one ballot each -- the path is run-structured, a round
// holds about ten -- and lets the first lane of every state add that state's observations in lane order, read from a staging row in
// LDS, to the state's accumulators in LDS.  The states of a round differ, so their lanes never meet in an accumulator; the observations
// of one state are added by one lane, one at a time, in ascending order -- no atomics, no tree.  LDS: 64 staged observations, then
// sum | sumsq | n of max_emit states.
__global__ void __launch_bounds__(64) state_stats_kernel(const VitTask* __restrict__ vit, const StateStatsTask* __restrict__ tasks, int n_tasks, int max_emit)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char state_stats_lds[];
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    if (i >= n_tasks) return;
    const StateStatsTask sk = tasks[i];
    const VitTask tk = vit[i];
    const int ne = sk.n_emit;
    double* xs = reinterpret_cast<double*>(state_stats_lds);
    double* a_sum = xs + 64; double* a_sq = a_sum + max_emit;
    int64_t* a_n = reinterpret_cast<int64_t*>(a_sq + max_emit);
    const bool open = static_cast<const VitResult*>(sk.result)->status == 0 && ne >= 0 && ne <= max_emit;
    bool bad = !open;
    if (open) {
        for (int e = lane; e < ne; e += 64) { a_sum[e] = 0.0; a_sq[e] = 0.0; a_n[e] = 0; }
        wave_fence();
        for (int64_t t0 = 0; t0 < tk.T; t0 += 64) {
            const int64_t t = t0 + lane;
            int s = -1; double x = 0.0; bool valid = false;
            if (t < tk.T) {
                s = sk.path[t];
                if (s < 0 || s >= ne) bad = true;
                else { x = vit_observation(tk, t); valid = x == x; }          // a missing observation (NaN) is neither counted nor summed
            }
            xs[lane] = x;
            wave_fence();
            uint64_t rest = __builtin_amdgcn_ballot_w64(valid), mine = 0;
            while (rest) {          // uniform: one turn per distinct state of the round
                const int leader = __builtin_ctzll(rest);
                const int ls = __builtin_amdgcn_readlane(s, leader);
                const uint64_t m = __builtin_amdgcn_ballot_w64(valid && s == ls);
                if (lane == leader) mine = m;
                rest &= ~m;
            }
            if (mine) {
                double su = a_sum[s], sq = a_sq[s];
                for (uint64_t m = mine; m; m &= m - 1) {
                    const double xv = xs[__builtin_ctzll(m)];
                    const double q = xv * xv;          // rounded before it is added
                    su = su + xv; sq = sq + q;
                }
                a_sum[s] = su; a_sq[s] = sq; a_n[s] += (int64_t)__builtin_popcountll(mine);
            }
            wave_fence();
        }
    }
    const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
    for (int e = lane; e < ne; e += 64) {
        sk.n[e] = any_bad ? 0 : a_n[e]; sk.sum[e] = any_bad ? 0.0 : a_sum[e]; sk.sumsq[e] = any_bad ? 0.0 : a_sq[e];
    }
    if (any_bad && lane == 0) *sk.bad = 1;
}

int launch_state_stats(hipStream_t s, const VitTask* vit, const StateStatsTask* tasks, int n, int max_emit)
{
    if (n <= 0) return 0;
    if (max_emit < 1 || max_emit > STATE_STATS_MAX_EMIT) return 2;
    const size_t lds = 64 * 8 + (size_t)max_emit * 24;          // at most 96.5 KB of the CU's 160 KB
    if (hipFuncSetAttribute((const void*)state_stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 1;
    hipLaunchKernelGGL(state_stats_kernel, dim3(n), dim3(64), lds, s, vit, tasks, n, max_emit);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace strq
