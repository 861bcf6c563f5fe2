// Scan: which target and strand a read spans, from its raw signal alone.  Every read is aligned against the two flanks of every
// candidate (one strand of one target); the candidates are compared on the normalised flank scores detect() reports
// (STRique.py:590-601), and only the winner's window goes to the HMM.
//   scan_select_kernel -- positions and scores of all candidates of a read, the rule, the winner's ReadGeom
//   scan_task_kernel   -- the winner's Viterbi task, once the host has grouped the winners by kernel shape
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "scan_kernels.h"

namespace strq {

// A gather (a few record words per candidate) and a reduce over n_cand: one thread per read.
// The rule: key = min(score_prefix, score_suffix); eligible when prefix_begin < suffix_end and key >= min_score (min_score > 0, so an
// eligible candidate passes the gate of STRique.py:603); the largest key wins, the lowest list position on a tie.  NaN is never eligible.
__global__ void __launch_bounds__(64) scan_select_kernel(ScanSelectArgs a)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.n_reads) return;
    const ReadCond rc = a.rc[r];
    ReadGeom win = {};
    int w = -1; double w_key = 0.0;
    for (int c = 0; c < a.n_cand; ++c) {
        const size_t ai = 2 * ((size_t)r * a.n_cand + c);
        ReadGeom g = {};
        if (rc.n > 0) {
            const int tp = a.task_of[ai], ts = a.task_of[ai + 1];
            prefix_geometry(a.tasks[tp], a.results[tp], a.trim[2 * c], g);
            suffix_geometry(a.tasks[ts], a.results[ts], a.trim[2 * c + 1], g);
            g.gate = geometry_gate(g);
        }
        a.scores[ai] = g.score_prefix; a.scores[ai + 1] = g.score_suffix;
        a.best[ai] = g.best_prefix; a.best[ai + 1] = g.best_suffix;
        const double key = g.score_prefix < g.score_suffix ? g.score_prefix : g.score_suffix;
        // a read that could not be normalised (status 1) has no winner
        const bool eligible = rc.n > 0 && rc.status == COND_OK && g.prefix_begin < g.suffix_end && g.score_prefix >= a.min_score && g.score_suffix >= a.min_score;
        if (eligible && (w < 0 || key > w_key)) { w = c; w_key = key; win = g; }
    }
    a.winner[r] = w;
    a.geom[r] = win;
}

__global__ void __launch_bounds__(128) scan_task_kernel(ScanTaskArgs a)
{
    const int r = blockIdx.x * 128 + threadIdx.x;
    if (r >= a.n_reads) return;
    a.vit[a.vit_slot[r]] = window_task(a.geom[r], a.rc[r], a.model_of[r], a.flt, a.is_f64, a.ps);
}

int launch_scan_select(hipStream_t s, const ScanSelectArgs& a)
{
    if (a.n_reads <= 0) return 0;
    hipLaunchKernelGGL(scan_select_kernel, dim3((a.n_reads + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_scan_tasks(hipStream_t s, const ScanTaskArgs& a)
{
    if (a.n_reads <= 0) return 0;
    hipLaunchKernelGGL(scan_task_kernel, dim3((a.n_reads + 127) / 128), dim3(128), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace strq
