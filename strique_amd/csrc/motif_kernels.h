// Internal: the motif track (strq_motif_track; not part of the C ABI).  strique_amd/motifs.py states the rule.
//
// A stretch of T observations is cut into n_seg = max(1, T / S) segments (segment i < n_seg - 1 is [i S, (i + 1) S), the last one runs
// to T), and every segment is scored under the loop model of each of the K candidate units (K <= MOTIF_MAX_CAND):
//   V[i][j] = max over the emitting states of the Viterbi value after the last observation of segment i under loop model j
// evaluated like oracle/viterbi_oracle.c: float64, best = max_e(v_prev[src_e] + in_logp[e]), v = best + log emission, no contraction.
// A loop model has emitting states, a start state that enters every one of them, and an end state every one of them reaches with
// log-probability 0 -- so the value of the end state is the maximum over the emitting states, and `max` is exact: neither the lane
// order nor the cut of a window into tasks can change a bit of V.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "vit_model.h"

namespace strq {

#define MOTIF_MAX_EMIT 64      // emitting states of a loop model: one per lane
#define MOTIF_DEG 8            // in-edges of an emitting state from emitting states (the loop models need 7)
#define MOTIF_MAX_CAND 4
#define MOTIF_SEG_MIN 32
#define MOTIF_SEG_MAX 4096
#define MOTIF_PAD 64           // source of a padding edge: the cell behind the 64 states, which stays -inf

// Edge image of a loop model, built on the host once per model from the uploaded in-edges (motif_build_image).  Emitting state l
// sits in lane l.  Rows are 64 lanes wide: MOTIF_PAD / -inf where a lane has no such edge, kind 0 where it has no state.
struct MotifModel {
    int32_t n_emit;
    int32_t deg;                 // rows of src / lp in use (the largest in-degree over the lanes)
    const int32_t* src;          // [MOTIF_DEG][64]: source lanes, ascending by state as in the baked model
    const double* lp;            // [MOTIF_DEG][64]
    const double* start_lp;      // [64]: log-probability of the edge from the start state, -inf if none
    const int32_t* kind;         // [64]: 0 no state, 1 Normal, 2 Uniform
    const double* ea;            // [64] each: mu | lo,  1 / (2 sigma^2) | hi,  -log(sigma sqrt(2 pi)) | -log(hi - lo)
    const double* eb;
    const double* ec;
};
size_t motif_image_bytes();
// The image of a baked loop model for a buffer at device address `dev_base`, into `blob` (motif_image_bytes()).  Returns 0, or 1
// with the reason in `why` for a model that is no loop model.
int motif_build_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end, const int32_t* in_ptr, const int32_t* in_src,
                      const double* in_logp, const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                      const void* dev_base, std::vector<char>& blob, std::string& why);

// one stretch: its observations as a decode would read them (VitTask::model is not used), its candidates, where its results go
struct MotifWindow {
    VitTask obs;
    const MotifModel* model[MOTIF_MAX_CAND];
    int32_t n_cand, segment;
    int64_t n_seg;
    double* V;                   // [n_seg][n_cand]
    int32_t* winner;             // [n_seg]
    int64_t* obs_won;            // [MOTIF_MAX_CAND]
    int32_t* majority;
};
// one wave's share of a window: the segments [seg_first, seg_first + seg_count)
struct MotifTask {
    int32_t window, seg_count;
    int64_t seg_first;
};
// segments one wave scores in a row (motif_run_segments(S) * S >= 256 observations per candidate, except at a window's end)
inline int motif_run_segments(int segment) { return segment >= 256 ? 1 : 256 / segment; }

// motif_track_kernel over the tasks, then motif_reduce_kernel over the windows.  n_cu sizes the grid of the former.
int launch_motif_track(hipStream_t s, const MotifWindow* windows, int n_windows, const MotifTask* tasks, int64_t n_tasks, int n_cu);

}  // namespace strq
