// Internal: methylation calls for the CpG groups of the flanks (not part of the C ABI; strique_amd/flank_mod.py states the rule).
//   flank_mod_bounds_kernel -- behind the segmentation decode of a flank stretch with its flank profile model: per CpG group the
//                              first and the last observation the path emits from the group's profile columns, and from them the
//                              status and the passage x[u .. w] its site model is scored on (mod_llr_kernels.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mod_llr_kernels.h"

namespace strq {

#define FMOD_MAX_GROUPS 64       // groups of one flank: one lane each
enum { FMOD_SCORED = 0, FMOD_NO_PATH = 1, FMOD_EDGE = 2, FMOD_SKIPPED = 3, FMOD_TOO_LONG = 4 };

struct FlankGroupRange { int32_t c0, c1; };      // profile columns c0 .. c1 of a group, inclusive
struct FlankGroupBounds { int32_t status, u, w; };      // u = first - 1, w = last + 1 (observations of the stretch); -1, -1 unless status is FMOD_SCORED

// where the score task of a group goes (the pass; the test hook has none): the image of its site model and its position among the
// LlrReads of the piece, which the host has ordered by the image's mode
struct FlankScoreSlot { const LlrModel* model; int32_t slot, pad_; };

// one flank stretch: the emitting states of its decode and the groups of its flank.  The kernel trusts neither the path nor the
// count: a state outside [0, n_emit) has no column, and groups beyond FMOD_MAX_GROUPS are not looked at (their records and score
// tasks stay as the caller initialised them) -- whoever builds tasks must keep n_groups within the limit, as flank_mod.check does.
struct FlankBoundTask {
    const int32_t* path;             // T states
    const int32_t* vit_status;       // status of the decode (0: a path; anything else: every group FMOD_NO_PATH), or null: a path
    const int32_t* column_of;        // per emitting state of the model: its profile column, -1 for none
    const FlankGroupRange* groups;
    FlankGroupBounds* out;           // n_groups records
    int64_t T;
    int32_t n_emit, n_groups;        // emitting states of the model (a path state outside them has no column); at most FMOD_MAX_GROUPS groups
    // with `score`: group g also gets its score task reads[score[g].slot] -- one LlrRead of one unit on x[u .. w] (the read starts at u,
    // its bound is wloc[slot] = w - u, its pair goes to scores[2 slot ..]); a group that is not scored gets a task without a passage (-inf, -inf)
    const FlankScoreSlot* score; const double* x; LlrRead* reads; int32_t* wloc; double* scores;
};
int launch_flank_mod_bounds(hipStream_t s, const FlankBoundTask* tasks, int n_tasks);

}  // namespace strq
