// Internal: the variant pass (strq_set_variants; not part of the C ABI).
//
// A variant model (hmm.RepeatVariantModel) is the dual model of the modification pass with NB = 2 .. 4 branches over one pore model:
// branch 0 the repeat unit, branch b >= 1 the k-mers around alt unit b.  Its best path on the repeat stretch x of a read alternates
// hub emissions (s0, e0) and passages -- maximal runs of emissions of one branch.  Passage j covers x[u_j .. w_j]: the s0 emission in
// front of it, its branch emissions, the e0 emission behind it (u_0 = 0, u_j = w_{j-1} + 1), and
//   V_b(j) = Viterbi log-probability (start -> end) of the model on x[u_j .. w_j] with every edge that touches an emitting state of
//            another branch removed,                                                         b in 0 .. NB - 1
// evaluated like oracle/viterbi_oracle.c: float64, best = max_e(v_prev[src_e] + in_logp[e]), v = best + emission, no contraction;
// -inf where a branch has no path.  (The mod-llr definition of mod_llr_kernels.h for NB branches.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace strq {

#define VAR_MAX_EMIT 128       // emitting states of a variant model: two per lane at most
#define VAR_MAX_NB 4           // branches: the repeat unit and up to three alt units
#define VAR_DEG 8              // in-edges of an emitting state that survive in its own copy
#define VAR_DEG2 4             // ... of a hub state inside the copy of one further branch
#define VAR_END_DEG 8          // in-edges of the end state
#define VAR_PAD 1024           // cell code of "no edge"

// branch of a state tag: 0 base, 1 / 3 / 4 alt branch 1 / 2 / 3; -1 for a hub (tag 2) and anything else
static inline __host__ __device__ int var_branch_of_tag(int tag) { return tag == 0 ? 0 : (tag == 1 ? 1 : ((tag == 3 || tag == 4) ? tag - 1 : -1)); }

// Edge image of a variant model, built on the host once per model from the uploaded in-edges (var_build_image).  Emitting state l
// sits in slot l / 64, lane l % 64.  All NB masked recurrences run side by side: a branch state carries the value of its own branch, a
// hub state one value per branch.  A source is a cell code: 128 c + l = copy c of state l (a branch state has copy 0 only),
// VAR_PAD = no edge.  Rows are 64 lanes wide.
struct VarModel {
    int32_t n_emit, n_branch;
    int32_t mode;                // 0: up to 32 states, two passages per wave; 1: up to 64, one state per lane; 2: up to 128, two per lane
    int32_t deg, deg2;           // rows of src / src2 in use
    int32_t end_deg[VAR_MAX_NB];
    const int32_t* src;          // [2 slots][VAR_DEG][64]: sources of the state's own value (a hub's: its copy 0)
    const double* lp;
    const int32_t* src2;         // [VAR_MAX_NB - 1 copies][2][VAR_DEG2][64]: sources of a hub's copy 1 ..
    const double* lp2;
    const double* start_lp;      // [2][64]: log-probability of the edge from the start state (into every copy of a hub), -inf if none
    const int32_t* kind;         // [2][64]: 0 no state, 1 Normal, 2 Uniform
    const double* ea;            // [2][64] each, as LlrModel
    const double* eb;
    const double* ec;
    const int32_t* hub;          // [2][64]: 1 for a hub state
    const int32_t* end_src;      // [VAR_MAX_NB copies][VAR_END_DEG]
    const double* end_lp;
};
size_t var_image_bytes();
// The image of a baked model for a buffer at device address `dev_base`, into `blob`.  Returns 0, or 1 with the reason in `why` for a
// model the pass does not cover (more than VAR_MAX_EMIT emitting states, silent states besides start and end, ...).
int var_build_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end, const int32_t* in_ptr, const int32_t* in_src,
                    const double* in_logp, const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                    const int32_t* state_tag, int32_t n_alt, const void* dev_base, std::vector<char>& blob, int32_t* mode, std::string& why);

// Passage bounds of one read, ascending: w[j] = observation of the e0 emission behind passage j, branch[j] its branch.  The number of
// passages is not known beforehand, so the bounds kernels run twice.  Count pass (w = branch = null, cap = T / 3 + 1: a passage takes
// three observations at least): *n = passages found.  Write pass (cap = that count): exactly `cap` entries are written, never more.
// *bad is set when the records / the path do not describe such a chain -- a record outside (0, T], times that do not descend, more
// passages than `cap`, a branch outside the model's -- or when the write pass finds another number of passages than the count pass.
struct VarBoundTask {
    const uint64_t* rec;     // hub records of the read's decode (T + 1), or null: take the bounds from `path`
    const void* result;      // VitResult of that decode (device)
    const int32_t* path;     // emitting states of the decode (back-pointer route)
    const int32_t* tag;      // state tags of the model
    int32_t* w; int32_t* branch;
    int32_t* n; int32_t* bad;
    int64_t T; int32_t cap, n_branch;
};
struct VarRead {
    const VarModel* model;
    const double* x;         // the clipped repeat stretch the variant model decoded
    const int32_t* w;
    double* out;             // NB doubles per passage
    int64_t T;
};
int launch_var_bounds(hipStream_t s, const VarBoundTask* hop, int n_hop, const VarBoundTask* scan, int n_scan);
// reads of one (mode, NB); first[n_reads + 1]: passages of the reads in front of read r.  n_cu sizes the grid.
int launch_var_score(hipStream_t s, int mode, int n_branch, const VarRead* reads, const int64_t* first, int n_reads, int64_t n_passages, int n_cu);

}  // namespace strq
