// Internal: per-unit scores of the modification pass (strq_set_mod_llr; not part of the C ABI).
//
// repeatModHMM.mod_repeats (reference scripts/STRique.py:492-500) reports one hard call per repeat unit: the branch (base | modified)
// the best path of the dual model takes between two hub emissions.  With that segmentation fixed, unit j covers the observations
// x[u_j .. w_j] -- the s0 emission in front of it, its branch emissions, the e0 emission behind it -- and
//   V_B(j) = Viterbi log-probability (start -> end) of the dual model on x[u_j .. w_j] with every edge that touches an emitting state
//            of the other branch removed,                                                        B in {base, mod}
// evaluated like oracle/viterbi_oracle.c: float64, best = max_e(v_prev[src_e] + in_logp[e]), v = best + emission, no contraction.
// llr_j = V_mod(j) - V_base(j).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace strq {

#define LLR_MAX_EMIT 128       // emitting states of a dual model: two per lane at most
#define LLR_DEG 8              // in-edges of an emitting state from emitting states (as the lane layouts of the Viterbi kernels)
#define LLR_DEG2 4             // ... of a hub state inside one branch copy
#define LLR_END_DEG 8          // in-edges of the end state

// Edge image of a dual model, built on the host once per model from the uploaded in-edges (llr_build_image).  Emitting state l sits
// in slot l / 64, lane l % 64.  Both masked recurrences run side by side: a branch state carries the value of its own branch, a hub
// state (tag 2) one value per branch.  A source is a cell code: l = value of state l (a hub's: its base copy), 128 + l = the mod
// copy of hub l, LLR_PAD = no edge (a cell that stays -inf).  Rows are 64 lanes wide, -inf / LLR_PAD where a lane has no such edge.
#define LLR_PAD 256
struct LlrModel {
    int32_t n_emit;
    int32_t mode;                // 0: up to 32 states, two units per wave; 1: up to 64, one state per lane; 2: up to 128, two per lane
    int32_t deg, deg2;           // rows of src / src2 in use (largest over the lanes and slots)
    int32_t end_deg[2];          // in-edges of the end state that survive in the base / mod copy
    const int32_t* src;          // [2 slots][LLR_DEG][64]: sources of the state's own value, ascending by state as in the baked model
    const double* lp;
    const int32_t* src2;         // [2][LLR_DEG2][64]: sources of a hub's mod copy
    const double* lp2;
    const double* start_lp;      // [2 copies][2 slots][64]: log-probability of the edge from the start state, -inf if none
    const int32_t* kind;         // [2][64]: 0 no state, 1 Normal, 2 Uniform
    const double* ea;            // [2][64] each: mu | lo,  1 / (2 sigma^2) | hi,  -log(sigma sqrt(2 pi)) | -log(hi - lo)
    const double* eb;
    const double* ec;
    const int32_t* hub;          // [2][64]: 1 for a hub state
    const int32_t* end_src;      // [2 copies][LLR_END_DEG]
    const double* end_lp;
};
// bytes of an image (the struct first, the arrays behind it)
size_t llr_image_bytes();
// The image of a baked model for a buffer at device address `dev_base`, into `blob` (llr_image_bytes()).  Returns 0, or 1 with the
// reason in `why` for a model the pass does not cover.
int llr_build_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end, const int32_t* in_ptr, const int32_t* in_src,
                    const double* in_logp, const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                    const int32_t* state_tag, const void* dev_base, std::vector<char>& blob, int32_t* mode, std::string& why);

// unit bounds of one read: w[j] = observation of the hub emission behind unit j, ascending (u_0 = 0, u_j = w[j - 1] + 1)
struct LlrBoundTask {
    const uint64_t* rec;     // hub records of the read's decode (T + 1), or null: take the bounds from `path`
    const void* result;      // VitResult of that decode (device): status, dbg[0] = time of the last e0 emission
    const int32_t* path;     // emitting states of the decode (back-pointer route)
    const int32_t* tag;      // state tags of the model (2 = hub)
    int32_t* w;              // n bounds
    int64_t n, T;            // units of the read (the length of its pattern string), observations
    int32_t* bad;            // set when the chain / path and the pattern disagree
};
struct LlrRead {
    const LlrModel* model;
    const double* x;         // the clipped repeat stretch the dual model decoded
    const int32_t* w;
    double* out;             // (V_base, V_mod) per unit
    int64_t T;
};
int launch_llr_bounds(hipStream_t s, const LlrBoundTask* hop, int n_hop, const LlrBoundTask* scan, int n_scan);
// reads of one mode; first[n_reads + 1]: units of the reads in front of read r.  n_cu sizes the grid.
int launch_llr_score(hipStream_t s, int mode, const LlrRead* reads, const int64_t* first, int n_reads, int64_t n_units, int n_cu);

}  // namespace strq
