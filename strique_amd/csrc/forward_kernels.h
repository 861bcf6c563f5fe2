// Internal: forward algorithm over the flanked-repeat HMM with the second-order expectation semiring (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "viterbi_kernels.h"

namespace strq {

// What forward_kernel needs beyond the lane-layout image of the model (VitModel): the transition PROBABILITIES of its edge rows.
// The Viterbi image holds log-probabilities, and where bake() met two spliced paths between the same pair of states it kept the
// larger one (a max over paths loses nothing by that); a sum over paths needs their sum, which strq_model_set_forward_logp
// supplies per in-edge.  Same row layout as VitModel::edge_src / chain_logp; padding entries are 0.
struct FwdModel {
    const VitModel* vit;
    const double* edge_w;            // n_edge_rows * 64
    const double* chain_w;           // spl * 64: weight of the chain edge into the cell, 0 without one
    int32_t n_stages;                // rounds of the silent phase: 1 + the longest run of non-chain silent -> silent edges
    int32_t pad_;
};

// Mass, and first and second moment of (v - c0), of all paths that end in the model's end state after the last observation;
// the mass is scaled by 2^-expo.  p == 0: no path.
struct FwdResult {
    double p, r, s;
    int64_t expo;
    int32_t steps_rescaled, pad_;
};

// log-likelihood, mean and variance of the visit count from a window's result (host; the one place this arithmetic lives, so that
// the model-level call and the detect pipeline report the same bits)
inline int fwd_finish(const FwdResult& f, int64_t c0, double* log_lik, double* mean, double* var)
{
    if (!(f.p > 0.0)) { *log_lik = -INFINITY; *mean = NAN; *var = NAN; return 1; }
    // mantissa and exponent apart: the same bits however the kernel split the likelihood between p and expo
    int e2 = 0;
    const double mant = std::frexp(f.p, &e2);
    *log_lik = std::log(mant) + (double)(f.expo + e2) * 0.693147180559945309417232121458;
    const double m = f.r / f.p;
    double v = f.s / f.p - m * m;
    if (!(v > 0.0)) v = 0.0;          // a variance below rounding error may come out negative
    *mean = (double)c0 + m; *var = v;
    return 0;
}

// shape: as vit_shape_of(model) gives it (lane layouts only).  Returns 0, 1 (launch failed), 2 (no forward kernel for this shape).
int launch_forward(hipStream_t stream, int shape, int max_cells, const VitTask* tasks, const FwdModel* const* models,
                   const int64_t* c0, FwdResult* results, int n_tasks, int* queue, int n_cu, const int* order, int rescale_every);

}  // namespace strq
