// Internal: per-state posterior occupancy of observation windows -- the forward-backward algorithm over the lane-layout image of a
// model (not part of the C ABI; strq_forward_state_stats and strq_set_state_posteriors in strique_hip.h, strique_amd/state_posteriors.py
// states the rule).  Two kernels, one wave64 per window each, persistent on a task queue like forward_kernel:
//   posterior_forward_kernel  -- the p plane of forward_kernel, rescaled by a power of two after EVERY time step; the scaled mass of
//                                every emitting cell and the running exponent go to the window's workspace in HBM
//   posterior_backward_kernel -- walks the window downwards with the out-edges of the model (PostModel, the transposed image), combines
//                                its vector with the stored one into gamma_t(s) and sums gamma, gamma x, gamma x^2 per emitting state
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "forward_kernels.h"

namespace strq {

// The transposed image of a model: what the backward recursion  beta_t(i) = sum_j a_ij b_j(x_t+1) beta_t+1(j)  gathers.  The lane
// layout, the cells and the chains are VitModel's; a row holds the j-th OUT-edge of the 64 cells of a slot (target cell and transition
// probability, the probabilities of FwdModel), padding entries point at the model's last cell with weight 0.  The chain edges stay out
// of the rows as they do in VitModel: chain_next_w is the weight of the chain edge that LEAVES a silent cell (to position + 1), so that
// along a chain  y[q] = own[q] + chain_next_w[q] * y[q + 1]  -- the recurrence of forward_kernel's silent phase, running the other way.
struct PostModel {
    const FwdModel* fwd;
    int32_t oe_deg[8], oe_base[8];       // padded out-degree and first row of every emitting slot
    int32_t os_deg[8], os_base[8];       // ... of every silent slot (without the chain edge)
    const int32_t* out_dst;              // n_out_rows * 64: LDS cell of the target state
    const double* out_w;                 // n_out_rows * 64
    const double* chain_next_w;          // spl * 64, by owner slot: 0 without a chain successor
};

// Where a window's pass writes.  alpha: T x epl x 64 doubles (time step, emitting slot, lane), expo: T running exponents; both null
// for a window whose vectors are not stored (over the budget: the forward half alone runs, for the likelihood).  w, wx, wxx: n_emit
// entries each, by state, zeroed by the caller -- the backward half writes them only where the window has a path.
struct PostTask {
    double* alpha;
    int32_t* expo;
    double* w;
    double* wx;
    double* wxx;
};

// bytes of a window's stored vectors (the unit of STRQ_STATE_POST_WS_BYTES); every window starts on a 16-byte boundary
inline size_t post_alpha_bytes(int64_t T, int epl) { return (size_t)T * (size_t)epl * 64 * 8; }
inline size_t post_window_bytes(int64_t T, int epl) { return (post_alpha_bytes(T, epl) + (size_t)T * 4 + 15) & ~(size_t)15; }

// shape: as vit_shape_of(model) gives it (lane layouts only); the windows of a launch fit that shape.  results: one FwdResult per task
// (p and expo; r = s = 0), written by the forward half and read by the backward half.  queue: two heads.  Returns 0, 1 (launch
// failed), 2 (no kernel for this shape).
int launch_posterior(hipStream_t stream, int shape, int max_cells, const VitTask* tasks, const PostModel* const* models,
                     const PostTask* post, FwdResult* results, int n_tasks, int* queue, int n_cu, const int* order);

}  // namespace strq
