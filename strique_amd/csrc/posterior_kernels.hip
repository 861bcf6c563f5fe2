// Forward-backward on gfx950: per-state posterior occupancy of observation windows, one wave64 per window, float64, linear space.
// strique_amd/state_posteriors.py states the rule; posterior_kernels.h the images and the workspace.
//
// With alpha_t(s) the mass of all start -> s paths that emit x_1..t (s emitting x_t) and beta_t(s) the mass of all s -> end paths
// that emit x_t+1..T,  gamma_t(s) = alpha_t(s) beta_t(s) / P,  P = alpha_T(end).  Per emitting state the pass sums gamma_t(s),
// gamma_t(s) x_t and gamma_t(s) x_t^2 over the t whose x_t is a number.
//
// Forward half (posterior_forward_kernel): the p plane of forward_kernel -- same lane layout, same in-edge registers, same silent
// phase (affine-map scan along the chains, n_stages rounds) -- with one third of its LDS.  After EVERY time step the vector is
// multiplied by 2^-e, e the exponent of its largest emitting cell; the scaled emitting cells and the running exponent go to HBM.
//
// Backward half (posterior_backward_kernel): the transposed image (PostModel).  One LDS vector Y per wave: at step t its emitting
// cells hold  b_j(x_t+1) beta_t+1(j), its silent cells beta_t.  A step
//   1. writes the emitting cells from the lane's registers (beta_t+1 of its own cells),
//   2. resolves the silent cells: own[q] = what the out-edge rows of q gather from Y, then along a chain
//          y[q] = own[q] + a[q + 1] y[q + 1]
//      -- the recurrence of the forward silent phase running the other way: every lane folds its slots, last first, into an affine map,
//      a suffix scan (four row_shl DPP steps inside the rows of 16, the three row carries through v_readlane) gives every lane what
//      enters it from lane + 1, and the slots are evaluated serially.  Out-edges into silent states that are no chain edges go
//      through LDS, the phase repeated n_stages times from scratch like the forward one,
//   3. gathers beta_t of the lane's emitting cells from Y through their out-edge rows, rescales by a power of two like the forward
//      half (exponent of the largest emitting cell), and
//   4. combines: gamma = alpha_t beta_t 2^(ea_t + eb_t - ea_T) / p_T from the stored vector, three additions per emitting slot into
//      the lane's own registers, in descending t.  One store per state at the end.
// The out-edge rows are read from memory in every step (they stay in the caches: a few KB per model) -- their degrees are not bounded
// by the kernel shapes, which are cut for in-degrees.
//
// Range: as forward_kernels.hip says for one vector, for either direction.  alpha_t(s) beta_t(s) is formed before the exponents are
// applied: a state more than 2^-1022 below the largest cell of BOTH vectors at once contributes +0.0.
//
// Determinism: a window is summed by one wave in an order fixed by the model image and t -- no atomics on values, no tree reduction,
// nothing that depends on the launch geometry, on which windows share a launch or on where the workspace lies.
#include "strq_opt.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "posterior_kernels.h"
#include "hmm_wave.h"

namespace strq {

#define POST_WAVES 4

// lane l receives lane l + 1; lane 63 receives +0.0 (readlane inside the wave: the rows of 16 end at lanes 15, 31, 47)
static __device__ __forceinline__ double post_shl1(double v, int lane)
{
    const double in_row = row_shl_f64<1>(0.0, v);
    const double r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
    return lane == 15 ? r1 : (lane == 31 ? r2 : (lane == 47 ? r3 : in_row));
}
// the power of two that brings the largest of the lane values v[0 .. N) of the wave (all >= 0) into [1, 2): its exponent, 0 when
// nothing is above 2^-1043 (no path is alive -- nothing to scale by)
template <int N>
static __device__ __forceinline__ int post_exponent(const double (&v)[N])
{
    int hi = 0;          // v >= 0: the high word orders like the value
#pragma unroll
    for (int s = 0; s < N; ++s) { const int h = (int)(uint32_t)(__builtin_bit_cast(uint64_t, v[s]) >> 32); hi = h > hi ? h : hi; }
    hi = wave_max_i32(hi);
    return hi == 0 ? 0 : ((hi >> 20) & 0x7FF) - 1023;
}
template <int EPL, int SPL, int DE, int DS>
__global__ void __launch_bounds__(64 * POST_WAVES)
posterior_forward_kernel(const VitTask* __restrict__ tasks, const PostModel* const* __restrict__ models, const PostTask* __restrict__ post,
                         FwdResult* __restrict__ results, int n_tasks, int* __restrict__ queue, const int* __restrict__ order, int cells_cap)
{
    extern __shared__ double post_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // this wave's slice: the state vector of the previous / current time step, cells_cap doubles each; cell numbering of VitModel,
    // the last cell of the model (n_cells - 1) holds 0 for padding edges
    const int BUF = cells_cap;
    double* const vbase = post_lds + (size_t)wave * 2 * BUF;
    const PostModel* cur = nullptr;
    int m_end = 0, n_stages = 1, m_epl = 0;
    bool has_e[EPL]; int ekind[EPL], ecell[EPL];
    int esrc[EPL][DE]; double ew[EPL][DE];
    double ea[EPL], eb[EPL], ec[EPL], eu[EPL];
    bool has_s[SPL], is_start[SPL]; int scell[SPL];
    int ssrc[SPL][DS]; double sw[SPL][DS], cw[SPL];

    for (;;) {
        const int tq = wave_next_task(queue, lane);
        if (tq >= n_tasks) break;
        const int ti = order ? order[tq] : tq;        // longest observation windows first
        const VitTask tk = tasks[ti];
        const PostTask pk = post[ti];
        const PostModel* pm = models[ti];
        if (pm != cur) {
            cur = pm;
            const FwdModel* fm = pm->fwd;
            const VitModel& M = *fm->vit;
            m_end = M.end_cell; n_stages = fm->n_stages; m_epl = M.epl;
            const int dummy = M.n_cells - 1, scell0 = M.epl * 64;
#pragma unroll
            for (int s = 0; s < EPL; ++s) {
                const bool on = s < M.epl;
                const int st = on ? M.own_e[s * 64 + lane] : -1;
                has_e[s] = st >= 0; ecell[s] = s * 64 + lane;
                ekind[s] = on ? M.emis_kind[s * 64 + lane] : 0;
                ea[s] = ekind[s] ? M.emis_a[s * 64 + lane] : 0.0; eb[s] = ekind[s] ? M.emis_b[s * 64 + lane] : 0.0;
                ec[s] = ekind[s] ? M.emis_c[s * 64 + lane] : 0.0;
                eu[s] = ekind[s] == 2 ? exp(ec[s]) : 0.0;
#pragma unroll
                for (int j = 0; j < DE; ++j) {
                    const bool ej = on && j < M.e_deg[s];
                    esrc[s][j] = ej ? M.edge_src[(M.e_base[s] + j) * 64 + lane] : dummy;
                    ew[s][j] = ej ? fm->edge_w[(M.e_base[s] + j) * 64 + lane] : 0.0;
                }
            }
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                const bool on = s < M.spl;
                const int st = on ? M.own_s[s * 64 + lane] : -1;
                has_s[s] = st >= 0; is_start[s] = st >= 0 && st == M.start;
                scell[s] = scell0 + lane * M.spl + s;          // chain position lane * spl + s (VitModel)
                cw[s] = on ? fm->chain_w[s * 64 + lane] : 1.0;          // a slot the model does not use passes the chain value on
#pragma unroll
                for (int j = 0; j < DS; ++j) {
                    const bool ej = on && j < M.s_deg[s];
                    ssrc[s][j] = ej ? M.edge_src[(M.s_base[s] + j) * 64 + lane] : dummy;
                    sw[s][j] = ej ? fm->edge_w[(M.s_base[s] + j) * 64 + lane] : 0.0;
                }
            }
        }
        const int64_t T = tk.T;
        for (int i = lane; i < 2 * BUF; i += 64) vbase[i] = 0.0;
        wave_fence();

        // silent states of the vector at `X` (its emitting cells are final); `pin`: the start state holds the whole mass (t = 0)
        auto silent_phase = [&](double* X, bool pin) {
            for (int round = 0; round < n_stages; ++round) {
                double own[SPL];
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    double p = 0.0;
#pragma unroll
                    for (int j = 0; j < DS; ++j) p = p + sw[s][j] * X[ssrc[s][j]];
                    if (pin && is_start[s]) p = 1.0;
                    own[s] = p;
                }
                // the lane's slots as one affine map y_out = B + A * y_in
                double A = cw[0], B = own[0];
#pragma unroll
                for (int s = 1; s < SPL; ++s) { B = own[s] + cw[s] * B; A = cw[s] * A; }
                // inclusive scan of the maps inside each row of 16 lanes
#define POST_SCAN_STEP(N)                                                                          \
                {                                                                                  \
                    const double a_src = row_shr_f64<N>(1.0, A), b_src = row_shr_f64<N>(0.0, B); \
                    B = B + A * b_src; A = A * a_src;                                              \
                }
                POST_SCAN_STEP(1) POST_SCAN_STEP(2) POST_SCAN_STEP(4) POST_SCAN_STEP(8)
#undef POST_SCAN_STEP
                // what enters a row: the last slot of the last lane of the row before (nothing enters row 0)
                const int row = lane >> 4;
                const double c1 = readlane_f64(B, 15);
                const double c2 = readlane_f64(B, 31) + readlane_f64(A, 31) * c1;
                const double c3 = readlane_f64(B, 47) + readlane_f64(A, 47) * c2;
                const double cin = row == 0 ? 0.0 : (row == 1 ? c1 : (row == 2 ? c2 : c3));
                const double ylast = B + A * cin;
                wave_fence();          // every lane has read the vector before anyone overwrites its silent cells
                double y = dpp_shr1_f64(ylast);
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    y = own[s] + cw[s] * y;
                    if (has_s[s]) X[scell[s]] = y;
                }
                wave_fence();
            }
        };

        silent_phase(vbase, true);

        int expo = 0, n_rescaled = 0;
        double xchunk = 0.0;
        for (int64_t t0 = 0; t0 < T; t0 += 64) {
            {   // observations t0 .. t0 + 63, one per lane: the window as the Viterbi kernels read it
                const int64_t idx = t0 + lane;
                double xv = 0.0;
                if (idx < T) xv = vit_observation(tk, idx);
                xchunk = xv;
            }
            const int send = (int)((T - t0) < 64 ? (T - t0) : 64);
            for (int s0 = 0; s0 < send; ++s0) {
                const double x = readlane_f64(xchunk, s0);
                const int64_t t = t0 + s0;
                const double* const RD = vbase + (t & 1) * BUF;
                double* const WR = vbase + ((t + 1) & 1) * BUF;
                double np_[EPL];
#pragma unroll
                for (int s = 0; s < EPL; ++s) {
                    double p = 0.0;
#pragma unroll
                    for (int j = 0; j < DE; ++j) p = p + ew[s][j] * RD[esrc[s][j]];
                    np_[s] = p * hmm_emission(x, has_e[s], ekind[s], ea[s], eb[s], ec[s], eu[s]);
                }
                const int e = post_exponent(np_);
                if (e != 0) {
#pragma unroll
                    for (int s = 0; s < EPL; ++s) np_[s] = __builtin_ldexp(np_[s], -e);
                    expo += e; ++n_rescaled;
                }
#pragma unroll
                for (int s = 0; s < EPL; ++s) {
                    if (has_e[s]) WR[ecell[s]] = np_[s];
                    if (pk.alpha && s < m_epl) pk.alpha[((size_t)t * (size_t)m_epl + (size_t)s) * 64 + lane] = np_[s];
                }
                if (pk.expo && lane == 0) pk.expo[t] = expo;
                wave_fence();
                silent_phase(WR, false);
            }
        }
        const double* const FIN = vbase + (T & 1) * BUF;
        FwdResult res;
        res.p = FIN[m_end]; res.r = 0.0; res.s = 0.0;
        res.expo = expo; res.steps_rescaled = n_rescaled; res.pad_ = 0;
        if (lane == 0) results[ti] = res;
        wave_fence();
    }
}

template <int EPL, int SPL>
__global__ void __launch_bounds__(64 * POST_WAVES)
posterior_backward_kernel(const VitTask* __restrict__ tasks, const PostModel* const* __restrict__ models, const PostTask* __restrict__ post,
                          const FwdResult* __restrict__ results, int n_tasks, int* __restrict__ queue, const int* __restrict__ order, int cells_cap)
{
    extern __shared__ double post_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* const Y = post_lds + (size_t)wave * cells_cap;          // see the head of the file; the model's last cell holds 0
    const PostModel* cur = nullptr;
    int n_stages = 1, m_epl = 0, n_cells = 0;
    int oe_deg[EPL], oe_base[EPL], os_deg[SPL], os_base[SPL];
    const int32_t* out_dst = nullptr; const double* out_w = nullptr;
    bool has_e[EPL]; int ekind[EPL], ecell[EPL], estate[EPL];
    double ea[EPL], eb[EPL], ec[EPL], eu[EPL];
    bool has_s[SPL], is_end[SPL]; int scell[SPL];
    double nw[SPL];

    for (;;) {
        const int tq = wave_next_task(queue, lane);
        if (tq >= n_tasks) break;
        const int ti = order ? order[tq] : tq;
        const VitTask tk = tasks[ti];
        const PostTask pk = post[ti];
        const FwdResult fr = results[ti];
        if (!pk.alpha || !(fr.p > 0.0)) continue;          // not stored, or no path: the rows stay zero
        const PostModel* pm = models[ti];
        if (pm != cur) {
            cur = pm;
            const FwdModel* fm = pm->fwd;
            const VitModel& M = *fm->vit;
            n_stages = fm->n_stages; m_epl = M.epl; n_cells = M.n_cells;
            out_dst = pm->out_dst; out_w = pm->out_w;
            const int scell0 = M.epl * 64;
#pragma unroll
            for (int s = 0; s < EPL; ++s) {
                const bool on = s < M.epl;
                const int st = on ? M.own_e[s * 64 + lane] : -1;
                has_e[s] = st >= 0; estate[s] = st; ecell[s] = s * 64 + lane;
                ekind[s] = on ? M.emis_kind[s * 64 + lane] : 0;
                ea[s] = ekind[s] ? M.emis_a[s * 64 + lane] : 0.0; eb[s] = ekind[s] ? M.emis_b[s * 64 + lane] : 0.0;
                ec[s] = ekind[s] ? M.emis_c[s * 64 + lane] : 0.0;
                eu[s] = ekind[s] == 2 ? exp(ec[s]) : 0.0;
                oe_deg[s] = on ? pm->oe_deg[s] : 0; oe_base[s] = on ? pm->oe_base[s] : 0;
            }
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                const bool on = s < M.spl;
                const int st = on ? M.own_s[s * 64 + lane] : -1;
                has_s[s] = st >= 0; is_end[s] = st >= 0 && st == M.end;
                scell[s] = scell0 + lane * M.spl + s;
                nw[s] = on ? pm->chain_next_w[s * 64 + lane] : 1.0;          // a slot the model does not use passes the chain value on
                os_deg[s] = on ? pm->os_deg[s] : 0; os_base[s] = on ? pm->os_base[s] : 0;
            }
        }
        const int64_t T = tk.T;
        for (int i = lane; i < n_cells; i += 64) Y[i] = 0.0;
        wave_fence();

        // silent cells of Y (its emitting cells are final); `pin`: the end state holds the whole mass (t = T)
        auto silent_phase = [&](bool pin) {
            for (int round = 0; round < n_stages; ++round) {
                double own[SPL];
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    double p = 0.0;
                    for (int j = 0; j < os_deg[s]; ++j) {
                        const int at = (os_base[s] + j) * 64 + lane;
                        p = p + out_w[at] * Y[out_dst[at]];
                    }
                    if (pin && is_end[s]) p = 1.0;
                    own[s] = p;
                }
                // the lane's slots, last first, as one affine map y_out = B + A * y_in (y_in: the first slot of lane + 1)
                double A = nw[SPL - 1], B = own[SPL - 1];
#pragma unroll
                for (int s = SPL - 2; s >= 0; --s) { B = own[s] + nw[s] * B; A = nw[s] * A; }
                // inclusive suffix scan of the maps inside each row of 16 lanes
#define POST_SCAN_STEP(N)                                                                          \
                {                                                                                  \
                    const double a_src = row_shl_f64<N>(1.0, A), b_src = row_shl_f64<N>(0.0, B); \
                    B = B + A * b_src; A = A * a_src;                                              \
                }
                POST_SCAN_STEP(1) POST_SCAN_STEP(2) POST_SCAN_STEP(4) POST_SCAN_STEP(8)
#undef POST_SCAN_STEP
                // what enters a row: the first slot of the first lane of the row behind (nothing enters row 3)
                const int row = lane >> 4;
                const double c2 = readlane_f64(B, 48);
                const double c1 = readlane_f64(B, 32) + readlane_f64(A, 32) * c2;
                const double c0 = readlane_f64(B, 16) + readlane_f64(A, 16) * c1;
                const double cin = row == 3 ? 0.0 : (row == 2 ? c2 : (row == 1 ? c1 : c0));
                const double yfirst = B + A * cin;
                wave_fence();          // every lane has read the vector before anyone overwrites its silent cells
                double y = post_shl1(yfirst, lane);
#pragma unroll
                for (int s = SPL - 1; s >= 0; --s) {
                    y = own[s] + nw[s] * y;
                    if (has_s[s]) Y[scell[s]] = y;
                }
                wave_fence();
            }
        };

        const double inv_p = 1.0 / fr.p;
        const int ea_T = (int)fr.expo;
        double beta[EPL], aw[EPL], awx[EPL], awxx[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) { beta[s] = 0.0; aw[s] = 0.0; awx[s] = 0.0; awxx[s] = 0.0; }
        int eb_t = 0;
        double x_next = 0.0;          // x_t+1: the observation the step before this one (t + 1) combined with
        // chunks of 64 observations, last first; inside a chunk t = t0 + s0 + 1 walks downwards
        for (int64_t t0 = ((T - 1) / 64) * 64; t0 >= 0 && T > 0; t0 -= 64) {
            double xchunk = 0.0; int echunk = 0;
            {
                const int64_t idx = t0 + lane;
                if (idx < T) { xchunk = vit_observation(tk, idx); echunk = pk.expo[idx]; }
            }
            const int send = (int)((T - t0) < 64 ? (T - t0) : 64);
            for (int s0 = send - 1; s0 >= 0; --s0) {
                const double x = readlane_f64(xchunk, s0);          // x_t
                const int ea_t = __builtin_amdgcn_readlane(echunk, s0);
                const int64_t t = t0 + s0 + 1;                        // 1-based time step: alpha_t is the stored vector t - 1
                const bool last = t == T;
                // 1. emitting cells: b_j(x_t+1) beta_t+1(j); nothing follows the last observation
#pragma unroll
                for (int s = 0; s < EPL; ++s)
                    if (has_e[s]) Y[ecell[s]] = last ? 0.0 : beta[s] * hmm_emission(x_next, true, ekind[s], ea[s], eb[s], ec[s], eu[s]);
                wave_fence();
                // 2. silent cells
                silent_phase(last);
                // 3. beta_t of the lane's emitting cells
#pragma unroll
                for (int s = 0; s < EPL; ++s) {
                    double b = 0.0;
                    for (int j = 0; j < oe_deg[s]; ++j) {
                        const int at = (oe_base[s] + j) * 64 + lane;
                        b = b + out_w[at] * Y[out_dst[at]];
                    }
                    beta[s] = has_e[s] ? b : 0.0;
                }
                wave_fence();          // every lane has read Y before step 1 of the next time step overwrites its emitting cells
                const int e = post_exponent(beta);
                if (e != 0) {
#pragma unroll
                    for (int s = 0; s < EPL; ++s) beta[s] = __builtin_ldexp(beta[s], -e);
                    eb_t += e;
                }
                // 4. gamma_t, summed where x_t is a number
                if (x == x) {
                    const int d = ea_t + eb_t - ea_T;
#pragma unroll
                    for (int s = 0; s < EPL; ++s) {
                        if (!has_e[s] || s >= m_epl) continue;
                        const double a = pk.alpha[((size_t)(t - 1) * (size_t)m_epl + (size_t)s) * 64 + lane];
                        const double g = __builtin_ldexp(a * beta[s], d) * inv_p;
                        aw[s] = aw[s] + g; awx[s] = awx[s] + g * x; awxx[s] = awxx[s] + (g * x) * x;
                    }
                }
                x_next = x;
            }
        }
#pragma unroll
        for (int s = 0; s < EPL; ++s)
            if (has_e[s]) { pk.w[estate[s]] = aw[s]; pk.wx[estate[s]] = awx[s]; pk.wxx[estate[s]] = awxx[s]; }
        wave_fence();
    }
}

// instance F of VIT_FWD_SHAPES
template <int F>
static int post_launch_shape(hipStream_t stream, int max_cells, const VitTask* tasks, const PostModel* const* models, const PostTask* post,
                             FwdResult* results, int n_tasks, int* queue, int n_cu, const int* order)
{
    constexpr int EPL = VIT_FWD_SHAPES[F].epl, SPL = VIT_FWD_SHAPES[F].spl, DE = VIT_FWD_SHAPES[F].de, DS = VIT_FWD_SHAPES[F].ds;
    if (max_cells > (EPL + SPL) * 64 + 1) return 2;
    const size_t lds_f = (size_t)POST_WAVES * 2 * (size_t)max_cells * sizeof(double), lds_b = lds_f / 2;
    if (lds_f > 160 * 1024) return 2;
    int blocks = (n_tasks + POST_WAVES - 1) / POST_WAVES;
    if (blocks > 2 * n_cu) blocks = 2 * n_cu;
    (void)hipFuncSetAttribute((const void*)posterior_forward_kernel<EPL, SPL, DE, DS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_f);
    hipLaunchKernelGGL((posterior_forward_kernel<EPL, SPL, DE, DS>), dim3(blocks), dim3(64 * POST_WAVES), lds_f, stream,
                       tasks, models, post, results, n_tasks, queue, order, max_cells);
    if (hipGetLastError() != hipSuccess) return 1;
    (void)hipFuncSetAttribute((const void*)posterior_backward_kernel<EPL, SPL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b);
    hipLaunchKernelGGL((posterior_backward_kernel<EPL, SPL>), dim3(blocks), dim3(64 * POST_WAVES), lds_b, stream,
                       tasks, models, post, (const FwdResult*)results, n_tasks, queue + 1, order, max_cells);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// one instance per family of lane layouts: the `fwd` column of VIT_SHAPES
int launch_posterior(hipStream_t stream, int shape, int max_cells, const VitTask* tasks, const PostModel* const* models,
                     const PostTask* post, FwdResult* results, int n_tasks, int* queue, int n_cu, const int* order)
{
    if (n_tasks <= 0) return 0;
    if (vit_shape_family(shape) != VIT_FAMILY_LANE) return 2;
    return vit_dispatch<(int)(sizeof(VIT_FWD_SHAPES) / sizeof(VIT_FWD_SHAPES[0]))>(VIT_SHAPES[shape & ~VIT_SHAPE_SS].fwd, [&](auto f) {
        return post_launch_shape<decltype(f)::value>(stream, max_cells, tasks, models, post, results, n_tasks, queue, n_cu, order);
    });
}

}  // namespace strq
