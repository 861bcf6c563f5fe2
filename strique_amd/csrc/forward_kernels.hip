// Forward algorithm on gfx950: one wave64 per observation window, float64, linear space.
//
// Replaces pomegranate 0.10.0 HiddenMarkovModel.log_probability(x) for the model of scripts/STRique.py:384-431, and carries
// the first two moments of the visit count v (observations emitted from the counted states repeatdummy1 / repeatdummy2,
// STRique.py:374-378,437) along with the probability mass -- the second-order expectation semiring: every state holds
//     p = sum over the paths that reach it of P(path, x_1..t),   r = sum of P * u,   s = sum of P * u^2,     u = v - c0.
// An edge or an emission multiplies all three by the same factor; an emission from a counted state maps
// (p, r, s) -> (p, r + p, s + 2 r + p).  At the end state  log_lik = log p,  E[v] = c0 + r / p,  Var[v] = s / p - (r / p)^2.
// c0 is the visit count of the Viterbi path: moments about it stay O(1) where moments about zero (v ~ 1000) would cancel
// twelve digits in s / p - (r / p)^2.  r is signed; linear space allows that.
//
// Same lane layout as viterbi_kernel (VitModel: EPL emitting + SPL silent slots per lane, in-edges in registers, the state
// vector of the previous / current time step in this wave's LDS slice), with the transition probabilities of FwdModel.
// Two things differ from a max-plus decode:
//
//  * Silent chains.  A sum is not idempotent, so the chains cannot be swept until nothing changes.  Along a chain
//        y[q] = own[q] + a[q] * y[q - 1]
//    (own: what the non-chain in-edges bring) is a linear recurrence: every lane folds its SPL slots into one affine map
//    y_out = B + A * y_in, a prefix scan over the maps of the 64 lanes (four row_shr DPP steps inside the rows of 16, the three
//    row carries through v_readlane) gives every lane its y_in, and the slots of a lane are then evaluated serially.  Every
//    predecessor enters exactly once.  Silent edges that are no chain edges (none in STRique's flanked models) go through LDS:
//    the silent phase is repeated FwdModel::n_stages times -- a fixed number, the depth of those edges -- each time from scratch,
//    so that after round k all states of depth <= k hold their final value.
//
//  * Range.  log_lik reaches -1e5 at 50 k samples.  After the emitting phase of a time step the whole vector is multiplied by
//    2^-e, e the exponent of its largest p, and e is added to an integer: a power of two scales exactly, so the result does not
//    depend on how often this happens (rescale_every, STRQ_FWD_RESCALE_EVERY) as long as nothing under- or overflows in
//    between.  What remains is the range of one vector: a state whose mass is below 2^-1022 of the largest one is lost, and a
//    time step on which EVERY state's emission density underflows (an observation hundreds of sigma from every Normal and
//    outside every Uniform) ends all paths where log space would keep one.
//
// Determinism: a window is summed by one wave in an order fixed by the model image alone -- no atomics on values, nothing that
// depends on the launch geometry or on which windows share the launch.
#include "strq_opt.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "forward_kernels.h"
#include "hmm_wave.h"

namespace strq {

#define FWD_WAVES 4

// x * 2^-e, exactly
static __device__ __forceinline__ double fwd_scale(double x, int e) { return __builtin_ldexp(x, -e); }

template <int EPL, int SPL, int DE, int DS>
__global__ void __launch_bounds__(64 * FWD_WAVES)
forward_kernel(const VitTask* __restrict__ tasks, const FwdModel* const* __restrict__ models, const int64_t* __restrict__ c0s,
               FwdResult* __restrict__ results, int n_tasks, int* __restrict__ queue, const int* __restrict__ order,
               int cells_cap, int rescale_every)
{
    extern __shared__ double fwd_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // this wave's slice: two state vectors of three planes (p, r, s) of cells_cap doubles each; cell numbering of VitModel,
    // the last cell of the model (n_cells - 1) holds 0 for padding edges
    const int PL = cells_cap, BUF = 3 * cells_cap;
    double* const vbase = fwd_lds + (size_t)wave * 2 * BUF;
    const FwdModel* cur = nullptr;
    int NP = 0, m_start = 0, m_end = 0, n_stages = 1;
    bool has_e[EPL], ecnt[EPL]; int ekind[EPL], ecell[EPL];
    int esrc[EPL][DE]; double ew[EPL][DE];
    double ea[EPL], eb[EPL], ec[EPL], eu[EPL];       // eu: density of a Uniform emission
    bool has_s[SPL], is_start[SPL]; int scell[SPL];
    int ssrc[SPL][DS]; double sw[SPL][DS], cw[SPL];

    for (;;) {
        const int tq = wave_next_task(queue, lane);
        if (tq >= n_tasks) break;
        const int ti = order ? order[tq] : tq;        // longest observation windows first
        const VitTask tk = tasks[ti];
        const FwdModel* fm = models[ti];
        if (fm != cur) {
            cur = fm;
            const VitModel& M = *fm->vit;
            NP = M.n_cells; m_start = M.start_cell; m_end = M.end_cell; n_stages = fm->n_stages;
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
                ecnt[s] = st >= 0 && M.count_inc[st] != 0;
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
        const double c0 = (double)(c0s ? c0s[ti] : 0);
        for (int i = lane; i < 2 * BUF; i += 64) vbase[i] = 0.0;
        wave_fence();
        (void)NP;

        // silent states of the vector at `X` (its emitting cells are final); `pin`: the start state holds the whole mass (t = 0)
        auto silent_phase = [&](double* X, bool pin) {
            for (int round = 0; round < n_stages; ++round) {
                double own[SPL][3];
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    double p = 0.0, r = 0.0, q = 0.0;
#pragma unroll
                    for (int j = 0; j < DS; ++j) {
                        const int cidx = ssrc[s][j]; const double w = sw[s][j];
                        p = p + w * X[cidx]; r = r + w * X[PL + cidx]; q = q + w * X[2 * PL + cidx];
                    }
                    if (pin && is_start[s]) { p = 1.0; r = -c0; q = c0 * c0; }
                    own[s][0] = p; own[s][1] = r; own[s][2] = q;
                }
                // the lane's slots as one affine map y_out = B + A * y_in
                double A = cw[0], B[3] = {own[0][0], own[0][1], own[0][2]};
#pragma unroll
                for (int s = 1; s < SPL; ++s) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) B[k] = own[s][k] + cw[s] * B[k];
                    A = cw[s] * A;
                }
                // inclusive scan of the maps inside each row of 16 lanes
#define FWD_SCAN_STEP(N)                                                                           \
                {                                                                                  \
                    const double a_src = row_shr_f64<N>(1.0, A);                                   \
                    const double b0 = row_shr_f64<N>(0.0, B[0]), b1 = row_shr_f64<N>(0.0, B[1]), b2 = row_shr_f64<N>(0.0, B[2]); \
                    B[0] = B[0] + A * b0; B[1] = B[1] + A * b1; B[2] = B[2] + A * b2;              \
                    A = A * a_src;                                                                 \
                }
                FWD_SCAN_STEP(1) FWD_SCAN_STEP(2) FWD_SCAN_STEP(4) FWD_SCAN_STEP(8)
#undef FWD_SCAN_STEP
                // what enters a row: the last slot of the last lane of the row before (nothing enters row 0)
                const int row = lane >> 4;
                double ylast[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double c1 = readlane_f64(B[k], 15);
                    const double c2 = readlane_f64(B[k], 31) + readlane_f64(A, 31) * c1;
                    const double c3 = readlane_f64(B[k], 47) + readlane_f64(A, 47) * c2;
                    const double cin = row == 0 ? 0.0 : (row == 1 ? c1 : (row == 2 ? c2 : c3));
                    ylast[k] = B[k] + A * cin;
                }
                wave_fence();          // every lane has read the vector before anyone overwrites its silent cells
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double y = dpp_shr1_f64(ylast[k]);
#pragma unroll
                    for (int s = 0; s < SPL; ++s) {
                        y = own[s][k] + cw[s] * y;
                        if (has_s[s]) X[k * PL + scell[s]] = y;
                    }
                }
                wave_fence();
            }
        };

        silent_phase(vbase, true);

        int64_t expo = 0; int n_rescaled = 0;
        int since = 0;
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
                double np_[EPL], nr_[EPL], nq_[EPL];
#pragma unroll
                for (int s = 0; s < EPL; ++s) {
                    double p = 0.0, r = 0.0, q = 0.0;
#pragma unroll
                    for (int j = 0; j < DE; ++j) {
                        const int cidx = esrc[s][j]; const double w = ew[s][j];
                        p = p + w * RD[cidx]; r = r + w * RD[PL + cidx]; q = q + w * RD[2 * PL + cidx];
                    }
                    const double em = hmm_emission(x, has_e[s], ekind[s], ea[s], eb[s], ec[s], eu[s]);
                    p = p * em; r = r * em; q = q * em;
                    if (ecnt[s]) { q = q + 2.0 * r + p; r = r + p; }
                    np_[s] = p; nr_[s] = r; nq_[s] = q;
                }
                if (++since >= rescale_every) {
                    since = 0;
                    int hi = 0;          // p >= 0: the high word orders like the value
#pragma unroll
                    for (int s = 0; s < EPL; ++s) { const int h = (int)(uint32_t)(__builtin_bit_cast(uint64_t, np_[s]) >> 32); hi = h > hi ? h : hi; }
                    hi = wave_max_i32(hi);
                    if (hi != 0) {          // (zero: no path is alive, or nothing above 2^-1043 -- nothing to scale by)
                        const int e = ((hi >> 20) & 0x7FF) - 1023;
                        if (e != 0) {
#pragma unroll
                            for (int s = 0; s < EPL; ++s) { np_[s] = fwd_scale(np_[s], e); nr_[s] = fwd_scale(nr_[s], e); nq_[s] = fwd_scale(nq_[s], e); }
                            expo += e; ++n_rescaled;
                        }
                    }
                }
#pragma unroll
                for (int s = 0; s < EPL; ++s)
                    if (has_e[s]) { WR[ecell[s]] = np_[s]; WR[PL + ecell[s]] = nr_[s]; WR[2 * PL + ecell[s]] = nq_[s]; }
                wave_fence();
                silent_phase(WR, false);
            }
        }
        const double* const FIN = vbase + (T & 1) * BUF;
        FwdResult res;
        res.p = FIN[m_end]; res.r = FIN[PL + m_end]; res.s = FIN[2 * PL + m_end];
        res.expo = expo; res.steps_rescaled = n_rescaled; res.pad_ = 0;
        if (lane == 0) results[ti] = res;
        wave_fence();
    }
}

// instance F of VIT_FWD_SHAPES
template <int F>
static int fwd_launch_shape(hipStream_t stream, int max_cells, const VitTask* tasks, const FwdModel* const* models, const int64_t* c0,
                            FwdResult* results, int n_tasks, int* queue, int n_cu, const int* order, int rescale_every)
{
    constexpr int EPL = VIT_FWD_SHAPES[F].epl, SPL = VIT_FWD_SHAPES[F].spl, DE = VIT_FWD_SHAPES[F].de, DS = VIT_FWD_SHAPES[F].ds;
    if (max_cells > (EPL + SPL) * 64 + 1) return 2;
    const size_t lds = (size_t)FWD_WAVES * 2 * 3 * (size_t)max_cells * sizeof(double);
    if (lds > 160 * 1024) return 2;
    int blocks = (n_tasks + FWD_WAVES - 1) / FWD_WAVES;
    if (blocks > 2 * n_cu) blocks = 2 * n_cu;
    (void)hipFuncSetAttribute((const void*)forward_kernel<EPL, SPL, DE, DS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((forward_kernel<EPL, SPL, DE, DS>), dim3(blocks), dim3(64 * FWD_WAVES), lds, stream,
                       tasks, models, c0, results, n_tasks, queue, order, max_cells, rescale_every);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// one instance per family of lane layouts: the `fwd` column of VIT_SHAPES
int launch_forward(hipStream_t stream, int shape, int max_cells, const VitTask* tasks, const FwdModel* const* models,
                   const int64_t* c0, FwdResult* results, int n_tasks, int* queue, int n_cu, const int* order, int rescale_every)
{
    if (n_tasks <= 0) return 0;
    if (rescale_every < 1) rescale_every = 1;
    if (vit_shape_family(shape) != VIT_FAMILY_LANE) return 2;
    return vit_dispatch<(int)(sizeof(VIT_FWD_SHAPES) / sizeof(VIT_FWD_SHAPES[0]))>(VIT_SHAPES[shape & ~VIT_SHAPE_SS].fwd, [&](auto f) {
        return fwd_launch_shape<decltype(f)::value>(stream, max_cells, tasks, models, c0, results, n_tasks, queue, n_cu, order, rescale_every);
    });
}

}  // namespace strq
