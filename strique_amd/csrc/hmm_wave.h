// Internal: what the wave-per-window HMM kernels share (viterbi_kernels.hip, forward_kernels.hip, posterior_kernels.hip,
// mod_llr_kernels.hip, motif_kernels.hip) -- the fetch of the next task, lane exchange of doubles, the DPP row shifts and the wave maximum of the
// linear-space kernels with their emission density, the wavefront fence, and how a window is read from its VitTask.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vit_model.h"

namespace strq {

// orders this wave's LDS accesses: the lanes of a wave exchange values through LDS without a workgroup barrier
static __device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
// the next index of a launch's task queue, the same in every lane
static __device__ __forceinline__ int wave_next_task(int* queue, int lane)
{
    __builtin_amdgcn_wave_barrier();
    int ti = 0;
    if (lane == 0) ti = atomicAdd(queue, 1);
    __builtin_amdgcn_wave_barrier();
    ti = __builtin_amdgcn_readfirstlane(ti);
    __builtin_amdgcn_wave_barrier();
    return ti;
}
static __device__ __forceinline__ double readlane_f64(double v, int l)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)u, l);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// wave_shr:1 -- lane l receives lane l-1; lane 0 receives +0.0 (bound_ctrl)
static __device__ __forceinline__ double dpp_shr1_f64(double v)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, 0x138, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), 0x138, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// DPP row shifts of a double inside the rows of 16 lanes: row_shr:N (lane l receives lane l - N) / row_shl:N (lane l + N); a lane
// without a source keeps `old`.  The steps of the affine-map scans along the silent chains (forward_kernels.hip, posterior_kernels.hip).
template <int CTRL>
static __device__ __forceinline__ double wave_dpp_f64(double old, double v)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v), o = __builtin_bit_cast(uint64_t, old);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)o, (int)(uint32_t)u, CTRL, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(o >> 32), (int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
template <int N> static __device__ __forceinline__ double row_shr_f64(double old, double v) { return wave_dpp_f64<0x110 + N>(old, v); }
template <int N> static __device__ __forceinline__ double row_shl_f64(double old, double v) { return wave_dpp_f64<0x100 + N>(old, v); }
// largest value of the wave, in every lane: butterflies inside the rows of 16 (quad_perm, row_half_mirror, row_mirror), the four
// row maxima through v_readlane
static __device__ __forceinline__ int wave_max_i32(int v)
{
    int o;
    o = __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); v = v > o ? v : o;       // quad_perm [1,0,3,2]
    o = __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true); v = v > o ? v : o;       // quad_perm [2,3,0,1]
    o = __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true); v = v > o ? v : o;      // row_half_mirror
    o = __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true); v = v > o ? v : o;      // row_mirror
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    const int ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}
// Emission density of observation x in linear space (the forward and the posterior kernels): a missing observation (NaN) has
// probability 1 under every distribution (`has`: the slot holds a state); kind 1 Normal (a = mu, b = 1 / (2 sigma^2), c = the log
// norm), kind 2 Uniform (a, b = its support, u = its density), 0 padding
static __device__ __forceinline__ double hmm_emission(double x, bool has, int kind, double a, double b, double c, double u)
{
    double em;
    if (x != x) em = has ? 1.0 : 0.0;
    else if (kind == 1) { const double d = x - a; em = exp(c - (d * d) * b); }
    else if (kind == 2) em = (x >= a && x <= b) ? u : 0.0;
    else em = 0.0;
    return em;
}
// Log emission density of observation x, as oracle/viterbi_oracle.c writes it (the motif track; the Viterbi and score kernels
// carry the same expressions inline): a missing observation (NaN) has log-probability 0 under every distribution; kind 1 Normal
// c - (x - a)^2 b, otherwise Uniform: c inside [a, b], -inf outside.  A lane without a state (kind 0) must not use the value.
static __device__ __forceinline__ double hmm_log_emission(double x, int kind, double a, double b, double c)
{
    const double d = x - a;
    const double en = c - (d * d) * b;
    const double eu = (x >= a && x <= b) ? c : -INFINITY;
    double em = kind == 1 ? en : eu;
    if (x != x) em = 0.0;
    return em;
}
// Observation `idx` (< T: the caller tests it) of a window: x = clip((s - c1) / h1 * h2 + c2, lo, hi) for the affine sources.
// The count decode and the unit, confidence and anchored passes are bit-equal because they all read a window through this.
static __device__ __forceinline__ double vit_observation(const VitTask& tk, int64_t idx)
{
    if (tk.src_kind == VIT_SRC_F64) return reinterpret_cast<const double*>(tk.sig)[idx];
    double sv = tk.src_kind == VIT_SRC_I16_AFFINE ? (double)reinterpret_cast<const int16_t*>(tk.sig)[idx]
                                                  : reinterpret_cast<const double*>(tk.sig)[idx];
    sv = (sv - tk.c1) / tk.h1;
    sv = sv * tk.h2 + tk.c2;
    sv = sv < tk.lo ? tk.lo : sv;          // np.clip
    sv = sv > tk.hi ? tk.hi : sv;
    return sv;
}
// End of a MARK decode of the lane and CSR kernels: the end state's payload, lo = count | enter[11:0] << 20,  hi = enter[21:12] | leave << 10
static __device__ __forceinline__ void vit_unpack_marks(uint64_t pay, bool has_path, int64_t T, VitResult& r)
{
    const uint32_t plo = (uint32_t)pay, phi = (uint32_t)(pay >> 32);
    r.counted = has_path ? (int64_t)(plo & 0xFFFFFu) : 0;
    r.dbg[0] = (plo >> 20) | ((phi & 0x3FFu) << 12);       // time (1-based) of the first repeat-section emission, 0 = none
    r.dbg[1] = phi >> 10;                                  // time of the first emission after the repeat section, 0 = none
    if (T >= VIT_MARK_T_MAX) r.status = 2;                 // window too long for the packed marks
}

}  // namespace strq
