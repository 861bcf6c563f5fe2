// The second normalisation step on gfx950 (strq_set_renorm; the rule: strique_amd/renorm.py).
//
//   histogram   1024 bins per (read, signal) of the samples under their current, unclipped map.  Reads of int16 samples and the 8-bit
//               levels are binned from the exact histograms conditioning has already taken (the map is a function of the sample's
//               value, so a bin of those histograms falls into one bin here): nothing is streamed twice.  float64 reads are streamed
//               once, 2048 samples per workgroup, with an LDS histogram per tile.
//   fit         one workgroup per (read, signal).  The occupied bins of h (compacted) and the target's Q as int16 are in LDS; a
//               thread owns one (a, b) and accumulates S(a, b, w) for the 15 shares w in int64; lanes run along b, so a wave reads
//               consecutive cells of a row Q[w].  Coarse grid first, then the neighbourhood of its winner (the schedule of the rule);
//               the argmax with its tie rule (smallest a, then b, then w) is reduced in the wave, then over the four waves.
//   fold        the gate, the new (c1, h1) of the fitted signals in ReadCond, the 256 level values of the morphology signal.
//
// The bin of a sample and the fold are float64 expressions evaluated one rounding at a time (-ffp-contract=off), everything between
// them is integer arithmetic: the records and the maps equal those of the rule bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "renorm_kernels.h"

namespace strq {

static __device__ __forceinline__ int rn_bin(double x, double c1, double h1, double h2, double c2, double lo, double d)
{
    double v = (x - c1) / h1;
    v = v * h2 + c2;
    const double t = floor((v - lo) / d);
    return (t >= 0.0 && t < (double)RN_GRID) ? (int)t : -1;          // a NaN compares false: dropped
}

// the map of one signal of a read: x' = (x - c1) / h1 * h2 + c2 (the fields are loaded one by one: no copy of the row in scratch)
struct RnMap { double c1, h1, h2, c2; };
static __device__ __forceinline__ RnMap rn_map_of(const ReadCond* rc, int sig)
{
    RnMap m;
    if (sig == 0) { m.c1 = rc->m_c1; m.h1 = rc->m_h1; }
    else if (sig == 1) { m.c1 = rc->f_c1; m.h1 = rc->f_h1; }
    else { m.c1 = rc->r_c1; m.h1 = rc->r_h1; }
    m.h2 = rc->h2; m.c2 = rc->c2;
    return m;
}

// a read is fitted when it was conditioned and its target has tables; its raw signal when the target has a modification model
static __device__ __forceinline__ bool rn_wanted(const ReadCond* rc, const RenormRead* rr, int sig)
{
    return rc->status == COND_OK && rc->n > 0 && rr->table != nullptr && (sig != 2 || rr->raw != 0);
}

// bins of an exact histogram (`nbins` values from `bias` on, `nbins` counters per read) into h[read][sig]
__global__ void __launch_bounds__(256)
renorm_rebin_kernel(const uint32_t* __restrict__ hist_all, int nbins, int bias, int sig, const ReadCond* __restrict__ rc_all,
                    const RenormRead* __restrict__ rr_all, RenormGrid g, uint32_t* __restrict__ h_all)
{
    __shared__ uint32_t hl[RN_GRID];
    const int read = blockIdx.x, t = threadIdx.x;
    const ReadCond* rc = rc_all + read;
    if (!rn_wanted(rc, rr_all + read, sig)) return;
    const RnMap m = rn_map_of(rc, sig);
    for (int k = t; k < RN_GRID; k += 256) hl[k] = 0;
    __syncthreads();
    const uint32_t* hist = hist_all + (size_t)read * nbins;
    for (int k = t; k < nbins; k += 256) {
        const uint32_t cnt = hist[k];
        if (!cnt) continue;
        const int b = rn_bin((double)(k + bias), m.c1, m.h1, m.h2, m.c2, g.lo, g.d);
        if (b >= 0) atomicAdd(&hl[b], cnt);
    }
    __syncthreads();
    uint32_t* h = h_all + ((size_t)read * RN_SIGNALS + sig) * RN_GRID;
    for (int k = t; k < RN_GRID; k += 256) h[k] = hl[k];
}

#define RN_TILE 2048
// float64 reads: blockIdx.z = 0 the filtered signal (h[read][1]), 1 the raw signal (h[read][2])
__global__ void __launch_bounds__(256)
renorm_stream_f64_kernel(const double* __restrict__ flt_all, const double* __restrict__ raw_all, const ReadCond* __restrict__ rc_all,
                         const RenormRead* __restrict__ rr_all, RenormGrid g, uint32_t* __restrict__ h_all)
{
    __shared__ uint32_t hl[RN_GRID];
    const int read = blockIdx.y, sig = 1 + (int)blockIdx.z, t = threadIdx.x;
    const ReadCond* rc = rc_all + read;
    const int base = blockIdx.x * RN_TILE, n = rc->n;
    if (base >= n || !rn_wanted(rc, rr_all + read, sig)) return;
    const double* x = (sig == 1 ? flt_all : raw_all) + rc->off;
    const RnMap m = rn_map_of(rc, sig);
    for (int k = t; k < RN_GRID; k += 256) hl[k] = 0;
    __syncthreads();
    const int end = min(n, base + RN_TILE);
    for (int i = base + t; i < end; i += 256) {
        const int b = rn_bin(x[i], m.c1, m.h1, m.h2, m.c2, g.lo, g.d);
        if (b >= 0) atomicAdd(&hl[b], 1u);
    }
    __syncthreads();
    uint32_t* h = h_all + ((size_t)read * RN_SIGNALS + sig) * RN_GRID;
    for (int k = t; k < RN_GRID; k += 256) if (hl[k]) atomicAdd(&h[k], hl[k]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct RnBest { long long s; int key; };      // key: a, b + RN_B_MAX, w packed in that order -- the smaller key wins a tie

static __device__ __forceinline__ int rn_key(int a, int b, int w) { return (a << 13) | ((b + RN_B_MAX) << 4) | w; }
static __device__ __forceinline__ void rn_take(RnBest& best, long long s, int key)
{
    if (s > best.s || (s == best.s && key < best.key)) { best.s = s; best.key = key; }
}

// S(a, b, w) for every w over the occupied bins, into `best`
static __device__ __forceinline__ void rn_eval(int a, int b, int nnz, const int16_t* bin_i, const uint32_t* bin_h, const int16_t* q, long long n_a, RnBest& best)
{
    long long acc[RN_NW];
#pragma unroll
    for (int w = 0; w < RN_NW; ++w) acc[w] = 0;
    for (int j = 0; j < nnz; ++j) {
        const int i = (int)bin_i[j] - RN_HALF;
        const int hv = (int)bin_h[j];
        int idx = RN_HALF + ((a * i) >> 6) + b;                       // >> of a negative product: floor division by RN_A_ONE
        idx = (unsigned)idx < (unsigned)RN_GRID ? idx : RN_GRID;      // a bin mapped outside the grid reads the row's last cell
#pragma unroll
        for (int w = 0; w < RN_NW; ++w) acc[w] += (long long)hv * (long long)q[w * RN_Q_STRIDE + idx];
    }
#pragma unroll
    for (int w = 0; w < RN_NW; ++w) rn_take(best, acc[w] + n_a, rn_key(a, b, w));
}

// the best of the workgroup, in every thread
static __device__ __forceinline__ RnBest rn_reduce(RnBest best, RnBest* wave_best)
{
    for (int m = 32; m > 0; m >>= 1) {
        const long long s = __shfl_xor(best.s, m, 64);
        const int key = __shfl_xor(best.key, m, 64);
        rn_take(best, s, key);
    }
    __syncthreads();                                                 // (the previous round's wave_best has been read)
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
    __syncthreads();
    RnBest r = wave_best[0];
    for (int k = 1; k < 4; ++k) rn_take(r, wave_best[k].s, wave_best[k].key);
    return r;
}

__global__ void __launch_bounds__(256)
renorm_fit_kernel(const uint32_t* __restrict__ h_all, const RenormRead* __restrict__ rr_all, strq_renorm* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) int16_t q[RN_NW * RN_Q_STRIDE];
    __shared__ int32_t a_tab[RN_A_MAX + 1];
    __shared__ int16_t bin_i[RN_GRID];
    __shared__ uint32_t bin_h[RN_GRID];
    __shared__ int n_nz;
    __shared__ unsigned long long n_tot;
    __shared__ RnBest wave_best[4];
    const int read = blockIdx.x, sig = blockIdx.y, t = threadIdx.x;
    const RenormTable* tab = rr_all[read].table;
    if (!tab || (sig == 2 && !rr_all[read].raw)) return;             // (the record stays zero: not fitted)
    if (t == 0) { n_nz = 0; n_tot = 0; }
    __syncthreads();
    const uint32_t* h = h_all + ((size_t)read * RN_SIGNALS + sig) * RN_GRID;
    unsigned long long mine = 0;
    for (int k = t; k < RN_GRID; k += 256) {
        const uint32_t hv = h[k];
        if (!hv) continue;
        const int pos = atomicAdd(&n_nz, 1);
        bin_i[pos] = (int16_t)k; bin_h[pos] = hv;
        mine += hv;
    }
    if (mine) atomicAdd(&n_tot, mine);
    __syncthreads();
    const long long N = (long long)n_tot;
    const int nnz = n_nz;
    if (N == 0) return;                                              // an empty histogram is not fitted (and copies no table)
    {
        const int32_t* src = reinterpret_cast<const int32_t*>(tab->q);
        int32_t* dst = reinterpret_cast<int32_t*>(q);
        for (int k = t; k < RN_NW * RN_Q_STRIDE / 2; k += 256) dst[k] = src[k];
        for (int k = t; k <= RN_A_MAX; k += 256) a_tab[k] = tab->a[k];
    }
    __syncthreads();
    constexpr int NA = (RN_A_MAX - RN_A_MIN) / RN_COARSE_A + 1, NB = 2 * RN_B_MAX / RN_COARSE_B + 1;
    RnBest best = {INT64_MIN, 0x7fffffff};
    for (int c = t; c < NA * NB; c += 256) {
        const int a = RN_A_MIN + RN_COARSE_A * (c / NB), b = -RN_B_MAX + RN_COARSE_B * (c % NB);
        rn_eval(a, b, nnz, bin_i, bin_h, q, N * (long long)a_tab[a], best);
    }
    best = rn_reduce(best, wave_best);
    const int a0 = best.key >> 13, b0 = ((best.key >> 4) & 511) - RN_B_MAX;
    const int a_lo = max(RN_A_MIN, a0 - RN_FINE_A), a_hi = min(RN_A_MAX, a0 + RN_FINE_A);
    const int b_lo = max(-RN_B_MAX, b0 - RN_FINE_B), b_hi = min(RN_B_MAX, b0 + RN_FINE_B);
    const int nb = b_hi - b_lo + 1, nf = (a_hi - a_lo + 1) * nb;
    best.s = INT64_MIN; best.key = 0x7fffffff;
    if (t < nf) {
        const int a = a_lo + t / nb, b = b_lo + t % nb;
        rn_eval(a, b, nnz, bin_i, bin_h, q, N * (long long)a_tab[a], best);
    }
    best = rn_reduce(best, wave_best);
    if (t == 0) {
        strq_renorm_fit f;
        f.a = best.key >> 13; f.b = ((best.key >> 4) & 511) - RN_B_MAX; f.w = best.key & 15; f.fitted = 1; f.score = best.s;
        out[read].fit[sig] = f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
renorm_fold_kernel(ReadCond* __restrict__ rc_all, RenormGrid g, double min_share, PoreStats ps, float* __restrict__ level_val_all,
                   strq_renorm* __restrict__ out)
{
    const int read = blockIdx.x, t = threadIdx.x;
    const strq_renorm rec = out[read];
    const strq_renorm_fit ff = rec.fit[1];
    const bool applied = ff.fitted && ff.w >= 0 && ff.w < RN_NW && !(g.w[ff.w] < min_share);
    if (!applied) return;                                            // the read keeps all its maps (applied stays 0)
    ReadCond* rc = rc_all + read;                                    // (the fields are loaded one by one: no copy of the row)
    const double h2 = rc->h2, c2 = rc->c2;
    double c1[RN_SIGNALS] = {rc->m_c1, rc->f_c1, rc->r_c1}, h1[RN_SIGNALS] = {rc->m_h1, rc->f_h1, rc->r_h1};
#pragma unroll
    for (int s = 0; s < RN_SIGNALS; ++s) {
        const strq_renorm_fit f = rec.fit[s];
        if (!f.fitted) continue;
        const double alpha = (double)f.a / (double)RN_A_ONE;
        const double h1n = h1[s] / alpha;
        double v = alpha * (c2 - g.p);
        v = v + g.p;
        v = v + (double)f.b * g.d;
        v = v - c2;
        v = v * h1n;
        v = v / h2;
        c1[s] = c1[s] - v; h1[s] = h1n;
    }
    if (rec.fit[0].fitted) {
        // as hist_stats_kernel writes them (cond_kernels.hip)
        double v = ((double)t - c1[0]) / h1[0];
        v = v * h2 + c2;
        v = v < ps.clip_lo ? ps.clip_lo : v;
        v = v > ps.clip_hi ? ps.clip_hi : v;
        level_val_all[(size_t)read * 256 + t] = (float)v;
    }
    __syncthreads();                                                 // every wave has loaded the row and the record (the gate above is uniform)
    if (t == 0) {
        rc->m_c1 = c1[0]; rc->m_h1 = h1[0]; rc->f_c1 = c1[1]; rc->f_h1 = h1[1]; rc->r_c1 = c1[2]; rc->r_h1 = h1[2];
        out[read].applied = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
int launch_renorm_hist_i16(hipStream_t s, const uint32_t* hist16, const uint32_t* hist_raw, const uint32_t* hist8, const ReadCond* rc,
                           const RenormRead* rr, int n_reads, RenormGrid g, uint32_t* h)
{
    if (n_reads <= 0) return 0;
    hipLaunchKernelGGL(renorm_rebin_kernel, dim3(n_reads), dim3(256), 0, s, hist8, 256, 0, 0, rc, rr, g, h);
    hipLaunchKernelGGL(renorm_rebin_kernel, dim3(n_reads), dim3(256), 0, s, hist16, 65536, -32768, 1, rc, rr, g, h);
    if (hist_raw) hipLaunchKernelGGL(renorm_rebin_kernel, dim3(n_reads), dim3(256), 0, s, hist_raw, 65536, -32768, 2, rc, rr, g, h);
    return hipGetLastError() != hipSuccess;
}

int launch_renorm_hist_f64(hipStream_t s, const double* flt, const double* raw, const uint32_t* hist8, const ReadCond* rc,
                           const RenormRead* rr, int n_reads, int max_n, RenormGrid g, uint32_t* h)
{
    if (n_reads <= 0) return 0;
    hipLaunchKernelGGL(renorm_rebin_kernel, dim3(n_reads), dim3(256), 0, s, hist8, 256, 0, 0, rc, rr, g, h);
    if (max_n > 0)
        hipLaunchKernelGGL(renorm_stream_f64_kernel, dim3((max_n + RN_TILE - 1) / RN_TILE, n_reads, raw ? 2 : 1), dim3(256), 0, s, flt, raw, rc, rr, g, h);
    return hipGetLastError() != hipSuccess;
}

int launch_renorm_fit(hipStream_t s, const uint32_t* h, const RenormRead* rr, int n_reads, strq_renorm* out)
{
    if (n_reads <= 0) return 0;
    hipLaunchKernelGGL(renorm_fit_kernel, dim3(n_reads, RN_SIGNALS), dim3(256), 0, s, h, rr, out);
    return hipGetLastError() != hipSuccess;
}

int launch_renorm_fold(hipStream_t s, ReadCond* rc, int n_reads, RenormGrid g, double min_share, PoreStats ps, float* level_val, strq_renorm* out)
{
    if (n_reads <= 0) return 0;
    hipLaunchKernelGGL(renorm_fold_kernel, dim3(n_reads), dim3(256), 0, s, rc, g, min_share, ps, level_val, out);
    return hipGetLastError() != hipSuccess;
}

}  // namespace strq
