// The motif track (motif_kernels.h; the rule: strique_amd/motifs.py).
//   motif_track_kernel  -- one wave per (window, run of consecutive segments), one lane per emitting state of a loop model: the
//                          Viterbi recurrence of every segment under every candidate, values in an LDS row, the segment's maximum
//                          over the lanes at its end.
//   motif_reduce_kernel -- one wave per window: winner of every segment, observations won per candidate, majority -- integers only.
// A segment is a few hundred observations on 8 to 64 states: a latency chain of LDS reads, as the per-unit scores (mod_llr_kernels.hip),
// so the kernel wants many waves per SIMD (1 KB of LDS per wave, no workgroup barrier) and a plain grid-stride loop over the tasks --
// segments are independent and about equally long, no queue and no atomics.  The candidates of a segment run one after another; each
// reads the observations once more, 64 at a time through vit_observation (they stay in the L2), which keeps one candidate's edge
// rows in registers for a whole segment.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "motif_kernels.h"
#include "hmm_wave.h"

namespace strq {

#define MOTIF_ROW 65           // cells of a value row: 64 states and the -inf cell of the padding edges

__global__ void __launch_bounds__(256)
motif_track_kernel(const MotifWindow* __restrict__ windows, const MotifTask* __restrict__ tasks, int64_t n_tasks)
{
    __shared__ double lds[4 * 2 * MOTIF_ROW];
    const double NEGINF = -INFINITY;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* const cell = lds + (size_t)wave * 2 * MOTIF_ROW;

    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < n_tasks; g += (int64_t)gridDim.x * 4) {
        const MotifTask tk = tasks[g];
        const MotifWindow* const W = windows + tk.window;
        const VitTask obs = W->obs;
        const int K = W->n_cand, S = W->segment;
        const int64_t n_seg = W->n_seg;
        for (int64_t seg = tk.seg_first; seg < tk.seg_first + tk.seg_count; ++seg) {
            const int64_t begin = seg * S;
            const int len = (int)((seg == n_seg - 1 ? obs.T : begin + S) - begin);          // S .. 2 S - 1, or T of a stretch below S
            for (int j = 0; j < K; ++j) {
                const MotifModel* const m = W->model[j];
                int off[MOTIF_DEG]; double lp[MOTIF_DEG];
#pragma unroll
                for (int k = 0; k < MOTIF_DEG; ++k) { off[k] = m->src[k * 64 + lane]; lp[k] = m->lp[k * 64 + lane]; }
                const double slp = m->start_lp[lane], ea = m->ea[lane], eb = m->eb[lane], ec = m->ec[lane];
                const int kind = m->kind[lane];
                const int deg = __builtin_amdgcn_readfirstlane(m->deg);
                for (int i = lane; i < 2 * MOTIF_ROW; i += 64) cell[i] = NEGINF;
                wave_fence();
                double last = NEGINF;
                for (int t0 = 0; t0 < len; t0 += 64) {
                    double xv = 0.0;
                    if (t0 + lane < len) xv = vit_observation(obs, begin + t0 + lane);
                    const int send = len - t0 < 64 ? len - t0 : 64;
                    for (int i = 0; i < send; ++i) {
                        const int t = t0 + i;
                        const double x = readlane_f64(xv, i);
                        const double* const src = cell + (t & 1) * MOTIF_ROW;
                        double* const dst = cell + ((t + 1) & 1) * MOTIF_ROW;
                        const double vstart = t == 0 ? 0.0 : NEGINF;          // the start state holds 0 in front of the first observation only
                        double best = NEGINF;
#pragma unroll
                        for (int k = 0; k < MOTIF_DEG; ++k)
                            if (k < deg) { const double c = src[off[k]] + lp[k]; best = c > best ? c : best; }
                        { const double c = vstart + slp; best = c > best ? c : best; }
                        last = best + hmm_log_emission(x, kind, ea, eb, ec);
                        if (kind) dst[lane] = last;
                        wave_fence();
                    }
                }
                // the end state: every emitting state reaches it with log-probability 0
                double v = kind ? last : NEGINF;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
                if (lane == 0) W->V[seg * K + j] = v;
            }
        }
    }
}

__global__ void __launch_bounds__(256) motif_reduce_kernel(const MotifWindow* __restrict__ windows, int n_windows)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_windows) return;
    const MotifWindow* const W = windows + w;
    const int K = W->n_cand;
    const int64_t n_seg = W->n_seg, S = W->segment;
    const int64_t last_len = W->obs.T - (n_seg - 1) * S;
    int64_t full[MOTIF_MAX_CAND] = {0, 0, 0, 0};          // whole segments in front of the last one a candidate won
    int last_win = 0;
    for (int64_t s0 = 0; s0 < n_seg; s0 += 64) {
        const int64_t seg = s0 + lane;
        const bool valid = seg < n_seg;
        int win = 0;
        if (valid) {
            double best = W->V[seg * K];
            for (int j = 1; j < K; ++j) { const double v = W->V[seg * K + j]; if (v > best) { best = v; win = j; } }          // a tie goes to the lowest index
            W->winner[seg] = win;
        }
        const bool is_last = valid && seg == n_seg - 1;
#pragma unroll
        for (int j = 0; j < MOTIF_MAX_CAND; ++j) {
            full[j] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(valid && !is_last && win == j));
            if (__builtin_amdgcn_ballot_w64(is_last && win == j) != 0) last_win = j;
        }
    }
    if (lane == 0) {
        int64_t most = -1; int maj = 0;
        for (int j = 0; j < MOTIF_MAX_CAND; ++j) {
            const int64_t won = j < K ? full[j] * S + (j == last_win ? last_len : 0) : 0;
            W->obs_won[j] = won;
            if (j < K && won > most) { most = won; maj = j; }
        }
        *W->majority = maj;
    }
}

int launch_motif_track(hipStream_t s, const MotifWindow* windows, int n_windows, const MotifTask* tasks, int64_t n_tasks, int n_cu)
{
    if (n_windows <= 0 || n_tasks <= 0) return 0;
    // eight workgroups of four waves per CU, the rest of the tasks by stride
    const int64_t want = (n_tasks + 3) / 4, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * 8;
    hipLaunchKernelGGL(motif_track_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, s, windows, tasks, n_tasks);
    hipLaunchKernelGGL(motif_reduce_kernel, dim3((unsigned)((n_windows + 3) / 4)), dim3(256), 0, s, windows, n_windows);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host: the edge image
namespace {
struct ImageLayout {
    size_t src, lp, start_lp, kind, ea, eb, ec, total;
    ImageLayout()
    {
        size_t o = (sizeof(MotifModel) + 15) & ~(size_t)15;
        auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
        src = take(MOTIF_DEG * 64 * 4); lp = take(MOTIF_DEG * 64 * 8);
        start_lp = take(64 * 8); kind = take(64 * 4); ea = take(64 * 8); eb = take(64 * 8); ec = take(64 * 8);
        total = o;
    }
};
}  // namespace

size_t motif_image_bytes() { return ImageLayout().total; }

int motif_build_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end, const int32_t* in_ptr, const int32_t* in_src,
                      const double* in_logp, const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                      const void* dev_base, std::vector<char>& blob, std::string& why)
{
    const int ne = silent_start;
    if (ne > MOTIF_MAX_EMIT) {
        why = "motifs: loop models of at most " + std::to_string(MOTIF_MAX_EMIT) + " emitting states are supported (units of up to 31 nt at k = 6); this one has " + std::to_string(ne);
        return 1;
    }
    if (ne < 1 || n_states != ne + 2 || start < ne || end < ne || start == end || in_ptr[start + 1] != in_ptr[start]) {
        why = "motifs: a loop model has no silent states besides start and end"; return 1;
    }
    // the end state: one edge from every emitting state, log-probability 0 -- what makes its value the maximum over the states
    std::vector<char> leaves((size_t)ne, 0);
    for (int e = in_ptr[end]; e < in_ptr[end + 1]; ++e) {
        const int k = in_src[e];
        if (k < 0 || k >= ne || in_logp[e] != 0.0 || leaves[(size_t)k]) { why = "motifs: every emitting state of a loop model reaches the end state once, with log-probability 0"; return 1; }
        leaves[(size_t)k] = 1;
    }
    if (in_ptr[end + 1] - in_ptr[end] != ne) { why = "motifs: every emitting state of a loop model reaches the end state once, with log-probability 0"; return 1; }
    const ImageLayout L;
    blob.assign(L.total, 0);
    int32_t* src = reinterpret_cast<int32_t*>(&blob[L.src]); double* lp = reinterpret_cast<double*>(&blob[L.lp]);
    double* slp = reinterpret_cast<double*>(&blob[L.start_lp]); int32_t* kind = reinterpret_cast<int32_t*>(&blob[L.kind]);
    double* ea = reinterpret_cast<double*>(&blob[L.ea]); double* eb = reinterpret_cast<double*>(&blob[L.eb]); double* ec = reinterpret_cast<double*>(&blob[L.ec]);
    for (int i = 0; i < MOTIF_DEG * 64; ++i) { src[i] = MOTIF_PAD; lp[i] = -INFINITY; }
    for (int i = 0; i < 64; ++i) slp[i] = -INFINITY;
    MotifModel M; std::memset(&M, 0, sizeof(M));
    M.n_emit = ne;
    for (int l = 0; l < ne; ++l) {
        if (emis_kind[l] != 1 && emis_kind[l] != 2) { why = "motifs: unknown emission kind"; return 1; }
        kind[l] = emis_kind[l]; ea[l] = emis_a[l]; eb[l] = emis_b[l]; ec[l] = emis_c[l];
        int n = 0;
        for (int e = in_ptr[l]; e < in_ptr[l + 1]; ++e) {
            const int k = in_src[e];
            if (k == start) { slp[l] = in_logp[e]; continue; }
            if (k < 0 || k >= ne) { why = "motifs: a loop model has no silent states besides start and end"; return 1; }
            if (n >= MOTIF_DEG) { why = "motifs: a state of the loop model has more than " + std::to_string(MOTIF_DEG) + " in-edges"; return 1; }
            src[n * 64 + l] = k; lp[n * 64 + l] = in_logp[e]; ++n;
        }
        M.deg = std::max(M.deg, n);
    }
    const char* base = static_cast<const char*>(dev_base);
    M.src = reinterpret_cast<const int32_t*>(base + L.src); M.lp = reinterpret_cast<const double*>(base + L.lp);
    M.start_lp = reinterpret_cast<const double*>(base + L.start_lp); M.kind = reinterpret_cast<const int32_t*>(base + L.kind);
    M.ea = reinterpret_cast<const double*>(base + L.ea); M.eb = reinterpret_cast<const double*>(base + L.eb); M.ec = reinterpret_cast<const double*>(base + L.ec);
    std::memcpy(&blob[0], &M, sizeof(M));
    return 0;
}

}  // namespace strq
