// Per-unit scores of the modification pass (mod_llr_kernels.h; reference scripts/STRique.py:492-500 reports the argmax only).
//   llr_hop_kernel / llr_scan_kernel -- the unit bounds w_j, from the hub records (one hop per unit, the chain mod_hub_pattern_kernel
//                                       walks) or from the traced state path (the route of mod_pattern_kernel);
//   mod_llr_kernel                   -- both masked Viterbi recurrences of a unit side by side in one wave, one lane per emitting
//                                       state (two per lane above 64 states, two units per wave up to 32), values in LDS.
// A unit is ~50 observations on ~26 states: the recurrences are latency chains of LDS reads, so the kernel wants many waves per
// SIMD (2 to 4 KB of LDS per wave, no workgroup barrier) and nothing else; units are independent and about equally long, so a plain
// grid-stride loop over (read, unit) keeps every wave busy -- no queue.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "mod_llr_kernels.h"
#include "hmm_wave.h"

namespace strq {

// One thread per read: the chain of hub records, last unit first (record t = the e0 emission at observation t - 1).
__global__ void __launch_bounds__(64) llr_hop_kernel(const LlrBoundTask* __restrict__ tasks, int n_tasks)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_tasks) return;
    const LlrBoundTask tk = tasks[i];
    const VitResult* r = static_cast<const VitResult*>(tk.result);
    if (r->status != 0) { if (tk.n != 0) *tk.bad = 1; return; }
    uint32_t p = r->dbg[0];
    int64_t j = tk.n;
    while (p != 0 && j > 0) {
        if ((int64_t)p > tk.T) break;
        tk.w[--j] = (int32_t)(p - 1);
        p = (uint32_t)tk.rec[p];
    }
    if (p != 0 || j != 0) *tk.bad = 1;
}

// One wave per read: a hub emission behind a non-hub one closes a unit; 64 observations per round, compacted with a ballot.
__global__ void __launch_bounds__(256) llr_scan_kernel(const LlrBoundTask* __restrict__ tasks, int n_tasks)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_tasks) return;
    const LlrBoundTask tk = tasks[i];
    const VitResult* r = static_cast<const VitResult*>(tk.result);
    if (r->status != 0) { if (lane == 0 && tk.n != 0) *tk.bad = 1; return; }
    int64_t k = 0;
    uint64_t carry = 1;                 // "the previous observation was a hub's" for the first one
    for (int64_t t0 = 0; t0 < tk.T; t0 += 64) {
        const int64_t t = t0 + lane;
        const bool hubt = t >= tk.T || tk.tag[tk.path[t]] == 2;
        const uint64_t hubs = __builtin_amdgcn_ballot_w64(hubt);
        const uint64_t prev = (hubs << 1) | carry;
        const bool hit = t < tk.T && hubt && !((prev >> lane) & 1);
        const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
        const int64_t at = k + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (hit && at < tk.n) tk.w[at] = (int32_t)t;
        k += __builtin_popcountll(m);
        carry = hubs >> 63;
    }
    if (lane == 0 && k != tk.n) *tk.bad = 1;
}

// S: states per lane; HALF: two units per wave, 32 lanes each.
template <int S, bool HALF>
__global__ void __launch_bounds__(256)
mod_llr_kernel(const LlrRead* __restrict__ reads, const int64_t* __restrict__ first, int n_reads, int64_t n_units)
{
    constexpr int W = HALF ? 32 : 64, NS = HALF ? 32 : 64 * S, NC = 2 * NS + 1, UPW = HALF ? 2 : 1;
    // per unit two buffers of NC cells: [0, NS) the states' own values, [NS, 2 NS) the hubs' mod copies, 2 NS = -inf for padding edges
    __shared__ double lds[4 * UPW * 2 * NC];
    const double NEGINF = -INFINITY;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & (W - 1), half = HALF ? lane >> 5 : 0;
    double* const cell = lds + (size_t)(wave * UPW + half) * 2 * NC;
    auto cell_of = [](int code) { return code < 128 ? code : (code < LLR_PAD ? NS + (code - 128) : 2 * NS); };
    const int64_t n_slots = (n_units + UPW - 1) / UPW;

    const LlrModel* cur = nullptr;
    int off[S][LLR_DEG], off2[S][LLR_DEG2], kind[S], hub[S];
    double lp[S][LLR_DEG], lp2[S][LLR_DEG2], slp[2][S], ea[S], eb[S], ec[S];
    int deg = 0, deg2 = 0;

    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < n_slots; g += (int64_t)gridDim.x * 4) {
        const int64_t uid = g * UPW + half;
        const bool valid = uid < n_units;
        int r = 0;
        if (valid) {          // the last read with first[r] <= uid
            int lo = 0, hi = n_reads - 1;
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= uid) lo = mid; else hi = mid - 1; }
            r = lo;
        }
        const LlrRead rd = reads[r];
        int64_t u = 0, j = 0; int len = 0;
        if (valid) {
            j = uid - first[r];
            u = j ? (int64_t)rd.w[j - 1] + 1 : 0;
            const int64_t wj = rd.w[j];
            if (u >= 0 && wj >= u && wj < rd.T && wj - u < ((int64_t)1 << 30)) len = (int)(wj - u + 1);      // anything else scores -inf, -inf
        }
        const LlrModel* m = rd.model;
        if (__builtin_amdgcn_ballot_w64(m != cur) != 0) {
#pragma unroll
            for (int s = 0; s < S; ++s) {
#pragma unroll
                for (int k = 0; k < LLR_DEG; ++k) { off[s][k] = cell_of(m->src[(s * LLR_DEG + k) * 64 + li]); lp[s][k] = m->lp[(s * LLR_DEG + k) * 64 + li]; }
#pragma unroll
                for (int k = 0; k < LLR_DEG2; ++k) { off2[s][k] = cell_of(m->src2[(s * LLR_DEG2 + k) * 64 + li]); lp2[s][k] = m->lp2[(s * LLR_DEG2 + k) * 64 + li]; }
                slp[0][s] = m->start_lp[s * 64 + li]; slp[1][s] = m->start_lp[(2 + s) * 64 + li];
                kind[s] = m->kind[s * 64 + li]; hub[s] = m->hub[s * 64 + li];
                ea[s] = m->ea[s * 64 + li]; eb[s] = m->eb[s * 64 + li]; ec[s] = m->ec[s * 64 + li];
            }
            // rows beyond a model's own degree are padding: the larger degree of the two halves serves both
            int d1 = m->deg, d2 = m->deg2;
            if (HALF) { d1 = max(__shfl(d1, 0), __shfl(d1, 32)); d2 = max(__shfl(d2, 0), __shfl(d2, 32)); }
            deg = __builtin_amdgcn_readfirstlane(d1); deg2 = __builtin_amdgcn_readfirstlane(d2);
            cur = m;
        }
        for (int i = li; i < 2 * NC; i += W) cell[i] = NEGINF;
        wave_fence();
        int maxlen = len;
        if (HALF) maxlen = max(__shfl(len, 0), __shfl(len, 32));
        maxlen = __builtin_amdgcn_readfirstlane(maxlen);
        for (int t0 = 0; t0 < maxlen; t0 += W) {
            double xv = 0.0;
            if (t0 + li < len) xv = rd.x[u + t0 + li];
            const int send = maxlen - t0 < W ? maxlen - t0 : W;
            for (int i = 0; i < send; ++i) {
                const int t = t0 + i;
                const double x = __shfl(xv, i, W);
                const double* const src = cell + (t & 1) * NC;
                double* const dst = cell + ((t + 1) & 1) * NC;
                const double vstart = t == 0 ? 0.0 : NEGINF;          // the start state holds 0 in front of the first observation only
                double nva[S], nvb[S];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    double ba = NEGINF, bb = NEGINF;
#pragma unroll
                    for (int k = 0; k < LLR_DEG; ++k)
                        if (k < deg) { const double c = src[off[s][k]] + lp[s][k]; ba = c > ba ? c : ba; }
#pragma unroll
                    for (int k = 0; k < LLR_DEG2; ++k)
                        if (k < deg2) { const double c = src[off2[s][k]] + lp2[s][k]; bb = c > bb ? c : bb; }
                    { const double c = vstart + slp[0][s]; ba = c > ba ? c : ba; }
                    { const double c = vstart + slp[1][s]; bb = c > bb ? c : bb; }
                    const double d = x - ea[s];
                    const double en = ec[s] - (d * d) * eb[s];
                    const double eu = (x >= ea[s] && x <= eb[s]) ? ec[s] : NEGINF;
                    double em = kind[s] == 1 ? en : eu;
                    if (x != x) em = 0.0;          // a missing observation has log-probability 0 under every distribution
                    nva[s] = ba + em; nvb[s] = bb + em;
                }
                if (t < len) {
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        if (kind[s]) dst[s * 64 + li] = nva[s];
                        if (hub[s]) dst[NS + s * 64 + li] = nvb[s];
                    }
                }
                wave_fence();
            }
        }
        if (valid && li == 0) {
            const double* const fin = cell + (len & 1) * NC;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                double best = NEGINF;
                for (int e = 0; e < m->end_deg[c] && e < LLR_END_DEG; ++e) {
                    const double v = fin[cell_of(m->end_src[c * LLR_END_DEG + e])] + m->end_lp[c * LLR_END_DEG + e];
                    best = v > best ? v : best;
                }
                rd.out[2 * j + c] = len > 0 ? best : NEGINF;
            }
        }
        wave_fence();
    }
}

int launch_llr_bounds(hipStream_t s, const LlrBoundTask* hop, int n_hop, const LlrBoundTask* scan, int n_scan)
{
    if (n_hop > 0) hipLaunchKernelGGL(llr_hop_kernel, dim3((n_hop + 63) / 64), dim3(64), 0, s, hop, n_hop);
    if (n_scan > 0) hipLaunchKernelGGL(llr_scan_kernel, dim3((n_scan + 3) / 4), dim3(256), 0, s, scan, n_scan);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_llr_score(hipStream_t s, int mode, const LlrRead* reads, const int64_t* first, int n_reads, int64_t n_units, int n_cu)
{
    if (n_reads <= 0 || n_units <= 0) return 0;
    const int64_t slots = mode == 0 ? (n_units + 1) / 2 : n_units;
    // eight workgroups of four waves per CU: eight waves per SIMD where the registers allow it, the rest of the units by stride
    const int64_t want = (slots + 3) / 4, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * 8;
    const dim3 grid((unsigned)(want < cap ? want : cap));
    if (mode == 0) hipLaunchKernelGGL((mod_llr_kernel<1, true>), grid, dim3(256), 0, s, reads, first, n_reads, n_units);
    else if (mode == 1) hipLaunchKernelGGL((mod_llr_kernel<1, false>), grid, dim3(256), 0, s, reads, first, n_reads, n_units);
    else if (mode == 2) hipLaunchKernelGGL((mod_llr_kernel<2, false>), grid, dim3(256), 0, s, reads, first, n_reads, n_units);
    else return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host: the edge image
namespace {
struct ImageLayout {
    size_t src, lp, src2, lp2, start_lp, kind, ea, eb, ec, hub, end_src, end_lp, total;
    ImageLayout()
    {
        size_t o = (sizeof(LlrModel) + 15) & ~(size_t)15;
        auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
        src = take(2 * LLR_DEG * 64 * 4); lp = take(2 * LLR_DEG * 64 * 8);
        src2 = take(2 * LLR_DEG2 * 64 * 4); lp2 = take(2 * LLR_DEG2 * 64 * 8);
        start_lp = take(4 * 64 * 8); kind = take(2 * 64 * 4);
        ea = take(2 * 64 * 8); eb = take(2 * 64 * 8); ec = take(2 * 64 * 8); hub = take(2 * 64 * 4);
        end_src = take(2 * LLR_END_DEG * 4); end_lp = take(2 * LLR_END_DEG * 8);
        total = o;
    }
};
}  // namespace

size_t llr_image_bytes() { return ImageLayout().total; }

int llr_build_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end, const int32_t* in_ptr, const int32_t* in_src,
                    const double* in_logp, const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                    const int32_t* state_tag, const void* dev_base, std::vector<char>& blob, int32_t* mode, std::string& why)
{
    const int ne = silent_start;
    if (!state_tag) { why = "mod-llr: the modification model carries no state tags"; return 1; }
    if (ne > LLR_MAX_EMIT) {
        why = "mod-llr: dual models of at most " + std::to_string(LLR_MAX_EMIT) + " emitting states are supported (repeat units of up to 31 nt at k = 6); this one has " + std::to_string(ne);
        return 1;
    }
    if (ne < 1 || n_states != ne + 2 || start < ne || end < ne || start == end || in_ptr[start + 1] != in_ptr[start]) {
        why = "mod-llr: the modification model has silent states besides start and end"; return 1;
    }
    const ImageLayout L;
    blob.assign(L.total, 0);
    int32_t* src = reinterpret_cast<int32_t*>(&blob[L.src]); double* lp = reinterpret_cast<double*>(&blob[L.lp]);
    int32_t* src2 = reinterpret_cast<int32_t*>(&blob[L.src2]); double* lp2 = reinterpret_cast<double*>(&blob[L.lp2]);
    double* slp = reinterpret_cast<double*>(&blob[L.start_lp]);
    int32_t* kind = reinterpret_cast<int32_t*>(&blob[L.kind]); int32_t* hub = reinterpret_cast<int32_t*>(&blob[L.hub]);
    double* ea = reinterpret_cast<double*>(&blob[L.ea]); double* eb = reinterpret_cast<double*>(&blob[L.eb]); double* ec = reinterpret_cast<double*>(&blob[L.ec]);
    int32_t* esrc = reinterpret_cast<int32_t*>(&blob[L.end_src]); double* elp = reinterpret_cast<double*>(&blob[L.end_lp]);
    for (int i = 0; i < 2 * LLR_DEG * 64; ++i) { src[i] = LLR_PAD; lp[i] = -INFINITY; }
    for (int i = 0; i < 2 * LLR_DEG2 * 64; ++i) { src2[i] = LLR_PAD; lp2[i] = -INFINITY; }
    for (int i = 0; i < 4 * 64; ++i) slp[i] = -INFINITY;
    for (int i = 0; i < 2 * LLR_END_DEG; ++i) { esrc[i] = LLR_PAD; elp[i] = -INFINITY; }
    LlrModel M; std::memset(&M, 0, sizeof(M));
    M.n_emit = ne; M.mode = ne <= 32 ? 0 : (ne <= 64 ? 1 : 2);
    for (int l = 0; l < ne; ++l) {
        const int tl = state_tag[l];
        if (tl < 0 || tl > 2) { why = "mod-llr: state tags of the modification model must be 0 (base), 1 (modified) or 2 (hub)"; return 1; }
        const int slot = l >> 6, lane = l & 63;
        kind[slot * 64 + lane] = emis_kind[l]; hub[slot * 64 + lane] = tl == 2;
        if (emis_kind[l] != 1 && emis_kind[l] != 2) { why = "mod-llr: unknown emission kind"; return 1; }
        ea[slot * 64 + lane] = emis_a[l]; eb[slot * 64 + lane] = emis_b[l]; ec[slot * 64 + lane] = emis_c[l];
        int n1 = 0, n2 = 0;
        for (int e = in_ptr[l]; e < in_ptr[l + 1]; ++e) {
            const int k = in_src[e];
            if (k == start) {          // into both copies of a hub, into the one value of a branch state
                slp[slot * 64 + lane] = in_logp[e];
                if (tl == 2) slp[(2 + slot) * 64 + lane] = in_logp[e];
                continue;
            }
            if (k >= ne) { why = "mod-llr: the modification model has silent states besides start and end"; return 1; }
            const int tk = state_tag[k];
            // own value: the base copy of a hub, the branch of a branch state; an edge from the other branch is masked
            const int b1 = tl == 2 ? 0 : tl;
            if (tk == 2 || tk == b1) {
                if (n1 >= LLR_DEG) { why = "mod-llr: a state of the modification model has more than " + std::to_string(LLR_DEG) + " in-edges"; return 1; }
                src[(slot * LLR_DEG + n1) * 64 + lane] = (tk == 2 && b1 == 1) ? 128 + k : k;
                lp[(slot * LLR_DEG + n1) * 64 + lane] = in_logp[e]; ++n1;
            }
            if (tl == 2 && (tk == 2 || tk == 1)) {          // the mod copy of a hub
                if (n2 >= LLR_DEG2) { why = "mod-llr: a hub state of the modification model has more than " + std::to_string(LLR_DEG2) + " in-edges inside one branch"; return 1; }
                src2[(slot * LLR_DEG2 + n2) * 64 + lane] = tk == 2 ? 128 + k : k;
                lp2[(slot * LLR_DEG2 + n2) * 64 + lane] = in_logp[e]; ++n2;
            }
        }
        M.deg = std::max(M.deg, n1); M.deg2 = std::max(M.deg2, n2);
    }
    for (int e = in_ptr[end]; e < in_ptr[end + 1]; ++e) {
        const int k = in_src[e];
        if (k >= ne) { why = "mod-llr: the modification model has silent states besides start and end"; return 1; }
        const int tk = state_tag[k];
        for (int c = 0; c < 2; ++c) {
            if (tk != 2 && tk != c) continue;
            if (M.end_deg[c] >= LLR_END_DEG) { why = "mod-llr: the end state of the modification model has more than " + std::to_string(LLR_END_DEG) + " in-edges"; return 1; }
            esrc[c * LLR_END_DEG + M.end_deg[c]] = (tk == 2 && c == 1) ? 128 + k : k;
            elp[c * LLR_END_DEG + M.end_deg[c]] = in_logp[e]; ++M.end_deg[c];
        }
    }
    const char* base = static_cast<const char*>(dev_base);
    M.src = reinterpret_cast<const int32_t*>(base + L.src); M.lp = reinterpret_cast<const double*>(base + L.lp);
    M.src2 = reinterpret_cast<const int32_t*>(base + L.src2); M.lp2 = reinterpret_cast<const double*>(base + L.lp2);
    M.start_lp = reinterpret_cast<const double*>(base + L.start_lp); M.kind = reinterpret_cast<const int32_t*>(base + L.kind);
    M.ea = reinterpret_cast<const double*>(base + L.ea); M.eb = reinterpret_cast<const double*>(base + L.eb); M.ec = reinterpret_cast<const double*>(base + L.ec);
    M.hub = reinterpret_cast<const int32_t*>(base + L.hub);
    M.end_src = reinterpret_cast<const int32_t*>(base + L.end_src); M.end_lp = reinterpret_cast<const double*>(base + L.end_lp);
    std::memcpy(&blob[0], &M, sizeof(M));
    *mode = M.mode;
    return 0;
}

}  // namespace strq
