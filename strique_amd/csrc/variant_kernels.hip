// The variant pass behind the decode of a variant model (variant_kernels.h):
//   var_hop_kernel / var_scan_kernel -- the passages (branch_j, w_j) of a read and their number, from the hub records (one hop per
//                                       passage) or from the traced state path (STRQ_MOD_BACKPOINTERS=1, models off the HUB shapes);
//   variant_score_kernel             -- all NB masked Viterbi recurrences of a passage side by side in one wave on the same
//                                       observation: one lane per emitting state (two per lane above 64 states, two passages per wave
//                                       up to 32), a branch state carries one value, a hub state NB; values in LDS.
// Same regime as mod_llr_kernel: a passage is ~20 to ~150 observations on 26 to 86 states, the recurrences are latency chains of LDS
// reads, passages are independent -- many waves, no workgroup barrier, a plain grid-stride loop over (read, passage).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "variant_kernels.h"
#include "hmm_wave.h"

namespace strq {

// One thread per read: the chain of hub records, last passage first (record t = the e0 emission at observation t - 1; its low word the
// time of the e0 emission before it, its high word the branch of the passage in between).  The count pass (w == null) walks and
// checks it; the write pass walks it again and writes ascending -- exactly `cap` entries, the count of the first pass.
__global__ void __launch_bounds__(64) var_hop_kernel(const VarBoundTask* __restrict__ tasks, int n_tasks)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_tasks) return;
    const VarBoundTask tk = tasks[i];
    const VitResult* r = static_cast<const VitResult*>(tk.result);
    if (!tk.w) *tk.n = 0;
    if (r->status != 0) { if (tk.w && tk.cap != 0) *tk.bad = 1; return; }          // no path: no passages
    int64_t cnt = 0; bool ok = true;
    for (uint32_t p = r->dbg[0]; p != 0;) {
        if ((int64_t)p > tk.T || cnt >= tk.cap) { ok = false; break; }
        const uint64_t v = tk.rec[p];
        if ((uint32_t)v >= p || (uint32_t)(v >> 32) >= (uint32_t)tk.n_branch) { ok = false; break; }
        ++cnt; p = (uint32_t)v;
    }
    if (!ok) { *tk.bad = 1; return; }
    if (!tk.w) { *tk.n = (int32_t)cnt; return; }
    if (cnt != tk.cap) { *tk.bad = 1; return; }          // the two walks disagree
    int64_t k = cnt;
    for (uint32_t p = r->dbg[0]; p != 0 && k > 0;) {
        const uint64_t v = tk.rec[p];
        --k; tk.w[k] = (int32_t)(p - 1); tk.branch[k] = (int32_t)(uint32_t)(v >> 32);
        p = (uint32_t)v;
    }
}

// One wave per read: a hub emission behind a non-hub one closes a passage of that state's branch; 64 observations per round.  Count pass
// and write pass as above.
__global__ void __launch_bounds__(256) var_scan_kernel(const VarBoundTask* __restrict__ tasks, int n_tasks)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_tasks) return;
    const VarBoundTask tk = tasks[i];
    const VitResult* r = static_cast<const VitResult*>(tk.result);
    if (r->status != 0) { if (lane == 0) { if (!tk.w) *tk.n = 0; else if (tk.cap != 0) *tk.bad = 1; } return; }
    int64_t k = 0;
    uint64_t carry = 1;                 // "the previous observation was a hub's" for the first one
    bool wrong = false;
    for (int64_t t0 = 0; t0 < tk.T; t0 += 64) {
        const int64_t t = t0 + lane;
        const bool hubt = t >= tk.T || tk.tag[tk.path[t]] == 2;
        const uint64_t hubs = __builtin_amdgcn_ballot_w64(hubt);
        const uint64_t prev = (hubs << 1) | carry;
        const bool hit = t < tk.T && hubt && !((prev >> lane) & 1);          // (never at t = 0)
        const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
        const int64_t at = k + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (hit) {
            const int b = var_branch_of_tag(tk.tag[tk.path[t - 1]]);
            if (b < 0 || b >= tk.n_branch) wrong = true;
            else if (tk.w && at < tk.cap) { tk.w[at] = (int32_t)t; tk.branch[at] = b; }
        }
        k += __builtin_popcountll(m);
        carry = hubs >> 63;
    }
    const bool any_wrong = __builtin_amdgcn_ballot_w64(wrong) != 0;
    if (lane == 0) {
        const bool bad = any_wrong || k > tk.cap || (tk.w && k != tk.cap);          // (the count pass: cap = T / 3 + 1, what T observations can hold)
        if (!tk.w) *tk.n = bad ? 0 : (int32_t)k;
        if (bad) *tk.bad = 1;
    }
}

// S: states per lane; NB: branches; HALF: two passages per wave, 32 lanes each.
template <int S, int NB, bool HALF>
__global__ void __launch_bounds__(256)
variant_score_kernel(const VarRead* __restrict__ reads, const int64_t* __restrict__ first, int n_reads, int64_t n_pass)
{
    constexpr int W = HALF ? 32 : 64, NS = HALF ? 32 : 64 * S, NC = NB * NS + 1, UPW = HALF ? 2 : 1;
    // per passage two buffers of NC cells: [c NS, (c + 1) NS) copy c of the states' values (a branch state: copy 0), NB NS = -inf for padding edges
    __shared__ double lds[4 * UPW * 2 * NC];
    const double NEGINF = -INFINITY;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & (W - 1), half = HALF ? lane >> 5 : 0;
    double* const cell = lds + (size_t)(wave * UPW + half) * 2 * NC;
    auto cell_of = [](int code) { return code >= VAR_PAD ? NB * NS : (code >> 7) * NS + (code & 127); };
    const int64_t n_slots = (n_pass + UPW - 1) / UPW;

    const VarModel* cur = nullptr;
    int off[S][VAR_DEG], off2[NB - 1][S][VAR_DEG2], kind[S], hub[S];
    double lp[S][VAR_DEG], lp2[NB - 1][S][VAR_DEG2], slp[S], ea[S], eb[S], ec[S];
    int deg = 0, deg2 = 0;

    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < n_slots; g += (int64_t)gridDim.x * 4) {
        const int64_t uid = g * UPW + half;
        const bool valid = uid < n_pass;
        int r = 0;
        if (valid) {          // the last read with first[r] <= uid
            int lo = 0, hi = n_reads - 1;
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= uid) lo = mid; else hi = mid - 1; }
            r = lo;
        }
        const VarRead rd = reads[r];
        int64_t u = 0, j = 0; int len = 0;
        if (valid) {
            j = uid - first[r];
            u = j ? (int64_t)rd.w[j - 1] + 1 : 0;
            const int64_t wj = rd.w[j];
            if (u >= 0 && wj >= u && wj < rd.T && wj - u < ((int64_t)1 << 30)) len = (int)(wj - u + 1);      // anything else scores -inf throughout
        }
        const VarModel* m = rd.model;
        if (__builtin_amdgcn_ballot_w64(m != cur) != 0) {
#pragma unroll
            for (int s = 0; s < S; ++s) {
#pragma unroll
                for (int k = 0; k < VAR_DEG; ++k) { off[s][k] = cell_of(m->src[(s * VAR_DEG + k) * 64 + li]); lp[s][k] = m->lp[(s * VAR_DEG + k) * 64 + li]; }
#pragma unroll
                for (int c = 0; c < NB - 1; ++c)
#pragma unroll
                    for (int k = 0; k < VAR_DEG2; ++k) {
                        off2[c][s][k] = cell_of(m->src2[((c * 2 + s) * VAR_DEG2 + k) * 64 + li]);
                        lp2[c][s][k] = m->lp2[((c * 2 + s) * VAR_DEG2 + k) * 64 + li];
                    }
                slp[s] = m->start_lp[s * 64 + li];
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
                double nva[S], nvb[NB - 1][S];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    double ba = NEGINF;
#pragma unroll
                    for (int k = 0; k < VAR_DEG; ++k)
                        if (k < deg) { const double c = src[off[s][k]] + lp[s][k]; ba = c > ba ? c : ba; }
                    const double cs = vstart + slp[s];
                    ba = cs > ba ? cs : ba;
                    const double d = x - ea[s];
                    const double en = ec[s] - (d * d) * eb[s];
                    const double eu = (x >= ea[s] && x <= eb[s]) ? ec[s] : NEGINF;
                    double em = kind[s] == 1 ? en : eu;
                    if (x != x) em = 0.0;          // a missing observation has log-probability 0 under every distribution
                    nva[s] = ba + em;
#pragma unroll
                    for (int c = 0; c < NB - 1; ++c) {
                        double bb = NEGINF;
#pragma unroll
                        for (int k = 0; k < VAR_DEG2; ++k)
                            if (k < deg2) { const double v = src[off2[c][s][k]] + lp2[c][s][k]; bb = v > bb ? v : bb; }
                        bb = cs > bb ? cs : bb;
                        nvb[c][s] = bb + em;
                    }
                }
                if (t < len) {
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        if (kind[s]) dst[s * 64 + li] = nva[s];
                        if (hub[s]) {
#pragma unroll
                            for (int c = 0; c < NB - 1; ++c) dst[(c + 1) * NS + s * 64 + li] = nvb[c][s];
                        }
                    }
                }
                wave_fence();
            }
        }
        if (valid && li == 0) {
            const double* const fin = cell + (len & 1) * NC;
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                double best = NEGINF;
                for (int e = 0; e < m->end_deg[c] && e < VAR_END_DEG; ++e) {
                    const double v = fin[cell_of(m->end_src[c * VAR_END_DEG + e])] + m->end_lp[c * VAR_END_DEG + e];
                    best = v > best ? v : best;
                }
                rd.out[NB * j + c] = len > 0 ? best : NEGINF;
            }
        }
        wave_fence();
    }
}

int launch_var_bounds(hipStream_t s, const VarBoundTask* hop, int n_hop, const VarBoundTask* scan, int n_scan)
{
    if (n_hop > 0) hipLaunchKernelGGL(var_hop_kernel, dim3((n_hop + 63) / 64), dim3(64), 0, s, hop, n_hop);
    if (n_scan > 0) hipLaunchKernelGGL(var_scan_kernel, dim3((n_scan + 3) / 4), dim3(256), 0, s, scan, n_scan);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <int NB>
static int launch_var_score_nb(hipStream_t s, int mode, dim3 grid, const VarRead* reads, const int64_t* first, int n_reads, int64_t n_pass)
{
    if (mode == 0) hipLaunchKernelGGL((variant_score_kernel<1, NB, true>), grid, dim3(256), 0, s, reads, first, n_reads, n_pass);
    else if (mode == 1) hipLaunchKernelGGL((variant_score_kernel<1, NB, false>), grid, dim3(256), 0, s, reads, first, n_reads, n_pass);
    else if (mode == 2) hipLaunchKernelGGL((variant_score_kernel<2, NB, false>), grid, dim3(256), 0, s, reads, first, n_reads, n_pass);
    else return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_var_score(hipStream_t s, int mode, int n_branch, const VarRead* reads, const int64_t* first, int n_reads, int64_t n_passages, int n_cu)
{
    if (n_reads <= 0 || n_passages <= 0) return 0;
    const int64_t slots = mode == 0 ? (n_passages + 1) / 2 : n_passages;
    // eight workgroups of four waves per CU, the rest of the passages by stride (as launch_llr_score)
    const int64_t want = (slots + 3) / 4, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * 8;
    const dim3 grid((unsigned)(want < cap ? want : cap));
    if (n_branch == 2) return launch_var_score_nb<2>(s, mode, grid, reads, first, n_reads, n_passages);
    if (n_branch == 3) return launch_var_score_nb<3>(s, mode, grid, reads, first, n_reads, n_passages);
    if (n_branch == 4) return launch_var_score_nb<4>(s, mode, grid, reads, first, n_reads, n_passages);
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host: the edge image
namespace {
struct VarImageLayout {
    size_t src, lp, src2, lp2, start_lp, kind, ea, eb, ec, hub, end_src, end_lp, total;
    VarImageLayout()
    {
        size_t o = (sizeof(VarModel) + 15) & ~(size_t)15;
        auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
        src = take(2 * VAR_DEG * 64 * 4); lp = take(2 * VAR_DEG * 64 * 8);
        src2 = take((VAR_MAX_NB - 1) * 2 * VAR_DEG2 * 64 * 4); lp2 = take((VAR_MAX_NB - 1) * 2 * VAR_DEG2 * 64 * 8);
        start_lp = take(2 * 64 * 8); kind = take(2 * 64 * 4);
        ea = take(2 * 64 * 8); eb = take(2 * 64 * 8); ec = take(2 * 64 * 8); hub = take(2 * 64 * 4);
        end_src = take(VAR_MAX_NB * VAR_END_DEG * 4); end_lp = take(VAR_MAX_NB * VAR_END_DEG * 8);
        total = o;
    }
};
}  // namespace

size_t var_image_bytes() { return VarImageLayout().total; }

int var_build_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end, const int32_t* in_ptr, const int32_t* in_src,
                    const double* in_logp, const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                    const int32_t* state_tag, int32_t n_alt, const void* dev_base, std::vector<char>& blob, int32_t* mode, std::string& why)
{
    const int ne = silent_start;
    const int NB = n_alt + 1;
    if (n_alt < 1 || NB > VAR_MAX_NB) { why = "variants: between 1 and " + std::to_string(VAR_MAX_NB - 1) + " alt units per target"; return 1; }
    if (!state_tag) { why = "variants: the variant model carries no state tags"; return 1; }
    if (ne > VAR_MAX_EMIT) {
        why = "variants: variant models of at most " + std::to_string(VAR_MAX_EMIT) + " emitting states are supported (2 + 2 L + 2 n_alt (m + 1) L for a unit of L nt with m context units); this one has " + std::to_string(ne);
        return 1;
    }
    if (ne < 1 || n_states != ne + 2 || start < ne || end < ne || start == end || in_ptr[start + 1] != in_ptr[start]) {
        why = "variants: the variant model has silent states besides start and end"; return 1;
    }
    const VarImageLayout L;
    blob.assign(L.total, 0);
    int32_t* src = reinterpret_cast<int32_t*>(&blob[L.src]); double* lp = reinterpret_cast<double*>(&blob[L.lp]);
    int32_t* src2 = reinterpret_cast<int32_t*>(&blob[L.src2]); double* lp2 = reinterpret_cast<double*>(&blob[L.lp2]);
    double* slp = reinterpret_cast<double*>(&blob[L.start_lp]);
    int32_t* kind = reinterpret_cast<int32_t*>(&blob[L.kind]); int32_t* hub = reinterpret_cast<int32_t*>(&blob[L.hub]);
    double* ea = reinterpret_cast<double*>(&blob[L.ea]); double* eb = reinterpret_cast<double*>(&blob[L.eb]); double* ec = reinterpret_cast<double*>(&blob[L.ec]);
    int32_t* esrc = reinterpret_cast<int32_t*>(&blob[L.end_src]); double* elp = reinterpret_cast<double*>(&blob[L.end_lp]);
    for (int i = 0; i < 2 * VAR_DEG * 64; ++i) { src[i] = VAR_PAD; lp[i] = -INFINITY; }
    for (int i = 0; i < (VAR_MAX_NB - 1) * 2 * VAR_DEG2 * 64; ++i) { src2[i] = VAR_PAD; lp2[i] = -INFINITY; }
    for (int i = 0; i < 2 * 64; ++i) slp[i] = -INFINITY;
    for (int i = 0; i < VAR_MAX_NB * VAR_END_DEG; ++i) { esrc[i] = VAR_PAD; elp[i] = -INFINITY; }
    VarModel M; std::memset(&M, 0, sizeof(M));
    M.n_emit = ne; M.n_branch = NB; M.mode = ne <= 32 ? 0 : (ne <= 64 ? 1 : 2);
    // branch of an emitting state, -1 for a hub; anything else is refused
    std::vector<int> br((size_t)ne);
    for (int l = 0; l < ne; ++l) {
        br[(size_t)l] = var_branch_of_tag(state_tag[l]);
        if ((br[(size_t)l] < 0 && state_tag[l] != 2) || br[(size_t)l] >= NB) {
            why = "variants: state tags of a variant model with " + std::to_string(n_alt) + " alt units must be 0 (base), 2 (hub) or 1 / 3 / 4 (alt branch 1 / 2 / 3)"; return 1;
        }
    }
    for (int b = 0; b < NB; ++b)
        if (std::find(br.begin(), br.end(), b) == br.end()) { why = "variants: the state tags of the variant model describe fewer than " + std::to_string(n_alt) + " alt branches (no state of branch " + std::to_string(b) + ")"; return 1; }
    for (int l = 0; l < ne; ++l) {
        const int bl = br[(size_t)l];
        const int slot = l >> 6, lane = l & 63;
        kind[slot * 64 + lane] = emis_kind[l]; hub[slot * 64 + lane] = bl < 0;
        if (emis_kind[l] != 1 && emis_kind[l] != 2) { why = "variants: unknown emission kind"; return 1; }
        ea[slot * 64 + lane] = emis_a[l]; eb[slot * 64 + lane] = emis_b[l]; ec[slot * 64 + lane] = emis_c[l];
        int n1 = 0, n2[VAR_MAX_NB] = {0, 0, 0, 0};
        for (int e = in_ptr[l]; e < in_ptr[l + 1]; ++e) {
            const int k = in_src[e];
            if (k == start) { slp[slot * 64 + lane] = in_logp[e]; continue; }          // into every copy of a hub, into the one value of a branch state
            if (k >= ne) { why = "variants: the variant model has silent states besides start and end"; return 1; }
            const int bk = br[(size_t)k];
            // own value: copy 0 of a hub, the branch of a branch state; an edge from another branch is masked
            const int own = bl < 0 ? 0 : bl;
            if (bk < 0 || bk == own) {
                if (n1 >= VAR_DEG) { why = "variants: a state of the variant model has more than " + std::to_string(VAR_DEG) + " in-edges inside one branch"; return 1; }
                src[(slot * VAR_DEG + n1) * 64 + lane] = bk < 0 ? 128 * own + k : k;
                lp[(slot * VAR_DEG + n1) * 64 + lane] = in_logp[e]; ++n1;
            }
            if (bl < 0) {
                for (int c = 1; c < NB; ++c) {          // the further copies of a hub
                    if (bk >= 0 && bk != c) continue;
                    if (n2[c] >= VAR_DEG2) { why = "variants: a hub state of the variant model has more than " + std::to_string(VAR_DEG2) + " in-edges inside one branch"; return 1; }
                    const size_t at = (size_t)(((c - 1) * 2 + slot) * VAR_DEG2 + n2[c]) * 64 + (size_t)lane;
                    src2[at] = bk < 0 ? 128 * c + k : k; lp2[at] = in_logp[e]; ++n2[c];
                }
            }
        }
        M.deg = std::max(M.deg, n1);
        for (int c = 1; c < NB; ++c) M.deg2 = std::max(M.deg2, n2[c]);
    }
    for (int e = in_ptr[end]; e < in_ptr[end + 1]; ++e) {
        const int k = in_src[e];
        if (k >= ne) { why = "variants: the variant model has silent states besides start and end"; return 1; }
        const int bk = br[(size_t)k];
        for (int c = 0; c < NB; ++c) {
            if (bk >= 0 && bk != c) continue;
            if (M.end_deg[c] >= VAR_END_DEG) { why = "variants: the end state of the variant model has more than " + std::to_string(VAR_END_DEG) + " in-edges"; return 1; }
            esrc[c * VAR_END_DEG + M.end_deg[c]] = bk < 0 ? 128 * c + k : k;
            elp[c * VAR_END_DEG + M.end_deg[c]] = in_logp[e]; ++M.end_deg[c];
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
