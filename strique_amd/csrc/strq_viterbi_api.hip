// C ABI: baked HMM upload and Viterbi decode (single and batched).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <vector>
#include <string>
#include "../../include/strique_hip.h"
#include "strq_ctx.h"
#include "detect_plan.h"
#include "viterbi_kernels.h"

using namespace strq;

namespace strq {

// A model image -- arrays and, behind them, the struct that points to them, in one device blob: put() carves the region of an array
// and keeps where its bytes come from, host() is the block as it goes up (the sources as they are then: the struct with its pointers set).
struct Image {
    Carve lay;
    struct Part { const void* src; size_t bytes, off; };
    std::vector<Part> parts;
    template <class T> size_t put(const T* src, size_t n) { parts.push_back({src, n * sizeof(T), lay.add<T>(n)}); return parts.back().off; }
    template <class T> size_t put(const std::vector<T>& v) { return put(v.data(), v.size()); }
    std::vector<char> host() const
    {
        std::vector<char> h(lay.total(), 0);
        for (const Part& pt : parts) if (pt.bytes) std::memcpy(&h[pt.off], pt.src, pt.bytes);
        return h;
    }
};

// What every builder relies on: in_ptr monotone from 0, sources in range, silent states in topological order, the in-edges
// of a state sorted by ascending source (the order ties are broken in), emitting states Normal (1) or Uniform (2).
// Returns the reason, or null.
static const char* validate_vit_model(int32_t n_states, int32_t silent_start, const int32_t* in_ptr, const int32_t* in_src, const int32_t* emis_kind)
{
    if (in_ptr[0] != 0) return "in_ptr must start at 0";
    for (int l = 0; l < n_states; ++l) if (in_ptr[l + 1] < in_ptr[l]) return "in_ptr must not decrease";
    for (int l = 0; l < n_states; ++l)
        for (int e = in_ptr[l]; e < in_ptr[l + 1]; ++e) {
            const int k = in_src[e];
            if (k < 0 || k >= n_states) return "edge source out of range";
            if (l >= silent_start && k >= l) return "silent states are not in topological order";
            if (e > in_ptr[l] && in_src[e - 1] >= k) return "in-edges must be sorted by source";
        }
    for (int e = 0; e < silent_start; ++e) if (emis_kind[e] != 1 && emis_kind[e] != 2) return "emission kind must be 1 (Normal) or 2 (Uniform)";
    return nullptr;
}

// The two counted states of a unit decode (VIT_UNIT_T_MAX): exactly two emitting states with count_inc 1 and no other counted state
// -- STRique's dummy states, STRique.py:374-378
static void vit_unit_states(VitModel& m, int32_t n_states, int32_t ne, const int32_t* count_inc)
{
    m.unit_state[0] = m.unit_state[1] = -1;
    if (!count_inc) return;
    int found = 0, st[2] = {-1, -1};
    for (int l = 0; l < n_states; ++l) {
        if (count_inc[l] == 0) continue;
        if (l >= ne || count_inc[l] != 1 || found == 2) return;
        st[found++] = l;
    }
    if (found == 2) { m.unit_state[0] = st[0]; m.unit_state[1] = st[1]; }
}

// The lane layout of a model as the host plans it -- no context, no device: the VitModel with its dimensions, degrees and flags (its
// pointers stay null) and every array of the image.  build_vit_model uploads it, strq_debug_viterbi_plan reports it.
struct VitPlan {
    VitModel m;
    std::vector<double> lp, a, b, cc, chain_lp;
    std::vector<int32_t> src, kind, inc, own_e, own_s, chain_src, tag, cell_state, edge_csr, chain_csr;
    int32_t fwd_stages = 1;
};

// Returns STRQ_OK, or the status build_vit_model is to return with the reason in *why.
static int plan_vit_model(int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                          const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                          const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                          const int32_t* count_inc, const int32_t* state_tag,
                          const int32_t* hint_slot, const int32_t* hint_lane, VitPlan& P, const char** why)
{
    const int ne = silent_start, ns = n_states - silent_start;
    if (n_states < 2 || ne < 1 || ns < 2 || start < ne || end < ne || start >= n_states || end >= n_states) {
        *why = "bad model dimensions"; return STRQ_ERR_ARG;
    }
    // the edge lists are validated before any size decision: a model too large for the lane layouts goes on to the general
    // kernel's builder, which indexes host arrays with these sources
    if (const char* bad = validate_vit_model(n_states, silent_start, in_ptr, in_src, emis_kind)) { *why = bad; return STRQ_ERR_ARG; }
    const int epl = (ne + 63) / 64, spl = (ns + 63) / 64;
    if (epl > 8 || spl > 4 || n_states >= 65535) { *why = "model too large for the compiled Viterbi kernels"; return STRQ_ERR_UNSUPPORTED; }
    VitModel& m = P.m;
    std::memset(&m, 0, sizeof(m));
    m.n_states = n_states; m.n_emit = ne; m.n_silent = ns; m.start = start; m.end = end; m.epl = epl; m.spl = spl;
    // emitting states: dealt to slots by descending in-degree (slot 0 takes the 64 busiest, ...)
    auto deg_of = [&](int st) { return in_ptr[st + 1] - in_ptr[st]; };
    std::vector<int> eord(ne);
    for (int i = 0; i < ne; ++i) eord[i] = i;
    std::stable_sort(eord.begin(), eord.end(), [&](int a, int b) { return deg_of(a) > deg_of(b); });
    std::vector<int32_t>& own_e = P.own_e;
    own_e.assign((size_t)epl * 64, -1);
    bool hinted = hint_slot && hint_lane;
    if (hinted) {      // caller-provided (slot, lane) of every emitting state: must be a valid injective map
        for (int e = 0; e < ne && hinted; ++e) {
            const int sl = hint_slot[e], ln = hint_lane[e];
            if (sl < 0 || sl >= epl || ln < 0 || ln >= 64 || own_e[sl * 64 + ln] >= 0) hinted = false; else own_e[sl * 64 + ln] = e;
        }
        if (!hinted) std::fill(own_e.begin(), own_e.end(), -1);
    }
    if (!hinted) for (int i = 0; i < ne; ++i) own_e[i] = eord[i];
    else if (epl >= 2) {
        // the few states with more than five in-edges (the first match / insert of the repeat unit) move into free lanes of
        // slot 0, so that the second busy slot gets by with five in-edge registers (kernel shape 5)
        std::vector<int> movers;
        for (int lane = 0; lane < 64; ++lane) { const int st = own_e[64 + lane]; if (st >= 0 && deg_of(st) > 5) movers.push_back(lane); }
        int free0 = 0;
        for (int lane = 0; lane < 64; ++lane) if (own_e[lane] < 0) ++free0;
        if (!movers.empty() && (int)movers.size() <= free0 && movers.size() <= 4) {
            int lane0 = 0;
            for (int lane : movers) {
                while (own_e[lane0] >= 0) ++lane0;
                own_e[lane0] = own_e[64 + lane]; own_e[64 + lane] = -1;
            }
        }
    }
    // silent states: chains.  The chain predecessor of b is its highest-numbered silent predecessor
    // (the last in-edge in evaluation order, so a strict '>' reproduces the tie rule) if that state
    // does not already lead another chain.
    std::vector<int> chain_pred(n_states, -1), chain_succ(n_states, -1), chain_e(n_states, -1); std::vector<double> chain_lp(n_states, 0.0);
    for (int b = ne; b < n_states; ++b) {
        int a = -1, ae = -1; double lpv = 0;
        for (int e = in_ptr[b]; e < in_ptr[b + 1]; ++e) if (in_src[e] >= ne) { a = in_src[e]; lpv = in_logp[e]; ae = e; }
        if (a >= 0 && chain_succ[a] < 0) { chain_pred[b] = a; chain_succ[a] = b; chain_lp[b] = lpv; chain_e[b] = ae; }
    }
    std::vector<std::vector<int>> chains;
    for (int b = ne; b < n_states; ++b) if (chain_pred[b] < 0) { std::vector<int> ch; for (int x = b; x >= 0; x = chain_succ[x]) ch.push_back(x); chains.push_back(ch); }
    std::stable_sort(chains.begin(), chains.end(), [](const std::vector<int>& x, const std::vector<int>& y) { return x.size() > y.size(); });
    // Chains zig-zag through the Z silent slots of a lane (the chains back to back; cell p of that sequence: lane p / Z,
    // slot p % Z; the first cell of a chain has no chain edge), so that one lane shift of the kernel's chain sweep carries
    // a value Z positions along (viterbi_kernels.hip).  Z is the slot count of the kernel shape the model runs on: the smallest layout is tried
    // first and widened until the shape that fits it has exactly that many silent slots.
    std::vector<int32_t>& own_s = P.own_s; std::vector<int32_t>& chain_src_v = P.chain_src; std::vector<double>& chain_lp_v = P.chain_lp;
    auto lay_out = [&](int Z) -> bool {
        if (ns > 64 * Z) return false;
        own_s.assign((size_t)Z * 64, -1); chain_src_v.assign((size_t)Z * 64, -1); chain_lp_v.assign((size_t)Z * 64, 0.0);
        int p = 0;
        for (auto& ch : chains) {
            for (size_t q = 0; q < ch.size(); ++q, ++p) {
                const int lane = p / Z, slot = p % Z, st = ch[q];
                own_s[(size_t)slot * 64 + lane] = st;
                if (q > 0) { chain_src_v[(size_t)slot * 64 + lane] = ch[q - 1]; chain_lp_v[(size_t)slot * 64 + lane] = chain_lp[st]; }
            }
        }
        m.spl = Z;
        return true;
    };
    auto slot_degrees = [&]() {
        for (int s2 = 0; s2 < 8; ++s2) m.s_deg[s2] = 0;
        for (int s2 = 0; s2 < m.spl; ++s2) {
            int deg = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int st = own_s[(size_t)s2 * 64 + lane];
                if (st < 0) continue;
                int dg = 0;
                for (int e = in_ptr[st]; e < in_ptr[st + 1]; ++e) if (chain_src_v[(size_t)s2 * 64 + lane] != in_src[e]) ++dg;
                deg = std::max(deg, dg);
            }
            m.s_deg[s2] = deg;
        }
    };
    for (int s2 = 0; s2 < epl; ++s2) {       // the shape test below needs the emitting degrees
        int deg = 0; bool flat = true;
        for (int lane = 0; lane < 64; ++lane) if (own_e[s2 * 64 + lane] >= 0) {
            deg = std::max(deg, deg_of(own_e[s2 * 64 + lane]));
            flat = flat && emis_kind[own_e[s2 * 64 + lane]] != 1;
        }
        m.e_deg[s2] = deg; m.e_flat[s2] = flat ? 1 : 0;
    }
    {
        bool placed = false;
        for (int Z = 1; Z <= 4 && !placed; Z *= 2) {
            if (!lay_out(Z)) continue;
            slot_degrees();
            m.single_stage = 1;      // refined below; the shape does not depend on it
            const int shape = vit_shape_of(m);
            if (shape >= 0 && vit_shape_silent_slots(shape) == Z) placed = true;
        }
        if (!placed) { *why = "model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
    }
    const int spl2 = m.spl;
    auto is_chain_edge = [&](int dst, int srcst) {
        for (int i = 0; i < spl2 * 64; ++i) if (own_s[i] == dst) return chain_src_v[i] == srcst;
        return false;
    };
    int rows = 0;
    for (int s = 0; s < epl; ++s) {
        int deg = 0;
        for (int lane = 0; lane < 64; ++lane) if (own_e[s * 64 + lane] >= 0) deg = std::max(deg, deg_of(own_e[s * 64 + lane]));
        m.e_deg[s] = deg; m.e_base[s] = rows; rows += deg;
    }
    std::vector<int> sdeg_state(n_states, 0);
    for (int b = ne; b < n_states; ++b) { int dg = 0; for (int e = in_ptr[b]; e < in_ptr[b + 1]; ++e) if (!is_chain_edge(b, in_src[e])) ++dg; sdeg_state[b] = dg; }
    for (int s = 0; s < spl2; ++s) {
        int deg = 0;
        for (int lane = 0; lane < 64; ++lane) if (own_s[s * 64 + lane] >= 0) deg = std::max(deg, sdeg_state[own_s[s * 64 + lane]]);
        m.s_deg[s] = deg; m.s_base[s] = rows; rows += deg;
    }
    m.single_stage = 1;
    for (int b = ne; b < n_states; ++b) for (int e = in_ptr[b]; e < in_ptr[b + 1]; ++e) if (in_src[e] >= ne && !is_chain_edge(b, in_src[e])) m.single_stage = 0;
    for (int s = 0; s < 8; ++s) if (m.e_deg[s] > 8 || m.s_deg[s] > 8) { *why = "a state has more than 8 in-edges"; return STRQ_ERR_UNSUPPORTED; }
    m.n_edge_rows = rows;
    // LDS cells: the owner (slot, lane) of a state is its cell; the last cell is the -inf cell
    m.n_cells = (epl + spl2) * 64 + 1;
    std::vector<int32_t> cell_of(n_states, -1); std::vector<int32_t>& cell_state = P.cell_state;
    cell_state.assign((size_t)m.n_cells, -1);
    for (int i = 0; i < epl * 64; ++i) if (own_e[i] >= 0) { cell_of[own_e[i]] = i; cell_state[i] = own_e[i]; }
    // silent cells are interleaved (cell = first silent cell + lane * spl + slot = position along the zig-zag), so that
    // the emitting states of consecutive lanes read their delete predecessors from consecutive LDS cells
    for (int i = 0; i < spl2 * 64; ++i) if (own_s[i] >= 0) {
        const int cell = epl * 64 + (i % 64) * spl2 + i / 64;
        cell_of[own_s[i]] = cell; cell_state[cell] = own_s[i];
    }
    m.start_cell = cell_of[start]; m.end_cell = cell_of[end];
    std::vector<int32_t>& src = P.src; std::vector<double>& lp = P.lp;
    src.assign((size_t)std::max(rows, 1) * 64, m.n_cells - 1);   // padding -> the -inf cell
    lp.assign((size_t)std::max(rows, 1) * 64, 0.0);
    P.edge_csr.assign((size_t)std::max(rows, 1) * 64, -1);
    auto fill = [&](int state, int base, int lane) {
        for (int e = in_ptr[state], j = 0; e < in_ptr[state + 1]; ++e) {
            if (state >= ne && is_chain_edge(state, in_src[e])) continue;
            src[(size_t)(base + j) * 64 + lane] = cell_of[in_src[e]];
            lp[(size_t)(base + j) * 64 + lane] = in_logp[e];
            P.edge_csr[(size_t)(base + j) * 64 + lane] = e;
            ++j;
        }
    };
    for (int s = 0; s < epl; ++s) for (int lane = 0; lane < 64; ++lane) if (own_e[s * 64 + lane] >= 0) fill(own_e[s * 64 + lane], m.e_base[s], lane);
    for (int s = 0; s < spl2; ++s) for (int lane = 0; lane < 64; ++lane) if (own_s[s * 64 + lane] >= 0) fill(own_s[s * 64 + lane], m.s_base[s], lane);
    // forward pass: the CSR edge behind every chain edge, and how many silent states a path can cross through edges that are
    // not chain edges (the silent phase of forward_kernel runs once more for each)
    P.chain_csr.assign((size_t)spl2 * 64, -1);
    for (int i = 0; i < spl2 * 64; ++i) if (own_s[i] >= 0 && chain_src_v[i] >= 0) P.chain_csr[i] = chain_e[own_s[i]];
    {
        std::vector<int> depth(n_states, 0); int deepest = 0;
        for (int b = ne; b < n_states; ++b) {
            int dp = 0;
            for (int e = in_ptr[b]; e < in_ptr[b + 1]; ++e) if (in_src[e] >= ne) dp = std::max(dp, depth[in_src[e]] + (is_chain_edge(b, in_src[e]) ? 0 : 1));
            depth[b] = dp; deepest = std::max(deepest, dp);
        }
        P.fwd_stages = deepest + 1;
    }
    std::vector<int32_t>& kind = P.kind; std::vector<double>& a = P.a; std::vector<double>& b = P.b; std::vector<double>& cc = P.cc;
    kind.assign((size_t)epl * 64, 0); a.assign((size_t)epl * 64, 0.0); b = a; cc = a;
    for (int i = 0; i < epl * 64; ++i) if (own_e[i] >= 0) { const int e = own_e[i]; kind[i] = emis_kind[e]; a[i] = emis_a[e]; b[i] = emis_b[e]; cc[i] = emis_c[e]; }
    m.uni_lo_max = -INFINITY; m.uni_hi_min = INFINITY;
    for (int e = 0; e < ne; ++e) if (emis_kind[e] == 2) { m.uni_lo_max = std::max(m.uni_lo_max, emis_a[e]); m.uni_hi_min = std::min(m.uni_hi_min, emis_b[e]); }
    P.inc.assign((size_t)n_states + 1, 0);
    if (count_inc) std::copy(count_inc, count_inc + n_states, P.inc.begin());
    P.tag.assign((size_t)n_states + 1, 0);
    if (state_tag) std::copy(state_tag, state_tag + n_states, P.tag.begin());
    m.rec_state = -1;
    for (int e = in_ptr[end]; e < in_ptr[end + 1]; ++e) if (in_src[e] < ne && state_tag && state_tag[in_src[e]] == 2) m.rec_state = in_src[e];
    m.silent_counted = 0;
    for (int s2 = ne; s2 < n_states; ++s2) if (count_inc && count_inc[s2] != 0) m.silent_counted = 1;
    vit_unit_states(m, n_states, ne, count_inc);
    return STRQ_OK;
}

int build_vit_model(strq_ctx* c, int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                    const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                    const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                    const int32_t* count_inc, const int32_t* state_tag,
                    const int32_t* hint_slot, const int32_t* hint_lane, HostModel** out)
{
    VitPlan P; const char* why = nullptr;
    if (const int prc = plan_vit_model(n_states, silent_start, start, end, in_ptr, in_src, in_logp, emis_kind, emis_a, emis_b, emis_c, count_inc, state_tag,
                                       hint_slot, hint_lane, P, &why)) { c->err = why; return prc; }
    HostModel* hm = new HostModel();
    VitModel& m = hm->h;
    m = P.m;
    hm->edge_csr.swap(P.edge_csr); hm->chain_csr.swap(P.chain_csr); hm->fwd_stages = P.fwd_stages; hm->cell_state = P.cell_state;
    // one device blob: the arrays, the VitModel that points to them behind
    Image im;
    const size_t o_lp = im.put(P.lp), o_a = im.put(P.a), o_b = im.put(P.b), o_c = im.put(P.cc), o_src = im.put(P.src), o_kind = im.put(P.kind), o_inc = im.put(P.inc),
                 o_own_e = im.put(P.own_e), o_own_s = im.put(P.own_s), o_chain_src = im.put(P.chain_src), o_chain_lp = im.put(P.chain_lp),
                 o_tag = im.put(P.tag), o_cell = im.put(P.cell_state), o_m = im.put(&m, 1);
    if (hm->blob.reserve(im.lay.total()) != hipSuccess) { delete hm; c->err = "out of device memory"; return STRQ_ERR_NOMEM; }
    void* d = hm->blob.p;
    m.edge_logp = Carve::at<const double>(d, o_lp); m.emis_a = Carve::at<const double>(d, o_a); m.emis_b = Carve::at<const double>(d, o_b);
    m.emis_c = Carve::at<const double>(d, o_c); m.edge_src = Carve::at<const int32_t>(d, o_src); m.emis_kind = Carve::at<const int32_t>(d, o_kind);
    m.count_inc = Carve::at<const int32_t>(d, o_inc); m.own_e = Carve::at<const int32_t>(d, o_own_e); m.own_s = Carve::at<const int32_t>(d, o_own_s);
    m.chain_src = Carve::at<const int32_t>(d, o_chain_src); m.chain_logp = Carve::at<const double>(d, o_chain_lp);
    m.state_tag = Carve::at<const int32_t>(d, o_tag); m.cell_state = Carve::at<const int32_t>(d, o_cell);
    hm->dev = Carve::at<const VitModel>(d, o_m);
    if (hipMemcpy(d, im.host().data(), im.lay.total(), hipMemcpyHostToDevice) != hipSuccess) { delete hm; c->err = "model upload failed"; return STRQ_ERR_DEVICE; }
    *out = hm;
    return STRQ_OK;
}

// The baked arrays as they are, for viterbi_csr_kernel (models the lane layouts do not cover).
int build_vit_model_csr(strq_ctx* c, int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                        const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                        const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                        const int32_t* count_inc, const int32_t* state_tag, HostModel** out)
{
    const int ne = silent_start, ns = n_states - silent_start;
    if (n_states > VIT_CSR_MAX_STATES) { c->err = "model too large: more than 4096 states"; return STRQ_ERR_UNSUPPORTED; }
    HostModel* hm = new HostModel();
    VitModel& m = hm->h;
    std::memset(&m, 0, sizeof(m));
    m.n_states = n_states; m.n_emit = ne; m.n_silent = ns; m.start = start; m.end = end; m.epl = 0; m.spl = 0;
    m.csr = 1; m.n_cells = n_states + 1; m.start_cell = start; m.end_cell = end; m.rec_state = -1; m.single_stage = 0;
    m.unit_state[0] = m.unit_state[1] = -1;          // no unit decode on this kernel: the unit pass takes back-pointers
    // level of a silent state: length of its longest chain of silent predecessors (they are in topological order)
    std::vector<int> level(n_states, 0); int nlev = 0;
    for (int l = ne; l < n_states; ++l) {
        int lv = 0;
        for (int e = in_ptr[l]; e < in_ptr[l + 1]; ++e) if (in_src[e] >= ne) lv = std::max(lv, level[in_src[e]] + 1);
        level[l] = lv; nlev = std::max(nlev, lv + 1);
    }
    std::vector<int32_t> level_ptr((size_t)nlev + 1, 0), level_state((size_t)std::max(ns, 1), 0);
    for (int l = ne; l < n_states; ++l) ++level_ptr[(size_t)level[l] + 1];
    for (int v = 0; v < nlev; ++v) level_ptr[(size_t)v + 1] += level_ptr[v];
    { std::vector<int32_t> pos(level_ptr.begin(), level_ptr.end() - 1);
      for (int l = ne; l < n_states; ++l) level_state[(size_t)pos[level[l]]++] = l; }
    m.n_levels = nlev;
    m.uni_lo_max = -INFINITY; m.uni_hi_min = INFINITY;
    for (int e = 0; e < ne; ++e) if (emis_kind[e] == 2) { m.uni_lo_max = std::max(m.uni_lo_max, emis_a[e]); m.uni_hi_min = std::min(m.uni_hi_min, emis_b[e]); }
    std::vector<int32_t> inc((size_t)n_states + 1, 0), tagv((size_t)n_states + 1, 0);
    if (count_inc) std::copy(count_inc, count_inc + n_states, inc.begin());
    if (state_tag) std::copy(state_tag, state_tag + n_states, tagv.begin());
    const int n_edges = in_ptr[n_states];
    Image im;
    const size_t o_lp = im.put(in_logp, (size_t)n_edges), o_a = im.put(emis_a, (size_t)ne), o_b = im.put(emis_b, (size_t)ne), o_c = im.put(emis_c, (size_t)ne),
                 o_ptr = im.put(in_ptr, (size_t)n_states + 1), o_src = im.put(in_src, (size_t)n_edges), o_kind = im.put(emis_kind, (size_t)ne),
                 o_inc = im.put(inc), o_tag = im.put(tagv), o_level_ptr = im.put(level_ptr), o_level_state = im.put(level_state), o_m = im.put(&m, 1);
    if (hm->blob.reserve(im.lay.total()) != hipSuccess) { delete hm; c->err = "out of device memory"; return STRQ_ERR_NOMEM; }
    void* d = hm->blob.p;
    m.csr_in_logp = Carve::at<const double>(d, o_lp); m.csr_a = Carve::at<const double>(d, o_a); m.csr_b = Carve::at<const double>(d, o_b);
    m.csr_c = Carve::at<const double>(d, o_c); m.csr_in_ptr = Carve::at<const int32_t>(d, o_ptr); m.csr_in_src = Carve::at<const int32_t>(d, o_src);
    m.csr_kind = Carve::at<const int32_t>(d, o_kind); m.count_inc = Carve::at<const int32_t>(d, o_inc); m.state_tag = Carve::at<const int32_t>(d, o_tag);
    m.csr_level_ptr = Carve::at<const int32_t>(d, o_level_ptr); m.csr_level_state = Carve::at<const int32_t>(d, o_level_state);
    hm->dev = Carve::at<const VitModel>(d, o_m);
    if (hipMemcpy(d, im.host().data(), im.lay.total(), hipMemcpyHostToDevice) != hipSuccess) { delete hm; c->err = "model upload failed"; return STRQ_ERR_DEVICE; }
    *out = hm;
    return STRQ_OK;
}

// Register-resident image of a profile chain (VitG2, vit_model.h) from the position of every emitting state along the
// chain: kind 0 = match-type, 1 = insert-type, pos >= 0.  Silent states take the position after their emitting / silent
// predecessors (a silent state without predecessors -- start -- the position before its match-type successor).  Every
// in-edge must fall into a column of the layout, in ascending column order (= ascending source state, the order ties are
// broken in); the states that need the even-position columns (a broadcast source, an insert-type state fed by the previous
// delete state) decide the parity of the whole chain.  Returns STRQ_ERR_UNSUPPORTED when the model is not such a chain:
// it then keeps running on its lane layout.
struct G2Host {
    std::vector<double> lp, em; std::vector<int32_t> knd, own, inc, tag;
    std::vector<uint64_t> mark_add;      // empty: the tagged states are no contiguous stretch of the chain
    VitG2 G;
    int odd = 0;
};

// host part: the tables of the image (no device involved), or the reason there is none
static bool g2_layout(const HostModel* hm, const int32_t* kind_hint, const int32_t* pos_hint, G2Host& out, std::string& why_out)
{
    const int n = hm->n_states, ne = hm->silent_start;
    const std::vector<int32_t>& in_ptr = hm->in_ptr; const std::vector<int32_t>& in_src = hm->in_src; const std::vector<double>& in_logp = hm->in_logp;
    auto unsupported = [&](const char* why) { why_out = why; return false; };
    for (int b = ne; b < n; ++b) if (!hm->count_inc.empty() && hm->count_inc[b] != 0) return unsupported("a silent state is counted");
    for (int e = 0; e < ne; ++e) {
        if ((kind_hint[e] != 0 && kind_hint[e] != 1) || pos_hint[e] < 0 || pos_hint[e] > 125) return unsupported("an emitting state has no position");
        if (kind_hint[e] == 1 && hm->emis_kind[e] == 1) return unsupported("an insert-type state has a Normal emission");
    }
    const double NEG = -INFINITY;
    std::string why = "?", why_all;
    struct Edge { int src; double lp; };
    for (int off = 0; off < 2; ++off) {
        if (off == 1) why_all = why + "; ";
        std::vector<int> g(n, -1), kind(n, 2);
        for (int e = 0; e < ne; ++e) { g[e] = pos_hint[e] + 1 + off; kind[e] = kind_hint[e]; }
        bool ok = true;
        for (int b = ne; b < n && ok; ++b) {
            int gp = -1;
            for (int e = in_ptr[b]; e < in_ptr[b + 1]; ++e) {
                const int k = in_src[e];
                if (g[k] < 0) { ok = false; why = "a silent state precedes its predecessor"; break; }
                if (gp < 0) gp = g[k] + 1; else if (gp != g[k] + 1) { ok = false; why = "a silent state has predecessors at two positions"; break; }
            }
            if (ok && gp < 0) {      // no predecessors: the position before its match-type successor (else that of its insert-type successor)
                int gm = -1, gi = -1;
                for (int l = 0; l < ne; ++l) for (int e = in_ptr[l]; e < in_ptr[l + 1]; ++e) if (in_src[e] == b) { if (kind[l] == 0) gm = g[l] - 1; else gi = g[l]; }
                gp = gm >= 0 ? gm : gi;
                if (gp < 0) {      // only silent successors: right before the first of them is decided below -- take position 0
                    gp = 0;
                }
            }
            g[b] = gp;
        }
        if (!ok) continue;
        // one state per (kind, position), positions below 128
        std::vector<int> at(3 * 128, -1);
        for (int l = 0; l < n && ok; ++l) {
            if (g[l] < 0 || g[l] > 127) { ok = false; why = "the chain has more than 128 positions"; break; }
            int& slot = at[kind[l] * 128 + g[l]];
            if (slot >= 0) { ok = false; why = "two states of one type at one position"; break; }
            slot = l;
        }
        if (!ok) continue;
        // ---- in-edges per state, then the virtual relay states (see vit_model.h).  The in-edges of an insert-type state T
        // at position g, in evaluation order, must read   F ++ mid ++ back   with
        //   F    = sources among {I_{g-1}, M_{g-1}}                         (repeat0i, dummy1 <- e1 <- last insert / match before them)
        //   mid  = the regular columns {I_g (T itself), M_g, D_g}
        //   back = [one far emitting state], [D_{g-1}]                      (repeat0i <- s1 <- {dummy1, last prefix delete})
        // F and back go to a virtual delete-type state V at T's own position (free in a profile without delete states): F in V's
        // two gather columns, the far state in V's broadcast column, D_{g-1} as V's chain edge -- V evaluates them in exactly this
        // order -- and T keeps mid ++ [V with 0.0].  V stands LAST in T's tournament although F stands first in T's list: the
        // lane is flagged in `hub_mask`, and there the kernel lets V win a tie against mid when V's own winner came from F.
        std::vector<std::vector<Edge>> edges(n);
        for (int l = 0; l < n; ++l) for (int e = in_ptr[l]; e < in_ptr[l + 1]; ++e) edges[l].push_back({in_src[e], in_logp[e]});
        const int n_real = n;
        uint64_t hub_mask = 0;
        for (int l = 0; l < ne && ok; ++l) {
            if (kind[l] != 1) continue;
            const std::vector<Edge> E = edges[l];
            size_t i = 0;
            std::vector<Edge> F, mid, back;
            while (i < E.size() && E[i].src < ne && E[i].src != l && g[l] - g[E[i].src] == 1) F.push_back(E[i++]);
            while (i < E.size() && (E[i].src == l || (kind[E[i].src] == 0 && g[E[i].src] == g[l]) || (kind[E[i].src] == 2 && g[E[i].src] == g[l]))) mid.push_back(E[i++]);
            if (i < E.size() && E[i].src < ne && !(g[l] - g[E[i].src] == 1 || g[l] == g[E[i].src])) back.push_back(E[i++]);      // a far emitting state
            if (i < E.size() && kind[E[i].src] == 2 && g[l] - g[E[i].src] == 1) back.push_back(E[i++]);                          // D_{g-1}
            if (i != E.size()) { ok = false; why = "an insert-type state with in-edges no relay covers"; break; }
            if (F.empty() && back.empty()) continue;
            if (at[2 * 128 + g[l]] >= 0) { ok = false; why = "an insert-type state with irregular in-edges and a delete state at its position"; break; }
            if (!F.empty() && !mid.empty()) {
                // ties between F and mid are decided by the flag: only the even insert slot evaluates it
                if (g[l] & 1) { ok = false; why = "a relayed insert-type state at an odd position (parity " + std::to_string(off) + ")"; break; }
                hub_mask |= (uint64_t)1 << (g[l] >> 1);
            }
            const int v = (int)edges.size();
            std::vector<Edge> ve(F); ve.insert(ve.end(), back.begin(), back.end());
            mid.push_back({v, 0.0});
            edges[l] = mid;                                   // before the push_back below: it may move the vectors
            edges.push_back(ve); g.push_back(g[l]); kind.push_back(2);
            at[2 * 128 + g[l]] = v;
        }
        if (!ok) continue;
        const int n_all = (int)edges.size();
        std::vector<double> lp((size_t)G2_ROWS * 64, NEG), em((size_t)12 * 64, 0.0);
        std::vector<int32_t> knd((size_t)4 * 64, 0), own((size_t)6 * 64, -1), inc((size_t)4 * 64, 0), tag((size_t)4 * 64, 0);
        int bc_state[2] = {-1, -1};
        for (int l = 0; l < n_all && ok; ++l) {
            const int gl = g[l], par = gl & 1, lane = gl >> 1;
            int last_col = -1;
            for (const Edge& ed : edges[l]) {
                const int k = ed.src, kk = kind[k], dg = gl - g[k];
                int col = -1, row = -1;
                if (kind[l] == 0) {          // match-type
                    row = par ? G2_ROW_MO : G2_ROW_ME;
                    if (kk == 0 && dg == 2) col = 0; else if (kk == 1 && dg == 1) col = 1; else if (kk == 0 && dg == 1) col = 2;
                    else if (kk == 1 && dg == 0) col = 3; else if (k == l) col = 4;
                    else if (kk == 2 && dg == 1) col = par ? 5 : 6;
                    else if (!par && kk == 0 && k < ne && (bc_state[0] < 0 || bc_state[0] == k)) { col = 5; bc_state[0] = k; }
                } else if (kind[l] == 1) {   // insert-type: itself, the match and the delete state of its position
                    row = par ? G2_ROW_IO : G2_ROW_IE;
                    if (k == l) col = 0; else if (kk == 0 && dg == 0) col = 1; else if (kk == 2 && dg == 0) col = 2;
                } else {                     // delete-type: the gather columns, then the chain edge
                    row = par ? G2_ROW_DO : G2_ROW_DE;
                    if (kk == 1 && dg == 1) col = 0;
                    else if (kk == 0 && dg == 1) col = 1;
                    else if (kk == 2 && dg == 1) { row = G2_ROW_CHAIN + par; col = 3; }
                    else if (!par && kk == 1 && k < ne && (bc_state[1] < 0 || bc_state[1] == k)) { col = 2; bc_state[1] = k; }
                }
                if (col < 0) { ok = false; why = "an edge outside the columns of the layout (parity " + std::to_string(off) + ": state " + std::to_string(l) + " at position " + std::to_string(gl) +
                                                 " <- state " + std::to_string(k) + " of type " + std::to_string(kk) + " at position " + std::to_string(g[k]) + ")"; break; }
                if (col <= last_col) { ok = false; why = "in-edges not in column order"; break; }
                last_col = col;
                lp[(size_t)(row + (kind[l] == 2 && col == 3 ? 0 : col)) * 64 + lane] = ed.lp;
            }
            if (!ok) break;
            if (kind[l] < 2) {
                const int slot = kind[l] * 2 + par;
                own[(size_t)slot * 64 + lane] = l; knd[(size_t)slot * 64 + lane] = hm->emis_kind[l];
                em[((size_t)slot * 3 + 0) * 64 + lane] = hm->emis_a[l]; em[((size_t)slot * 3 + 1) * 64 + lane] = hm->emis_b[l]; em[((size_t)slot * 3 + 2) * 64 + lane] = hm->emis_c[l];
                inc[(size_t)slot * 64 + lane] = hm->count_inc.empty() ? 0 : hm->count_inc[l];
                tag[(size_t)slot * 64 + lane] = (!hm->state_tag.empty() && hm->state_tag[l] == 1) ? 1 : 0;
            } else own[(size_t)(4 + par) * 64 + lane] = l < n_real ? l : -2;
        }
        if (!ok) continue;
        if (in_ptr[hm->start + 1] != in_ptr[hm->start]) { why = "the start state has in-edges"; continue; }
        VitG2& G = out.G; std::memset(&G, 0, sizeof(G));
        for (int i = 0; i < 2; ++i) {
            G.bc_slot[i] = 2 * i; G.bc_lane[i] = -1;
            if (bc_state[i] >= 0) { G.bc_slot[i] = kind[bc_state[i]] * 2 + (g[bc_state[i]] & 1); G.bc_lane[i] = g[bc_state[i]] >> 1; }
        }
        G.start_slot = g[hm->start] & 1; G.start_lane = g[hm->start] >> 1; G.end_slot = g[hm->end] & 1; G.end_lane = g[hm->end] >> 1;
        G.hub_mask = hub_mask;
        // one code path per parity of the broadcast sources (a repeat profile of odd length puts them at an odd position)
        int par_bc = -1; bool bad_par = false;
        for (int i = 0; i < 2; ++i) if (bc_state[i] >= 0) { const int pb = g[bc_state[i]] & 1; if (par_bc >= 0 && par_bc != pb) bad_par = true; par_bc = pb; }
        if (bad_par) { why = "broadcast sources at positions of both parities"; continue; }
        out.odd = par_bc == 1 ? 1 : 0;
        // the kernel adds count increments only in the two slots of that parity (STRique counts the two dummy states: the broadcast sources)
        bool inc_elsewhere = false;
        for (int k = 0; k < 4; ++k) if ((k & 1) != out.odd) for (int lane = 0; lane < 64; ++lane) if (inc[(size_t)k * 64 + lane] != 0) inc_elsewhere = true;
        if (inc_elsewhere) { why = "a counted state at a position of the other parity"; continue; }
        // mark decodes: tagged emitting states must fill one stretch of positions [g_lo, g_hi] (every emitting state there is
        // tagged), so that a path -- which only moves forward along the chain, the loop inside the stretch apart -- emits
        // untagged / tagged / untagged in that order and two counters give the two boundaries (G2_MARK_*)
        out.mark_add.clear();
        if (!hm->state_tag.empty()) {
            int g_lo = 1 << 30, g_hi = -1; bool any = false, holes = false;
            for (int e = 0; e < ne; ++e) if (hm->state_tag[e] == 1) { any = true; g_lo = std::min(g_lo, g[e]); g_hi = std::max(g_hi, g[e]); }
            for (int e = 0; e < ne; ++e) if (hm->state_tag[e] != 1 && g[e] >= g_lo && g[e] <= g_hi) holes = true;
            if (any && !holes) {
                out.mark_add.assign((size_t)4 * 64, 0);
                for (int e = 0; e < ne; ++e) {
                    const size_t at_ = (size_t)(kind[e] * 2 + (g[e] & 1)) * 64 + (size_t)(g[e] >> 1);
                    uint64_t a = hm->state_tag[e] == 1 ? 1 : (g[e] > g_hi ? (uint64_t)1 << G2_MARK_BEHIND_SHIFT : 0);
                    if (!hm->count_inc.empty()) a += (uint64_t)(uint32_t)hm->count_inc[e] << G2_MARK_COUNT_SHIFT;
                    out.mark_add[at_] = a;
                }
            }
        }
        out.lp.swap(lp); out.em.swap(em); out.knd.swap(knd); out.own.swap(own); out.inc.swap(inc); out.tag.swap(tag);
        return true;
    }
    why = why_all + why;
    return unsupported(why.c_str());
}

int build_vit_g2(strq_ctx* c, HostModel* hm, const int32_t* kind_hint, const int32_t* pos_hint)
{
    if (hm->h.csr) { c->err = "no register-resident layout: the model runs on the general kernel"; return STRQ_ERR_UNSUPPORTED; }
    G2Host L; std::string why;
    if (!g2_layout(hm, kind_hint, pos_hint, L, why)) { c->err = "no register-resident layout: " + why; return STRQ_ERR_UNSUPPORTED; }
    {
        VitG2& G = L.G;
        std::vector<double>& lp = L.lp; std::vector<double>& em = L.em;
        std::vector<int32_t>& knd = L.knd; std::vector<int32_t>& own = L.own; std::vector<int32_t>& inc = L.inc; std::vector<int32_t>& tag = L.tag;
        Image im;
        const size_t o_lp = im.put(lp), o_em = im.put(em), o_kind = im.put(knd), o_own = im.put(own), o_inc = im.put(inc), o_tag = im.put(tag),
                     o_mark = im.put(L.mark_add), o_g = im.put(&G, 1);
        if (hm->g2_blob.reserve(im.lay.total()) != hipSuccess) { c->err = "out of device memory"; return STRQ_ERR_NOMEM; }
        void* d = hm->g2_blob.p;
        G.lp = Carve::at<const double>(d, o_lp); G.em = Carve::at<const double>(d, o_em);
        G.kind = Carve::at<const int32_t>(d, o_kind); G.own = Carve::at<const int32_t>(d, o_own);
        G.inc = Carve::at<const int32_t>(d, o_inc); G.tag = Carve::at<const int32_t>(d, o_tag);
        G.mark_add = L.mark_add.empty() ? nullptr : Carve::at<const uint64_t>(d, o_mark);
        if (hipMemcpy(d, im.host().data(), im.lay.total(), hipMemcpyHostToDevice) != hipSuccess) { c->err = "model upload failed"; return STRQ_ERR_DEVICE; }
        hm->h.g2 = Carve::at<const VitG2>(d, o_g); hm->h.g2_odd = L.odd; hm->h.g2_mark = L.mark_add.empty() ? 0 : 1;
        // unit decodes: the two counted states are the broadcast sources, one in each of their slots (record index = the slot's)
        {
            int hits[2] = {0, 0}; bool other = false;
            for (int k = 0; k < 4; ++k)
                for (int lane = 0; lane < 64; ++lane) {
                    const int32_t v = inc[(size_t)k * 64 + lane];
                    if (!v) continue;
                    if (v == 1 && (k == L.odd || k == 2 + L.odd) && lane == G.bc_lane[k >> 1] &&
                        (own[(size_t)k * 64 + lane] == hm->h.unit_state[0] || own[(size_t)k * 64 + lane] == hm->h.unit_state[1])) ++hits[k >> 1];
                    else other = true;
                }
            hm->h.g2_unit = (hm->h.unit_state[0] >= 0 && hits[0] == 1 && hits[1] == 1 && !other) ? 1 : 0;
        }
        if (hipMemcpy(const_cast<VitModel*>(hm->dev), &hm->h, sizeof(VitModel), hipMemcpyHostToDevice) != hipSuccess) { hm->h.g2 = nullptr; c->err = "model upload failed"; return STRQ_ERR_DEVICE; }
        return STRQ_OK;
    }
}

// Forward image of a model: the transition probabilities behind the rows of its lane layout (FwdModel).  exp() of the per-edge
// log-probabilities runs here, on the host, once per model.
int forward_model(strq_ctx* c, HostModel* hm)
{
    if (hm->fwd_dev) return STRQ_OK;
    if (hm->h.csr) { c->err = "forward pass: the model has no lane layout (more than 512 emitting / 256 silent states or more than 8 in-edges per state)"; return STRQ_ERR_UNSUPPORTED; }
    for (int l = 0; l < hm->n_states && !hm->count_inc.empty(); ++l)
        if (hm->count_inc[l] != 0 && (l >= hm->silent_start || hm->count_inc[l] != 1)) { c->err = "forward pass: counted states must be emitting states with an increment of 1"; return STRQ_ERR_UNSUPPORTED; }
    if (vit_shape_of(hm->h) < 0) { c->err = "forward pass: model does not fit a compiled kernel"; return STRQ_ERR_UNSUPPORTED; }
    const std::vector<double>& lp = hm->fwd_logp.empty() ? hm->in_logp : hm->fwd_logp;
    std::vector<double> ew(hm->edge_csr.size(), 0.0), cw(hm->chain_csr.size(), 0.0);
    for (size_t i = 0; i < ew.size(); ++i) if (hm->edge_csr[i] >= 0) ew[i] = std::exp(lp[(size_t)hm->edge_csr[i]]);
    for (size_t i = 0; i < cw.size(); ++i) if (hm->chain_csr[i] >= 0) cw[i] = std::exp(lp[(size_t)hm->chain_csr[i]]);
    FwdModel F; std::memset(&F, 0, sizeof(F));
    Image im;
    const size_t o_e = im.put(ew), o_c = im.put(cw), o_m = im.put(&F, 1);
    if (hm->fwd_blob.reserve(im.lay.total()) != hipSuccess) { c->err = "out of device memory"; return STRQ_ERR_NOMEM; }
    void* d = hm->fwd_blob.p;
    F.vit = hm->dev; F.edge_w = Carve::at<const double>(d, o_e); F.chain_w = Carve::at<const double>(d, o_c); F.n_stages = hm->fwd_stages;
    if (hipMemcpy(d, im.host().data(), im.lay.total(), hipMemcpyHostToDevice) != hipSuccess) { c->err = "model upload failed"; return STRQ_ERR_DEVICE; }
    hm->fwd_dev = Carve::at<const FwdModel>(d, o_m);
    hm->post_dev = nullptr;          // (it points to the image this one replaced)
    return STRQ_OK;
}

// Transposed image of a model (PostModel): every entry of the forward image's edge rows is an in-edge of the cell that owns the row --
// turned round it is an out-edge of its source cell, with the same probability.  The out-edges of a cell keep the order of the rows
// (and of the lanes inside a row) they come from; the chain edges turn into chain_next_w.
int posterior_model(strq_ctx* c, HostModel* hm)
{
    if (const int rc = forward_model(c, hm)) return rc;
    if (hm->post_dev) return STRQ_OK;
    const VitModel& m = hm->h;
    const int epl = m.epl, spl = m.spl, dummy = m.n_cells - 1;
    if (hm->cell_state.size() != (size_t)m.n_cells) { c->err = "state posteriors: the model has no lane layout"; return STRQ_ERR_UNSUPPORTED; }
    std::vector<int32_t> cell_of((size_t)hm->n_states, -1);
    for (int cell = 0; cell < m.n_cells; ++cell) if (hm->cell_state[(size_t)cell] >= 0) cell_of[(size_t)hm->cell_state[(size_t)cell]] = cell;
    const std::vector<double>& lp = hm->fwd_logp.empty() ? hm->in_logp : hm->fwd_logp;
    std::vector<std::vector<std::pair<int32_t, double>>> outs((size_t)m.n_cells);
    auto turn = [&](int slot_base, int deg, int lane, int dst_cell) {
        for (int j = 0; j < deg; ++j) {
            const int e = hm->edge_csr[(size_t)(slot_base + j) * 64 + (size_t)lane];
            if (e < 0) continue;
            outs[(size_t)cell_of[(size_t)hm->in_src[(size_t)e]]].push_back({dst_cell, std::exp(lp[(size_t)e])});
        }
    };
    for (int s = 0; s < epl; ++s) for (int lane = 0; lane < 64; ++lane) turn(m.e_base[s], m.e_deg[s], lane, s * 64 + lane);
    for (int s = 0; s < spl; ++s) for (int lane = 0; lane < 64; ++lane) turn(m.s_base[s], m.s_deg[s], lane, epl * 64 + lane * spl + s);
    PostModel P; std::memset(&P, 0, sizeof(P));
    int rows = 0;
    for (int s = 0; s < epl; ++s) {
        size_t deg = 0;
        for (int lane = 0; lane < 64; ++lane) deg = std::max(deg, outs[(size_t)(s * 64 + lane)].size());
        P.oe_deg[s] = (int32_t)deg; P.oe_base[s] = rows; rows += (int)deg;
    }
    for (int s = 0; s < spl; ++s) {
        size_t deg = 0;
        for (int lane = 0; lane < 64; ++lane) deg = std::max(deg, outs[(size_t)(epl * 64 + lane * spl + s)].size());
        P.os_deg[s] = (int32_t)deg; P.os_base[s] = rows; rows += (int)deg;
    }
    std::vector<int32_t> dst((size_t)std::max(rows, 1) * 64, dummy); std::vector<double> w((size_t)std::max(rows, 1) * 64, 0.0);
    auto fill = [&](int base, int lane, int cell) {
        const auto& o = outs[(size_t)cell];
        for (size_t j = 0; j < o.size(); ++j) { dst[((size_t)base + j) * 64 + (size_t)lane] = o[j].first; w[((size_t)base + j) * 64 + (size_t)lane] = o[j].second; }
    };
    for (int s = 0; s < epl; ++s) for (int lane = 0; lane < 64; ++lane) fill(P.oe_base[s], lane, s * 64 + lane);
    for (int s = 0; s < spl; ++s) for (int lane = 0; lane < 64; ++lane) fill(P.os_base[s], lane, epl * 64 + lane * spl + s);
    // the chain edge INTO position p (slot p % spl of lane p / spl) leaves position p - 1
    std::vector<double> nw((size_t)spl * 64, 0.0);
    for (int i = 0; i < spl * 64; ++i) {
        if (hm->chain_csr[(size_t)i] < 0) continue;
        const int p = (i % 64) * spl + i / 64 - 1;
        if (p < 0) { c->err = "state posteriors: chain edge into the first chain position"; return STRQ_ERR_UNSUPPORTED; }
        nw[(size_t)(p % spl) * 64 + (size_t)(p / spl)] = std::exp(lp[(size_t)hm->chain_csr[(size_t)i]]);
    }
    Image im;
    const size_t o_d = im.put(dst), o_w = im.put(w), o_n = im.put(nw), o_m = im.put(&P, 1);
    if (hm->post_blob.reserve(im.lay.total()) != hipSuccess) { c->err = "out of device memory"; return STRQ_ERR_NOMEM; }
    void* d = hm->post_blob.p;
    P.fwd = hm->fwd_dev; P.out_dst = Carve::at<const int32_t>(d, o_d); P.out_w = Carve::at<const double>(d, o_w); P.chain_next_w = Carve::at<const double>(d, o_n);
    if (hipMemcpy(d, im.host().data(), im.lay.total(), hipMemcpyHostToDevice) != hipSuccess) { c->err = "model upload failed"; return STRQ_ERR_DEVICE; }
    hm->post_dev = Carve::at<const PostModel>(d, o_m);
    return STRQ_OK;
}

}  // namespace strq

int strq::viterbi_launch_status(int vrc) { return vrc == 0 ? STRQ_OK : (vrc == 2 || vrc == 3) ? STRQ_ERR_UNSUPPORTED : STRQ_ERR_DEVICE; }

extern "C" {

int strq_model_create(strq_ctx* c, int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                      const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                      const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                      const int32_t* count_inc, const int32_t* state_tag,
                      const int32_t* hint_slot, const int32_t* hint_lane, int32_t* model_id)
{
    strq::CtxScope scope_(c);
    if (!c) return STRQ_ERR_ARG;
    if (!in_ptr || !in_src || !in_logp || !emis_kind || !emis_a || !emis_b || !emis_c || !model_id) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    STRQ_HIP(c, hipSetDevice(c->device));
    HostModel* hm = nullptr;
    int rc = build_vit_model(c, n_states, silent_start, start, end, in_ptr, in_src, in_logp, emis_kind, emis_a, emis_b, emis_c, count_inc, state_tag, hint_slot, hint_lane, &hm);
    if (rc == STRQ_ERR_UNSUPPORTED)      // no lane layout: the model runs on the general (slow) kernel
        rc = build_vit_model_csr(c, n_states, silent_start, start, end, in_ptr, in_src, in_logp, emis_kind, emis_a, emis_b, emis_c, count_inc, state_tag, &hm);
    if (rc) return rc;
    hm->n_states = n_states; hm->silent_start = silent_start; hm->start = start; hm->end = end;
    hm->in_ptr.assign(in_ptr, in_ptr + n_states + 1);
    hm->in_src.assign(in_src, in_src + in_ptr[n_states]); hm->in_logp.assign(in_logp, in_logp + in_ptr[n_states]);
    hm->emis_kind.assign(emis_kind, emis_kind + silent_start); hm->emis_a.assign(emis_a, emis_a + silent_start);
    hm->emis_b.assign(emis_b, emis_b + silent_start); hm->emis_c.assign(emis_c, emis_c + silent_start);
    if (count_inc) hm->count_inc.assign(count_inc, count_inc + n_states);
    if (state_tag) hm->state_tag.assign(state_tag, state_tag + n_states);
    c->models.push_back(hm);
    *model_id = (int32_t)c->models.size() - 1;
    return STRQ_OK;
}

// Host-only (no context, no device): the tables strq_model_set_positions would upload, for tests of the layout.
// out_lp[G2_ROWS * 64], out_own[6 * 64], out_meta[10] = {bc_slot0, bc_lane0, bc_slot1, bc_lane1, start_slot, start_lane, end_slot, end_lane, hub_mask lo, hub_mask hi}.
int strq_debug_g2_layout(int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                         const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                         const int32_t* emis_kind, const int32_t* count_inc, const int32_t* kind, const int32_t* pos,
                         double* out_lp, int32_t* out_own, int32_t* out_meta, char* why, int32_t why_len)
{
    HostModel hm;
    hm.n_states = n_states; hm.silent_start = silent_start; hm.start = start; hm.end = end;
    hm.in_ptr.assign(in_ptr, in_ptr + n_states + 1); hm.in_src.assign(in_src, in_src + in_ptr[n_states]); hm.in_logp.assign(in_logp, in_logp + in_ptr[n_states]);
    hm.emis_kind.assign(emis_kind, emis_kind + silent_start); hm.emis_a.assign(silent_start, 0.0); hm.emis_b.assign(silent_start, 0.0); hm.emis_c.assign(silent_start, 0.0);
    if (count_inc) hm.count_inc.assign(count_inc, count_inc + n_states);
    for (int e = 0; e < silent_start; ++e) if ((kind[e] != 0 && kind[e] != 1) || pos[e] < 0 || pos[e] > 125) { if (why && why_len > 0) snprintf(why, why_len, "an emitting state has no position"); return STRQ_ERR_UNSUPPORTED; }
    for (int e = 0; e < silent_start; ++e) if (kind[e] == 1 && emis_kind[e] == 1) { if (why && why_len > 0) snprintf(why, why_len, "an insert-type state has a Normal emission"); return STRQ_ERR_UNSUPPORTED; }
    G2Host L; std::string w;
    if (!g2_layout(&hm, kind, pos, L, w)) { if (why && why_len > 0) snprintf(why, why_len, "%s", w.c_str()); return STRQ_ERR_UNSUPPORTED; }
    std::memcpy(out_lp, L.lp.data(), L.lp.size() * 8); std::memcpy(out_own, L.own.data(), L.own.size() * 4);
    const int32_t meta[10] = {L.G.bc_slot[0], L.G.bc_lane[0], L.G.bc_slot[1], L.G.bc_lane[1], L.G.start_slot, L.G.start_lane, L.G.end_slot, L.G.end_lane,
                              (int32_t)(uint32_t)L.G.hub_mask, (int32_t)(uint32_t)(L.G.hub_mask >> 32)};
    std::memcpy(out_meta, meta, sizeof(meta));
    return STRQ_OK;
}

// Host-only (no context, no device): which kernel shape strq_model_create would put this model on and what its layout looks like.
// out[48]: [0..4] the shape id of a launch of mode 0..4 (vit_shape_of, VIT_SHAPE_SS included; -1: none), [5..9] 1 where the product
// has a launch of that mode for the model, [10] epl, [11] spl, [12..19] e_deg, [20..27] s_deg, [28..35] e_flat, [36] single_stage,
// [37] silent_counted, [38] rec_state, [39..40] unit_state, [41] 1 = the general kernel (no lane layout), the rest 0.
int strq_debug_viterbi_plan(int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                            const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                            const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                            const int32_t* count_inc, const int32_t* state_tag,
                            const int32_t* hint_slot, const int32_t* hint_lane, int32_t* out, char* why, int32_t why_len)
{
    auto say = [&](const char* w) { if (why && why_len > 0) snprintf(why, why_len, "%s", w); };
    if (!in_ptr || !in_src || !in_logp || !emis_kind || !emis_a || !emis_b || !emis_c || !out) { say("bad argument"); return STRQ_ERR_ARG; }
    VitPlan P; const char* w = nullptr;
    int rc = plan_vit_model(n_states, silent_start, start, end, in_ptr, in_src, in_logp, emis_kind, emis_a, emis_b, emis_c, count_inc, state_tag,
                            hint_slot, hint_lane, P, &w);
    if (rc == STRQ_ERR_UNSUPPORTED) {          // as strq_model_create: the general kernel takes what no lane layout holds
        if (n_states > VIT_CSR_MAX_STATES) { say("model too large: more than 4096 states"); return STRQ_ERR_UNSUPPORTED; }
        std::memset(&P.m, 0, sizeof(P.m));
        P.m.csr = 1; P.m.rec_state = -1; P.m.unit_state[0] = P.m.unit_state[1] = -1;
        rc = STRQ_OK;
    }
    if (rc) { say(w ? w : "?"); return rc; }
    const VitModel& m = P.m;
    std::fill(out, out + 48, 0);
    const int shape = vit_shape_of(m);
    for (int mode = VIT_COUNT; mode <= VIT_UNIT; ++mode) {
        out[mode] = shape;
        out[5 + mode] = (vit_mode_ok(shape, mode) && (mode != VIT_HUB || m.rec_state >= 0) && (mode != VIT_UNIT || vit_unit_ok(m, shape))) ? 1 : 0;
    }
    out[10] = m.epl; out[11] = m.spl;
    for (int i = 0; i < 8; ++i) { out[12 + i] = m.e_deg[i]; out[20 + i] = m.s_deg[i]; out[28 + i] = m.e_flat[i]; }
    out[36] = m.single_stage; out[37] = m.silent_counted; out[38] = m.rec_state; out[39] = m.unit_state[0]; out[40] = m.unit_state[1]; out[41] = m.csr;
    return STRQ_OK;
}

int strq_model_set_positions(strq_ctx* c, int32_t model_id, const int32_t* kind, const int32_t* pos)
{
    STRQ_ENTER(c);
    if (model_id < 0 || model_id >= (int32_t)c->models.size() || !c->models[model_id] || !kind || !pos) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    // a detect sub-batch whose Viterbi launches are not yet queued points to the model's present device image through its tasks
    { const int rc = detect_drain(c); if (rc) return rc; }
    return build_vit_g2(c, c->models[model_id], kind, pos);
}

// One window of a model: T observations at `sig` (with an affine kind the caller adds the constants); everything else zero
static VitTask plain_task(const HostModel* hm, const void* sig, int64_t T, int32_t src_kind = VIT_SRC_F64)
{
    VitTask t; std::memset(&t, 0, sizeof(t));
    t.model = hm->dev; t.sig = sig; t.T = T; t.src_kind = src_kind;
    return t;
}

// The windows of a standalone entry point.  check_windows: the model, at most max_seq windows (0: any number), x_off from 0 up and never
// decreasing, observations where there are any.  upload_windows (n_seq > 0, checked): the observations into c->vit_x, a float64 task each.
static int check_windows(strq_ctx* c, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off, int64_t max_seq)
{
    if (model_id < 0 || model_id >= (int32_t)c->models.size() || !c->models[model_id] || n_seq < 0 || (max_seq && n_seq > max_seq) || (n_seq > 0 && !x_off)) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (n_seq == 0) return STRQ_OK;
    if (x_off[n_seq] < 0 || (x_off[n_seq] > 0 && !x)) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    for (int64_t i = 0; i < n_seq; ++i) if (x_off[i + 1] < x_off[i] || x_off[i] < 0) { c->err = "bad argument (x_off must not decrease)"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}
static int upload_windows(strq_ctx* c, const HostModel* hm, int64_t n_seq, const double* x, const int64_t* x_off, std::vector<VitTask>& tasks)
{
    const int64_t tot = x_off[n_seq];
    STRQ_HIP(c, c->vit_x.reserve((size_t)tot * 8 + 64));
    if (tot) STRQ_HIP(c, hipMemcpyAsync(c->vit_x.p, x, (size_t)tot * 8, hipMemcpyHostToDevice, c->stream));
    tasks.resize((size_t)n_seq);
    for (int64_t i = 0; i < n_seq; ++i) tasks[(size_t)i] = plain_task(hm, c->vit_x.as<double>() + x_off[i], x_off[i + 1] - x_off[i]);
    return STRQ_OK;
}

// strq_viterbi_batch, strq_viterbi, the count decode of strq_viterbi_state_stats; `keep` (or null) takes the tasks, input order, no bp
static int viterbi_batch(strq_ctx* c, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off, int64_t max_seq,
                         double* logp, int64_t* counted, int32_t* status, int32_t* paths, std::vector<VitTask>* keep)
{
    if (n_seq > 0 && !x) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (const int rc = check_windows(c, model_id, n_seq, x, x_off, max_seq)) return rc;
    if (n_seq == 0) return STRQ_OK;
    HostModel* hm = c->models[model_id];
    hipStream_t st = c->stream;
    const int64_t tot = x_off[n_seq];
    const int n = hm->h.n_states;
    std::vector<VitTask> in;
    if (const int rc = upload_windows(c, hm, n_seq, x, x_off, in)) return rc;
    Carve lay;
    const size_t o_tasks = lay.add<VitTask>((size_t)n_seq), o_res = lay.add<VitResult>((size_t)n_seq), o_paths = lay.add<int32_t*>((size_t)n_seq);
    STRQ_HIP(c, c->vit_tasks.reserve(lay.total()));
    VitTask* d_tasks = Carve::at<VitTask>(c->vit_tasks.p, o_tasks); VitResult* d_res = Carve::at<VitResult>(c->vit_tasks.p, o_res);
    int32_t** d_paths = Carve::at<int32_t*>(c->vit_tasks.p, o_paths);
    size_t bp_cells = 0;
    for (int64_t i = 0; paths && i < n_seq; ++i) bp_cells += (size_t)(in[(size_t)i].T + 1) * n;
    if (paths) { STRQ_HIP(c, c->vit_bp.reserve(bp_cells * 2 + 64)); STRQ_HIP(c, c->vit_path.reserve((size_t)tot * 4 + 64)); }
    std::vector<int64_t> order(n_seq);          // longest first
    for (int64_t i = 0; i < n_seq; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return in[(size_t)a].T > in[(size_t)b].T; });
    std::vector<VitTask> tasks(n_seq); std::vector<int32_t*> hp(n_seq, nullptr);
    size_t bp_off = 0;
    for (int64_t pos = 0; pos < n_seq; ++pos) {
        const int64_t i = order[pos];
        VitTask& t = tasks[pos] = in[(size_t)i];
        if (paths) { t.bp = c->vit_bp.as<uint16_t>() + bp_off; bp_off += (size_t)(t.T + 1) * n; hp[pos] = c->vit_path.as<int32_t>() + x_off[i]; }
    }
    STRQ_HIP(c, hipMemcpyAsync(d_tasks, tasks.data(), (size_t)n_seq * sizeof(VitTask), hipMemcpyHostToDevice, st));
    if (paths) STRQ_HIP(c, hipMemcpyAsync(d_paths, hp.data(), (size_t)n_seq * 8, hipMemcpyHostToDevice, st));
    if (const int qrc = reset_queue_heads(c, st)) return qrc;
    STRQ_HIP(c, hipEventRecord(c->ev[0], st));
    const int shape = vit_shape_for(hm->h, paths ? VIT_BACKPTR : VIT_COUNT);
    if (shape < 0) { c->err = "model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
    int rc = launch_viterbi(st, shape, hm->h.n_cells, d_tasks, d_res, (int)n_seq, c->queue.as<int>(), c->n_cu, paths ? VIT_BACKPTR : VIT_COUNT);
    if (rc) { c->err = "viterbi launch failed"; return viterbi_launch_status(rc); }
    STRQ_HIP(c, hipEventRecord(c->ev[1], st));
    if (paths && launch_vit_traceback(st, d_tasks, d_res, d_paths, (int)n_seq)) { c->err = "traceback launch failed"; return STRQ_ERR_DEVICE; }
    STRQ_HIP(c, hipEventRecord(c->ev[2], st));
    std::vector<VitResult> res(n_seq);
    STRQ_HIP(c, hipMemcpyAsync(res.data(), d_res, (size_t)n_seq * sizeof(VitResult), hipMemcpyDeviceToHost, st));
    if (paths) STRQ_HIP(c, hipMemcpyAsync(paths, c->vit_path.p, (size_t)tot * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    for (int64_t pos = 0; pos < n_seq; ++pos) {
        const int64_t i = order[pos];
        if (logp) logp[i] = res[pos].logp;
        if (counted) counted[i] = res[pos].counted;
        if (status) status[i] = res[pos].status;
    }
    std::fill(c->timing, c->timing + 8, 0.0f);
    STRQ_HIP(c, hipEventElapsedTime(&c->timing[0], c->ev[0], c->ev[1]));
    STRQ_HIP(c, hipEventElapsedTime(&c->timing[1], c->ev[1], c->ev[2]));
    c->timing[3] = c->timing[0] + c->timing[1];
    if (keep) keep->swap(in);
    return STRQ_OK;
}

int strq_viterbi_batch(strq_ctx* c, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                       double* logp, int64_t* counted, int32_t* status, int32_t* paths)
{
    STRQ_ENTER(c);
    return viterbi_batch(c, model_id, n_seq, x, x_off, 0, logp, counted, status, paths, nullptr);
}

// The two test hooks below: one launch_viterbi of `mode` over the windows, on buffers of the call's own (strique_hip.h).  src_kind
// VIT_SRC_F64: x holds the observations themselves, consts is not read; the affine kinds: x holds int16 / float64 samples and
// consts six doubles per window (c1, h1, h2, c2, lo, hi) -- what window_task() (scan_kernels.h) gives the pipeline's windows.
// tracts: the wide-payload count launch of strq_viterbi_tracts (sorted order, never the register-resident image).
static int debug_viterbi_launch(strq_ctx* c, int32_t model_id, int32_t mode, int64_t n_seq, int32_t src_kind, const void* x, const int64_t* x_off,
                                const double* consts, bool tracts, double* logp, int64_t* counted, int32_t* status, uint32_t* dbg,
                                void* records, const int64_t* rec_off, int64_t* tract_counts, int32_t* launched)
{
    const char* bad = "bad argument";
    if (model_id < 0 || model_id >= (int32_t)c->models.size() || !c->models[model_id] || n_seq < 1 || n_seq > 8192 || !x_off || !launched || x_off[0] != 0) { c->err = bad; return STRQ_ERR_ARG; }
    if (mode != VIT_COUNT && mode != VIT_MARK && mode != VIT_HUB && mode != VIT_UNIT) { c->err = "bad argument (mode: count, mark, hub or unit)"; return STRQ_ERR_ARG; }
    const bool rec = mode == VIT_HUB || mode == VIT_UNIT;
    if (rec && (!records || !rec_off || rec_off[0] != 0)) { c->err = bad; return STRQ_ERR_ARG; }
    for (int64_t i = 0; i < n_seq; ++i) {
        const int64_t T = x_off[i + 1] - x_off[i];
        if (T < 0 || T >= ((int64_t)1 << 28)) { c->err = "bad argument (window lengths)"; return STRQ_ERR_ARG; }
        // HUB: T + 1 records of 8 bytes; UNIT: 2 T records of 4 bytes
        if (rec && rec_off[i + 1] - rec_off[i] != (mode == VIT_HUB ? 8 * (T + 1) : 8 * T)) { c->err = "bad argument (rec_off: the bytes of every window's records)"; return STRQ_ERR_ARG; }
    }
    const int64_t tot = x_off[n_seq];
    if (tot > 0 && !x) { c->err = bad; return STRQ_ERR_ARG; }
    const size_t esz = src_kind == VIT_SRC_I16_AFFINE ? 2 : 8;
    if (src_kind != VIT_SRC_F64) {
        if (!consts) { c->err = bad; return STRQ_ERR_ARG; }
        for (int64_t i = 0; i < n_seq; ++i) {
            const double* k = consts + 6 * i;
            if (k[1] == 0.0 || !(k[4] <= k[5])) { c->err = "bad argument (window constants: h1 must not be 0, lo must not exceed hi)"; return STRQ_ERR_ARG; }
        }
        // the branch-free emission code has no test for a missing observation: samples are numbers
        if (src_kind == VIT_SRC_F64_AFFINE)
            for (int64_t i = 0; i < tot; ++i) { const double v = static_cast<const double*>(x)[i]; if (v != v) { c->err = "bad argument (a float64 sample is not a number)"; return STRQ_ERR_ARG; } }
    }
    HostModel* hm = c->models[model_id];
    if (tracts && (mode != VIT_COUNT || !hm->h.tract_inc || !tract_counts)) { c->err = "bad argument (tract payload: a count launch of a model with tracts)"; return STRQ_ERR_ARG; }
    const int shape = tracts ? vit_shape_of(hm->h) : vit_shape_for(hm->h, (VitMode)mode);
    launched[0] = shape;
    if (shape < 0 || !vit_mode_ok(shape, mode) || (mode == VIT_HUB && hm->h.rec_state < 0) || (mode == VIT_UNIT && !vit_unit_ok(hm->h, shape))) {
        c->err = "the model has no launch of this decode mode"; return STRQ_ERR_UNSUPPORTED;
    }
    hipStream_t st = c->stream;
    const size_t rec_bytes = rec ? (size_t)rec_off[n_seq] : 0;
    DevBuf b_x, b_tasks, b_res, b_rec, b_queue, b_order;
    STRQ_HIP(c, b_x.reserve((size_t)tot * esz + 64)); STRQ_HIP(c, b_tasks.reserve((size_t)n_seq * sizeof(VitTask)));
    STRQ_HIP(c, b_res.reserve((size_t)n_seq * sizeof(VitResult))); STRQ_HIP(c, b_rec.reserve(rec_bytes + 64)); STRQ_HIP(c, b_queue.reserve(64));
    if (tracts) STRQ_HIP(c, b_order.reserve((size_t)n_seq * sizeof(int) + 64));
    std::vector<VitTask> tasks((size_t)n_seq);
    for (int64_t i = 0; i < n_seq; ++i) {
        VitTask& t = tasks[(size_t)i];
        t = plain_task(hm, b_x.as<char>() + (size_t)x_off[i] * esz, x_off[i + 1] - x_off[i], src_kind);
        if (src_kind != VIT_SRC_F64) { const double* k = consts + 6 * i; t.c1 = k[0]; t.h1 = k[1]; t.h2 = k[2]; t.c2 = k[3]; t.lo = k[4]; t.hi = k[5]; }
        if (rec) t.bp = reinterpret_cast<uint16_t*>(b_rec.as<char>() + rec_off[i]);
    }
    if (tot) STRQ_HIP(c, hipMemcpyAsync(b_x.p, x, (size_t)tot * esz, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(b_tasks.p, tasks.data(), (size_t)n_seq * sizeof(VitTask), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemsetAsync(b_res.p, 0, (size_t)n_seq * sizeof(VitResult), st));
    STRQ_HIP(c, hipMemsetAsync(b_rec.p, 0, rec_bytes + 64, st));
    STRQ_HIP(c, hipMemsetAsync(b_queue.p, 0, 64, st));
    if (tracts && launch_vit_sort(st, b_tasks.as<VitTask>(), (int)n_seq, b_order.as<int>())) { (void)hipStreamSynchronize(st); c->err = "sort launch failed"; return STRQ_ERR_DEVICE; }
    const int lrc = launch_viterbi(st, shape, hm->h.n_cells, b_tasks.as<VitTask>(), b_res.as<VitResult>(), (int)n_seq, b_queue.as<int>(), c->n_cu, (VitMode)mode,
                                   tracts ? b_order.as<int>() : nullptr, 0, tracts);
    if (lrc) { (void)hipStreamSynchronize(st); c->err = "viterbi launch failed"; return viterbi_launch_status(lrc); }
    std::vector<VitResult> res((size_t)n_seq);
    STRQ_HIP(c, hipMemcpyAsync(res.data(), b_res.p, (size_t)n_seq * sizeof(VitResult), hipMemcpyDeviceToHost, st));
    if (rec_bytes) STRQ_HIP(c, hipMemcpyAsync(records, b_rec.p, rec_bytes, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    for (int64_t i = 0; i < n_seq; ++i) {
        const VitResult& r = res[(size_t)i];
        if (logp) logp[i] = r.logp;
        if (counted) counted[i] = r.counted;
        if (status) status[i] = r.status;
        if (dbg) std::memcpy(dbg + 4 * i, r.dbg, sizeof(r.dbg));
        if (tracts) {          // as strq_viterbi_tracts unpacks them
            const uint64_t pay = r.status == 0 ? (uint64_t)r.counted : 0;
            for (int j = 0; j < VIT_TRACTS_MAX; ++j) tract_counts[3 * i + j] = vit_tract_count(pay, j);
        }
    }
    return STRQ_OK;
}

int strq_debug_viterbi_mode(strq_ctx* c, int32_t model_id, int32_t mode, int64_t n_seq, const double* x, const int64_t* x_off,
                            double* logp, int64_t* counted, int32_t* status, uint32_t* dbg, void* records, const int64_t* rec_off,
                            int32_t* launched)
{
    STRQ_ENTER(c);
    return debug_viterbi_launch(c, model_id, mode, n_seq, VIT_SRC_F64, x, x_off, nullptr, false, logp, counted, status, dbg, records, rec_off, nullptr, launched);
}

int strq_debug_viterbi_sourced(strq_ctx* c, int32_t model_id, int32_t mode, int32_t src_kind, int32_t tracts, int64_t n_seq,
                               const void* samples, const int64_t* x_off, const double* consts,
                               double* logp, int64_t* counted, int32_t* status, uint32_t* dbg, void* records, const int64_t* rec_off,
                               int64_t* tract_counts, int32_t* launched)
{
    STRQ_ENTER(c);
    if (src_kind != VIT_SRC_F64_AFFINE && src_kind != VIT_SRC_I16_AFFINE) { c->err = "bad argument (source kind: 1 float64 samples, 2 int16 samples)"; return STRQ_ERR_ARG; }
    return debug_viterbi_launch(c, model_id, mode, n_seq, src_kind, samples, x_off, consts, tracts != 0, logp, counted, status, dbg, records, rec_off, tract_counts, launched);
}

int strq_model_set_forward_logp(strq_ctx* c, int32_t model_id, const double* in_logp_sum)
{
    STRQ_ENTER(c);
    if (model_id < 0 || model_id >= (int32_t)c->models.size() || !c->models[model_id] || !in_logp_sum) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    HostModel* hm = c->models[model_id];
    for (size_t e = 0; e < hm->in_logp.size(); ++e)
        if (!(in_logp_sum[e] >= hm->in_logp[e])) { c->err = "the summed log-probability of an edge is below its largest term"; return STRQ_ERR_ARG; }
    // a detect sub-batch in flight may be about to run its forward pass on the present image
    { const int rc = detect_drain(c); if (rc) return rc; }
    hm->fwd_logp.assign(in_logp_sum, in_logp_sum + hm->in_logp.size());
    hm->fwd_dev = nullptr; hm->post_dev = nullptr;          // built again on the next forward pass
    return STRQ_OK;
}

int strq_forward_batch(strq_ctx* c, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off, const int64_t* c0,
                       double* log_lik, double* visits_mean, double* visits_var, int32_t* status)
{
    STRQ_ENTER(c);
    if (const int rc = check_windows(c, model_id, n_seq, x, x_off, 8192)) return rc;
    if (n_seq == 0) return STRQ_OK;
    HostModel* hm = c->models[model_id];
    if (const int rc = forward_model(c, hm)) return rc;
    hipStream_t st = c->stream;
    std::vector<VitTask> tasks;
    if (const int rc = upload_windows(c, hm, n_seq, x, x_off, tasks)) return rc;
    Carve lay;
    const size_t o_tasks = lay.add<VitTask>((size_t)n_seq), o_res = lay.add<FwdResult>((size_t)n_seq), o_fm = lay.add<const FwdModel*>((size_t)n_seq),
                 o_c0 = lay.add<int64_t>((size_t)n_seq), o_order = lay.add<int>((size_t)n_seq);
    STRQ_HIP(c, c->vit_tasks.reserve(lay.total() + 64));
    void* tb = c->vit_tasks.p;
    VitTask* d_tasks = Carve::at<VitTask>(tb, o_tasks); FwdResult* d_res = Carve::at<FwdResult>(tb, o_res); const FwdModel** d_fm = Carve::at<const FwdModel*>(tb, o_fm);
    int64_t* d_c0 = Carve::at<int64_t>(tb, o_c0); int* d_order = Carve::at<int>(tb, o_order);
    std::vector<const FwdModel*> fms((size_t)n_seq, hm->fwd_dev); std::vector<int64_t> c0v((size_t)n_seq, 0);
    if (c0) c0v.assign(c0, c0 + n_seq);
    STRQ_HIP(c, hipMemcpyAsync(d_tasks, tasks.data(), (size_t)n_seq * sizeof(VitTask), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_fm, fms.data(), (size_t)n_seq * 8, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_c0, c0v.data(), (size_t)n_seq * 8, hipMemcpyHostToDevice, st));
    if (const int qrc = reset_queue_heads(c, st)) return qrc;
    if (launch_vit_sort(st, d_tasks, (int)n_seq, d_order)) { c->err = "forward pass: sort launch failed"; return STRQ_ERR_DEVICE; }
    int every = 1;
    if (const char* e = strq::opt("STRQ_FWD_RESCALE_EVERY")) { const int v = atoi(e); if (v >= 1) every = v; }
    const int lrc = launch_forward(st, vit_shape_of(hm->h), hm->h.n_cells, d_tasks, d_fm, d_c0, d_res, (int)n_seq, c->queue.as<int>(), c->n_cu, d_order, every);
    if (lrc) { c->err = lrc == 2 ? "forward pass: no kernel for this model's layout" : "forward launch failed"; return lrc == 2 ? STRQ_ERR_UNSUPPORTED : STRQ_ERR_DEVICE; }
    std::vector<FwdResult> res(n_seq);
    STRQ_HIP(c, hipMemcpyAsync(res.data(), d_res, (size_t)n_seq * sizeof(FwdResult), hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    for (int64_t i = 0; i < n_seq; ++i) {
        double ll, mean, var;
        const int s = fwd_finish(res[i], c0v[(size_t)i], &ll, &mean, &var);
        if (log_lik) log_lik[i] = ll;
        if (visits_mean) visits_mean[i] = mean;
        if (visits_var) visits_var[i] = var;
        if (status) status[i] = s;
    }
    return STRQ_OK;
}

int strq_model_set_tracts(strq_ctx* c, int32_t model_id, int32_t n_tracts, const int32_t* tract_of)
{
    STRQ_ENTER(c);
    if (model_id < 0 || model_id >= (int32_t)c->models.size() || !c->models[model_id] || !tract_of) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (n_tracts < 1 || n_tracts > VIT_TRACTS_MAX) { c->err = "bad argument (between 1 and 3 tracts)"; return STRQ_ERR_ARG; }
    HostModel* hm = c->models[model_id];
    const int n = hm->n_states;
    std::vector<uint64_t> inc((size_t)n + 1, 0);
    for (int l = 0; l < n; ++l) {
        const int j = tract_of[l];
        if (j == -1) continue;
        if (j < 0 || j >= n_tracts) { c->err = "bad argument (tract_of: -1 or a tract below n_tracts)"; return STRQ_ERR_ARG; }
        if (l >= hm->silent_start || hm->count_inc.empty() || hm->count_inc[l] != 1) { c->err = "a state with a tract must be an emitting state with count_inc 1"; return STRQ_ERR_ARG; }
        inc[(size_t)l] = (uint64_t)1 << (VIT_TRACT_BITS * j);
    }
    // a detect sub-batch in flight points to the model's present device image through its tasks
    { const int rc = detect_drain(c); if (rc) return rc; }
    STRQ_HIP(c, hipStreamSynchronize(c->stream));
    STRQ_HIP(c, hm->tract_blob.reserve(inc.size() * 8));
    STRQ_HIP(c, hipMemcpy(hm->tract_blob.p, inc.data(), inc.size() * 8, hipMemcpyHostToDevice));
    hm->h.tract_inc = hm->tract_blob.as<const uint64_t>(); hm->n_tracts = n_tracts;
    if (hipMemcpy(const_cast<VitModel*>(hm->dev), &hm->h, sizeof(VitModel), hipMemcpyHostToDevice) != hipSuccess) {
        hm->h.tract_inc = nullptr; hm->n_tracts = 0; c->err = "model upload failed"; return STRQ_ERR_DEVICE;
    }
    return STRQ_OK;
}

// strq_viterbi_tracts and strq_viterbi_tract_positions: the tract decode of the windows; `keep` (or null) takes the tasks as they were
// launched and their results
static int viterbi_tracts(strq_ctx* c, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                          double* logp, int64_t* counts, int32_t* status, std::pair<std::vector<VitTask>, std::vector<VitResult>>* keep)
{
    if (const int rc = check_windows(c, model_id, n_seq, x, x_off, 8192)) return rc;
    HostModel* hm = c->models[model_id];
    if (!hm->h.tract_inc) { c->err = "the model has no tracts (strq_model_set_tracts)"; return STRQ_ERR_ARG; }
    const int shape = vit_shape_of(hm->h);          // never the register-resident image: it has one loop
    if (n_seq == 0) return STRQ_OK;
    if (shape < 0) { c->err = "model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
    hipStream_t st = c->stream;
    std::vector<VitTask> tasks;
    if (const int rc = upload_windows(c, hm, n_seq, x, x_off, tasks)) return rc;
    Carve lay;
    const size_t o_tasks = lay.add<VitTask>((size_t)n_seq), o_res = lay.add<VitResult>((size_t)n_seq), o_order = lay.add<int>((size_t)n_seq);
    STRQ_HIP(c, c->vit_tasks.reserve(lay.total() + 64));
    VitTask* d_tasks = Carve::at<VitTask>(c->vit_tasks.p, o_tasks); VitResult* d_res = Carve::at<VitResult>(c->vit_tasks.p, o_res);
    int* d_order = Carve::at<int>(c->vit_tasks.p, o_order);
    STRQ_HIP(c, hipMemcpyAsync(d_tasks, tasks.data(), (size_t)n_seq * sizeof(VitTask), hipMemcpyHostToDevice, st));
    if (const int qrc = reset_queue_heads(c, st)) return qrc;
    if (launch_vit_sort(st, d_tasks, (int)n_seq, d_order)) { c->err = "tract decode: sort launch failed"; return STRQ_ERR_DEVICE; }
    const int lrc = launch_viterbi(st, shape, hm->h.n_cells, d_tasks, d_res, (int)n_seq, c->queue.as<int>(), c->n_cu, VIT_COUNT, d_order, 0, true);
    if (lrc) { (void)hipStreamSynchronize(st); c->err = "viterbi launch failed"; return viterbi_launch_status(lrc); }
    c->tract_shape_last = shape;
    std::vector<VitResult> res((size_t)n_seq);
    STRQ_HIP(c, hipMemcpyAsync(res.data(), d_res, (size_t)n_seq * sizeof(VitResult), hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    for (int64_t i = 0; i < n_seq; ++i) {
        const VitResult& r = res[(size_t)i];
        const uint64_t pay = r.status == 0 ? (uint64_t)r.counted : 0;
        if (logp) logp[i] = r.logp;
        if (status) status[i] = r.status;
        if (counts) for (int j = 0; j < VIT_TRACTS_MAX; ++j) counts[3 * i + j] = vit_tract_count(pay, j);
    }
    if (keep) { keep->first.swap(tasks); keep->second.swap(res); }
    return STRQ_OK;
}

int strq_viterbi_tracts(strq_ctx* c, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                        double* logp, int64_t* counts, int32_t* status)
{
    STRQ_ENTER(c);
    return viterbi_tracts(c, model_id, n_seq, x, x_off, logp, counts, status, nullptr);
}

int strq_viterbi_tract_positions(strq_ctx* c, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                                 double* logp, int64_t* counts, int32_t* status, int64_t* pos_off, int64_t* pool, int64_t pool_cap)
{
    STRQ_ENTER(c);
    if (!pos_off || pool_cap < 0 || (pool_cap > 0 && !pool)) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    std::pair<std::vector<VitTask>, std::vector<VitResult>> kept;
    std::vector<int32_t> st_own((size_t)std::max<int64_t>(n_seq, 0));
    if (const int rc = viterbi_tracts(c, model_id, n_seq, x, x_off, logp, counts, st_own.data(), &kept)) return rc;
    pos_off[0] = 0;
    if (n_seq == 0) return STRQ_OK;
    const HostModel* hm = c->models[model_id];
    std::vector<TractPosWindow> pw; std::vector<int64_t> win;
    for (int64_t i = 0; i < n_seq; ++i) {
        const VitResult& r = kept.second[(size_t)i];
        if (r.status != 0) continue;
        TractPosWindow w; w.task = kept.first[(size_t)i]; w.hm = hm; w.base = 0;
        for (int j = 0; j < 3; ++j) w.n[j] = vit_tract_count((uint64_t)r.counted, j);
        pw.push_back(w); win.push_back(i);
    }
    TractPosOut po;
    if (!pw.empty()) { if (const int rc = tract_positions(c, pw, po, nullptr)) return rc; }
    std::vector<const std::vector<int64_t>*> of((size_t)n_seq * 3, nullptr);
    for (size_t k = 0; k < pw.size(); ++k) {
        if (po.status[k] == 2) st_own[(size_t)win[k]] = 4;
        for (int j = 0; j < 3; ++j) of[3 * (size_t)win[k] + (size_t)j] = &po.pos[3 * k + (size_t)j];
    }
    if (status) std::memcpy(status, st_own.data(), (size_t)n_seq * 4);
    const int64_t done = pack_ragged(3 * n_seq, pos_off, pool != nullptr, pool_cap, [&](int64_t i) { return of[(size_t)i] ? (int64_t)of[(size_t)i]->size() : 0; },
                                     [&](int64_t i, int64_t pos) { if (of[(size_t)i] && !of[(size_t)i]->empty()) std::memcpy(pool + pos, of[(size_t)i]->data(), of[(size_t)i]->size() * 8); });
    if (done < 3 * n_seq) { c->err = "tract position pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_viterbi_state_stats(strq_ctx* c, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                             double* logp, int64_t* counted, int32_t* status, int64_t* n_obs, double* sum, double* sumsq)
{
    STRQ_ENTER(c);
    if (n_seq > 0 && (!x_off || x_off[0] != 0 || !n_obs || !sum || !sumsq)) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (const int rc = check_windows(c, model_id, n_seq, x, x_off, 8192)) return rc;
    if (n_seq == 0) return STRQ_OK;
    const HostModel* hm = c->models[model_id];
    // the count decode first: logp, counted and status are strq_viterbi_batch's, and the observations stay in the context's buffer
    std::vector<double> lp((size_t)n_seq); std::vector<int64_t> cn((size_t)n_seq); std::vector<int32_t> stv((size_t)n_seq); std::vector<VitTask> tasks;
    if (const int rc = viterbi_batch(c, model_id, n_seq, x, x_off, 8192, lp.data(), cn.data(), stv.data(), nullptr, &tasks)) return rc;
    const size_t ne = (size_t)hm->silent_start;
    std::fill(n_obs, n_obs + (size_t)n_seq * ne, (int64_t)0); std::fill(sum, sum + (size_t)n_seq * ne, 0.0); std::fill(sumsq, sumsq + (size_t)n_seq * ne, 0.0);
    std::vector<StateStatsWindow> sw; std::vector<int64_t> win;
    for (int64_t i = 0; i < n_seq; ++i) {
        if (stv[(size_t)i] != 0) continue;
        StateStatsWindow w; w.task = tasks[(size_t)i];
        w.hm = hm; w.logp = lp[(size_t)i]; w.counted = cn[(size_t)i];
        sw.push_back(w); win.push_back(i);
    }
    StateStatsOut so;
    if (!sw.empty()) { if (const int rc = state_stats(c, sw, so, nullptr)) return rc; }
    for (size_t k = 0; k < sw.size(); ++k) {
        const size_t i = (size_t)win[k];
        if (so.status[k] == 2) { stv[i] = 4; continue; }
        std::memcpy(n_obs + i * ne, so.n[k].data(), ne * 8); std::memcpy(sum + i * ne, so.sum[k].data(), ne * 8); std::memcpy(sumsq + i * ne, so.sumsq[k].data(), ne * 8);
    }
    for (int64_t i = 0; i < n_seq; ++i) {
        if (logp) logp[i] = lp[(size_t)i];
        if (counted) counted[i] = cn[(size_t)i];
        if (status) status[i] = stv[(size_t)i];
    }
    return STRQ_OK;
}

int strq_forward_state_stats(strq_ctx* c, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                             double* log_lik, int32_t* status, double* w, double* wx, double* wxx)
{
    STRQ_ENTER(c);
    if (n_seq > 0 && (!x_off || x_off[0] != 0 || !w || !wx || !wxx)) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (const int rc = check_windows(c, model_id, n_seq, x, x_off, 8192)) return rc;
    if (n_seq == 0) return STRQ_OK;
    HostModel* hm = c->models[model_id];
    if (const int rc = posterior_model(c, hm)) return rc;
    std::vector<VitTask> tasks;
    if (const int rc = upload_windows(c, hm, n_seq, x, x_off, tasks)) return rc;
    std::vector<StatePostWindow> pw((size_t)n_seq);
    for (int64_t i = 0; i < n_seq; ++i) { pw[(size_t)i].task = tasks[(size_t)i]; pw[(size_t)i].hm = hm; }
    StatePostOut po;
    if (const int rc = state_posteriors(c, pw, po, nullptr)) return rc;
    const size_t ne = (size_t)hm->silent_start;
    std::fill(w, w + (size_t)n_seq * ne, 0.0); std::fill(wx, wx + (size_t)n_seq * ne, 0.0); std::fill(wxx, wxx + (size_t)n_seq * ne, 0.0);
    for (int64_t i = 0; i < n_seq; ++i) {
        double ll, mean, var;
        (void)fwd_finish(po.fwd[(size_t)i], 0, &ll, &mean, &var);
        if (log_lik) log_lik[i] = ll;
        if (status) status[i] = po.status[(size_t)i] == 2 ? 4 : po.status[(size_t)i];
        if (po.status[(size_t)i] != 0) continue;
        std::memcpy(w + (size_t)i * ne, po.w[(size_t)i].data(), ne * 8); std::memcpy(wx + (size_t)i * ne, po.wx[(size_t)i].data(), ne * 8);
        std::memcpy(wxx + (size_t)i * ne, po.wxx[(size_t)i].data(), ne * 8);
    }
    return STRQ_OK;
}

int strq_debug_tract_shape(const strq_ctx* c, int32_t* shape)
{
    if (!c || !shape) return STRQ_ERR_ARG;
    *shape = c->tract_shape_last;
    return STRQ_OK;
}

int strq_viterbi(strq_ctx* c, int32_t model_id, const double* x, int64_t T, double* logp, int64_t* counted,
                 int32_t* status, int32_t* path)
{
    STRQ_ENTER(c);
    const int64_t off[2] = {0, T};
    return viterbi_batch(c, model_id, 1, x, off, 0, logp, counted, status, path, nullptr);
}

}  // extern "C"
