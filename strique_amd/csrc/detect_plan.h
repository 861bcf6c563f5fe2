// Host-side bookkeeping of the detect pipeline (strq_detect_api.hip) that needs no device: the optional passes (switches, counters,
// refusals), the ragged packer of their fetches, the per-read rows of a batch, and the grouping of Viterbi tasks into launches.  Plain C++: no HIP headers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "../../include/strique_hip.h"

namespace strq {

// The layout of one block of memory, said once: add<T>(count) hands out the byte offset of a region of `count` T and advances, every
// region starts on a 16-byte boundary (a region of no elements takes no bytes), total() is what to reserve, at<T>(base, offset) the
// region's pointer in a block that starts at `base` (null in no block).  A block and its mirror (device / pinned) take their pointers
// from one Carve.
struct Carve {
    size_t end = 0;
    template <class T> size_t add(size_t count)
    {
        const size_t at = end;
        end += (count * sizeof(T) + 15) & ~(size_t)15;
        return at;
    }
    size_t total() const { return end; }
    template <class T> static T* at(void* base, size_t offset) { return base ? reinterpret_cast<T*>(static_cast<char*>(base) + offset) : nullptr; }
};

// The piece rule of the passes that decode windows once more into a workspace (records, back-pointers, stored forward vectors), said
// once.  The windows, in their order, are cut into pieces: a piece takes windows while the sum of their sizes stays within the budget
// and, with `max_windows`, while it holds fewer than that many.  A window that alone exceeds the budget is oversize, and a pass names
// what becomes of it: ALONE, it stays in its place as a piece of its own, over the budget (unit pass, flank-mod pass); LEFT_OUT, it is
// in no piece (tract positions, state statistics: status 2); IN_FRONT, it is carried ahead of all others with no bytes (state
// posteriors: status 2, the forward half still runs).  The sizes are the caller's: whoever places windows on 16-byte boundaries
// passes rounded sizes (bp_window_bytes), and the bytes of a piece are the sum of what was passed.
enum Oversize { OVERSIZE_ALONE, OVERSIZE_LEFT_OUT, OVERSIZE_IN_FRONT };
struct Piece { size_t first, last, bytes; };          // the windows order[first .. last) and what they take together
// order: the windows the pieces hold, as indices into the sizes; bytes: per position of `order`, what the window takes (0 for one carried
// in front); oversize: the windows left out or carried in front, ascending
struct PiecePlan { std::vector<int32_t> order; std::vector<size_t> bytes; std::vector<Piece> pieces; std::vector<int32_t> oversize; };
inline PiecePlan plan_pieces(const std::vector<size_t>& sizes, size_t budget, Oversize policy, size_t max_windows = 0)
{
    PiecePlan P;
    for (size_t i = 0; i < sizes.size(); ++i) if (policy != OVERSIZE_ALONE && sizes[i] > budget) P.oversize.push_back((int32_t)i);
    if (policy == OVERSIZE_IN_FRONT) { P.order = P.oversize; P.bytes.assign(P.oversize.size(), 0); }
    for (size_t i = 0; i < sizes.size(); ++i) if (policy == OVERSIZE_ALONE || sizes[i] <= budget) { P.order.push_back((int32_t)i); P.bytes.push_back(sizes[i]); }
    for (size_t c0 = 0; c0 < P.order.size();) {
        size_t c1 = c0, sum = 0;
        while (c1 < P.order.size() && (!max_windows || c1 - c0 < max_windows) && (c1 == c0 || sum + P.bytes[c1] <= budget)) sum += P.bytes[c1++];
        P.pieces.push_back({c0, c1, sum}); c0 = c1;
    }
    return P;
}
// the budget of a pass: 8 GiB, or what its option says where that is a number above 0 (callers pass strq::opt("STRQ_..._WS_BYTES"))
inline size_t ws_budget(const char* option_value) { const long long v = option_value ? atoll(option_value) : 0; return v > 0 ? (size_t)v : (size_t)8 << 30; }
// back-pointers of one window: uint16 per (time step, state), T + 1 steps; every window starts on a 16-byte boundary
inline size_t bp_window_bytes(int64_t T, int n_states) { return ((size_t)(T + 1) * (size_t)n_states * 2 + 15) & ~(size_t)15; }

// The switches of the optional passes around the count decode (PASSES below lists them), and the thresholds anchored counting and renorm
// come with.  DetectState holds what the next run call uses, a slot what its sub-batch was launched with, Batch what the last run call
// ran with.
struct Extras { bool units = false, conf = false, llr = false, anch = false, var = false; double anch_min = 0.0; bool renorm = false; double renorm_min = 0.0; bool amod = false;
                bool tracts = false, fmod = false, tpos = false, sstats = false, spost = false;
                bool motifs = false; int motif_segment = 0; };

// The passes, said once.  What the last run call's pass did is one PassStats: the GPU milliseconds and up to seven counters, which the
// pass's own enum names.  A row of PASSES holds what the entry points need of a pass: its name in messages, its switch, what a batch
// that ran without it lacks and the entry that turns it on (the "ran without" refusal of its fetch), whether a scan refuses it, and the
// layout strq_last_* hands out -- `out[k]` is the counter at position k, MS the milliseconds.
enum Pass { PASS_UNITS, PASS_CONF, PASS_LLR, PASS_VAR, PASS_ANCH, PASS_AMOD, PASS_TRACTS, PASS_RENORM, PASS_FMOD, PASS_TPOS, PASS_SSTATS, PASS_SPOST, PASS_MOTIFS, N_PASS };
struct PassStats { float ms; double v[7]; };
enum { UNIT_BYTES, UNIT_READS, UNIT_POSITIONS, CONF_WINDOWS = 0, CONF_NOPATH, CONF_EXPO, LLR_UNITS = 0, LLR_READS, LLR_LAUNCHES,
       VAR_LAUNCHES = 0, VAR_PASSAGES, VAR_READS, ANCH_KINDS = 0 /* .. 3: reads of kind 0 .. 3 */, ANCH_LAUNCHES = 4, ANCH_G2, ANCH_LANE,
       AMOD_READS = 0, AMOD_UNITS, AMOD_LAUNCHES, TRACT_WINDOWS = 0, TRACT_LAUNCHES, TRACT_FAILED, RN_FITTED = 0, RN_APPLIED, RN_LAUNCHES,
       FMOD_FLANKS = 0, FMOD_GROUPS, FMOD_LAUNCHES, TPOS_WINDOWS = 0, TPOS_LAUNCHES, TPOS_BYTES,
       SST_WINDOWS = 0, SST_LAUNCHES, SST_BYTES, SPOST_WINDOWS = 0, SPOST_LAUNCHES, SPOST_BYTES,
       MOTIF_READS = 0, MOTIF_SEGMENTS, MOTIF_LAUNCHES, MOTIF_DECODES /* strq_last_motifs hands it out behind the row's four */ };
constexpr int8_t MS = -1;
struct PassInfo { const char* name; bool Extras::* on; const char* lacks; const char* entry; bool scan_refuses; int n_out; int8_t out[8]; };
constexpr PassInfo PASSES[N_PASS] = {
    {"units", &Extras::units, "unit positions", "strq_set_units", false, 4, {MS, 0, 1, 2}},
    {"confidence", &Extras::conf, "confidence", "strq_set_confidence", false, 4, {MS, 0, 1, 2}},
    {"mod-llr", &Extras::llr, "per-unit scores", "strq_set_mod_llr", false, 4, {MS, 0, 1, 2}},
    {"variants", &Extras::var, "variants", "strq_set_variants", true, 4, {VAR_LAUNCHES, VAR_PASSAGES, MS, VAR_READS}},
    {"anchored", &Extras::anch, "anchored counting", "strq_set_anchored", true, 8, {MS, 0, 1, 2, 3, ANCH_LAUNCHES, ANCH_G2, ANCH_LANE}},
    {"anchored-mod", &Extras::amod, "anchored methylation calls", "strq_set_anchored_mod", true, 4, {MS, 0, 1, 2}},
    {"tracts", &Extras::tracts, "tracts", "strq_set_tracts", true, 4, {MS, 0, 1, 2}},
    {"renorm", &Extras::renorm, "renorm", "strq_set_renorm", true, 4, {MS, 0, 1, 2}},
    {"flank-mod", &Extras::fmod, "flank methylation calls", "strq_set_flank_mod", true, 4, {MS, 0, 1, 2}},
    {"tract-positions", &Extras::tpos, "tract positions", "strq_set_tract_positions", true, 4, {MS, 0, 1, 2}},
    {"state-stats", &Extras::sstats, "state statistics", "strq_set_state_stats", true, 4, {MS, 0, 1, 2}},
    {"state-posteriors", &Extras::spost, "state posteriors", "strq_set_state_posteriors", true, 4, {MS, 0, 1, 2}},
    {"motifs", &Extras::motifs, "the motif track", "strq_set_motifs", true, 4, {MS, 0, 1, 2}},
};
inline void pass_stats_out(Pass p, const PassStats& s, double* out)
{
    for (int k = 0; k < PASSES[p].n_out; ++k) out[k] = PASSES[p].out[k] == MS ? (double)s.ms : s.v[PASSES[p].out[k]];
}
// The pass a scan refuses first among those switched on, in the order the run call has always looked (N_PASS: none); the refusals as text
constexpr Pass SCAN_CHECKS[] = {PASS_AMOD, PASS_ANCH, PASS_VAR, PASS_TRACTS, PASS_RENORM, PASS_FMOD, PASS_TPOS, PASS_SSTATS, PASS_SPOST, PASS_MOTIFS};
inline Pass scan_refusal(const Extras& ex)
{
    for (Pass p : SCAN_CHECKS) if (PASSES[p].scan_refuses && ex.*PASSES[p].on) return p;
    return N_PASS;
}
inline std::string scan_refusal_text(Pass p) { return std::string(PASSES[p].name) + ": not available in a scan (strq_scan_set)"; }
inline std::string ran_without_text(Pass p) { return std::string("the last batch ran without ") + PASSES[p].lacks + " (" + PASSES[p].entry + ")"; }

// off[0 .. n] of a ragged output of n reads, and with `pools` its values: len(i, &k, &k2) gives the elements read i adds to either pool,
// copy(i, pos, pos2) puts them at those positions -- called only where both pools hold them (`cap`, `cap2`).  Returns n, or the read
// whose values did not fit: off[] is then written up to that read.  Without pools it only measures.  off2 (or null) takes the second
// pool's offsets per read, total2 (or null) its size.
template <class Len, class Copy>
int64_t pack_ragged2(int64_t n, int64_t* off, int64_t* off2, bool pools, int64_t cap, int64_t cap2, int64_t* total2, Len len, Copy copy)
{
    int64_t pos = 0, pos2 = 0;
    for (int64_t i = 0; i < n; ++i) {
        off[i] = pos;
        if (off2) off2[i] = pos2;
        int64_t k = 0, k2 = 0;
        len(i, &k, &k2);
        if (pools) {
            if (pos + k > cap || pos2 + k2 > cap2) return i;
            copy(i, pos, pos2);
        }
        pos += k; pos2 += k2;
    }
    off[n] = pos;
    if (off2) off2[n] = pos2;
    if (total2) *total2 = pos2;
    return n;
}
// ... with one pool: len(i) elements of read i, copy(i, pos)
template <class Len, class Copy>
int64_t pack_ragged(int64_t n, int64_t* off, bool pool, int64_t cap, Len len, Copy copy)
{
    return pack_ragged2(n, off, nullptr, pool, cap, 0, nullptr, [&](int64_t i, int64_t* k, int64_t*) { *k = len(i); }, [&](int64_t i, int64_t pos, int64_t) { copy(i, pos); });
}

// What the variant pass leaves per read: the passages of its variant-model decode (strq_batch_fetch_variants)
struct VariantRow {
    int32_t decoded = 0, count_v = 0, n_branch = 0;
    std::vector<int8_t> branch; std::vector<int64_t> end; std::vector<double> V;      // per passage: branch, raw sample of w_j, n_branch scores
};

// What a batch holds per read: the row, the modification pattern and the outputs of the optional passes.  One place sizes them, one
// function puts a read back to its initial values -- a row that was never computed is never handed out.
struct ReadRows {
    std::vector<strq_result> results;
    std::vector<std::string> mod;                 // modification pattern ('-' if none)
    std::vector<int64_t> flank_ends;              // two per read: where the whole prefix flank begins and the whole suffix flank ends (strq_batch_fetch_flank_ranges)
    std::vector<std::vector<int64_t>> units;      // unit positions (strq_batch_fetch_units)
    std::vector<uint8_t> unit_dec;                // 1: the read was decoded (gate passed, the flanked model found a path)
    std::vector<double> conf;                     // log_lik, count_mean, count_sd (strq_batch_fetch_confidence); NaN while not decoded
    std::vector<uint8_t> conf_dec;
    std::vector<std::vector<double>> llr;         // (V_base, V_mod) per repeat unit (strq_batch_fetch_mod_llr); empty: none
    std::vector<strq_anchored> anch;              // kind and decode of a read that holds one flank (strq_batch_fetch_anchored); zeros: kind 0
    // methylation calls of anchored reads: empty until a run call with the switch on sizes them (size_amod), like `renorm`
    std::vector<uint8_t> amod_called;             // 1: the read has an anchored methylation call (strq_batch_fetch_anchored_mod)
    std::vector<std::string> amod;                // ... its pattern ('-': the dual model found no path)
    std::vector<std::vector<double>> amod_llr;    // ... (V_base, V_mod) per character of it, with strq_set_mod_llr on; empty: none
    std::vector<VariantRow> var;                  // passages of the variant model (strq_batch_fetch_variants); decoded = 0: none
    std::vector<strq_renorm> renorm;              // fits of the second normalisation step (strq_batch_fetch_renorm); zeros: not fitted.  Empty
                                                  // until a run call with the switch on sizes it (size_renorm)
    void size_reads(int64_t n)
    {
        const size_t m = (size_t)n;
        results.assign(m, strq_result()); mod.assign(m, std::string("-")); flank_ends.assign(2 * m, 0);
        units.assign(m, std::vector<int64_t>()); unit_dec.assign(m, 0);
        conf.assign(3 * m, NAN); conf_dec.assign(m, 0);
        llr.assign(m, std::vector<double>());
        anch.assign(m, strq_anchored());
        amod_called.clear(); amod.clear(); amod_llr.clear();
        var.assign(m, VariantRow());
        renorm.clear(); tracts.clear(); fmod_called.clear(); fmod.clear(); tpos_status.clear(); tpos.clear(); sst_status.clear(); sst.clear(); spost_status.clear(); spost.clear();
        motifs.clear(); motif_V.clear(); motif_win.clear();
    }
    std::vector<strq_tracts> tracts;              // per-tract counts of the compound model (strq_batch_fetch_tracts); status 1: not decoded.  Empty
                                                  // until a run call with the switch on sizes it (size_tracts)
    // flank methylation calls (strq_batch_fetch_flank_mod): empty until a run call with the switch on sizes them (size_fmod)
    std::vector<uint8_t> fmod_called;             // 1: the read qualified
    std::vector<std::vector<strq_flank_mod_group>> fmod;      // ... its records, prefix groups first
    void size_fmod() { if (fmod_called.size() != results.size()) { fmod_called.assign(results.size(), 0); fmod.assign(results.size(), std::vector<strq_flank_mod_group>()); } }
    // unit positions of the tracts (strq_batch_fetch_tract_positions): empty until a run call with the switch on sizes them (size_tpos)
    std::vector<int32_t> tpos_status;             // 0 positions, 1 none (tract status is not 0), 2 back-pointers over the budget
    std::vector<std::vector<int64_t>> tpos;       // three per read, model order
    void size_tpos() { if (tpos_status.size() != results.size()) { tpos_status.assign(results.size(), 1); tpos.assign(3 * results.size(), std::vector<int64_t>()); } }
    // state statistics of the flanked decode (strq_batch_fetch_state_stats): empty until a run call with the switch on sizes them (size_sst)
    struct StateStatsRow { std::vector<int64_t> n; std::vector<double> sum, sumsq; };
    std::vector<int32_t> sst_status;              // 0 statistics, 1 none (not decoded), 2 back-pointers over the budget
    std::vector<StateStatsRow> sst;               // n_emit entries each where the status is 0, else empty
    void size_sst() { if (sst_status.size() != results.size()) { sst_status.assign(results.size(), 1); sst.assign(results.size(), StateStatsRow()); } }
    // state posteriors of the flanked decode (strq_batch_fetch_state_posteriors): empty until a run call with the switch on sizes them (size_spost)
    struct StatePostRow { double log_lik = NAN; std::vector<double> w, wx, wxx; };
    std::vector<int32_t> spost_status;            // 0 statistics, 1 none (not decoded, or no path in the forward pass), 2 stored vectors over the budget
    std::vector<StatePostRow> spost;              // n_emit entries each where the status is 0, else empty
    // the motif track (strq_batch_fetch_motifs): empty until a run call with the switch on sizes them (size_motifs)
    std::vector<strq_motifs> motifs;              // status 1: not scored
    std::vector<std::vector<double>> motif_V;     // n_seg * n_cand scores per read, segment-major
    std::vector<std::vector<int32_t>> motif_win;  // n_seg winners per read
    static strq_motifs no_motifs() { strq_motifs m = strq_motifs(); m.status = 1; m.decode_status = 1; return m; }
    void size_motifs() { if (motifs.size() != results.size()) { motifs.assign(results.size(), no_motifs()); motif_V.assign(results.size(), std::vector<double>()); motif_win.assign(results.size(), std::vector<int32_t>()); } }
    void size_spost() { if (spost_status.size() != results.size()) { spost_status.assign(results.size(), 1); spost.assign(results.size(), StatePostRow()); } }
    static strq_tracts no_tracts() { strq_tracts t = strq_tracts(); t.status = 1; return t; }
    void size_tracts() { if (tracts.size() != results.size()) tracts.assign(results.size(), no_tracts()); }
    void size_renorm() { if (renorm.size() != results.size()) renorm.assign(results.size(), strq_renorm()); }
    void size_amod()
    {
        if (amod_called.size() == results.size()) return;
        amod_called.assign(results.size(), 0); amod.assign(results.size(), std::string()); amod_llr.assign(results.size(), std::vector<double>());
    }
    void clear_read(int64_t read)
    {
        const size_t r = (size_t)read;
        if (read < 0 || r >= results.size()) return;
        results[r] = strq_result(); mod[r] = "-"; flank_ends[2 * r] = flank_ends[2 * r + 1] = 0;
        units[r].clear(); unit_dec[r] = 0;
        conf[3 * r] = conf[3 * r + 1] = conf[3 * r + 2] = NAN; conf_dec[r] = 0;
        llr[r].clear();
        anch[r] = strq_anchored();
        if (r < amod_called.size()) { amod_called[r] = 0; amod[r].clear(); amod_llr[r].clear(); }
        var[r] = VariantRow();
        if (r < renorm.size()) renorm[r] = strq_renorm();
        if (r < tracts.size()) tracts[r] = no_tracts();
        if (r < fmod_called.size()) { fmod_called[r] = 0; fmod[r].clear(); }
        if (r < tpos_status.size()) { tpos_status[r] = 1; for (int j = 0; j < 3; ++j) tpos[3 * r + j].clear(); }
        if (r < sst_status.size()) { sst_status[r] = 1; sst[r] = StateStatsRow(); }
        if (r < spost_status.size()) { spost_status[r] = 1; spost[r] = StatePostRow(); }
        if (r < motifs.size()) { motifs[r] = no_motifs(); motif_V[r].clear(); motif_win[r].clear(); }
    }
};

// The record of a read of kind 2 (ends in the repeat) or 3 (starts in it) from the MARK decode of its window: `first` observations
// into the read, T observations, `enter` / `leave` the 1-based observation of the first emission inside the repeat section and of the
// first one behind it (0: none), as VitResult::dbg[0 .. 1] report them.  The free state of kind 2 emits behind the section, that of kind 3
// in front of it.  A decode without a path, or one whose marks do not describe such a path, keeps the kind with zeros.
inline strq_anchored anchored_record(int32_t kind, int64_t first, int64_t T, int32_t vit_status, int64_t visits, int32_t bias, double logp,
                                     int64_t enter, int64_t leave)
{
    strq_anchored a = strq_anchored();
    a.kind = kind; a.status = vit_status ? (vit_status == 2 ? 2 : 1) : 0;
    if (a.status) return a;
    if (leave == 0) leave = T + 1;          // the section reaches the end of the window
    if (enter < 1 || leave <= enter || leave > T + 1) { a.status = 1; return a; }
    a.count = (int32_t)(visits + bias); a.log_p = logp;
    a.begin = first + enter - 1; a.end = first + leave - 1;
    a.free_samples = kind == 2 ? T - (leave - 1) : enter - 1;
    return a;
}

struct VitGroup { int shape, first, count, max_cells, route; };      // one Viterbi launch: kernel shape, task range, largest n_cells of its models; its route (unit pass)

struct GroupItem { int route, shape, n_cells; };

// The launches of `items`: one per (route, shape) in ascending order, the items of a launch in their own order.  pos[k]: the task
// position of item k; order[p]: the item at task position p.
struct Grouping { std::vector<VitGroup> groups; std::vector<int32_t> pos, order; };

inline Grouping group_items(const std::vector<GroupItem>& items)
{
    std::map<std::pair<int, int>, std::vector<int32_t>> by_key;
    for (size_t k = 0; k < items.size(); ++k) by_key[{items[k].route, items[k].shape}].push_back((int32_t)k);
    Grouping G; G.pos.assign(items.size(), 0); G.order.reserve(items.size());
    for (const auto& g : by_key) {
        VitGroup v = {g.first.second, (int)G.order.size(), (int)g.second.size(), 0, g.first.first};
        for (int32_t k : g.second) {
            v.max_cells = std::max(v.max_cells, items[(size_t)k].n_cells);
            G.pos[(size_t)k] = (int32_t)G.order.size(); G.order.push_back(k);
        }
        G.groups.push_back(v);
    }
    return G;
}

// The order of a second decode of the reads `who` of a sub-batch (tract pass, anchored pass, forward pass): of(i, item, model) gives
// the route, shape and cells of read i's model and the model's device image, or false for a read the pass cannot take (nothing is
// planned then).  The launches, and per task position the read and its model.
template <class Model> struct DecodeOrder { Grouping G; std::vector<int32_t> read_of; std::vector<const Model*> model; };
template <class Model, class Of>
bool decode_order(const std::vector<int>& who, Of of, DecodeOrder<Model>& out)
{
    std::vector<GroupItem> items(who.size()); std::vector<const Model*> mv(who.size());
    for (size_t k = 0; k < who.size(); ++k) if (!of(who[k], items[k], mv[k])) return false;
    out.G = group_items(items);
    for (int32_t k : out.G.order) { out.read_of.push_back(who[(size_t)k]); out.model.push_back(mv[(size_t)k]); }
    return true;
}

}  // namespace strq
