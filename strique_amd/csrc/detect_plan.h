// Host-side bookkeeping of the detect pipeline (strq_detect_api.hip) that needs no device: the optional per-read outputs and their
// switches, the per-read rows of a batch, and the grouping of Viterbi tasks into launches.  Plain C++: no HIP headers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
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

// The optional passes behind the count decode: unit positions (strq_set_units), forward pass (strq_set_confidence), per-unit scores
// (strq_set_mod_llr).  DetectState holds what the next run call uses, a slot what its sub-batch was launched with, Batch what the last
// run call ran with.
// Anchored counting (strq_set_anchored) is the fourth: it comes with its score threshold.
// The variant pass (strq_set_variants) is the fifth.
// Renorm (strq_set_renorm) is the sixth, in front of the alignments instead of behind the decode: it comes with its share threshold.
// Methylation calls of anchored reads (strq_set_anchored_mod) are the seventh: behind the anchored decode, which they need.
// The tract pass (strq_set_tracts) is the eighth: where the forward pass runs, behind the rows.
struct Extras { bool units = false, conf = false, llr = false, anch = false, var = false; double anch_min = 0.0; bool renorm = false; double renorm_min = 0.0; bool amod = false;
                bool tracts = false; };

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
        results.assign(m, strq_result()); mod.assign(m, std::string("-"));
        units.assign(m, std::vector<int64_t>()); unit_dec.assign(m, 0);
        conf.assign(3 * m, NAN); conf_dec.assign(m, 0);
        llr.assign(m, std::vector<double>());
        anch.assign(m, strq_anchored());
        amod_called.clear(); amod.clear(); amod_llr.clear();
        var.assign(m, VariantRow());
        renorm.clear(); tracts.clear();
    }
    std::vector<strq_tracts> tracts;              // per-tract counts of the compound model (strq_batch_fetch_tracts); status 1: not decoded.  Empty
                                                  // until a run call with the switch on sizes it (size_tracts)
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
        results[r] = strq_result(); mod[r] = "-";
        units[r].clear(); unit_dec[r] = 0;
        conf[3 * r] = conf[3 * r + 1] = conf[3 * r + 2] = NAN; conf_dec[r] = 0;
        llr[r].clear();
        anch[r] = strq_anchored();
        if (r < amod_called.size()) { amod_called[r] = 0; amod[r].clear(); amod_llr[r].clear(); }
        var[r] = VariantRow();
        if (r < renorm.size()) renorm[r] = strq_renorm();
        if (r < tracts.size()) tracts[r] = no_tracts();
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

}  // namespace strq
