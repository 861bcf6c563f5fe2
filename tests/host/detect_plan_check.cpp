// Stand-alone host program over strique_amd/csrc/detect_plan.h (no HIP): the anchored record from the marks of a MARK decode, the
// per-read rows, the grouping of tasks, the layout of a workspace (Carve), the ragged packer of the fetches, the pass table with the
// layouts of strq_last_*, the order of a second decode, the piece planner against the five loops it replaced.  Built and run under ASan/UBSan by tests/test_detect_plan_host.py; exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../strique_amd/csrc/detect_plan.h"
#include "../../strique_amd/csrc/vit_model.h"

using namespace strq;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static bool zero_but_kind(const strq_anchored& a, int32_t kind, int32_t status)
{
    return a.kind == kind && a.status == status && a.count == 0 && a.log_p == 0.0 && a.begin == 0 && a.end == 0 && a.free_samples == 0;
}

// Carve: `counts[k]` elements of T per region k, other element types in between.  Every offset a multiple of 16, no two regions overlap,
// total() covers the last one; then every element written through its typed pointer in a block of exactly total() bytes and read back
// (ASan sees an overrun, UBSan a misaligned pointer).
struct Odd { char c[20]; int32_t v; };          // 24 bytes: no multiple of 16
template <class T> static T value_of(size_t region, size_t i) { return (T)(region * 37 + i * 3 + 1); }
template <> Odd value_of<Odd>(size_t region, size_t i) { Odd o; std::memset(o.c, (int)(region + 1), sizeof(o.c)); o.v = (int32_t)(region * 1000 + i); return o; }
static bool same(const Odd& a, const Odd& b) { return std::memcmp(a.c, b.c, sizeof(a.c)) == 0 && a.v == b.v; }
template <class T> static bool same(const T& a, const T& b) { return a == b; }

template <class T> static void carve_case(const std::vector<size_t>& counts)
{
    Carve lay;
    std::vector<size_t> off;
    for (size_t n : counts) off.push_back(lay.add<T>(n));
    const size_t tail = lay.add<char>(3);          // a region of another element size behind them
    for (size_t k = 0; k < counts.size(); ++k) {
        CHECK(off[k] % 16 == 0);
        const size_t end = off[k] + counts[k] * sizeof(T);
        CHECK(end <= lay.total());
        const size_t next = k + 1 < counts.size() ? off[k + 1] : tail;
        CHECK(end <= next);          // offsets ascend, so this is every pair
    }
    CHECK(tail % 16 == 0 && tail + 3 <= lay.total());
    std::vector<char> block(lay.total());
    CHECK(Carve::at<T>(nullptr, off.empty() ? 0 : off[0]) == nullptr);
    for (size_t k = 0; k < counts.size(); ++k) {
        T* p = Carve::at<T>(block.data(), off[k]);
        for (size_t i = 0; i < counts[k]; ++i) p[i] = value_of<T>(k, i);
    }
    char* t = Carve::at<char>(block.data(), tail); t[0] = 'a'; t[1] = 'b'; t[2] = 'c';
    for (size_t k = 0; k < counts.size(); ++k) {
        const T* p = Carve::at<const T>(block.data(), off[k]);
        for (size_t i = 0; i < counts[k]; ++i) CHECK(same(p[i], value_of<T>(k, i)));
    }
    CHECK(t[0] == 'a' && t[1] == 'b' && t[2] == 'c');
}

static void carve_checks()
{
    CHECK(Carve().total() == 0);
    // element counts 0, 1 and odd ones, a region of no elements between two others, at the front and at the end
    const std::vector<std::vector<size_t>> shapes = {{0}, {1}, {3}, {1, 0, 1}, {5, 0, 7}, {0, 9, 0}, {17, 1, 33, 4}, {1, 1, 1, 1}};
    for (const auto& counts : shapes) {
        carve_case<char>(counts); carve_case<int32_t>(counts); carve_case<int64_t>(counts); carve_case<Odd>(counts);
    }
    // mixed element types in one block, as a pass lays out its tasks: the neighbours of an empty region do not share a byte
    Carve lay;
    const size_t a = lay.add<Odd>(3), none = lay.add<int64_t>(0), b = lay.add<char>(1), c = lay.add<int32_t>(5);
    CHECK(a == 0 && b == 80 && none == b && c == 96 && lay.total() == 128);          // 72 -> 80, nothing, 1 -> 16, 20 -> 32
    std::vector<char> block(lay.total(), 0);
    Carve::at<Odd>(block.data(), a)[2] = value_of<Odd>(9, 2);
    *Carve::at<char>(block.data(), b) = 'x';
    for (int i = 0; i < 5; ++i) Carve::at<int32_t>(block.data(), c)[i] = -1 - i;
    CHECK(same(Carve::at<Odd>(block.data(), a)[2], value_of<Odd>(9, 2)) && *Carve::at<char>(block.data(), b) == 'x' && Carve::at<int32_t>(block.data(), c)[4] == -5);
}

// The ragged packer on lengths {0, 3, 0, 1}: offsets, a pool that is exactly filled, one that is an element short, no pool, no reads,
// and two pools at once.  Pools are exactly as large as their capacity (ASan sees a copy behind it).
static void packer_checks()
{
    const std::vector<std::vector<int32_t>> reads = {{}, {7, 8, 9}, {}, {5}};
    const int64_t want[5] = {0, 0, 3, 3, 4};
    auto len = [&](int64_t i) { return (int64_t)reads[(size_t)i].size(); };
    int copies = 0;
    auto run = [&](int64_t n, int64_t* off, int32_t* pool, int64_t cap) {
        return pack_ragged(n, off, pool != nullptr, cap, len, [&](int64_t i, int64_t pos) {
            ++copies;
            for (size_t j = 0; j < reads[(size_t)i].size(); ++j) pool[pos + (int64_t)j] = reads[(size_t)i][j];
        });
    };
    std::vector<int64_t> off(5, -1); std::vector<int32_t> pool(4, -1);
    CHECK(run(4, off.data(), pool.data(), 4) == 4);
    for (int k = 0; k < 5; ++k) CHECK(off[(size_t)k] == want[k]);
    CHECK(pool[0] == 7 && pool[1] == 8 && pool[2] == 9 && pool[3] == 5);
    // capacity 3: read 3 does not fit; the offsets up to it are written, nothing behind them
    std::vector<int64_t> off3(5, -1); std::vector<int32_t> pool3(3, -1);
    CHECK(run(4, off3.data(), pool3.data(), 3) == 3);
    CHECK(off3[0] == 0 && off3[1] == 0 && off3[2] == 3 && off3[3] == 3 && off3[4] == -1 && pool3[2] == 9);
    // no pool: the same offsets, nothing copied
    std::vector<int64_t> offm(5, -1);
    copies = 0;
    CHECK(run(4, offm.data(), nullptr, 0) == 4 && copies == 0);
    for (int k = 0; k < 5; ++k) CHECK(offm[(size_t)k] == want[k]);
    // no reads: off[0] alone
    std::vector<int64_t> off0(1, -1);
    CHECK(run(0, off0.data(), pool.data(), 4) == 0 && off0[0] == 0);
    // two pools: values of lengths {0, 6, 0, 2} beside them
    const int64_t vlen[4] = {0, 6, 0, 2}, want2[5] = {0, 0, 6, 6, 8};
    std::vector<int64_t> offa(5, -1), offb(5, -1); std::vector<int32_t> pa(4, -1); std::vector<double> pb(8, -1.0);
    int64_t total2 = -1;
    auto run2 = [&](int64_t* o2, bool pools, int64_t cap, int64_t cap2) {
        return pack_ragged2(4, offa.data(), o2, pools, cap, cap2, &total2, [&](int64_t i, int64_t* k, int64_t* k2) { *k = len(i); *k2 = vlen[i]; },
                            [&](int64_t i, int64_t pos, int64_t pos2) {
                                for (int64_t j = 0; j < len(i); ++j) pa[(size_t)(pos + j)] = reads[(size_t)i][(size_t)j];
                                for (int64_t j = 0; j < vlen[i]; ++j) pb[(size_t)(pos2 + j)] = (double)(10 * i + j);
                            });
    };
    CHECK(run2(offb.data(), true, 4, 8) == 4 && total2 == 8);
    for (int k = 0; k < 5; ++k) CHECK(offa[(size_t)k] == want[k] && offb[(size_t)k] == want2[k]);
    CHECK(pa[3] == 5 && pb[0] == 10.0 && pb[5] == 15.0 && pb[6] == 30.0 && pb[7] == 31.0);
    CHECK(run2(nullptr, true, 4, 7) == 3);          // the second pool an element short, no offsets of its own
    CHECK(run2(offb.data(), true, 2, 8) == 1);      // the first pool too small for read 1
    total2 = -1;
    CHECK(run2(nullptr, false, 0, 0) == 4 && total2 == 8);
}

// The layouts of strq_last_*: every field of a PassStats distinct, the two layouts that do not start with the milliseconds as literals.
static void stats_checks()
{
    PassStats s; s.ms = 0.5f;
    for (int k = 0; k < 7; ++k) s.v[k] = 10.0 + k;
    for (int p = 0; p < N_PASS; ++p) {
        double out[9]; for (double& o : out) o = -1.0;
        pass_stats_out((Pass)p, s, out);
        const int n = PASSES[p].n_out;
        CHECK(n == (p == PASS_ANCH ? 8 : 4) && out[n] == -1.0);
        if (p == PASS_VAR) CHECK(out[0] == 10.0 && out[1] == 11.0 && out[2] == 0.5 && out[3] == 12.0);          // launches, passages, ms, reads
        else if (p == PASS_ANCH) {          // ms, kinds[4], launches, g2, lane
            CHECK(out[0] == 0.5 && out[1] == 10.0 && out[2] == 11.0 && out[3] == 12.0 && out[4] == 13.0 && out[5] == 14.0 && out[6] == 15.0 && out[7] == 16.0);
        } else CHECK(out[0] == 0.5 && out[1] == 10.0 && out[2] == 11.0 && out[3] == 12.0);
        for (int a = 0; a < n; ++a) for (int b = a + 1; b < n; ++b) CHECK(out[a] != out[b]);          // no field handed out twice
    }
    CHECK(VAR_LAUNCHES == 0 && VAR_PASSAGES == 1 && VAR_READS == 2 && ANCH_KINDS == 0 && ANCH_LAUNCHES == 4 && ANCH_G2 == 5 && ANCH_LANE == 6);
    PassStats all[N_PASS];
    for (PassStats& t : all) t = s;
    std::fill(all, all + N_PASS, PassStats());
    for (const PassStats& t : all) { CHECK(t.ms == 0.0f); for (double v : t.v) CHECK(v == 0.0); }
    // what a scan refuses, in the order the run call looks: anchored-mod in front of anchored; units, confidence and mod-llr never
    Extras ex;
    CHECK(scan_refusal(ex) == N_PASS);
    ex.units = ex.conf = ex.llr = true;
    CHECK(scan_refusal(ex) == N_PASS);
    ex.renorm = true; CHECK(scan_refusal(ex) == PASS_RENORM);
    ex.tracts = true; CHECK(scan_refusal(ex) == PASS_TRACTS);
    ex.var = true; CHECK(scan_refusal(ex) == PASS_VAR);
    ex.anch = true; CHECK(scan_refusal(ex) == PASS_ANCH);
    ex.amod = true; CHECK(scan_refusal(ex) == PASS_AMOD);
    CHECK(scan_refusal_text(PASS_AMOD) == "anchored-mod: not available in a scan (strq_scan_set)");
    CHECK(ran_without_text(PASS_UNITS) == "the last batch ran without unit positions (strq_set_units)");
    CHECK(ran_without_text(PASS_AMOD) == "the last batch ran without anchored methylation calls (strq_set_anchored_mod)");
}

// The order of a second decode: five reads over two shapes and two routes.
static void decode_order_checks()
{
    struct M { int id; };
    const M models[5] = {{0}, {1}, {2}, {3}, {4}};
    const std::vector<int> who = {3, 4, 7, 9, 12};
    const GroupItem item[5] = {{1, 9, 100}, {0, 5, 300}, {0, 9, 200}, {1, 9, 50}, {0, 5, 10}};
    auto of = [&](int i, GroupItem& it, const M*& m) {
        const size_t k = (size_t)(std::find(who.begin(), who.end(), i) - who.begin());
        it = item[k]; m = &models[k];
        return true;
    };
    DecodeOrder<M> D;
    CHECK(decode_order<M>(who, of, D));
    CHECK(D.G.groups.size() == 3 && D.G.groups[0].route == 0 && D.G.groups[0].shape == 5 && D.G.groups[1].shape == 9 && D.G.groups[2].route == 1 && D.G.groups[2].count == 2);
    CHECK(D.read_of.size() == 5 && D.model.size() == 5);
    for (size_t at = 0; at < 5; ++at) {
        const size_t k = (size_t)D.G.order[at];
        CHECK(D.read_of[at] == who[k] && D.model[at] == &models[k] && D.G.pos[k] == (int32_t)at);
    }
    CHECK(D.read_of[0] == 4 && D.read_of[1] == 12 && D.read_of[2] == 7 && D.read_of[3] == 3 && D.read_of[4] == 9);
    // a read the pass cannot take: nothing is planned
    DecodeOrder<M> R;
    CHECK(!decode_order<M>(who, [&](int i, GroupItem& it, const M*& m) { return i != 7 && of(i, it, m); }, R) && R.G.groups.empty() && R.read_of.empty());
    DecodeOrder<M> E;
    CHECK(decode_order<M>(std::vector<int>(), of, E) && E.G.groups.empty() && E.read_of.empty() && E.model.empty());
}

// The piece planner against the five loops it replaced, each as its pass had it (the pass's own names: ws / fl, c0, c1, bytes, budget);
// a loop records the windows in its order, what it added per window, its pieces and the windows it gave status 2.
struct RefPlan { std::vector<int32_t> order; std::vector<size_t> bytes; std::vector<Piece> pieces; std::vector<int32_t> oversize; };
struct RefW { int i; size_t bytes; };

static RefPlan ref_unit_pass(const std::vector<size_t>& raw, size_t budget)          // sums the sizes as they are
{
    RefPlan R; std::vector<RefW> ws;
    for (size_t i = 0; i < raw.size(); ++i) ws.push_back({(int)i, raw[i]});
    for (size_t c0 = 0; c0 < ws.size();) {
        size_t c1 = c0, bytes = 0;
        while (c1 < ws.size() && (c1 == c0 || bytes + ws[c1].bytes <= budget)) bytes += ws[c1++].bytes;
        R.pieces.push_back({c0, c1, bytes});
        c0 = c1;
    }
    for (const RefW& w : ws) { R.order.push_back(w.i); R.bytes.push_back(w.bytes); }
    return R;
}
static RefPlan ref_flank_mod_pass(const std::vector<size_t>& raw, size_t budget)     // sums the 16-byte-rounded sizes
{
    RefPlan R; std::vector<RefW> fl;
    for (size_t i = 0; i < raw.size(); ++i) fl.push_back({(int)i, raw[i]});
    for (size_t c0 = 0; c0 < fl.size();) {
        size_t c1 = c0, bytes = 0;
        while (c1 < fl.size() && (c1 == c0 || bytes + ((fl[c1].bytes + 15) & ~(size_t)15) <= budget)) bytes += (fl[c1++].bytes + 15) & ~(size_t)15;
        R.pieces.push_back({c0, c1, bytes});
        c0 = c1;
    }
    for (const RefW& f : fl) { R.order.push_back(f.i); R.bytes.push_back((f.bytes + 15) & ~(size_t)15); }
    return R;
}
static RefPlan ref_tract_positions(const std::vector<size_t>& sizes, size_t budget)  // an oversize window is dropped first
{
    RefPlan R; std::vector<RefW> ws;
    for (size_t i = 0; i < sizes.size(); ++i) {
        const size_t bytes = sizes[i];
        if (bytes > budget) { R.oversize.push_back((int32_t)i); continue; }
        ws.push_back({(int)i, bytes});
    }
    for (size_t c0 = 0; c0 < ws.size();) {
        size_t c1 = c0, bytes = 0;
        while (c1 < ws.size() && bytes + ws[c1].bytes <= budget) bytes += ws[c1++].bytes;          // (every window fits alone)
        R.pieces.push_back({c0, c1, bytes});
        c0 = c1;
    }
    for (const RefW& w : ws) { R.order.push_back(w.i); R.bytes.push_back(w.bytes); }
    return R;
}
static RefPlan ref_state_stats(const std::vector<size_t>& sizes, size_t budget)      // as tract_positions, its own copy
{
    RefPlan R; std::vector<RefW> ws;
    for (size_t i = 0; i < sizes.size(); ++i) {
        const size_t bytes = sizes[i];
        if (bytes > budget) { R.oversize.push_back((int32_t)i); continue; }
        ws.push_back({(int)i, bytes});
    }
    for (size_t c0 = 0; c0 < ws.size();) {
        size_t c1 = c0, bytes = 0;
        while (c1 < ws.size() && bytes + ws[c1].bytes <= budget) bytes += ws[c1++].bytes;          // (every window fits alone)
        R.pieces.push_back({c0, c1, bytes});
        c0 = c1;
    }
    for (const RefW& w : ws) { R.order.push_back(w.i); R.bytes.push_back(w.bytes); }
    return R;
}
static RefPlan ref_state_posteriors(const std::vector<size_t>& sizes, size_t budget) // oversize windows in front with 0 bytes, 8192 a piece
{
    RefPlan R; std::vector<RefW> ws, over;
    for (size_t i = 0; i < sizes.size(); ++i) {
        const size_t bytes = sizes[i];
        if (bytes > budget) { R.oversize.push_back((int32_t)i); over.push_back({(int)i, 0}); continue; }
        ws.push_back({(int)i, bytes});
    }
    ws.insert(ws.begin(), over.begin(), over.end());
    for (size_t c0 = 0; c0 < ws.size();) {
        size_t c1 = c0, bytes = 0;
        while (c1 < ws.size() && c1 - c0 < 8192 && bytes + ws[c1].bytes <= budget) bytes += ws[c1++].bytes;          // (every window fits alone)
        R.pieces.push_back({c0, c1, bytes});
        c0 = c1;
    }
    for (const RefW& w : ws) { R.order.push_back(w.i); R.bytes.push_back(w.bytes); }
    return R;
}

static bool same_plan(const PiecePlan& P, const RefPlan& R)
{
    if (P.order != R.order || P.bytes != R.bytes || P.oversize != R.oversize || P.pieces.size() != R.pieces.size()) return false;
    for (size_t k = 0; k < P.pieces.size(); ++k)
        if (P.pieces[k].first != R.pieces[k].first || P.pieces[k].last != R.pieces[k].last || P.pieces[k].bytes != R.pieces[k].bytes) return false;
    return true;
}
// what every plan holds, whatever the policy: the pieces tile the order, none is empty, every window is in the order or oversize
static bool sound_plan(const PiecePlan& P, size_t n, size_t budget, Oversize policy)
{
    size_t at = 0;
    for (const Piece& pc : P.pieces) {
        if (pc.first != at || pc.last <= pc.first) return false;
        size_t sum = 0;
        for (size_t k = pc.first; k < pc.last; ++k) sum += P.bytes[k];
        if (sum != pc.bytes || (pc.bytes > budget && !(policy == OVERSIZE_ALONE && pc.last - pc.first == 1))) return false;
        at = pc.last;
    }
    if (at != P.order.size() || P.bytes.size() != P.order.size()) return false;
    std::vector<int> seen(n, 0);
    for (int32_t i : P.order) ++seen[(size_t)i];
    if (policy == OVERSIZE_LEFT_OUT) for (int32_t i : P.oversize) ++seen[(size_t)i];
    for (int v : seen) if (v != 1) return false;
    return policy != OVERSIZE_ALONE || P.oversize.empty();
}
static int plan_cases = 0;
static bool seen_rounding_differs = false;
static void planner_case(const std::vector<size_t>& raw, size_t budget)
{
    ++plan_cases;
    std::vector<size_t> rounded(raw);
    for (size_t& b : rounded) b = (b + 15) & ~(size_t)15;
    const PiecePlan units = plan_pieces(raw, budget, OVERSIZE_ALONE), fmod = plan_pieces(rounded, budget, OVERSIZE_ALONE);
    CHECK(same_plan(units, ref_unit_pass(raw, budget)) && sound_plan(units, raw.size(), budget, OVERSIZE_ALONE));
    CHECK(same_plan(fmod, ref_flank_mod_pass(raw, budget)) && sound_plan(fmod, raw.size(), budget, OVERSIZE_ALONE));
    if (units.pieces.size() != fmod.pieces.size()) seen_rounding_differs = true;
    // the traced passes and the posteriors hand in sizes they rounded themselves; the raw ones are as good a list
    const std::vector<size_t>* const lists[2] = {&raw, &rounded};
    for (const std::vector<size_t>* sizes : lists) {
        const PiecePlan out = plan_pieces(*sizes, budget, OVERSIZE_LEFT_OUT), front = plan_pieces(*sizes, budget, OVERSIZE_IN_FRONT, 8192);
        CHECK(same_plan(out, ref_tract_positions(*sizes, budget)) && same_plan(out, ref_state_stats(*sizes, budget)) && sound_plan(out, sizes->size(), budget, OVERSIZE_LEFT_OUT));
        CHECK(same_plan(front, ref_state_posteriors(*sizes, budget)) && sound_plan(front, sizes->size(), budget, OVERSIZE_IN_FRONT));
        for (const Piece& pc : front.pieces) CHECK(pc.last - pc.first <= 8192);
    }
}
static void planner_checks()
{
    const size_t B = 4096;
    // the named cases: no windows, sizes of 0, sums and single windows at the budget and a byte over, sizes that are no multiple of 16,
    // every window oversize
    planner_case({}, B);
    planner_case({0}, B); planner_case({0, 0, 0}, B); planner_case({0, B, 0}, B); planner_case({0, B + 1, 0}, B);
    planner_case({B}, B); planner_case({B + 1}, B); planner_case({B, B}, B); planner_case({B + 1, B + 1, B + 1}, B);
    planner_case({1000, 3096}, B); planner_case({1000, 3097}, B); planner_case({1000, 2000, 1096, 1}, B); planner_case({1000, 2000, 1097}, B);
    planner_case({4081, 1}, B); planner_case({4081}, B); planner_case({4090, 4090}, B); planner_case({100, 100, 100}, 300); planner_case({100, 100, 100}, 299);
    planner_case({8, 8}, 16); planner_case({9, 7}, 16); planner_case({1, 1, 1}, 32); planner_case({1, 1, 1}, 31);
    planner_case({5000, 1, 6000, 2, 7000}, B); planner_case({1, 5000, 2}, B);
    // an oversize window rides alone where the policy lets it, is left out or carried in front with no bytes elsewhere
    {
        const std::vector<size_t> sizes = {16, 5008, 32, 4096, 16};
        const PiecePlan a = plan_pieces(sizes, B, OVERSIZE_ALONE), o = plan_pieces(sizes, B, OVERSIZE_LEFT_OUT), f = plan_pieces(sizes, B, OVERSIZE_IN_FRONT, 8192);
        CHECK(a.pieces.size() == 5 && a.pieces[1].first == 1 && a.pieces[1].last == 2 && a.pieces[1].bytes == 5008 && a.pieces[2].bytes == 32 && a.pieces[3].bytes == 4096 && a.oversize.empty());
        CHECK(o.order == std::vector<int32_t>({0, 2, 3, 4}) && o.oversize == std::vector<int32_t>({1}) && o.pieces.size() == 3 && o.pieces[0].bytes == 48 && o.pieces[1].bytes == 4096);
        CHECK(f.order == std::vector<int32_t>({1, 0, 2, 3, 4}) && f.bytes[0] == 0 && f.oversize == std::vector<int32_t>({1}) && f.pieces.size() == 3 && f.pieces[0].last == 3 && f.pieces[0].bytes == 48);
    }
    // the cap of the state posteriors: 8193 windows of no bytes are two pieces; without a cap they are one
    {
        const std::vector<size_t> zeros(8193, 0);
        planner_case(zeros, B);
        const PiecePlan f = plan_pieces(zeros, B, OVERSIZE_IN_FRONT, 8192);
        CHECK(f.pieces.size() == 2 && f.pieces[0].last == 8192 && f.pieces[1].last == 8193 && f.pieces[1].bytes == 0);
        CHECK(plan_pieces(zeros, B, OVERSIZE_LEFT_OUT).pieces.size() == 1);
        std::vector<size_t> mixed(8193, 0); mixed[8192] = B + 1; mixed[17] = B;          // the oversize one comes to the front and counts towards the cap
        planner_case(mixed, B);
        CHECK(plan_pieces(mixed, B, OVERSIZE_IN_FRONT, 8192).order[0] == 8192);
    }
    // generated lists: 0 to 40 windows; a list draws from one of several mixes so that zeros, windows at the budget and a byte over,
    // all-oversize lists and sums that land on the budget or a byte over all come up (fixed seed)
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&](uint64_t below) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (size_t)((rng >> 33) % below); };
    const size_t budgets[] = {16, 100, 4096, 65536, (size_t)1 << 33};
    int n_exact = 0, n_over1 = 0, n_all_over = 0;
    for (int t = 0; t < 4000; ++t) {
        const size_t budget = budgets[next(5)], n = next(41), mix = next(6);
        std::vector<size_t> raw(n);
        size_t run = 0;
        for (size_t i = 0; i < n; ++i) {
            size_t b;
            switch (mix) {
            case 0: b = next(budget / 3 + 2); break;                                      // several to a piece, mostly no multiple of 16
            case 1: b = next(4) == 0 ? 0 : next(budget + budget / 4 + 2); break;          // zeros, some oversize
            case 2: b = budget + 1 + next(budget); break;                                 // every window oversize
            case 3: b = next(3) == 0 ? budget : next(2) ? budget + 1 : next(budget + 1); break;
            case 4: b = 16 * next(budget / 48 + 2); break;                                // multiples of 16
            default:                                                                      // runs that end exactly at the budget, or a byte over
                b = next(budget / 2 + 1);
                if (run + b > budget || next(4) == 0) { b = budget - run + next(2); }
                break;
            }
            run = run + b > budget ? 0 : run + b;
            if (run == budget) run = 0;
            raw[i] = b;
        }
        planner_case(raw, budget);
        const PiecePlan p = plan_pieces(raw, budget, OVERSIZE_LEFT_OUT);
        for (const Piece& pc : p.pieces) {
            if (pc.last - pc.first > 1 && pc.bytes == budget) ++n_exact;
            if (pc.last < p.order.size() && pc.bytes + p.bytes[pc.last] == budget + 1) ++n_over1;
        }
        if (n && p.oversize.size() == n) ++n_all_over;
    }
    CHECK(plan_cases > 4000 && n_exact > 50 && n_over1 > 50 && n_all_over > 50 && seen_rounding_differs);

    CHECK(ws_budget(nullptr) == (size_t)8 << 30 && ws_budget("0") == (size_t)8 << 30 && ws_budget("-5") == (size_t)8 << 30 && ws_budget("4096") == 4096);
    CHECK(ws_budget("") == (size_t)8 << 30 && ws_budget("x") == (size_t)8 << 30 && ws_budget("1") == 1);
    // back-pointers: uint16 per (time step, state), T + 1 steps, rounded up to 16 bytes
    CHECK(bp_window_bytes(0, 1) == 16 && bp_window_bytes(0, 8) == 16 && bp_window_bytes(0, 9) == 32);
    CHECK(bp_window_bytes(6, 1) == 16 && bp_window_bytes(6, 9) == 128 && bp_window_bytes(7, 1) == 16 && bp_window_bytes(14, 1) == 32);          // 7, 63, 8, 15 cells
    CHECK(bp_window_bytes(((int64_t)1 << 21) - 1, 4096) == (size_t)1 << 34);
    // the three 21-bit counters of a tract payload, each at 0 and at 2^21 - 1
    const int64_t top = ((int64_t)1 << VIT_TRACT_BITS) - 1;
    for (int mask = 0; mask < 8; ++mask) {
        uint64_t pay = 0;
        for (int j = 0; j < VIT_TRACTS_MAX; ++j) if (mask >> j & 1) pay += (uint64_t)top << (VIT_TRACT_BITS * j);
        for (int j = 0; j < VIT_TRACTS_MAX; ++j) CHECK(vit_tract_count(pay, j) == ((mask >> j & 1) ? top : 0));
    }
    const uint64_t pay = (uint64_t)5 | (uint64_t)70000 << VIT_TRACT_BITS | (uint64_t)1 << (2 * VIT_TRACT_BITS);
    CHECK(vit_tract_count(pay, 0) == 5 && vit_tract_count(pay, 1) == 70000 && vit_tract_count(pay, 2) == 1);
    CHECK(vit_tract_count(~(uint64_t)0, 2) == top);          // the bit above the three counters is not theirs
}

int main()
{
    planner_checks();
    carve_checks();
    packer_checks();
    stats_checks();
    decode_order_checks();

    // a read that ends in the repeat: window of 1000 observations from sample 5000, section from observation 40 to 979, 20 behind it
    strq_anchored a = anchored_record(2, 5000, 1000, 0, 44, -1, -1234.5, 41, 981);
    CHECK(a.kind == 2 && a.status == 0 && a.count == 43 && a.log_p == -1234.5 && a.begin == 5040 && a.end == 5980 && a.free_samples == 20);
    // a read that starts in it: 7 observations in front of the section
    a = anchored_record(3, 0, 800, 0, 30, 0, -99.0, 8, 500);
    CHECK(a.kind == 3 && a.status == 0 && a.count == 30 && a.begin == 7 && a.end == 499 && a.free_samples == 7);
    // the section reaches the end of the window (no emission behind it)
    a = anchored_record(2, 10, 100, 0, 5, -1, -1.0, 11, 0);
    CHECK(a.status == 0 && a.begin == 20 && a.end == 110 && a.free_samples == 0);
    // the longest window a MARK decode takes, at the far end of a read of 2^30 samples
    const int64_t T = ((int64_t)1 << 21) - 1, first = ((int64_t)1 << 30) - T;
    a = anchored_record(2, first, T, 0, 300000, -1, -1e7, 1, T);
    CHECK(a.status == 0 && a.begin == first && a.end == first + T - 1 && a.free_samples == 1 && a.count == 299999);
    // no path, a window too long for the marks, marks that describe no such path: the kind stays, everything else is zero
    CHECK(zero_but_kind(anchored_record(2, 5000, 1000, 1, 44, -1, -5.0, 41, 981), 2, 1));
    CHECK(zero_but_kind(anchored_record(3, 0, (int64_t)1 << 22, 2, 44, 0, -5.0, 41, 981), 3, 2));
    CHECK(zero_but_kind(anchored_record(2, 0, 1000, 0, 44, -1, -5.0, 0, 0), 2, 1));
    CHECK(zero_but_kind(anchored_record(2, 0, 1000, 0, 44, -1, -5.0, 500, 400), 2, 1));
    CHECK(zero_but_kind(anchored_record(3, 0, 1000, 0, 44, 0, -5.0, 10, 1002), 3, 1));

    // rows: sized once, a read put back to its initial values, reads outside the batch ignored
    ReadRows rows; rows.size_reads(3);
    CHECK(rows.anch.size() == 3 && rows.results.size() == 3 && rows.conf.size() == 9);
    rows.anch[1] = anchored_record(2, 5000, 1000, 0, 44, -1, -1234.5, 41, 981); rows.units[1].push_back(7); rows.mod[1] = "01";
    rows.clear_read(1); rows.clear_read(-1); rows.clear_read(3);
    CHECK(zero_but_kind(rows.anch[1], 0, 0) && rows.units[1].empty() && rows.mod[1] == "-");
    rows.size_reads(0);
    CHECK(rows.anch.empty());
    Extras ex;
    CHECK(!ex.anch && ex.anch_min == 0.0 && !ex.units && !ex.conf && !ex.llr);

    // grouping: one launch per (route, shape), tasks of a launch in their own order
    std::vector<GroupItem> items = {{0, 9, 100}, {0, 5, 300}, {0, 9, 200}, {1, 5, 50}, {0, 5, 10}};
    const Grouping G = group_items(items);
    CHECK(G.groups.size() == 3 && G.order.size() == 5);
    CHECK(G.groups[0].shape == 5 && G.groups[0].route == 0 && G.groups[0].count == 2 && G.groups[0].max_cells == 300 && G.groups[0].first == 0);
    CHECK(G.groups[1].shape == 9 && G.groups[1].count == 2 && G.groups[1].first == 2 && G.groups[2].route == 1 && G.groups[2].first == 4);
    for (size_t k = 0; k < items.size(); ++k) CHECK(G.order[(size_t)G.pos[k]] == (int32_t)k);
    CHECK(group_items(std::vector<GroupItem>()).groups.empty());
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("detect_plan ok");
    return 0;
}
