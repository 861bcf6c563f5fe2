// Stand-alone host program over strique_amd/csrc/detect_plan.h (no HIP): the anchored record from the marks of a MARK decode, the
// per-read rows, the grouping of tasks, the layout of a workspace (Carve).  Built and run under ASan/UBSan by tests/test_detect_plan_host.py; exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../strique_amd/csrc/detect_plan.h"

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

int main()
{
    carve_checks();

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
