// Stand-alone host program over strique_amd/csrc/screen_lds_layout.h (no HIP): the lane-major LDS image of the two-flank screen's score
// tables.  For flanks of 145/145, 100/140, 1/145 and 158/158 classes, with bands that touch level 0 and level 255: every look-up of a
// lane falls in the lane's own bank and half, no two (lane, row) pairs share a slot, row 0 is reached by padding classes only, every
// address stays below the size the host allocates, and the fallback to the class rows triggers exactly above the limit.  Built and run
// under ASan/UBSan by tests/test_screen_lds_layout_host.py; exits 0 when every check holds.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../strique_amd/csrc/screen_lds_layout.h"

using namespace strq;
namespace sl = strq::screen_lanes;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { if (failures < 20) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % n; }

// band descriptors of a flank of k classes: bands of about `width` levels around a random centre, cut at levels 0 and 255; the first class
// starts at level 0, the second ends at level 255, the third spans one level, row offsets as the table kernel packs them (a repeated
// k-mer shares the row of its first occurrence: class 7 repeats class 5, inside one lane)
static std::vector<uint32_t> flank(int k, int width, int* need)
{
    std::vector<uint32_t> d(k);
    int off = 0; *need = 0;
    for (int c = 0; c < k; ++c) {
        int centre = (int)rnd(256), lo = std::max(0, centre - width / 2), hi = std::min(255, centre + width / 2 + (int)rnd(3));
        if (c == 0) { lo = 0; hi = std::min(255, width); }
        if (c == 1) { hi = 255; lo = std::max(0, 255 - width); }
        if (c == 2) { lo = hi = 200; }
        d[c] = (uint32_t)lo | ((uint32_t)(hi - lo) << 8) | ((uint32_t)off << 16);
        if (c == 7) d[c] = d[5];
        else off += hi - lo + 1;
        *need = std::max(*need, sl::desc_w1(d[c]) + 1);
    }
    return d;
}

static void one_read(int ka, int kb, int width)
{
    int need[2];
    const std::vector<uint32_t> desc[2] = {flank(ka, width, &need[0]), flank(kb, width, &need[1])};
    const int k[2] = {ka, kb};
    const int rows_host = sl::rows_bound(need[0], need[1]);
    const size_t size = sl::bytes(rows_host);
    std::vector<int> owner(size / 2, -1);          // 16-bit slots of the image: lane * 65536 + row
    int tallest = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const int f = lane >> 5, lf = lane & 31;
        uint32_t mine[sl::CPL] = {0, 0, 0, 0, 0};
        int nc = 0, rowbase[sl::CPL];
        for (int c = 0; c < sl::CPL; ++c) if (lf * sl::CPL + c < k[f]) mine[nc++] = desc[f][lf * sl::CPL + c];
        const int rows = sl::row_bases(mine, nc, rowbase);
        tallest = std::max(tallest, rows);
        CHECK(rows <= rows_host);
        // the lane's slots, row by row: its own, inside the image, in its bank and half
        for (int r = 0; r < rows; ++r) {
            const int a = sl::slot(lane) + r * sl::ROW_BYTES;
            CHECK(a >= 0 && (size_t)a + 2 <= size && a % 2 == 0);
            if (a < 0 || (size_t)a + 2 > size) continue;
            CHECK(owner[a / 2] == -1);
            owner[a / 2] = lane * 65536 + r;
            CHECK((a / 4) % 32 == (lane & 31) && (a % 4) / 2 == (lane >> 5));
        }
        int expect_base = 1;
        for (int c = 0; c < sl::CPL; ++c) {
            const bool real = c < nc;
            const sl::ClassAddr ca = real ? sl::class_addr(lane, rowbase[c], mine[c]) : sl::padding_addr(lane);
            if (real) { CHECK(rowbase[c] == expect_base); expect_base += sl::desc_w1(mine[c]) + 1; }
            else CHECK(rowbase[c] == 0);
            CHECK(ca.lo2 >= 0 && ca.hi2 <= 255 * sl::ROW_BYTES && ca.hi2 < 65536);
            for (int level = 0; level < 256; ++level) {
                const int a = sl::address(ca, level);
                CHECK(a >= 0 && (size_t)a + 2 <= size);
                CHECK((a / 4) % 32 == (lane & 31) && (a % 4) / 2 == (lane >> 5));          // bank and half of the lane, whatever class or level
                const int row = a / sl::ROW_BYTES;
                if (!real) { CHECK(row == 0); continue; }
                CHECK(row >= 1);                                                            // row 0: padding classes only
                const int lo = sl::desc_lo(mine[c]), w1 = sl::desc_w1(mine[c]);
                const int i = std::min(std::max(level, lo), lo + w1) - lo;                   // the band entry the clamp selects
                CHECK(a == sl::entry_address(lane, rowbase[c], i));
                CHECK(a >= 0 && (size_t)a + 2 <= size && owner[a / 2] == lane * 65536 + rowbase[c] + i);
            }
        }
        CHECK(expect_base == rows);
    }
    CHECK(sl::bytes(tallest) <= size);
}

static void limit()
{
    // the fallback triggers exactly above MAX_ROWS
    CHECK(sl::fits(sl::MAX_ROWS) && !sl::fits(sl::MAX_ROWS + 1) && sl::fits(1));
    int widest_ok = 0;
    for (int need = 1; need <= 256; ++need) {
        const bool ok = sl::fits(sl::rows_bound(need, 1));
        CHECK(ok == (1 + sl::CPL * need <= sl::MAX_ROWS));
        CHECK(ok == sl::fits(sl::rows_bound(1, need)));
        if (ok) widest_ok = need;
        CHECK(ok == (sl::bytes(sl::rows_bound(need, 1)) <= sl::MAX_BYTES));
    }
    CHECK(widest_ok == (sl::MAX_ROWS - 1) / sl::CPL && widest_ok >= 44);          // the benchmark's bands (about 44 levels) fit
    // the budget behind MAX_ROWS: four screen workgroups (image + 4 bytes of static LDS) beside a four-wave Viterbi workgroup of
    // 4 x 5200 bytes in the 160 KB of a CU, handed out in granules of 1280 bytes; alone, five such workgroups fit
    auto granules = [](size_t b) { return (b + 1279) / 1280; };
    CHECK(4 * granules(sl::MAX_BYTES + 4) + granules(4 * 5200) <= granules(160 * 1024));
    CHECK(granules(160 * 1024) * 1280 == 160 * 1024);
    CHECK(5 * granules(sl::bytes(sl::rows_bound(46, 46)) + 4) <= granules(160 * 1024));
}

int main()
{
    const int shapes[4][2] = {{145, 145}, {100, 140}, {1, 145}, {158, 158}};
    for (const auto& s : shapes)
        for (int width : {1, 12, 44, 52, 120, 255}) one_read(s[0], s[1], width);
    limit();
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("screen_lds_layout ok\n");
    return 0;
}
