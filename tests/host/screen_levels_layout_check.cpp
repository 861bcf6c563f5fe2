// Stand-alone host program over strique_amd/csrc/screen_levels_layout.h (no HIP): the level image of the coarse two-flank screen's score
// tables.  For every (lane, class, level) -- levels inside and outside the image's range, ranges that start at level 0, lie in the
// middle and end at level 255, a range of one level -- the address rule equals a direct restatement, no two (lane, class) pairs share a
// byte of a row, every byte a lane reads lies in bank lane mod 32, every address stays below the bytes the host allocates, the
// pre-evaluated clamp picks the band entry the run-time clamp of the other layouts would, the LDS budget arithmetic holds and the
// fall-back triggers exactly above the limit; the byte scale of STRique's parameters is 6 with every entry <= 255, and parameters
// whose hh / MERGE is no integer at any byte scale are refused.  Built and run under ASan/UBSan by
// tests/test_screen_levels_layout_host.py; exits 0 when every check holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../strique_amd/csrc/screen_levels_layout.h"

namespace sv = strq::screen_levels;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { if (failures < 20) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

// the rule, restated: row = clamp(level) - lvl0; a row is three sub-rows of 128 bytes; lanes 0 .. 31 own the low halves of dwords
// 0 .. 31 of every sub-row, lanes 32 .. 63 the high halves; classes 0 1 | 2 3 | 4 are the bytes of the lane's halves in sub-rows 0 1 2
static int restated(int lane, int c, int level, int lvl0, int lvl1)
{
    const int row = std::min(std::max(level, lvl0), lvl1) - lvl0;
    const int dword = lane % 32, half = lane / 32, sub = c / 2, byte = c % 2;
    return row * 384 + sub * 128 + dword * 4 + half * 2 + byte;
}

static void check_range(int lvl0, int lvl1)
{
    const int rows = lvl1 - lvl0 + 1;
    const uint32_t r = sv::pack_range(lvl0, lvl1);
    CHECK(sv::range_lo(r) == lvl0 && sv::range_hi(r) == lvl1 && sv::rows_of(r) == rows);
    const size_t bytes = sv::bytes(rows);
    CHECK(bytes == (size_t)rows * 384);
    std::vector<int> owner(bytes, -1);
    for (int lane = 0; lane < 64; ++lane)
        for (int c = 0; c < sv::CPL; ++c)
            for (int level = 0; level < 256; ++level) {
                const int a = sv::address(lane, c, level, lvl0, lvl1);
                CHECK(a == restated(lane, c, level, lvl0, lvl1));
                CHECK(a >= 0 && (size_t)a < bytes);
                CHECK((a / 4) % 32 == lane % 32);                     // the bank of every byte a lane reads
                // what the kernel computes: 3 x the 16-bit half of the level pair + the lane's slot, then the class's immediate offset
                const int q = sv::scaled_level(level, lvl0, lvl1);
                CHECK(q >= 0 && q < 65536 && q % sv::SUB_BYTES == 0);
                CHECK(sv::column_address(q, lane) + sv::class_offset(c) == a);
                if (level >= lvl0 && level <= lvl1) {                 // one owner per byte
                    const int id = lane * sv::CPL + c;
                    CHECK(owner[(size_t)a] == -1 || owner[(size_t)a] == id);
                    owner[(size_t)a] = id;
                } else CHECK(a == sv::address(lane, c, level < lvl0 ? lvl0 : lvl1, lvl0, lvl1));      // outside: the row of the nearest end
            }
    size_t used = 0;
    for (int o : owner) used += o >= 0;
    CHECK(used == (size_t)rows * 64 * sv::CPL);                       // 320 of the 384 bytes of a row: the high byte of sub-row 2 is free
}

static void check_band_index()
{
    // entry = table[off + clamp(level, lo, lo + w1) - lo]: the clamp the other layouts evaluate per look-up
    const int bands[][2] = {{0, 0}, {0, 44}, {100, 46}, {211, 44}, {255, 0}, {0, 255}, {37, 176}};
    for (const auto& b : bands) {
        const uint32_t d = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | (1234u << 16);
        CHECK(sv::desc_lo(d) == b[0] && sv::desc_w1(d) == b[1] && sv::desc_off(d) == 1234);
        for (int level = 0; level < 256; ++level)
            CHECK(sv::band_index(d, level) == std::min(std::max(level, b[0]), b[0] + b[1]) - b[0]);
    }
    // the span of two tables, and levels beyond it: every class is clamped there, so the row of the nearest end holds its entry
    const uint32_t j = sv::join_ranges(sv::pack_range(40, 200), sv::pack_range(33, 180));
    CHECK(sv::range_lo(j) == 33 && sv::range_hi(j) == 200);
    CHECK(sv::rows_of(sv::join_ranges(sv::pack_range(0, 0), sv::pack_range(0, 0))) == 1);
    CHECK(sv::rows_of(sv::join_ranges(sv::pack_range(0, 255), sv::pack_range(7, 9))) == 256);
}

static void check_budget()
{
    // granules of 1280 bytes, 128 per CU; the four-wave Viterbi workgroup beside the screen takes 17; two screen workgroups of eight
    // waves share the rest, each with 4 bytes of static LDS on top of its image
    auto granules = [](size_t bytes) { return (int)((bytes + 1279) / 1280); };
    CHECK(granules(4 * 5200) == 17);
    CHECK(17 + 2 * granules(sv::bytes(sv::MAX_ROWS) + 4) <= 128);
    CHECK(17 + 2 * granules(sv::bytes(sv::MAX_ROWS + 1) + 4) > 128);
    CHECK(sv::fits(1) && sv::fits(sv::MAX_ROWS) && !sv::fits(sv::MAX_ROWS + 1) && !sv::fits(256) && !sv::fits(0));
    CHECK(sv::MAX_BYTES == sv::bytes(sv::MAX_ROWS) && sv::MAX_BYTES + 4 <= 160 * 1024 / 2);
    CHECK(sv::SEG == 8 && sv::MERGE == 3 && sv::CPL == 5 && sv::ROW_BYTES == 384);
    CHECK(255 * sv::SUB_BYTES < 65536);                               // the scaled level fits the 16-bit half of the level pair
}

static void check_scale()
{
    // STRique: e_h = -1, e_v = -16, dist_offset = 16
    const int sc = sv::byte_scale(-1.0, -16.0, 16.0);
    CHECK(sc == 6);
    const int hh = 6, v = 96;
    CHECK(hh % sv::MERGE == 0);
    for (int i = 0; i <= 16000; ++i) {                                // every score 0 .. dist_offset in steps of 0.001
        const double s = i * 0.001;
        const int e = (int)std::ceil(s * sc) + hh + v;
        CHECK(e >= hh + v && e <= 255);
    }
    CHECK((int)std::ceil(16.0 * sc) + hh + v == 198);
    // the next integer scales fail one condition each: 7 is no multiple of MERGE, 9 overflows the byte
    CHECK((int)std::ceil(16.0 * 9) + 9 + 144 > 255);
    // half the gap scores: -0.5, -8, 8 -> sc = 12 (hh = 6, v = 96, entries <= 198)
    CHECK(sv::byte_scale(-0.5, -8.0, 8.0) == 12);
    // hh / MERGE is no integer at any scale that fits a byte: e_h = -1, e_v = -100 (v alone exceeds 255 from sc = 3 on, hh = 1, 2 are no multiples of 3)
    CHECK(sv::byte_scale(-1.0, -100.0, 16.0) == 0);
    // a vertical gap that alone does not fit a byte at the smallest scale
    CHECK(sv::byte_scale(-3.0, -200.0, 64.0) == 0);
}

int main()
{
    check_range(0, 0);            // a read with a single level
    check_range(0, 136);          // lvl0 at 0
    check_range(37, 205);         // the benchmark's reads: 167 .. 172 rows in the middle of the level range
    check_range(255 - 182, 255);  // lvl1 at 255, the tallest image that fits
    check_range(255, 255);
    check_band_index();
    check_budget();
    check_scale();
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("screen_levels_layout ok\n");
    return 0;
}
