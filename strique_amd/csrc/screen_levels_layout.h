// Internal: the level image of the coarse two-flank screen's score tables (screen_kernels.hip: screen2_body<..., LDS_LEVELS>,
// DESIGN.md 4.2e) -- what the kernel, the host's LDS sizing and the host check (tests/host/screen_levels_layout_check.cpp) agree
// on.  Plain C++, no HIP header: the host check compiles it alone.
//
// The lane-major image (screen_lds_layout.h) stacks a lane's classes down its column, so a look-up needs the class's own clamp
// (v_med3_i32) and offset (v_add_u32).  Here the image is indexed by LEVEL: one row per level of the read's range [lvl0, lvl1],
// and the row holds, for every lane, the entries of its five classes AT that level -- the band clamp is evaluated when the image
// is filled (entry = table[clamp(level, lo, lo + w1)]), so a column needs ONE address (row offset + the lane's slot) and its
// five scores are plain byte reads off it with immediate offsets.  A byte holds an entry because the kernel works in units of
// T / MERGE: entry = ceil(s sc) + hh + v (not MERGE times that), potential step hh / MERGE -- see byte_scale below.  The entry is
// the same for every merge factor: align_screen6_kernel (MERGE_CLASS = 6, one DP row per class) reads the image align_screen3_kernel reads.
//
// A row is 384 bytes = three sub-rows of 128 bytes = three passes over the 32 LDS banks.  Lane l owns the same 16-bit slot of
// every sub-row as in the lane-major image: lanes 0 .. 31 (prefix flank) the low halves of dwords 0 .. 31, lanes 32 .. 63
// (suffix flank) the high halves.  Classes 0, 1 of the lane are the two bytes of its slot in sub-row 0, classes 2, 3 in sub-row 1,
// class 4 the low byte in sub-row 2 (its high byte is unused): offsets {0, 1, 128, 129, 256} from the column's address, the same
// for every lane.  Whatever level a lane is at, every byte it reads lies in bank (lane & 31) -- the 32 lanes of a lane group hit 32
// banks, the two flanks are in different lane groups: no bank conflict by construction.
// (One dword of four classes per lane and a byte select in the cell's addition was the first plan; v_add_u32_sdwa issues like
// v_med3_i32 on gfx950, not like v_add_u32 -- profiles/screen_level_image.md, gate a -- so the scores are read as bytes.)
//
// The range.  [lvl0, lvl1] spans the bands of the read's two tables (lut_build_kernel reports it per table: LutInfo::lvl): below
// lvl0 every class is clamped to its first entry, above lvl1 to its last, so a level outside the range reads the row of the
// nearest end -- the kernel clamps the levels into the range where it loads them (once per 128 columns and lane, not per step).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STRQ_LEVELS_HD __host__ __device__ __forceinline__
#else
#define STRQ_LEVELS_HD inline
#endif

namespace strq {
namespace screen_levels {

constexpr int SUB_BYTES = 128;           // one 16-bit slot per lane
constexpr int SUBS = 3;                  // sub-rows per level: classes 0 1 | 2 3 | 4
constexpr int ROW_BYTES = SUBS * SUB_BYTES;
constexpr int Q_SHIFT = 7;               // the level pair holds (level - lvl0) * 128 in each 16-bit half; the address is 3 x that
constexpr int CPL = 5;                   // classes per lane (STRQ_SCREEN2_CPL)
constexpr int MERGE = 3;                 // the coarse screen only
constexpr int SEG = 8;                   // waves per workgroup = pieces per read
static_assert(SUB_BYTES == 1 << Q_SHIFT && 255 * SUB_BYTES < 65536, "a scaled level has to fit the 16-bit half of the level pair");

// LDS budget.  As for the lane-major image what counts is the occupancy beside the Viterbi: one four-wave Viterbi workgroup of
// 20 800 bytes = 17 granules of 1280 bytes (160 KB = 128 granules) and four screen waves per SIMD.  An image of ~170 levels does
// not fit four times, so the workgroup has EIGHT waves (eight pieces per read) and two of them share a CU: (128 - 17) / 2 = 55
// granules = 70 400 bytes each, of which 4 are the kernel's static next_group: at most (70 400 - 4) / 384 = 183 rows.
constexpr int MAX_ROWS = 183;
constexpr size_t MAX_BYTES = (size_t)MAX_ROWS * ROW_BYTES;

// band descriptor of a class (AlignTask::band_lo): first level | (levels - 1) << 8 | row offset in the float table << 16
STRQ_LEVELS_HD int desc_lo(uint32_t d) { return (int)(d & 255u); }
STRQ_LEVELS_HD int desc_w1(uint32_t d) { return (int)((d >> 8) & 255u); }
STRQ_LEVELS_HD int desc_off(uint32_t d) { return (int)(d >> 16); }

// the level range of a table as lut_build_kernel packs it (LutInfo::lvl): lvl0 | lvl1 << 8
STRQ_LEVELS_HD uint32_t pack_range(int lvl0, int lvl1) { return (uint32_t)lvl0 | ((uint32_t)lvl1 << 8); }
STRQ_LEVELS_HD int range_lo(uint32_t r) { return (int)(r & 255u); }
STRQ_LEVELS_HD int range_hi(uint32_t r) { return (int)((r >> 8) & 255u); }
// ... and of a read: the span of both tables
STRQ_LEVELS_HD uint32_t join_ranges(uint32_t a, uint32_t b)
{
    const int lo = range_lo(a) < range_lo(b) ? range_lo(a) : range_lo(b), hi = range_hi(a) > range_hi(b) ? range_hi(a) : range_hi(b);
    return pack_range(lo, hi < lo ? lo : hi);
}
STRQ_LEVELS_HD int rows_of(uint32_t r) { return range_hi(r) - range_lo(r) + 1; }

// byte offset of lane l's slot inside every sub-row, and of class c (0 .. CPL - 1) relative to the slot
STRQ_LEVELS_HD int slot(int lane) { return (lane & 31) * 4 + (lane >> 5) * 2; }
STRQ_LEVELS_HD int class_offset(int c) { return (c >> 1) * SUB_BYTES + (c & 1); }

// what the level pair holds for `level`: the row, clamped into the range, times SUB_BYTES
STRQ_LEVELS_HD int scaled_level(int level, int lvl0, int lvl1)
{
    const int l = level < lvl0 ? lvl0 : (level > lvl1 ? lvl1 : level);
    return (l - lvl0) << Q_SHIFT;
}
// the column's address (relative to the image) from it: what v_mad_u32_u16 computes with the lane's slot as addend
STRQ_LEVELS_HD int column_address(int scaled, int lane) { return scaled * SUBS + slot(lane); }
// byte address of the entry of (lane, class) at `level`
STRQ_LEVELS_HD int address(int lane, int c, int level, int lvl0, int lvl1) { return column_address(scaled_level(level, lvl0, lvl1), lane) + class_offset(c); }
// index into a class's band of the float table that the entry at `level` comes from (the pre-evaluated clamp)
STRQ_LEVELS_HD int band_index(uint32_t desc, int level)
{
    const int lo = desc_lo(desc), w1 = desc_w1(desc);
    return level < lo ? 0 : (level > lo + w1 ? w1 : level - lo);
}

STRQ_LEVELS_HD size_t bytes(int rows) { return (size_t)rows * ROW_BYTES; }
STRQ_LEVELS_HD bool fits(int rows) { return rows >= 1 && rows <= MAX_ROWS; }

// The byte scale: the largest integer sc at which -ext_h sc and -ext_v sc are integers, hh = -ext_h sc is a multiple of MERGE (the
// kernel's potential step is hh / MERGE) and the largest entry ceil(dist_offset sc) + hh + v fits a byte.  0: none (the flank keeps
// the lane-major image and its power-of-two scale).  STRique's parameters (-1, -16, 16) give 6: hh = 6, v = 96, entries <= 198.
// `merge`: the flank rows per DP row of the kernel that reads the image -- MERGE, or MERGE_CLASS (one DP row per k-mer class:
// align_screen6_kernel).  The entry does not depend on it, only the divisibility of hh: STRique's parameters give 6 for both.
constexpr int MERGE_CLASS = 6;
constexpr STRQ_LEVELS_HD bool merge_ok(int merge) { return merge == MERGE || merge == MERGE_CLASS; }
inline int byte_scale(double ext_h, double ext_v, double dist_offset, int merge = MERGE)
{
    for (int sc = 255; sc >= 1; --sc) {
        const double hh = -ext_h * sc, v = -ext_v * sc;
        if (hh != (double)(long)hh || v != (double)(long)v || hh < merge) continue;
        if ((long)hh % merge != 0) continue;
        const double top = dist_offset * sc;
        const long smax = (long)top + ((double)(long)top < top ? 1 : 0);
        if ((double)smax + hh + v > 255.0) continue;
        return sc;
    }
    return 0;
}

}  // namespace screen_levels
}  // namespace strq
