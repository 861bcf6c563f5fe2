// Internal: the lane-major LDS image of the two-flank screen's score tables (screen_kernels.hip: Screen2) -- what
// the kernel, the host's LDS sizing and the host check (tests/host/screen_lds_layout_check.cpp) agree on.  Plain C++, no HIP
// header: the host check compiles it alone.
//
// The image is a 2-D array of rows of 128 bytes = 32 dwords = one pass over the 32 LDS banks.  Lane l owns ONE 16-bit slot of
// every row: lanes 0 .. 31 (prefix flank) the low halves of dwords 0 .. 31, lanes 32 .. 63 (suffix flank) the high halves of the
// same dwords.  A lane's classes (STRQ_SCREEN2_CPL = 5 whole classes per lane) are stacked down its own column: row 0 is zero
// for every lane (what a class beyond the flank scores), class c starts at rowbase[c] = 1 + the band rows of the lane's
// earlier classes, entry i of its band (level lo + i) sits in row rowbase[c] + i.  Whatever class and level a lane looks up,
// its address falls in bank (base / 4 + (l & 31)) mod 32: the 32 lanes of a lane group of ds_read_u16 hit 32 different banks,
// and the two flanks are in different lane groups -- no bank conflict by construction, where the ragged class rows of the
// row layout put the lanes on effectively random banks.
// A class shared by two lanes, or repeated inside one lane, is stored once per occurrence: the image is larger than the row
// layout's (which stores a repeated k-mer's row once), 128 bytes per row of the TALLEST lane.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STRQ_LAYOUT_HD __host__ __device__ __forceinline__
#else
#define STRQ_LAYOUT_HD inline
#endif

namespace strq {
namespace screen_lanes {

constexpr int ROW_BYTES = 128;           // one 16-bit slot per lane
constexpr int ROW_SHIFT = 7;             // a level pre-scaled by ROW_BYTES is its row offset in bytes: 255 * 128 = 32 640 fits a 16-bit half
constexpr int CPL = 5;                   // classes per lane (STRQ_SCREEN2_CPL)
static_assert(ROW_BYTES == 1 << ROW_SHIFT && 255 * ROW_BYTES < 65536, "a scaled level has to fit the 16-bit half of the level pair");

// LDS budget.  What counts is the occupancy beside the Viterbi (strq_detect_api.hip: two sub-batches in flight): four screen
// workgroups per CU (one wave per SIMD each: the four-wave Viterbi workgroup's 192 VGPRs leave 320 per SIMD = four screen waves)
// next to one Viterbi workgroup of 4 x G2_LDS_WAVE_BYTES = 20 800 bytes.  LDS is handed out in granules of 1280 bytes on gfx950
// (160 KB = 128 granules): the Viterbi workgroup takes 17, four screen workgroups may take (128 - 17) / 4 = 27 each = 34 560
// bytes, of which 4 are the kernel's static next_group: at most (34 560 - 4) / 128 = 269 rows.  MAX_ROWS = 264 (33 KB) keeps a
// little room; above it the task groups run on the row layout.
constexpr int MAX_ROWS = 264;
constexpr size_t MAX_BYTES = (size_t)MAX_ROWS * ROW_BYTES;

// band descriptor of a class (AlignTask::band_lo): first level | (levels - 1) << 8 | row offset in the float table << 16
STRQ_LAYOUT_HD int desc_lo(uint32_t d) { return (int)(d & 255u); }
STRQ_LAYOUT_HD int desc_w1(uint32_t d) { return (int)((d >> 8) & 255u); }
STRQ_LAYOUT_HD int desc_off(uint32_t d) { return (int)(d >> 16); }

// byte offset of lane l's slot inside every row
STRQ_LAYOUT_HD int slot(int lane) { return (lane & 31) * 4 + (lane >> 5) * 2; }

// Row bases of a lane from the descriptors of its n (0 .. CPL) classes inside the flank; classes beyond the flank (padding)
// get row 0.  Returns the rows the lane's column takes, row 0 included.
STRQ_LAYOUT_HD int row_bases(const uint32_t* desc, int n, int (&rowbase)[CPL])
{
    int rows = 1;
    for (int c = 0; c < CPL; ++c) {
        if (c < n) { rowbase[c] = rows; rows += desc_w1(desc[c]) + 1; }
        else rowbase[c] = 0;
    }
    return rows;
}

// What the kernel keeps per class: the look-up is ds_read_u16 at med3(level * ROW_BYTES, lo2, hi2) + off
struct ClassAddr { int lo2, hi2, off; };
STRQ_LAYOUT_HD ClassAddr class_addr(int lane, int rowbase, uint32_t desc)
{
    const int lo = desc_lo(desc), w1 = desc_w1(desc);
    return ClassAddr{lo * ROW_BYTES, (lo + w1) * ROW_BYTES, slot(lane) + (rowbase - lo) * ROW_BYTES};
}
STRQ_LAYOUT_HD ClassAddr padding_addr(int lane) { return ClassAddr{0, 0, slot(lane)}; }

// byte address (relative to the image) of the entry a lane reads for a class at `level` (0 .. 255): the level is clamped into the band
STRQ_LAYOUT_HD int address(const ClassAddr& a, int level)
{
    const int q = level * ROW_BYTES;
    const int m = q < a.lo2 ? a.lo2 : (q > a.hi2 ? a.hi2 : q);
    return m + a.off;
}
// byte address of entry i of a class's band (what the prologue fills)
STRQ_LAYOUT_HD int entry_address(int lane, int rowbase, int i) { return slot(lane) + (rowbase + i) * ROW_BYTES; }

STRQ_LAYOUT_HD size_t bytes(int rows) { return (size_t)rows * ROW_BYTES; }

// What the host knows before the launch: `need`, the widest band of a flank's table (LutInfo::need).  No lane's column is taller
// than this, whatever the flank's length.
STRQ_LAYOUT_HD int rows_bound(int need_a, int need_b) { return 1 + CPL * (need_a > need_b ? need_a : need_b); }
STRQ_LAYOUT_HD bool fits(int rows) { return rows <= MAX_ROWS; }

}  // namespace screen_lanes
}  // namespace strq
