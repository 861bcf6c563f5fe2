// Internal: what host and device agree on about the profile-HMM decodes -- the device images of a model and of a window, the
// decode modes, and the table of kernel shapes with the functions that choose among them.  Plain C++, no HIP header: the host
// check (tests/host/vit_shapes_check.cpp) compiles it alone.  Launch declarations: viterbi_kernels.h.
#pragma once
#include <stdint.h>
#include <type_traits>
#include <utility>

namespace strq {

// Device image of a baked model (strique_amd/hmm.py: bake), laid out for one wave64.
// Every lane owns up to `epl` emitting and `spl` silent states (slot-major: entry slot*64 + lane).
// With layout hints (strq_model_create) a state sits in the lane of its profile position, so that
// the j-th in-edge of all lanes of a slot reads consecutive LDS cells (no bank conflicts);
// otherwise states are dealt to slots by descending in-degree.
// Silent states are laid out in chains: when the highest-numbered silent predecessor of a silent
// state is free, the pair becomes chain neighbours and that edge leaves the edge list (chain_src /
// chain_logp).  A chain zig-zags through the silent slots: position p sits in lane p / spl, slot p % spl.
// In-edge j of the state owned by (slot, lane) is entry (base[slot] + j) * 64 + lane of
// edge_src / edge_logp; padding edges point at the extra cell v[n_states] == -inf.
// Register-resident layout of a profile chain (viterbi_g2_kernel): the model's states as ONE chain of positions g, two
// positions per lane (g = 2 * lane + parity), every position holding at most a match-type state M_g, an insert-type state
// I_g (both emitting) and a delete-type silent state D_g.  All in-edges of the regular part connect a position with itself
// or its predecessor, so a time step needs the lane's own previous values and those of lane - 1 -- no gathers:
//   M_g <- M_{g-2}, I_{g-1}, M_{g-1}, I_g, M_g, [B0], D_{g-1}             (B0 only at even g)
//   I_g <- I_g, M_g, D_g
//   D_g <- I_{g-1}, M_{g-1}, [B1] (this time step's values; B1 only at even g), then its chain predecessor D_{g-1}
// in this order -- which must be the ascending order of the source states, the order the oracle breaks ties in; B0 / B1 are
// two designated emitting states (STRique: the dummy states that close the repeat loop) whose values are broadcast.
// Round 4: an insert-type state has three columns, not seven.  What bake() splices out of STRique's graph -- the silent
// hubs repeat.e1 (in front of dummy1) and repeat.s1 (in front of the first insert of the repeat unit), scripts/STRique.py:
// 339-344 -- comes back in the IMAGE as a virtual delete-type state at a free position (the repeat unit has no delete
// states): dummy1 <- V <- {last insert, last match of the unit}, and repeat0i <- {itself, repeat0m, V' <- {dummy1, last
// prefix delete}}.  A virtual state forwards with log-probability 0.0: x + lp + 0.0 == x + lp bit for bit, the payload of a
// silent state is its predecessor's, and the relayed sources are the LAST of their target's in-edges in evaluation order
// and adjacent, so that every tie is broken as in the baked model (g2_layout checks all of it and refuses otherwise).
// Rows of `lp` (64 doubles each, -inf where a lane has no such edge): see G2_ROW_* below.
struct VitG2 {
    const double* lp;            // G2_ROWS x 64
    const double* em;            // [slot][a | b | c][lane]: emission parameters of the emitting slots (Me, Mo, Ie, Io), as in VitModel
    const int32_t* kind;         // [slot][lane]: 0 none, 1 Normal, 2 Uniform
    const int32_t* own;          // [6][lane]: state of Me, Mo, Ie, Io, De, Do; -1 none, -2 a virtual relay state
    const int32_t* inc;          // [4][lane]: count_inc of the emitting states
    const int32_t* tag;          // [4][lane]: state_tag == 1
    int32_t bc_slot[2], bc_lane[2];      // broadcast sources B0 (slot 0 / 1: feeds match-type states) and B1 (slot 2 / 3: feeds delete-type states); lane -1: none
    int32_t start_slot, start_lane, end_slot, end_lane;      // silent slots 0 (even g) / 1 (odd g)
    const uint64_t* mark_add;    // [4][lane] or null: what an emission of (slot, lane) adds to the 64-bit payload of a mark decode (see G2_MARK_*)
    uint64_t hub_mask;           // lanes whose even delete slot is a virtual relay that lets its target win a tie when the relay's own winner was one of its gather columns
};
// Payload of a mark decode on this layout (VIT_MARK: the modification pass needs the stretch of the window decoded into the
// repeat section, scripts/STRique.py:608): three counters in one 64-bit integer, every emission adds a per-(slot, lane) constant
// with one 64-bit addition -- [0, 21) emissions from tagged states, [21, 43) visits of counted states, [43, 64) emissions from
// untagged states BEHIND the tagged stretch of the chain.  The model is one-way (prefix -> repeat section -> suffix), so with
// T observations the first tagged emission is observation T - behind - tagged and the first one after the section T - behind.
enum { G2_MARK_COUNT_SHIFT = 21, G2_MARK_BEHIND_SHIFT = 43 };
enum { G2_ROW_ME = 0, G2_ROW_MO = 7, G2_ROW_IE = 13, G2_ROW_IO = 16, G2_ROW_DE = 19, G2_ROW_DO = 22, G2_ROW_CHAIN = 24, G2_ROWS = 26 };

struct VitModel {
    int32_t n_states, n_emit, n_silent, start, end;
    int32_t epl, spl;                 // slots per lane (emitting / silent)
    int32_t e_deg[8], e_base[8];      // padded in-degree and first edge row of every emitting slot
    int32_t s_deg[8], s_base[8];
    int32_t n_edge_rows;
    int32_t single_stage;             // 1: no silent state has a silent predecessor outside its chain
    int32_t n_cells, start_cell, end_cell;   // LDS cells: emitting slot s lane l -> s*64+l, silent -> (epl+s)*64+l, last = -inf
    const int32_t* edge_src;          // n_edge_rows * 64: LDS cell of the source state
    const int32_t* cell_state;        // n_cells: state held by a cell, -1 if none
    const double* edge_logp;          // n_edge_rows * 64
    const int32_t* own_e;             // epl * 64: state owned by (slot, lane) or -1
    const int32_t* own_s;             // spl * 64
    const int32_t* chain_src;         // spl * 64: the chain predecessor of the cell -- the state in (slot - 1, lane), for slot 0 in (spl - 1, lane - 1) -- or -1
    const double* chain_logp;         // spl * 64: log-probability of that chain edge
    const int32_t* emis_kind;         // epl * 64, by owner slot  (0 = padding)
    const double* emis_a;             // mu | lo
    const double* emis_b;             // 1/(2 sigma^2) | hi
    const double* emis_c;             // -log(sigma sqrt(2pi)) | -log(hi - lo)
    const int32_t* count_inc;         // n_states + 1, by state
    const int32_t* state_tag;         // n_states + 1, by state
    double uni_lo_max, uni_hi_min;    // tightest bounds of the uniform emissions: observations inside them need no range test
    int32_t rec_state;                // the hub state (tag 2) with an edge into `end` (e0 of the modification model), or -1
    int32_t silent_counted;           // 1: some silent state has a non-zero count_inc (STRique counts emitting states only: dummy1 / dummy2)
    int32_t e_flat[8];                // emitting slot without a Normal emission (uniform inserts, padding): its emission is a constant per lane
    // Models no lane layout covers (more than 512 emitting / 256 silent states, more than 8 in-edges): the baked arrays as
    // they are, for viterbi_csr_kernel -- one workgroup per window, a cell per state, silent states level by level.
    int32_t csr, n_levels;            // csr = 1: the fields above that describe a lane layout are unused (epl = spl = 0, cell = state)
    const int32_t* csr_in_ptr;        // n_states + 1
    const int32_t* csr_in_src;        // in-edges by ascending source
    const double* csr_in_logp;
    const int32_t* csr_kind;          // n_emit: 1 Normal, 2 Uniform
    const double* csr_a;
    const double* csr_b;
    const double* csr_c;
    const int32_t* csr_level_ptr;     // n_levels + 1: silent states by the length of their longest silent predecessor chain
    const int32_t* csr_level_state;   // n_silent
    const VitG2* g2;                  // register-resident profile layout of the same model, or null (strq_model_set_positions)
    int32_t g2_odd, g2_mark;          // that image has its broadcast sources at odd positions; it can carry the repeat-section marks (mark_add)
    // unit decodes (VIT_UNIT): the model's two counted states (emitting, count_inc 1, ascending; -1: the model has no such pair),
    // and whether the register-resident image holds them in the slots of its two broadcast sources (B0: record 0, B1: record 1)
    int32_t unit_state[2];
    int32_t g2_unit;
    // tract decodes (a VIT_COUNT launch with the wide payload, strq_model_set_tracts): n_states + 1 by state, what an emission of the
    // state adds to the 64-bit payload -- (uint64_t)1 << (VIT_TRACT_BITS * j) for a counted state of tract j, else 0 -- or null
    const uint64_t* tract_inc;
};
// three counters of 21 bits: windows below VIT_MARK_T_MAX observations cannot carry from one into the next (every counted state emits)
#define VIT_TRACT_BITS 21
#define VIT_TRACTS_MAX 3
// counter j of such a payload (VitResult::counted of a tract decode), on the host
inline int64_t vit_tract_count(uint64_t payload, int j) { return (int64_t)((payload >> (VIT_TRACT_BITS * j)) & (((uint64_t)1 << VIT_TRACT_BITS) - 1)); }
#define VIT_CSR_MAX_STATES 4096      // two buffers of 16-byte cells in 160 KB of LDS

enum { VIT_SRC_F64 = 0, VIT_SRC_F64_AFFINE = 1, VIT_SRC_I16_AFFINE = 2 };

struct VitTask {
    const VitModel* model;   // device image of the HMM this window is decoded with
    const void* sig;         // first observation
    int64_t T;
    int32_t src_kind, pad_;
    double c1, h1, h2, c2, lo, hi;    // x = clip((s - c1) / h1 * h2 + c2, lo, hi)  (STRique.py:159-160,178-179)
    uint16_t* bp;            // (T + 1) x (n_states) predecessor states, nullable (count-only mode); hub mode: (T + 1) 8-byte hub records;
                             // unit mode: 2 x T 4-byte unit records (see VIT_UNIT_T_MAX)
};

// UNIT decode (VIT_UNIT, flanked model): the best path carries a 32-bit payload  p = (t + 1) << 1 | k  -- the observation t of its
// last emission from a counted state and which of the two it was (k = 0: VitModel::unit_state[0]), 0 = none.  Every emission of
// counted state k at observation t stores the payload it replaces as record 2 t + k of the task's buffer, so that the observations
// of all counted emissions on the best path are read back from the end state's payload (VitResult::dbg[0]) with one hop per repeat
// unit (unit_kernels.hip).  Windows below 2^30 observations (reads are at most 2^30 samples long: strq_batch_upload).
#define VIT_UNIT_T_MAX ((int64_t)1 << 30)
// MARK decode: the packed marks of the lane and CSR kernels hold times below 2^21 (viterbi_kernels.hip)
#define VIT_MARK_T_MAX ((int64_t)1 << 21)

struct VitResult {
    double logp;
    int64_t counted;
    int32_t status;          // 0 ok, 1 no path
    int32_t pad_;
    uint32_t dbg[4];         // reserved (zero)
};

// What a launch carries along the best path (the numeric values are part of the tests' and tools' vocabulary: keep them).
enum VitMode {
    VIT_COUNT = 0,       // the visit count of the counted states
    VIT_BACKPTR = 1,     // ... and a predecessor per (time step, state) for launch_vit_traceback
    VIT_MARK = 2,        // ... and the repeat-section marks (flanked model; windows below VIT_MARK_T_MAX)
    VIT_HUB = 3,         // hub records (modification model)
    VIT_UNIT = 4         // unit records (flanked model; windows below VIT_UNIT_T_MAX)
};
constexpr unsigned vit_mode_bit(int mode) { return 1u << mode; }
constexpr unsigned VIT_MODES_HUB = vit_mode_bit(VIT_HUB), VIT_MODES_UNIT = vit_mode_bit(VIT_UNIT), VIT_MODES_PLAIN = vit_mode_bit(VIT_COUNT) | vit_mode_bit(VIT_BACKPTR) | vit_mode_bit(VIT_MARK);
constexpr unsigned VIT_MODES_CSR = VIT_MODES_PLAIN, VIT_MODES_G2 = vit_mode_bit(VIT_COUNT) | vit_mode_bit(VIT_MARK) | VIT_MODES_UNIT;      // the shapes without lanes (VIT_SHAPE_CSR, VIT_SHAPE_G2)

// The lane-layout kernel shapes: viterbi_kernel<EPL, SPL, DE_HI, DE_LO, DS, ..> is instantiated from a row, for the modes of the row and no
// others.  Emitting slots are sorted by in-degree: the first half of the slots gets DE_HI edge registers, the second half DE_LO; silent slots
// get DS (without their chain edge).  DE_HI above 16 packs two degrees: tens = in-edge registers of slot 0, units = of the other busy slots
// (65: the one or two states of a flanked-repeat model with six in-edges sit in slot 0, the matches with five in the next); those kernels leave
// the count increments of silent states out (STRique counts the emitting dummy states, STRique.py:341-342,375-377).  DE_LO above 10: the units
// are the degree, and every slot of the second half holds uniform emissions only (the inserts).  HUB records need a model of at most two
// emitting slots, UNIT records one of at least two.  `fwd`: the forward_kernel instance (VIT_FWD_SHAPES) that covers the row.
struct VitShape { int id, epl, spl, de_hi, de_lo, ds, fwd; unsigned modes; };
struct VitFwdShape { int epl, spl, de, ds; };
constexpr VitFwdShape VIT_FWD_SHAPES[] = {{4, 2, 6, 3}, {2, 2, 8, 4}, {8, 4, 8, 8}};
constexpr VitShape VIT_SHAPES[] = {
    {0, 4, 2, 6, 3, 3, 0, VIT_MODES_PLAIN | VIT_MODES_UNIT},                    // flanked-repeat models
    {1, 1, 1, 8, 8, 4, 1, VIT_MODES_PLAIN | VIT_MODES_HUB},                     // modification models
    {2, 2, 2, 8, 8, 4, 1, VIT_MODES_PLAIN | VIT_MODES_HUB | VIT_MODES_UNIT},
    {3, 4, 4, 8, 8, 8, 2, VIT_MODES_PLAIN | VIT_MODES_UNIT},
    {4, 8, 4, 8, 8, 8, 2, VIT_MODES_PLAIN | VIT_MODES_UNIT},
    {5, 4, 2, 65, 3, 2, 0, VIT_MODES_PLAIN | VIT_MODES_UNIT},                   // flanked-repeat models, six-edge states in slot 0
    {6, 1, 1, 5, 5, 1, 1, VIT_MODES_PLAIN | VIT_MODES_HUB},                     // STRique's dual base / mCpG model: 26 + 2 states, at most five in-edges
    {7, 4, 2, 65, 13, 2, 0, VIT_MODES_PLAIN | VIT_MODES_UNIT},                  // ... and only uniform emissions in the last two slots
};
constexpr int VIT_LANE_SHAPES = (int)(sizeof(VIT_SHAPES) / sizeof(VIT_SHAPES[0]));
// the order vit_shape_base tries them in: the narrowest kernel that covers the model
constexpr int VIT_SHAPE_TRY[VIT_LANE_SHAPES] = {6, 1, 2, 7, 5, 0, 3, 4};
enum {
    VIT_SHAPE_CSR = VIT_LANE_SHAPES,         // models no lane layout covers (VitModel::csr): viterbi_csr_kernel
    VIT_SHAPE_G2 = VIT_LANE_SHAPES + 1,      // models with a VitG2 image: viterbi_g2_kernel; both parities (g2_odd) share the launch
    VIT_SHAPE_SS = 16                        // flag in the shape id: single-stage model (lane shapes only)
};
static_assert(VIT_SHAPE_G2 < VIT_SHAPE_SS, "the ids stay clear of the single-stage flag");      // (a row's id is its index: the host check)

constexpr int vit_deg_slot0(int de_hi) { return de_hi > 16 ? de_hi / 10 : de_hi; }
constexpr int vit_deg_hi(int de_hi) { return de_hi > 16 ? de_hi % 10 : de_hi; }
constexpr int vit_deg_lo(int de_lo) { return de_lo > 10 ? de_lo % 10 : de_lo; }
constexpr bool vit_lo_flat(int de_lo) { return de_lo > 10; }
constexpr bool vit_silent_counted(int de_hi) { return de_hi <= 16; }
// in-edge registers of emitting slot `slot` of a row
constexpr int vit_slot_deg(const VitShape& r, int slot) { return slot == 0 ? vit_deg_slot0(r.de_hi) : (slot < (r.epl + 1) / 2 ? vit_deg_hi(r.de_hi) : vit_deg_lo(r.de_lo)); }

// vit_dispatch<N>(i, fn): fn(std::integral_constant<int, i>) for a run-time i in [0, N) -- the template instance of a table row; 2 outside
template <class Fn, int... I>
inline int vit_dispatch(std::integer_sequence<int, I...>, int i, Fn&& fn)
{
    int rc = 2;
    (void)((i == I && ((rc = fn(std::integral_constant<int, I>{})), true)) || ...);
    return rc;
}
template <int N, class Fn> inline int vit_dispatch(int i, Fn&& fn) { return vit_dispatch(std::make_integer_sequence<int, N>{}, i, fn); }

enum VitFamily { VIT_FAMILY_NONE = -1, VIT_FAMILY_LANE = 0, VIT_FAMILY_CSR = 1, VIT_FAMILY_G2 = 2 };
constexpr VitFamily vit_shape_family(int shape)
{
    if (shape < 0) return VIT_FAMILY_NONE;
    const int b = shape & ~VIT_SHAPE_SS;
    return b < VIT_LANE_SHAPES ? VIT_FAMILY_LANE : (b == VIT_SHAPE_CSR ? VIT_FAMILY_CSR : (b == VIT_SHAPE_G2 ? VIT_FAMILY_G2 : VIT_FAMILY_NONE));
}
// the one place that says which (shape, mode) pairs exist: planners ask it, launchers obey it
constexpr bool vit_mode_ok(int shape, int mode)
{
    if (mode < VIT_COUNT || mode > VIT_UNIT) return false;
    const VitFamily f = vit_shape_family(shape);
    const unsigned modes = f == VIT_FAMILY_LANE ? VIT_SHAPES[shape & ~VIT_SHAPE_SS].modes : (f == VIT_FAMILY_CSR ? VIT_MODES_CSR : (f == VIT_FAMILY_G2 ? VIT_MODES_G2 : 0u));
    return (modes & vit_mode_bit(mode)) != 0;
}
// silent slots per lane of a kernel shape (the template's SPL); 0 for the shapes without lanes
constexpr int vit_shape_silent_slots(int shape) { return vit_shape_family(shape) == VIT_FAMILY_LANE ? VIT_SHAPES[shape & ~VIT_SHAPE_SS].spl : 0; }

// a row's slots and edge registers hold the model, and the model has what the row's kernels take for granted
inline bool vit_shape_covers(const VitShape& r, const VitModel& mh)
{
    if (mh.epl > r.epl || mh.spl > r.spl) return false;
    if (!vit_silent_counted(r.de_hi) && mh.silent_counted) return false;
    for (int i = 0; i < mh.epl; ++i) if (mh.e_deg[i] > vit_slot_deg(r, i)) return false;
    for (int i = 0; i < mh.spl; ++i) if (mh.s_deg[i] > r.ds) return false;
    for (int i = (r.epl + 1) / 2; vit_lo_flat(r.de_lo) && i < r.epl; ++i) if (i >= mh.epl || !mh.e_flat[i]) return false;
    return true;
}
inline int vit_shape_base(const VitModel& mh) { for (int id : VIT_SHAPE_TRY) if (vit_shape_covers(VIT_SHAPES[id], mh)) return id; return -1; }
// One launch decodes windows of several models as long as they fit the same kernel shape; -1 if no compiled shape fits
inline int vit_shape_of(const VitModel& mh)
{
    if (mh.csr) return VIT_SHAPE_CSR;
    const int b = vit_shape_base(mh);
    return b < 0 ? b : (b | (mh.single_stage ? VIT_SHAPE_SS : 0));
}
// the same, or VIT_SHAPE_G2 when the model has a register-resident image that carries the mode (either parity of the chain:
// decided per window inside the kernel) and the caller allows it
inline int vit_shape_for(const VitModel& mh, VitMode mode, bool allow_g2)
{
    if (mh.g2 && allow_g2 && vit_mode_ok(VIT_SHAPE_G2, mode) && (mode != VIT_MARK || mh.g2_mark) && (mode != VIT_UNIT || mh.g2_unit)) return VIT_SHAPE_G2;
    return vit_shape_of(mh);
}
// a VIT_UNIT launch of this shape decodes this model
inline bool vit_unit_ok(const VitModel& mh, int shape)
{
    return mh.unit_state[0] >= 0 && mh.unit_state[1] >= 0 && !mh.silent_counted && vit_mode_ok(shape, VIT_UNIT) && (vit_shape_family(shape) != VIT_FAMILY_G2 || (mh.g2 && mh.g2_unit));
}

}  // namespace strq
