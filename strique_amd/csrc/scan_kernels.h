// Internal: positions / gate of a read from its flank alignments (shared by finalize_kernel of the detect pipeline and the scan
// kernels), and the scan itself: all candidates of a read compared, the winner's window handed to the HMM (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "align_kernels.h"
#include "cond_kernels.h"
#include "viterbi_kernels.h"

namespace strq {

struct ReadGeom {           // per read, written by finalize_kernel / scan_select_kernel
    double score_prefix, score_suffix;
    int64_t prefix_begin, prefix_end, suffix_begin, suffix_end;
    int32_t gate, pad_;
    float best_prefix, best_suffix;      // raw alignment scores (the overlap planning of the next sub-batch reads their distribution)
    int64_t prefix_begin_whole, suffix_end_whole;      // where flank row 0 of the prefix and the last row of the suffix sit: the ends before the trim
                                                       // (strq_batch_fetch_flank_ranges: the stretches of the whole configured flanks)
};

#ifdef __HIPCC__
// position of flank row k in the read: argmin_i |a_idx[i] - b_idx[k]| of __detect_range__
// (STRique.py:540-547) evaluated on the compact record: a diagonal row sits on its sample; a row
// inside a vertical run sits between two samples and takes the nearer one, the lower index on a tie.
static __device__ inline int64_t row_position(const int32_t* rec, int m, int k, int n)
{
    const int32_t r = rec[k];
    const int64_t j = r >> 1;
    if (!(r & 1)) return j - 1;
    int k1 = k; while (k1 > 0 && rec[k1 - 1] == r) --k1;
    int k2 = k; while (k2 < m - 1 && rec[k2 + 1] == r) ++k2;
    const int d_prev = k - k1 + 1, d_next = k2 - k + 1;
    const bool has_prev = j >= 1, has_next = j < n;
    if (has_prev && (!has_next || d_prev <= d_next)) return j - 1;
    return j;
}

// the prefix half of a ReadGeom from the traced prefix alignment (STRique.py:598: the first `trim` rows are the extension)
static __device__ inline void prefix_geometry(const AlignTask& tp, const AlignResult& rp, int trim, ReadGeom& g)
{
    const int64_t b = row_position(tp.rec, tp.m_total, 0, tp.n), e = row_position(tp.rec, tp.m_total, tp.m_total - 1, tp.n);
    g.score_prefix = e > b ? (double)rp.best / (double)(e - b) : 0.0;
    g.best_prefix = rp.best;
    g.prefix_begin = row_position(tp.rec, tp.m_total, trim, tp.n);
    g.prefix_begin_whole = b;
    g.prefix_end = e;
}

// ... and the suffix half (STRique.py:599: the last `trim` rows are the extension)
static __device__ inline void suffix_geometry(const AlignTask& ts, const AlignResult& rs, int trim, ReadGeom& g)
{
    const int64_t b = row_position(ts.rec, ts.m_total, 0, ts.n), e = row_position(ts.rec, ts.m_total, ts.m_total - 1, ts.n);
    g.score_suffix = e > b ? (double)rs.best / (double)(e - b) : 0.0;
    g.best_suffix = rs.best;
    g.suffix_begin = b;
    g.suffix_end = row_position(ts.rec, ts.m_total, ts.m_total - 1 - trim, ts.n);
    g.suffix_end_whole = e;
}

// the reference's gate (STRique.py:602) looks at the two alignments only: a read whose 8-bit morphology signal
// normalises while its filtered signal does not (empty percentile tails: NaN constants) still goes to the HMM,
// as a window of NaN observations -- pomegranate's missing-value rule, see viterbi_kernels.hip
static __device__ inline int geometry_gate(const ReadGeom& g)
{
    return (g.prefix_begin < g.suffix_end && g.score_prefix > 0.0 && g.score_suffix > 0.0) ? 1 : 0;
}

// the Viterbi task of a window [begin, end) of a read's filtered signal (an empty task when `open` is 0); the host writes the windows
// of the motif pass with it
static __host__ __device__ inline VitTask window_task(int open, int64_t begin, int64_t end, const ReadCond& rc, const VitModel* model, const void* flt, int is_f64, const PoreStats& ps)
{
    VitTask vt = {};
    vt.model = model;
    if (open) {
        vt.T = end - begin;
        if (is_f64) { vt.sig = reinterpret_cast<const double*>(flt) + rc.off + begin; vt.src_kind = VIT_SRC_F64_AFFINE; }
        else { vt.sig = reinterpret_cast<const int16_t*>(flt) + rc.off + begin; vt.src_kind = VIT_SRC_I16_AFFINE; }
        vt.c1 = rc.f_c1; vt.h1 = rc.f_h1; vt.h2 = rc.h2; vt.c2 = rc.c2; vt.lo = ps.clip_lo; vt.hi = ps.clip_hi;
    }
    return vt;
}

// the Viterbi task of a read: the window [prefix_begin, suffix_end) of its filtered signal when the gate passed, else an empty one
static __device__ inline VitTask window_task(const ReadGeom& g, const ReadCond& rc, const VitModel* model, const void* flt, int is_f64, const PoreStats& ps)
{
    return window_task(g.gate, g.prefix_begin, g.suffix_end, rc, model, flt, is_f64, ps);
}
#endif

// scan_select_kernel: one thread per read.  The read's 2 * n_cand alignments are (candidate c: prefix, suffix) at alignment
// indices 2 * (r * n_cand + c) and + 1 of the sub-batch part; task_of maps an alignment index to its task.
struct ScanSelectArgs {
    const AlignTask* tasks; const AlignResult* results;
    const int32_t* task_of;        // 2 * n_cand per read
    const int32_t* trim;           // 2 per candidate: pre_trim of its prefix flank, post_trim of its suffix flank
    const ReadCond* rc;
    double min_score;
    ReadGeom* geom;                // per read: the winner's positions (gate 1), or zeros (gate 0)
    int32_t* winner;               // per read: position in the candidate list, -1 = none
    double* scores;                // 2 per (read, candidate): score_prefix, score_suffix
    float* best;                   // 2 per (read, candidate): the raw alignment scores
    int n_reads, n_cand;
};
int launch_scan_select(hipStream_t s, const ScanSelectArgs& a);

// scan_task_kernel: the Viterbi task of every read of the sub-batch from the ReadGeom scan_select_kernel left, with the model of its
// winner (model_of / vit_slot: planned on the host once the winners are known)
struct ScanTaskArgs {
    const ReadGeom* geom; const ReadCond* rc;
    const int32_t* vit_slot; const VitModel* const* model_of;
    const void* flt; int is_f64;
    PoreStats ps;
    VitTask* vit;
    int n_reads;
};
int launch_scan_tasks(hipStream_t s, const ScanTaskArgs& a);

}  // namespace strq
