// Internal context of libstrique_hip (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <map>
#include <cstdio>
#include <functional>
#include <mutex>
#include <atomic>
#include <utility>
#include "align_kernels.h"
#include "viterbi_kernels.h"
#include "forward_kernels.h"
#include "posterior_kernels.h"
#include "mod_llr_kernels.h"
#include "variant_kernels.h"
#include "motif_kernels.h"
#include "screen_kernels.h"
#include "strq_opt.h"

namespace strq {

// Blocks the process holds right now (strq_debug_live_allocations): [0] device, [1] pinned host memory.  Atomic: the upload thread of
// a context allocates too.
inline std::atomic<int64_t> live_allocations[2];

// Grow-only buffer that owns its block: device memory (DevBuf) or pinned host memory (PinBuf).  reserve() frees the old block and takes
// a larger one with slack; the destructor frees -- whatever holds a buffer (the context, the detect state, a slot, a HostModel) gives it
// back when it is deleted.  Not copyable.
template <bool PINNED> struct OwnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf&) = delete;
    OwnedBuf& operator=(const OwnedBuf&) = delete;
    ~OwnedBuf() { release(); }
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        const size_t want = bytes + bytes / 8 + (PINNED ? 0 : 256);
        const hipError_t e = PINNED ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want; ++live_allocations[PINNED];
        return e;
    }
    void release()
    {
        if (p) { (void)(PINNED ? hipHostFree(p) : hipFree(p)); --live_allocations[PINNED]; }
        p = nullptr; cap = 0;
    }
    void swap(OwnedBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
using DevBuf = OwnedBuf<false>;
using PinBuf = OwnedBuf<true>;

// strq_ctx::queue: work-queue heads of the persistent kernels, one zero-initialised int per launch of a call (index 0:
// the table kernel's count of borderline entries, launches from index STRQ_QUEUE_FIRST on)
#define STRQ_QUEUE_BYTES 65536
#define STRQ_QUEUE_FIRST 8
#define STRQ_QUEUE_SLOTS (STRQ_QUEUE_BYTES / 4)

// one sub-batch of alignments for align_core (strq_align_api.hip)
struct AlignCoreIn {
    int nb = 0, samples = 6;
    const uint8_t* d_levels = nullptr;     // device: concatenated level streams
    const int64_t* read_off = nullptr;     // host: offsets of the reads in d_levels
    const float* d_level_val = nullptr;    // device: 256 level values per read
    const int32_t* read = nullptr;         // host, per alignment
    const int* n = nullptr; const int* m = nullptr; const int* k = nullptr; const int* R = nullptr;
    const int* NS = nullptr;               // strips per alignment (1 or 2)
    const float* const* flank = nullptr;   // host: flank template of each alignment
    // called once the score-table kernel of the sub-batch is queued (whatever is to share the GPU with the alignment kernels that
    // follow is launched behind it -- strq_detect_api.hip); a non-zero return aborts the call
    std::function<int()> after_tables;
};
struct AlignCoreOut {
    std::vector<int> order;                // task position -> alignment index
    std::vector<size_t> rec_off;           // per alignment: offset of its record in d_rec
    size_t rec_total = 0;
    AlignTask* d_tasks = nullptr; AlignResult* d_results = nullptr; int32_t* d_rec = nullptr;
    int n_hard = 0;
    int n_launches = 0;                    // forward-kernel launches
    double wave_steps = 0, columns = 0;    // forward work of this sub-batch
    int segs = 1, tables = 0, packed = 0, rows_per_lane = 0;
    int overlap_first = 0, overlap_worst = 0;      // columns the pieces of the last segmented launch were cut with first / in the worst case
};

struct HostModel {
    VitModel h;              // host copy (pointers are device pointers)
    const VitModel* dev = nullptr;
    DevBuf blob;
    DevBuf g2_blob;          // register-resident image of the same model (strq_model_set_positions), if any
    // the baked arrays as they were handed to strq_model_create (strq_model_set_positions lays them out once more)
    int32_t n_states = 0, silent_start = 0, start = 0, end = 0;
    std::vector<int32_t> in_ptr, in_src, emis_kind, count_inc, state_tag;
    std::vector<double> in_logp, emis_a, emis_b, emis_c;
    // forward pass (forward_kernels.h): which CSR in-edge every entry of the image's edge rows / chain edges holds (-1: padding),
    // rounds of its silent phase, the per-edge log-probabilities of a sum over paths where they differ from in_logp
    // (strq_model_set_forward_logp), and the image of transition probabilities, built on first use
    std::vector<int32_t> edge_csr, chain_csr;
    int32_t fwd_stages = 1;
    std::vector<double> fwd_logp;
    DevBuf fwd_blob;
    const FwdModel* fwd_dev = nullptr;
    // state posteriors (posterior_kernels.h): the state held by every cell of the lane layout (VitModel::cell_state), and the transposed
    // image of the forward image -- built on first use, dropped with it
    std::vector<int32_t> cell_state;
    DevBuf post_blob;
    const PostModel* post_dev = nullptr;
    // per-unit scores of the modification pass (mod_llr_kernels.h): the edge image of a dual model, built on first use
    DevBuf llr_blob;
    const LlrModel* llr_dev = nullptr;
    int32_t llr_mode = -1;
    // variant pass (variant_kernels.h): the edge image of a variant model, built by strq_target_set_variants
    DevBuf var_blob;
    const VarModel* var_dev = nullptr;
    int32_t var_mode = -1, var_nb = 0;
    // motif track (motif_kernels.h): the edge image of a loop model, built on first use
    DevBuf motif_blob;
    const MotifModel* motif_dev = nullptr;
    // tract decodes (strq_model_set_tracts): the per-state increments behind VitModel::tract_inc
    DevBuf tract_blob;
    int32_t n_tracts = 0;
};

}  // namespace strq

struct strq_ctx {
    // strq_set_option: per-context switches (key -> value; an empty value = "unset", whatever the environment says).  Every switch
    // of the library is read through strq::opt(key): this map first, then the process-wide table (strq_set_option(NULL, ...)),
    // then the environment variable of the same name -- so that one process can run A/B legs on the same resident batches.
    std::map<std::string, std::string> options;
    mutable std::mutex options_mu;            // strq_set_option on one thread, strq::opt on another (the upload thread of the context; a second context's host thread never sees this map)
    int device = 0;
    int n_cu = 0;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;        // the largest forward launch of a screened sub-batch beside the others (align_core), created on first use
    hipEvent_t ev_fork = nullptr, side_join = nullptr;
    hipEvent_t ev[8] = {};
    strq::AlignParams ap{-2.0f, -8.0f, -2.0f, -8.0f, 8.0f, -16.0f};   // src/align_raw.h:51-60
    std::string err;
    float timing[8] = {};
    double counters[8] = {};
    int32_t geometry[8] = {};                 // strq_last_geometry
    int32_t vit_launches[4] = {};             // strq_last_viterbi_launches
    int32_t tract_shape_last = -1;            // strq_debug_tract_shape: kernel shape of the last tract launch
    int64_t second_round[2] = {};             // strq_last_second_round: alignments that ran the second forward round / alignments, last batched call
    strq::DevBuf redo_total;                  // device counter: alignments whose first forward round missed its certificate (second look + whole-read second round)
    int64_t look2_served = 0;                 // of them, resolved by the coarse screen's second look (or dropped with an attempt that started over): not whole-read reruns
    double screen_stats[8] = {};              // strq_last_screen
    double overlap[4] = {};                   // strq_last_overlap
    bool screen_ran = false;                  // the last align_core call ran the screen (events 5, 6 bracket it)
    // The screen pays when nearly every alignment gets windows (a read that holds its flank clearly) and costs a pass when not:
    // a sub-batch in which fewer than 90 % did, whose windows hold more than 6 % of the columns, or in which more than one alignment
    // in 4096 is left with over 32 k columns to run (a tail behind thousands of small windows) pauses it for the next eight
    // sub-batches of this context, then it is tried again.
    int screen_pause = 0;
    // the coarse screen in front of it (align_screen3_kernel): paused the same way when it leaves too many columns or certifies too
    // few alignments in its first look; its candidate margin (score units below the best chunk bound) is a constant
    int coarse_pause = 0;
    int coarse_fail = 0, screen_fail = 0;     // consecutive sub-batches on which the coarse / the fine screen did not pay: the pause doubles (8, 16, ... 256)
    float coarse_margin = 384.0f;
    float aborted_fwd_ms = 0, aborted_screen_ms = 0;      // forward / screen time of an attempt align_core stopped and started over (added to the call's times)
    int screen_mode_last = 0;                 // screen of the last align_core call: 0 none, 1 fine, 2 coarse
    int coarse_merge_last = 0;                // ... and the flank rows per DP row of the coarse one
    int screen_byte_sc_last = 0;              // ... and, on the level image, the scale the kernel rounds its byte entries at (0 otherwise)
    int screen_lds_last = 0;                  // ... and the LDS layout of its score tables: 1 lane-major image, 2 class rows, 3 level image (0: the one-flank kernel)
    
    // workspace
    strq::DevBuf levels, level_val, flank_cls, tables, tables3, band_lo, col0, ckpt, rec, tasks, results,
        queue, scratch, lutinfo, hard, misc, vit_x, vit_tasks, vit_bp, vit_path, bnd,
        gen_codes, gen_table, gen_bnd, gen_trace, gen_hard,      // generic align_overlap path
        screen,                                                   // upper-bound screen: tasks, chunk maxima, windows
        ckpt2;                                                    // checkpoints of the coarse screen's second look
    std::vector<strq::HostModel*> models;
    void* detect = nullptr;                   // DetectState (strq_detect_api.hip)
    size_t max_ws_bytes = (size_t)96 << 30;   // cap for checkpoint workspace per sub-batch
    // best flank scores of the previous detect sub-batch as fractions of m * dist_offset (sorted), and its mean read
    // length: the column segments of the next sub-batch are cut with the overlap that is cheapest for that distribution
    std::vector<float> score_fracs; double mean_n = 0;
};

namespace strq {
// marks `c` as that context for the lifetime of the object (every C-ABI entry that takes a context opens one)
struct CtxScope { const strq_ctx* prev; explicit CtxScope(const strq_ctx* c); ~CtxScope(); };
int align_core(strq_ctx* c, const AlignCoreIn& in, AlignCoreOut& out);
int align_core_times(strq_ctx* c, float* t_lut, float* t_fwd, float* t_tr);
int align_validate_flank(strq_ctx* c, const float* f, int64_t m, int samples, int* k_out, int* R_out, int* NS_out);
size_t align_workspace_bytes(int n, int m, int R, int NS);   // checkpoints + strip boundary of one alignment
float host_cell_score(const AlignParams& p, float h, float v);
void detect_state_free(strq_ctx* c);
int detect_drain(strq_ctx* c);              // rows of every detect sub-batch in flight taken (strq_detect_api.hip); nothing to do without detect state
// launch_viterbi's return code as a status of the C ABI.  2 / 3: this kernel shape has no such decode mode -- the caller's input, not a device fault
int viterbi_launch_status(int vrc);
// the forward image of a model (HostModel::fwd_dev), built if it is not there; STRQ_ERR_UNSUPPORTED (c->err says why) for a model without one
int forward_model(strq_ctx* c, HostModel* hm);
// ... and its transposed image (HostModel::post_dev) behind it, for the backward half of the state posteriors
int posterior_model(strq_ctx* c, HostModel* hm);
// the edge image of a loop model for the motif track (HostModel::motif_dev), built if it is not there; STRQ_ERR_UNSUPPORTED (c->err says
// why) for a model that is no loop model (strq_motif_api.hip)
int motif_model(strq_ctx* c, HostModel* hm);
// Unit positions of the tracts of decoded windows (strq_set_tract_positions, strq_viterbi_tract_positions; strq_detect_api.hip): every
// window once more with back-pointers, traced back and scanned (tract_scan_kernel).  Pieces: the rule of detect_plan.h on the windows'
// back-pointers against STRQ_TRACT_POS_WS_BYTES, an oversize window left out.  task: the window as its count decode had it (bp is set here); n[j]: the visits of tract j that decode found; base:
// what position 0 of the window is reported as.  status[i]: 0 positions in pos[3 i + j] (model order), 2 the window's back-pointers
// alone exceed the budget (not traced).  stats (or null): windows traced, kernels launched, peak back-pointer bytes of a piece.
struct TractPosWindow { VitTask task; const HostModel* hm; int64_t base; int64_t n[3]; };
struct TractPosOut { std::vector<int32_t> status; std::vector<std::vector<int64_t>> pos; };
int tract_positions(strq_ctx* c, const std::vector<TractPosWindow>& w, TractPosOut& out, double* stats);
// State statistics of decoded windows (strq_set_state_stats, strq_viterbi_state_stats; strq_detect_api.hip, the rule: strique_amd/
// state_stats.py): every window once more with back-pointers, traced back and summed per emitting state (state_stats_kernel).  Pieces:
// the rule of detect_plan.h on the windows' back-pointers against STRQ_STATE_STATS_WS_BYTES, an oversize window left out.  task: the window as its count decode had it (bp is set here); logp, counted:
// what that decode found -- a back-pointer decode with other bits fails the call (STRQ_ERR_DEVICE).  status[i]: 0 the rows n / sum /
// sumsq[i] hold silent_start entries, 2 the window's back-pointers alone exceed the budget (no rows).  stats (or null): windows, kernels
// launched, peak back-pointer bytes of a piece.
struct StateStatsWindow { VitTask task; const HostModel* hm; double logp; int64_t counted; };
struct StateStatsOut { std::vector<int32_t> status; std::vector<std::vector<int64_t>> n; std::vector<std::vector<double>> sum, sumsq; };
int state_stats(strq_ctx* c, const std::vector<StateStatsWindow>& w, StateStatsOut& out, double* stats);
// State posteriors of windows (strq_set_state_posteriors, strq_forward_state_stats; strq_detect_api.hip, the rule: strique_amd/
// state_posteriors.py): forward-backward over every window (posterior_kernels.h).  Pieces: the rule of detect_plan.h on the windows'
// stored forward vectors against STRQ_STATE_POST_WS_BYTES, at most 8192 windows each, an oversize window carried in front.  task: the window (bp unused).  fwd[i]: the forward half's result of every window (fwd_finish gives the likelihood);
// status[i]: 0 the rows w / wx / wxx[i] hold silent_start entries, 1 no path (no rows), 2 the window's stored vectors alone exceed the
// budget (no rows; fwd[i] is valid).  stats (or null): windows, kernels launched, peak workspace bytes of a piece.
struct StatePostWindow { VitTask task; HostModel* hm; };
struct StatePostOut { std::vector<int32_t> status; std::vector<FwdResult> fwd; std::vector<std::vector<double>> w, wx, wxx; };
int state_posteriors(strq_ctx* c, const std::vector<StatePostWindow>& w, StatePostOut& out, double* stats);
void host_stats_batch(const double* signals, const int64_t* offsets, int64_t n_reads, bool want_raw, double* out,
                      const double* const* reads = nullptr);   // host_stats.hip; reads: one buffer per read instead of `signals`
}

// The way into the library, first statement of an entry point that can reach the device or strq::opt: a null context is rejected,
// then the context's scope, then its device.
#define STRQ_ENTER(ctx)                                                                        \
    if (!(ctx)) return STRQ_ERR_ARG;                                                           \
    strq::CtxScope scope_(ctx);                                                                \
    STRQ_HIP(ctx, hipSetDevice((ctx)->device))

#define STRQ_HIP(ctx, call)                                                                    \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
            return STRQ_ERR_DEVICE;                                                            \
        }                                                                                      \
    } while (0)

namespace strq {
// the first 256 queue heads of the context zeroed on `st`, in front of the Viterbi / forward launches of a pass (one head each)
inline int reset_queue_heads(strq_ctx* c, hipStream_t st)
{
    STRQ_HIP(c, c->queue.reserve(1024));
    STRQ_HIP(c, hipMemsetAsync(c->queue.p, 0, 1024, st));
    return STRQ_OK;
}
}
