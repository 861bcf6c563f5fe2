// C ABI: repeatCounter.add_target / detect as a batched device pipeline
// (reference scripts/STRique.py:553-618):
//   conditioning -> score tables -> 2 flank alignments per read -> positions / gate -> HMM Viterbi
// Everything between upload and fetch stays in HBM; the host only sequences kernels, reads back the
// table-width class of each alignment and assembles the result records.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <time.h>
#include <vector>
#include "../../include/strique_hip.h"
#include "strq_ctx.h"
#include "detect_plan.h"
#include "cond_kernels.h"
#include "viterbi_kernels.h"
#include "mod_kernels.h"
#include "unit_kernels.h"
#include "forward_kernels.h"
#include "scan_kernels.h"
#include "anchored_kernels.h"
#include "tract_kernels.h"
#include "renorm_kernels.h"
#include "variant_kernels.h"
#include "flank_mod_kernels.h"
#include "state_stats_kernels.h"
#include "posterior_kernels.h"

using namespace strq;

#define STRQ_DBG(...) do { if (strq::opt("STRQ_DEBUG")) { fprintf(stderr, "[strq] " __VA_ARGS__); fprintf(stderr, "\n"); fflush(stderr); } } while (0)
static double now_s() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

namespace strq {

struct FinalizeArgs {
    const AlignTask* tasks; const AlignResult* results;
    const int32_t* task_of;        // 2 per read: task position of the prefix / suffix alignment
    const int32_t* trim;           // 2 per read: pre_trim of the prefix flank, post_trim of the suffix flank
    const int32_t* vit_slot;       // per read: index of its VitTask
    const ReadCond* rc;
    const VitModel* const* model_of;   // per read
    const void* flt;               // filtered signal (int16 or double), concatenated
    int is_f64;
    PoreStats ps;
    ReadGeom* geom; VitTask* vit;
    int n_reads;
};

__global__ void finalize_kernel(FinalizeArgs a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_reads) return;
    const ReadCond rc = a.rc[r];
    ReadGeom g = {};
    // the alignments run on whatever the conditioning produced (an all-NaN signal scores dist_min in every
    // cell, as it does in the reference), so the positions are reported for every non-empty read
    if (rc.n > 0) {
        const int tp = a.task_of[2 * r], ts = a.task_of[2 * r + 1];
        prefix_geometry(a.tasks[tp], a.results[tp], a.trim[2 * r], g);
        suffix_geometry(a.tasks[ts], a.results[ts], a.trim[2 * r + 1], g);
        g.gate = geometry_gate(g);
    }
    a.geom[r] = g;
    a.vit[a.vit_slot[r]] = window_task(g, rc, a.model_of[r], a.flt, a.is_f64, a.ps);
}

struct Target {
    std::vector<float> prefix_ext, suffix_ext;
    int trim_prefix = 0, trim_suffix = 0, samples = 6;
    int kp = 0, Rp = 0, NSp = 1, ks = 0, Rs = 0, NSs = 1;
    int model_id = -1, count_bias = 0;
    int mod_model_id = -1; double mod_min = 0, mod_max = 0;
    int end_model_id = -1, end_bias = 0, start_model_id = -1, start_bias = 0;      // strq_target_set_anchored: both models or none
    int var_model_id = -1, var_nalt = 0, var_ctx = 0; double var_lo = 0, var_hi = 0;      // strq_target_set_variants
    const RenormTable* rn_dev = nullptr;      // strq_target_set_renorm: the tables of the target on the device (DetectState::rn_tables owns them)
    int tract_model_id = -1, n_tracts = 0, tract_bias[3] = {0, 0, 0};      // strq_target_set_tracts
    // strq_target_set_flank_mod: per flank as the strand reads it the profile model, the flank's length, its column table on the device,
    // and per group the columns, the site model and what the records report (flank as configured, pos, n_sites)
    struct FlankMod { int model_id = -1, len = 0; std::shared_ptr<DevBuf> col; std::vector<FlankGroupRange> range; std::vector<int> site; std::vector<int32_t> info; };
    FlankMod fmod[2];
    int n_motifs = 0, motif_loop[MOTIF_MAX_CAND] = {-1, -1, -1, -1}, motif_flanked[MOTIF_MAX_CAND] = {-1, -1, -1, -1}, motif_bias[MOTIF_MAX_CAND] = {0, 0, 0, 0};      // strq_target_set_motifs
    bool has_fmod() const { return mod_model_id >= 0 && fmod[0].model_id >= 0 && fmod[1].model_id >= 0; }
};

struct Batch : ReadRows {
    int64_t n_reads = 0;
    int dtype = 0;                       // 0 int16, 1 float64
    std::vector<int64_t> off;            // n_reads + 1
    std::vector<int32_t> target;
    std::vector<int32_t> target_given;   // a scan run writes the winners' targets into `target`: what the caller uploaded, for a plain run after it
    int scan_ncand = 0;                  // the last run call was a scan over this many candidates (0: a plain detect)
    std::vector<int32_t> cand;           // scan: winner of every read as a position in the candidate list, -1 = none
    std::vector<double> scores;          // scan: score_prefix, score_suffix of every (read, candidate)
    std::vector<double> host_stats;      // 6 per read (float64 input only)
    DevBuf raw;                          // all reads, resident
    bool on_host = false;                // samples still (partly) in the caller's memory: uploaded sub-batch by sub-batch
    const char* host_src = nullptr;      // strq_detect_batch: the caller's concatenated buffer
    std::vector<const char*> host_reads; // strq_detect_batch_reads: one buffer per read instead
    void forget_host() { on_host = false; host_src = nullptr; host_reads.clear(); }
    int64_t uploaded = 0;                // reads whose samples are in `raw`
    Extras ran;                          // what the last run call ran with: fetching an output it did not produce is an error
    // a new batch of n reads: rows, patterns and the optional outputs at their initial values, no samples uploaded, nothing of the caller's referenced
    void begin(int64_t n, int dt)
    {
        forget_host();
        n_reads = n; dtype = dt; uploaded = 0; host_stats.clear();
        target_given.clear(); scan_ncand = 0; cand.clear(); scores.clear();
        size_reads(n); ran = Extras();
    }
    float t_cond = 0, t_lut = 0, t_fwd = 0, t_trace = 0, t_vit = 0, t_total = 0;
    double n_hard = 0;
    int n_fwd_launches = 0;
};

struct DetectState {
    PoreStats ps{0, 0, 0, 0};
    bool have_ps = false;
    std::vector<Target> targets;
    Batch batch;
    DevBuf rc, hist16, hist8, geom, idx, hist_raw, bp, path, modtask, modsig, modlen, pattern, hrange, modpool, f64s;
    DevBuf unit_task, unit_ws, unit_path, unit_pool;      // unit pass (run_unit_pass): tasks, records / back-pointers, state paths, positions
    Extras extras;                       // strq_set_units, strq_set_confidence, strq_set_mod_llr: what the next run call uses
    PassStats stats[N_PASS] = {}; double& stat(Pass p, int k) { return stats[p].v[k]; }      // strq_last_*: what every pass of the last run call did
    DevBuf llr_ws;                       // per-unit scores (run_llr_pass): tasks, unit bounds, scores
    DevBuf var_ws, var_bounds, var_out;  // variant pass (run_variant_tail): tasks and passage counts; passage bounds; scores
    DevBuf conf_task;                    // forward pass (run_conf_pass): tasks, model images, c0, results, order
    DevBuf fmod_ws, fmod_bp;             // flank methylation calls (run_flank_mod_pass): tasks, stretches and paths of a piece; its back-pointers
    DevBuf tract_ws, tract_task;         // tract pass (run_tract_pass): geometry and conditioning rows of a sub-batch; tasks, results, their reads and models
    DevBuf motif_ws, motif_rows, motif_task;              // motif pass (run_motif_pass): windows, tasks and results of the track; rows and tasks of the majority decodes
    DevBuf tpos_task, tpos_bp, tpos_path, tpos_pool;     // tract positions (tract_positions): tasks and results of a piece, its back-pointers, state paths, positions
    DevBuf sst_task, sst_bp, sst_path, sst_out;           // state statistics (state_stats): tasks and results of a piece, its back-pointers, state paths, rows
    DevBuf post_task, post_ws, post_out;                  // state posteriors (state_posteriors): tasks and results of a piece, its stored forward vectors, rows
    DevBuf anch_ws, anch_task;           // anchored pass (run_anchored_pass): geometry, conditioning rows and kinds of a sub-batch; tasks, results, their reads and models
    hipEvent_t amod_ev[2] = {};          // methylation calls of anchored reads (run_anchored_mod): their own bracket, inside the anchored pass
    // renorm (run_renorm_part): the tables of the targets, the grid and the shares, the histograms and the per-read table rows of a sub-batch
    std::vector<std::unique_ptr<DevBuf>> rn_tables;
    RenormGrid rn_grid = {}; bool rn_have_grid = false;
    DevBuf rn_h, rn_reads;
    hipEvent_t rn_ev[4] = {}; int rn_timed = 0;      // one pair of events per piece of a sub-batch (at most two); pairs recorded by the sub-batch under way
    // strq_scan_set: run calls compare these candidates (target ids) on every read instead of taking the read's own target
    bool scan_on = false; std::vector<int32_t> scan_cand; double scan_min = 0;
    DevBuf scan_idx, scan_out;           // scan: task table and candidate trims / winners, scores and raw scores of a sub-batch
    PinBuf scan_pin;                     // ... and what the host reads of them before the Viterbi launches are planned
    hipEvent_t ev[4] = {};
    int64_t part_reads = 0;              // strq_batch_upload_part: reads uploaded so far
    // Two sub-batches are in flight at a time: the Viterbi launches of sub-batch k run on `vit_stream` while the conditioning and the
    // flank alignments of sub-batch k + 1 are queued on the context's stream (the Viterbi launch lasts as long as its longest window --
    // reads whose flanks were mislocated decode 10^5 steps and more -- and most of the GPU idles under that tail).  What a Viterbi launch
    // reads or writes exists twice (filtered signal, tasks, results, order, queue heads); results come back one sub-batch late.
    struct Slot {
        DevBuf flt, vit, vres, order, vq;
        DevBuf rn_rec; PinBuf rn_pin;    // renorm: the records of the sub-batch on the device and what the host reads of them
        // Idle -> Forward: publish_forward, the forward stage of reads [r0, r0 + nr) is queued, its Viterbi launches are not (they go behind the
        //   score-table kernel of the next sub-batch)
        // Forward -> Decoding: launch_viterbi_of, once the launches and the copy of their results are queued and `v1` is recorded
        // Decoding -> Idle: harvest, once the rows are in Batch::results and the modification / unit pass of the sub-batch has run
        // A failure on the way goes through abandon(): Idle, the rows at their initial values.
        enum State { Idle, Forward, Decoding };
        State state = Idle;
        std::vector<VitGroup> vls;       // the Viterbi launches of the sub-batch
        VitMode vit_mode = VIT_COUNT;    // or VIT_MARK (modification pass follows)
        Extras ex;                       // the switches when the sub-batch was launched: the unit pass, the forward pass, the per-unit scores (behind the modification pass) follow
        bool scan = false;               // a scan sub-batch: a read without a winner has no row
        int64_t r0 = 0; int nr = 0;
        const char* flt_base = nullptr;  // where the filtered signal of the sub-batch starts in `flt` (ReadCond::off counts from here)
        std::vector<int32_t> vit_slot;
        PinBuf pinned;
        hipEvent_t fwd_done = nullptr, v0 = nullptr, v1 = nullptr;
        // the pinned block of the slot: what the host reads of a sub-batch of `nr` reads
        struct Pinned {
            ReadGeom* geom; VitResult* vres; ReadCond* rc; unsigned int* redo; size_t bytes;
            Pinned(void* base, int n)
            {
                Carve L;
                geom = Carve::at<ReadGeom>(base, L.add<ReadGeom>(n)); vres = Carve::at<VitResult>(base, L.add<VitResult>(n));
                rc = Carve::at<ReadCond>(base, L.add<ReadCond>(n)); redo = Carve::at<unsigned int>(base, L.add<unsigned int>(1));
                bytes = L.total();
            }
        };
        Pinned host() const { return Pinned(pinned.p, nr); }
        // buffers and pinned block for a sub-batch of `n` reads with `flt_bytes` of filtered signal
        int reserve(strq_ctx* c, int n, size_t flt_bytes)
        {
            STRQ_HIP(c, flt.reserve(flt_bytes));
            STRQ_HIP(c, vit.reserve((size_t)n * sizeof(VitTask)));
            STRQ_HIP(c, vres.reserve((size_t)n * sizeof(VitResult)));
            STRQ_HIP(c, order.reserve((size_t)n * 4 + 64));
            STRQ_HIP(c, vq.reserve(1024));
            STRQ_HIP(c, pinned.reserve(Pinned(nullptr, n).bytes + 64));
            return STRQ_OK;
        }
    };
    Slot slot[2];
    int next_slot = 0;
    // samples of the NEXT sub-batch travel host -> HBM on a thread of their own while this thread sequences the kernels of the current one
    // (align_core blocks it in three host round trips per sub-batch: an upload from the same thread only started when those were through,
    // and the GPU idled under it -- 250 ms per 4096 reads instead of 175: gpurun_out/r6n)
    std::thread up_thread;
    int up_rc = 0;
    hipStream_t vit_stream = nullptr;
    int levels_shift = 0;                // bytes the level stream of the current sub-batch starts behind the buffer's base (alignment phase)
    // strq_debug_filtered: the slot that holds the filtered signal of the last sub-batch, the bytes it starts behind the buffer's base, its reads
    int last_slot = -1, flt_shift = 0, last_nr = 0;
    hipStream_t copy_stream = nullptr;   // host -> HBM uploads that overlap the kernels of the previous sub-batch
    static constexpr int N_STAGE = 4;    // pinned staging ring of upload_reads
    PinBuf stage[N_STAGE]; hipEvent_t stage_ev[N_STAGE] = {}; bool stage_busy[N_STAGE] = {};
};

// the target of a read of the batch and its models: the flanked one, the modification model, the anchored model of a read of `kind`
static const Target& target_of(const DetectState* d, int64_t read) { return d->targets[d->batch.target[(size_t)read]]; }
static HostModel* flank_model(const strq_ctx* c, const DetectState* d, int64_t read) { return c->models[target_of(d, read).model_id]; }
// the dual models of a target: the modification model (base | mCpG over two pore models), the variant model (repeat unit | alt units)
enum Dual { DUAL_MOD, DUAL_VAR };
static int dual_id(const Target& t, Dual which) { return which == DUAL_MOD ? t.mod_model_id : t.var_model_id; }
static HostModel* dual_model(const strq_ctx* c, const DetectState* d, int64_t read, Dual which) { return c->models[dual_id(target_of(d, read), which)]; }
static HostModel* mod_model(const strq_ctx* c, const DetectState* d, int64_t read) { return dual_model(c, d, read, DUAL_MOD); }
static HostModel* anchored_model(const strq_ctx* c, const DetectState* d, int64_t read, int kind)
{
    return c->models[kind == ANCH_ENDS ? target_of(d, read).end_model_id : target_of(d, read).start_model_id];
}

static int upload_join(DetectState* d);

static DetectState* dstate(strq_ctx* c)
{
    if (!c->detect) c->detect = new DetectState();
    return static_cast<DetectState*>(c->detect);
}

void detect_state_free(strq_ctx* c)
{
    if (!c->detect) return;
    DetectState* d = static_cast<DetectState*>(c->detect);
    (void)upload_join(d);
    if (d->vit_stream) (void)hipStreamSynchronize(d->vit_stream);
    for (auto& sl : d->slot)
        for (hipEvent_t e : {sl.fwd_done, sl.v0, sl.v1}) if (e) (void)hipEventDestroy(e);
    if (d->vit_stream) (void)hipStreamDestroy(d->vit_stream);
    for (hipEvent_t e : d->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->rn_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->amod_ev) if (e) (void)hipEventDestroy(e);
    if (d->copy_stream) (void)hipStreamDestroy(d->copy_stream);
    for (hipEvent_t e : d->stage_ev) if (e) (void)hipEventDestroy(e);
    delete d;          // its buffers, device and pinned, go with it
    c->detect = nullptr;
}

// One group of Viterbi tasks (`tasks`, `results`, `order`: the arrays the group's range indexes).  Its tasks in descending window length
// first, where vit_sort_kernel takes that many ...
static int* group_order(int* order, const VitGroup& g) { return g.count <= 8192 ? order + g.first : nullptr; }
static int sort_viterbi_group(strq_ctx* c, hipStream_t st, const VitGroup& g, const VitTask* tasks, int* order)
{
    int* d_order = group_order(order, g);
    if (d_order && launch_vit_sort(st, tasks + g.first, g.count, d_order)) { c->err = "sort launch failed"; return STRQ_ERR_DEVICE; }
    return STRQ_OK;
}
// ... then the persistent launch in decode mode `mode` on queue head `queue` (`what`: who says that the shape has no such mode)
static int launch_viterbi_group(strq_ctx* c, hipStream_t st, const VitGroup& g, const VitTask* tasks, VitResult* results, int* order, int* queue,
                                VitMode mode, int waves_hint = 0, const char* what = "viterbi: ", bool tracts = false)
{
    const int vrc = launch_viterbi(st, g.shape, g.max_cells, tasks + g.first, results + g.first, g.count, queue, c->n_cu, mode, group_order(order, g), waves_hint, tracts);
    if (viterbi_launch_status(vrc) == STRQ_ERR_UNSUPPORTED) c->err = std::string(what) + "decode mode not available for this model's kernel shape";
    else if (vrc) c->err = "viterbi launch failed";
    return viterbi_launch_status(vrc);
}

// The launches of a second decode of a sub-batch (unit pass, forward pass, tract pass, anchored pass, dual models), on stream `st` with
// the context's queue heads: the heads are reset, then group by group the sort and the launch.  What differs between the passes:
using GroupHook = std::function<int(const VitGroup&)>;
struct GroupDecode {
    VitTask* tasks; VitResult* results; int* order;      // the arrays the groups index; the order buffer is the slot's, or the pass's own
    VitMode mode[2];                                     // decode mode of a group by its route (the unit pass alone has two routes)
    const char* what; bool tracts;                       // who says that the shape has no such mode; the wide payload of the tract counts
    double* launches;                                    // (or null) takes 2 for a sorted group, 1 otherwise
    GroupHook before, after;                             // (or none) in front of a group's sort; behind its launch
    std::function<int(const VitGroup&, int*)> launch;    // (or none) in place of sort and launch: the forward pass's own two on a queue head
};
static int launch_groups(strq_ctx* c, hipStream_t st, const std::vector<VitGroup>& groups, const GroupDecode& v)
{
    if (const int qrc = reset_queue_heads(c, st)) return qrc;
    int qi = 0;
    for (const VitGroup& g : groups) {
        int* queue = c->queue.as<int>() + qi++;
        if (v.before) { if (const int rc = v.before(g)) return rc; }
        if (v.launch) { if (const int rc = v.launch(g, queue)) return rc; }
        else {
            if (const int src = sort_viterbi_group(c, st, g, v.tasks, v.order)) return src;
            if (const int lrc = launch_viterbi_group(c, st, g, v.tasks, v.results, v.order, queue, v.mode[g.route], 0, v.what, v.tracts)) return lrc;
            if (v.launches) *v.launches += group_order(v.order, g) ? 2 : 1;
        }
        if (v.after) { if (const int rc = v.after(g)) return rc; }
    }
    return STRQ_OK;
}

// read-back of the modification pass: the lengths first, then the strings gathered into a dense pool (the sparse buffer has one byte per
// time step: ~180 MB per 4096 reads of 50 kb, 25 ms through pageable memory, for ~4 MB of strings)
static int read_mod_patterns(strq_ctx* c, DetectState* d, int64_t r0, const std::vector<int>& who, const std::vector<int>& slot2, const std::vector<int64_t>& len,
                             const std::vector<size_t>& p2_off, const int64_t* d_plen, const char* d_chars, std::vector<std::string>& dst)
{
    hipStream_t st = c->stream;
    const int nm = (int)who.size();
    std::vector<int64_t> plen(nm);
    STRQ_HIP(c, hipMemcpyAsync(plen.data(), d_plen, (size_t)nm * 8, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    std::vector<GatherTask> gt(nm); size_t dense = 0;
    for (int k = 0; k < nm; ++k) {
        const int64_t ln = std::max<int64_t>(0, std::min<int64_t>(plen[slot2[k]], len[k] + 1));
        gt[k] = {(int64_t)p2_off[k], (int64_t)dense, ln}; dense += (size_t)ln;
    }
    STRQ_HIP(c, d->modpool.reserve(dense + (size_t)nm * sizeof(GatherTask) + 64));
    GatherTask* d_gt = d->modpool.as<GatherTask>(); char* d_dense = reinterpret_cast<char*>(d_gt + nm);
    STRQ_HIP(c, hipMemcpyAsync(d_gt, gt.data(), (size_t)nm * sizeof(GatherTask), hipMemcpyHostToDevice, st));
    if (launch_mod_gather(st, d_gt, nm, d_chars, d_dense)) { c->err = "gather launch failed"; return STRQ_ERR_DEVICE; }
    std::vector<char> chars(dense + 1);
    if (dense) STRQ_HIP(c, hipMemcpyAsync(chars.data(), d_dense, dense, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    for (int k = 0; k < nm; ++k) dst[(size_t)(r0 + who[k])] = std::string(chars.data() + gt[k].dst, (size_t)gt[k].len);
    return STRQ_OK;
}

// The edge image of a dual model for the per-unit scores (HostModel::llr_dev), built if it is not there; STRQ_ERR_UNSUPPORTED
// (c->err says why) for a model the pass does not cover.
static int llr_model(strq_ctx* c, HostModel* hm)
{
    if (hm->llr_dev) return STRQ_OK;
    if (hm->llr_blob.reserve(llr_image_bytes()) != hipSuccess) { c->err = "out of device memory"; return STRQ_ERR_NOMEM; }
    std::vector<char> blob; std::string why; int32_t mode = -1;
    if (llr_build_image(hm->n_states, hm->silent_start, hm->start, hm->end, hm->in_ptr.data(), hm->in_src.data(), hm->in_logp.data(),
                        hm->emis_kind.data(), hm->emis_a.data(), hm->emis_b.data(), hm->emis_c.data(),
                        hm->state_tag.empty() ? nullptr : hm->state_tag.data(), hm->llr_blob.p, blob, &mode, why)) { c->err = why; return STRQ_ERR_UNSUPPORTED; }
    STRQ_HIP(c, hipMemcpy(hm->llr_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    hm->llr_dev = hm->llr_blob.as<LlrModel>(); hm->llr_mode = mode;
    return STRQ_OK;
}

// GPU time of a pass on the context's stream, between the events ev[0] and ev[1]: pass_start before its first command (it makes the
// events if they are not there), pass_stop behind its last one -- it waits for the stream and adds the milliseconds in between to
// `into`.  The passes share the pair pass_ev(d); the methylation calls of anchored reads run inside the anchored pass's bracket and
// have a pair of their own (DetectState::amod_ev).
static hipEvent_t* pass_ev(DetectState* d) { return d->ev + 2; }
static int pass_start(strq_ctx* c, hipEvent_t* ev)
{
    for (int k = 0; k < 2; ++k) if (!ev[k]) STRQ_HIP(c, hipEventCreate(&ev[k]));
    STRQ_HIP(c, hipEventRecord(ev[0], c->stream));
    return STRQ_OK;
}
static int pass_stop(strq_ctx* c, hipEvent_t* ev, PassStats& into)
{
    STRQ_HIP(c, hipEventRecord(ev[1], c->stream));
    STRQ_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0; STRQ_HIP(c, hipEventElapsedTime(&ms, ev[0], ev[1])); into.ms += ms;
    return STRQ_OK;
}

// The decoded windows of a sub-batch whose rows are being taken: the reads whose gate passed and whose flanked model found a path, and
// the slot's Viterbi tasks (same windows, same affine source) as the count / MARK launch had them.  The unit pass and the forward pass
// both start from here; the tasks are read back once, and only when there is a decoded read.
struct Decoded { std::vector<int> who; std::vector<VitTask> vt; };
static int read_decoded(strq_ctx* c, DetectState::Slot& sl, Decoded& out)
{
    const ReadGeom* geom = sl.host().geom; const VitResult* vres = sl.host().vres;
    for (int i = 0; i < sl.nr; ++i)
        if (geom[i].gate && vres[sl.vit_slot[i]].status == 0) out.who.push_back(i);
    if (out.who.empty()) return STRQ_OK;
    out.vt.resize((size_t)sl.nr);
    STRQ_HIP(c, hipMemcpyAsync(out.vt.data(), sl.vit.p, (size_t)sl.nr * sizeof(VitTask), hipMemcpyDeviceToHost, c->stream));
    STRQ_HIP(c, hipStreamSynchronize(c->stream));
    return STRQ_OK;
}

// what run_mod_pass hands to run_llr_pass: its reads, where their decode left signal, records / paths and results
struct LlrPassIn {
    const std::vector<int>* who; const std::vector<int>* slot2; const std::vector<int64_t>* len;
    const std::vector<size_t>* sig_off; const std::vector<size_t>* bp2_off; const std::vector<int32_t*>* paths;
    bool use_hub; VitResult* results;
    // whose patterns are scored and where the scores go: the rows' (Batch::mod / llr), or the anchored calls' (Batch::amod / amod_llr)
    const std::vector<std::string>* pattern; std::vector<std::vector<double>>* scores; bool anchored;
};

// Per-unit scores of the reads of one sub-batch (strq_set_mod_llr; mod_llr_kernels.h): behind the pattern read-back of run_mod_pass, on
// the context's stream.  The pattern lengths size everything: one bound and two doubles per unit.
static int run_llr_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl, const LlrPassIn& in)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0;
    const std::vector<int>& who = *in.who;
    const int nm = (int)who.size();
    std::vector<int64_t> n_units((size_t)nm), unit_off((size_t)nm + 1, 0);
    for (int k = 0; k < nm; ++k) {
        const std::string& pat = (*in.pattern)[(size_t)(r0 + who[k])];
        n_units[(size_t)k] = pat == "-" ? 0 : (int64_t)pat.size();
        unit_off[(size_t)k + 1] = unit_off[(size_t)k] + n_units[(size_t)k];
    }
    const int64_t U = unit_off[(size_t)nm];
    if (!U) return STRQ_OK;
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    // reads with units, by kernel mode (states per lane / units per wave)
    std::vector<int> by_mode[3];
    for (int k = 0; k < nm; ++k) {
        if (!n_units[(size_t)k]) continue;
        HostModel* hm = mod_model(c, d, r0 + who[k]);
        // the image was built, and a model without one refused, when the switch went on or the target's model was registered:
        // nothing is built or refused in the middle of a batch
        if (!hm->llr_dev || hm->llr_mode < 0 || hm->llr_mode > 2) { c->err = "mod-llr: modification model without an edge image (strq_set_mod_llr validates them)"; return STRQ_ERR_DEVICE; }
        by_mode[hm->llr_mode].push_back(k);
    }
    Carve lay;
    const size_t o_out = lay.add<double>(2 * (size_t)U), o_w = lay.add<int32_t>((size_t)U), o_bt = lay.add<LlrBoundTask>((size_t)nm),
                 o_rd = lay.add<LlrRead>((size_t)nm), o_first = lay.add<int64_t>((size_t)nm + 3), o_bad = lay.add<int32_t>((size_t)nm);
    STRQ_HIP(c, d->llr_ws.reserve(lay.total() + 64));
    void* ws = d->llr_ws.p;
    double* d_out = Carve::at<double>(ws, o_out); int32_t* d_w = Carve::at<int32_t>(ws, o_w);
    LlrBoundTask* d_bt = Carve::at<LlrBoundTask>(ws, o_bt); LlrRead* d_rd = Carve::at<LlrRead>(ws, o_rd);
    int64_t* d_first = Carve::at<int64_t>(ws, o_first); int32_t* d_bad = Carve::at<int32_t>(ws, o_bad);
    std::vector<LlrBoundTask> bt; std::vector<LlrRead> rdv; std::vector<int64_t> first;
    struct L { int mode, at, n, first_at; int64_t units; };
    std::vector<L> launches;
    for (int mode = 0; mode < 3; ++mode) {
        if (by_mode[mode].empty()) continue;
        L l = {mode, (int)rdv.size(), (int)by_mode[mode].size(), (int)first.size(), 0};
        for (int k : by_mode[mode]) {
            HostModel* hm = mod_model(c, d, r0 + who[k]);
            const int s2 = (*in.slot2)[(size_t)k];
            LlrBoundTask b; std::memset(&b, 0, sizeof(b));
            b.rec = in.use_hub ? reinterpret_cast<const uint64_t*>(d->bp.as<uint16_t>() + (*in.bp2_off)[(size_t)k]) : nullptr;
            b.result = in.results + s2; b.path = in.use_hub ? nullptr : (*in.paths)[(size_t)s2]; b.tag = hm->h.state_tag;
            b.w = d_w + unit_off[(size_t)k]; b.n = n_units[(size_t)k]; b.T = (*in.len)[(size_t)k]; b.bad = d_bad + (int)bt.size();
            bt.push_back(b);
            LlrRead r; r.model = hm->llr_dev; r.x = d->modsig.as<double>() + (*in.sig_off)[(size_t)k]; r.w = b.w;
            r.out = d_out + 2 * unit_off[(size_t)k]; r.T = b.T;
            rdv.push_back(r);
            first.push_back(l.units); l.units += n_units[(size_t)k];
        }
        first.push_back(l.units);
        launches.push_back(l);
    }
    const int nb = (int)bt.size();
    STRQ_HIP(c, hipMemcpyAsync(d_bt, bt.data(), (size_t)nb * sizeof(LlrBoundTask), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_rd, rdv.data(), (size_t)nb * sizeof(LlrRead), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_first, first.data(), first.size() * 8, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemsetAsync(d_bad, 0, (size_t)nb * 4, st));
    STRQ_HIP(c, hipMemsetAsync(d_w, 0xFF, (size_t)U * 4, st));          // a bound nobody wrote is -1: its unit scores -inf, -inf
    if (launch_llr_bounds(st, in.use_hub ? d_bt : nullptr, in.use_hub ? nb : 0, in.use_hub ? nullptr : d_bt, in.use_hub ? 0 : nb)) { c->err = "mod-llr: bounds launch failed"; return STRQ_ERR_DEVICE; }
    for (const L& l : launches)
        if (launch_llr_score(st, l.mode, d_rd + l.at, d_first + l.first_at, l.n, l.units, c->n_cu)) { c->err = "mod-llr: launch failed"; return STRQ_ERR_DEVICE; }
    std::vector<double> out((size_t)U * 2); std::vector<int32_t> bad((size_t)nb);
    STRQ_HIP(c, hipMemcpyAsync(out.data(), d_out, (size_t)U * 16, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(bad.data(), d_bad, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    if (const int rc = pass_stop(c, pass_ev(d), d->stats[in.anchored ? PASS_AMOD : PASS_LLR])) return rc;
    for (int32_t b : bad) if (b) { c->err = "mod-llr: the unit bounds of a read disagree with its pattern"; return STRQ_ERR_DEVICE; }
    for (int k = 0; k < nm; ++k)
        if (n_units[(size_t)k]) (*in.scores)[(size_t)(r0 + who[k])].assign(out.begin() + (ptrdiff_t)(2 * unit_off[(size_t)k]), out.begin() + (ptrdiff_t)(2 * unit_off[(size_t)k + 1]));
    if (in.anchored) { d->stat(PASS_AMOD, AMOD_LAUNCHES) += 1 + (double)launches.size(); return STRQ_OK; }
    d->stat(PASS_LLR, LLR_UNITS) += (double)U; d->stat(PASS_LLR, LLR_READS) += nb; d->stat(PASS_LLR, LLR_LAUNCHES) += 1 + (double)launches.size();
    return STRQ_OK;
}

// The edge image of a variant model with `n_alt` alt branches (HostModel::var_dev), built if it is not there; STRQ_ERR_UNSUPPORTED
// (c->err says why) for a model the pass does not cover.  `decoded`: the model is to be decoded as well (the pipeline), so it must
// fit a Viterbi kernel; strq_debug_variant_scores scores given passages only.
static int variant_model(strq_ctx* c, HostModel* hm, int32_t n_alt, bool decoded = true)
{
    const char* no_shape = "variants: the variant model does not fit a compiled Viterbi kernel";
    if (hm->var_dev && hm->var_nb == n_alt + 1) {
        if (decoded && vit_shape_of(hm->h) < 0) { c->err = no_shape; return STRQ_ERR_UNSUPPORTED; }          // (an image the hook built)
        return STRQ_OK;
    }
    std::vector<char> blob; std::string why; int32_t mode = -1;
    if (var_build_image(hm->n_states, hm->silent_start, hm->start, hm->end, hm->in_ptr.data(), hm->in_src.data(), hm->in_logp.data(),
                        hm->emis_kind.data(), hm->emis_a.data(), hm->emis_b.data(), hm->emis_c.data(),
                        hm->state_tag.empty() ? nullptr : hm->state_tag.data(), n_alt, nullptr, blob, &mode, why)) { c->err = why; return STRQ_ERR_UNSUPPORTED; }
    if (decoded && vit_shape_of(hm->h) < 0) { c->err = no_shape; return STRQ_ERR_UNSUPPORTED; }
    if (hm->var_blob.reserve(var_image_bytes()) != hipSuccess) { c->err = "out of device memory"; return STRQ_ERR_NOMEM; }
    var_build_image(hm->n_states, hm->silent_start, hm->start, hm->end, hm->in_ptr.data(), hm->in_src.data(), hm->in_logp.data(),
                    hm->emis_kind.data(), hm->emis_a.data(), hm->emis_b.data(), hm->emis_c.data(), hm->state_tag.data(), n_alt, hm->var_blob.p, blob, &mode, why);
    STRQ_HIP(c, hipMemcpy(hm->var_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    hm->var_dev = hm->var_blob.as<VarModel>(); hm->var_mode = mode; hm->var_nb = n_alt + 1;
    return STRQ_OK;
}

// The task of the count pass of the variant bounds kernels for one read of T observations: its hub records (or null and its traced
// path), the result of its decode, the model's tags; no bounds yet, and cap = T / 3 + 1 -- a passage takes three observations at
// least (s0, one branch emission, e0).  The write pass is the same task with w, branch and the count as cap filled in.
static VarBoundTask var_count_task(const uint64_t* rec, const VitResult* result, const int32_t* path, const int32_t* tag, int32_t* n, int32_t* bad,
                                   int64_t T, int32_t n_branch)
{
    VarBoundTask b; std::memset(&b, 0, sizeof(b));
    b.rec = rec; b.result = result; b.path = path; b.tag = tag;
    b.w = nullptr; b.branch = nullptr; b.n = n; b.bad = bad;
    b.T = T; b.cap = (int32_t)(T / 3 + 1); b.n_branch = n_branch;
    return b;
}

// Behind the decode of the variant models of one sub-batch (run_mod_pass, DUAL_VAR): the passages of every read from its hub records
// or its traced path (their number comes back first: it sizes the scores), all branches' scores of every passage, the rows.
static int run_variant_tail(strq_ctx* c, DetectState* d, DetectState::Slot& sl, const LlrPassIn& in, const std::vector<int64_t>& first)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0;
    const ReadGeom* geom = sl.host().geom;
    const std::vector<int>& who = *in.who;
    const int nm = (int)who.size();
    // count pass (var_count_task)
    Carve lay;
    const size_t o_n = lay.add<int32_t>((size_t)nm), o_bad = lay.add<int32_t>((size_t)nm), o_bt = lay.add<VarBoundTask>((size_t)nm),
                 o_rd = lay.add<VarRead>((size_t)nm), o_first = lay.add<int64_t>((size_t)nm + 16);
    STRQ_HIP(c, d->var_ws.reserve(lay.total() + 64));
    void* ws = d->var_ws.p;
    int32_t* d_n = Carve::at<int32_t>(ws, o_n); int32_t* d_bad = Carve::at<int32_t>(ws, o_bad);
    VarBoundTask* d_bt = Carve::at<VarBoundTask>(ws, o_bt); VarRead* d_rd = Carve::at<VarRead>(ws, o_rd);
    int64_t* d_first = Carve::at<int64_t>(ws, o_first);
    std::vector<VarBoundTask> bt((size_t)nm);
    for (int k = 0; k < nm; ++k) {
        HostModel* hm = dual_model(c, d, r0 + who[k], DUAL_VAR);
        // (strq_target_set_variants built the image or refused the model: nothing is built or refused in the middle of a batch)
        if (!hm->var_dev || hm->var_mode < 0 || hm->var_mode > 2) { c->err = "variants: variant model without an edge image (strq_target_set_variants validates them)"; return STRQ_ERR_DEVICE; }
        const int s2 = (*in.slot2)[(size_t)k];
        bt[(size_t)k] = var_count_task(in.use_hub ? reinterpret_cast<const uint64_t*>(d->bp.as<uint16_t>() + (*in.bp2_off)[(size_t)k]) : nullptr, in.results + s2,
                                       in.use_hub ? nullptr : (*in.paths)[(size_t)s2], hm->h.state_tag, d_n + k, d_bad + k, (*in.len)[(size_t)k], hm->var_nb);
    }
    auto bounds = [&]() -> int {
        STRQ_HIP(c, hipMemcpyAsync(d_bt, bt.data(), (size_t)nm * sizeof(VarBoundTask), hipMemcpyHostToDevice, st));
        if (launch_var_bounds(st, in.use_hub ? d_bt : nullptr, in.use_hub ? nm : 0, in.use_hub ? nullptr : d_bt, in.use_hub ? 0 : nm)) { c->err = "variants: bounds launch failed"; return STRQ_ERR_DEVICE; }
        return STRQ_OK;
    };
    STRQ_HIP(c, hipMemsetAsync(d_n, 0, (size_t)nm * 4, st));
    STRQ_HIP(c, hipMemsetAsync(d_bad, 0, (size_t)nm * 4, st));
    if (const int rc = bounds()) return rc;
    std::vector<int32_t> np((size_t)nm), bad((size_t)nm); std::vector<VitResult> vr((size_t)nm);
    STRQ_HIP(c, hipMemcpyAsync(np.data(), d_n, (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(bad.data(), d_bad, (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(vr.data(), in.results, (size_t)nm * sizeof(VitResult), hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    const char* no_chain = "variants: the hub records / the traced path of a read do not describe a chain of passages";
    std::vector<size_t> cap_off((size_t)nm + 1, 0);
    for (int k = 0; k < nm; ++k) {
        if (bad[(size_t)k] || np[(size_t)k] < 0 || np[(size_t)k] > bt[(size_t)k].cap) { c->err = no_chain; return STRQ_ERR_DEVICE; }
        cap_off[(size_t)k + 1] = cap_off[(size_t)k] + (size_t)np[(size_t)k];
    }
    // write pass: the counts size the bounds -- dense, exactly as many as were counted (another number sets `bad`)
    const size_t caps = cap_off[(size_t)nm];
    STRQ_HIP(c, d->var_bounds.reserve(caps * 8 + 64));
    int32_t* d_w = d->var_bounds.as<int32_t>(); int32_t* d_br = d_w + caps;
    std::vector<int32_t> w(caps + 1), br(caps + 1);
    double launches = in.use_hub ? 1 : 2;          // count pass (behind the traceback on the back-pointer route)
    if (caps) {
        for (int k = 0; k < nm; ++k) { VarBoundTask& b = bt[(size_t)k]; b.w = d_w + cap_off[(size_t)k]; b.branch = d_br + cap_off[(size_t)k]; b.cap = np[(size_t)k]; }
        if (const int rc = bounds()) return rc;
        launches += 1;
        STRQ_HIP(c, hipMemcpyAsync(w.data(), d_w, caps * 4, hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipMemcpyAsync(br.data(), d_br, caps * 4, hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipMemcpyAsync(bad.data(), d_bad, (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    }
    // scores: the reads with passages by (kernel mode, branches), NB doubles per passage, dense
    std::vector<size_t> v_off((size_t)nm + 1, 0);
    for (int k = 0; k < nm; ++k) v_off[(size_t)k + 1] = v_off[(size_t)k] + (size_t)np[(size_t)k] * (size_t)dual_model(c, d, r0 + who[k], DUAL_VAR)->var_nb;
    const size_t nv = v_off[(size_t)nm];
    std::vector<double> out(nv + 1);
    double passages = 0;
    if (nv) {
        STRQ_HIP(c, d->var_out.reserve(nv * 8 + 64));
        double* d_out = d->var_out.as<double>();
        std::vector<VarRead> rdv; std::vector<int64_t> firstv;
        struct L { int mode, nb, at, n, first_at; int64_t passages; };
        std::vector<L> ls;
        for (int mode = 0; mode < 3; ++mode)
            for (int nb = 2; nb <= VAR_MAX_NB; ++nb) {
                L l = {mode, nb, (int)rdv.size(), 0, (int)firstv.size(), 0};
                for (int k = 0; k < nm; ++k) {
                    HostModel* hm = dual_model(c, d, r0 + who[k], DUAL_VAR);
                    if (!np[(size_t)k] || hm->var_mode != mode || hm->var_nb != nb) continue;
                    VarRead r; r.model = hm->var_dev; r.x = d->modsig.as<double>() + (*in.sig_off)[(size_t)k]; r.w = d_w + cap_off[(size_t)k];
                    r.out = d_out + v_off[(size_t)k]; r.T = (*in.len)[(size_t)k];
                    rdv.push_back(r); firstv.push_back(l.passages); l.passages += np[(size_t)k]; ++l.n;
                }
                if (!l.n) continue;
                firstv.push_back(l.passages); ls.push_back(l);
            }
        if (firstv.size() > (size_t)nm + 16) { c->err = "variants: workspace"; return STRQ_ERR_NOMEM; }
        STRQ_HIP(c, hipMemcpyAsync(d_rd, rdv.data(), rdv.size() * sizeof(VarRead), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_first, firstv.data(), firstv.size() * 8, hipMemcpyHostToDevice, st));
        for (const L& l : ls) {
            if (launch_var_score(st, l.mode, l.nb, d_rd + l.at, d_first + l.first_at, l.n, l.passages, c->n_cu)) { c->err = "variants: launch failed"; return STRQ_ERR_DEVICE; }
            passages += (double)l.passages;
        }
        launches += (double)ls.size();
        STRQ_HIP(c, hipMemcpyAsync(out.data(), d_out, nv * 8, hipMemcpyDeviceToHost, st));
    }
    if (const int rc = pass_stop(c, pass_ev(d), d->stats[PASS_VAR])) return rc;
    for (int32_t b : bad) if (b) { c->err = no_chain; return STRQ_ERR_DEVICE; }
    for (int k = 0; k < nm; ++k) {
        const int i = who[k]; const Target& t = target_of(d, r0 + i);
        if (vr[(size_t)(*in.slot2)[(size_t)k]].status != 0) continue;          // the variant model found no path: not decoded
        VariantRow& row = B.var[(size_t)(r0 + i)];
        row.decoded = 1; row.n_branch = t.var_nalt + 1;
        const int n = np[(size_t)k]; int64_t units = 0;
        row.branch.resize((size_t)n); row.end.resize((size_t)n);
        for (int j = 0; j < n; ++j) {
            const int32_t b = br[cap_off[(size_t)k] + (size_t)j];
            row.branch[(size_t)j] = (int8_t)b; units += b ? t.var_ctx + 1 : 1;
            // observation t of the stretch is raw sample first + t: the repeat section of a flanked model is one contiguous stretch
            row.end[(size_t)j] = geom[i].prefix_begin + first[(size_t)k] + (int64_t)w[cap_off[(size_t)k] + (size_t)j];
        }
        row.V.assign(out.begin() + (ptrdiff_t)v_off[(size_t)k], out.begin() + (ptrdiff_t)v_off[(size_t)k + 1]);
        row.count_v = (int32_t)(units + t.count_bias);
        d->stat(PASS_VAR, VAR_READS) += 1;
    }
    d->stat(PASS_VAR, VAR_LAUNCHES) += launches; d->stat(PASS_VAR, VAR_PASSAGES) += passages;
    return STRQ_OK;
}

// Steps 1 to 3 of a dual-model pass for a list of stretches, and what they leave for the steps behind them.  A stretch is `len`
// raw samples of read `who` of the sub-batch from sample `raw_first` of that read: the samples a MARK decode put into the repeat
// section (detect step 13, STRique.py:608, hands exactly those to repeatModHMM.mod_repeats, STRique.py:492-500,605-609).  The
// spanning caller (run_mod_pass) knows its stretches on the host; the anchored caller (run_anchored_mod) may know only the windows
// they lie in: then `len` is that bound, it sizes every buffer, and anchored_mod_task_kernel writes the tasks from the device copies
// of the records (`dev`) -- nothing waits for the host between the anchored decode and the pattern read-back.
struct AnchoredModSrc { const AnchoredClass* cls; const ReadCond* rc; const VitResult* res; int n_res; std::vector<int32_t> res_of; };
struct DualRun {
    std::vector<int> who; std::vector<int64_t> raw_first, len;
    std::vector<size_t> sig_off, bp2_off, p2_off; std::vector<int> slot2; std::vector<int32_t*> tp2;
    bool use_hub = false; double launches = 0;
    VitTask* d_tb = nullptr; VitResult* d_tr = nullptr; int32_t** d_tp = nullptr; PatTask* d_pt = nullptr;
    char* d_chars = nullptr; int64_t* d_plen = nullptr; HubTask* d_ht = nullptr;
};
// hub records (one 8-byte record per time step, read back with one hop per repeat unit) when every model of the list has the hub
// structure; back-pointers + traceback otherwise
static int dual_route(strq_ctx* c, DetectState* d, int64_t r0, Dual which, const DualRun& R, std::vector<GroupItem>& items, bool& use_hub)
{
    const int nm = (int)R.who.size();
    items.resize((size_t)nm);
    use_hub = !strq::opt("STRQ_MOD_BACKPOINTERS");
    for (int k = 0; k < nm; ++k) {
        HostModel* hm = dual_model(c, d, r0 + R.who[k], which);
        const int shape = vit_shape_of(hm->h);
        if (shape < 0) { c->err = "modification model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
        items[k] = {0, shape, hm->h.n_cells};
        if (hm->h.rec_state < 0 || !vit_mode_ok(shape, VIT_HUB) || R.len[k] >= ((int64_t)1 << 31)) use_hub = false;
    }
    return STRQ_OK;
}
static int dual_decode(strq_ctx* c, DetectState* d, DetectState::Slot& sl, Dual which, DualRun& R, const AnchoredModSrc* dev = nullptr)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0;
    const ReadCond* rc = sl.host().rc;
    const int esz = B.dtype == 0 ? 2 : 8;
    const int64_t s0 = B.off[r0];
    const std::vector<int>& who = R.who; const std::vector<int64_t>& len = R.len;
    const int nm = (int)who.size();
    // 1. + 2. the samples decoded into repeat states: one contiguous stretch, renormalised from the raw signal and clipped
    size_t sig_tot = 0; R.sig_off.resize(nm);
    for (int k = 0; k < nm; ++k) { R.sig_off[k] = sig_tot; sig_tot += (size_t)len[k]; }
    const std::vector<size_t>& sig_off = R.sig_off;
    std::vector<GroupItem> items;
    if (const int rrc = dual_route(c, d, r0, which, R, items, R.use_hub)) return rrc;
    const bool use_hub = R.use_hub;
    if (dev && !use_hub) { c->err = "anchored-mod: tasks from the device need the hub route"; return STRQ_ERR_DEVICE; }
    Carve lay;
    const size_t o_tb = lay.add<VitTask>((size_t)nm), o_tr = lay.add<VitResult>((size_t)nm), o_tp = lay.add<int32_t*>((size_t)nm),
                 o_mt = lay.add<ModTask>((size_t)nm), o_pt = lay.add<PatTask>((size_t)nm), o_it = lay.add<AnchoredModItem>(dev ? (size_t)nm : 0);
    STRQ_HIP(c, d->modtask.reserve(lay.total() + 256));
    void* ws = d->modtask.p;
    VitTask* d_tb = Carve::at<VitTask>(ws, o_tb); VitResult* d_tr = Carve::at<VitResult>(ws, o_tr); int32_t** d_tp = Carve::at<int32_t*>(ws, o_tp);
    ModTask* d_mt = Carve::at<ModTask>(ws, o_mt); PatTask* d_pt = Carve::at<PatTask>(ws, o_pt);
    STRQ_HIP(c, d->modsig.reserve(sig_tot * 8 + 64));
    STRQ_HIP(c, d->modlen.reserve((size_t)nm * 16 + 64));
    const Grouping G = group_items(items);
    R.slot2 = G.pos;          // task position of read k
    const std::vector<int>& slot2 = R.slot2;
    std::vector<VitTask> vt2(nm); R.tp2.assign(nm, nullptr);
    size_t bp2 = 0, p2 = 0; R.bp2_off.resize(nm); R.p2_off.resize(nm);
    for (int k = 0; k < nm; ++k) {
        // back-pointers: uint16 per (time step, state); hub records: 8 bytes per time step (in uint16 units: 4)
        R.bp2_off[k] = bp2; bp2 += use_hub ? (size_t)(len[k] + 1) * 4 : (size_t)(len[k] + 1) * dual_model(c, d, r0 + who[k], which)->h.n_states;
        R.p2_off[k] = p2; p2 += (size_t)len[k] + 1;
    }
    STRQ_HIP(c, d->bp.reserve(bp2 * 2 + 64));
    // traced state paths (back-pointer route only), the pattern strings, the tasks of the hub route
    Carve pat;
    const size_t o_path2 = pat.add<int32_t>(use_hub ? 0 : p2), o_chars = pat.add<char>(p2), o_ht = pat.add<HubTask>(use_hub ? (size_t)nm : 0);
    STRQ_HIP(c, d->pattern.reserve(pat.total() + 64));
    int32_t* d_path2 = Carve::at<int32_t>(d->pattern.p, o_path2);
    R.d_chars = Carve::at<char>(d->pattern.p, o_chars); R.d_ht = Carve::at<HubTask>(d->pattern.p, o_ht);
    R.d_tb = d_tb; R.d_tr = d_tr; R.d_tp = d_tp; R.d_pt = d_pt;
    std::vector<ModTask> mt(dev ? 0 : nm);
    if (dev) {
        // the tasks from the records on the device (anchored_mod_task_kernel): both the ModTask and the HUB VitTask of every read
        std::vector<AnchoredModItem> it((size_t)nm);
        for (int k = 0; k < nm; ++k) {
            const Target& t = target_of(d, r0 + who[k]);
            AnchoredModItem& a = it[(size_t)k]; std::memset(&a, 0, sizeof(a));
            a.read = who[k]; a.res = dev->res_of[(size_t)k]; a.slot = slot2[k];
            a.model = dual_model(c, d, r0 + who[k], which)->dev;
            a.out = d->modsig.as<double>() + sig_off[k]; a.bp = d->bp.as<uint16_t>() + R.bp2_off[k];
            a.mod_lo = t.mod_min; a.mod_hi = t.mod_max; a.cap = len[k];
        }
        AnchoredModItem* d_it = Carve::at<AnchoredModItem>(ws, o_it);
        STRQ_HIP(c, hipMemcpyAsync(d_it, it.data(), (size_t)nm * sizeof(AnchoredModItem), hipMemcpyHostToDevice, st));
        AnchoredModTaskArgs ta;
        ta.cls = dev->cls; ta.rc = dev->rc; ta.res = dev->res; ta.item = d_it;
        ta.raw = d->batch.raw.as<char>() + (size_t)s0 * esz; ta.is_f64 = B.dtype;
        ta.clip_lo = d->ps.clip_lo; ta.clip_hi = d->ps.clip_hi;
        ta.mod = d_mt; ta.vit = d_tb; ta.n_items = nm; ta.n_reads = sl.nr; ta.n_res = dev->n_res;
        if (launch_anchored_mod_tasks(st, ta)) { c->err = "anchored-mod: task launch failed"; return STRQ_ERR_DEVICE; }
        R.launches += 1;
    } else {
        for (int k = 0; k < nm; ++k) {
            const int i = who[k]; const Target& t = target_of(d, r0 + i);
            ModTask& m = mt[k];
            m.path = nullptr; m.tag = nullptr;          // contiguous stretch: every sample is kept
            m.raw = d->batch.raw.as<char>() + (size_t)(s0 + rc[i].off + R.raw_first[k]) * esz;
            m.out = d->modsig.as<double>() + sig_off[k]; m.T = len[k]; m.is_f64 = B.dtype; m.pad_ = 0;
            m.c1 = rc[i].r_c1; m.h1 = rc[i].r_h1; m.h2 = rc[i].h2; m.c2 = rc[i].c2;
            m.clip_lo = d->ps.clip_lo; m.clip_hi = d->ps.clip_hi;
            m.mod_lo = which == DUAL_MOD ? t.mod_min : t.var_lo; m.mod_hi = which == DUAL_MOD ? t.mod_max : t.var_hi;
        }
        STRQ_HIP(c, hipMemcpyAsync(d_mt, mt.data(), (size_t)nm * sizeof(ModTask), hipMemcpyHostToDevice, st));
    }
    int64_t* d_len = d->modlen.as<int64_t>();
    R.d_plen = d_len;
    if (launch_mod_compact(st, d_mt, nm, d_len)) { c->err = "compaction launch failed"; return STRQ_ERR_DEVICE; }
    R.launches += 1;
    // 3. Viterbi on the dual model
    for (int k = 0; k < nm; ++k) {
        R.tp2[slot2[k]] = d_path2 + R.p2_off[k];
        if (dev) continue;
        VitTask& v = vt2[slot2[k]]; v = VitTask();
        v.model = dual_model(c, d, r0 + who[k], which)->dev; v.sig = mt[k].out; v.T = len[k]; v.src_kind = VIT_SRC_F64;
        v.bp = d->bp.as<uint16_t>() + R.bp2_off[k];
    }
    GroupHook upload;          // the tasks of a group go up in front of its sort
    if (!dev) upload = [&](const VitGroup& vg) -> int {
        STRQ_HIP(c, hipMemcpyAsync(d_tb + vg.first, vt2.data() + vg.first, (size_t)vg.count * sizeof(VitTask), hipMemcpyHostToDevice, st));
        return STRQ_OK;
    };
    return launch_groups(c, st, G.groups, {d_tb, d_tr, sl.order.as<int>(), {use_hub ? VIT_HUB : VIT_BACKPTR}, "viterbi: ", false, &R.launches, upload});
}

// Step 4 behind dual_decode for a modification model: the pattern strings from the hub records, or from traced paths, into `dst`
static int dual_patterns(strq_ctx* c, DetectState* d, DetectState::Slot& sl, Dual which, DualRun& R, std::vector<std::string>& dst)
{
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0;
    const int nm = (int)R.who.size();
    const std::vector<int>& slot2 = R.slot2;
    if (R.use_hub) {
        // 4. pattern strings from the hub records
        std::vector<HubTask> ht(nm);
        for (int k = 0; k < nm; ++k) {
            const int sl = slot2[k];
            ht[sl].rec = reinterpret_cast<const uint64_t*>(d->bp.as<uint16_t>() + R.bp2_off[k]);
            ht[sl].result = R.d_tr + sl; ht[sl].out = R.d_chars + R.p2_off[k];
        }
        STRQ_HIP(c, hipMemcpyAsync(R.d_ht, ht.data(), (size_t)nm * sizeof(HubTask), hipMemcpyHostToDevice, st));
        if (launch_mod_hub_pattern(st, R.d_ht, nm, R.d_plen)) { c->err = "pattern launch failed"; return STRQ_ERR_DEVICE; }
        R.launches += 1;
    } else {
        STRQ_HIP(c, hipMemcpyAsync(R.d_tp, R.tp2.data(), (size_t)nm * 8, hipMemcpyHostToDevice, st));
        if (launch_vit_traceback(st, R.d_tb, R.d_tr, R.d_tp, nm)) { c->err = "traceback launch failed"; return STRQ_ERR_DEVICE; }
        // 4. pattern strings
        std::vector<PatTask> pt(nm);
        for (int k = 0; k < nm; ++k) {
            const int sl = slot2[k];
            pt[sl].path = R.tp2[sl]; pt[sl].tag = dual_model(c, d, r0 + R.who[k], which)->h.state_tag; pt[sl].out = R.d_chars + R.p2_off[k]; pt[sl].T = R.len[k];
            pt[sl].status = &R.d_tr[sl].status;
        }
        STRQ_HIP(c, hipMemcpyAsync(R.d_pt, pt.data(), (size_t)nm * sizeof(PatTask), hipMemcpyHostToDevice, st));
        if (launch_mod_pattern(st, R.d_pt, nm, R.d_plen)) { c->err = "pattern launch failed"; return STRQ_ERR_DEVICE; }
        R.launches += 2;
    }
    R.launches += 1;          // (the gather of read_mod_patterns)
    return read_mod_patterns(c, d, r0, R.who, slot2, R.len, R.p2_off, R.d_plen, R.d_chars, dst);
}

// what the steps behind the decode take from it
static LlrPassIn dual_tail_in(const DualRun& R)
{
    LlrPassIn li = {};
    li.who = &R.who; li.slot2 = &R.slot2; li.len = &R.len; li.sig_off = &R.sig_off; li.bp2_off = &R.bp2_off; li.paths = &R.tp2;
    li.use_hub = R.use_hub; li.results = R.d_tr;
    return li;
}

// The pass of one of the targets' dual models (`which`) for the reads of one sub-batch whose target has that model: the modification
// pass (patterns, and the per-unit scores behind them), or the variant pass (strq_set_variants: passages and their scores).
// The flanked-model Viterbi ran in MARK mode (viterbi_kernels.hip): its result carries the first and
// last sample decoded into the repeat section, which is all detect step 13 (STRique.py:608) needs.
static int run_mod_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl, Dual which = DUAL_MOD)
{
    Batch& B = d->batch;
    const int64_t r0 = sl.r0; const int nr = sl.nr;
    const DetectState::Slot::Pinned h = sl.host();
    const ReadGeom* geom = h.geom; const VitResult* vres = h.vres;
    const std::vector<int32_t>& vit_slot = sl.vit_slot;
    DualRun R;
    std::vector<int>& who = R.who;             // reads that reach the modification model
    for (int i = 0; i < nr; ++i) {
        if (dual_id(target_of(d, r0 + i), which) < 0 || !geom[i].gate) continue;
        const VitResult& v = vres[vit_slot[i]];
        if (v.status == 2 && which == DUAL_VAR) continue;          // not decoded: no variants
        if (v.status == 2) { c->err = "modification pass: repeat window of 2^21 samples or more"; return STRQ_ERR_UNSUPPORTED; }
        if (v.status == 0) who.push_back(i);
    }
    const int nm = (int)who.size();
    if (!nm) return STRQ_OK;
    if (which == DUAL_VAR) { if (const int rc = pass_start(c, pass_ev(d))) return rc; }          // one bracket around the whole variant pass
    // the samples decoded into repeat states: one contiguous stretch [enter, leave) of the window
    std::vector<int64_t> first(nm);
    R.len.resize(nm); R.raw_first.resize(nm);
    for (int k = 0; k < nm; ++k) {
        const int i = who[k];
        const VitResult& v = vres[vit_slot[i]];
        const int64_t T = geom[i].suffix_end - geom[i].prefix_begin;
        const int64_t enter = v.dbg[0], leave = v.dbg[1];
        first[k] = enter ? enter - 1 : 0;
        R.len[k] = enter ? (leave ? leave - 1 : T) - (enter - 1) : 0;
        R.raw_first[k] = geom[i].prefix_begin + first[k];
    }
    if (const int drc = dual_decode(c, d, sl, which, R)) return drc;
    if (which == DUAL_VAR) {
        // 4. + 5. passages and their scores (the back-pointer route traces the paths first)
        if (!R.use_hub) {
            STRQ_HIP(c, hipMemcpyAsync(R.d_tp, R.tp2.data(), (size_t)nm * 8, hipMemcpyHostToDevice, c->stream));
            if (launch_vit_traceback(c->stream, R.d_tb, R.d_tr, R.d_tp, nm)) { c->err = "traceback launch failed"; return STRQ_ERR_DEVICE; }
        }
        return run_variant_tail(c, d, sl, dual_tail_in(R), first);
    }
    if (const int prc = dual_patterns(c, d, sl, which, R, B.mod)) return prc;
    if (!sl.ex.llr) return STRQ_OK;
    // 5. per-unit scores of both branches: modsig, the records / the traced paths and the results are live until the next pass
    LlrPassIn li = dual_tail_in(R);
    li.pattern = &B.mod; li.scores = &B.llr; li.anchored = false;
    return run_llr_pass(c, d, sl, li);
}

// Unit positions of the reads of one sub-batch (strq_set_units; repeatHMM.count_repeats' path, STRique.py:374-378,433-441): the
// windows the count / MARK launch decoded, once more with the same tasks (same windows, same affine source) -- in UNIT mode (unit
// records, VIT_UNIT_T_MAX) where the model and the window allow it, else (STRQ_UNITS_BACKPOINTERS=1: always) with back-pointers and a
// traceback.  Runs on the context's stream when the rows of the sub-batch are taken: the slot's filtered signal and tasks are live
// until the slot is used again, which harvests it first.  Pieces (detect_plan.h) of records / back-pointers against STRQ_UNITS_WS_BYTES,
// an oversize window alone.  Two routes and two position kernels: it uses the plan, not the traced re-decode.
static int run_unit_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl, const Decoded& dec)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0;
    const ReadGeom* geom = sl.host().geom; const VitResult* vres = sl.host().vres;
    const std::vector<int>& who = dec.who; const std::vector<VitTask>& vt = dec.vt;
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    const bool force_bp = strq::opt("STRQ_UNITS_BACKPOINTERS") != nullptr;
    struct W { int i; int shape; bool rec; };
    std::vector<W> ws; std::vector<size_t> sizes;
    for (int i : who) {
        HostModel* hm = flank_model(c, d, r0 + i);
        const int64_t T = vt[(size_t)sl.vit_slot[i]].T;
        W w; w.i = i; w.shape = vit_shape_for(hm->h, VIT_UNIT);
        w.rec = !force_bp && vit_unit_ok(hm->h, w.shape) && T < VIT_UNIT_T_MAX;
        if (!w.rec) w.shape = vit_shape_of(hm->h);
        if (w.shape < 0) { c->err = "unit pass: model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
        // unit records: two uint32 per observation; back-pointers: uint16 per (time step, state), and the state path
        sizes.push_back(w.rec ? (size_t)T * 8 : (size_t)(T + 1) * (size_t)hm->h.n_states * 2);
        ws.push_back(w);
    }
    const PiecePlan plan = plan_pieces(sizes, ws_budget(strq::opt("STRQ_UNITS_WS_BYTES")), OVERSIZE_ALONE);
    for (const Piece& pc : plan.pieces) {
        const size_t c0 = pc.first, c1 = pc.last, bytes = pc.bytes;
        // this piece's windows grouped by (route, kernel shape): unit-record launches (route 0) first
        const int m = (int)(c1 - c0);
        std::vector<GroupItem> items((size_t)m);
        for (int k = 0; k < m; ++k) {
            const W& w = ws[c0 + (size_t)k];
            items[(size_t)k] = {w.rec ? 0 : 1, w.shape, flank_model(c, d, r0 + w.i)->h.n_cells};
        }
        const Grouping G = group_items(items);
        Carve lay;
        const size_t o_vt = lay.add<VitTask>((size_t)m), o_vr = lay.add<VitResult>((size_t)m), o_paths = lay.add<int32_t*>((size_t)m),
                     o_ut = lay.add<UnitTask>((size_t)m), o_bad = lay.add<int32_t>((size_t)m);
        STRQ_HIP(c, d->unit_task.reserve(lay.total() + 256));
        void* tb = d->unit_task.p;
        VitTask* d_vt = Carve::at<VitTask>(tb, o_vt); VitResult* d_vr = Carve::at<VitResult>(tb, o_vr); int32_t** d_paths = Carve::at<int32_t*>(tb, o_paths);
        UnitTask* d_ut = Carve::at<UnitTask>(tb, o_ut); int32_t* d_bad = Carve::at<int32_t>(tb, o_bad);
        size_t path_n = 0, pos_n = 0;
        for (size_t k = c0; k < c1; ++k) {
            if (!ws[k].rec) path_n += (size_t)vt[(size_t)sl.vit_slot[ws[k].i]].T;
            pos_n += (size_t)vres[sl.vit_slot[ws[k].i]].counted;
        }
        STRQ_HIP(c, d->unit_ws.reserve(bytes + (size_t)m * 16 + 64));
        if (path_n) STRQ_HIP(c, d->unit_path.reserve(path_n * 4 + 64));
        STRQ_HIP(c, d->unit_pool.reserve(pos_n * 8 + 64));
        std::vector<VitTask> tv((size_t)m); std::vector<int32_t*> pv((size_t)m, nullptr); std::vector<UnitTask> uv((size_t)m);
        std::vector<int> read_of((size_t)m); std::vector<size_t> pos_off((size_t)m);
        size_t wo = 0, po = 0, xo = 0; int n_rec = 0;
        for (int at = 0; at < m; ++at) {          // in task order: the workspace, the paths and the positions lie in that order too
            const W& w = ws[c0 + (size_t)G.order[(size_t)at]];
            HostModel* hm = flank_model(c, d, r0 + w.i);
            const VitResult& v0 = vres[sl.vit_slot[w.i]];
            VitTask t = vt[(size_t)sl.vit_slot[w.i]];
            t.bp = reinterpret_cast<uint16_t*>(d->unit_ws.as<char>() + wo); wo += (sizes[c0 + (size_t)G.order[(size_t)at]] + 15) & ~(size_t)15;
            if (wo > d->unit_ws.cap) { c->err = "unit pass: workspace"; return STRQ_ERR_NOMEM; }
            UnitTask u; std::memset(&u, 0, sizeof(u));
            u.rec = w.rec ? reinterpret_cast<const uint32_t*>(t.bp) : nullptr;
            if (!w.rec) { pv[(size_t)at] = d->unit_path.as<int32_t>() + po; u.path = pv[(size_t)at]; u.count_inc = hm->h.count_inc; po += (size_t)t.T; }
            u.result = d_vr + at; u.out = d->unit_pool.as<int64_t>() + xo; u.T = t.T; u.base = geom[w.i].prefix_begin; u.n = v0.counted; u.bad = d_bad + at;
            pos_off[(size_t)at] = xo; xo += (size_t)v0.counted;
            tv[(size_t)at] = t; uv[(size_t)at] = u; read_of[(size_t)at] = w.i;
            n_rec += w.rec ? 1 : 0;
        }
        STRQ_HIP(c, hipMemcpyAsync(d_vt, tv.data(), (size_t)m * sizeof(VitTask), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_paths, pv.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_ut, uv.data(), (size_t)m * sizeof(UnitTask), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemsetAsync(d_bad, 0, (size_t)m * 4, st));
        if (path_n) STRQ_HIP(c, hipMemsetAsync(d->unit_path.p, 0, path_n * 4, st));      // a traceback that stops early leaves valid states behind
        const GroupHook trace = [&](const VitGroup& g) -> int {          // by route: unit records, or back-pointers and a traceback
            if (g.route == 1 && launch_vit_traceback(st, d_vt + g.first, d_vr + g.first, d_paths + g.first, g.count)) { c->err = "traceback launch failed"; return STRQ_ERR_DEVICE; }
            return STRQ_OK;
        };
        if (const int grc = launch_groups(c, st, G.groups, {d_vt, d_vr, sl.order.as<int>(), {VIT_UNIT, VIT_BACKPTR}, "unit pass: ", false, nullptr, nullptr, trace})) return grc;
        if (launch_unit_hop(st, d_ut, n_rec) || launch_unit_scan(st, d_ut + n_rec, m - n_rec)) { c->err = "unit position launch failed"; return STRQ_ERR_DEVICE; }
        std::vector<int64_t> pos(xo + 1); std::vector<int32_t> bad((size_t)m);
        if (xo) STRQ_HIP(c, hipMemcpyAsync(pos.data(), d->unit_pool.p, xo * 8, hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipMemcpyAsync(bad.data(), d_bad, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipStreamSynchronize(st));
        for (int k = 0; k < m; ++k) {
            if (bad[(size_t)k]) { c->err = "unit pass: the unit decode of a window disagrees with its count decode"; return STRQ_ERR_DEVICE; }
            const int i = read_of[(size_t)k];
            const int64_t n = vres[sl.vit_slot[i]].counted;
            B.units[(size_t)(r0 + i)].assign(pos.begin() + (ptrdiff_t)pos_off[(size_t)k], pos.begin() + (ptrdiff_t)(pos_off[(size_t)k] + (size_t)n));
            B.unit_dec[(size_t)(r0 + i)] = 1;
        }
        d->stat(PASS_UNITS, UNIT_BYTES) = std::max(d->stat(PASS_UNITS, UNIT_BYTES), (double)bytes); d->stat(PASS_UNITS, UNIT_READS) += m; d->stat(PASS_UNITS, UNIT_POSITIONS) += (double)xo;
    }
    return pass_stop(c, pass_ev(d), d->stats[PASS_UNITS]);
}

// Count confidence of the reads of one sub-batch (strq_set_confidence): the forward pass (forward_kernels.hip) over the windows the
// count / MARK launch decoded, with the same tasks -- same windows, same affine source on the slot's filtered signal -- and c0 = the
// visits of the best path from the rows just taken.  Runs on the context's stream like the unit pass; one launch per kernel shape.
static int run_conf_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl, const Decoded& dec)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0;
    const VitResult* vres = sl.host().vres;
    const std::vector<int>& who = dec.who; const std::vector<VitTask>& vt = dec.vt;
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    const int m = (int)who.size();
    DecodeOrder<FwdModel> D; int frc = STRQ_OK;
    decode_order(who, [&](int i, GroupItem& it, const FwdModel*& fm) {
        HostModel* hm = flank_model(c, d, r0 + i);
        if ((frc = forward_model(c, hm))) return false;
        it = {0, vit_shape_of(hm->h), hm->h.n_cells}; fm = hm->fwd_dev;
        return true;
    }, D);
    if (frc) return frc;
    const std::vector<int32_t>& read_of = D.read_of; const std::vector<const FwdModel*>& fv = D.model;
    Carve lay;
    const size_t o_vt = lay.add<VitTask>((size_t)m), o_fr = lay.add<FwdResult>((size_t)m), o_fm = lay.add<const FwdModel*>((size_t)m),
                 o_c0 = lay.add<int64_t>((size_t)m), o_order = lay.add<int>((size_t)m);
    STRQ_HIP(c, d->conf_task.reserve(lay.total() + 256));
    void* tb = d->conf_task.p;
    VitTask* d_vt = Carve::at<VitTask>(tb, o_vt); FwdResult* d_fr = Carve::at<FwdResult>(tb, o_fr); const FwdModel** d_fm = Carve::at<const FwdModel*>(tb, o_fm);
    int64_t* d_c0 = Carve::at<int64_t>(tb, o_c0); int* d_order = Carve::at<int>(tb, o_order);
    std::vector<VitTask> tv((size_t)m); std::vector<int64_t> cv((size_t)m);
    for (int at = 0; at < m; ++at) {
        const int i = read_of[(size_t)at];
        tv[(size_t)at] = vt[(size_t)sl.vit_slot[i]]; tv[(size_t)at].bp = nullptr;
        cv[(size_t)at] = vres[sl.vit_slot[i]].counted;
    }
    STRQ_HIP(c, hipMemcpyAsync(d_vt, tv.data(), (size_t)m * sizeof(VitTask), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_fm, fv.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_c0, cv.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
    int every = 1;
    if (const char* e = strq::opt("STRQ_FWD_RESCALE_EVERY")) { const int v = atoi(e); if (v >= 1) every = v; }
    GroupDecode gd = {};
    gd.launch = [&](const VitGroup& l, int* queue) -> int {
        if (launch_vit_sort(st, d_vt + l.first, l.count, d_order + l.first)) { c->err = "forward pass: sort launch failed"; return STRQ_ERR_DEVICE; }
        const int lrc = launch_forward(st, l.shape, l.max_cells, d_vt + l.first, d_fm + l.first, d_c0 + l.first, d_fr + l.first, l.count,
                                       queue, c->n_cu, d_order + l.first, every);
        if (lrc) { c->err = lrc == 2 ? "forward pass: no kernel for this model's layout" : "forward launch failed"; return lrc == 2 ? STRQ_ERR_UNSUPPORTED : STRQ_ERR_DEVICE; }
        return STRQ_OK;
    };
    if (const int grc = launch_groups(c, st, D.G.groups, gd)) return grc;
    std::vector<FwdResult> fr((size_t)m);
    STRQ_HIP(c, hipMemcpyAsync(fr.data(), d_fr, (size_t)m * sizeof(FwdResult), hipMemcpyDeviceToHost, st));
    if (const int rc = pass_stop(c, pass_ev(d), d->stats[PASS_CONF])) return rc;
    for (int k = 0; k < m; ++k) {
        const int64_t r = r0 + read_of[(size_t)k];
        double ll, mean, var;
        const int nopath = fwd_finish(fr[(size_t)k], cv[(size_t)k], &ll, &mean, &var);
        B.conf[3 * (size_t)r] = ll;
        B.conf[3 * (size_t)r + 1] = nopath ? mean : (double)target_of(d, r).count_bias + mean;
        B.conf[3 * (size_t)r + 2] = nopath ? var : std::sqrt(var);
        B.conf_dec[(size_t)r] = 1;
        d->stat(PASS_CONF, CONF_NOPATH) += nopath; d->stat(PASS_CONF, CONF_EXPO) = std::max(d->stat(PASS_CONF, CONF_EXPO), std::fabs((double)fr[(size_t)k].expo));
    }
    d->stat(PASS_CONF, CONF_WINDOWS) += m;
    return STRQ_OK;
}

// The geometry and the conditioning rows of a sub-batch back on the device, from the slot's pinned block (the device copies belong to
// the sub-batch that followed): two regions at the front of `buf`, and `tail_bytes` of the caller's behind them.
struct SlotRows { ReadGeom* geom = nullptr; ReadCond* rc = nullptr; void* tail = nullptr; };
static int upload_slot_rows(strq_ctx* c, const DetectState::Slot& sl, DevBuf& buf, SlotRows& rows, size_t tail_bytes = 0)
{
    const DetectState::Slot::Pinned h = sl.host();
    const size_t nr = (size_t)sl.nr;
    Carve wl;
    const size_t o_geom = wl.add<ReadGeom>(nr), o_rc = wl.add<ReadCond>(nr), o_tail = wl.add<char>(tail_bytes);
    STRQ_HIP(c, buf.reserve(wl.total() + 64));
    rows.geom = Carve::at<ReadGeom>(buf.p, o_geom); rows.rc = Carve::at<ReadCond>(buf.p, o_rc); rows.tail = Carve::at<char>(buf.p, o_tail);
    STRQ_HIP(c, hipMemcpyAsync(rows.geom, h.geom, nr * sizeof(ReadGeom), hipMemcpyHostToDevice, c->stream));
    STRQ_HIP(c, hipMemcpyAsync(rows.rc, h.rc, nr * sizeof(ReadCond), hipMemcpyHostToDevice, c->stream));
    return STRQ_OK;
}

// The traced re-decode of windows (tract positions, state statistics): every window (`task`, `hm` of a Window) once more with
// back-pointers, traced back into a zeroed path buffer, then one kernel of the consumer over the paths.  The windows whose back-pointers
// alone exceed the budget get status 2, the others go in pieces (detect_plan.h: OVERSIZE_LEFT_OUT); a piece's windows are grouped by
// kernel shape, and its back-pointers, paths and the consumer's output lie in task order.  One set of uploads, one launch per shape
// (two where it sorts), one traceback per shape, the consumer's kernel, one read-back and one wait per piece.  A consumer K has: name
// and budget_option (the prefix of its messages, the option of its budget); bufs (the pass's buffers in the detect state); Task (its
// kernel's task, zeroed for fill); refuses(hm): why it cannot take this model, or null; size_pool: a piece begins with these m windows,
// the bytes of its output pool; fill: the task of window x at task position `at`, dev its path, result and bad flag on the device;
// launch: its kernel over the piece, what failed or null; read_back: queues its copies to the host (the driver adds the bad flags and
// waits); scatter: the output of window i at task position `at`, false where the decode disagrees with the count decode.
// stats (or null): windows traced, kernels launched, peak back-pointer bytes of a piece.
struct TraceBufs { DevBuf &task, &bp, &path, &pool; };
struct TraceSlot { int32_t* path; VitResult* result; int32_t* bad; };
template <class Window, class K>
static int traced_redecode(strq_ctx* c, const std::vector<Window>& w, K& k, std::vector<int32_t>& status, double* stats)
{
    hipStream_t st = c->stream;
    const std::string name = k.name;
    status.assign(w.size(), 0);
    std::vector<int> shape(w.size()); std::vector<size_t> sizes(w.size());
    for (size_t i = 0; i < w.size(); ++i) {
        const VitModel& h = w[i].hm->h; shape[i] = vit_shape_for(h, VIT_BACKPTR);
        const char* why = (shape[i] < 0 || !vit_mode_ok(shape[i], VIT_BACKPTR)) ? "the model has no back-pointer decode" : k.refuses(*w[i].hm);
        if (why) { c->err = name + why; return STRQ_ERR_UNSUPPORTED; }
        sizes[i] = bp_window_bytes(w[i].task.T, h.n_states);
    }
    const PiecePlan plan = plan_pieces(sizes, ws_budget(strq::opt(k.budget_option)), OVERSIZE_LEFT_OUT);
    for (int32_t i : plan.oversize) status[(size_t)i] = 2;
    for (const Piece& pc : plan.pieces) {
        const int m = (int)(pc.last - pc.first); const int32_t* wins = plan.order.data() + pc.first;
        std::vector<GroupItem> items((size_t)m); size_t path_n = 0;
        for (int j = 0; j < m; ++j) { const Window& x = w[(size_t)wins[j]]; items[(size_t)j] = {0, shape[(size_t)wins[j]], x.hm->h.n_cells}; path_n += (size_t)x.task.T; }
        const Grouping G = group_items(items);
        Carve lay;
        const size_t o_vt = lay.add<VitTask>((size_t)m), o_vr = lay.add<VitResult>((size_t)m), o_paths = lay.add<int32_t*>((size_t)m),
                     o_ts = lay.add<typename K::Task>((size_t)m), o_bad = lay.add<int32_t>((size_t)m), o_order = lay.add<int>((size_t)m);
        STRQ_HIP(c, k.bufs.task.reserve(lay.total() + 64));
        void* tb = k.bufs.task.p;
        VitTask* d_vt = Carve::at<VitTask>(tb, o_vt); VitResult* d_vr = Carve::at<VitResult>(tb, o_vr); int32_t** d_paths = Carve::at<int32_t*>(tb, o_paths);
        typename K::Task* d_ts = Carve::at<typename K::Task>(tb, o_ts); int32_t* d_bad = Carve::at<int32_t>(tb, o_bad); int* d_order = Carve::at<int>(tb, o_order);
        STRQ_HIP(c, k.bufs.bp.reserve(pc.bytes)); STRQ_HIP(c, k.bufs.path.reserve(path_n * 4 + 64));
        STRQ_HIP(c, k.bufs.pool.reserve(k.size_pool(w, wins, m)));
        std::vector<VitTask> tv((size_t)m); std::vector<int32_t*> pv((size_t)m); std::vector<typename K::Task> sv((size_t)m);
        size_t wo = 0, po = 0;
        for (int at = 0; at < m; ++at) {          // in task order
            const int32_t i = wins[G.order[(size_t)at]]; const Window& x = w[(size_t)i]; VitTask t = x.task;
            t.bp = reinterpret_cast<uint16_t*>(k.bufs.bp.template as<char>() + wo); wo += sizes[(size_t)i];
            if (wo > k.bufs.bp.cap) { c->err = name + "workspace"; return STRQ_ERR_NOMEM; }
            pv[(size_t)at] = k.bufs.path.template as<int32_t>() + po; po += (size_t)t.T;
            std::memset(&sv[(size_t)at], 0, sizeof(typename K::Task));
            k.fill(at, x, TraceSlot{pv[(size_t)at], d_vr + at, d_bad + at}, sv[(size_t)at]);
            tv[(size_t)at] = t;
        }
        STRQ_HIP(c, hipMemcpyAsync(d_vt, tv.data(), (size_t)m * sizeof(VitTask), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_paths, pv.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_ts, sv.data(), (size_t)m * sizeof(typename K::Task), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemsetAsync(d_bad, 0, (size_t)m * 4, st));
        if (path_n) STRQ_HIP(c, hipMemsetAsync(k.bufs.path.p, 0, path_n * 4, st));      // a traceback that stops early leaves valid states behind
        double launches = 0;
        const GroupHook trace = [&](const VitGroup& g) -> int {
            if (launch_vit_traceback(st, d_vt + g.first, d_vr + g.first, d_paths + g.first, g.count)) { c->err = name + "traceback launch failed"; return STRQ_ERR_DEVICE; }
            launches += 1; return STRQ_OK;
        };
        if (const int grc = launch_groups(c, st, G.groups, {d_vt, d_vr, d_order, {VIT_BACKPTR}, k.name, false, &launches, nullptr, trace})) return grc;
        if (const char* why = k.launch(st, d_vt, d_ts, m)) { c->err = name + why; return STRQ_ERR_DEVICE; }
        launches += 1; std::vector<int32_t> bad((size_t)m);
        if (const int rc = k.read_back(c, st, d_vr, m)) return rc;
        STRQ_HIP(c, hipMemcpyAsync(bad.data(), d_bad, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipStreamSynchronize(st));
        for (int at = 0; at < m; ++at) {
            const size_t i = (size_t)wins[G.order[(size_t)at]];
            if (bad[(size_t)at] || !k.scatter(at, i, w[i], sv[(size_t)at])) { c->err = name + "the back-pointer decode of a window disagrees with its count decode"; return STRQ_ERR_DEVICE; }
        }
        if (stats) { stats[0] += m; stats[1] += launches; stats[2] = std::max(stats[2], (double)pc.bytes); }
    }
    return STRQ_OK;
}

// Unit positions of the tracts of decoded windows (strq_ctx.h states the interface; strique_amd/tracts.py the rule): the traced paths
// scanned with one ballot per tract (tract_scan_kernel).  The buffers are the detect state's own and exist only once this ran.
struct TractPosConsumer {
    using Task = TractScanTask;
    TraceBufs bufs; TractPosOut& out;
    const char *name = "tract positions: ", *budget_option = "STRQ_TRACT_POS_WS_BYTES";
    std::vector<size_t> pos_off; size_t xo = 0;          // of the piece: where a task's positions begin in the pool, and its fill
    std::vector<int64_t> pos;
    const char* refuses(const HostModel& hm) const { return hm.h.tract_inc ? nullptr : "the model has no back-pointer decode"; }
    size_t size_pool(const std::vector<TractPosWindow>& w, const int32_t* wins, int m)
    {
        size_t pos_n = 0; pos_off.assign((size_t)m, 0); xo = 0;
        for (int k = 0; k < m; ++k) { const TractPosWindow& x = w[(size_t)wins[k]]; for (int j = 0; j < x.hm->n_tracts; ++j) pos_n += (size_t)x.n[j]; }
        return pos_n * 8 + 64;
    }
    void fill(int at, const TractPosWindow& x, const TraceSlot& dev, TractScanTask& s)
    {
        s.path = dev.path; s.tract_inc = x.hm->h.tract_inc; s.result = dev.result; s.out = bufs.pool.as<int64_t>() + xo;
        s.T = x.task.T; s.base = x.base; s.n_tracts = x.hm->n_tracts; s.n_states = x.hm->h.n_states; s.bad = dev.bad;
        pos_off[(size_t)at] = xo;
        for (int j = 0; j < x.hm->n_tracts; ++j) { s.off[j] = (int64_t)(xo - pos_off[(size_t)at]); s.n[j] = x.n[j]; xo += (size_t)x.n[j]; }
    }
    const char* launch(hipStream_t st, const VitTask*, const TractScanTask* d_ts, int m) { return launch_tract_scan(st, d_ts, m) ? "scan launch failed" : nullptr; }
    int read_back(strq_ctx* c, hipStream_t st, const VitResult*, int)
    {
        pos.resize(xo + 1); if (xo) STRQ_HIP(c, hipMemcpyAsync(pos.data(), bufs.pool.p, xo * 8, hipMemcpyDeviceToHost, st));
        return STRQ_OK;
    }
    bool scatter(int at, size_t i, const TractPosWindow&, const TractScanTask& s)
    {
        for (int j = 0; j < s.n_tracts; ++j) { const int64_t* from = pos.data() + pos_off[(size_t)at] + s.off[j]; out.pos[3 * i + (size_t)j].assign(from, from + s.n[j]); }
        return true;
    }
};
int tract_positions(strq_ctx* c, const std::vector<TractPosWindow>& w, TractPosOut& out, double* stats)
{
    DetectState* d = dstate(c); out.pos.assign(3 * w.size(), std::vector<int64_t>());
    TractPosConsumer k{{d->tpos_task, d->tpos_bp, d->tpos_path, d->tpos_pool}, out};
    return traced_redecode(c, w, k, out.status, stats);
}

// State statistics of decoded windows (strq_ctx.h states the interface; strique_amd/state_stats.py the rule): the observations of the
// traced paths summed per emitting state (state_stats_kernel), n | sum | sumsq rows of the piece's windows in one pool.  A decode whose
// status, log-probability or count is not what the count decode found disagrees with it.  The buffers exist only once this ran.
struct StateStatsConsumer {
    using Task = StateStatsTask;
    TraceBufs bufs; StateStatsOut& out;
    const char *name = "state-stats: ", *budget_option = "STRQ_STATE_STATS_WS_BYTES";
    size_t row_n = 0, xo = 0; int max_emit = 1; std::vector<size_t> row_off;          // of the piece: rows in all, rows handed out, a task's first row
    std::vector<int64_t> rows; std::vector<VitResult> vr;
    const char* refuses(const HostModel& hm) const { return (hm.silent_start < 1 || hm.silent_start > STATE_STATS_MAX_EMIT) ? "the model's emitting states do not fit the kernel" : nullptr; }
    size_t size_pool(const std::vector<StateStatsWindow>& w, const int32_t* wins, int m)
    {
        row_n = 0; xo = 0; max_emit = 1; row_off.assign((size_t)m, 0);
        for (int k = 0; k < m; ++k) { const int ne = (int)w[(size_t)wins[k]].hm->silent_start; row_n += (size_t)ne; max_emit = std::max(max_emit, ne); }
        return row_n * 24 + 64;
    }
    void fill(int at, const StateStatsWindow& x, const TraceSlot& dev, StateStatsTask& s)
    {
        int64_t* o_n = bufs.pool.as<int64_t>(); double* o_sum = reinterpret_cast<double*>(o_n + row_n); double* o_sq = o_sum + row_n;
        s.path = dev.path; s.result = dev.result; s.n = o_n + xo; s.sum = o_sum + xo; s.sumsq = o_sq + xo; s.n_emit = x.hm->silent_start; s.bad = dev.bad;
        row_off[(size_t)at] = xo; xo += (size_t)x.hm->silent_start;
    }
    const char* launch(hipStream_t st, const VitTask* d_vt, const StateStatsTask* d_ts, int m) { return launch_state_stats(st, d_vt, d_ts, m, max_emit) ? "kernel launch failed" : nullptr; }
    int read_back(strq_ctx* c, hipStream_t st, const VitResult* d_vr, int m)
    {
        rows.resize(3 * row_n + 1); vr.resize((size_t)m);
        STRQ_HIP(c, hipMemcpyAsync(rows.data(), bufs.pool.p, row_n * 24, hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipMemcpyAsync(vr.data(), d_vr, (size_t)m * sizeof(VitResult), hipMemcpyDeviceToHost, st));
        return STRQ_OK;
    }
    bool scatter(int at, size_t i, const StateStatsWindow& x, const StateStatsTask&)
    {
        const VitResult& v = vr[(size_t)at]; if (v.status != 0 || std::memcmp(&v.logp, &x.logp, 8) != 0 || v.counted != x.counted) return false;
        const int64_t* h_n = rows.data(); const double* h_sum = reinterpret_cast<const double*>(h_n + row_n); const double* h_sq = h_sum + row_n;
        const size_t o = row_off[(size_t)at], ne = (size_t)x.hm->silent_start;
        out.n[i].assign(h_n + o, h_n + o + ne); out.sum[i].assign(h_sum + o, h_sum + o + ne); out.sumsq[i].assign(h_sq + o, h_sq + o + ne);
        return true;
    }
};
int state_stats(strq_ctx* c, const std::vector<StateStatsWindow>& w, StateStatsOut& out, double* stats)
{
    DetectState* d = dstate(c); out.n.assign(w.size(), std::vector<int64_t>()); out.sum.assign(w.size(), std::vector<double>()); out.sumsq.assign(w.size(), std::vector<double>());
    StateStatsConsumer k{{d->sst_task, d->sst_bp, d->sst_path, d->sst_out}, out};
    return traced_redecode(c, w, k, out.status, stats);
}

// State posteriors of windows (strq_ctx.h states the interface; strique_amd/state_posteriors.py the rule).  No back-pointers and no
// traceback, so it plans its pieces like the traced re-decode but runs them itself: the windows of a piece grouped by kernel shape, one forward and one backward launch per shape on two queue heads (posterior_kernels.h),
// the stored forward vectors of the piece in one buffer.  A window whose vectors alone exceed the budget rides along in the first piece
// with nothing stored: its forward half still gives the likelihood.  One read-back and one wait per piece; the buffers exist only once
// this ran.
int state_posteriors(strq_ctx* c, const std::vector<StatePostWindow>& w, StatePostOut& out, double* stats)
{
    DetectState* d = dstate(c);
    hipStream_t st = c->stream;
    const size_t nw = w.size();
    out.status.assign(nw, 0); out.fwd.assign(nw, FwdResult()); out.w.assign(nw, std::vector<double>()); out.wx.assign(nw, std::vector<double>()); out.wxx.assign(nw, std::vector<double>());
    std::vector<int> shape(nw); std::vector<size_t> sizes(nw);
    for (size_t i = 0; i < nw; ++i) {
        if (const int rc = posterior_model(c, w[i].hm)) return rc;
        const VitModel& h = w[i].hm->h;
        shape[i] = vit_shape_of(h);
        if (vit_shape_family(shape[i]) != VIT_FAMILY_LANE) { c->err = "state posteriors: the model has no forward kernel"; return STRQ_ERR_UNSUPPORTED; }
        sizes[i] = post_window_bytes(w[i].task.T, h.epl);
    }
    // at most 8192 windows a piece; a window over the budget rides in front with nothing stored (detect_plan.h: OVERSIZE_IN_FRONT)
    const PiecePlan plan = plan_pieces(sizes, ws_budget(strq::opt("STRQ_STATE_POST_WS_BYTES")), OVERSIZE_IN_FRONT, 8192);
    for (int32_t i : plan.oversize) out.status[(size_t)i] = 2;
    for (const Piece& pc : plan.pieces) {
        const size_t c0 = pc.first, bytes = pc.bytes;
        const int m = (int)(pc.last - pc.first);
        std::vector<GroupItem> items((size_t)m);
        size_t row_n = 0;
        for (int k = 0; k < m; ++k) {
            const StatePostWindow& x = w[(size_t)plan.order[c0 + (size_t)k]];
            items[(size_t)k] = {0, shape[(size_t)plan.order[c0 + (size_t)k]], x.hm->h.n_cells};
            row_n += (size_t)x.hm->silent_start;
        }
        const Grouping G = group_items(items);
        if (2 * G.groups.size() > 256) { c->err = "state posteriors: too many kernel shapes in one piece"; return STRQ_ERR_UNSUPPORTED; }
        Carve lay;
        const size_t o_vt = lay.add<VitTask>((size_t)m), o_fr = lay.add<FwdResult>((size_t)m), o_pm = lay.add<const PostModel*>((size_t)m),
                     o_pt = lay.add<PostTask>((size_t)m), o_order = lay.add<int>((size_t)m);
        STRQ_HIP(c, d->post_task.reserve(lay.total() + 64));
        void* tb = d->post_task.p;
        VitTask* d_vt = Carve::at<VitTask>(tb, o_vt); FwdResult* d_fr = Carve::at<FwdResult>(tb, o_fr); const PostModel** d_pm = Carve::at<const PostModel*>(tb, o_pm);
        PostTask* d_pt = Carve::at<PostTask>(tb, o_pt); int* d_order = Carve::at<int>(tb, o_order);
        STRQ_HIP(c, d->post_ws.reserve(bytes + 64));
        STRQ_HIP(c, d->post_out.reserve(row_n * 24 + 64));          // w | wx | wxx, row_n entries each
        double* o_w = d->post_out.as<double>(); double* o_wx = o_w + row_n; double* o_wxx = o_wx + row_n;
        std::vector<VitTask> tv((size_t)m); std::vector<const PostModel*> mv((size_t)m); std::vector<PostTask> pv((size_t)m);
        std::vector<int> win_of((size_t)m); std::vector<size_t> row_off((size_t)m);
        size_t wo = 0, xo = 0;
        for (int at = 0; at < m; ++at) {          // in task order: the stored vectors and the rows lie in that order too
            const size_t at_plan = c0 + (size_t)G.order[(size_t)at];
            const StatePostWindow& x = w[(size_t)plan.order[at_plan]];
            PostTask p; std::memset(&p, 0, sizeof(p));
            if (plan.bytes[at_plan]) {
                p.alpha = reinterpret_cast<double*>(d->post_ws.as<char>() + wo);
                p.expo = reinterpret_cast<int32_t*>(d->post_ws.as<char>() + wo + post_alpha_bytes(x.task.T, x.hm->h.epl));
                wo += plan.bytes[at_plan];
                if (wo > d->post_ws.cap) { c->err = "state posteriors: workspace"; return STRQ_ERR_NOMEM; }
            }
            p.w = o_w + xo; p.wx = o_wx + xo; p.wxx = o_wxx + xo;
            row_off[(size_t)at] = xo; xo += (size_t)x.hm->silent_start;
            tv[(size_t)at] = x.task; tv[(size_t)at].bp = nullptr; mv[(size_t)at] = x.hm->post_dev; pv[(size_t)at] = p; win_of[(size_t)at] = plan.order[at_plan];
        }
        STRQ_HIP(c, hipMemcpyAsync(d_vt, tv.data(), (size_t)m * sizeof(VitTask), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_pm, mv.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_pt, pv.data(), (size_t)m * sizeof(PostTask), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemsetAsync(d->post_out.p, 0, row_n * 24, st));          // a window without a path keeps +0.0 rows
        if (const int qrc = reset_queue_heads(c, st)) return qrc;
        double launches = 0; int qi = 0;
        for (const VitGroup& g : G.groups) {
            if (launch_vit_sort(st, d_vt + g.first, g.count, d_order + g.first)) { c->err = "state posteriors: sort launch failed"; return STRQ_ERR_DEVICE; }
            const int lrc = launch_posterior(st, g.shape, g.max_cells, d_vt + g.first, d_pm + g.first, d_pt + g.first, d_fr + g.first, g.count,
                                             c->queue.as<int>() + qi, c->n_cu, d_order + g.first);
            if (lrc) { c->err = lrc == 2 ? "state posteriors: no kernel for this model's layout" : "state posteriors: kernel launch failed"; return lrc == 2 ? STRQ_ERR_UNSUPPORTED : STRQ_ERR_DEVICE; }
            qi += 2; launches += 3;
        }
        std::vector<double> rows(3 * row_n + 1); std::vector<FwdResult> fr((size_t)m);
        STRQ_HIP(c, hipMemcpyAsync(rows.data(), d->post_out.p, row_n * 24, hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipMemcpyAsync(fr.data(), d_fr, (size_t)m * sizeof(FwdResult), hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipStreamSynchronize(st));
        const double* h_w = rows.data(); const double* h_wx = h_w + row_n; const double* h_wxx = h_wx + row_n;
        for (int at = 0; at < m; ++at) {
            const size_t i = (size_t)win_of[(size_t)at], o = row_off[(size_t)at], ne = (size_t)w[i].hm->silent_start;
            out.fwd[i] = fr[(size_t)at];
            if (out.status[i] == 2) continue;
            if (!(fr[(size_t)at].p > 0.0)) { out.status[i] = 1; continue; }
            out.w[i].assign(h_w + o, h_w + o + ne); out.wx[i].assign(h_wx + o, h_wx + o + ne); out.wxx[i].assign(h_wxx + o, h_wxx + o + ne);
        }
        if (stats) { stats[0] += m; stats[1] += launches; stats[2] = std::max(stats[2], (double)bytes); }
    }
    return STRQ_OK;
}

// State posteriors of the reads of one sub-batch (strq_set_state_posteriors): the windows the count / MARK launch decoded, once more
// with the same tasks -- same windows, same affine source on the slot's filtered signal -- like the forward pass of strq_set_confidence.
// Runs on the context's stream when the rows of the sub-batch are taken.
static int run_state_posteriors_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl, const Decoded& dec)
{
    Batch& B = d->batch;
    const int64_t r0 = sl.r0;
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    std::vector<StatePostWindow> pw;
    for (int i : dec.who) {
        StatePostWindow x; x.task = dec.vt[(size_t)sl.vit_slot[i]]; x.task.bp = nullptr; x.hm = flank_model(c, d, r0 + i);
        pw.push_back(x);
    }
    StatePostOut po;
    if (const int rc = state_posteriors(c, pw, po, d->stats[PASS_SPOST].v)) return rc;
    for (size_t k = 0; k < pw.size(); ++k) {
        const size_t r = (size_t)(r0 + dec.who[k]);
        double mean, var;
        (void)fwd_finish(po.fwd[k], 0, &B.spost[r].log_lik, &mean, &var);
        B.spost_status[r] = po.status[k];
        B.spost[r].w.swap(po.w[k]); B.spost[r].wx.swap(po.wx[k]); B.spost[r].wxx.swap(po.wxx[k]);
    }
    return pass_stop(c, pass_ev(d), d->stats[PASS_SPOST]);
}

// State statistics of the reads of one sub-batch (strq_set_state_stats): the windows the count / MARK launch decoded, once more with the
// same tasks -- same windows, same affine source on the slot's filtered signal -- like the back-pointer route of the unit pass.  Runs on
// the context's stream when the rows of the sub-batch are taken.
static int run_state_stats_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl, const Decoded& dec)
{
    Batch& B = d->batch;
    const int64_t r0 = sl.r0;
    const VitResult* vres = sl.host().vres;
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    std::vector<StateStatsWindow> sw;
    for (int i : dec.who) {
        const VitResult& v0 = vres[sl.vit_slot[i]];
        StateStatsWindow x; x.task = dec.vt[(size_t)sl.vit_slot[i]]; x.task.bp = nullptr; x.hm = flank_model(c, d, r0 + i); x.logp = v0.logp; x.counted = v0.counted;
        sw.push_back(x);
    }
    StateStatsOut so;
    if (const int rc = state_stats(c, sw, so, d->stats[PASS_SSTATS].v)) return rc;
    for (size_t k = 0; k < sw.size(); ++k) {
        const size_t r = (size_t)(r0 + dec.who[k]);
        B.sst_status[r] = so.status[k];
        B.sst[r].n.swap(so.n[k]); B.sst[r].sum.swap(so.sum[k]); B.sst[r].sumsq.swap(so.sumsq[k]);
    }
    return pass_stop(c, pass_ev(d), d->stats[PASS_SSTATS]);
}

// Tract counts of the reads of one sub-batch (strq_set_tracts): every read whose gate passed, that was normalised, whose flanked decode
// found a path and whose target has a compound model is decoded once more with that model, on the window of the count decode.  Runs
// on the context's stream when the rows of the sub-batch are taken, like the forward pass: the geometry and the conditioning rows go
// back up from the slot's pinned block (the device copies belong to the sub-batch that followed), the host groups the reads by
// kernel shape, tract_task_kernel writes their tasks on the slot's filtered signal, and the Viterbi kernels decode them as a count
// launch with the wide payload -- one launch per kernel instance in use; the first wait is the read-back of the results.
static int run_tract_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0; const int nr = sl.nr;
    if (nr <= 0 || sl.scan) return STRQ_OK;
    const DetectState::Slot::Pinned h = sl.host();
    std::vector<int> who;
    for (int i = 0; i < nr; ++i) {
        const Target& t = target_of(d, r0 + i);
        if (t.tract_model_id < 0 || !h.geom[i].gate || h.rc[i].status != COND_OK || h.vres[sl.vit_slot[i]].status != 0) continue;
        who.push_back(i);
    }
    const int m = (int)who.size();
    if (!m) return STRQ_OK;
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    DecodeOrder<VitModel> D;
    if (!decode_order(who, [&](int i, GroupItem& it, const VitModel*& vm) {
            HostModel* hm = c->models[target_of(d, r0 + i).tract_model_id];
            const int shape = vit_shape_of(hm->h);          // (never the register-resident image: it has one loop)
            if (shape < 0 || !hm->h.tract_inc) return false;
            it = {0, shape, hm->h.n_cells}; vm = hm->dev;
            return true;
        }, D)) { c->err = "tracts: the target's model has no tract decode"; return STRQ_ERR_UNSUPPORTED; }
    const std::vector<int32_t>& read_of = D.read_of;
    SlotRows rows;
    if (const int rc = upload_slot_rows(c, sl, d->tract_ws, rows)) return rc;
    Carve tl;
    const size_t o_vt = tl.add<VitTask>((size_t)m), o_vr = tl.add<VitResult>((size_t)m), o_md = tl.add<const VitModel*>((size_t)m), o_rd = tl.add<int32_t>((size_t)m),
                 o_order = tl.add<int>((size_t)m);
    STRQ_HIP(c, d->tract_task.reserve(tl.total() + 64));
    void* tb = d->tract_task.p;
    VitTask* d_vt = Carve::at<VitTask>(tb, o_vt); VitResult* d_vr = Carve::at<VitResult>(tb, o_vr);
    const VitModel** d_md = Carve::at<const VitModel*>(tb, o_md); int32_t* d_rd = Carve::at<int32_t>(tb, o_rd); int* d_order = Carve::at<int>(tb, o_order);
    STRQ_HIP(c, hipMemcpyAsync(d_rd, read_of.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_md, D.model.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
    TractTaskArgs ta;
    ta.geom = rows.geom; ta.rc = rows.rc; ta.read = d_rd; ta.model = d_md; ta.flt = sl.flt_base; ta.is_f64 = B.dtype; ta.ps = d->ps;
    ta.vit = d_vt; ta.n_tasks = m; ta.n_reads = nr;
    if (launch_tract_tasks(st, ta)) { c->err = "tracts: task launch failed"; return STRQ_ERR_DEVICE; }
    d->stat(PASS_TRACTS, TRACT_LAUNCHES) += 1;
    if (const int grc = launch_groups(c, st, D.G.groups, {d_vt, d_vr, d_order, {VIT_COUNT}, "tracts: ", true, &d->stat(PASS_TRACTS, TRACT_LAUNCHES)})) return grc;
    std::vector<VitResult> vr((size_t)m); std::vector<VitTask> tv(sl.ex.tpos ? (size_t)m : 0);
    STRQ_HIP(c, hipMemcpyAsync(vr.data(), d_vr, (size_t)m * sizeof(VitResult), hipMemcpyDeviceToHost, st));
    // (the positions start from the tasks as tract_task_kernel wrote them: they come back in the same wait)
    if (sl.ex.tpos) STRQ_HIP(c, hipMemcpyAsync(tv.data(), d_vt, (size_t)m * sizeof(VitTask), hipMemcpyDeviceToHost, st));
    if (const int rc = pass_stop(c, pass_ev(d), d->stats[PASS_TRACTS])) return rc;
    for (int at = 0; at < m; ++at) {
        const int i = read_of[(size_t)at];
        const Target& t = target_of(d, r0 + i);
        const VitResult& v = vr[(size_t)at];
        strq_tracts o = strq_tracts();
        o.status = v.status == 0 ? 0 : (v.status == 2 ? 2 : 3);
        if (o.status == 0) {
            o.n_tracts = t.n_tracts; o.log_p = v.logp;
            for (int j = 0; j < t.n_tracts; ++j)
                o.count[j] = (int32_t)vit_tract_count((uint64_t)v.counted, j) + t.tract_bias[j];
            d->stat(PASS_TRACTS, TRACT_WINDOWS) += 1;
        } else d->stat(PASS_TRACTS, TRACT_FAILED) += 1;
        B.tracts[(size_t)(r0 + i)] = o;
    }
    if (!sl.ex.tpos) return STRQ_OK;
    // Unit positions of the tracts (strq_set_tract_positions): the windows of status 0 once more, their counters sizing the pool
    std::vector<TractPosWindow> pw; std::vector<int> pw_read;
    for (int at = 0; at < m; ++at) {
        if (vr[(size_t)at].status != 0) continue;
        const int i = read_of[(size_t)at];
        TractPosWindow x; x.task = tv[(size_t)at]; x.hm = c->models[target_of(d, r0 + i).tract_model_id]; x.base = h.geom[i].prefix_begin;
        for (int j = 0; j < 3; ++j) x.n[j] = vit_tract_count((uint64_t)vr[(size_t)at].counted, j);
        pw.push_back(x); pw_read.push_back(i);
    }
    if (pw.empty()) return STRQ_OK;
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    TractPosOut po;
    if (const int rc = tract_positions(c, pw, po, d->stats[PASS_TPOS].v)) return rc;
    for (size_t k = 0; k < pw.size(); ++k) {
        const size_t r = (size_t)(r0 + pw_read[k]);
        B.tpos_status[r] = po.status[k];
        for (int j = 0; j < 3; ++j) B.tpos[3 * r + (size_t)j].swap(po.pos[3 * k + (size_t)j]);
    }
    return pass_stop(c, pass_ev(d), d->stats[PASS_TPOS]);
}

// The motif track of the reads of one sub-batch (strq_set_motifs; strique_amd/motifs.py states the rule): every read whose gate passed,
// that was conditioned, with prefix_end < suffix_begin and whose target has candidates.  The geometry and the conditioning constants are
// on the host (the slot's pinned block), so the stretches -- [prefix_end, suffix_begin) on the slot's filtered signal -- are written
// there; motif_track_kernel scores their segments, motif_reduce_kernel sums them up, one read-back.  Then the reads whose majority is
// not candidate 0 are decoded with the flanked model of the majority unit as the tract pass decodes its windows: tract_task_kernel
// on [prefix_begin, suffix_end), a count launch per kernel instance in use.  Runs on the context's stream when the rows are taken.
static int run_motif_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0; const int nr = sl.nr;
    if (nr <= 0 || sl.scan) return STRQ_OK;
    const DetectState::Slot::Pinned h = sl.host();
    const int S = sl.ex.motif_segment, run = motif_run_segments(S);
    std::vector<int> who; std::vector<MotifWindow> wv; std::vector<MotifTask> tv; std::vector<size_t> seg_at, v_at;
    size_t total_seg = 0, total_v = 0;
    for (int i = 0; i < nr; ++i) {
        const Target& t = target_of(d, r0 + i);
        const ReadGeom& g = h.geom[i]; const ReadCond& rc = h.rc[i];
        if (t.n_motifs < 2 || !g.gate || rc.status != COND_OK || !(g.prefix_end >= 0 && g.prefix_end < g.suffix_begin && g.suffix_begin <= (int64_t)rc.n)) continue;
        MotifWindow w; std::memset(&w, 0, sizeof(w));
        w.obs = window_task(1, g.prefix_end, g.suffix_begin, rc, nullptr, sl.flt_base, B.dtype, d->ps);
        w.n_cand = t.n_motifs; w.segment = S; w.n_seg = w.obs.T / S > 1 ? w.obs.T / S : 1;
        for (int j = 0; j < t.n_motifs; ++j) {
            const HostModel* lm = t.motif_loop[j] >= 0 && t.motif_loop[j] < (int)c->models.size() ? c->models[t.motif_loop[j]] : nullptr;
            if (!lm || !lm->motif_dev) { c->err = "motifs: loop model without an edge image (strq_target_set_motifs builds them)"; return STRQ_ERR_DEVICE; }
            w.model[j] = lm->motif_dev;
        }
        for (int64_t s = 0; s < w.n_seg; s += run) {
            MotifTask k; k.window = (int32_t)who.size(); k.seg_first = s; k.seg_count = (int32_t)(w.n_seg - s < run ? w.n_seg - s : run);
            tv.push_back(k);
        }
        who.push_back(i); wv.push_back(w); seg_at.push_back(total_seg); v_at.push_back(total_v);
        total_seg += (size_t)w.n_seg; total_v += (size_t)w.n_seg * (size_t)w.n_cand;
    }
    const int m = (int)who.size();
    if (!m) return STRQ_OK;
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    Carve lay;
    const size_t o_V = lay.add<double>(total_v), o_win = lay.add<int32_t>(total_seg), o_won = lay.add<int64_t>((size_t)m * MOTIF_MAX_CAND), o_maj = lay.add<int32_t>((size_t)m),
                 o_w = lay.add<MotifWindow>((size_t)m), o_t = lay.add<MotifTask>(tv.size());
    STRQ_HIP(c, d->motif_ws.reserve(lay.total() + 64));
    void* ws = d->motif_ws.p;
    double* d_V = Carve::at<double>(ws, o_V); int32_t* d_win = Carve::at<int32_t>(ws, o_win); int64_t* d_won = Carve::at<int64_t>(ws, o_won);
    int32_t* d_maj = Carve::at<int32_t>(ws, o_maj); MotifWindow* d_w = Carve::at<MotifWindow>(ws, o_w); MotifTask* d_t = Carve::at<MotifTask>(ws, o_t);
    for (int k = 0; k < m; ++k) {
        MotifWindow& w = wv[(size_t)k];
        w.V = d_V + v_at[(size_t)k]; w.winner = d_win + seg_at[(size_t)k]; w.obs_won = d_won + (size_t)k * MOTIF_MAX_CAND; w.majority = d_maj + k;
    }
    STRQ_HIP(c, hipMemcpyAsync(d_w, wv.data(), (size_t)m * sizeof(MotifWindow), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_t, tv.data(), tv.size() * sizeof(MotifTask), hipMemcpyHostToDevice, st));
    if (launch_motif_track(st, d_w, m, d_t, (int64_t)tv.size(), c->n_cu)) { c->err = "motifs: launch failed"; return STRQ_ERR_DEVICE; }
    d->stat(PASS_MOTIFS, MOTIF_LAUNCHES) += 2;
    std::vector<double> hV(total_v); std::vector<int32_t> hwin(total_seg), hmaj((size_t)m); std::vector<int64_t> hwon((size_t)m * MOTIF_MAX_CAND);
    STRQ_HIP(c, hipMemcpyAsync(hV.data(), d_V, total_v * 8, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(hwin.data(), d_win, total_seg * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(hwon.data(), d_won, (size_t)m * MOTIF_MAX_CAND * 8, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(hmaj.data(), d_maj, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    std::vector<int> other;          // reads whose array is not made of the configured unit
    for (int k = 0; k < m; ++k) {
        const int i = who[(size_t)k];
        const size_t r = (size_t)(r0 + i);
        const MotifWindow& w = wv[(size_t)k];
        strq_motifs o = strq_motifs();
        o.n_cand = w.n_cand; o.n_seg = w.n_seg; o.majority = hmaj[(size_t)k]; o.begin = h.geom[i].prefix_end; o.end = h.geom[i].suffix_begin;
        for (int j = 0; j < MOTIF_MAX_CAND; ++j) o.obs_won[j] = hwon[(size_t)k * MOTIF_MAX_CAND + (size_t)j];
        if (o.majority < 0 || o.majority >= w.n_cand) { c->err = "motifs: the reduction returned a majority beyond the candidates"; return STRQ_ERR_DEVICE; }
        o.decode_status = 1;
        if (o.majority == 0) {
            if (h.vres[sl.vit_slot[i]].status == 0) { o.decode_status = 0; o.count_m = B.results[r].count; o.log_p_m = B.results[r].log_p; }
        } else other.push_back(k);
        B.motifs[r] = o;
        B.motif_V[r].assign(hV.begin() + (ptrdiff_t)v_at[(size_t)k], hV.begin() + (ptrdiff_t)(v_at[(size_t)k] + (size_t)w.n_seg * (size_t)w.n_cand));
        B.motif_win[r].assign(hwin.begin() + (ptrdiff_t)seg_at[(size_t)k], hwin.begin() + (ptrdiff_t)(seg_at[(size_t)k] + (size_t)w.n_seg));
        d->stat(PASS_MOTIFS, MOTIF_READS) += 1; d->stat(PASS_MOTIFS, MOTIF_SEGMENTS) += (double)w.n_seg;
    }
    if (other.empty()) return pass_stop(c, pass_ev(d), d->stats[PASS_MOTIFS]);
    // the count decode under the majority unit
    std::vector<int> who2;
    for (int k : other) who2.push_back(who[(size_t)k]);
    const int m2 = (int)who2.size();
    DecodeOrder<VitModel> D;
    if (!decode_order(who2, [&](int i, GroupItem& it, const VitModel*& vm) {
            const Target& t = target_of(d, r0 + i);
            const int id = t.motif_flanked[B.motifs[(size_t)(r0 + i)].majority];
            HostModel* hm = id >= 0 && id < (int)c->models.size() ? c->models[id] : nullptr;
            const int shape = hm ? vit_shape_for(hm->h, VIT_COUNT) : -1;
            if (shape < 0) return false;
            it = {0, shape, hm->h.n_cells}; vm = hm->dev;
            return true;
        }, D)) { c->err = "motifs: a candidate's flanked model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
    SlotRows rows;
    if (const int rc = upload_slot_rows(c, sl, d->motif_rows, rows)) return rc;
    Carve tl;
    const size_t o_vt = tl.add<VitTask>((size_t)m2), o_vr = tl.add<VitResult>((size_t)m2), o_md = tl.add<const VitModel*>((size_t)m2), o_rd = tl.add<int32_t>((size_t)m2),
                 o_order = tl.add<int>((size_t)m2);
    STRQ_HIP(c, d->motif_task.reserve(tl.total() + 64));
    void* tb = d->motif_task.p;
    VitTask* d_vt = Carve::at<VitTask>(tb, o_vt); VitResult* d_vr = Carve::at<VitResult>(tb, o_vr);
    const VitModel** d_md = Carve::at<const VitModel*>(tb, o_md); int32_t* d_rd = Carve::at<int32_t>(tb, o_rd); int* d_order = Carve::at<int>(tb, o_order);
    STRQ_HIP(c, hipMemcpyAsync(d_rd, D.read_of.data(), (size_t)m2 * 4, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_md, D.model.data(), (size_t)m2 * 8, hipMemcpyHostToDevice, st));
    TractTaskArgs ta;
    ta.geom = rows.geom; ta.rc = rows.rc; ta.read = d_rd; ta.model = d_md; ta.flt = sl.flt_base; ta.is_f64 = B.dtype; ta.ps = d->ps;
    ta.vit = d_vt; ta.n_tasks = m2; ta.n_reads = nr;
    if (launch_tract_tasks(st, ta)) { c->err = "motifs: task launch failed"; return STRQ_ERR_DEVICE; }
    d->stat(PASS_MOTIFS, MOTIF_LAUNCHES) += 1;
    if (const int grc = launch_groups(c, st, D.G.groups, {d_vt, d_vr, d_order, {VIT_COUNT}, "motifs: ", false, &d->stat(PASS_MOTIFS, MOTIF_LAUNCHES)})) return grc;
    std::vector<VitResult> vr((size_t)m2);
    STRQ_HIP(c, hipMemcpyAsync(vr.data(), d_vr, (size_t)m2 * sizeof(VitResult), hipMemcpyDeviceToHost, st));
    if (const int rc = pass_stop(c, pass_ev(d), d->stats[PASS_MOTIFS])) return rc;
    for (int at = 0; at < m2; ++at) {
        const int i = D.read_of[(size_t)at];
        strq_motifs& o = B.motifs[(size_t)(r0 + i)];
        const VitResult& v = vr[(size_t)at];
        if (v.status == 0) { o.decode_status = 0; o.count_m = (int32_t)v.counted + target_of(d, r0 + i).motif_bias[o.majority]; o.log_p_m = v.logp; }
        d->stat(PASS_MOTIFS, MOTIF_DECODES) += 1;
    }
    return STRQ_OK;
}

// Methylation calls for the CpG groups of the flanks of one sub-batch (strq_set_flank_mod; strique_amd/flank_mod.py states the rule):
// every read whose gate passed, that could be conditioned and whose target has a modification model and the flank models.  Per flank
// with begin < end -- the prefix on the raw samples [whole prefix begin, prefix_end), the suffix on [suffix_begin, whole suffix end) --
// the stretch is normalised like the modification pass's (mod_compact_kernel without a path), decoded with the flank's profile model
// (back-pointers, traceback), flank_mod_bounds_kernel turns the path into the groups' bounds and their score tasks, and the passage
// scorer of the per-unit scores scores them, one launch per mode.  Runs behind the rows on the context's stream, in pieces (detect_plan.h)
// of back-pointers against STRQ_FLANK_MOD_WS_BYTES, an oversize stretch alone; one read-back and one wait per piece.  The geometry, the
// conditioning constants and so the lengths are on the host already (the slot's pinned block), so the tasks are written there.
static int run_flank_mod_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0; const int nr = sl.nr;
    if (nr <= 0 || sl.scan) return STRQ_OK;
    const DetectState::Slot::Pinned h = sl.host();
    const int esz = B.dtype == 0 ? 2 : 8;
    const int64_t s0 = B.off[r0];
    // test hook: the observations per flank base beyond which a stretch is not decoded (the rule's 64), so that the too_long branch can be reached
    int64_t max_per_base = 64;
    if (const char* e = strq::opt("STRQ_FLANK_MOD_MAX_STRETCH")) { const long long v = atoll(e); if (v > 0) max_per_base = (int64_t)v; }
    struct F { int i, which; int64_t begin, T; size_t first_rec; };
    std::vector<F> fl; std::vector<size_t> sizes;
    const double nan = std::nan("");
    for (int i = 0; i < nr; ++i) {
        const Target& t = target_of(d, r0 + i);
        const ReadGeom& g = h.geom[i]; const ReadCond& rc = h.rc[i];
        if (!t.has_fmod() || !g.gate || rc.status != COND_OK) continue;
        std::vector<strq_flank_mod_group>& recs = B.fmod[(size_t)(r0 + i)];
        B.fmod_called[(size_t)(r0 + i)] = 1; recs.clear();
        for (int which = 0; which < 2; ++which) {
            const Target::FlankMod& fm = t.fmod[which];
            const int64_t begin = which == 0 ? g.prefix_begin_whole : g.suffix_begin, end = which == 0 ? g.prefix_end : g.suffix_end_whole;
            if (!(begin >= 0 && begin < end && end <= (int64_t)rc.n) || fm.range.empty()) continue;
            const int64_t T = end - begin;
            const bool too_long = T > max_per_base * fm.len;          // a flank alignment that spread over a wrong place must not size the back-pointers
            const size_t first_rec = recs.size();
            for (size_t k = 0; k < fm.range.size(); ++k) {
                strq_flank_mod_group o = strq_flank_mod_group();
                o.flank = fm.info[3 * k]; o.pos = fm.info[3 * k + 1]; o.n_sites = fm.info[3 * k + 2]; o.n_columns = fm.range[k].c1 - fm.range[k].c0 + 1;
                o.status = too_long ? FMOD_TOO_LONG : FMOD_NO_PATH; o.begin = o.end = -1; o.v_base = o.v_mod = nan;
                recs.push_back(o);
            }
            if (!too_long) { fl.push_back({i, which, begin, T, first_rec}); sizes.push_back(bp_window_bytes(T, c->models[fm.model_id]->h.n_states)); }
        }
    }
    if (fl.empty()) return STRQ_OK;
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    const PiecePlan plan = plan_pieces(sizes, ws_budget(strq::opt("STRQ_FLANK_MOD_WS_BYTES")), OVERSIZE_ALONE);
    for (const Piece& pc : plan.pieces) {
        const size_t c0 = pc.first, c1 = pc.last, bytes = pc.bytes;
        const int m = (int)(c1 - c0);
        std::vector<GroupItem> items((size_t)m);
        size_t sumT = 0, Gs = 0; int n_mode[3] = {0, 0, 0};
        for (int k = 0; k < m; ++k) {
            const F& f = fl[c0 + (size_t)k];
            const Target::FlankMod& fm = target_of(d, r0 + f.i).fmod[f.which];
            HostModel* hm = c->models[fm.model_id];
            const int shape = vit_shape_for(hm->h, VIT_BACKPTR);
            if (shape < 0) { c->err = "flank-mod: the flank profile model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
            items[(size_t)k] = {0, shape, hm->h.n_cells};
            sumT += (size_t)f.T; Gs += fm.range.size();
            for (int sid : fm.site) {
                HostModel* sm = c->models[sid];
                if (!sm->llr_dev || sm->llr_mode < 0 || sm->llr_mode > 2) { c->err = "flank-mod: site model without an edge image (strq_target_set_flank_mod builds them)"; return STRQ_ERR_DEVICE; }
                ++n_mode[sm->llr_mode];
            }
        }
        const Grouping G = group_items(items);
        Carve lay;
        const size_t o_mt = lay.add<ModTask>((size_t)m), o_len = lay.add<int64_t>((size_t)m), o_vt = lay.add<VitTask>((size_t)m), o_vr = lay.add<VitResult>((size_t)m),
                     o_pp = lay.add<int32_t*>((size_t)m), o_bt = lay.add<FlankBoundTask>((size_t)m), o_order = lay.add<int>((size_t)m + 16),
                     o_gr = lay.add<FlankGroupRange>(Gs), o_ss = lay.add<FlankScoreSlot>(Gs), o_gb = lay.add<FlankGroupBounds>(Gs), o_rd = lay.add<LlrRead>(Gs),
                     o_w = lay.add<int32_t>(Gs), o_sc = lay.add<double>(2 * Gs), o_iota = lay.add<int64_t>(Gs + 1), o_x = lay.add<double>(sumT), o_path = lay.add<int32_t>(sumT);
        STRQ_HIP(c, d->fmod_ws.reserve(lay.total() + 64));
        STRQ_HIP(c, d->fmod_bp.reserve(bytes + 64));
        void* ws = d->fmod_ws.p;
        ModTask* d_mt = Carve::at<ModTask>(ws, o_mt); int64_t* d_len = Carve::at<int64_t>(ws, o_len); VitTask* d_vt = Carve::at<VitTask>(ws, o_vt);
        VitResult* d_vr = Carve::at<VitResult>(ws, o_vr); int32_t** d_pp = Carve::at<int32_t*>(ws, o_pp); FlankBoundTask* d_bt = Carve::at<FlankBoundTask>(ws, o_bt);
        int* d_order = Carve::at<int>(ws, o_order); FlankGroupRange* d_gr = Carve::at<FlankGroupRange>(ws, o_gr); FlankScoreSlot* d_ss = Carve::at<FlankScoreSlot>(ws, o_ss);
        FlankGroupBounds* d_gb = Carve::at<FlankGroupBounds>(ws, o_gb); LlrRead* d_rd = Carve::at<LlrRead>(ws, o_rd); int32_t* d_w = Carve::at<int32_t>(ws, o_w);
        double* d_sc = Carve::at<double>(ws, o_sc); int64_t* d_iota = Carve::at<int64_t>(ws, o_iota); double* d_x = Carve::at<double>(ws, o_x); int32_t* d_path = Carve::at<int32_t>(ws, o_path);
        std::vector<ModTask> mt((size_t)m); std::vector<VitTask> vt((size_t)m); std::vector<int32_t*> pp((size_t)m); std::vector<FlankBoundTask> bt((size_t)m);
        std::vector<FlankGroupRange> gr(Gs); std::vector<FlankScoreSlot> ss(Gs); std::vector<int64_t> iota(Gs + 1); std::vector<size_t> g_at((size_t)m);
        for (size_t k = 0; k <= Gs; ++k) iota[k] = (int64_t)k;
        int next_slot[3] = {0, n_mode[0], n_mode[0] + n_mode[1]};
        size_t xo = 0, go = 0, bo = 0;
        for (int k = 0; k < m; ++k) {
            const F& f = fl[c0 + (size_t)k];
            const Target& t = target_of(d, r0 + f.i); const Target::FlankMod& fm = t.fmod[f.which];
            const ReadCond& rc = h.rc[f.i];
            HostModel* hm = c->models[fm.model_id];
            const int at = G.pos[(size_t)k];
            ModTask& mk = mt[(size_t)k]; std::memset(&mk, 0, sizeof(mk));
            mk.raw = d->batch.raw.as<char>() + (size_t)(s0 + rc.off + f.begin) * esz;
            mk.out = d_x + xo; mk.T = f.T; mk.is_f64 = B.dtype;
            mk.c1 = rc.r_c1; mk.h1 = rc.r_h1; mk.h2 = rc.h2; mk.c2 = rc.c2;
            mk.clip_lo = d->ps.clip_lo; mk.clip_hi = d->ps.clip_hi; mk.mod_lo = t.mod_min; mk.mod_hi = t.mod_max;
            VitTask& v = vt[(size_t)at]; v = VitTask();
            v.model = hm->dev; v.sig = mk.out; v.T = f.T; v.src_kind = VIT_SRC_F64;
            v.bp = reinterpret_cast<uint16_t*>(d->fmod_bp.as<char>() + bo); bo += sizes[c0 + (size_t)k];
            pp[(size_t)at] = d_path + xo;
            FlankBoundTask& b = bt[(size_t)k]; std::memset(&b, 0, sizeof(b));
            b.path = d_path + xo; b.vit_status = &d_vr[at].status; b.column_of = fm.col->as<int32_t>();
            b.groups = d_gr + go; b.out = d_gb + go; b.T = f.T; b.n_emit = hm->silent_start; b.n_groups = (int32_t)fm.range.size();
            b.score = d_ss + go; b.x = mk.out; b.reads = d_rd; b.wloc = d_w; b.scores = d_sc;
            g_at[(size_t)k] = go;
            for (size_t j = 0; j < fm.range.size(); ++j) {
                HostModel* sm = c->models[fm.site[j]];
                gr[go + j] = fm.range[j];
                ss[go + j] = {sm->llr_dev, next_slot[sm->llr_mode]++, 0};
            }
            go += fm.range.size(); xo += (size_t)f.T;
        }
        if (bo > d->fmod_bp.cap) { c->err = "flank-mod: workspace"; return STRQ_ERR_NOMEM; }
        STRQ_HIP(c, hipMemcpyAsync(d_mt, mt.data(), (size_t)m * sizeof(ModTask), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_vt, vt.data(), (size_t)m * sizeof(VitTask), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_pp, pp.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_bt, bt.data(), (size_t)m * sizeof(FlankBoundTask), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_gr, gr.data(), Gs * sizeof(FlankGroupRange), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_ss, ss.data(), Gs * sizeof(FlankScoreSlot), hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemcpyAsync(d_iota, iota.data(), (Gs + 1) * 8, hipMemcpyHostToDevice, st));
        STRQ_HIP(c, hipMemsetAsync(d_path, 0, sumT * 4, st));          // a traceback that stops early leaves valid states behind
        if (launch_mod_compact(st, d_mt, m, d_len)) { c->err = "flank-mod: normalisation launch failed"; return STRQ_ERR_DEVICE; }
        d->stat(PASS_FMOD, FMOD_LAUNCHES) += 1;
        const GroupHook trace = [&](const VitGroup& g) -> int {
            if (launch_vit_traceback(st, d_vt + g.first, d_vr + g.first, d_pp + g.first, g.count)) { c->err = "flank-mod: traceback launch failed"; return STRQ_ERR_DEVICE; }
            d->stat(PASS_FMOD, FMOD_LAUNCHES) += 1;
            return STRQ_OK;
        };
        if (const int grc = launch_groups(c, st, G.groups, {d_vt, d_vr, d_order, {VIT_BACKPTR}, "flank-mod: ", false, &d->stat(PASS_FMOD, FMOD_LAUNCHES), nullptr, trace})) return grc;
        if (launch_flank_mod_bounds(st, d_bt, m)) { c->err = "flank-mod: bounds launch failed"; return STRQ_ERR_DEVICE; }
        d->stat(PASS_FMOD, FMOD_LAUNCHES) += 1;
        for (int mode = 0, at = 0; mode < 3; at += n_mode[mode++]) {
            if (!n_mode[mode]) continue;
            if (launch_llr_score(st, mode, d_rd + at, d_iota, n_mode[mode], n_mode[mode], c->n_cu)) { c->err = "flank-mod: score launch failed"; return STRQ_ERR_DEVICE; }
            d->stat(PASS_FMOD, FMOD_LAUNCHES) += 1;
        }
        std::vector<FlankGroupBounds> gb(Gs); std::vector<double> sc(2 * Gs);
        STRQ_HIP(c, hipMemcpyAsync(gb.data(), d_gb, Gs * sizeof(FlankGroupBounds), hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipMemcpyAsync(sc.data(), d_sc, 2 * Gs * 8, hipMemcpyDeviceToHost, st));
        STRQ_HIP(c, hipStreamSynchronize(st));
        for (int k = 0; k < m; ++k) {
            const F& f = fl[c0 + (size_t)k];
            const Target::FlankMod& fm = target_of(d, r0 + f.i).fmod[f.which];
            std::vector<strq_flank_mod_group>& recs = B.fmod[(size_t)(r0 + f.i)];
            for (size_t j = 0; j < fm.range.size(); ++j) {
                const FlankGroupBounds& b = gb[g_at[(size_t)k] + j];
                strq_flank_mod_group& o = recs[f.first_rec + j];
                o.status = b.status;
                if (b.status != FMOD_SCORED) continue;
                const int slot = ss[g_at[(size_t)k] + j].slot;
                o.begin = f.begin + b.u; o.end = f.begin + b.w; o.v_base = sc[2 * (size_t)slot]; o.v_mod = sc[2 * (size_t)slot + 1];
                d->stat(PASS_FMOD, FMOD_GROUPS) += 1;
            }
        }
        d->stat(PASS_FMOD, FMOD_FLANKS) += m;
    }
    return pass_stop(c, pass_ev(d), d->stats[PASS_FMOD]);
}

// Methylation calls of the anchored reads of one sub-batch (strq_set_anchored_mod), behind their records: a read of `R` is called
// when its record has status 0 -- its stretch [begin, end) is then not empty.  queued: dual_decode and dual_patterns ran behind the
// anchored decode on window-sized buffers (hub route); the patterns of the reads that turned out not to qualify are dropped and the
// lengths become the stretches'.  Otherwise (back-pointer route) the same two steps run here, on the stretches of the reads that
// qualify.  Then, with strq_set_mod_llr on, the per-unit scores of both branches as for a spanning read.
static int run_anchored_mod(strq_ctx* c, DetectState* d, DetectState::Slot& sl, DualRun& R, bool queued)
{
    Batch& B = d->batch;
    const int64_t r0 = sl.r0;
    auto called = [&](int i) { const strq_anchored& a = B.anch[(size_t)(r0 + i)]; return (a.kind == ANCH_ENDS || a.kind == ANCH_STARTS) && a.status == 0 && a.begin < a.end; };
    if (queued) {
        for (size_t k = 0; k < R.who.size(); ++k) {
            const strq_anchored& a = B.anch[(size_t)(r0 + R.who[k])];
            if (called(R.who[k])) R.len[k] = a.end - a.begin; else { R.len[k] = 0; B.amod[(size_t)(r0 + R.who[k])].clear(); }
        }
    } else {
        DualRun X;
        for (int i : R.who) {
            if (!called(i)) continue;
            const strq_anchored& a = B.anch[(size_t)(r0 + i)];
            X.who.push_back(i); X.raw_first.push_back(a.begin); X.len.push_back(a.end - a.begin);
        }
        R = std::move(X);
        if (R.who.empty()) return STRQ_OK;
        if (const int arc = pass_start(c, d->amod_ev)) return arc;
        if (const int drc = dual_decode(c, d, sl, DUAL_MOD, R)) return drc;
        if (const int prc = dual_patterns(c, d, sl, DUAL_MOD, R, B.amod)) return prc;
        if (const int arc = pass_stop(c, d->amod_ev, d->stats[PASS_AMOD])) return arc;
    }
    for (int i : R.who) {
        if (!called(i)) continue;
        const std::string& pat = B.amod[(size_t)(r0 + i)];
        B.amod_called[(size_t)(r0 + i)] = 1;
        d->stat(PASS_AMOD, AMOD_READS) += 1; d->stat(PASS_AMOD, AMOD_UNITS) += pat == "-" ? 0.0 : (double)pat.size();
    }
    d->stat(PASS_AMOD, AMOD_LAUNCHES) += R.launches;
    if (!sl.ex.llr) return STRQ_OK;
    LlrPassIn li = dual_tail_in(R);
    li.pattern = &B.amod; li.scores = &B.amod_llr; li.anchored = true;
    return run_llr_pass(c, d, sl, li);
}

// Anchored counting of the reads of one sub-batch (strq_set_anchored): the reads that hold one flank only are decoded once more, from
// their flank to their end (or from their start to their flank), with the target's end / start model.  Runs on the context's stream
// when the rows of the sub-batch are taken, like the unit pass: the geometry and the conditioning rows go back up from the slot's
// pinned block (the device copies belong to the sub-batch that followed), anchored_classify_kernel applies the rule, the host groups
// the reads of kind 2 / 3 by kernel shape, anchored_task_kernel writes their tasks on the slot's filtered signal, and the Viterbi
// kernels decode them in MARK mode: visits, log_p and the bounds of the repeat section in one decode.
static int run_anchored_pass(strq_ctx* c, DetectState* d, DetectState::Slot& sl)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int64_t r0 = sl.r0; const int nr = sl.nr;
    if (nr <= 0) return STRQ_OK;
    const DetectState::Slot::Pinned h = sl.host();
    if (const int rc = pass_start(c, pass_ev(d))) return rc;
    SlotRows rows;          // ... and the kinds of the reads behind them
    if (const int rc = upload_slot_rows(c, sl, d->anch_ws, rows, (size_t)nr * sizeof(AnchoredClass))) return rc;
    ReadCond* d_rc = rows.rc; AnchoredClass* d_cls = static_cast<AnchoredClass*>(rows.tail);
    AnchoredClassifyArgs ca;
    ca.geom = rows.geom; ca.rc = d_rc; ca.min_score = sl.ex.anch_min; ca.out = d_cls; ca.n_reads = nr;
    if (launch_anchored_classify(st, ca)) { c->err = "anchored: classify launch failed"; return STRQ_ERR_DEVICE; }
    std::vector<AnchoredClass> cls((size_t)nr);
    STRQ_HIP(c, hipMemcpyAsync(cls.data(), d_cls, (size_t)nr * sizeof(AnchoredClass), hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    d->stat(PASS_ANCH, ANCH_LAUNCHES) += 1;
    std::vector<int> who;
    for (int i = 0; i < nr; ++i) {
        const AnchoredClass& k = cls[(size_t)i];
        if (k.kind < ANCH_NONE || k.kind > ANCH_STARTS) { c->err = "anchored: kind outside the rule"; return STRQ_ERR_DEVICE; }
        d->stat(PASS_ANCH, ANCH_KINDS + k.kind) += 1;
        B.anch[(size_t)(r0 + i)].kind = k.kind;
        if (k.kind != ANCH_ENDS && k.kind != ANCH_STARTS) continue;
        // the window once more on the host, against the read as the conditioning saw it
        if (k.begin < 0 || k.begin >= k.end || k.end > (int64_t)h.rc[i].n) { c->err = "anchored: window outside its read"; return STRQ_ERR_DEVICE; }
        who.push_back(i);
    }
    const int m = (int)who.size();
    if (!m) return pass_stop(c, pass_ev(d), d->stats[PASS_ANCH]);
    DecodeOrder<VitModel> D; int orc = STRQ_OK;
    decode_order(who, [&](int i, GroupItem& it, const VitModel*& vm) {
        const Target& t = target_of(d, r0 + i);
        // (run_range refused the call before any launch when a target of the range had none)
        if (t.end_model_id < 0 || t.start_model_id < 0) { c->err = "anchored: target without anchored models (strq_target_set_anchored)"; orc = STRQ_ERR_ARG; return false; }
        HostModel* hm = anchored_model(c, d, r0 + i, cls[(size_t)i].kind);
        const int shape = vit_shape_for(hm->h, VIT_MARK);
        if (shape < 0) { c->err = "anchored: model does not fit a compiled Viterbi kernel"; orc = STRQ_ERR_UNSUPPORTED; return false; }
        it = {0, shape, hm->h.n_cells}; vm = hm->dev;
        return true;
    }, D);
    if (orc) return orc;
    const std::vector<int32_t>& read_of = D.read_of;
    Carve tl;
    const size_t o_vt = tl.add<VitTask>((size_t)m), o_vr = tl.add<VitResult>((size_t)m), o_md = tl.add<const VitModel*>((size_t)m), o_rd = tl.add<int32_t>((size_t)m);
    STRQ_HIP(c, d->anch_task.reserve(tl.total() + 64));
    VitTask* d_vt = Carve::at<VitTask>(d->anch_task.p, o_vt); VitResult* d_vr = Carve::at<VitResult>(d->anch_task.p, o_vr);
    const VitModel** d_md = Carve::at<const VitModel*>(d->anch_task.p, o_md); int32_t* d_rd = Carve::at<int32_t>(d->anch_task.p, o_rd);
    STRQ_HIP(c, hipMemcpyAsync(d_rd, read_of.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_md, D.model.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
    AnchoredTaskArgs ta;
    ta.cls = d_cls; ta.rc = d_rc; ta.read = d_rd; ta.model = d_md; ta.flt = sl.flt_base; ta.is_f64 = B.dtype; ta.ps = d->ps;
    ta.vit = d_vt; ta.n_tasks = m; ta.n_reads = nr;
    if (launch_anchored_tasks(st, ta)) { c->err = "anchored: task launch failed"; return STRQ_ERR_DEVICE; }
    d->stat(PASS_ANCH, ANCH_LAUNCHES) += 1;
    const GroupHook by_family = [&](const VitGroup& g) -> int {          // the windows by the family of kernels that decoded them
        const VitFamily fam = vit_shape_family(g.shape);
        if (fam == VIT_FAMILY_G2) d->stat(PASS_ANCH, ANCH_G2) += g.count; else if (fam == VIT_FAMILY_LANE) d->stat(PASS_ANCH, ANCH_LANE) += g.count;
        return STRQ_OK;
    };
    if (const int grc = launch_groups(c, st, D.G.groups, {d_vt, d_vr, sl.order.as<int>(), {VIT_MARK}, "anchored: ", false, &d->stat(PASS_ANCH, ANCH_LAUNCHES), nullptr, by_family})) return grc;
    std::vector<VitResult> vr((size_t)m);
    STRQ_HIP(c, hipMemcpyAsync(vr.data(), d_vr, (size_t)m * sizeof(VitResult), hipMemcpyDeviceToHost, st));
    // methylation calls (strq_set_anchored_mod): the reads of kind 2 / 3 whose target has a modification model, in task order
    DualRun R; AnchoredModSrc src = {d_cls, d_rc, d_vr, m, {}};
    if (sl.ex.amod)
        for (int at = 0; at < m; ++at) {
            const int i = read_of[(size_t)at];
            if (target_of(d, r0 + i).mod_model_id < 0) continue;
            const AnchoredClass& k = cls[(size_t)i];
            R.who.push_back(i); R.raw_first.push_back(k.begin); R.len.push_back(k.end - k.begin); src.res_of.push_back(at);
        }
    bool queued = false;
    if (!R.who.empty()) {
        // With hub records the pass is queued behind the decode, its buffers sized by the windows (the stretch of a read is never
        // longer), and the bracket of the anchored pass closes without a wait; the back-pointer route waits for the records first.
        std::vector<GroupItem> items; bool use_hub = false;
        if (const int rrc = dual_route(c, d, r0, DUAL_MOD, R, items, use_hub)) return rrc;
        if (use_hub) {
            STRQ_HIP(c, hipEventRecord(pass_ev(d)[1], st));
            if (const int arc = pass_start(c, d->amod_ev)) return arc;
            if (const int drc = dual_decode(c, d, sl, DUAL_MOD, R, &src)) return drc;
            if (const int prc = dual_patterns(c, d, sl, DUAL_MOD, R, B.amod)) return prc;          // (waits for the stream: the records are here)
            float ms = 0; STRQ_HIP(c, hipEventElapsedTime(&ms, pass_ev(d)[0], pass_ev(d)[1])); d->stats[PASS_ANCH].ms += ms;
            if (const int arc = pass_stop(c, d->amod_ev, d->stats[PASS_AMOD])) return arc;
            queued = true;
        }
    }
    if (!queued) { if (const int rc = pass_stop(c, pass_ev(d), d->stats[PASS_ANCH])) return rc; }
    for (int at = 0; at < m; ++at) {
        const int i = read_of[(size_t)at];
        const AnchoredClass& k = cls[(size_t)i];
        const Target& t = target_of(d, r0 + i);
        const VitResult& v = vr[(size_t)at];
        B.anch[(size_t)(r0 + i)] = anchored_record(k.kind, k.begin, k.end - k.begin, v.status, v.counted, k.kind == ANCH_ENDS ? t.end_bias : t.start_bias,
                                                   v.logp, (int64_t)v.dbg[0], (int64_t)v.dbg[1]);
    }
    return R.who.empty() ? STRQ_OK : run_anchored_mod(c, d, sl, R, queued);
}

// bytes [pos, pos + len) of the batch (reads back to back) from the caller's memory: one buffer, or one per read
static void host_bytes(const Batch& B, size_t esz, char* dst, size_t pos, size_t len)
{
    if (B.host_reads.empty()) { std::memcpy(dst, B.host_src + pos, len); return; }
    // the read that holds byte `pos`
    size_t r = (size_t)(std::upper_bound(B.off.begin(), B.off.end(), (int64_t)(pos / esz)) - B.off.begin()) - 1;
    while (len > 0) {
        const size_t r_begin = (size_t)B.off[r] * esz, r_end = (size_t)B.off[r + 1] * esz;
        const size_t take = std::min(len, r_end - pos);
        if (take) std::memcpy(dst, B.host_reads[r] + (pos - r_begin), take);
        dst += take; pos += take; len -= take; ++r;
    }
}

static int upload_reads(strq_ctx* c, DetectState* d, int64_t upto);

// waits for the prefetch thread (if any); returns what its upload returned
static int upload_join(DetectState* d)
{
    if (d->up_thread.joinable()) d->up_thread.join();
    const int rc = d->up_rc; d->up_rc = 0;
    return rc;
}

static void upload_prefetch(strq_ctx* c, DetectState* d, int64_t upto)
{
    Batch& B = d->batch;
    if (!B.on_host || upto <= B.uploaded) return;
    d->up_thread = std::thread([c, d, upto] {
        strq::CtxScope scope_(c);
        if (hipSetDevice(c->device) != hipSuccess) { d->up_rc = STRQ_ERR_DEVICE; return; }
        d->up_rc = upload_reads(c, d, upto);
    });
}

// Samples of reads [B.uploaded, upto) from the caller's (pageable) buffer into `raw`.  The runtime's own
// pageable path measures 8.3 GB/s; here the bytes go through a ring of pinned staging buffers: a few host
// threads copy the next piece into a free slot while the DMA engine drains the previous ones on the copy
// stream.  The calling thread blocks here while the kernels already queued on the compute stream keep
// running: that is the overlap of sub-batch k + 1's upload with sub-batch k's kernels.
static int upload_reads(strq_ctx* c, DetectState* d, int64_t upto)
{
    Batch& B = d->batch;
    if (!B.on_host || upto <= B.uploaded) return STRQ_OK;
    if (!d->copy_stream) STRQ_HIP(c, hipStreamCreateWithFlags(&d->copy_stream, hipStreamNonBlocking));
    const size_t esz = B.dtype == 0 ? 2 : 8;
    const size_t b0 = (size_t)B.off[B.uploaded] * esz, b1 = (size_t)B.off[upto] * esz;
    const size_t SLOT = (size_t)32 << 20;
    int n_threads = 6;
    if (const char* e = strq::opt("STRQ_UPLOAD_THREADS")) { const int v = atoi(e); if (v >= 0 && v <= 32) n_threads = v; }
    if (b1 > b0 && n_threads == 0) {          // the runtime's pageable path
        if (B.host_reads.empty()) STRQ_HIP(c, hipMemcpyAsync(B.raw.as<char>() + b0, B.host_src + b0, b1 - b0, hipMemcpyHostToDevice, d->copy_stream));
        else for (int64_t r = B.uploaded; r < upto; ++r) {
            const size_t rb = (size_t)B.off[r] * esz, rl = (size_t)(B.off[r + 1] - B.off[r]) * esz;
            if (rl) STRQ_HIP(c, hipMemcpyAsync(B.raw.as<char>() + rb, B.host_reads[r], rl, hipMemcpyHostToDevice, d->copy_stream));
        }
        STRQ_HIP(c, hipStreamSynchronize(d->copy_stream));
    } else if (b1 > b0) {
        for (int i = 0; i < DetectState::N_STAGE; ++i) {          // every entry on its own: what an earlier call could not get is tried again
            STRQ_HIP(c, d->stage[i].reserve(SLOT));
            if (!d->stage_ev[i]) STRQ_HIP(c, hipEventCreateWithFlags(&d->stage_ev[i], hipEventDisableTiming));
        }
        int slot = 0;
        for (size_t pos = b0; pos < b1; pos += SLOT, slot = (slot + 1) % DetectState::N_STAGE) {
            const size_t len = std::min(SLOT, b1 - pos);
            if (d->stage_busy[slot]) { STRQ_HIP(c, hipEventSynchronize(d->stage_ev[slot])); d->stage_busy[slot] = false; }
            char* dst = d->stage[slot].as<char>();
            const size_t part = ((len + n_threads - 1) / n_threads + 4095) & ~(size_t)4095;
            std::vector<std::thread> th;
            const Batch* Bp = &B;
            for (int t = 1; t < n_threads; ++t) {
                const size_t o = (size_t)t * part;
                if (o < len) th.emplace_back([=] { host_bytes(*Bp, esz, dst + o, pos + o, std::min(part, len - o)); });
            }
            host_bytes(B, esz, dst, pos, std::min(part, len));
            for (auto& t : th) t.join();
            STRQ_HIP(c, hipMemcpyAsync(B.raw.as<char>() + pos, dst, len, hipMemcpyHostToDevice, d->copy_stream));
            STRQ_HIP(c, hipEventRecord(d->stage_ev[slot], d->copy_stream));
            d->stage_busy[slot] = true;
        }
        STRQ_HIP(c, hipStreamSynchronize(d->copy_stream));
        for (int i = 0; i < DetectState::N_STAGE; ++i) d->stage_busy[i] = false;
    }
    B.uploaded = upto;
    return STRQ_OK;
}

static void publish_timing(strq_ctx* c, const Batch& B)
{
    std::fill(c->timing, c->timing + 8, 0.0f);
    c->timing[0] = B.t_lut; c->timing[1] = B.t_fwd; c->timing[2] = B.t_trace; c->timing[5] = B.t_cond; c->timing[6] = B.t_vit;
    c->timing[3] = B.t_lut + B.t_fwd + B.t_trace + B.t_cond + B.t_vit; c->timing[4] = (float)B.n_hard; c->timing[7] = (float)B.n_fwd_launches;
}

// A slot whose sub-batch cannot be completed: Idle, and the rows of its reads back at their initial values, so that no later call hands
// out rows that were never computed.  Returns `rc`, the error of the call that found out.
static int abandon(DetectState* d, DetectState::Slot& sl, int rc)
{
    Batch& B = d->batch;
    sl.state = DetectState::Slot::Idle;
    for (int64_t r = sl.r0; r < sl.r0 + sl.nr && r < (int64_t)B.results.size(); ++r) {
        B.clear_read(r);
        if (sl.scan && (size_t)r < B.cand.size()) {
            B.cand[(size_t)r] = -1;
            std::fill(B.scores.begin() + (ptrdiff_t)((size_t)r * 2 * B.scan_ncand), B.scores.begin() + (ptrdiff_t)((size_t)(r + 1) * 2 * B.scan_ncand), 0.0);
        }
    }
    return rc;
}

// the launches of launch_viterbi_of
static int queue_viterbi_launches(strq_ctx* c, DetectState::Slot& sl, hipStream_t vs, hipEvent_t after)
{
    if (after) STRQ_HIP(c, hipStreamWaitEvent(vs, after, 0));
    STRQ_HIP(c, hipMemsetAsync(sl.vq.p, 0, 1024, vs));
    for (auto& v : sl.vls) if (const int src = sort_viterbi_group(c, vs, v, sl.vit.as<VitTask>(), sl.order.as<int>())) return src;
    STRQ_HIP(c, hipEventRecord(sl.v0, vs));
    int qi = 0;
    std::memset(c->vit_launches, 0, sizeof(c->vit_launches));
    for (auto& v : sl.vls) {
        ++c->vit_launches[0];
        const VitFamily fam = vit_shape_family(v.shape);
        ++c->vit_launches[fam == VIT_FAMILY_G2 ? 1 : (fam == VIT_FAMILY_CSR ? 3 : 2)];
        const int lrc = launch_viterbi_group(c, vs, v, sl.vit.as<VitTask>(), sl.vres.as<VitResult>(), sl.order.as<int>(), sl.vq.as<int>() + qi++,
                                             sl.vit_mode, (after && vs != c->stream) ? 4 : 0);
        if (lrc) return lrc;
    }
    STRQ_HIP(c, hipMemcpyAsync(sl.host().vres, sl.vres.p, (size_t)sl.nr * sizeof(VitResult), hipMemcpyDeviceToHost, vs));
    STRQ_HIP(c, hipEventRecord(sl.v1, vs));
    return STRQ_OK;
}

// Queues the Viterbi launches of a sub-batch whose forward stage is complete (sort by window length, one persistent launch per kernel
// shape, results to pinned host memory) on `vs`, behind `after` when given.
static int launch_viterbi_of(strq_ctx* c, DetectState* d, DetectState::Slot& sl, hipStream_t vs, hipEvent_t after)
{
    if (sl.state != DetectState::Slot::Forward) return STRQ_OK;
    if (const int rc = queue_viterbi_launches(c, sl, vs, after)) return abandon(d, sl, rc);
    sl.state = DetectState::Slot::Decoding;
    return STRQ_OK;
}

// the rows of harvest
static int take_rows(strq_ctx* c, DetectState* d, DetectState::Slot& sl, bool under_current)
{
    Batch& B = d->batch;
    STRQ_HIP(c, hipEventSynchronize(sl.v1));
    const int nr = sl.nr; const int64_t r0 = sl.r0;
    const DetectState::Slot::Pinned h = sl.host();
    for (int i = 0; i < nr; ++i) {
        B.clear_read(r0 + i);          // row, pattern and the outputs of the passes below: whatever is not computed now stays at its initial value
        strq_result& o = B.results[r0 + i];
        const ReadGeom& g = h.geom[i];
        const VitResult& v = h.vres[sl.vit_slot[i]];
        o.status = h.rc[i].status == COND_OK ? 0 : 1;
        if (sl.ex.renorm) {
            const strq_renorm& rn = sl.rn_pin.as<strq_renorm>()[i];
            B.renorm[(size_t)(r0 + i)] = rn;
            d->stat(PASS_RENORM, RN_FITTED) += rn.fit[1].fitted != 0; d->stat(PASS_RENORM, RN_APPLIED) += rn.applied != 0;
        }
        if (sl.scan && B.cand[(size_t)(r0 + i)] < 0) continue;          // no winner: no row (the scores of its candidates are in Batch::scores)
        o.score_prefix = g.score_prefix; o.score_suffix = g.score_suffix;
        o.prefix_begin = g.prefix_begin; o.prefix_end = g.prefix_end; o.suffix_begin = g.suffix_begin; o.suffix_end = g.suffix_end;
        o.offset = g.prefix_end; o.ticks = std::max<int64_t>(g.suffix_begin - g.prefix_end, 0);
        B.flank_ends[2 * (size_t)(r0 + i)] = g.prefix_begin_whole; B.flank_ends[2 * (size_t)(r0 + i) + 1] = g.suffix_end_whole;
        if (g.gate) c->counters[7] += (double)(g.suffix_end - g.prefix_begin);
        if (g.gate && v.status == 0) {
            o.count = (int32_t)v.counted + target_of(d, r0 + i).count_bias;
            o.log_p = v.logp;
        }
    }
    float ms;
    STRQ_HIP(c, hipEventElapsedTime(&ms, sl.v0, sl.v1)); B.t_vit += ms;
    c->overlap[0] += ms;
    if (under_current) {
        // how much of these launches lay under the alignment kernels of the sub-batch that followed (whose events are the context's
        // current ones): [forward stage start, trace end], and the screen kernel alone
        auto under = [&](hipEvent_t a, hipEvent_t b) -> double {
            float ta = 0, tb = 0;
            if (hipEventElapsedTime(&ta, sl.v0, a) != hipSuccess || hipEventElapsedTime(&tb, sl.v0, b) != hipSuccess) return 0.0;
            return std::max(0.0, std::min((double)ms, (double)tb) - std::max(0.0, (double)ta));
        };
        if (c->screen_ran) c->overlap[1] += under(c->ev[5], c->ev[6]);
        c->overlap[2] += under(c->ev[2], c->ev[4]);
        c->overlap[3] += 1;
    }
    publish_timing(c, B);
    // the mode the launches ran with decides, not what the targets say by now
    if (sl.vit_mode == VIT_MARK) { const int mrc = run_mod_pass(c, d, sl); if (mrc) return mrc; }
    if (sl.vit_mode == VIT_MARK && sl.ex.var) { const int vrc = run_mod_pass(c, d, sl, DUAL_VAR); if (vrc) return vrc; }
    if (sl.ex.units || sl.ex.conf || sl.ex.sstats || sl.ex.spost) {
        Decoded dec;
        if (const int drc = read_decoded(c, sl, dec)) return drc;
        if (!dec.who.empty()) {
            if (sl.ex.units) { const int urc = run_unit_pass(c, d, sl, dec); if (urc) return urc; }
            if (sl.ex.conf) { const int crc = run_conf_pass(c, d, sl, dec); if (crc) return crc; }
            if (sl.ex.sstats) { const int src = run_state_stats_pass(c, d, sl, dec); if (src) return src; }
            if (sl.ex.spost) { const int prc = run_state_posteriors_pass(c, d, sl, dec); if (prc) return prc; }
        }
    }
    if (sl.ex.tracts) { const int trc = run_tract_pass(c, d, sl); if (trc) return trc; }
    if (sl.ex.fmod) { const int frc = run_flank_mod_pass(c, d, sl); if (frc) return frc; }
    if (sl.ex.motifs) { const int mrc = run_motif_pass(c, d, sl); if (mrc) return mrc; }
    return sl.ex.anch ? run_anchored_pass(c, d, sl) : STRQ_OK;
}

// Results of a sub-batch in flight: queues its Viterbi launches if nobody came after it, waits for them, fills Batch::results (and runs
// the modification pass of the sub-batch, which needs the decoded repeat stretch on the host, and its unit pass).
static int harvest(strq_ctx* c, DetectState* d, DetectState::Slot& sl, bool under_current = false)
{
    if (sl.state == DetectState::Slot::Idle) return STRQ_OK;
    if (const int lrc = launch_viterbi_of(c, d, sl, d->vit_stream, nullptr)) return lrc;
    if (const int rc = take_rows(c, d, sl, under_current)) return abandon(d, sl, rc);
    sl.state = DetectState::Slot::Idle;
    return STRQ_OK;
}

// every sub-batch still in flight, oldest first
static int drain(strq_ctx* c, DetectState* d)
{
    for (int k = 0; k < 2; ++k) { const int rc = harvest(c, d, d->slot[(d->next_slot + k) & 1]); if (rc) return rc; }
    return STRQ_OK;
}

int detect_drain(strq_ctx* c) { return c->detect ? drain(c, static_cast<DetectState*>(c->detect)) : STRQ_OK; }

// the Viterbi stream and the events of the pipeline, created once
static int ensure_sync_objects(strq_ctx* c, DetectState* d)
{
    for (auto& e : d->ev) if (!e) STRQ_HIP(c, hipEventCreate(&e));
    for (auto& sl : d->slot) {
        if (sl.fwd_done) continue;
        STRQ_HIP(c, hipEventCreateWithFlags(&sl.fwd_done, hipEventDisableTiming));
        STRQ_HIP(c, hipEventCreate(&sl.v0)); STRQ_HIP(c, hipEventCreate(&sl.v1));
    }
    if (!d->vit_stream) {
        // the older sub-batch's Viterbi launches go first where both streams have workgroups to place
        int lo = 0, hi = 0;
        STRQ_HIP(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
        STRQ_HIP(c, hipStreamCreateWithPriority(&d->vit_stream, hipStreamNonBlocking, hi));
    }
    return STRQ_OK;
}

// what the stages of one run_sub_batch call share
struct SubBatch {
    int64_t r0 = 0, s0 = 0, tot = 0;     // first read; its first sample in the batch; samples of the sub-batch
    int nr = 0, esz = 2;
    DetectState::Slot* sl = nullptr; DetectState::Slot* other = nullptr;
    bool any_mod = false, serial = false;
    int nc = 0;                          // scan: candidates per read (0: a plain detect, every read with its own target)
    std::vector<ReadCond> rc; std::vector<int64_t> loff;      // per read (host): conditioning row, offset in the sub-batch
    const char* raw = nullptr; char* flt_base = nullptr; uint8_t* levels = nullptr;
    ReadCond* d_rc = nullptr; uint32_t* d_hist_raw = nullptr; uint32_t* d_range = nullptr;
    int32_t* d_task_of = nullptr; int32_t* d_trim = nullptr; int32_t* d_slot = nullptr; const VitModel** d_model_of = nullptr;
    // scan: task table (2 * nc per read), trims (2 per candidate); scores, raw scores and winners on the device and in pinned memory
    int32_t* d_scan_task_of = nullptr; int32_t* d_scan_trim = nullptr;
    double* d_scores = nullptr; float* d_best = nullptr; int32_t* d_winner = nullptr;
    const double* h_scores = nullptr; const float* h_best = nullptr; const int32_t* h_winner = nullptr;
    size_t scan_out_bytes = 0;
};

// stage 1: the ReadCond rows and offsets of the reads (with the caller's statistics, for float64 reads that bring them)
static void read_table(DetectState* d, SubBatch& S)
{
    const Batch& B = d->batch;
    const int nr = S.nr; const int64_t r0 = S.r0;
    S.rc.resize(nr); S.loff.resize(nr + 1);
    for (int i = 0; i < nr; ++i) {
        ReadCond& rc = S.rc[i];
        std::memset(&rc, 0, sizeof(ReadCond));
        rc.off = B.off[r0 + i] - S.s0; rc.n = (int)(B.off[r0 + i + 1] - B.off[r0 + i]);
        S.loff[i] = rc.off;
        if (B.dtype == 1) {
            rc.h2 = (d->ps.M_hi - d->ps.M_lo) / 2; rc.c2 = d->ps.M_lo + (d->ps.M_hi - d->ps.M_lo) / 2;
        }
        if (B.dtype == 1 && !B.host_stats.empty()) {
            const double* hs = &B.host_stats[(size_t)(r0 + i) * 6];
            rc.med = hs[0]; rc.mad = hs[1]; rc.f_c1 = hs[2]; rc.f_h1 = hs[3]; rc.r_c1 = hs[4]; rc.r_h1 = hs[5];
            const bool okv = std::isfinite(hs[0]) && hs[1] > 0.0 && std::isfinite(hs[2]) && hs[3] > 0.0 && std::isfinite(hs[3]);
            rc.status = okv ? COND_OK : COND_DEGENERATE;
        }
        // (the variant pass needs the bounds of the repeat section like the modification pass: a MARK decode)
        if (!S.nc) S.any_mod |= target_of(d, r0 + i).mod_model_id >= 0 || (d->extras.var && target_of(d, r0 + i).var_model_id >= 0);
    }
    // scan: any candidate may win
    for (int c = 0; c < S.nc; ++c) S.any_mod |= d->targets[d->scan_cand[(size_t)c]].mod_model_id >= 0;
    S.loff[nr] = S.tot;
}

// stage 2: the buffers of the sub-batch, zeroed where the kernels accumulate; the ReadCond rows go up
static int reserve_buffers(strq_ctx* c, DetectState* d, SubBatch& S)
{
    const Batch& B = d->batch;
    hipStream_t st = c->stream;
    const int nr = S.nr;
    // both slots are sized together: the first sub-batch on the second slot would otherwise pay a 3 GB hipMalloc in the middle of a run
    // (a slot in flight is left alone: its buffers are in use and large enough for what it holds)
    for (DetectState::Slot* q : {S.sl, S.other})
        if (q == S.sl || q->state == DetectState::Slot::Idle) { const int rc = q->reserve(c, nr, (size_t)S.tot * S.esz + 64 + 16); if (rc) return rc; }
    STRQ_HIP(c, c->levels.reserve((size_t)S.tot + 64 + 8));
    STRQ_HIP(c, c->level_val.reserve((size_t)nr * 256 * 4));
    STRQ_HIP(c, d->rc.reserve((size_t)nr * sizeof(ReadCond)));
    STRQ_HIP(c, d->hist8.reserve((size_t)nr * 256 * 4));
    if (B.dtype == 0) STRQ_HIP(c, d->hist16.reserve((size_t)nr * 65536 * 4));
    STRQ_HIP(c, d->geom.reserve((size_t)nr * sizeof(ReadGeom)));
    S.d_rc = d->rc.as<ReadCond>();
    STRQ_HIP(c, hipMemcpyAsync(S.d_rc, S.rc.data(), (size_t)nr * sizeof(ReadCond), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemsetAsync(d->hist8.p, 0, (size_t)nr * 256 * 4, st));
    S.raw = B.raw.as<char>() + (size_t)S.s0 * S.esz;
    // the filtered signal of the sub-batch starts at the same offset inside a 16-byte line as its raw signal, so that the
    // conditioning kernels can move both with aligned 16-byte accesses
    S.flt_base = S.sl->flt.as<char>() + (reinterpret_cast<uintptr_t>(S.raw) & 15);
    d->last_slot = (int)(S.sl - d->slot); d->flt_shift = (int)(reinterpret_cast<uintptr_t>(S.raw) & 15); d->last_nr = nr;
    // levels: the same sample phase as the raw / filtered signal, so that a tile's eight-level groups are 8-byte aligned
    d->levels_shift = (int)((reinterpret_cast<uintptr_t>(S.raw) & 15) >> (S.esz == 2 ? 1 : 4));
    S.levels = c->levels.as<uint8_t>() + d->levels_shift;
    if (B.dtype == 0) {
        STRQ_HIP(c, hipMemsetAsync(d->hist16.p, 0, (size_t)nr * 65536 * 4, st));
        if (S.any_mod) {
            STRQ_HIP(c, d->hist_raw.reserve((size_t)nr * 65536 * 4));
            STRQ_HIP(c, hipMemsetAsync(d->hist_raw.p, 0, (size_t)nr * 65536 * 4, st));
            S.d_hist_raw = d->hist_raw.as<uint32_t>();
        }
        STRQ_HIP(c, d->hrange.reserve((size_t)nr * 16));
        STRQ_HIP(c, hipMemsetAsync(d->hrange.p, 0, (size_t)nr * 16, st));
        S.d_range = d->hrange.as<uint32_t>();
    }
    Carve lay;
    const size_t o_task_of = lay.add<int32_t>(2 * (size_t)nr), o_trim = lay.add<int32_t>(2 * (size_t)nr), o_slot = lay.add<int32_t>((size_t)nr),
                 o_model_of = lay.add<const VitModel*>((size_t)nr);
    STRQ_HIP(c, d->idx.reserve(lay.total() + 64));
    S.d_task_of = Carve::at<int32_t>(d->idx.p, o_task_of); S.d_trim = Carve::at<int32_t>(d->idx.p, o_trim); S.d_slot = Carve::at<int32_t>(d->idx.p, o_slot);
    S.d_model_of = Carve::at<const VitModel*>(d->idx.p, o_model_of);
    return STRQ_OK;
}

// stage 3: the Viterbi launches of the sub-batch.  Tasks are grouped by kernel shape over the whole sub-batch (windows of all models
// with one shape share a launch); finalize_kernel writes the task of read i to position vit_slot[i].
static int plan_viterbi(strq_ctx* c, DetectState* d, SubBatch& S)
{
    DetectState::Slot& sl = *S.sl;
    const int nr = S.nr;
    std::vector<GroupItem> items(nr);
    std::vector<const VitModel*> model_of(nr);
    for (int i = 0; i < nr; ++i) {
        HostModel* hm = flank_model(c, d, S.r0 + i);
        model_of[i] = hm->dev;
        const int shape = vit_shape_for(hm->h, S.any_mod ? VIT_MARK : VIT_COUNT);
        if (shape < 0) { c->err = "model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
        items[i] = {0, shape, hm->h.n_cells};
    }
    Grouping G = group_items(items);
    sl.vls.swap(G.groups); sl.vit_slot.swap(G.pos);
    STRQ_HIP(c, hipMemcpyAsync(S.d_model_of, model_of.data(), (size_t)nr * 8, hipMemcpyHostToDevice, c->stream));
    STRQ_HIP(c, hipMemcpyAsync(S.d_slot, sl.vit_slot.data(), (size_t)nr * 4, hipMemcpyHostToDevice, c->stream));
    return STRQ_OK;
}

// per upload part, reads [i0, i0 + np) of the sub-batch: conditioning (STRique.py:590-597)
static int condition_part(strq_ctx* c, DetectState* d, const SubBatch& S, int i0, int np)
{
    const Batch& B = d->batch;
    hipStream_t st = c->stream;
    ReadCond* d_rc = S.d_rc + i0;
    int longest = 0;
    for (int i = i0; i < i0 + np; ++i) longest = std::max(longest, S.rc[i].n);
    int bad = 0;
    float* level_val = c->level_val.as<float>() + (size_t)i0 * 256;
    uint32_t* hist8 = d->hist8.as<uint32_t>() + (size_t)i0 * 256;
    if (B.dtype == 0) {
        uint32_t* h16 = d->hist16.as<uint32_t>() + (size_t)i0 * 65536;
        uint32_t* hraw = S.d_hist_raw ? S.d_hist_raw + (size_t)i0 * 65536 : nullptr;
        uint32_t* rng = S.d_range + (size_t)i0 * 4;
        bad |= launch_medfilt_hist_i16(st, reinterpret_cast<const int16_t*>(S.raw), reinterpret_cast<int16_t*>(S.flt_base), d_rc, np, longest, h16, hraw, rng);
        bad |= launch_hist_stats(st, h16, 65536, -32768, d_rc, np, d->ps, 0, nullptr, rng, 4);
        if (S.any_mod) bad |= launch_hist_stats(st, hraw, 65536, -32768, d_rc, np, d->ps, 2, nullptr, rng + 2, 4);
        bad |= launch_quant_morph_i16(st, reinterpret_cast<const int16_t*>(S.flt_base), S.levels, d_rc, np, longest, hist8);
    } else {
        bad |= launch_medfilt_f64(st, reinterpret_cast<const double*>(S.raw), reinterpret_cast<double*>(S.flt_base), d_rc, np, longest);
        if (B.host_stats.empty()) {
            // median, MAD and the two 'minmax' maps of every read: one double of scratch per 8192 samples (numpy's mean)
            std::vector<int64_t> first((size_t)np + 1, 0);
            for (int i = 0; i < np; ++i) first[(size_t)i + 1] = first[(size_t)i] + (S.rc[i0 + i].n + 8191) / 8192;
            const size_t first_bytes = (((size_t)np + 1) * 8 + 255) & ~(size_t)255;
            STRQ_HIP(c, d->f64s.reserve(first_bytes + (size_t)first[(size_t)np] * 8 + 256));
            STRQ_HIP(c, hipMemcpyAsync(d->f64s.p, first.data(), ((size_t)np + 1) * 8, hipMemcpyHostToDevice, st));
            bad |= launch_f64_stats(st, reinterpret_cast<const double*>(S.flt_base), S.any_mod ? reinterpret_cast<const double*>(S.raw) : nullptr, d_rc, np,
                                    reinterpret_cast<double*>(d->f64s.as<char>() + first_bytes), d->f64s.as<int64_t>());
        } else {
            // the caller's statistics: nothing ties them to the samples -- a NaN among them makes the read degenerate
            bad |= launch_f64_nan_guard(st, reinterpret_cast<const double*>(S.flt_base), S.any_mod ? reinterpret_cast<const double*>(S.raw) : nullptr, d_rc, np);
        }
        bad |= launch_quant_morph_f64(st, reinterpret_cast<const double*>(S.flt_base), S.levels, d_rc, np, longest, hist8);
    }
    bad |= launch_hist_stats(st, hist8, 256, 0, d_rc, np, d->ps, 1, level_val, nullptr, 0);
    if (bad) { c->err = "conditioning launch failed"; return STRQ_ERR_DEVICE; }
    return STRQ_OK;
}

// per upload part, with strq_set_renorm on: the second normalisation step of its reads (strique_amd/renorm.py), between the conditioning
// statistics and everything that reads them.  Histograms of the three signals under their maps, the fit of each, the gate and the
// fold into the ReadCond rows and the level values; the records stay in the slot until its rows are taken.
static int run_renorm_part(strq_ctx* c, DetectState* d, const SubBatch& S, int i0, int np)
{
    const Batch& B = d->batch;
    hipStream_t st = c->stream;
    DetectState::Slot& sl = *S.sl;
    STRQ_HIP(c, d->rn_h.reserve((size_t)S.nr * RN_SIGNALS * RN_GRID * 4));
    STRQ_HIP(c, d->rn_reads.reserve((size_t)S.nr * sizeof(RenormRead)));
    STRQ_HIP(c, sl.rn_rec.reserve((size_t)S.nr * sizeof(strq_renorm)));
    for (auto& e : d->rn_ev) if (!e) STRQ_HIP(c, hipEventCreate(&e));
    std::vector<RenormRead> rr((size_t)np);
    int longest = 0;
    for (int i = 0; i < np; ++i) {
        const Target& t = target_of(d, S.r0 + i0 + i);
        rr[(size_t)i].table = t.rn_dev; rr[(size_t)i].raw = t.mod_model_id >= 0; rr[(size_t)i].pad_ = 0;
        longest = std::max(longest, S.rc[i0 + i].n);
    }
    RenormRead* d_rr = d->rn_reads.as<RenormRead>() + i0;
    uint32_t* h = d->rn_h.as<uint32_t>() + (size_t)i0 * RN_SIGNALS * RN_GRID;
    strq_renorm* rec = sl.rn_rec.as<strq_renorm>() + i0;
    ReadCond* d_rc = S.d_rc + i0;
    const uint32_t* hist8 = d->hist8.as<uint32_t>() + (size_t)i0 * 256;
    STRQ_HIP(c, hipMemcpyAsync(d_rr, rr.data(), (size_t)np * sizeof(RenormRead), hipMemcpyHostToDevice, st));
    const bool timed = d->rn_timed < 2;
    if (timed) STRQ_HIP(c, hipEventRecord(d->rn_ev[2 * d->rn_timed], st));
    STRQ_HIP(c, hipMemsetAsync(h, 0, (size_t)np * RN_SIGNALS * RN_GRID * 4, st));
    STRQ_HIP(c, hipMemsetAsync(rec, 0, (size_t)np * sizeof(strq_renorm), st));
    int bad = 0;
    if (B.dtype == 0) {
        const uint32_t* hraw = S.d_hist_raw ? S.d_hist_raw + (size_t)i0 * 65536 : nullptr;
        bad |= launch_renorm_hist_i16(st, d->hist16.as<uint32_t>() + (size_t)i0 * 65536, hraw, hist8, d_rc, d_rr, np, d->rn_grid, h);
        d->stat(PASS_RENORM, RN_LAUNCHES) += hraw ? 3 : 2;
    } else {
        bad |= launch_renorm_hist_f64(st, reinterpret_cast<const double*>(S.flt_base), S.any_mod ? reinterpret_cast<const double*>(S.raw) : nullptr, hist8, d_rc, d_rr,
                                      np, longest, d->rn_grid, h);
        d->stat(PASS_RENORM, RN_LAUNCHES) += longest > 0 ? 2 : 1;
    }
    bad |= launch_renorm_fit(st, h, d_rr, np, rec);
    bad |= launch_renorm_fold(st, d_rc, np, d->rn_grid, d->extras.renorm_min, d->ps, c->level_val.as<float>() + (size_t)i0 * 256, rec);
    d->stat(PASS_RENORM, RN_LAUNCHES) += 2;
    if (timed) { STRQ_HIP(c, hipEventRecord(d->rn_ev[2 * d->rn_timed + 1], st)); ++d->rn_timed; }
    if (bad) { c->err = "renorm: launch failed"; return STRQ_ERR_DEVICE; }
    return STRQ_OK;
}

// per upload part: the two flank alignments of every read.  The first part's score-table kernel is where the Viterbi launches of the
// sub-batch before this one are queued.
static int align_part(strq_ctx* c, DetectState* d, const SubBatch& S, int i0, int np, bool first_part, AlignCoreOut& co, std::vector<int32_t>& trim)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    DetectState::Slot& other = *S.other;
    // a plain detect aligns the two flanks of the read's target; a scan those of every candidate, all on the one conditioned read
    const int per = S.nc ? S.nc : 1;
    const int na = 2 * per * np;
    std::vector<int32_t> a_read(na); std::vector<int> n(na), m(na), k(na), R(na), NS(na); std::vector<const float*> fl(na);
    trim.resize(na);
    int samples = 6;
    for (int j = 0; j < np; ++j) for (int ci = 0; ci < per; ++ci) {
        const Target& t = d->targets[S.nc ? d->scan_cand[(size_t)ci] : B.target[S.r0 + i0 + j]];
        const int p = 2 * (j * per + ci), q = p + 1;
        samples = t.samples;
        a_read[p] = a_read[q] = j;
        n[p] = n[q] = S.rc[i0 + j].n;
        m[p] = (int)t.prefix_ext.size(); k[p] = t.kp; R[p] = t.Rp; NS[p] = t.NSp; fl[p] = t.prefix_ext.data(); trim[p] = t.trim_prefix;
        m[q] = (int)t.suffix_ext.size(); k[q] = t.ks; R[q] = t.Rs; NS[q] = t.NSs; fl[q] = t.suffix_ext.data(); trim[q] = t.trim_suffix;
    }
    AlignCoreIn ci;
    ci.nb = na; ci.samples = samples; ci.d_levels = S.levels; ci.read_off = S.loff.data() + i0; ci.d_level_val = c->level_val.as<float>() + (size_t)i0 * 256;
    ci.read = a_read.data(); ci.n = n.data(); ci.m = m.data(); ci.k = k.data(); ci.R = R.data(); ci.NS = NS.data(); ci.flank = fl.data();
    // (Launched behind this sub-batch's SCREEN instead -- under the exact pass and the trace, whose launches leave most of the GPU idle --
    // the eight Viterbi waves per CU take the LDS and registers those launches need: exact pass 69 instead of 19 ms, 180 against 175 ms per
    // step on clean reads, 400 against 338 on empirical ones: gpurun_out/r6r.)
    if (first_part) ci.after_tables = [&]() -> int {
        // The sub-batch before this one: its Viterbi launches start when this sub-batch's conditioning and score tables are through
        // -- a few ms of HBM-bound streaming kernels that crawl next to a GPU full of Viterbi waves (gpurun_out/r6d: 66 ms instead
        // of 5.7 ms; hist_stats_kernel alone keeps 60 KB of LDS per workgroup), and queued before the table kernel the Viterbi
        // launch kept the next screen from being dispatched until it had ended (gpurun_out/r6h against r6i, measured, both
        // priorities).  The alignment kernels that follow share the SIMDs with the Viterbi waves.
        const bool queued_now = other.state == DetectState::Slot::Forward;
        const int lrc = launch_viterbi_of(c, d, other, d->vit_stream, c->ev[1]); if (lrc) return lrc;
        // ... and they are dispatched after them: persistent workgroups that fill every CU for the length of the screen would
        // otherwise win the race now and then, and the Viterbi workgroups (eight waves of 192 VGPRs each: a whole CU's worth at
        // once) could not be placed before the screen has ended -- the serial order again
        if (queued_now) STRQ_HIP(c, hipStreamWaitEvent(st, other.v0, 0));
        return STRQ_OK;
    };
    const int rcode = align_core(c, ci, co);
    if (rcode) return rcode;
    B.n_hard += co.n_hard; B.n_fwd_launches += co.n_launches;
    c->counters[0] += co.wave_steps; c->counters[1] += co.columns; c->counters[2] += na;
    c->counters[3] = co.segs; c->counters[4] = co.tables; c->counters[5] = co.packed; c->counters[6] = co.rows_per_lane;
    return STRQ_OK;
}

// per upload part: positions, gate and Viterbi tasks of its reads
static int finalize_part(strq_ctx* c, DetectState* d, const SubBatch& S, int i0, int np, const AlignCoreOut& co, const std::vector<int32_t>& trim)
{
    hipStream_t st = c->stream;
    const int na = 2 * np;
    std::vector<int32_t> task_of(na);
    for (int pos = 0; pos < na; ++pos) task_of[co.order[pos]] = pos;
    STRQ_HIP(c, hipMemcpyAsync(S.d_task_of + 2 * (size_t)i0, task_of.data(), (size_t)na * 4, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(S.d_trim + 2 * (size_t)i0, trim.data(), (size_t)na * 4, hipMemcpyHostToDevice, st));
    FinalizeArgs fa;
    fa.tasks = co.d_tasks; fa.results = co.d_results; fa.task_of = S.d_task_of + 2 * (size_t)i0; fa.trim = S.d_trim + 2 * (size_t)i0; fa.vit_slot = S.d_slot + i0;
    fa.rc = S.d_rc + i0; fa.model_of = S.d_model_of + i0; fa.flt = S.flt_base; fa.is_f64 = d->batch.dtype; fa.ps = d->ps;
    fa.geom = d->geom.as<ReadGeom>() + i0; fa.vit = S.sl->vit.as<VitTask>(); fa.n_reads = np;
    hipLaunchKernelGGL(finalize_kernel, dim3((np + 127) / 128), dim3(128), 0, st, fa);
    STRQ_HIP(c, hipGetLastError());
    return STRQ_OK;
}

// scan: the task table, the candidates' trims and the outputs of scan_select_kernel for the sub-batch
static int scan_reserve(strq_ctx* c, DetectState* d, SubBatch& S)
{
    const size_t nr = (size_t)S.nr, nc = (size_t)S.nc;
    const size_t n_sc = 2 * nc * nr;
    Carve il;
    const size_t o_task_of = il.add<int32_t>(n_sc), o_trim = il.add<int32_t>(2 * nc);
    STRQ_HIP(c, d->scan_idx.reserve(il.total() + 64));
    S.d_scan_task_of = Carve::at<int32_t>(d->scan_idx.p, o_task_of); S.d_scan_trim = Carve::at<int32_t>(d->scan_idx.p, o_trim);
    // one layout for the outputs on the device and their pinned mirror (resolve_winners copies the block)
    Carve ol;
    const size_t o_scores = ol.add<double>(n_sc), o_best = ol.add<float>(n_sc), o_winner = ol.add<int32_t>(nr);
    S.scan_out_bytes = ol.total();
    STRQ_HIP(c, d->scan_out.reserve(S.scan_out_bytes + 64));
    STRQ_HIP(c, d->scan_pin.reserve(S.scan_out_bytes));
    S.d_scores = Carve::at<double>(d->scan_out.p, o_scores); S.d_best = Carve::at<float>(d->scan_out.p, o_best); S.d_winner = Carve::at<int32_t>(d->scan_out.p, o_winner);
    S.h_scores = Carve::at<double>(d->scan_pin.p, o_scores); S.h_best = Carve::at<float>(d->scan_pin.p, o_best); S.h_winner = Carve::at<int32_t>(d->scan_pin.p, o_winner);
    std::vector<int32_t> trim(2 * nc);
    for (size_t ci = 0; ci < nc; ++ci) {
        const Target& t = d->targets[d->scan_cand[ci]];
        trim[2 * ci] = t.trim_prefix; trim[2 * ci + 1] = t.trim_suffix;
    }
    STRQ_HIP(c, hipMemcpyAsync(S.d_scan_trim, trim.data(), 2 * nc * 4, hipMemcpyHostToDevice, c->stream));
    return STRQ_OK;
}

// scan, per upload part: positions and scores of all candidates of its reads, and the winner of each (scan_select_kernel)
static int select_part(strq_ctx* c, DetectState* d, const SubBatch& S, int i0, int np, const AlignCoreOut& co)
{
    hipStream_t st = c->stream;
    const size_t per = 2 * (size_t)S.nc;
    const int na = (int)per * np;
    std::vector<int32_t> task_of(na);
    for (int pos = 0; pos < na; ++pos) task_of[co.order[pos]] = pos;
    STRQ_HIP(c, hipMemcpyAsync(S.d_scan_task_of + per * i0, task_of.data(), (size_t)na * 4, hipMemcpyHostToDevice, st));
    ScanSelectArgs sa;
    sa.tasks = co.d_tasks; sa.results = co.d_results; sa.task_of = S.d_scan_task_of + per * i0; sa.trim = S.d_scan_trim; sa.rc = S.d_rc + i0;
    sa.min_score = d->scan_min; sa.geom = d->geom.as<ReadGeom>() + i0; sa.winner = S.d_winner + i0;
    sa.scores = S.d_scores + per * i0; sa.best = S.d_best + per * i0; sa.n_reads = np; sa.n_cand = S.nc;
    if (launch_scan_select(st, sa)) { c->err = "scan select launch failed"; return STRQ_ERR_DEVICE; }
    return STRQ_OK;
}

// scan: the winners of the sub-batch come back (one pinned copy, one wait on a stream that align_core has just waited on), every read
// takes the target of its winner, and from there the sub-batch is a plain one: its Viterbi launches are grouped by kernel shape on the
// host (plan_viterbi) and scan_task_kernel writes the winners' windows where finalize_kernel would have
static int resolve_winners(strq_ctx* c, DetectState* d, SubBatch& S)
{
    Batch& B = d->batch;
    hipStream_t st = c->stream;
    STRQ_HIP(c, hipMemcpyAsync(d->scan_pin.p, d->scan_out.p, S.scan_out_bytes, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    const size_t per = 2 * (size_t)S.nc;
    for (int i = 0; i < S.nr; ++i) {
        const int32_t w = S.h_winner[i];
        if (w < -1 || w >= S.nc) { c->err = "scan: winner outside the candidate list"; return STRQ_ERR_DEVICE; }
        B.cand[(size_t)(S.r0 + i)] = w;
        // a read without a winner keeps a (gate 0, never decoded) task with the first candidate's model
        B.target[(size_t)(S.r0 + i)] = d->scan_cand[(size_t)(w < 0 ? 0 : w)];
        std::memcpy(&B.scores[(size_t)(S.r0 + i) * per], S.h_scores + (size_t)i * per, per * 8);
    }
    if (const int rc = plan_viterbi(c, d, S)) return rc;
    ScanTaskArgs ta;
    ta.geom = d->geom.as<ReadGeom>(); ta.rc = S.d_rc; ta.vit_slot = S.d_slot; ta.model_of = S.d_model_of; ta.flt = S.flt_base; ta.is_f64 = B.dtype;
    ta.ps = d->ps; ta.vit = S.sl->vit.as<VitTask>(); ta.n_reads = S.nr;
    if (launch_scan_tasks(st, ta)) { c->err = "scan task launch failed"; return STRQ_ERR_DEVICE; }
    return STRQ_OK;
}

// the forward stage is queued: positions and conditioning status of the sub-batch to the host (pinned: the copies do not block), then
// the fork: everything the Viterbi launches read is final behind `fwd_done`
static int publish_forward(strq_ctx* c, DetectState* d, const SubBatch& S)
{
    DetectState::Slot& sl = *S.sl;
    hipStream_t st = c->stream;
    const DetectState::Slot::Pinned h = sl.host();
    STRQ_HIP(c, hipMemcpyAsync(h.geom, d->geom.p, (size_t)S.nr * sizeof(ReadGeom), hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(h.rc, S.d_rc, (size_t)S.nr * sizeof(ReadCond), hipMemcpyDeviceToHost, st));
    if (d->extras.renorm && !S.nc) {
        STRQ_HIP(c, sl.rn_pin.reserve((size_t)S.nr * sizeof(strq_renorm) + 64));
        STRQ_HIP(c, hipMemcpyAsync(sl.rn_pin.p, sl.rn_rec.p, (size_t)S.nr * sizeof(strq_renorm), hipMemcpyDeviceToHost, st));
    }
    *h.redo = 0;
    if (c->redo_total.p) STRQ_HIP(c, hipMemcpyAsync(h.redo, c->redo_total.p, 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipEventRecord(sl.fwd_done, st));
    sl.vit_mode = S.any_mod ? VIT_MARK : VIT_COUNT;
    sl.ex = d->extras;
    sl.scan = S.nc > 0;
    sl.flt_base = S.flt_base;
    sl.state = DetectState::Slot::Forward;
    return STRQ_OK;
}

// score distribution of this sub-batch for the overlap planning of the next one (align_core)
static void plan_next_overlap(strq_ctx* c, DetectState* d, const SubBatch& S)
{
    if (!(c->ap.dist_offset > 0.0f)) return;
    const ReadGeom* h_geom = S.sl->host().geom;
    c->score_fracs.clear(); double sum_n = 0;
    for (int i = 0; i < S.nr; ++i) {
        if (S.rc[i].n <= 0) continue;
        if (S.nc) {          // a scan: the next sub-batch aligns every candidate again, most of them on reads that do not hold their flanks
            for (int ci = 0; ci < S.nc; ++ci) {
                const Target& t = d->targets[d->scan_cand[(size_t)ci]];
                const float* b = S.h_best + 2 * ((size_t)i * S.nc + ci);
                c->score_fracs.push_back(b[0] / ((float)t.prefix_ext.size() * c->ap.dist_offset));
                c->score_fracs.push_back(b[1] / ((float)t.suffix_ext.size() * c->ap.dist_offset));
                sum_n += S.rc[i].n;
            }
            continue;
        }
        const Target& t = target_of(d, S.r0 + i);
        c->score_fracs.push_back(h_geom[i].best_prefix / ((float)t.prefix_ext.size() * c->ap.dist_offset));
        c->score_fracs.push_back(h_geom[i].best_suffix / ((float)t.suffix_ext.size() * c->ap.dist_offset));
        sum_n += S.rc[i].n;
    }
    std::sort(c->score_fracs.begin(), c->score_fracs.end());
    c->mean_n = c->score_fracs.empty() ? 0.0 : sum_n / (double)(c->score_fracs.size() / 2);
}

// What follows the published forward stage: the Viterbi launches in the serial order, the wait for the forward stage, the planning of
// the next sub-batch, the times, and the rows that are due.
static int complete_sub_batch(strq_ctx* c, DetectState* d, const SubBatch& S)
{
    Batch& B = d->batch;
    DetectState::Slot& sl = *S.sl; DetectState::Slot& other = *S.other;
    // The Viterbi launches of this sub-batch: now on the context's stream (serial order), or -- two sub-batches in flight -- behind the
    // conditioning of the NEXT sub-batch (launch_viterbi_of from there), at the latest when somebody asks for the rows.  Conditioning is a
    // few ms of HBM-bound streaming kernels that crawl next to a GPU full of Viterbi waves (gpurun_out/r6d: 66 ms instead of 5.7 ms); the
    // flank-alignment kernels that follow share the SIMDs with them at little cost.
    if (S.serial) { const int lrc = launch_viterbi_of(c, d, sl, c->stream, nullptr); if (lrc) return lrc; }
    // the forward stage of this sub-batch is complete here (its Viterbi launches need not be)
    STRQ_HIP(c, hipEventSynchronize(sl.fwd_done));
    c->second_round[0] = (int64_t)*sl.host().redo - c->look2_served; c->second_round[1] += 2 * (int64_t)S.nr * (S.nc ? S.nc : 1);
    plan_next_overlap(c, d, S);
    float ms;
    STRQ_HIP(c, hipEventElapsedTime(&ms, d->ev[0], d->ev[1])); B.t_cond += ms;
    for (int k = 0; k < d->rn_timed; ++k) { STRQ_HIP(c, hipEventElapsedTime(&ms, d->rn_ev[2 * k], d->rn_ev[2 * k + 1])); d->stats[PASS_RENORM].ms += ms; }
    d->rn_timed = 0;
    const int rcode = align_core_times(c, &B.t_lut, &B.t_fwd, &B.t_trace);      // of the last piece when the sub-batch ran in pieces
    if (rcode) return rcode;
    // results: of the sub-batch before this one (its Viterbi launches ran under this sub-batch's forward stage) -- or, serially, of this one
    if (strq::opt("STRQ_DEBUG") && !S.serial && other.state == DetectState::Slot::Decoding && c->screen_ran) {
        float a = 0, b = 0, e = 0;
        (void)hipEventSynchronize(other.v1);
        (void)hipEventElapsedTime(&a, other.v0, c->ev[5]); (void)hipEventElapsedTime(&e, other.v0, c->ev[6]); (void)hipEventElapsedTime(&b, other.v0, other.v1);
        STRQ_DBG("overlap: Viterbi launches of the previous sub-batch start at 0, end at %.1f ms; this sub-batch's screen runs from %.1f to %.1f ms", b, a, e);
    }
    if (S.serial) return harvest(c, d, sl);
    return harvest(c, d, other, /*under_current=*/true);
}

static int run_sub_batch(strq_ctx* c, DetectState* d, int64_t r0, int64_t r1, int64_t next_r1)
{
    Batch& B = d->batch;
    SubBatch S;
    S.r0 = r0; S.nr = (int)(r1 - r0); S.esz = B.dtype == 0 ? 2 : 8;
    S.s0 = B.off[r0]; S.tot = B.off[r1] - S.s0;
    // the slot of this sub-batch (its previous user's results are taken first: normally done a sub-batch ago)
    DetectState::Slot& sl = d->slot[d->next_slot];
    S.sl = &sl; S.other = &d->slot[d->next_slot ^ 1];
    { const int urc = upload_join(d); if (urc) { c->err = "upload of the sub-batch's samples failed (prefetch thread)"; return urc; } }
    { const int hrc = harvest(c, d, sl); if (hrc) return hrc; }
    d->next_slot ^= 1;
    sl.r0 = r0; sl.nr = S.nr;
    // STRQ_SERIAL=1: the Viterbi launches on the context's own stream and their results before the call returns, as up to round 5.
    // (A sub-batch with a modification model is pipelined like any other: its MARK-mode Viterbi launches run under the next sub-batch's
    // alignments; its second pass -- which needs the decoded repeat stretch on the host -- runs when its rows are taken, on the context's
    // stream, which is idle then: the taking thread has just waited for the following sub-batch's forward stage, or is the caller's fetch.)
    S.serial = strq::opt("STRQ_SERIAL") != nullptr;
    S.nc = B.scan_ncand;
    read_table(d, S);
    if (const int rc = reserve_buffers(c, d, S)) return rc;
    // a scan plans its Viterbi launches when the winners are known (resolve_winners)
    if (S.nc) { if (const int rc = scan_reserve(c, d, S)) return rc; }
    else if (const int rc = plan_viterbi(c, d, S)) return rc;
    // Conditioning, the two flank alignments and the positions / gate of the reads, in `parts` pieces: a
    // sub-batch whose samples are still in the caller's buffer is uploaded piece by piece, each piece's
    // kernels running under the upload of the next (only the first piece's upload is exposed); a resident
    // or prefetched sub-batch is one piece.  The Viterbi launches always cover the whole sub-batch.
    const int parts = (B.on_host && B.uploaded < r1 && S.nr >= 1024) ? 2 : 1;
    for (int part = 0; part < parts; ++part) {
        const int i0 = (int)((int64_t)S.nr * part / parts), i1 = (int)((int64_t)S.nr * (part + 1) / parts), np = i1 - i0;
        if (np <= 0) continue;
        if (const int urc = upload_reads(c, d, r0 + i1)) return urc;
        // this sub-batch's samples are in HBM (or queued): the next sub-batch's follow on their own thread from here on
        if (part == parts - 1) upload_prefetch(c, d, next_r1);
        if (part == 0) STRQ_HIP(c, hipEventRecord(d->ev[0], c->stream));
        if (const int rc = condition_part(c, d, S, i0, np)) return rc;
        if (part == 0) STRQ_HIP(c, hipEventRecord(d->ev[1], c->stream));
        if (d->extras.renorm && !S.nc) { if (const int rc = run_renorm_part(c, d, S, i0, np)) return rc; }
        AlignCoreOut co; std::vector<int32_t> trim;
        if (const int rc = align_part(c, d, S, i0, np, part == 0, co, trim)) return rc;
        if (S.nc) { if (const int rc = select_part(c, d, S, i0, np, co)) return rc; }
        else if (const int rc = finalize_part(c, d, S, i0, np, co, trim)) return rc;
    }
    if (S.nc) if (const int rc = resolve_winners(c, d, S)) { sl.scan = true; return abandon(d, sl, rc); }
    if (const int rc = publish_forward(c, d, S)) return rc;
    // from here on the slot is in flight: a failure leaves no rows behind that were not computed
    if (const int rc = complete_sub_batch(c, d, S)) return abandon(d, sl, rc);
    return STRQ_OK;
}

}  // namespace strq

namespace {

// target ids and read lengths of `n` reads as a caller hands them over
int check_reads(strq_ctx* c, const DetectState* d, int64_t n, const int64_t* offsets, const int32_t* target_id)
{
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (target_id[i] < 0 || target_id[i] >= (int32_t)d->targets.size()) { c->err = "unknown target id"; return STRQ_ERR_ARG; }
        if (len < 0 || len > ((int64_t)1 << 30)) { c->err = "bad offsets"; return STRQ_ERR_ARG; }
    }
    return STRQ_OK;
}

// a new batch of `n` reads: the sub-batches of the previous one that are still in flight are taken first
int begin_batch(strq_ctx* c, DetectState* d, int64_t n, int dtype)
{
    if (const int rc = drain(c, d)) return rc;
    if (const int rc = ensure_sync_objects(c, d)) return rc;
    d->batch.begin(n, dtype);
    d->part_reads = 0;
    return STRQ_OK;
}

int batch_prepare(strq_ctx* c, int64_t n_reads, const void* signals, int32_t dtype, const int64_t* offsets,
                  const int32_t* target_id, const double* host_stats, bool lazy, const void* const* reads = nullptr)
{
    DetectState* d = dstate(c);
    if (n_reads < 0 || (n_reads > 0 && ((!signals && !reads) || !offsets || !target_id)) || (dtype != 0 && dtype != 1)) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (!d->have_ps) { c->err = "strq_set_pore_stats has not been called"; return STRQ_ERR_ARG; }
    if (const int rc = begin_batch(c, d, n_reads, dtype)) return rc;
    Batch& B = d->batch;
    B.off.assign(offsets, offsets + n_reads + 1);
    B.target.assign(target_id, target_id + n_reads);
    if (const int rc = check_reads(c, d, n_reads, offsets, target_id)) return rc;
    // float64 reads have no exact histogram: their order statistics come from a radix selection on the GPU (cond_kernels.hip:
    // f64_stats_kernel) unless the caller hands over its own (numpy's) six scalars per read
    if (dtype == 1 && host_stats) B.host_stats.assign(host_stats, host_stats + n_reads * 6);
    const size_t bytes = (size_t)(n_reads ? B.off[n_reads] : 0) * (dtype == 0 ? 2 : 8);
    STRQ_HIP(c, B.raw.reserve(bytes + 64));
    B.host_src = static_cast<const char*>(signals); B.on_host = true;
    if (reads) B.host_reads.assign(reinterpret_cast<const char* const*>(reads), reinterpret_cast<const char* const*>(reads) + n_reads);
    if (!lazy) {
        const int rc = upload_reads(c, d, n_reads);      // resident batch: everything now
        if (rc) return rc;
        B.forget_host();
    }
    return STRQ_OK;
}

// sub-batches of reads [first, last): returns the cuts
std::vector<int64_t> cut_sub_batches(const strq_ctx* c, const DetectState* d, int64_t first, int64_t last)
{
    const Batch& B = d->batch;
    // Sub-batch size: 16 reads (32 alignments) per CU.  The alignments of a batch are about equally
    // long, so the forward DP proceeds in rounds: 32 per CU is four full rounds of the eight waves the
    // 24-bit tables allow (and, with six float32 waves -- two alone on their SIMD at 60.6 ms per
    // alignment, four sharing one at 73 ms -- 6 x 60.6 = 5 x 73 ends without a ragged tail as well;
    // 4608 reads measured 437 ms against 365 ms for 4096).
    int64_t cap = std::min<int64_t>(16 * (int64_t)c->n_cu, 8192);      // 8192: task limit of vit_sort_kernel
    // a scan aligns every read 2 * n_cand times: as many alignments per sub-batch as a plain detect has
    if (B.scan_ncand) cap = std::max<int64_t>(1, cap / B.scan_ncand);
    if (const char* e = strq::opt("STRQ_SUBBATCH_READS")) { const int64_t v = atoll(e); if (v > 0) cap = std::min<int64_t>(v, B.scan_ncand ? std::max<int64_t>(1, 8192 / B.scan_ncand) : 8192); }      // testing: force small sub-batches
    std::vector<int64_t> cuts(1, first);
    for (int64_t r0 = first; r0 < last;) {
        int64_t r1 = r0; size_t ck = 0; int64_t samples = 0;
        while (r1 < last && r1 - r0 < cap) {
            const int n = (int)(B.off[r1 + 1] - B.off[r1]);
            size_t need = 0;
            for (int ci = 0; ci < std::max(1, B.scan_ncand); ++ci) {
                const Target& t = d->targets[B.scan_ncand ? d->scan_cand[(size_t)ci] : B.target[r1]];
                need += align_workspace_bytes(n, 0, t.Rp, t.NSp) + align_workspace_bytes(n, 0, t.Rs, t.NSs);
            }
            if (r1 > r0 && (ck + need > c->max_ws_bytes || samples + n > ((int64_t)3 << 30))) break;
            ck += need; samples += n; ++r1;
        }
        cuts.push_back(r1);
        r0 = r1;
    }
    return cuts;
}

int run_range(strq_ctx* c, DetectState* d, int64_t first, int64_t last)
{
    Batch& B = d->batch;
    if (first < 0 || last < first || last > B.n_reads) { c->err = "read range outside the uploaded batch"; return STRQ_ERR_ARG; }
    B.t_cond = B.t_lut = B.t_fwd = B.t_trace = B.t_vit = 0; B.n_hard = 0; B.n_fwd_launches = 0;
    std::fill(c->counters, c->counters + 8, 0.0);
    std::fill(c->overlap, c->overlap + 4, 0.0);
    c->second_round[0] = c->second_round[1] = 0; c->look2_served = 0;
    for (double& v : c->screen_stats) v = 0;
    // Rows in flight belong to the call that launched them: a change between scan and plain detect takes them first.
    if ((d->scan_on ? (int)d->scan_cand.size() : 0) != B.scan_ncand) {
        if (const int rc = drain(c, d)) return rc;
        // What the context has learnt about its workload does not carry over: three alignments in four of a scan look for a flank the
        // read does not hold, so the screens' pauses and the score distribution of the overlap planning would send the first sub-batches
        // of a detect after a scan (or of a scan after a detect) down the route of the other workload.
        c->screen_pause = c->coarse_pause = 0; c->screen_fail = c->coarse_fail = 0;
        c->score_fracs.clear(); c->mean_n = 0;
    }
    if (d->scan_on) {
        if (B.target_given.empty()) B.target_given = B.target;
        B.scan_ncand = (int)d->scan_cand.size();
        if (B.cand.size() != (size_t)B.n_reads || B.scores.size() != (size_t)B.n_reads * 2 * (size_t)B.scan_ncand) {
            B.cand.assign((size_t)B.n_reads, -1); B.scores.assign((size_t)B.n_reads * 2 * (size_t)B.scan_ncand, 0.0);
        }
    } else {
        if (!B.target_given.empty()) { B.target = B.target_given; B.target_given.clear(); }
        B.scan_ncand = 0; B.cand.clear(); B.scores.clear();
    }
    // refused here, before any launch: a scan has no anchored records, variants, tracts or fits (the first pass in SCAN_CHECKS says so)
    if (d->scan_on) { const Pass p = scan_refusal(d->extras); if (p != N_PASS) { c->err = scan_refusal_text(p); return STRQ_ERR_ARG; } }
    if (d->extras.amod) {
        // (the calls hang on the anchored records)
        if (!d->extras.anch) { c->err = "anchored-mod: needs anchored counting (strq_set_anchored)"; return STRQ_ERR_ARG; }
        B.size_amod();
    }
    if (d->extras.anch) {
        // nothing is launched for a call the anchored pass could not finish
        for (int64_t r = first; r < last; ++r) {
            const Target& t = d->targets[B.target_given.empty() ? B.target[(size_t)r] : B.target_given[(size_t)r]];
            if (t.end_model_id < 0 || t.start_model_id < 0) { c->err = "anchored: target without anchored models (strq_target_set_anchored)"; return STRQ_ERR_ARG; }
        }
    }
    if (d->extras.tracts) B.size_tracts();
    if (d->extras.tpos) {
        // (the positions hang on the tract records); nothing is launched for a call whose compound models cannot be traced back
        if (!d->extras.tracts) { c->err = "tract-positions: needs the tract pass (strq_set_tracts)"; return STRQ_ERR_ARG; }
        for (int64_t r = first; r < last; ++r) {
            const Target& t = d->targets[B.target_given.empty() ? B.target[(size_t)r] : B.target_given[(size_t)r]];
            if (t.tract_model_id < 0) continue;
            const VitModel& mh = c->models[t.tract_model_id]->h;
            if (!vit_mode_ok(vit_shape_for(mh, VIT_BACKPTR), VIT_BACKPTR)) { c->err = "tract-positions: a target's compound model has no back-pointer decode"; return STRQ_ERR_UNSUPPORTED; }
        }
        B.size_tpos();
    }
    if (d->extras.fmod) B.size_fmod();
    if (d->extras.motifs) B.size_motifs();
    if (d->extras.sstats) {
        // nothing is launched for a call whose flanked models cannot be traced back
        for (int64_t r = first; r < last; ++r) {
            const VitModel& mh = c->models[d->targets[B.target_given.empty() ? B.target[(size_t)r] : B.target_given[(size_t)r]].model_id]->h;
            if (!vit_mode_ok(vit_shape_for(mh, VIT_BACKPTR), VIT_BACKPTR)) { c->err = "state-stats: a target's model has no back-pointer decode"; return STRQ_ERR_UNSUPPORTED; }
        }
        B.size_sst();
    }
    if (d->extras.spost) {
        // nothing is launched for a call whose flanked models have no forward kernel
        for (int64_t r = first; r < last; ++r) {
            HostModel* hm = c->models[d->targets[B.target_given.empty() ? B.target[(size_t)r] : B.target_given[(size_t)r]].model_id];
            if (const int rc = posterior_model(c, hm)) return rc;
        }
        B.size_spost();
    }
    if (d->extras.renorm) {
        // nothing is launched for a call whose reads the pass could not fit
        if (!d->rn_have_grid) { c->err = "renorm: no tables (strq_target_set_renorm)"; return STRQ_ERR_ARG; }
        for (int64_t r = first; r < last; ++r)
            if (!d->targets[B.target_given.empty() ? B.target[(size_t)r] : B.target_given[(size_t)r]].rn_dev) { c->err = "renorm: target without tables (strq_target_set_renorm)"; return STRQ_ERR_ARG; }
        B.size_renorm();
    }
    B.ran = d->extras;
    std::fill(d->stats, d->stats + N_PASS, PassStats()); d->rn_timed = 0;
    STRQ_HIP(c, c->redo_total.reserve(64));
    STRQ_HIP(c, hipMemsetAsync(c->redo_total.p, 0, 64, c->stream));
    // partition into sub-batches first, so that the upload of piece k + 1 can overlap the kernels of piece k
    const std::vector<int64_t> cuts = cut_sub_batches(c, d, first, last);
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        const double t1 = now_s();
        // samples not yet in HBM (first sub-batch of strq_detect_batch) are uploaded piece by piece inside
        const int rc = run_sub_batch(c, d, cuts[k], cuts[k + 1], k + 2 < cuts.size() ? cuts[k + 2] : cuts[k + 1]);
        if (rc) { (void)upload_join(d); return rc; }          // (the prefetch thread reads the caller's buffers: never left running)
        STRQ_DBG("sub-batch %zu: reads %ld..%ld  %.1f ms", k, (long)cuts[k], (long)cuts[k + 1], (now_s() - t1) * 1e3);
    }
    { const int urc = upload_join(d); if (urc) { c->err = "upload of the batch's samples failed (prefetch thread)"; return urc; } }
    B.forget_host();      // the caller's buffers are not referenced after the call
    publish_timing(c, B);
    return STRQ_OK;
}

// tail of strq_detect_batch(_reads): the prepared batch through the pipeline, its rows to `out`
int run_and_fetch(strq_ctx* c, strq_result* out)
{
    DetectState* d = dstate(c);
    const int rc = run_range(c, d, 0, d->batch.n_reads);
    d->batch.forget_host();
    if (rc) return rc;
    if (!out) return STRQ_ERR_ARG;
    if (const int drc = drain(c, d)) return drc;
    std::memcpy(out, d->batch.results.data(), d->batch.results.size() * sizeof(strq_result));
    return STRQ_OK;
}

// the arguments of a scan: at least one candidate, every one a target of the context, a threshold above 0
int scan_check(strq_ctx* c, const DetectState* d, int32_t n_cand, const int32_t* ids, double min_score)
{
    if (n_cand <= 0 || n_cand > 256 || !ids) { c->err = "scan: between 1 and 256 candidates"; return STRQ_ERR_ARG; }
    if (!(min_score > 0.0)) { c->err = "scan: min_score must be above 0"; return STRQ_ERR_ARG; }
    for (int32_t i = 0; i < n_cand; ++i)
        if (ids[i] < 0 || ids[i] >= (int32_t)d->targets.size()) { c->err = "scan: unknown target id"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

// winners and scores of the last run call (drained by the caller)
int copy_scan(strq_ctx* c, const DetectState* d, int32_t* out_cand, double* out_scores)
{
    const Batch& B = d->batch;
    if (!B.scan_ncand) { c->err = "the last run call was no scan (strq_scan_set)"; return STRQ_ERR_ARG; }
    if (!out_cand && B.n_reads > 0) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (!B.cand.empty()) std::memcpy(out_cand, B.cand.data(), B.cand.size() * 4);
    if (out_scores && !B.scores.empty()) std::memcpy(out_scores, B.scores.data(), B.scores.size() * 8);
    return STRQ_OK;
}

// strq_set_<pass>: one switch of DetectState::extras.  An argument other than 0 or 1 is refused in the entry's name; `validate`: what
// must hold before the switch goes on.  A switch that comes with a threshold (anchored, renorm): `level` is where it goes (0 with the
// switch off), `level_ok` whether the value will do and `level_bad` the message if not; a scan refuses renorm here already.
int set_extra(strq_ctx* c, int32_t on, Pass p, int (*validate)(strq_ctx*, DetectState*) = nullptr,
              double Extras::* level = nullptr, double value = 0.0, bool level_ok = true, const char* level_bad = nullptr)
{
    if (on != 0 && on != 1) { c->err = std::string("bad argument (") + PASSES[p].entry + " takes 0 or 1)"; return STRQ_ERR_ARG; }
    if (on && !level_ok) { c->err = level_bad; return STRQ_ERR_ARG; }
    DetectState* d = dstate(c);
    if (on && p == PASS_RENORM && d->scan_on) { c->err = scan_refusal_text(p); return STRQ_ERR_ARG; }
    // sub-batches in flight keep the mode they were launched with: their pass (or none) runs now
    if (const int rc = drain(c, d)) return rc;
    if (on && validate) { if (const int rc = validate(c, d)) return rc; }
    d->extras.*PASSES[p].on = on != 0;
    if (level) d->extras.*level = on ? value : 0.0;
    return STRQ_OK;
}

// strq_last_<pass>: the pass's counters in the layout of its entry
int last_pass(strq_ctx* c, Pass p, double* out)
{
    if (!out) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    pass_stats_out(p, dstate(c)->stats[p], out);
    return STRQ_OK;
}

// strq_batch_fetch_<pass> begins: the sub-batches in flight are taken, and a batch that ran without the pass has nothing to fetch
int fetch_begin(strq_ctx* c, DetectState* d, Pass p)
{
    if (const int rc = drain(c, d)) return rc;
    if (!(d->batch.ran.*PASSES[p].on)) { c->err = ran_without_text(p); return STRQ_ERR_ARG; }
    return STRQ_OK;
}

// strq_batch_fetch_anchored / _tracts / _renorm: one record per read
template <class T>
int fetch_records(strq_ctx* c, Pass p, std::vector<T> ReadRows::* rows, T* out, int64_t n)
{
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, p)) return rc;
    const Batch& B = d->batch;
    if (n != B.n_reads || (n > 0 && !out) || (B.*rows).size() != (size_t)n) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (n) std::memcpy(out, (B.*rows).data(), (size_t)n * sizeof(T));
    return STRQ_OK;
}

// strq_detect_batch*: a plain detect whatever scan set the context holds (put back when the call is through)
struct PlainScope {
    DetectState* d; bool on;
    explicit PlainScope(DetectState* d_) : d(d_), on(d_->scan_on) { d->scan_on = false; }
    ~PlainScope() { d->scan_on = on; }
};

// strq_debug_variant_image / strq_debug_mod_llr_image: what an image built for a null device base holds, as plain numbers -- the
// pointers of its struct are then the byte offsets of the arrays
template <class Model>
int debug_image_out(int brc, const std::vector<char>& blob, const std::string& reason, int n_branch,
                    int32_t* build_rc, int32_t* head, int64_t* offsets, void* image, int64_t image_cap, int64_t* image_bytes, char* why, int32_t why_len)
{
    *build_rc = brc;
    if (why && why_len > 0) snprintf(why, (size_t)why_len, "%s", brc ? reason.c_str() : "");
    for (int i = 0; i < 10; ++i) head[i] = 0;
    for (int i = 0; i < 12; ++i) offsets[i] = 0;
    *image_bytes = 0;
    if (brc) return STRQ_OK;
    Model M; std::memcpy(&M, blob.data(), sizeof(M));
    head[0] = M.n_emit; head[1] = n_branch; head[2] = M.mode; head[3] = M.deg; head[4] = M.deg2;
    for (size_t i = 0; i < sizeof(M.end_deg) / sizeof(M.end_deg[0]); ++i) head[5 + i] = M.end_deg[i];
    const void* at[12] = {M.src, M.lp, M.src2, M.lp2, M.start_lp, M.kind, M.hub, M.ea, M.eb, M.ec, M.end_src, M.end_lp};
    for (int i = 0; i < 12; ++i) offsets[i] = (int64_t)reinterpret_cast<intptr_t>(at[i]);
    *image_bytes = (int64_t)blob.size();
    if (image && image_cap >= (int64_t)blob.size()) std::memcpy(image, blob.data(), blob.size());
    return STRQ_OK;
}

// strq_debug_variant_scores / strq_debug_mod_llr_scores: the reads with bounds as Read structs over buffers of the call's own, one
// launch, the scores back.  dev[r]: the device image of read r's model; nv doubles per bound.
template <class Read, class Model, class Launch>
int debug_scores(strq_ctx* c, int32_t n_reads, const std::vector<const Model*>& dev, int nv, const double* x, const int64_t* x_off,
                 const int32_t* w, const int64_t* w_off, double* out, Launch launch)
{
    hipStream_t st = c->stream;
    const int64_t nx = x_off[n_reads], nw = w_off[n_reads];
    if (!nw) return STRQ_OK;
    DevBuf b_x, b_w, b_out, b_rd, b_first;
    STRQ_HIP(c, b_x.reserve((size_t)nx * 8 + 64)); STRQ_HIP(c, b_w.reserve((size_t)nw * 4 + 64)); STRQ_HIP(c, b_out.reserve((size_t)nw * nv * 8 + 64));
    STRQ_HIP(c, b_rd.reserve((size_t)n_reads * sizeof(Read) + 64)); STRQ_HIP(c, b_first.reserve(((size_t)n_reads + 1) * 8 + 64));
    std::vector<Read> rdv; std::vector<int64_t> first, at;
    int64_t total = 0;
    for (int32_t r = 0; r < n_reads; ++r) {          // (a read without bounds takes no part, as in the pipeline)
        const int64_t k = w_off[r + 1] - w_off[r];
        if (!k) continue;
        Read rd; rd.model = dev[(size_t)r]; rd.x = b_x.as<double>() + x_off[r]; rd.w = b_w.as<int32_t>() + w_off[r];
        rd.out = b_out.as<double>() + (size_t)nv * (size_t)w_off[r]; rd.T = x_off[r + 1] - x_off[r];
        rdv.push_back(rd); first.push_back(total); total += k;
    }
    first.push_back(total);
    if (nx) STRQ_HIP(c, hipMemcpyAsync(b_x.p, x, (size_t)nx * 8, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(b_w.p, w, (size_t)nw * 4, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(b_rd.p, rdv.data(), rdv.size() * sizeof(Read), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(b_first.p, first.data(), first.size() * 8, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemsetAsync(b_out.p, 0, (size_t)nw * nv * 8, st));
    if (launch(st, b_rd.as<Read>(), b_first.as<int64_t>(), (int)rdv.size(), total)) { c->err = "score launch failed"; return STRQ_ERR_DEVICE; }
    STRQ_HIP(c, hipMemcpyAsync(out, b_out.p, (size_t)nw * nv * 8, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    return STRQ_OK;
}

// the arguments the two score hooks share
int debug_scores_args(strq_ctx* c, int32_t n_reads, const int32_t* model_id, const double* x, const int64_t* x_off, const int32_t* w,
                      const int64_t* w_off, double* out, int32_t* launched)
{
    const char* bad = "bad argument";
    if (n_reads < 1 || !model_id || !x_off || !w_off || !out || !launched || x_off[0] != 0 || w_off[0] != 0) { c->err = bad; return STRQ_ERR_ARG; }
    for (int32_t r = 0; r < n_reads; ++r) {
        if (x_off[r + 1] < x_off[r] || w_off[r + 1] < w_off[r]) { c->err = "bad argument (offsets must not decrease)"; return STRQ_ERR_ARG; }
        if (model_id[r] < 0 || model_id[r] >= (int32_t)c->models.size() || !c->models[(size_t)model_id[r]]) { c->err = "bad argument (no such model)"; return STRQ_ERR_ARG; }
    }
    if ((x_off[n_reads] > 0 && !x) || (w_off[n_reads] > 0 && !w)) { c->err = bad; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

}  // namespace

extern "C" {

int strq_set_pore_stats(strq_ctx* c, double tail_lo, double tail_hi, double model_min, double model_max)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (const int rc = drain(c, d)) return rc;          // a sub-batch in flight is taken with the statistics it ran with
    d->ps.M_lo = tail_lo; d->ps.M_hi = tail_hi; d->ps.clip_lo = model_min + .5; d->ps.clip_hi = model_max - .5;
    d->have_ps = true;
    return STRQ_OK;
}

int strq_target_add(strq_ctx* c, const float* prefix_ext, int64_t m_prefix, const float* suffix_ext, int64_t m_suffix,
                    int32_t trim_prefix, int32_t trim_suffix, int32_t samples, int32_t hmm_model_id, int32_t count_bias,
                    int32_t* target_id)
{
    STRQ_ENTER(c);
    if (!prefix_ext || !suffix_ext || !target_id || hmm_model_id < 0 || hmm_model_id >= (int32_t)c->models.size() ||
        trim_prefix < 0 || trim_suffix < 0 || trim_prefix >= m_prefix || trim_suffix >= m_suffix) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    DetectState* d = dstate(c);
    Target t;
    int rc = align_validate_flank(c, prefix_ext, m_prefix, samples, &t.kp, &t.Rp, &t.NSp); if (rc) return rc;
    rc = align_validate_flank(c, suffix_ext, m_suffix, samples, &t.ks, &t.Rs, &t.NSs); if (rc) return rc;
    t.prefix_ext.assign(prefix_ext, prefix_ext + m_prefix); t.suffix_ext.assign(suffix_ext, suffix_ext + m_suffix);
    t.trim_prefix = trim_prefix; t.trim_suffix = trim_suffix; t.samples = align_effective_samples(samples); t.model_id = hmm_model_id; t.count_bias = count_bias;
    d->targets.push_back(t);
    *target_id = (int32_t)d->targets.size() - 1;
    return STRQ_OK;
}

int strq_target_set_mod(strq_ctx* c, int32_t target_id, int32_t mod_model_id, double mod_min, double mod_max)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (target_id < 0 || target_id >= (int32_t)d->targets.size() || mod_model_id < 0 || mod_model_id >= (int32_t)c->models.size()) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (const int rc = drain(c, d)) return rc;          // a sub-batch in flight is taken with the target it ran with
    if (d->extras.llr) { if (const int rc = llr_model(c, c->models[mod_model_id])) return rc; }          // (the target stays as it was)
    d->targets[target_id].mod_model_id = mod_model_id; d->targets[target_id].mod_min = mod_min; d->targets[target_id].mod_max = mod_max;
    return STRQ_OK;
}

int strq_batch_fetch_mod(strq_ctx* c, char* pool, int64_t pool_cap, int64_t* off)
{
    STRQ_ENTER(c);
    if (!off) return STRQ_ERR_ARG;
    DetectState* d = dstate(c);
    if (const int rc = drain(c, d)) return rc;
    const std::vector<std::string>& mod = d->batch.mod;
    const int64_t n = (int64_t)mod.size();
    if (pack_ragged(n, off, pool != nullptr, pool_cap, [&](int64_t i) { return (int64_t)mod[(size_t)i].size(); },
                    [&](int64_t i, int64_t pos) { std::memcpy(pool + pos, mod[(size_t)i].data(), mod[(size_t)i].size()); }) < n) { c->err = "pattern pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_set_units(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_UNITS);
}

int strq_batch_fetch_units(strq_ctx* c, int64_t* pool, int64_t pool_cap, int64_t* off, int32_t* decoded)
{
    STRQ_ENTER(c);
    if (!off) return STRQ_ERR_ARG;
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, PASS_UNITS)) return rc;
    const Batch& B = d->batch;
    const int64_t n = (int64_t)B.units.size();
    const int64_t done = pack_ragged(n, off, pool != nullptr, pool_cap, [&](int64_t i) { return (int64_t)B.units[(size_t)i].size(); }, [&](int64_t i, int64_t pos) {
        const std::vector<int64_t>& u = B.units[(size_t)i];
        if (!u.empty()) std::memcpy(pool + pos, u.data(), u.size() * 8);
    });
    if (decoded) for (int64_t i = 0; i < done; ++i) decoded[i] = B.unit_dec[(size_t)i];          // (of the reads that fitted)
    if (done < n) { c->err = "unit pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_last_units(strq_ctx* c, double* out4)
{
    if (!c || !out4) return STRQ_ERR_ARG;          // (no way into the device and no message: the entry is older than STRQ_ENTER)
    return last_pass(c, PASS_UNITS, out4);
}

int strq_set_confidence(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_CONF);
}

int strq_batch_fetch_confidence(strq_ctx* c, double* out3, int32_t* decoded)
{
    STRQ_ENTER(c);
    if (!out3) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, PASS_CONF)) return rc;
    const Batch& B = d->batch;
    if (!B.conf.empty()) std::memcpy(out3, B.conf.data(), B.conf.size() * 8);
    if (decoded) for (size_t i = 0; i < B.conf_dec.size(); ++i) decoded[i] = B.conf_dec[i];
    return STRQ_OK;
}

int strq_last_confidence(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_CONF, out4);
}

int strq_set_mod_llr(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    // every modification model registered so far must be one the pass covers (later ones: strq_target_set_mod)
    return set_extra(c, on, PASS_LLR, [](strq_ctx* c, DetectState* d) -> int {
        for (const Target& t : d->targets)
            if (t.mod_model_id >= 0) { if (const int rc = llr_model(c, c->models[t.mod_model_id])) return rc; }
        return STRQ_OK;
    });
}

int strq_batch_fetch_mod_llr(strq_ctx* c, double* pool, int64_t pool_cap, int64_t* off)
{
    STRQ_ENTER(c);
    if (!off) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    DetectState* d = dstate(c);
    if (const int rc = drain(c, d)) return rc;
    const Batch& B = d->batch;
    if (pack_ragged(B.n_reads, off, pool != nullptr, pool_cap, [&](int64_t i) { return (int64_t)B.llr[(size_t)i].size() / 2; }, [&](int64_t i, int64_t pos) {
            const std::vector<double>& v = B.llr[(size_t)i];
            if (v.size() / 2) std::memcpy(pool + 2 * pos, v.data(), v.size() / 2 * 16);
        }) < B.n_reads) { c->err = "mod-llr pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_last_mod_llr(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_LLR, out4);
}

int strq_target_set_variants(strq_ctx* c, int32_t target_id, int32_t model_id, double lo, double hi, int32_t n_alt, int32_t context_units)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (target_id < 0 || target_id >= (int32_t)d->targets.size() || model_id < -1 || model_id >= (int32_t)c->models.size()) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (model_id >= 0 && (n_alt < 1 || n_alt > VAR_MAX_NB - 1 || context_units < 0 || !(lo < hi))) { c->err = "bad argument (strq_target_set_variants: 1 to 3 alt units, context_units >= 0, lo < hi)"; return STRQ_ERR_ARG; }
    if (const int rc = drain(c, d)) return rc;          // a sub-batch in flight is taken with the target it ran with
    if (model_id >= 0) { if (const int rc = variant_model(c, c->models[model_id], n_alt)) return rc; }          // (the target stays as it was)
    Target& t = d->targets[target_id];
    t.var_model_id = model_id; t.var_nalt = model_id < 0 ? 0 : n_alt; t.var_ctx = model_id < 0 ? 0 : context_units;
    t.var_lo = model_id < 0 ? 0 : lo; t.var_hi = model_id < 0 ? 0 : hi;
    return STRQ_OK;
}

int strq_set_variants(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_VAR);
}

int strq_batch_fetch_variants(strq_ctx* c, int32_t* count_v, int32_t* decoded, int64_t* off, int8_t* branch, int64_t* end, int64_t pass_cap,
                              double* vpool, int64_t* voff, int64_t v_cap, int64_t* v_total)
{
    STRQ_ENTER(c);
    if (!off) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, PASS_VAR)) return rc;
    const Batch& B = d->batch;
    const bool pools = branch || end || vpool || voff;
    if (pools && !(branch && end && vpool && voff)) { c->err = "bad argument (strq_batch_fetch_variants: all pools or none)"; return STRQ_ERR_ARG; }
    // two pools: the passages (branch, end and the offset of their scores), and the scores
    int64_t vtot = 0;
    const int64_t done = pack_ragged2(B.n_reads, off, nullptr, pools, pass_cap, v_cap, &vtot, [&](int64_t i, int64_t* n, int64_t* nv) {
        const VariantRow& r = B.var[(size_t)i];
        if (count_v) count_v[i] = r.count_v;
        if (decoded) decoded[i] = r.decoded;
        *n = (int64_t)r.branch.size(); *nv = (int64_t)r.V.size();
    }, [&](int64_t i, int64_t pos, int64_t vpos) {
        const VariantRow& r = B.var[(size_t)i];
        for (int64_t j = 0; j < (int64_t)r.branch.size(); ++j) {
            branch[pos + j] = r.branch[(size_t)j]; end[pos + j] = r.end[(size_t)j];
            voff[pos + j] = vpos + j * r.n_branch;
        }
        if (!r.V.empty()) std::memcpy(vpool + vpos, r.V.data(), r.V.size() * 8);
    });
    if (done < B.n_reads) { c->err = "variant pool too small"; return STRQ_ERR_ARG; }
    if (pools) voff[off[B.n_reads]] = vtot;
    if (v_total) *v_total = vtot;
    return STRQ_OK;
}

int strq_last_variants(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_VAR, out4);
}

int strq_target_set_anchored(strq_ctx* c, int32_t target_id, int32_t end_model_id, int32_t end_bias, int32_t start_model_id, int32_t start_bias)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    const int32_t nm = (int32_t)c->models.size();
    const bool none = end_model_id == -1 && start_model_id == -1;
    if (target_id < 0 || target_id >= (int32_t)d->targets.size() ||
        (!none && (end_model_id < 0 || end_model_id >= nm || start_model_id < 0 || start_model_id >= nm))) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (!none)
        for (int32_t id : {end_model_id, start_model_id})
            if (vit_shape_for(c->models[id]->h, VIT_MARK) < 0) { c->err = "anchored: model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
    if (const int rc = drain(c, d)) return rc;          // a sub-batch in flight is taken with the target it ran with
    Target& t = d->targets[target_id];
    t.end_model_id = end_model_id; t.start_model_id = start_model_id;
    t.end_bias = none ? 0 : end_bias; t.start_bias = none ? 0 : start_bias;
    return STRQ_OK;
}

int strq_set_anchored(strq_ctx* c, int32_t on, double min_score)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_ANCH, nullptr, &Extras::anch_min, min_score, min_score > 0.0, "anchored: min_score must be above 0");
}

int strq_batch_fetch_anchored(strq_ctx* c, strq_anchored* out, int64_t n)
{
    STRQ_ENTER(c);
    return fetch_records(c, PASS_ANCH, &ReadRows::anch, out, n);
}

int strq_last_anchored(strq_ctx* c, double* out8)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_ANCH, out8);
}

int strq_target_set_tracts(strq_ctx* c, int32_t target_id, int32_t model_id, int32_t n_tracts, const int32_t* bias)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (target_id < 0 || target_id >= (int32_t)d->targets.size()) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (model_id != -1) {
        if (model_id < 0 || model_id >= (int32_t)c->models.size() || !c->models[model_id] || !bias) { c->err = "bad argument"; return STRQ_ERR_ARG; }
        const HostModel* hm = c->models[model_id];
        if (!hm->h.tract_inc || hm->n_tracts < 1) { c->err = "tracts: the model has no tracts (strq_model_set_tracts)"; return STRQ_ERR_ARG; }
        if (n_tracts != hm->n_tracts) { c->err = "tracts: the model has another number of tracts"; return STRQ_ERR_ARG; }
        if (vit_shape_of(hm->h) < 0) { c->err = "tracts: model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
    }
    if (const int rc = drain(c, d)) return rc;          // a sub-batch in flight is taken with the target it ran with
    Target& t = d->targets[target_id];
    t.tract_model_id = model_id; t.n_tracts = model_id < 0 ? 0 : n_tracts;
    for (int j = 0; j < 3; ++j) t.tract_bias[j] = (model_id >= 0 && j < n_tracts) ? bias[j] : 0;
    return STRQ_OK;
}

int strq_set_tracts(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_TRACTS);
}

int strq_batch_fetch_tracts(strq_ctx* c, strq_tracts* out, int64_t n)
{
    STRQ_ENTER(c);
    return fetch_records(c, PASS_TRACTS, &ReadRows::tracts, out, n);
}

int strq_last_tracts(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_TRACTS, out4);
}

int strq_target_set_motifs(strq_ctx* c, int32_t target_id, int32_t n, const int32_t* loop_model_ids, const int32_t* flanked_model_ids, const int32_t* bias)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (target_id < 0 || target_id >= (int32_t)d->targets.size() || (n != 0 && (n < 2 || n > MOTIF_MAX_CAND || !loop_model_ids || !flanked_model_ids || !bias))) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    for (int32_t j = 0; j < n; ++j) {
        const int32_t l = loop_model_ids[j], f = flanked_model_ids[j];
        if (l < 0 || l >= (int32_t)c->models.size() || !c->models[l] || (j > 0 && (f < 0 || f >= (int32_t)c->models.size() || !c->models[f]))) { c->err = "bad argument (no such model)"; return STRQ_ERR_ARG; }
        if (const int rc = motif_model(c, c->models[l])) return rc;
        if (j > 0 && vit_shape_for(c->models[f]->h, VIT_COUNT) < 0) { c->err = "motifs: a candidate's flanked model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
    }
    if (const int rc = drain(c, d)) return rc;          // a sub-batch in flight is taken with the target it ran with
    Target& t = d->targets[target_id];
    t.n_motifs = n;
    for (int j = 0; j < MOTIF_MAX_CAND; ++j) {
        t.motif_loop[j] = j < n ? loop_model_ids[j] : -1; t.motif_flanked[j] = (j < n && j > 0) ? flanked_model_ids[j] : -1; t.motif_bias[j] = j < n ? bias[j] : 0;
    }
    return STRQ_OK;
}

int strq_set_motifs(strq_ctx* c, int32_t on, int32_t segment)
{
    STRQ_ENTER(c);
    if (on == 1 && (segment < MOTIF_SEG_MIN || segment > MOTIF_SEG_MAX)) {
        c->err = "motifs: the segment length must lie between " + std::to_string(MOTIF_SEG_MIN) + " and " + std::to_string(MOTIF_SEG_MAX); return STRQ_ERR_ARG;
    }
    if (const int rc = set_extra(c, on, PASS_MOTIFS)) return rc;
    dstate(c)->extras.motif_segment = on ? segment : 0;
    return STRQ_OK;
}

int strq_batch_fetch_motifs(strq_ctx* c, strq_motifs* out, int64_t n, int64_t* off, double* V, int32_t* winners, int64_t seg_cap)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, PASS_MOTIFS)) return rc;
    const Batch& B = d->batch;
    if (n != B.n_reads || !off || (n > 0 && !out) || B.motifs.size() != (size_t)n || (V == nullptr) != (winners == nullptr) || seg_cap < 0) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (n) std::memcpy(out, B.motifs.data(), (size_t)n * sizeof(strq_motifs));
    if (pack_ragged(n, off, V != nullptr, seg_cap, [&](int64_t i) { return (int64_t)B.motif_win[(size_t)i].size(); },
                    [&](int64_t i, int64_t pos) {
                        const std::vector<int32_t>& w = B.motif_win[(size_t)i]; const std::vector<double>& v = B.motif_V[(size_t)i];
                        const int K = B.motifs[(size_t)i].n_cand;
                        for (size_t s = 0; s < w.size(); ++s) {
                            winners[pos + (int64_t)s] = w[s];
                            for (int j = 0; j < MOTIF_MAX_CAND; ++j) V[MOTIF_MAX_CAND * (pos + (int64_t)s) + j] = j < K ? v[s * (size_t)K + (size_t)j] : 0.0;
                        }
                    }) < n) { c->err = "segment pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_last_motifs(strq_ctx* c, double* out5)
{
    STRQ_ENTER(c);
    if (const int rc = last_pass(c, PASS_MOTIFS, out5)) return rc;
    out5[4] = dstate(c)->stats[PASS_MOTIFS].v[MOTIF_DECODES];
    return STRQ_OK;
}

int strq_set_tract_positions(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_TPOS);
}

int strq_batch_fetch_tract_positions(strq_ctx* c, int32_t* pos_status, int64_t* off, int64_t* pool, int64_t pool_cap)
{
    STRQ_ENTER(c);
    if (!off) return STRQ_ERR_ARG;
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, PASS_TPOS)) return rc;
    const Batch& B = d->batch;
    const int64_t n = (int64_t)B.tpos.size();          // three entries per read
    const int64_t done = pack_ragged(n, off, pool != nullptr, pool_cap, [&](int64_t i) { return (int64_t)B.tpos[(size_t)i].size(); }, [&](int64_t i, int64_t pos) {
        const std::vector<int64_t>& u = B.tpos[(size_t)i];
        if (!u.empty()) std::memcpy(pool + pos, u.data(), u.size() * 8);
    });
    if (pos_status) for (int64_t i = 0; i < done / 3; ++i) pos_status[i] = B.tpos_status[(size_t)i];          // (of the reads that fitted)
    if (done < n) { c->err = "tract position pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_last_tract_positions(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_TPOS, out4);
}

int strq_set_state_stats(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_SSTATS);
}

int strq_batch_fetch_state_stats(strq_ctx* c, int64_t* off, int64_t* n_obs, double* sum, double* sumsq, int64_t cap, int32_t* status)
{
    STRQ_ENTER(c);
    if (!off || cap < 0) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    const bool pools = n_obs || sum || sumsq;
    if (pools && !(n_obs && sum && sumsq)) { c->err = "bad argument (strq_batch_fetch_state_stats: all pools or none)"; return STRQ_ERR_ARG; }
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, PASS_SSTATS)) return rc;
    const Batch& B = d->batch;
    const int64_t n = (int64_t)B.sst.size();
    const int64_t done = pack_ragged(n, off, pools, cap, [&](int64_t i) { return (int64_t)B.sst[(size_t)i].n.size(); }, [&](int64_t i, int64_t pos) {
        const ReadRows::StateStatsRow& r = B.sst[(size_t)i];
        if (r.n.empty()) return;
        std::memcpy(n_obs + pos, r.n.data(), r.n.size() * 8); std::memcpy(sum + pos, r.sum.data(), r.n.size() * 8); std::memcpy(sumsq + pos, r.sumsq.data(), r.n.size() * 8);
    });
    if (status) for (int64_t i = 0; i < done; ++i) status[i] = B.sst_status[(size_t)i];          // (of the reads that fitted)
    if (done < n) { c->err = "state statistics pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_last_state_stats(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_SSTATS, out4);
}

int strq_set_state_posteriors(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_SPOST);
}

int strq_batch_fetch_state_posteriors(strq_ctx* c, int64_t* off, double* w, double* wx, double* wxx, int64_t cap, double* log_lik, int32_t* status)
{
    STRQ_ENTER(c);
    if (!off || cap < 0) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    const bool pools = w || wx || wxx;
    if (pools && !(w && wx && wxx)) { c->err = "bad argument (strq_batch_fetch_state_posteriors: all pools or none)"; return STRQ_ERR_ARG; }
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, PASS_SPOST)) return rc;
    const Batch& B = d->batch;
    const int64_t n = (int64_t)B.spost.size();
    const int64_t done = pack_ragged(n, off, pools, cap, [&](int64_t i) { return (int64_t)B.spost[(size_t)i].w.size(); }, [&](int64_t i, int64_t pos) {
        const ReadRows::StatePostRow& r = B.spost[(size_t)i];
        if (r.w.empty()) return;
        std::memcpy(w + pos, r.w.data(), r.w.size() * 8); std::memcpy(wx + pos, r.wx.data(), r.w.size() * 8); std::memcpy(wxx + pos, r.wxx.data(), r.w.size() * 8);
    });
    for (int64_t i = 0; i < done; ++i) {          // (of the reads that fitted)
        if (log_lik) log_lik[i] = B.spost[(size_t)i].log_lik;
        if (status) status[i] = B.spost_status[(size_t)i];
    }
    if (done < n) { c->err = "state posteriors pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_last_state_posteriors(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_SPOST, out4);
}

int strq_target_set_flank_mod(strq_ctx* c, int32_t target_id, int32_t which, int32_t profile_model_id, int32_t flank_len,
                              const int32_t* column_of, int32_t n_groups, const int32_t* groups)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    auto model = [&](int32_t id) -> HostModel* { return id >= 0 && id < (int32_t)c->models.size() ? c->models[(size_t)id] : nullptr; };
    HostModel* hm = model(profile_model_id);
    if (target_id < 0 || target_id >= (int32_t)d->targets.size() || (which != 0 && which != 1) || !hm || flank_len < 1 || !column_of ||
        n_groups < 0 || (n_groups > 0 && !groups)) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (n_groups > FMOD_MAX_GROUPS) { c->err = "flank-mod: at most " + std::to_string(FMOD_MAX_GROUPS) + " CpG groups per flank"; return STRQ_ERR_UNSUPPORTED; }
    if (vit_shape_for(hm->h, VIT_BACKPTR) < 0) { c->err = "flank-mod: the flank profile model does not fit a compiled Viterbi kernel"; return STRQ_ERR_UNSUPPORTED; }
    if (const int rc = drain(c, d)) return rc;          // a sub-batch in flight is taken with the models it ran with
    Target::FlankMod fm;
    fm.model_id = profile_model_id; fm.len = flank_len;
    for (int32_t k = 0; k < n_groups; ++k) {
        const int32_t* g = groups + 6 * k;
        HostModel* sm = model(g[2]);
        if (!sm || g[0] < 0 || g[1] < g[0] || (g[3] != 0 && g[3] != 1)) { c->err = "bad argument (a group's columns, site model or flank)"; return STRQ_ERR_ARG; }
        if (const int rc = llr_model(c, sm)) return rc;
        fm.range.push_back({g[0], g[1]}); fm.site.push_back(g[2]);
        fm.info.push_back(g[3]); fm.info.push_back(g[4]); fm.info.push_back(g[5]);
    }
    fm.col = std::make_shared<DevBuf>();
    STRQ_HIP(c, fm.col->reserve((size_t)hm->silent_start * 4 + 64));
    STRQ_HIP(c, hipMemcpy(fm.col->p, column_of, (size_t)hm->silent_start * 4, hipMemcpyHostToDevice));
    d->targets[(size_t)target_id].fmod[which] = fm;
    return STRQ_OK;
}

int strq_set_flank_mod(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_FMOD);
}

int strq_batch_fetch_flank_mod(strq_ctx* c, int32_t* called, int64_t* off, strq_flank_mod_group* pool, int64_t pool_cap)
{
    STRQ_ENTER(c);
    if (!off) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, PASS_FMOD)) return rc;
    const Batch& B = d->batch;
    const int64_t done = pack_ragged(B.n_reads, off, pool != nullptr, pool_cap, [&](int64_t i) {
        if (called) called[i] = B.fmod_called[(size_t)i];
        return (int64_t)B.fmod[(size_t)i].size();
    }, [&](int64_t i, int64_t pos) {
        const std::vector<strq_flank_mod_group>& v = B.fmod[(size_t)i];
        if (!v.empty()) std::memcpy(pool + pos, v.data(), v.size() * sizeof(strq_flank_mod_group));
    });
    if (done < B.n_reads) { c->err = "flank-mod pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_last_flank_mod(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_FMOD, out4);
}

int strq_set_anchored_mod(strq_ctx* c, int32_t on)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_AMOD);
}

int strq_batch_fetch_anchored_mod(strq_ctx* c, int32_t* called, int64_t* off, char* chars, int64_t chars_cap, int64_t* voff, double* pool, int64_t pool_cap)
{
    STRQ_ENTER(c);
    if (!off || !voff) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    DetectState* d = dstate(c);
    if (const int rc = fetch_begin(c, d, PASS_AMOD)) return rc;
    const Batch& B = d->batch;
    const bool pools = chars || pool;
    if (pools && !(chars && pool)) { c->err = "bad argument (strq_batch_fetch_anchored_mod: both pools or none)"; return STRQ_ERR_ARG; }
    // two pools: the characters of the patterns and their pairs; a read without a call adds to neither
    const int64_t done = pack_ragged2(B.n_reads, off, voff, pools, chars_cap, pool_cap, nullptr, [&](int64_t i, int64_t* n, int64_t* nv) {
        if (called) called[i] = B.amod_called[(size_t)i];
        if (!B.amod_called[(size_t)i]) return;
        *n = (int64_t)B.amod[(size_t)i].size(); *nv = (int64_t)B.amod_llr[(size_t)i].size() / 2;
    }, [&](int64_t i, int64_t pos, int64_t vpos) {
        const std::string& p = B.amod[(size_t)i]; const std::vector<double>& v = B.amod_llr[(size_t)i];
        if (!B.amod_called[(size_t)i]) return;
        if (!p.empty()) std::memcpy(chars + pos, p.data(), p.size());
        if (v.size() / 2) std::memcpy(pool + 2 * vpos, v.data(), v.size() / 2 * 16);
    });
    if (done < B.n_reads) { c->err = "anchored-mod pool too small"; return STRQ_ERR_ARG; }
    return STRQ_OK;
}

int strq_last_anchored_mod(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_AMOD, out4);
}

int strq_target_set_renorm(strq_ctx* c, int32_t target_id, const int16_t* Q, int32_t q_out, const int32_t* A, const double* W,
                           double grid_lo, double grid_d, double grid_p)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (target_id < 0 || target_id >= (int32_t)d->targets.size()) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (const int rc = drain(c, d)) return rc;          // a sub-batch in flight is taken with the target it ran with
    // after the drain nothing on the device reads the tables the target had before: they are freed here
    auto drop_tables = [&]() {
        const RenormTable* old = d->targets[target_id].rn_dev;
        d->targets[target_id].rn_dev = nullptr;
        d->rn_tables.erase(std::remove_if(d->rn_tables.begin(), d->rn_tables.end(), [old](const std::unique_ptr<DevBuf>& b) { return old && b->p == (const void*)old; }),
                           d->rn_tables.end());
        if (d->rn_tables.empty()) d->rn_have_grid = false;
    };
    if (!Q) { drop_tables(); return STRQ_OK; }
    if (!A || !W || !(grid_d > 0.0) || !std::isfinite(grid_lo) || !std::isfinite(grid_d) || !std::isfinite(grid_p) || q_out < -32768 || q_out > 32767) {
        c->err = "bad argument (strq_target_set_renorm: tables, shares and a grid of positive bin width)"; return STRQ_ERR_ARG;
    }
    for (int w = 0; w < RN_NW; ++w) if (!(W[w] >= 0.0 && W[w] < 1.0)) { c->err = "bad argument (strq_target_set_renorm: shares inside [0, 1))"; return STRQ_ERR_ARG; }
    // the grid and the shares are the context's: while another target holds tables, a call with other ones is refused, not taken for both
    const bool others = d->rn_tables.size() > (d->targets[target_id].rn_dev ? 1u : 0u);
    if (d->rn_have_grid && others) {
        bool same = d->rn_grid.lo == grid_lo && d->rn_grid.d == grid_d && d->rn_grid.p == grid_p;
        for (int w = 0; w < RN_NW; ++w) same = same && d->rn_grid.w[w] == W[w];
        if (!same) { c->err = "renorm: grid or shares differ from those of the tables the context holds (strq_target_set_renorm)"; return STRQ_ERR_ARG; }
    }
    std::vector<RenormTable> img(1);
    RenormTable& t = img[0];
    for (int w = 0; w < RN_NW; ++w) {
        std::memcpy(t.q + (size_t)w * RN_Q_STRIDE, Q + (size_t)w * RN_GRID, RN_GRID * sizeof(int16_t));
        for (int k = RN_GRID; k < RN_Q_STRIDE; ++k) t.q[(size_t)w * RN_Q_STRIDE + k] = (int16_t)q_out;
    }
    std::memcpy(t.a, A, sizeof(t.a)); t.pad_ = 0;
    std::unique_ptr<DevBuf> buf(new DevBuf());
    STRQ_HIP(c, buf->reserve(sizeof(RenormTable)));
    STRQ_HIP(c, hipMemcpy(buf->p, &t, sizeof(RenormTable), hipMemcpyHostToDevice));
    drop_tables();
    d->targets[target_id].rn_dev = buf->as<RenormTable>();
    d->rn_tables.push_back(std::move(buf));
    d->rn_grid.lo = grid_lo; d->rn_grid.d = grid_d; d->rn_grid.p = grid_p;
    for (int w = 0; w < RN_NW; ++w) d->rn_grid.w[w] = W[w];
    d->rn_have_grid = true;
    return STRQ_OK;
}

int strq_set_renorm(strq_ctx* c, int32_t on, double min_share)
{
    STRQ_ENTER(c);
    return set_extra(c, on, PASS_RENORM, nullptr, &Extras::renorm_min, min_share, min_share > 0.0 && min_share < 1.0, "renorm: min_share must be inside (0, 1)");
}

int strq_batch_fetch_renorm(strq_ctx* c, strq_renorm* out, int64_t n)
{
    STRQ_ENTER(c);
    return fetch_records(c, PASS_RENORM, &ReadRows::renorm, out, n);
}

int strq_debug_renorm_fit(strq_ctx* c, int32_t target_id, const uint32_t* h3, strq_renorm* out)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (target_id < 0 || target_id >= (int32_t)d->targets.size() || !h3 || !out) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (!d->targets[target_id].rn_dev) { c->err = "renorm: target without tables (strq_target_set_renorm)"; return STRQ_ERR_ARG; }
    for (int k = 0; k < RN_SIGNALS * RN_GRID; ++k) if (h3[k] >> 31) { c->err = "bad argument (strq_debug_renorm_fit: a counter of 2^31 or more)"; return STRQ_ERR_ARG; }
    if (const int rc = drain(c, d)) return rc;
    Carve lay;
    const size_t o_h = lay.add<uint32_t>(RN_SIGNALS * RN_GRID), o_rr = lay.add<RenormRead>(1), o_rec = lay.add<strq_renorm>(1);
    DevBuf ws;
    STRQ_HIP(c, ws.reserve(lay.total()));
    const RenormRead rr = {d->targets[target_id].rn_dev, 1, 0};
    STRQ_HIP(c, hipMemcpyAsync(Carve::at<uint32_t>(ws.p, o_h), h3, RN_SIGNALS * RN_GRID * 4, hipMemcpyHostToDevice, c->stream));
    STRQ_HIP(c, hipMemcpyAsync(Carve::at<RenormRead>(ws.p, o_rr), &rr, sizeof(rr), hipMemcpyHostToDevice, c->stream));
    STRQ_HIP(c, hipMemsetAsync(Carve::at<strq_renorm>(ws.p, o_rec), 0, sizeof(strq_renorm), c->stream));
    if (launch_renorm_fit(c->stream, Carve::at<uint32_t>(ws.p, o_h), Carve::at<RenormRead>(ws.p, o_rr), 1, Carve::at<strq_renorm>(ws.p, o_rec))) { c->err = "renorm: launch failed"; return STRQ_ERR_DEVICE; }
    STRQ_HIP(c, hipMemcpyAsync(out, Carve::at<strq_renorm>(ws.p, o_rec), sizeof(strq_renorm), hipMemcpyDeviceToHost, c->stream));
    STRQ_HIP(c, hipStreamSynchronize(c->stream));
    return STRQ_OK;
}

int strq_last_renorm(strq_ctx* c, double* out4)
{
    STRQ_ENTER(c);
    return last_pass(c, PASS_RENORM, out4);
}

int strq_scan_set(strq_ctx* c, int32_t n_cand, const int32_t* cand_target_id, double min_score)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (const int rc = scan_check(c, d, n_cand, cand_target_id, min_score)) return rc;
    if (const int rc = drain(c, d)) return rc;          // sub-batches in flight are taken as what they were launched as
    d->scan_cand.assign(cand_target_id, cand_target_id + n_cand); d->scan_min = min_score; d->scan_on = true;
    return STRQ_OK;
}

int strq_scan_clear(strq_ctx* c)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (const int rc = drain(c, d)) return rc;
    d->scan_on = false; d->scan_cand.clear(); d->scan_min = 0;
    return STRQ_OK;
}

int strq_batch_fetch_scan(strq_ctx* c, int32_t* out_cand, double* out_scores)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (const int rc = drain(c, d)) return rc;
    return copy_scan(c, d, out_cand, out_scores);
}

int strq_scan_batch_reads(strq_ctx* c, int64_t n_reads, const void* const* reads, const int64_t* lengths, int32_t dtype,
                          int32_t n_cand, const int32_t* cand_target_id, double min_score,
                          strq_result* out_rows, int32_t* out_cand, double* out_scores)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (const int rc = scan_check(c, d, n_cand, cand_target_id, min_score)) return rc;
    if (n_reads < 0 || (n_reads > 0 && (!reads || !lengths || !out_rows || !out_cand))) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    std::vector<int64_t> off((size_t)n_reads + 1, 0);
    for (int64_t i = 0; i < n_reads; ++i) {
        if (lengths[i] < 0 || (lengths[i] > 0 && !reads[i])) { c->err = "bad argument"; return STRQ_ERR_ARG; }
        off[(size_t)i + 1] = off[(size_t)i] + lengths[i];
    }
    if (const int rc = drain(c, d)) return rc;
    // the scan set of the context (if any) is put back when the call is through
    const bool on0 = d->scan_on; const std::vector<int32_t> cand0 = d->scan_cand; const double min0 = d->scan_min;
    d->scan_cand.assign(cand_target_id, cand_target_id + n_cand); d->scan_min = min_score; d->scan_on = true;
    const std::vector<int32_t> tid((size_t)n_reads, cand_target_id[0]);      // every read's target until its winner is known
    int rc = batch_prepare(c, n_reads, nullptr, dtype, off.data(), tid.data(), nullptr, true, reads);
    if (!rc) rc = run_and_fetch(c, out_rows);
    if (!rc) rc = copy_scan(c, d, out_cand, out_scores);
    if (rc) { (void)upload_join(d); d->batch.forget_host(); }
    d->scan_on = on0; d->scan_cand = cand0; d->scan_min = min0;
    return rc;
}

int strq_batch_upload(strq_ctx* c, int64_t n_reads, const void* signals, int32_t dtype, const int64_t* offsets,
                      const int32_t* target_id, const double* host_stats)
{
    STRQ_ENTER(c);
    return batch_prepare(c, n_reads, signals, dtype, offsets, target_id, host_stats, false);
}

int strq_batch_upload_part(strq_ctx* c, int64_t total_reads, int64_t total_samples, int64_t first_read, int64_t n_reads,
                           const void* signals, int32_t dtype, const int64_t* offsets, const int32_t* target_id)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (total_reads < 0 || total_samples < 0 || first_read < 0 || n_reads < 0 || first_read + n_reads > total_reads || dtype != 0 ||
        (n_reads > 0 && (!signals || !offsets || !target_id))) { c->err = "bad argument (strq_batch_upload_part takes int16 reads)"; return STRQ_ERR_ARG; }
    if (!d->have_ps) { c->err = "strq_set_pore_stats has not been called"; return STRQ_ERR_ARG; }
    Batch& B = d->batch;
    if (first_read == 0) {
        // a new resident batch: device memory for all of it now, the parts follow in order
        if (const int rc = begin_batch(c, d, total_reads, dtype)) return rc;
        B.off.assign((size_t)total_reads + 1, 0); B.target.assign((size_t)total_reads, 0);
        STRQ_HIP(c, B.raw.reserve((size_t)total_samples * 2 + 64));      // total_samples is a hint: the buffer grows (below) when the parts hold more
    }
    if (B.n_reads != total_reads || d->part_reads != first_read) { c->err = "parts of a resident batch must follow each other, first_read = reads uploaded so far"; return STRQ_ERR_ARG; }
    if (n_reads == 0) return STRQ_OK;
    if (const int rc = check_reads(c, d, n_reads, offsets, target_id)) return rc;
    const int64_t base = B.off[(size_t)first_read];
    for (int64_t i = 0; i < n_reads; ++i) {
        B.off[(size_t)(first_read + i + 1)] = base + (offsets[i + 1] - offsets[0]);
        B.target[(size_t)(first_read + i)] = target_id[i];
        if (!B.target_given.empty()) B.target_given[(size_t)(first_read + i)] = target_id[i];
    }
    {
        const size_t need = (size_t)B.off[(size_t)(first_read + n_reads)] * 2 + 64;
        if (need > B.raw.cap) {          // more samples than announced: a larger buffer, the parts uploaded so far move over
            DevBuf bigger;
            STRQ_HIP(c, bigger.reserve(need + need / 2));
            if (base > 0) {
                const hipError_t e = hipMemcpy(bigger.p, B.raw.p, (size_t)base * 2, hipMemcpyDeviceToDevice);
                if (e != hipSuccess) { c->err = std::string("hipMemcpy (growing the resident batch): ") + hipGetErrorString(e); return STRQ_ERR_DEVICE; }
            }
            B.raw.swap(bigger);          // the old block goes with `bigger`
        }
    }
    for (int64_t i = first_read + n_reads; i < total_reads; ++i) B.off[(size_t)i + 1] = B.off[(size_t)(first_read + n_reads)];      // reads not yet uploaded: empty
    // the staging ring of upload_reads addresses the caller's buffer by the batch's own byte positions
    B.host_src = static_cast<const char*>(signals) + (size_t)offsets[0] * 2 - (size_t)base * 2;
    B.host_reads.clear(); B.uploaded = first_read; B.on_host = true;
    const int rc = upload_reads(c, d, first_read + n_reads);
    B.forget_host();
    if (rc) return rc;
    d->part_reads = first_read + n_reads;
    return STRQ_OK;
}

int strq_batch_run(strq_ctx* c)
{
    STRQ_ENTER(c);
    return run_range(c, dstate(c), 0, dstate(c)->batch.n_reads);
}

int strq_batch_run_range(strq_ctx* c, int64_t first, int64_t last)
{
    STRQ_ENTER(c);
    return run_range(c, dstate(c), first, last);
}

int strq_batch_fetch(strq_ctx* c, strq_result* out)
{
    STRQ_ENTER(c);
    if (!out) return STRQ_ERR_ARG;
    DetectState* d = dstate(c);
    if (const int rc = drain(c, d)) return rc;
    std::memcpy(out, d->batch.results.data(), d->batch.results.size() * sizeof(strq_result));
    return STRQ_OK;
}

// the stretches of the whole configured flanks: the row's prefix_end / suffix_begin and the ends before the trim
int strq_batch_fetch_flank_ranges(strq_ctx* c, int64_t* out4, int64_t n)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (const int rc = drain(c, d)) return rc;
    const Batch& B = d->batch;
    if (n != B.n_reads || (n > 0 && !out4) || B.flank_ends.size() != 2 * (size_t)n) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    for (int64_t r = 0; r < n; ++r) {
        const strq_result& o = B.results[(size_t)r];
        out4[4 * r] = B.flank_ends[2 * (size_t)r]; out4[4 * r + 1] = o.prefix_end; out4[4 * r + 2] = o.suffix_begin; out4[4 * r + 3] = B.flank_ends[2 * (size_t)r + 1];
    }
    return STRQ_OK;
}

int strq_batch_fetch_range(strq_ctx* c, int64_t first, int64_t last, strq_result* out)
{
    STRQ_ENTER(c);
    if (!out) return STRQ_ERR_ARG;
    DetectState* d = dstate(c);
    if (first < 0 || last < first || last > d->batch.n_reads) { c->err = "read range outside the uploaded batch"; return STRQ_ERR_ARG; }
    // only the sub-batches in flight that hold reads of the range are waited for (oldest first): a caller that runs range k + 1
    // before it fetches range k never waits for the Viterbi launches of k + 1
    for (int k = 0; k < 2; ++k) {
        DetectState::Slot& sl = d->slot[(d->next_slot + k) & 1];
        if (sl.state != DetectState::Slot::Idle && sl.r0 < last && sl.r0 + sl.nr > first) { const int rc = harvest(c, d, sl); if (rc) return rc; }
    }
    std::memcpy(out, d->batch.results.data() + first, (size_t)(last - first) * sizeof(strq_result));
    return STRQ_OK;
}

int strq_detect_batch(strq_ctx* c, int64_t n_reads, const void* signals, int32_t dtype, const int64_t* offsets,
                      const int32_t* target_id, const double* host_stats, strq_result* out)
{
    STRQ_ENTER(c);
    // signals stay in the caller's buffer and are uploaded one sub-batch ahead of the kernels
    if (const int rc = drain(c, dstate(c))) return rc;
    PlainScope plain_(dstate(c));
    if (const int rc = batch_prepare(c, n_reads, signals, dtype, offsets, target_id, host_stats, true)) return rc;
    return run_and_fetch(c, out);
}

int strq_detect_batch_reads(strq_ctx* c, int64_t n_reads, const void* const* reads, const int64_t* lengths, int32_t dtype,
                            const int32_t* target_id, const double* host_stats, strq_result* out)
{
    STRQ_ENTER(c);
    // one buffer per read (what a caller holding a list of arrays has): no concatenated copy on the host, the staging
    // threads gather straight from the reads
    if (n_reads < 0 || (n_reads > 0 && (!reads || !lengths))) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    std::vector<int64_t> off((size_t)n_reads + 1, 0);
    for (int64_t i = 0; i < n_reads; ++i) {
        if (lengths[i] < 0 || (lengths[i] > 0 && !reads[i])) { c->err = "bad argument"; return STRQ_ERR_ARG; }
        off[(size_t)i + 1] = off[(size_t)i] + lengths[i];
    }
    if (const int rc = drain(c, dstate(c))) return rc;
    PlainScope plain_(dstate(c));
    if (const int rc = batch_prepare(c, n_reads, nullptr, dtype, off.data(), target_id, host_stats, true, reads)) return rc;
    return run_and_fetch(c, out);
}

// conditioning outputs of the last sub-batch (parity tests of STRique.py:590-597): levels of read
// `read` (index inside the last sub-batch), its 256 level values and the scalars.
int strq_debug_conditioning(strq_ctx* c, int64_t read, uint8_t* levels, int64_t n, float* level_val, double* scalars10)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (const int drc = drain(c, d)) return drc;
    ReadCond rc;
    STRQ_HIP(c, hipMemcpy(&rc, d->rc.as<ReadCond>() + read, sizeof(rc), hipMemcpyDeviceToHost));
    if (levels) STRQ_HIP(c, hipMemcpy(levels, c->levels.as<uint8_t>() + d->levels_shift + rc.off, (size_t)std::min<int64_t>(n, rc.n), hipMemcpyDeviceToHost));
    if (level_val) STRQ_HIP(c, hipMemcpy(level_val, c->level_val.as<float>() + read * 256, 1024, hipMemcpyDeviceToHost));
    if (scalars10) {
        const double v[10] = {rc.med, rc.mad, rc.f_c1, rc.f_h1, rc.m_c1, rc.m_h1, rc.r_c1, rc.r_h1, rc.h2, rc.c2};
        std::memcpy(scalars10, v, sizeof(v));
    }
    return STRQ_OK;
}

// the median-filtered samples of read `read` of the last sub-batch, in the batch's element type: the slot's buffer outlives the
// sub-batch (it is reallocated only when a later sub-batch reserves it)
int strq_debug_filtered(strq_ctx* c, int64_t read, void* out, int64_t n)
{
    STRQ_ENTER(c);
    DetectState* d = dstate(c);
    if (const int drc = drain(c, d)) return drc;
    if (d->last_slot < 0 || read < 0 || read >= d->last_nr || n < 0 || (n > 0 && !out)) { c->err = "no such read in the last sub-batch"; return STRQ_ERR_ARG; }
    const size_t esz = d->batch.dtype == 0 ? 2 : 8;
    ReadCond rc;
    STRQ_HIP(c, hipMemcpy(&rc, d->rc.as<ReadCond>() + read, sizeof(rc), hipMemcpyDeviceToHost));
    const size_t count = (size_t)std::min<int64_t>(n, rc.n);
    if (count) STRQ_HIP(c, hipMemcpy(out, d->slot[d->last_slot].flt.as<char>() + d->flt_shift + (size_t)rc.off * esz, count * esz, hipMemcpyDeviceToHost));
    return STRQ_OK;
}

// the edge images of the variant pass and of the per-unit scores as plain arrays (host only): what the CPU tests interpret
int strq_debug_variant_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end, const int32_t* in_ptr, const int32_t* in_src,
                             const double* in_logp, const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                             const int32_t* state_tag, int32_t n_alt, int32_t* build_rc, int32_t* head, int64_t* offsets,
                             void* image, int64_t image_cap, int64_t* image_bytes, char* why, int32_t why_len)
{
    if (!in_ptr || !in_src || !in_logp || !emis_kind || !emis_a || !emis_b || !emis_c || !build_rc || !head || !offsets || !image_bytes ||
        n_states < 2 || silent_start < 0 || start < 0 || start >= n_states || end < 0 || end >= n_states) return STRQ_ERR_ARG;
    std::vector<char> blob; std::string reason; int32_t mode = -1;
    const int brc = var_build_image(n_states, silent_start, start, end, in_ptr, in_src, in_logp, emis_kind, emis_a, emis_b, emis_c, state_tag, n_alt,
                                    nullptr, blob, &mode, reason);
    return debug_image_out<VarModel>(brc, blob, reason, n_alt + 1, build_rc, head, offsets, image, image_cap, image_bytes, why, why_len);
}

int strq_debug_mod_llr_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end, const int32_t* in_ptr, const int32_t* in_src,
                             const double* in_logp, const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                             const int32_t* state_tag, int32_t* build_rc, int32_t* head, int64_t* offsets,
                             void* image, int64_t image_cap, int64_t* image_bytes, char* why, int32_t why_len)
{
    if (!in_ptr || !in_src || !in_logp || !emis_kind || !emis_a || !emis_b || !emis_c || !build_rc || !head || !offsets || !image_bytes ||
        n_states < 2 || silent_start < 0 || start < 0 || start >= n_states || end < 0 || end >= n_states) return STRQ_ERR_ARG;
    std::vector<char> blob; std::string reason; int32_t mode = -1;
    const int brc = llr_build_image(n_states, silent_start, start, end, in_ptr, in_src, in_logp, emis_kind, emis_a, emis_b, emis_c, state_tag,
                                    nullptr, blob, &mode, reason);
    return debug_image_out<LlrModel>(brc, blob, reason, 2, build_rc, head, offsets, image, image_cap, image_bytes, why, why_len);
}

// given passages / units through one launch of the score kernels
int strq_debug_variant_scores(strq_ctx* c, int32_t n_reads, const int32_t* model_id, int32_t n_alt, const double* x, const int64_t* x_off,
                              const int32_t* w, const int64_t* w_off, double* out, int32_t* launched)
{
    STRQ_ENTER(c);
    if (const int rc = debug_scores_args(c, n_reads, model_id, x, x_off, w, w_off, out, launched)) return rc;
    std::vector<const VarModel*> dev((size_t)n_reads);
    int mode = -1;
    for (int32_t r = 0; r < n_reads; ++r) {
        HostModel* hm = c->models[(size_t)model_id[r]];
        if (const int rc = variant_model(c, hm, n_alt, false)) return rc;
        if (mode >= 0 && hm->var_mode != mode) { c->err = "bad argument (the models of a call must share the kernel mode and the branches)"; return STRQ_ERR_ARG; }
        mode = hm->var_mode; dev[(size_t)r] = hm->var_dev;
    }
    launched[0] = mode; launched[1] = n_alt + 1;
    const int n_cu = c->n_cu;
    return debug_scores<VarRead, VarModel>(c, n_reads, dev, n_alt + 1, x, x_off, w, w_off, out,
        [=](hipStream_t st, const VarRead* rd, const int64_t* first, int n, int64_t total) { return launch_var_score(st, mode, n_alt + 1, rd, first, n, total, n_cu); });
}

int strq_debug_mod_llr_scores(strq_ctx* c, int32_t n_reads, const int32_t* model_id, const double* x, const int64_t* x_off,
                              const int32_t* w, const int64_t* w_off, double* out, int32_t* launched)
{
    STRQ_ENTER(c);
    if (const int rc = debug_scores_args(c, n_reads, model_id, x, x_off, w, w_off, out, launched)) return rc;
    std::vector<const LlrModel*> dev((size_t)n_reads);
    int mode = -1;
    for (int32_t r = 0; r < n_reads; ++r) {
        HostModel* hm = c->models[(size_t)model_id[r]];
        if (const int rc = llr_model(c, hm)) return rc;
        if (mode >= 0 && hm->llr_mode != mode) { c->err = "bad argument (the models of a call must share the kernel mode)"; return STRQ_ERR_ARG; }
        mode = hm->llr_mode; dev[(size_t)r] = hm->llr_dev;
    }
    launched[0] = mode; launched[1] = 2;
    const int n_cu = c->n_cu;
    return debug_scores<LlrRead, LlrModel>(c, n_reads, dev, 2, x, x_off, w, w_off, out,
        [=](hipStream_t st, const LlrRead* rd, const int64_t* first, int n, int64_t total) { return launch_llr_score(st, mode, rd, first, n, total, n_cu); });
}

// count pass and write pass of the variant bounds kernels, the tasks filled as run_variant_tail fills them
int strq_debug_variant_bounds(strq_ctx* c, int32_t model_id, int32_t n_alt, int32_t n_reads, const int64_t* off, const int32_t* path,
                              const uint64_t* rec, const uint32_t* last, const int32_t* status, const int32_t* cap, int32_t stride,
                              int32_t guard, int32_t* n, int32_t* bad, int32_t* w, int32_t* branch, int32_t* untouched)
{
    STRQ_ENTER(c);
    const char* bad_arg = "bad argument";
    if (model_id < 0 || model_id >= (int32_t)c->models.size() || !c->models[(size_t)model_id] || n_alt < 1 || n_alt > VAR_MAX_NB - 1 || n_reads < 1 ||
        !off || off[0] != 0 || (!path && (!rec || !last)) || !status || !cap || stride < 1 || guard < 0 || guard > stride || !n || !bad || !w || !branch || !untouched) {
        c->err = bad_arg; return STRQ_ERR_ARG;
    }
    HostModel* hm = c->models[(size_t)model_id];
    if (!hm->h.state_tag) { c->err = "bad argument (the model carries no state tags)"; return STRQ_ERR_ARG; }
    const bool hop = !path;
    for (int32_t r = 0; r < n_reads; ++r) {
        const int64_t T = off[r + 1] - off[r];
        if (T < 0 || T >= ((int64_t)1 << 30) || T / 3 + 1 > stride - guard || cap[r] < -1 || cap[r] > stride - guard) { c->err = "bad argument (a read's length or cap against the stride)"; return STRQ_ERR_ARG; }
        if (!hop) for (int64_t t = off[r]; t < off[r + 1]; ++t) if (path[t] < 0 || path[t] >= hm->silent_start) { c->err = "bad argument (a path state that does not emit)"; return STRQ_ERR_ARG; }
    }
    hipStream_t st = c->stream;
    const int64_t nT = off[n_reads];
    const size_t n_in = hop ? (size_t)nT + (size_t)n_reads : (size_t)nT, slots = (size_t)n_reads * (size_t)stride;
    DevBuf b_in, b_res, b_bt, b_n, b_bad, b_w;
    STRQ_HIP(c, b_in.reserve(n_in * (hop ? 8 : 4) + 64)); STRQ_HIP(c, b_res.reserve((size_t)n_reads * sizeof(VitResult) + 64));
    STRQ_HIP(c, b_bt.reserve((size_t)n_reads * sizeof(VarBoundTask) + 64)); STRQ_HIP(c, b_n.reserve((size_t)n_reads * 4 + 64));
    STRQ_HIP(c, b_bad.reserve((size_t)n_reads * 4 + 64)); STRQ_HIP(c, b_w.reserve(slots * 8 + 64));
    int32_t* d_n = b_n.as<int32_t>(); int32_t* d_bad = b_bad.as<int32_t>(); int32_t* d_w = b_w.as<int32_t>(); int32_t* d_br = d_w + slots;
    VarBoundTask* d_bt = b_bt.as<VarBoundTask>();
    std::vector<VitResult> res((size_t)n_reads); std::vector<VarBoundTask> bt((size_t)n_reads);
    for (int32_t r = 0; r < n_reads; ++r) {
        VitResult& v = res[(size_t)r]; std::memset(&v, 0, sizeof(v));
        v.status = status[r]; v.dbg[0] = hop ? last[r] : 0;
        bt[(size_t)r] = var_count_task(hop ? b_in.as<uint64_t>() + off[r] + r : nullptr, b_res.as<VitResult>() + r, hop ? nullptr : b_in.as<int32_t>() + off[r],
                                       hm->h.state_tag, d_n + r, d_bad + r, off[r + 1] - off[r], n_alt + 1);
    }
    auto bounds = [&]() -> int {
        STRQ_HIP(c, hipMemcpyAsync(d_bt, bt.data(), (size_t)n_reads * sizeof(VarBoundTask), hipMemcpyHostToDevice, st));
        if (launch_var_bounds(st, hop ? d_bt : nullptr, hop ? n_reads : 0, hop ? nullptr : d_bt, hop ? 0 : n_reads)) { c->err = "variants: bounds launch failed"; return STRQ_ERR_DEVICE; }
        return STRQ_OK;
    };
    if (n_in) STRQ_HIP(c, hipMemcpyAsync(b_in.p, hop ? static_cast<const void*>(rec) : static_cast<const void*>(path), n_in * (hop ? 8 : 4), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(b_res.p, res.data(), (size_t)n_reads * sizeof(VitResult), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemsetAsync(d_n, 0, (size_t)n_reads * 4, st));
    STRQ_HIP(c, hipMemsetAsync(d_bad, 0, (size_t)n_reads * 4, st));
    STRQ_HIP(c, hipMemsetAsync(d_w, 0x7F, slots * 8, st));
    if (const int rc = bounds()) return rc;
    std::vector<int32_t> bad1((size_t)n_reads), bad2((size_t)n_reads);
    STRQ_HIP(c, hipMemcpyAsync(n, d_n, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(bad1.data(), d_bad, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    // write pass: the count (or the caller's number) as the cap, bounds at the read's stride
    for (int32_t r = 0; r < n_reads; ++r) {
        VarBoundTask& b = bt[(size_t)r];
        if (cap[r] < 0 && (n[r] < 0 || n[r] > stride - guard)) { c->err = "variants: the count pass returned a count beyond what the read can hold"; return STRQ_ERR_DEVICE; }
        b.w = d_w + (size_t)r * (size_t)stride; b.branch = d_br + (size_t)r * (size_t)stride; b.cap = cap[r] >= 0 ? cap[r] : n[r];
    }
    STRQ_HIP(c, hipMemsetAsync(d_bad, 0, (size_t)n_reads * 4, st));
    if (const int rc = bounds()) return rc;
    STRQ_HIP(c, hipMemcpyAsync(w, d_w, slots * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(branch, d_br, slots * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(bad2.data(), d_bad, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    for (int32_t r = 0; r < n_reads; ++r) {
        bad[2 * r] = bad1[(size_t)r]; bad[2 * r + 1] = bad2[(size_t)r];
        int same = 1;
        for (int32_t k = bt[(size_t)r].cap; k < stride; ++k)
            if (w[(size_t)r * (size_t)stride + (size_t)k] != 0x7F7F7F7F || branch[(size_t)r * (size_t)stride + (size_t)k] != 0x7F7F7F7F) same = 0;
        untouched[r] = same;
    }
    return STRQ_OK;
}

// one launch of flank_mod_bounds_kernel over the caller's paths: one task per stretch, all of one model's column table
int strq_debug_flank_mod_bounds(strq_ctx* c, int32_t n_flanks, const int64_t* off, const int32_t* path, const int32_t* status,
                                int32_t n_emit, const int32_t* column_of, const int64_t* g_off, const int32_t* groups, int32_t* out)
{
    STRQ_ENTER(c);
    if (n_flanks < 1 || !off || off[0] != 0 || n_emit < 1 || !column_of || !g_off || g_off[0] != 0 || !out) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    for (int32_t f = 0; f < n_flanks; ++f) {
        const int64_t T = off[f + 1] - off[f], G = g_off[f + 1] - g_off[f];
        if (T < 0 || T >= ((int64_t)1 << 30) || (T > 0 && !path)) { c->err = "bad argument (a stretch's length)"; return STRQ_ERR_ARG; }
        if (G < 0 || G > FMOD_MAX_GROUPS || (G > 0 && !groups)) { c->err = "bad argument (at most " + std::to_string(FMOD_MAX_GROUPS) + " groups per flank)"; return STRQ_ERR_ARG; }
        for (int64_t t = off[f]; t < off[f + 1]; ++t) if (path[t] < 0 || path[t] >= n_emit) { c->err = "bad argument (a path state that does not emit)"; return STRQ_ERR_ARG; }
    }
    const int64_t nT = off[n_flanks], nG = g_off[n_flanks];
    if (!nG) return STRQ_OK;
    hipStream_t st = c->stream;
    Carve lay;
    const size_t o_path = lay.add<int32_t>((size_t)nT), o_col = lay.add<int32_t>((size_t)n_emit), o_st = lay.add<int32_t>((size_t)n_flanks),
                 o_g = lay.add<FlankGroupRange>((size_t)nG), o_out = lay.add<FlankGroupBounds>((size_t)nG), o_task = lay.add<FlankBoundTask>((size_t)n_flanks);
    DevBuf ws;
    STRQ_HIP(c, ws.reserve(lay.total() + 64));
    int32_t* d_path = Carve::at<int32_t>(ws.p, o_path); int32_t* d_col = Carve::at<int32_t>(ws.p, o_col); int32_t* d_st = Carve::at<int32_t>(ws.p, o_st);
    FlankGroupRange* d_g = Carve::at<FlankGroupRange>(ws.p, o_g); FlankGroupBounds* d_out = Carve::at<FlankGroupBounds>(ws.p, o_out);
    FlankBoundTask* d_task = Carve::at<FlankBoundTask>(ws.p, o_task);
    std::vector<FlankBoundTask> tasks((size_t)n_flanks);
    for (int32_t f = 0; f < n_flanks; ++f) {
        FlankBoundTask& t = tasks[(size_t)f];
        t.path = d_path + off[f]; t.vit_status = status ? d_st + f : nullptr; t.column_of = d_col;
        t.groups = d_g + g_off[f]; t.out = d_out + g_off[f];
        t.T = off[f + 1] - off[f]; t.n_emit = n_emit; t.n_groups = (int32_t)(g_off[f + 1] - g_off[f]);
    }
    if (nT) STRQ_HIP(c, hipMemcpyAsync(d_path, path, (size_t)nT * 4, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_col, column_of, (size_t)n_emit * 4, hipMemcpyHostToDevice, st));
    if (status) STRQ_HIP(c, hipMemcpyAsync(d_st, status, (size_t)n_flanks * 4, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_g, groups, (size_t)nG * sizeof(FlankGroupRange), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_task, tasks.data(), (size_t)n_flanks * sizeof(FlankBoundTask), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemsetAsync(d_out, 0x7F, (size_t)nG * sizeof(FlankGroupBounds), st));
    if (launch_flank_mod_bounds(st, d_task, n_flanks)) { c->err = "flank-mod: bounds launch failed"; return STRQ_ERR_DEVICE; }
    STRQ_HIP(c, hipMemcpyAsync(out, d_out, (size_t)nG * sizeof(FlankGroupBounds), hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    return STRQ_OK;
}

}  // extern "C"
