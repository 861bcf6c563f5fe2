/*
 * libstrique_hip -- C ABI of the MI355X (gfx950) implementation of STRique's per-read hot path.
 *
 * Plain C, caller-owned buffers, no torch / pybind types.  Every function returns 0 on success
 * or a STRQ_ERR_* code; strq_last_error(ctx) gives the message.  One ctx per process per GPU;
 * calls on one ctx are not re-entrant (the reference holds the GIL for the whole native call,
 * src/pyalign.cpp:59-61, and each worker process owns its own aligner, scripts/STRique.py:743-745).
 *
 * What each entry point replaces in giesselmann/STRique (file:line in the reference tree):
 *   strq_ctx_create / strq_ctx_destroy   pyseqan.align_raw()            src/pyalign.cpp:50
 *   strq_set_align_params / get          the 8 float properties         src/pyalign.cpp:51-58,
 *                                                                       src/align_raw.h:84-103
 *   strq_align_overlap                   align_raw.align_overlap(a, b)  src/pyalign.cpp:59-61,
 *                                                                       src/align_raw.h:106-158
 *   strq_model_create / strq_viterbi     pomegranate HiddenMarkovModel.bake()/.viterbi() as used
 *                                        at scripts/STRique.py:431,434,490,493
 *   strq_target_add / strq_detect_batch  repeatCounter.add_target / detect
 *                                                                       scripts/STRique.py:553-618
 */
#ifndef STRIQUE_HIP_H
#define STRIQUE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STRQ_OK 0
#define STRQ_ERR_ARG 1          /* bad argument */
#define STRQ_ERR_DEVICE 2       /* HIP runtime / no GPU */
#define STRQ_ERR_UNSUPPORTED 3  /* input outside what the kernels cover (documented per call) */
#define STRQ_ERR_NOMEM 4

typedef struct strq_ctx strq_ctx;

/* Version of this ABI (bumped on any signature change). */
int strq_abi_version(void);   /* currently 13 (13: strq_debug_filtered; 12: strq_batch_fetch_range, strq_last_overlap, two sub-batches in flight; 11: strq_set_option, strq_get_option, strq_batch_upload_part, strq_last_screen_mode; 10: strq_last_screen, strq_debug_screen_plan; 9: strq_last_viterbi_launches, strq_last_second_round, strq_inflate_backend, strq_inflate_many, strq_inflate_stats, strq_h5_locate, strq_vbz_chunks; 8: strq_model_set_positions; 5: strq_host_stats, host_stats of strq_detect_batch / strq_batch_upload optional; 6: strq_detect_batch_reads; 7: strq_last_geometry, strq_batch_run_range, strq_inflate_chunks) */

/* Create a context on HIP device `device_id`.  Fails (STRQ_ERR_DEVICE) when no GPU is present:
 * there is no CPU fallback in this library. */
int strq_ctx_create(int device_id, strq_ctx** out);
void strq_ctx_destroy(strq_ctx* ctx);
const char* strq_last_error(const strq_ctx* ctx);
/* hipDeviceSynchronize on the context's device (benchmark brackets). */
int strq_device_synchronize(strq_ctx* ctx);

/* Switches of the library (the experiment / A-B switches that used to be environment variables only, e.g. STRQ_NO_SCREEN,
 * STRQ_OVERLAP, STRQ_SEG; README "Switches"): per context when ctx != NULL, process-wide when ctx == NULL.  Every switch is read
 * in this order: context, process, environment variable of the same name.  value NULL removes the entry (back to the next level),
 * "" means "not set" whatever the lower levels say.  Keys start with "STRQ_".  No switch changes a result -- they choose between
 * kernels / plans that are all exact (the reference has no counterpart: scripts/STRique.py:904-914 exposes --t and --config only).
 * strq_get_option writes the effective value ("" when unset) to out[cap]. */
int strq_set_option(strq_ctx* ctx, const char* key, const char* value);
int strq_get_option(const strq_ctx* ctx, const char* key, char* out, int32_t cap);

/* Alignment parameters, order: open_h, ext_h, open_v, ext_v, dist_offset, dist_min.
 * Defaults after create are align_raw's own (src/align_raw.h:51-60): -2,-8,-2,-8, 8,-16;
 * STRique overrides them from its config (scripts/STRique.py:507-523). */
int strq_set_align_params(strq_ctx* ctx, const float params[6]);
int strq_get_align_params(const strq_ctx* ctx, float params[6]);

/*
 * Semi-global alignment of flank `b` (m samples, end to end) inside read `a` (n samples, free
 * ends) -- align_raw.align_overlap(a, b).
 *   score      best score (float32, as the reference returns it)
 *   a_idx[n]   view position of every element of a   (nullable)
 *   b_idx[m]   view position of every element of b   (nullable)
 *   rec[m]     compact per-flank-row record (nullable): (j << 1) | is_vertical, where for a
 *              diagonal step b[k] is aligned to a[j-1] and for a vertical step j samples of `a`
 *              precede b[k]
 *   j_end,j0   DP columns where the path ends / leaves the free top row (nullable)
 * Any float32 inputs are accepted, like the reference (src/pyalign.cpp:59-61).  What
 * repeatCounter.detect passes -- `a` with at most 256 distinct values (an 8-bit morphology signal) and `b`
 * made of runs of 6 equal samples, m <= 49152 (scripts/STRique.py:592-601,562-565) -- runs on the
 * LDS-table wavefront kernels; everything else on a generic kernel (one trace byte per cell in HBM like
 * the reference: (n + 1) x (m + 1) <= 1.7e10, at most 2e9 distinct (a, b) value pairs), same results.
 */
int strq_align_overlap(strq_ctx* ctx, const float* a, int64_t n, const float* b, int64_t m,
                       float* score, uint64_t* a_idx, uint64_t* b_idx,
                       int32_t* rec, int64_t* j_end, int64_t* j0);

/*
 * Batched form of the same alignment for 8-bit level signals (the throughput path).
 *   n_align            number of alignments
 *   levels             concatenated level streams (uint8), one per *read*
 *   read_off[n_reads+1]offsets of each read in `levels`
 *   level_val          n_reads x 256 float32: value of each level of each read
 *   align_read[n_align]read index of each alignment
 *   flank              concatenated flank templates (float32, runs of `samples` equal values)
 *   flank_off[n_align+1]
 *   samples            run length of the flank templates (6)
 * Outputs per alignment: score, j_end, j0 and rec (concatenated like `flank`).
 */
int strq_align_batch(strq_ctx* ctx, int64_t n_align, int64_t n_reads,
                     const uint8_t* levels, const int64_t* read_off, const float* level_val,
                     const int32_t* align_read, const float* flank, const int64_t* flank_off,
                     int32_t samples,
                     float* score, int64_t* j_end, int64_t* j0, int32_t* rec);

/*
 * Upload a "baked" profile HMM (what pomegranate's HiddenMarkovModel.bake(merge='All') leaves,
 * scripts/STRique.py:431,490): emitting states first, silent states after them in topological
 * order, in-edges in CSR form sorted by source.
 *   emis_kind  1 = Normal(mu, sigma):  a = mu, b = 1/(2 sigma^2), c = -log(sigma sqrt(2 pi))
 *              2 = Uniform(lo, hi):    a = lo, b = hi,            c = -log(hi - lo)
 *   count_inc  n_states ints (nullable): states whose visits along the best path are counted
 *              (the two dummy states of repeatHMM, scripts/STRique.py:374-378)
 *   state_tag  n_states ints (nullable): 1 = state belongs to the repeat section (flanked model,
 *              `'repeat' in name`, STRique.py:608) or to the modified branch (modification model,
 *              `'mod' in name`, STRique.py:497); 2 = hub state s0/e0 of the modification model
 *   hint_slot / hint_lane  n_states ints each (nullable): where to keep an emitting state on the
 *              wave -- states of one profile column type in one slot, lane = profile position -- so
 *              that the LDS reads of neighbouring lanes are contiguous.  Purely a performance hint:
 *              an invalid or missing hint falls back to an automatic placement, results are identical.
 * Models of up to 512 emitting and 256 silent states with at most 8 in-edges per state run on the wave-per-window
 * kernels; anything beyond, up to 4096 states, on a general (slower) kernel; larger ones return STRQ_ERR_UNSUPPORTED.
 */
int strq_model_create(strq_ctx* ctx, int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                      const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                      const int32_t* emis_kind, const double* emis_a, const double* emis_b,
                      const double* emis_c, const int32_t* count_inc, const int32_t* state_tag,
                      const int32_t* hint_slot, const int32_t* hint_lane, int32_t* model_id);

/*
 * Optional, after strq_model_create: where every emitting state of a profile-HMM chain sits along the chain --
 * kind[e] 0 for a match-type state, 1 for an insert-type state, pos[e] >= 0 its position (prefix profile, repeat unit,
 * the two dummy states at one position, suffix profile: scripts/STRique.py:236-300,313-354,401-417 laid end to end).
 * A model that is such a chain (every in-edge joins a position with itself or the one before, plus the two edges that close
 * the repeat loop) additionally gets a register-resident image: count / mark decodes then keep the value vector in VGPRs
 * and touch no LDS.  Purely a performance hint: results are identical; STRQ_ERR_UNSUPPORTED (strq_last_error says why)
 * when the model is not such a chain -- it stays valid and runs on its lane layout.
 */
int strq_model_set_positions(strq_ctx* ctx, int32_t model_id, const int32_t* kind, const int32_t* pos);

/*
 * HiddenMarkovModel.viterbi(x) (scripts/STRique.py:434,493).
 *   logp     log-probability of the best path (-inf and status 1 when there is none)
 *   counted  visits of count_inc states on that path
 *   path[T]  emitting state (index in the baked order) of every observation (nullable; asking
 *            for it makes the kernel write back-pointers)
 */
int strq_viterbi(strq_ctx* ctx, int32_t model_id, const double* x, int64_t T,
                 double* logp, int64_t* counted, int32_t* status, int32_t* path);
int strq_viterbi_batch(strq_ctx* ctx, int32_t model_id, int64_t n_seq, const double* x,
                       const int64_t* x_off, double* logp, int64_t* counted, int32_t* status,
                       int32_t* paths);

/*
 * HiddenMarkovModel.log_probability(x) -- the forward algorithm, a sum over all paths where strq_viterbi takes the best one --
 * and the spread of the visit count over those paths, for n_seq windows (x_off[n_seq + 1], at most 8192 windows).
 *   log_lik      log sum_paths P(path, x); never below strq_viterbi's logp but for rounding (-inf and status 1 without a path)
 *   visits_mean  E[v | x], v = observations a path emits from count_inc states (what `counted` is on the best path)
 *   visits_var   Var[v | x], clamped at 0 (NaN, like the mean, without a path)
 *   c0[n_seq]    nullable: the moments are accumulated about c0[i] -- pass the window's `counted`; they stay O(1) then, where
 *                moments about zero lose the variance of a count near 1000 to cancellation.  Any value gives the same
 *                mathematical result.
 * float64, one wave per window, deterministic: the same window gives the same bits whatever else is in the call.  Missing
 * observations (NaN) have probability 1 under every distribution, as in strq_viterbi.  Models on the wave-per-window kernels
 * (strq_model_create) whose counted states are emitting states; others return STRQ_ERR_UNSUPPORTED, strq_last_error says why.
 * No count bias is applied: raw visits.
 */
int strq_forward_batch(strq_ctx* ctx, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                       const int64_t* c0, double* log_lik, double* visits_mean, double* visits_var, int32_t* status);
/*
 * Optional, after strq_model_create: in_logp_sum[e] for every in-edge e of the arrays given there.  Where the baked graph holds
 * ONE edge for several parallel paths of the original graph (two spliced silent states between the same pair of states), in_logp
 * carries the largest of them -- all a best-path decode needs -- and in_logp_sum the log of their summed probability, which a sum
 * over paths needs; equal to in_logp everywhere else.  Only the forward pass reads it.  STRQ_ERR_ARG when an entry is below in_logp's.
 */
int strq_model_set_forward_logp(strq_ctx* ctx, int32_t model_id, const double* in_logp_sum);
/*
 * Tract decodes: compound models -- several repeat loops in a fixed order, hmm.CompoundRepeatModel -- count the visits of every loop
 * separately.  Optional, after strq_model_create: tract_of[n_states] is -1 or the tract 0 .. n_tracts - 1 (n_tracts 1 .. 3) whose
 * counter an emission of the state advances.  A state with a tract must be an emitting state with count_inc 1, otherwise
 * STRQ_ERR_ARG.  The per-state increments are a device array of the model's own (uint64: 1 << 21 j for tract j); state_tag and
 * count_inc keep their meaning, every other decode of the model is unchanged.  Waits for detect sub-batches in flight.
 */
int strq_model_set_tracts(strq_ctx* ctx, int32_t model_id, int32_t n_tracts, const int32_t* tract_of);
/*
 * The tract decode of n_seq float64 windows as they are given (x_off[n_seq + 1], at most 8192 windows, offsets must not decrease):
 * strq_viterbi's best path -- the same log-probability bits and tie-breaks, the count decode of the model's lane row or of the
 * general kernel with a 64-bit payload of three 21-bit counters -- with
 *   logp            log-probability of the best path (-inf without one)
 *   counts[3 i + j] emissions of the states of tract j on the best path of window i (0 beyond n_tracts, without a path, and
 *                   for a window that was not decoded); no bias applied
 *   status          0 ok, 1 no path, 2 a window of 2^21 observations or more: the counters could carry into each other, the
 *                   window is not decoded
 * Never the register-resident kernel (its image has one loop).  STRQ_ERR_ARG for a model without tracts.
 */
int strq_viterbi_tracts(strq_ctx* ctx, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                        double* logp, int64_t* counts, int32_t* status);
/*
 * strq_viterbi_tracts, plus where the counted emissions lie: the windows of status 0 are decoded once more with back-pointers (the
 * model's lane row or the general kernel), traced back, and the state path is scanned with one ballot per tract -- the kernels of
 * the tract-position pass (strq_set_tract_positions), in pieces of at most STRQ_TRACT_POS_WS_BYTES of back-pointers.
 *   pos_off[3 n_seq + 1]  tract j of window i is pool[pos_off[3 i + j] .. pos_off[3 i + j + 1]): counts[3 i + j] ascending
 *                         observation indices (0-based), empty without a path and for a window that was not traced
 *   status                as strq_viterbi_tracts, and 4: decoded, counts valid, but the window's back-pointers alone exceed the
 *                         budget -- not traced, no positions
 * logp, counts: as strq_viterbi_tracts, bit for bit.  pool may be NULL (pool_cap 0) to query the total in pos_off[3 n_seq];
 * STRQ_ERR_ARG for a pool that is too small (the observations of all windows always suffice).  STRQ_ERR_DEVICE when the
 * back-pointer decode of a window disagrees with its count decode.
 */
int strq_viterbi_tract_positions(strq_ctx* ctx, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                                 double* logp, int64_t* counts, int32_t* status, int64_t* pos_off, int64_t* pool, int64_t pool_cap);
/*
 * State statistics of the best path (strique_amd/state_stats.py states the rule): for n_seq float64 windows as they are given
 * (x_off[n_seq + 1] from 0, at most 8192 windows, offsets must not decrease) and every emitting state s < silent_start of the model,
 *   n_obs[i n_emit + s]  observations of window i that strq_viterbi's best path emits from s and that are numbers (a NaN is skipped)
 *   sum, sumsq           their sum and the sum of their squares: float64 from +0.0, one addition per observation in ascending
 *                        order, the square rounded before it is added -- defined to the bit
 * rows of n_emit = silent_start entries, row-major; a state the path never visits has 0, +0.0, +0.0.  The windows are decoded as by
 * strq_viterbi_batch (logp, counted: its bits), those with a path once more with back-pointers (the model's lane row or the general
 * kernel), traced back and summed by state_stats_kernel -- the kernels of the pass of strq_set_state_stats -- in pieces of at most
 * STRQ_STATE_STATS_WS_BYTES of back-pointers (default 8 GiB).
 *   status  0 ok, 1 no path (zero rows), 4: decoded, logp and counted valid, but the window's back-pointers alone exceed the
 *           budget -- not traced, zero rows
 * logp, counted, status are nullable.  Every model strq_model_create accepts.  STRQ_ERR_DEVICE when the back-pointer decode of a
 * window disagrees with its count decode in logp bits or counted.
 */
int strq_viterbi_state_stats(strq_ctx* ctx, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                             double* logp, int64_t* counted, int32_t* status, int64_t* n_obs, double* sum, double* sumsq);
/*
 * State posteriors, the soft counterpart of strq_viterbi_state_stats (strique_amd/state_posteriors.py states the rule): for n_seq
 * float64 windows as they are given (x_off[n_seq + 1] from 0, at most 8192 windows, offsets must not decrease) and every emitting
 * state s < silent_start of the model, with gamma_t(s) = P(the path emits x_t from s | x) over all start -> end paths (the transition
 * probabilities of the forward pass: strq_model_set_forward_logp),
 *   w[i n_emit + s]   sum of gamma_t(s) over the observations t of window i that are numbers (a NaN is skipped)
 *   wx, wxx           sum of gamma_t(s) x_t and of gamma_t(s) x_t^2 over the same t
 *   log_lik           log sum_paths P(path, x), the quantity strq_forward_batch reports (-inf without a path)
 * rows of n_emit = silent_start entries, row-major, float64.  Forward-backward in linear space, one wave per window
 * (posterior_kernels.hip): rescaled by a power of two after every time step (no interval switch; STRQ_FWD_RESCALE_EVERY is not
 * read), deterministic to the bit -- no atomics on values, no tree reduction, nothing depends on which windows share the call or on
 * how it was cut into pieces -- and not defined to the bit against a log-space restatement.  The forward half stores its scaled
 * vector of every time step: T * epl * 64 * 8 + 4 T bytes per window (epl = ceil(n_emit / 64)), in pieces of at most
 * STRQ_STATE_POST_WS_BYTES of them (default 8 GiB).
 *   status  0 ok, 1 no path (zero rows, log_lik -inf), 4: log_lik valid, but the window's stored vectors alone exceed the budget --
 *           no backward half, zero rows
 * log_lik, status are nullable.  Models with a forward kernel (see strq_forward_batch); others return STRQ_ERR_UNSUPPORTED.
 */
int strq_forward_state_stats(strq_ctx* ctx, int32_t model_id, int64_t n_seq, const double* x, const int64_t* x_off,
                             double* log_lik, int32_t* status, double* w, double* wx, double* wxx);
/* Test hook: the kernel shape id (as strq_debug_viterbi_plan gives it) of the context's last tract launch; -1 before the first. */
int strq_debug_tract_shape(const strq_ctx* ctx, int32_t* shape);
/*
 * The motif track (strique_amd/motifs.py states the rule): which of n_models = K candidate repeat units (2 to 4) each stretch of a
 * window is made of.  model_ids: the candidates' loop models -- models of strq_model_create with at most 64 emitting states, no
 * silent state besides start and end, at most 8 in-edges per emitting state from emitting states, and an end state every emitting
 * state reaches once with log-probability 0 (motifs.loop_arrays builds them); any other model returns STRQ_ERR_UNSUPPORTED.
 * n_seq float64 windows as they are given (x_off[n_seq + 1] from 0; every window holds at least one observation; NaN: missing).
 * A window of T observations has n_seg = max(1, T / segment) segments (32 <= segment <= 4096): segment s < n_seg - 1 covers
 * [s segment, (s + 1) segment), the last one runs to T.
 *   n_seg[i]            segments of window i; the pools below hold the segments of all windows in window order
 *   V[seg K + j]        the largest Viterbi value over the emitting states after the last observation of the segment under loop model
 *                       j, every segment decoded from the start state: float64, evaluated like strq_viterbi -- defined to the bit,
 *                       whatever windows share the call
 *   winners[seg]        the candidate with the largest V (the lowest index among equals)
 *   obs_won[4 i + j]    observations of the segments of window i that candidate j won (0 for j >= K)
 *   majority[i]         the candidate with the most observations won (the lowest index among equals)
 * seg_cap: segments the pools V (seg_cap * K doubles) and winners hold; STRQ_ERR_ARG when the windows have more.
 */
int strq_motif_track(strq_ctx* ctx, int32_t n_models, const int32_t* model_ids, int32_t segment, int64_t n_seq, const double* x, const int64_t* x_off,
                     int64_t seg_cap, double* V, int32_t* winners, int64_t* n_seg, int64_t* obs_won, int32_t* majority);

/*
 * ---- repeatCounter.add_target / detect (scripts/STRique.py:553-618) as one device pipeline ----
 *
 * strq_set_pore_stats   the four model-side constants of pore_model.normalize2model('minmax')
 *                       (STRique.py:154,157-158,123-126): medians of the k-mer means below the 1st /
 *                       above the 99th percentile, model_min, model_max.
 * strq_target_add       one strand of one target (the reference's target_classifier tuple,
 *                       STRique.py:560-576): the two full flank templates generate_signal(*_ext,
 *                       samples) as float32, trim_prefix = len(prefix_ext) - len(prefix) and
 *                       trim_suffix likewise (STRique.py:598-599), the flanked-repeat HMM uploaded
 *                       with strq_model_create and count_bias = flanking_count - repeat_offset
 *                       (STRique.py:374-378,412,437).  samples: the run length of the templates (6 is
 *                       what STRique ships; any value works, on slower kernel shapes).  A template of up
 *                       to 8192 k-mer classes (49152 samples at samples = 6: a flank of 8197 nt; the
 *                       bundled loci have 150 nt = 870 samples) -- longer ones return STRQ_ERR_UNSUPPORTED.
 * strq_detect_batch     detect() for n_reads reads.  signals: concatenated raw samples,
 *                       dtype 0 = int16 (fast5 DAC values), 1 = float64 (pA, as the reference's
 *                       unit tests feed them).  For int16 every order statistic of the conditioning
 *                       comes from exact histograms on the GPU and host_stats is ignored.  float64
 *                       reads have no histogram: their six scalars per read -- median and MAD of the
 *                       median-filtered signal, (c1, h1) of its minmax map and of the raw signal's
 *                       (STRique.py:142-143,152-160,590-592) -- come from a radix selection over the
 *                       samples and numpy's own summation tree on the GPU when host_stats is NULL
 *                       (cond_kernels.hip: f64_stats_kernel; bit-equal to np.median / np.mean /
 *                       np.percentile), or from the caller (six doubles per read, e.g. strq_host_stats).
 *                       A read with a NaN among its median-filtered samples is undefined (below) whatever
 *                       the caller's scalars say: the library looks at the samples for that itself.
 * A read whose normalisation is undefined (constant signal, empty percentile tails: numpy hands the
 * reference NaN medians there) gets status 1 and the n = 0 row the reference writes for it -- its
 * offset / ticks come from aligning an all-NaN signal, every cell scoring dist_min, which is what
 * align_overlap makes of it (src/align_raw.h:100); it never aborts the batch.
 */
typedef struct strq_result {
    int32_t count;          /* repeat count n (0 if the gate failed, STRique.py:602-603) */
    int32_t status;         /* 0 ok, 1 signal could not be normalised */
    double score_prefix, score_suffix, log_p;
    int64_t offset, ticks;  /* prefix_end, max(suffix_begin - prefix_end, 0) (STRique.py:616) */
    int64_t prefix_begin, prefix_end, suffix_begin, suffix_end;
} strq_result;

int strq_set_pore_stats(strq_ctx* ctx, double tail_lo, double tail_hi, double model_min, double model_max);
int strq_target_add(strq_ctx* ctx, const float* prefix_ext, int64_t m_prefix, const float* suffix_ext,
                    int64_t m_suffix, int32_t trim_prefix, int32_t trim_suffix, int32_t samples,
                    int32_t hmm_model_id, int32_t count_bias, int32_t* target_id);
/* Base-modification pass of a target (repeatModHMM, STRique.py:447-500,605-609): the dual
 * (unmodified | modified) repeat-unit model uploaded with strq_model_create and its emission range
 * min(model_mins), max(model_maxs).  Reads of such a target also get a modification pattern. */
int strq_target_set_mod(strq_ctx* ctx, int32_t target_id, int32_t mod_model_id, double mod_min, double mod_max);
/* Modification patterns of the last batch: pattern of read i is pool[off[i] .. off[i+1]) ('0'/'1'
 * per repeat unit, "-" when there is none).  pool may be NULL to query the total size in off[n]. */
int strq_batch_fetch_mod(strq_ctx* ctx, char* pool, int64_t pool_cap, int64_t* off);
/* Repeat-unit positions (flankedRepeatHMM.count_repeats' Viterbi path, STRique.py:374-378,433-441, which detect drops at :604):
 * with on = 1, later run calls (strq_batch_run*, strq_detect_batch*) also report, for every read whose gate passed and whose
 * flanked-model decode found a path, the raw-signal sample indices prefix_begin + t of the observations t of the window
 * [prefix_begin, suffix_end) that the best path -- the one whose count and log_p the row reports -- emits from a counted state
 * (repeatdummy1 / repeatdummy2): count - count_bias ascending positions, one per repeat unit.  Sub-batches still in flight keep
 * the mode they were launched with (the call waits for them).  Default 0. */
int strq_set_units(strq_ctx* ctx, int32_t on);
/* Unit positions of the last batch: read i's are pool[off[i] .. off[i+1]); decoded[i] (nullable) = 1 when the read was decoded,
 * 0 when not (gate failed, signal not normalised, no path: no positions, unlike a decoded read with none).  pool may be NULL to
 * query the total in off[n].  STRQ_ERR_ARG when the last run call ran with unit positions off. */
int strq_batch_fetch_units(strq_ctx* ctx, int64_t* pool, int64_t pool_cap, int64_t* off, int32_t* decoded);
/* The unit pass of the last run call: out[0] = ms on the GPU (all its sub-batches), out[1] = largest workspace of unit records /
 * back-pointers one piece of it used (bytes), out[2] = windows decoded, out[3] = positions. */
int strq_last_units(strq_ctx* ctx, double* out4);
/* Per-unit scores behind the hard mCpG calls (repeatModHMM.mod_repeats, STRique.py:492-500, keeps the argmax only): with on = 1,
 * later run calls also score every repeat unit of every modification pattern under both branches of the dual model.  With the
 * segmentation of the pattern's decode fixed, unit j covers the observations x[u_j .. w_j] of the clipped repeat stretch (the s0
 * emission in front of it, its branch emissions, the e0 emission behind it) and V_B(j), B in {base, mod}, is the Viterbi
 * log-probability (start to end, float64, evaluated edge by edge like the decode itself) of the dual model on them with every edge
 * removed that has an emitting state of the other branch at either end; -inf when that branch has no path.  The log-likelihood
 * ratio of unit j is V_mod(j) - V_base(j): >= 0 (up to rounding) where the pattern says '1', <= 0 where it says '0'.  Rows,
 * patterns, unit positions and confidence do not change.  Sub-batches still in flight keep the mode they were launched with (the
 * call waits for them).  Dual models of at most 128 emitting states whose only silent states are start and end (repeat units of up
 * to 31 nt at k = 6): STRQ_ERR_UNSUPPORTED, and the switch stays off, when a modification model registered with a target is not
 * such a model -- and from strq_target_set_mod, which then leaves the target alone, while the switch is on.  Default 0: no further
 * kernel runs and no further buffer is reserved. */
int strq_set_mod_llr(strq_ctx* ctx, int32_t on);
/* Scores of the last batch (STRique.py:492-500: one entry per character of the pattern string): the units of read i are
 * [off[i], off[i+1]), unit k of the batch has V_base = pool[2 k], V_mod = pool[2 k + 1]; pool_cap counts units.  A read has as many
 * units as its pattern has characters, none when the pattern is "-", when its target has no modification model or when the run
 * call ran with the switch off.  pool may be NULL to query the total in off[n]. */
int strq_batch_fetch_mod_llr(strq_ctx* ctx, double* pool, int64_t pool_cap, int64_t* off);
/* The scoring pass of the last run call (STRique.py:492-500 has no counterpart): out[0] = ms on the GPU (all its sub-batches),
 * out[1] = units scored, out[2] = reads with units, out[3] = kernels launched (bounds and scoring; 0 with the switch off). */
int strq_last_mod_llr(strq_ctx* ctx, double* out4);
/* Sequence variants of the repeat unit (interruptions; the reference has no counterpart): a variant model is a dual model with 2 to 4
 * branches over one pore model -- branch 0 the repeat unit, branch b >= 1 the k-mers around alt unit b (state tags: 0 base, 2 the hub
 * states s0 / e0, 1 / 3 / 4 alt branch 1 / 2 / 3; n_alt of them), decoded on the clipped repeat stretch the modification pass decodes
 * (clipped to [lo, hi]).  context_units = m: the units in front of an alt unit that its branch holds besides it, so a passage through
 * an alt branch stands for m + 1 units.  model_id = -1 takes the variant model away.  STRQ_ERR_UNSUPPORTED, and the target stays as
 * it was, for a model the pass does not cover: more than 128 emitting states, silent states besides start and end, tags that do not
 * describe exactly n_alt alt branches (a tag beyond them, or a branch without a state), no compiled Viterbi kernel -- never in the
 * middle of a batch.  A target may hold a modification model and a variant model. */
int strq_target_set_variants(strq_ctx* ctx, int32_t target_id, int32_t model_id, double lo, double hi, int32_t n_alt, int32_t context_units);
/* With on = 1, later run calls also decode the variant model of every read whose gate passed, whose flanked-model decode found a
 * path (in a window below 2^21 samples) and whose target has a variant model.  A passage is a maximal run of emissions of one branch
 * on the best path; passage j covers the observations x[u_j .. w_j] (the s0 emission in front of it, its branch emissions, the e0
 * emission behind it), and V_b(j), b in 0 .. n_alt, is the Viterbi log-probability (start to end, float64, evaluated edge by edge
 * like the decode itself) of the model on them with every edge removed that touches an emitting state of another branch; -inf
 * where a branch has no path.  A base passage scored under an alt branch is an (m + 1)-unit profile forced onto one unit of signal:
 * meaningful only as "very negative".  Rows, modification patterns and every other output do not change, with one exception: a
 * sub-batch that holds a read of a target with a variant model decodes with the packed marks of the modification pass, so a read of
 * it whose window has 2^21 samples or more keeps count 0 (as the sub-batch mates of a modification target do).  Sub-batches still in
 * flight keep the mode they were launched with (the call waits for them).  Default 0: no further kernel runs and no further buffer
 * is reserved. */
int strq_set_variants(strq_ctx* ctx, int32_t on);
/* Variants of the last batch.  Per read i: count_v[i] = units of its passages (1 per base passage, m + 1 per alt passage) + the
 * target's count_bias, decoded[i] = 1 when its variant model was decoded (else count_v[i] = 0 and the read has no passages).  The
 * passages of read i are [off[i], off[i+1]): branch[k] in 0 .. n_alt, end[k] = raw sample (index into the read) of the e0 emission
 * w_j -- observation t of the stretch is raw sample first + t, first = the first repeat emission of the flanked path, because the
 * repeat section of a flanked model cannot be re-entered -- and V of passage k at vpool[voff[k] .. voff[k + 1]) (n_alt + 1 doubles,
 * voff has off[n] + 1 entries).  pass_cap counts passages, v_cap doubles.  branch, end, vpool and voff may be NULL to query the
 * totals: off[n] passages, and v_total (nullable) doubles.  STRQ_ERR_ARG when the last run call ran with the switch off. */
int strq_batch_fetch_variants(strq_ctx* ctx, int32_t* count_v, int32_t* decoded, int64_t* off, int8_t* branch, int64_t* end, int64_t pass_cap,
                              double* vpool, int64_t* voff, int64_t v_cap, int64_t* v_total);
/* The variant pass of the last run call: out[0] = kernels launched (0 with the switch off: the count and the write pass of the bounds,
 * one scoring launch per kernel instance in use, and the traceback where the bounds come from traced paths), out[1] = passages,
 * out[2] = ms on the GPU (all its sub-batches: compaction, decode, bounds, scoring), out[3] = reads decoded. */
int strq_last_variants(strq_ctx* ctx, double* out4);
/* Count confidence: with on = 1, later run calls also run the forward pass (strq_forward_batch) over the window
 * [prefix_begin, suffix_end) of every read whose gate passed and whose flanked-model decode found a path -- the same observations,
 * normalised and clipped, that the decode saw, with c0 = the visits of the best path.  Rows, modification patterns and unit
 * positions do not change.  Sub-batches still in flight keep the mode they were launched with (the call waits for them).
 * Default 0: no further kernel runs and no further buffer is reserved. */
int strq_set_confidence(strq_ctx* ctx, int32_t on);
/* Confidence of the last batch: out3[3 i .. 3 i + 3) = log_lik, count_mean = count_bias + E[v | x], count_sd = sqrt(Var[v | x])
 * of read i; decoded[i] (nullable) = 1 when the read was decoded, 0 when not (its three values are NaN).  A decoded window
 * without a path in the forward pass (see forward_kernels.hip on range) reports -inf, NaN, NaN.  STRQ_ERR_ARG when the last
 * run call ran with confidence off. */
int strq_batch_fetch_confidence(strq_ctx* ctx, double* out3, int32_t* decoded);
/* The forward pass of the last run call: out[0] = ms on the GPU (all its sub-batches), out[1] = windows processed,
 * out[2] = of them, windows without a path, out[3] = largest rescale exponent of a window (|log2| of its likelihood). */
int strq_last_confidence(strq_ctx* ctx, double* out4);
int strq_detect_batch(strq_ctx* ctx, int64_t n_reads, const void* signals, int32_t dtype,
                      const int64_t* offsets, const int32_t* target_id, const double* host_stats,
                      strq_result* out);
/* The same with one buffer per read (reads[i]: lengths[i] samples of `dtype`) instead of one concatenated buffer:
 * a caller that holds a list of arrays -- repeatCounter.detect_batch, the `count` command -- does not have to copy
 * them together first. */
int strq_detect_batch_reads(strq_ctx* ctx, int64_t n_reads, const void* const* reads, const int64_t* lengths, int32_t dtype,
                            const int32_t* target_id, const double* host_stats, strq_result* out);
/* The same in three steps, so that a caller can keep the signals resident in HBM and time (or
 * repeat) the device work alone: upload = host -> HBM copy, run = all kernels, fetch = results. */
int strq_batch_upload(strq_ctx* ctx, int64_t n_reads, const void* signals, int32_t dtype,
                      const int64_t* offsets, const int32_t* target_id, const double* host_stats);
/* strq_batch_upload in parts, so that a caller never holds more than one part in host memory: the first call (first_read = 0)
 * sizes the resident batch for total_reads reads / total_samples int16 samples (a hint: the buffer grows when the parts hold
 * more), every call uploads n_reads reads (signals +
 * offsets[0 .. n_reads], offsets relative to `signals`) behind the ones before it (first_read = reads uploaded so far).  Reads not
 * yet uploaded are empty.  int16 only (dtype 0).  bench.py stages its resident batches with it (synthesise -> upload -> free). */
int strq_batch_upload_part(strq_ctx* ctx, int64_t total_reads, int64_t total_samples, int64_t first_read, int64_t n_reads,
                           const void* signals, int32_t dtype, const int64_t* offsets, const int32_t* target_id);
int strq_batch_run(strq_ctx* ctx);
/* Only reads [first, last) of the uploaded batch (several batches kept resident side by side: a benchmark that
 * times a different one every step); strq_batch_fetch still returns the rows of the whole upload.
 * The run calls work in sub-batches (16 reads per CU) and keep TWO of them in flight: the HMM Viterbi launches of a sub-batch
 * run on a second stream under the conditioning and flank alignments of the next (the reference's workers are independent in the
 * same way, scripts/STRique.py:743-746), and its rows are taken one sub-batch late.  A run call therefore returns with the
 * Viterbi launches of its LAST sub-batch still queued; every call that hands out rows waits for what it needs:
 * strq_batch_fetch / strq_batch_fetch_mod / strq_detect_batch* for everything, strq_batch_fetch_range for the sub-batches that
 * hold reads of [first, last) only -- so `run(k + 1); fetch_range(k)` never waits for k + 1.  The rows are the same whatever
 * the order (STRQ_SERIAL=1: everything on one stream, rows before the run call returns, as up to ABI 11). */
int strq_batch_run_range(strq_ctx* ctx, int64_t first, int64_t last);
int strq_batch_fetch(strq_ctx* ctx, strq_result* out);
/* Methylation calls for the CpG groups of the configured flanks (strique_amd/flank_mod.py states the rule).  One record per group
 * of a flank whose stretch exists: flank 0 prefix / 1 suffix as configured, pos the + strand position of the group's first C in the
 * configured string, status 0 scored, 1 no path, 2 edge, 3 skipped, 4 too long; begin / end the raw samples of u and w (-1 unless
 * scored), v_base / v_mod the two masked Viterbi log-probabilities (NaN unless scored; llr = v_mod - v_base). */
typedef struct {
    int32_t flank, pos, n_sites, n_columns, status, pad_;
    int64_t begin, end;
    double v_base, v_mod;
} strq_flank_mod_group;
/* The models of one flank of a target, `which` 0 prefix / 1 suffix AS THE STRAND OF THE TARGET READS IT: profile_model_id the flank
 * profile model (hmm.FlankProfileModel of the whole configured flank, flank_len bases; it must fit a Viterbi kernel with
 * back-pointers), column_of one entry per emitting state of it (-1: no column), and n_groups (0 .. 64) groups of six int32 each:
 * c0, c1 (profile columns, inclusive), the site model (hmm.SiteModModel, at most 128 emitting states: its edge image is built here),
 * and what the records report -- flank as configured, pos, n_sites.  Both flanks and a modification model (strq_target_set_mod) make
 * a target one whose reads are called. */
int strq_target_set_flank_mod(strq_ctx* ctx, int32_t target_id, int32_t which, int32_t profile_model_id, int32_t flank_len,
                              const int32_t* column_of, int32_t n_groups, const int32_t* groups);
/* on = 1: later run calls also call the CpG groups of the flanks of every read whose gate passed, that could be conditioned and whose
 * target has the models above -- the prefix flank on the raw samples [whole prefix begin, prefix_end), the suffix flank on
 * [suffix_begin, whole suffix end) (strq_batch_fetch_flank_ranges), where begin < end.  Segmentation in pieces of at most
 * STRQ_FLANK_MOD_WS_BYTES of back-pointers (default 8 GiB).  Rows and every other output are unchanged; refused by a scan. */
int strq_set_flank_mod(strq_ctx* ctx, int32_t on);
/* The records of the last batch, ragged: called[r] = 1 for a read that qualified, records off[r] .. off[r + 1] of `pool` (prefix
 * groups first, in flank order).  Two calls: pool = NULL measures (off is written), then with pool_cap >= off[n]. */
int strq_batch_fetch_flank_mod(strq_ctx* ctx, int32_t* called, int64_t* off, strq_flank_mod_group* pool, int64_t pool_cap);
/* The pass of the last run call: [0] GPU ms  [1] flank stretches decoded  [2] groups scored  [3] launches. */
int strq_last_flank_mod(strq_ctx* ctx, double* out4);
/* The stretches of the whole configured flanks of every read of the last batch, in raw samples: out4[4 r ..] = where flank row 0
 * of the prefix alignment sits, prefix_end, suffix_begin, where the last flank row of the suffix alignment sits -- the positions of
 * __detect_range__ (scripts/STRique.py:538-548) without pre_trim / post_trim.  The row's prefix_begin and suffix_end are taken
 * `trim` rows further in (STRique.py:598-599) and bound the inner 50 nt of a 150-nt flank; the flank methylation calls
 * (strique_amd/flank_mod.py) are defined on the whole flank.  Zeros for a read without a row.  n: the reads of the batch. */
int strq_batch_fetch_flank_ranges(strq_ctx* ctx, int64_t* out4, int64_t n);
int strq_batch_fetch_range(strq_ctx* ctx, int64_t first, int64_t last, strq_result* out);
/* ---- scan: which target and strand a read spans, from its signal alone (no counterpart in the reference, which takes both from a
 * SAM record: scripts/STRique.py:673-679,689-692) ----
 * A candidate is a target id of strq_target_add: one strand of one target.  Every read is uploaded and conditioned once and aligned
 * against both flanks of every candidate; for candidate c the six values score_prefix, score_suffix, prefix_begin, prefix_end,
 * suffix_begin, suffix_end are exactly those of strq_detect_batch for (read, c).  With key_c = min(score_prefix, score_suffix),
 * c is eligible when prefix_begin < suffix_end and key_c >= min_score (min_score > 0); the eligible candidate with the largest key
 * wins, the lowest position in the list on a tie.  Only the winner's window is decoded: the read's row is the row strq_detect_batch
 * gives for (read, winner), field for field.  A read without a winner (none eligible, or status 1) has out_cand -1 and a row that is
 * zero but for its status.  One winner per read.
 * out_cand[i]: the winner of read i as a position in cand_target_id.  out_scores (nullable): n_reads x n_cand x 2 doubles,
 * score_prefix and score_suffix of every candidate.  STRQ_ERR_ARG: n_cand < 1 (or > 256), an unknown target id, min_score <= 0.
 * strq_batch_fetch_mod / strq_batch_fetch_units after a scan refer to the winners. */
int strq_scan_batch_reads(strq_ctx* ctx, int64_t n_reads, const void* const* reads, const int64_t* lengths, int32_t dtype,
                          int32_t n_cand, const int32_t* cand_target_id, double min_score,
                          strq_result* out_rows, int32_t* out_cand, double* out_scores);
/* The resident form: after strq_scan_set the run calls (strq_batch_run, strq_batch_run_range) scan the uploaded reads for these
 * candidates (the target ids given at upload are not used, and are in force again after strq_scan_clear); strq_batch_fetch* hand
 * out the winners' rows, strq_batch_fetch_scan the winners and scores (out_scores nullable) of the whole upload -- like the rows, those
 * of a read are the ones of the last scan run call that covered it (-1 and zeros when none has since the upload or since the
 * candidate count changed).  Sub-batches in flight are taken first by both calls.  strq_detect_batch* stay plain
 * detects whatever is set here. */
int strq_scan_set(strq_ctx* ctx, int32_t n_cand, const int32_t* cand_target_id, double min_score);
int strq_scan_clear(strq_ctx* ctx);
int strq_batch_fetch_scan(strq_ctx* ctx, int32_t* out_cand, double* out_scores);
/* ---- anchored counting: reads that end or start inside the repeat (no counterpart in the reference, whose gate, STRique.py:602,
 * sends such a read to the flanked model between one flank and a position that means nothing) ----
 * A read that could be conditioned (status 0, n > 0 samples) is, with m = min_score and the scores / positions of its row:
 *   kind 1 spanning           score_prefix >= m, score_suffix >= m and prefix_begin < suffix_end
 *   kind 2 ends in repeat     score_prefix >= m and score_suffix <  m      window [prefix_begin, n)
 *   kind 3 starts in repeat   score_suffix >= m and score_prefix <  m      window [0, suffix_end)
 *   kind 0 none               everything else (a NaN score; both flanks at m or above in the wrong order)
 * (strique_amd/anchored.py states the same rule).  A read of kind 2 / 3 is decoded once more, on its window of the filtered signal,
 * with the target's end / start model: the flanked model with the missing flank profile replaced by one free emitting state
 * (strq_model_create; counted states and tag 1 on the repeat section as in the flanked model).  count = visits of the counted states
 * + the model's bias; it is a lower bound on the allele up to the decode's own error, not a proven one.  free_samples, the
 * observations the free state emitted, is the check on the classification: a handful on a read that really ends in the repeat,
 * thousands on one that does not. */
typedef struct strq_anchored {
    int32_t kind;           /* 0 none, 1 spanning, 2 ends in repeat, 3 starts in repeat */
    int32_t status;         /* kind 2 / 3: 0 decoded, 1 no path, 2 window of 2^21 samples or more (then the fields below are zero) */
    int32_t count, pad_;
    double log_p;
    int64_t begin, end;     /* raw-signal samples [begin, end) the best path decodes into the repeat section */
    int64_t free_samples;
} strq_anchored;
/* The two models of a target and their biases.  Both or none: a model id of -1 in both places takes them away. */
int strq_target_set_anchored(strq_ctx* ctx, int32_t target_id, int32_t end_model_id, int32_t end_bias, int32_t start_model_id, int32_t start_bias);
/* on = 1: later run calls classify every read and decode those of kind 2 / 3 behind the rows (which do not change, nor do the
 * other optional outputs).  STRQ_ERR_ARG for min_score not above 0 (it has no default: the scores of a flank that is there and of
 * one that is not overlap on noisy reads).  A run call with the switch on fails before any launch (STRQ_ERR_ARG) when a read's
 * target has no anchored models, and when it is a scan.  Sub-batches still in flight keep the mode they were launched with (the
 * call waits for them).  Default 0: no further kernel runs and no further buffer is reserved. */
int strq_set_anchored(strq_ctx* ctx, int32_t on, double min_score);
/* One record per read of the last batch (n = its reads).  STRQ_ERR_ARG when the last run call ran with the switch off. */
int strq_batch_fetch_anchored(strq_ctx* ctx, strq_anchored* out, int64_t n);
/* The anchored pass of the last run call: out[0] = ms on the GPU (all its sub-batches), out[1 .. 4] = reads of kind 0, 1, 2, 3,
 * out[5] = kernels launched (classification, tasks, sorts and decodes; 0 with the switch off), out[6] / out[7] = of the decodes,
 * windows that ran on the register-resident / on a lane-layout kernel shape.  After a run call that failed inside the pass the
 * figures are those of the part that ran (the rows of the failed sub-batch are back at their initial values). */
int strq_last_anchored(strq_ctx* ctx, double* out8);
/* Methylation calls of anchored reads (repeatModHMM.mod_repeats, STRique.py:492-500, on the stretch detect step 13,
 * STRique.py:605-609, would hand it -- the reference itself calls spanning reads only).  With on = 1, a read gets a call when
 *   its anchored record has kind 2 or 3 and status 0, begin < end (which status 0 implies), and its target has a modification model
 *   (strq_target_set_mod);
 * with nrm = normalize2model(raw, 'minmax') of the RAW signal, as the modification pass of a spanning read takes it,
 *   pattern = mod_repeats(mod_model, [mod_min, mod_max], nrm[begin:end]): one character per unit the best path of the dual model
 *   passes ('0' / '1'), "-" when that decode has no path;
 * and, with strq_set_mod_llr on, (V_base(j), V_mod(j)) per character, defined on this stretch exactly as strq_set_mod_llr defines
 * them on the stretch of a spanning read.  Spanning reads (their row has the pattern), kinds 0 / 1, records of status 1 / 2 and
 * targets without a modification model get nothing.  The number of characters is not tied to the record's count.  Rows, records
 * and every other output do not change.  A run call with the switch on fails before any launch (STRQ_ERR_ARG) when anchored
 * counting is off, and when it is a scan.  Sub-batches still in flight keep the mode they were launched with (the call waits for
 * them).  Default 0: no further kernel runs and no further buffer is reserved. */
int strq_set_anchored_mod(strq_ctx* ctx, int32_t on);
/* Calls of the last batch, in two calls like the other variable-length outputs: with chars = pool = NULL the lengths -- called[i]
 * (nullable) = 1 when read i has a call, its characters are [off[i], off[i+1]), its units [voff[i], voff[i+1]) (none unless the run
 * call also ran with strq_set_mod_llr; else as many as characters, none for "-"), totals in off[n] and voff[n]; then the
 * characters in chars (chars_cap bytes) and V_base = pool[2 k], V_mod = pool[2 k + 1] of unit k (pool_cap counts units).
 * STRQ_ERR_ARG when the last run call ran with the switch off. */
int strq_batch_fetch_anchored_mod(strq_ctx* ctx, int32_t* called, int64_t* off, char* chars, int64_t chars_cap, int64_t* voff, double* pool, int64_t pool_cap);
/* The calls of the last run call: out[0] = ms on the GPU (all its sub-batches: tasks, compaction, decode, patterns, scores),
 * out[1] = reads called, out[2] = units (characters '0' / '1'), out[3] = kernels launched (0 with the switch off). */
int strq_last_anchored_mod(strq_ctx* ctx, double* out4);
/* ---- tracts: per-tract unit counts for compound repeat loci (no counterpart in the reference, whose flankedRepeatHMM,
 * STRique.py:384-431, has one repeat loop) ----
 * A target may hold a compound model beside its flanked one: K = 2 or 3 repeat loops in a fixed order with profiles between them
 * (strq_model_create + strq_model_set_tracts; strique_amd/tracts.py states the rule).  With the switch on, every read whose gate
 * passed, that could be normalised, whose flanked decode found a path and whose target has a compound model is decoded once more on
 * the window of the count decode -- [prefix_begin, suffix_end) of the filtered signal under the read's conditioning record -- with
 * the tract decode of strq_viterbi_tracts: count[j] = emissions of the counted states of tract j on the best path + bias[j], in model
 * order; log_p the log-probability of that path.  Limits: K <= 3, windows below 2^21 samples, tracts in a fixed order, every tract
 * at least bias[j] + 1 units long (each loop is passed once), one compound model per target, no anchored reads, no scan. */
typedef struct strq_tracts {
    int32_t status;         /* 0 decoded, 1 not decoded (gate failed, read not normalised, no path in the flanked decode, target without
                             * tracts), 2 window of 2^21 samples or more, 3 no path in the compound model; 1 .. 3: the fields below are zero */
    int32_t n_tracts;
    int32_t count[3];       /* model order, bias applied; zero beyond n_tracts */
    int32_t pad_;
    double log_p;
} strq_tracts;
/* The compound model of a target and the biases of its tracts (bias[j] read for j < n_tracts).  model_id = -1 takes it away.
 * STRQ_ERR_ARG for a model without tracts or with another number of them (strq_model_set_tracts), STRQ_ERR_UNSUPPORTED for a model
 * no compiled Viterbi kernel takes; the target stays as it was.  Never in the middle of a batch: sub-batches in flight are taken first. */
int strq_target_set_tracts(strq_ctx* ctx, int32_t target_id, int32_t model_id, int32_t n_tracts, const int32_t bias[3]);
/* on = 1: later run calls run the tract pass behind the rows, where the forward pass of strq_set_confidence runs: a task kernel writes
 * the windows on the device, one decode launch per kernel instance in use.  Rows and every other output do not change.  A run call
 * with the switch on fails before any launch (STRQ_ERR_ARG) when it is a scan.  Sub-batches still in flight keep the mode they were
 * launched with (the call waits for them).  Default 0: no further kernel runs and no further buffer is reserved. */
int strq_set_tracts(strq_ctx* ctx, int32_t on);
/* One record per read of the last batch (n = its reads).  STRQ_ERR_ARG when the last run call ran with the switch off. */
int strq_batch_fetch_tracts(strq_ctx* ctx, strq_tracts* out, int64_t n);
/* The tract pass of the last run call: out[0] = ms on the GPU (all its sub-batches), out[1] = windows decoded (status 0),
 * out[2] = kernels launched (tasks, sorts and decodes; 0 with the switch off), out[3] = windows with status 2 or 3. */
int strq_last_tracts(strq_ctx* ctx, double* out4);
/* Where the units of every tract lie (strique_amd/tracts.py states the rule).  on = 1: later run calls, behind the tract pass and once
 * its records are on the host, decode every window of tract status 0 once more with back-pointers (its task as the tract pass wrote
 * it, (T + 1) * n_states * 2 bytes), trace it back and scan the state path with one ballot per tract.  Position prefix_begin + t
 * belongs to tract j when the best path emits observation t from a counted state of loop j; per tract the positions ascend and there
 * are count[j] - bias[j] of them.  Pieces of at most STRQ_TRACT_POS_WS_BYTES of back-pointers (default 8 GiB), one read-back and one
 * wait per piece; a window whose back-pointers alone exceed the budget is not traced (pos_status 2, its counts stay).  A run call
 * with the switch on fails before any launch: STRQ_ERR_ARG without strq_set_tracts or in a scan, STRQ_ERR_UNSUPPORTED when a
 * target's compound model has no back-pointer decode.  STRQ_ERR_DEVICE when the back-pointer decode of a window disagrees with its
 * count decode.  Rows, tract records and every other output do not change.  Sub-batches still in flight keep the mode they were
 * launched with (the call waits for them).  Default 0: no further kernel runs and no further buffer is reserved. */
int strq_set_tract_positions(strq_ctx* ctx, int32_t on);
/* Tract positions of the last batch of n reads, ragged: off[3 n + 1], tract j of read i is pool[off[3 i + j] .. off[3 i + j + 1]) in
 * model order (raw-signal sample indices); pos_status[i] (nullable): 0 positions, 1 none (the tract record's status is not 0),
 * 2 back-pointers over the budget.  pool may be NULL to query the total in off[3 n], like strq_batch_fetch_units.  STRQ_ERR_ARG
 * when the last run call ran with the switch off. */
int strq_batch_fetch_tract_positions(strq_ctx* ctx, int32_t* pos_status, int64_t* off, int64_t* pool, int64_t pool_cap);
/* The tract-position pass of the last run call: out[0] = ms on the GPU (all its sub-batches), out[1] = windows traced,
 * out[2] = kernels launched (sorts, decodes, tracebacks, scans; 0 with the switch off), out[3] = peak back-pointer bytes of a piece. */
int strq_last_tract_positions(strq_ctx* ctx, double* out4);
/* ---- motifs: which repeat unit each stretch of the array is made of (no counterpart in the reference; strique_amd/motifs.py states
 * the rule, strq_motif_track is the model-level entry) ----
 * A target may hold K = 2 to 4 candidate units: per candidate a loop model (see strq_motif_track) and the flanked model of that
 * unit with its count bias; candidate 0 is the unit of the target's own flanked model.  With the switch on, every read whose gate
 * passed, that could be conditioned, with prefix_end < suffix_begin and whose target has candidates is scored: the stretch
 * [prefix_end, suffix_begin) of the filtered signal under the read's conditioning record -- the row's offset and offset + ticks,
 * which come from the two flank alignments and so do not depend on the configured unit -- cut into segments and scored as
 * strq_motif_track scores a window.  A flanked decode is not required.  A read whose majority is not candidate 0 is decoded once
 * more with the flanked model of the majority unit on the window of the count decode, [prefix_begin, suffix_end).
 * Limits: no anchored reads (their stretch has one end), no scan. */
typedef struct strq_motifs {
    int32_t status;         /* 0 scored, 1 not scored (gate failed, read not conditioned, empty stretch, target without candidates):
                             * the fields below are zero and the read has no segments */
    int32_t n_cand;
    int64_t n_seg;
    int32_t majority;       /* candidate with the most observations won */
    int32_t decode_status;  /* 0: count_m and log_p_m are valid; 1: none -- majority 0 and the row has no decode, or the majority
                             * model found no path */
    int64_t begin, end;     /* the stretch in raw samples */
    int64_t obs_won[4];     /* zero beyond n_cand */
    int32_t count_m;        /* the count under the majority unit: the row's count for majority 0, else visits + that model's bias */
    int32_t pad_;
    double log_p_m;
} strq_motifs;
/* The candidates of a target: n = 2 to 4, loop_model_ids[j] / flanked_model_ids[j] / bias[j] of candidate j; flanked_model_ids[0] is
 * not read (candidate 0 takes the row's decode).  n = 0 takes them away.  STRQ_ERR_UNSUPPORTED for a loop model the track does not
 * cover or a flanked model no compiled Viterbi kernel takes; the target stays as it was.  Never in the middle of a batch. */
int strq_target_set_motifs(strq_ctx* ctx, int32_t target_id, int32_t n, const int32_t* loop_model_ids, const int32_t* flanked_model_ids, const int32_t* bias);
/* on = 1: later run calls run the motif pass behind the rows with segments of `segment` observations (32 .. 4096): the host writes
 * the stretches from the geometry it holds, one launch of the track kernel and one of the reduction per sub-batch, one read-back;
 * then, for the reads whose majority is not candidate 0, a task kernel and one count-decode launch per kernel instance in use.
 * Rows and every other output do not change.  A run call with the switch on fails before any launch (STRQ_ERR_ARG) when it is a
 * scan.  Default 0: no further kernel runs and no further buffer is reserved. */
int strq_set_motifs(strq_ctx* ctx, int32_t on, int32_t segment);
/* One record per read of the last batch (n = its reads), and ragged the segments: off[n + 1] counts segments, segment s of read i has
 * winners[off[i] + s] and the scores V[4 (off[i] + s) + j] of candidate j (zero beyond n_cand).  V and winners may both be NULL to
 * query the total in off[n]; seg_cap: segments the pools hold.  STRQ_ERR_ARG when the last run call ran with the switch off. */
int strq_batch_fetch_motifs(strq_ctx* ctx, strq_motifs* out, int64_t n, int64_t* off, double* V, int32_t* winners, int64_t seg_cap);
/* The motif pass of the last run call: out[0] = ms on the GPU (all its sub-batches), out[1] = reads scored, out[2] = segments,
 * out[3] = kernels launched (track, reduction, tasks, sorts and decodes; 0 with the switch off), out[4] = majority decodes. */
int strq_last_motifs(strq_ctx* ctx, double* out5);
/* ---- state statistics: what the best path of the flanked decode assigns to every emitting state (no counterpart in the reference;
 * strique_amd/state_stats.py states the rule, strique_amd/calibrate.py re-estimates k-mer levels from it) ----
 * on = 1: later run calls, once the rows of a sub-batch are on the host, decode every window whose gate passed and whose flanked decode
 * found a path once more with back-pointers -- the task of the count / MARK launch: same window, same affine source on the filtered
 * signal, (T + 1) * n_states * 2 bytes -- trace it back and sum the observations per emitting state as strq_viterbi_state_stats does.
 * Pieces of at most STRQ_STATE_STATS_WS_BYTES of back-pointers (default 8 GiB), launches grouped by kernel shape, one read-back and one
 * wait per piece; a window whose back-pointers alone exceed the budget is not traced (status 2).  A run call with the switch on fails
 * before any launch: STRQ_ERR_ARG in a scan, STRQ_ERR_UNSUPPORTED when a target's model has no back-pointer decode.  STRQ_ERR_DEVICE
 * when the back-pointer decode of a window disagrees with its count decode in logp bits or counted.  Rows and every other output do not
 * change.  Sub-batches still in flight keep the mode they were launched with (the call waits for them).  Default 0: no further kernel
 * runs, no further buffer is reserved. */
int strq_set_state_stats(strq_ctx* ctx, int32_t on);
/* State statistics of the last batch of n reads, ragged: off[n + 1], read i owns entries off[i] .. off[i + 1] of the three pools --
 * silent_start of its flanked model, or none for a read without statistics; status[i] (nullable): 0 statistics, 1 none (the gate
 * failed, the read was not conditioned, or the flanked decode found no path), 2 back-pointers over the budget.  The pools (cap entries
 * each) may all be NULL to query the total in off[n], like strq_batch_fetch_units.  STRQ_ERR_ARG when the last run call ran with the
 * switch off. */
int strq_batch_fetch_state_stats(strq_ctx* ctx, int64_t* off, int64_t* n_obs, double* sum, double* sumsq, int64_t cap, int32_t* status);
/* The state-statistics pass of the last run call: out[0] = ms on the GPU (all its sub-batches), out[1] = windows traced,
 * out[2] = kernels launched (sorts, decodes, tracebacks, sums; 0 with the switch off), out[3] = peak back-pointer bytes of a piece. */
int strq_last_state_stats(strq_ctx* ctx, double* out4);
/* ---- state posteriors: the soft counterpart of the state statistics (no counterpart in the reference; strique_amd/state_posteriors.py
 * states the rule, `calibrate --posterior` re-estimates k-mer levels from it) ----
 * on = 1: later run calls, once the rows of a sub-batch are on the host, run forward-backward (strq_forward_state_stats) over every
 * window whose gate passed and whose flanked decode found a path -- the task of the count / MARK launch: same window, same affine
 * source on the filtered signal.  Pieces of at most STRQ_STATE_POST_WS_BYTES of stored forward vectors (default 8 GiB), launches
 * grouped by kernel shape, one read-back and one wait per piece; a window whose vectors alone exceed the budget gets its likelihood
 * and no rows (status 2).  A run call with the switch on fails before any launch: STRQ_ERR_ARG in a scan, STRQ_ERR_UNSUPPORTED when a
 * target's flanked model has no forward kernel.  Rows and every other output do not change.  Sub-batches still in flight keep the
 * mode they were launched with (the call waits for them).  Default 0: no further kernel runs, no further buffer is reserved. */
int strq_set_state_posteriors(strq_ctx* ctx, int32_t on);
/* State posteriors of the last batch of n reads, ragged like strq_batch_fetch_state_stats: off[n + 1], read i owns entries off[i] ..
 * off[i + 1] of the three pools -- silent_start of its flanked model, or none; log_lik[i] (nullable): the forward log-likelihood of its
 * window (NaN for a read that was not decoded, -inf without a forward path); status[i] (nullable): 0 statistics, 1 none (the gate
 * failed, the read was not conditioned, the flanked decode found no path, or the forward pass found none), 2 stored vectors over the
 * budget.  The pools (cap entries each) may all be NULL to query the total in off[n].  STRQ_ERR_ARG when the last run call ran with the
 * switch off. */
int strq_batch_fetch_state_posteriors(strq_ctx* ctx, int64_t* off, double* w, double* wx, double* wxx, int64_t cap, double* log_lik, int32_t* status);
/* The state-posteriors pass of the last run call: out[0] = ms on the GPU (all its sub-batches), out[1] = windows, out[2] = kernels
 * launched (sorts, forward and backward halves; 0 with the switch off), out[3] = peak bytes of stored forward vectors of a piece. */
int strq_last_state_posteriors(strq_ctx* ctx, double* out4);
/* ---- renorm: a second normalisation step for reads that are mostly repeat (no counterpart in the reference, whose 'minmax' map,
 * STRique.py:150-180, assumes that a read's k-mer composition looks like the pore model's) ----
 * Between the conditioning statistics and the flank alignments, every conditioned read of a target with tables gets scale and shift
 * of each of its normalised signals (0 the 8-bit morphology levels, 1 the median-filtered signal, 2 the raw signal where the target
 * has a modification model) refitted against the mixture w * (the target's repeat k-mers) + (1 - w) * (all k-mers) on a grid of 1024
 * bins: alpha = a / 64, beta = b bins, w one of 15 shares.  The fit maximises an int64 score over the signal's histogram
 * (strique_amd/renorm.py states grid, tables, schedule and tie rule; the kernels apply the same integer arithmetic).  A read whose
 * filtered signal fits a share below min_share keeps all its maps (applied = 0); every other fitted read gets the corrected c1, h1
 * of its fitted signals and the level values of the morphology signal, and everything behind conditioning runs on them. */
typedef struct strq_renorm_fit {
    int32_t a, b, w;        /* alpha * 64, beta in bins, index of the share */
    int32_t fitted;         /* 0: not fitted (degenerate read, empty histogram, no tables, no such signal); the other fields are zero then */
    int64_t score;          /* the best score */
} strq_renorm_fit;
typedef struct strq_renorm {
    int32_t applied, pad_;
    strq_renorm_fit fit[3]; /* morphology levels, filtered signal, raw signal */
} strq_renorm;
/* The tables of a target: Q[15][1024] (the scores of the grid's bins per share, |Q| < 2^15), q_out (the score of a bin mapped outside
 * the grid), A[105] (A[a] = the score of the scale a; entries below 24 are not read), W[15] (the shares), and the grid: start of bin
 * 0, bin width, pivot.  W and the grid belong to the context: while another target holds tables, a call whose W or grid differ from theirs is
 * refused (STRQ_ERR_ARG).  A call replaces the tables the target had (they are freed); Q = NULL takes them away. */
int strq_target_set_renorm(strq_ctx* ctx, int32_t target_id, const int16_t* Q, int32_t q_out, const int32_t* A, const double* W,
                           double grid_lo, double grid_d, double grid_p);
/* on = 1: later run calls refit the maps as described above.  STRQ_ERR_ARG for min_share outside (0, 1) (it has no default), and
 * while a scan is set (strq_scan_set); a run call with the switch on fails before any launch (STRQ_ERR_ARG) when a read's target has
 * no tables, and when it is a scan.  Sub-batches still in flight keep the mode they were launched with (the call waits for them).
 * Default 0: no further kernel runs and no further buffer is reserved. */
int strq_set_renorm(strq_ctx* ctx, int32_t on, double min_share);
/* One record per read of the last batch (n = its reads).  STRQ_ERR_ARG when the last run call ran with the switch off. */
int strq_batch_fetch_renorm(strq_ctx* ctx, strq_renorm* out, int64_t n);
/* The renorm pass of the last run call: out[0] = ms on the GPU (all its sub-batches), out[1] = reads whose filtered
 * signal was fitted, out[2] = reads applied, out[3] = kernels launched (0 with the switch off). */
int strq_last_renorm(strq_ctx* ctx, double* out4);
/* Testing: the fit kernel alone on three histograms of 1024 counters (every one below 2^31) with the tables of `target_id`:
 * out->fit[k] is the fit of h3[k * 1024 ..], out->applied stays 0. */
int strq_debug_renorm_fit(strq_ctx* ctx, int32_t target_id, const uint32_t* h3, strq_renorm* out);
/* A host-side helper, not on the path of strq_detect_batch (which takes these on the GPU): the statistics of float64 reads
 * with numpy's arithmetic (no context, no device): out[6 * i ..] = median, MAD, c1, h1 of
 * medfilt(read i, 3) and c1, h1 of read i itself (0, 1 unless want_raw) -- what numpy's median / mean / percentile
 * give repeatCounter.detect (STRique.py:590-597). */
int strq_host_stats(const double* signals, const int64_t* offsets, int64_t n_reads, int32_t want_raw, double* out);
/* Host-side helper of the fast5 reader (strique_amd/vbz.py): the variable-byte layer of a VBZ chunk -- n integers of
 * isize (2 | 4) bytes from key_bits (2: StreamVByte, 1: the 16-bit variant) keys + data, optionally zig-zag coded
 * differences.  Returns the stream bytes consumed (the caller checks it against the stream length) or -1. */
int64_t strq_svb_decode(const uint8_t* stream, int64_t stream_len, int64_t n, int32_t key_bits, int32_t zigzag,
                        int32_t isize, void* out);
/* Host-side helper of the fast5 reader (strique_amd/fast5.py): n_chunks deflate-compressed chunks of a 1-D chunked HDF5
 * dataset, chunk k at file offset addr[k] (csize[k] stored bytes, first element elem_off[k]), inflated from the mapped file
 * `base` into out[n_total] (elements of elem_size bytes; shuffle != 0: undo the HDF5 shuffle filter).  What h5py does
 * for the reference's get_raw (STRique_lib/fast5Index.py:220-233).  Returns 0, -1 on a bad argument, -(k + 2) when
 * chunk k is out of bounds or does not inflate. */
int64_t strq_inflate_chunks(const uint8_t* base, int64_t base_len, int64_t n_chunks, const int64_t* addr,
                            const int32_t* csize, const int64_t* elem_off, int32_t elem_size, int32_t shuffle,
                            int64_t chunk_elems, int64_t n_total, void* out);
/* Host-side helper of the fast5 reader: resolve the 1-D dataset `path` (components separated by '/') below the old-style group
 * whose version-1 object header sits at `group_ohdr` of the mapped file, and list its chunks -- what h5py does when the reference
 * opens /read_<id>/Raw/Signal (STRique_lib/fast5Index.py:76-84,220-233).  meta = {elements, element size, 0 unsigned | 1 signed |
 * 2 float, layout 1 contiguous | 2 chunked, data address (contiguous) or chunk B-tree address, elements per chunk, filters
 * (bit 0 deflate, bit 1 shuffle before it, bit 2 VBZ alone), 1 when the chunks tile the dataset -- every element is then written by
 * the decoder, then the VBZ client data {version, integer size, zig-zag flag, zstd level}, four reserved zeros}.  Returns the number of chunks written to chunk_addr / chunk_size / chunk_off (0 for
 * a contiguous dataset), STRQ_H5_MORE_CHUNKS when max_chunks is too small, STRQ_H5_UNHANDLED for anything else -- a structure this
 * helper does not cover or a malformed file: the caller then takes its general (Python) path, which also reports errors. */
#define STRQ_H5_UNHANDLED (-100)
#define STRQ_H5_MORE_CHUNKS (-101)
int64_t strq_h5_locate(const uint8_t* base, int64_t base_len, int64_t group_ohdr, const char* path, int64_t meta[16],
                       int64_t* chunk_addr, int32_t* chunk_size, int64_t* chunk_off, int64_t max_chunks);
/* The same for n_ds datasets in one call (one reader task of the `count` command): dataset i owns the chunks
 * [chunk_first[i], chunk_first[i + 1]) of addr / csize / elem_off and has its own mapped file base[i].  status[i] receives what
 * strq_inflate_chunks would return for it; the return value is the number of datasets that failed (-1: bad argument). */
int64_t strq_inflate_many(int64_t n_ds, const uint8_t* const* base, const int64_t* base_len, const int64_t* chunk_first,
                          const int64_t* addr, const int32_t* csize, const int64_t* elem_off, const int32_t* elem_size,
                          const int32_t* shuffle, const int64_t* chunk_elems, const int64_t* n_total, void* const* out,
                          int64_t* status);
/* The same contract for chunks behind the VBZ filter (HDF5 filter 32020: Oxford Nanopore's vbz_compression, what MinKNOW writes;
 * strique_amd/vbz.py has the format -- unpinned: no VBZ file or plugin exists in the image or the reference tree) with client data
 * {version, integer size, zig-zag flag, zstd level}: zstd through the system's libzstd (dlopen), then strq_svb_decode.  -1 also for
 * a combination this helper does not decode: the caller's general path then does, or says why not. */
int64_t strq_vbz_chunks(const uint8_t* base, int64_t base_len, int64_t n_chunks, const int64_t* addr, const int32_t* csize,
                        const int64_t* elem_off, int32_t elem_size, int32_t version, int32_t isize, int32_t zigzag, int32_t level,
                        int64_t chunk_elems, int64_t n_total, void* out);
/* Diagnostics of the two calls above: out[0] = nanoseconds spent inside the inflate itself (all threads together), out[1] = zlib
 * streams inflated, out[2] = bytes produced, since the last reset; reset != 0 clears the counters. */
void strq_inflate_stats(int64_t out[3], int32_t reset);
/* 1 when libdeflate (dlopen of libdeflate.so.0) decodes the zlib streams of strq_inflate_chunks in this process, 0 when
 * zlib does (library absent, or STRQ_NO_LIBDEFLATE=1).  Same bytes either way. */
int strq_inflate_backend(void);
/* Test hook: conditioning outputs (8-bit morphology levels, their 256 float32 values, and
 * {median, MAD, c1/h1 of the filtered, morphology and raw signal, h2, c2}) of read `read` of the
 * last sub-batch processed by strq_batch_run. */
int strq_debug_conditioning(strq_ctx* ctx, int64_t read, uint8_t* levels, int64_t n, float* level_val,
                            double* scalars10);
/* Test hook: the median-filtered signal (scipy.signal.medfilt(raw, 3)) of read `read` of the last sub-batch processed by
 * strq_batch_run, in the element type of the batch (int16 or float64): min(n, length of the read) elements to `out`.
 * STRQ_ERR_ARG when the last sub-batch has no such read. */
int strq_debug_filtered(strq_ctx* ctx, int64_t read, void* out, int64_t n);
/* Test hook, no context and no device: the blocks of memory the library holds in this process right now, over all contexts --
 * out[0] device blocks, out[1] blocks of pinned host memory.  Whatever a context, its models and its batches allocated is given
 * back by strq_ctx_destroy: the two numbers are then what they were before strq_ctx_create. */
int strq_debug_live_allocations(int64_t out[2]);
/* Test hook, host only (no context, no device): the tables strq_model_set_positions would upload for this model --
 * out_lp[31 * 64] (log-probability of every column of the layout per lane, -inf where a lane has no such edge),
 * out_own[6 * 64] (state of every slot and lane, -1 if none, -2 for a virtual relay state), out_meta[10] = {slot, lane of
 * the two broadcast sources, of start and of end, then the low and high word of the lane mask of relayed hub states} -- the
 * caller provides TEN int32.  STRQ_ERR_UNSUPPORTED and the reason in `why` when the model is no profile chain.
 * tests/test_g2_layout.py drives a plain restatement of the kernel's time step with them. */
int strq_debug_g2_layout(int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                         const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                         const int32_t* emis_kind, const int32_t* count_inc, const int32_t* kind, const int32_t* pos,
                         double* out_lp, int32_t* out_own, int32_t* out_meta, char* why, int32_t why_len);

/* Test hook, host only (no context, no device): the Viterbi kernel shape strq_model_create would put this model on.  Model arrays
 * and placement hints as strq_model_create takes them (count_inc, state_tag, hint_slot, hint_lane may be NULL).  out[48]:
 *   [0..4]    the shape id of a launch of decode mode 0 count, 1 back-pointers, 2 mark, 3 hub, 4 unit: the row of the lane-layout
 *             table (csrc/vit_model.h, VIT_SHAPES) plus 16 for a single-stage model, or 8 for the general kernel; -1: no kernel
 *             (the register-resident image of strq_model_set_positions is not planned here: it needs no row)
 *   [5..9]    1 where the library has a launch of that mode for this model (the shape has the mode; hub: the model has a hub state
 *             with an edge into `end`; unit: exactly two counted emitting states and no counted silent one)
 *   [10] emitting, [11] silent slots per lane   [12..19] in-edge registers of the emitting, [20..27] of the silent slots (without
 *   chain edges)   [28..35] 1: the emitting slot holds no Normal emission   [36] single-stage   [37] a silent state is counted
 *   [38] the recording hub state or -1   [39], [40] the two counted states of a unit decode or -1   [41] 1: the general kernel
 * STRQ_ERR_ARG (bad arrays) or STRQ_ERR_UNSUPPORTED (more than 4096 states) with the reason in `why`. */
int strq_debug_viterbi_plan(int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                            const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                            const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                            const int32_t* count_inc, const int32_t* state_tag,
                            const int32_t* hint_slot, const int32_t* hint_lane, int32_t* out, char* why, int32_t why_len);
/* Test hook: ONE Viterbi launch of decode mode `mode` (0 count, 2 mark, 3 hub, 4 unit) over n_seq (1 ... 8192) windows
 * x[x_off[i] .. x_off[i + 1]) of model `model_id`, on the kernel shape the pipeline would take for that mode (STRQ_VIT_NO_G2 and
 * STRQ_VIT_G2_* act as they do there).  Everything comes back raw, per window: logp, counted, status, dbg[4 i .. 4 i + 3] -- mark:
 * dbg[0] / dbg[1] the 1-based time of the first emission of a state tagged 1 / of the first emission behind that stretch, 0 = none;
 * hub, unit: dbg[0] the payload of the end state -- and the record buffer of window i, zeroed before the launch, at
 * records + rec_off[i] (bytes): hub T + 1 records of 8 bytes (record t, written by the emission of the recording hub state at
 * time t: low word the time of the previous such emission on that state's best path, high word the branch of the unit in between:
 * tag 1 -> 1, 3 -> 2, 4 -> 3, else 0), unit 2 T records of 4 bytes (record 2 t + k, written by counted state k at observation t:
 * the payload (t' + 1) << 1 | k' of the previous counted emission, 0 = none).  rec_off[i + 1] - rec_off[i] must be 8 (T + 1) / 8 T;
 * records and rec_off may be NULL for count and mark.  launched[0] = the shape id that ran (as strq_debug_viterbi_plan reports it;
 * 9 = the register-resident kernel).  STRQ_ERR_UNSUPPORTED where the library has no launch of that mode for the model.
 * Own buffers on the context's stream: a batch in flight and its results are left alone. */
int strq_debug_viterbi_mode(strq_ctx* ctx, int32_t model_id, int32_t mode, int64_t n_seq, const double* x, const int64_t* x_off,
                            double* logp, int64_t* counted, int32_t* status, uint32_t* dbg, void* records, const int64_t* rec_off,
                            int32_t* launched);
/* Test hook: the same launch over windows given the way the detect pipeline gives them -- samples and a per-window map instead of
 * observations.  src_kind 2: `samples` are int16_t, 1: double; x_off counts samples.  consts[6 i .. 6 i + 5] = c1, h1, h2, c2, lo, hi
 * of window i: the kernels read observation x = clip((s - c1) / h1 * h2 + c2, lo, hi), every operation rounded on its own, and take
 * their branch-free emission code for a window whose [lo, hi] lies inside every uniform emission's support and whose c1 and h1 are
 * numbers (NaN c1 or h1: a window of missing observations).  tracts != 0 (mode 0, a model with strq_model_set_tracts): the
 * wide-payload count launch of strq_viterbi_tracts -- never the register-resident kernel -- and tract_counts[3 i .. 3 i + 2] as that
 * call returns them (`counted` then holds the raw payload); tract_counts may be NULL otherwise.  Everything else as
 * strq_debug_viterbi_mode.  STRQ_ERR_ARG: a source kind other than 1 or 2, h1 == 0, lo > hi (or either not a number), a float64
 * sample that is not a number (the branch-free code has no test for a missing observation; the pipeline never hands it one),
 * tracts with another mode or a model without tracts.  STRQ_ERR_UNSUPPORTED exactly where strq_debug_viterbi_mode returns it. */
int strq_debug_viterbi_sourced(strq_ctx* ctx, int32_t model_id, int32_t mode, int32_t src_kind, int32_t tracts, int64_t n_seq,
                               const void* samples, const int64_t* x_off, const double* consts,
                               double* logp, int64_t* counted, int32_t* status, uint32_t* dbg, void* records, const int64_t* rec_off,
                               int64_t* tract_counts, int32_t* launched);

/* Test hook, host only (no context, no device): the integer frame the upper-bound screen would run in for these alignment
 * parameters (open_h, ext_h, open_v, ext_v, dist_offset, dist_min; src/align_raw.h:84-103) and reads of up to `max_n` samples.
 * Returns 1 and out[6] = {scale, -ext_h * scale, -ext_v * scale, what is added to every table entry, float32 slack * scale,
 * columns below which candidate chunks merge}, or 0 when the parameters allow no screen (then the float32 DP runs over whole reads). */
int strq_debug_screen_plan(const float params[6], int32_t samples, int32_t max_n, int32_t out[6]);

/* Test hook: the score tables of the flank DP (csrc/lut_kernels.hip) as strq_align_batch would build them for n_jobs (1 ... 4096)
 * (read, flank) pairs under the context's current alignment parameters -- the same code: the build kernel, the host's
 * re-evaluation of the borderline entries and the patch kernel, the host's rebuild of the tables the kernel gave up on.
 *   level_val[n_jobs x 256]   the 256 level values of job j's read (any float32)
 *   cls_val, cls_off[n_jobs + 1]   the class values of job j's flank are cls_val[cls_off[j] .. cls_off[j + 1]): 1 ... 158 per job
 * Out, raw -- job j has k = cls_off[j + 1] - cls_off[j] classes:
 *   info[5 j ..]   total (entries of the ragged table), need (widest row), packed (1: the 24-bit copy holds the same numbers),
 *                  n_hard (borderline entries listed for the host; -1: the whole table went to the host) -- all four as the kernel
 *                  reported them -- and the entries of the finished table (256 k after a rebuild, else `total`)
 *   band_lo[cls_off[j] + x]   row descriptor of class x: e_l | (e_r - e_l) << 8 | row offset << 16.  The entry the DP reads for
 *                  level q is table[row offset + clamp(q, e_l, e_r) - e_l]
 *   table[256 cls_off[j] ..]   the float32 entries of job j (a slot of 256 k)
 *   planes[768 cls_off[j] + 8 j ..]   the 24-bit copy of job j's entries as the kernel wrote it (a slot of 768 k + 8 bytes): `total`
 *                  uint16 (bits 8-23 of every entry), then from byte (2 total + 3) & ~3 on `total` uint8 (bits 0-7); an entry is
 *                  (hi16 << 8 | lo8) * 2^-20.  Meaningful where packed = 1; zeros for a table the kernel left before it wrote any
 *   handed[4 i ..], n_handed   the borderline entries the kernel listed: job, class, level, index into the job's table; at most
 *                  handed_cap are written, *n_handed is their number (strq_last_timing [4] of a batched call)
 * Uses the context's alignment workspace: not while a batch is resident or in flight on it. */
int strq_debug_score_tables(strq_ctx* ctx, int32_t n_jobs, const float* level_val, const float* cls_val, const int64_t* cls_off,
                            int32_t* info, int32_t* band_lo, float* table, uint8_t* planes,
                            int32_t* handed, int32_t handed_cap, int32_t* n_handed);

/* Test hooks, host only (no context, no device): the edge image the variant pass / the per-unit scores of the modification pass
 * would upload for this model (csrc/variant_kernels.h VarModel, csrc/mod_llr_kernels.h LlrModel), built for a null device base.
 * Model arrays as strq_model_create takes them; n_alt as strq_target_set_variants takes it.
 *   *build_rc      what the image builder returned: 0, or 1 with the reason in `why` (a model the pass does not cover)
 *   head[10]       n_emit, branches (2 for the dual model), mode, deg, deg2, end_deg[0 .. 3], 0
 *   offsets[12]    byte offsets inside `image` of src, lp, src2, lp2, start_lp, kind, hub, ea, eb, ec, end_src, end_lp -- int32 / float64
 *                  arrays in the layout the two headers document (rows of 64 lanes)
 *   image          the image itself, *image_bytes of it (nothing is copied when image_cap is smaller; image may then be NULL)
 * STRQ_ERR_ARG for a null array or a start / end outside the states; STRQ_OK otherwise, whatever *build_rc is.
 * tests/passage_cases.py interprets the image on the CPU. */
int strq_debug_variant_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                             const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                             const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                             const int32_t* state_tag, int32_t n_alt, int32_t* build_rc, int32_t* head, int64_t* offsets,
                             void* image, int64_t image_cap, int64_t* image_bytes, char* why, int32_t why_len);
int strq_debug_mod_llr_image(int32_t n_states, int32_t silent_start, int32_t start, int32_t end,
                             const int32_t* in_ptr, const int32_t* in_src, const double* in_logp,
                             const int32_t* emis_kind, const double* emis_a, const double* emis_b, const double* emis_c,
                             const int32_t* state_tag, int32_t* build_rc, int32_t* head, int64_t* offsets,
                             void* image, int64_t image_cap, int64_t* image_bytes, char* why, int32_t why_len);
/* Test hooks: the scores of given passages / units, by one launch of the score kernel of the variant pass / of the per-unit scores --
 * the kernels of strq_set_variants / strq_set_mod_llr without the pipeline around them.  For n_reads (1 ...) reads: model_id[r] a
 * model of strq_model_create (its image is built, or reused, as strq_target_set_variants / strq_set_mod_llr build it -- but a model
 * that fits no Viterbi kernel is not refused: nothing is decoded), the stretch x[x_off[r] .. x_off[r + 1]) and its bounds
 * w[w_off[r] .. w_off[r + 1]) -- any int32: passage j of a read covers x[u_j .. w_j], u_0 = 0, u_j = w_{j-1} + 1, and scores -inf
 * throughout unless 0 <= u_j <= w_j < T.  out: NB = n_alt + 1 (or 2) doubles per bound, in the order of w.  launched[0] = the kernel
 * mode that ran (0: two passages per wave, 1: one state per lane, 2: two states per lane), launched[1] = NB.
 * STRQ_ERR_ARG when the models of a call do not share (mode, NB), STRQ_ERR_UNSUPPORTED for a model the pass does not cover.
 * Own buffers on the context's stream: a batch in flight and its results are left alone. */
int strq_debug_variant_scores(strq_ctx* ctx, int32_t n_reads, const int32_t* model_id, int32_t n_alt, const double* x,
                              const int64_t* x_off, const int32_t* w, const int64_t* w_off, double* out, int32_t* launched);
int strq_debug_mod_llr_scores(strq_ctx* ctx, int32_t n_reads, const int32_t* model_id, const double* x, const int64_t* x_off,
                              const int32_t* w, const int64_t* w_off, double* out, int32_t* launched);
/* Test hook: the two passes of the bounds kernels of the variant pass (count, then write) for n_reads reads of one model, set up as
 * the pipeline sets them up.  Read r has T_r = off[r + 1] - off[r] observations.  Scan route (path != NULL): path[off[r] ..] the
 * emitting state of every observation (each below silent_start).  Hop route (path == NULL): rec[off[r] + r ..] the T_r + 1 hub
 * records of the read, last[r] the index of the last record (what the decode leaves in its result).  status[r]: the decode status
 * to present (0 a path, 1 none).  cap[r] >= 0 replaces the count of the first pass as the `cap` of the write pass (at most
 * stride - guard); -1 takes the count.  Out: n[r] passages counted; bad[2 r], bad[2 r + 1] the flag behind the count / the write
 * pass; w, branch [r * stride ..]: `stride` entries per read as the write pass left them, 0x7F7F7F7F where nothing was written;
 * untouched[r] = 1 when every entry from the write pass's cap on still holds that value.
 * STRQ_ERR_ARG for a state outside the emitting ones, a cap beyond the stride, n_alt outside 1 .. 3. */
int strq_debug_variant_bounds(strq_ctx* ctx, int32_t model_id, int32_t n_alt, int32_t n_reads, const int64_t* off,
                              const int32_t* path, const uint64_t* rec, const uint32_t* last, const int32_t* status,
                              const int32_t* cap, int32_t stride, int32_t guard, int32_t* n, int32_t* bad, int32_t* w,
                              int32_t* branch, int32_t* untouched);
/* Test hook: the bounds kernel of the flank methylation calls (strique_amd/flank_mod.py states the rule) for n_flanks (1 ...) flank
 * stretches decoded with one flank profile model of n_emit emitting states, column_of[s] the profile column of emitting state s
 * (-1: none).  Stretch f has T_f = off[f + 1] - off[f] observations (below 2^30), path[off[f] ..] the emitting state of every
 * observation, status[f] the decode status to present (0 a path, anything else none; NULL: a path everywhere), and the CpG groups
 * g_off[f] .. g_off[f + 1] (at most 64 per stretch): group g covers the profile columns groups[2 g] .. groups[2 g + 1].
 * out: three int32 per group -- status (0 scored, 1 no path, 2 edge: the first emission from the group's columns is the stretch's
 * first observation or the last one its last, 3 skipped: no emission from them), u = first - 1 and w = last + 1 (-1, -1 unless
 * scored).  STRQ_ERR_ARG for a state outside the emitting ones or more than 64 groups in a stretch.  Own buffers on the context's
 * stream: a batch in flight and its results are left alone. */
int strq_debug_flank_mod_bounds(strq_ctx* ctx, int32_t n_flanks, const int64_t* off, const int32_t* path, const int32_t* status,
                                int32_t n_emit, const int32_t* column_of, const int64_t* g_off, const int32_t* groups, int32_t* out);

/* Kernel timing of the last batched call, milliseconds (HIP events on the library's stream):
 * [0] table build  [1] forward DP  [2] trace pass  [3] total  [4] table entries re-evaluated on
 * the host  [5] conditioning  [6] Viterbi  [7] number of forward-DP kernel launches.  */
int strq_last_timing(const strq_ctx* ctx, float ms[8]);
/* Work counters of the last batched call (what the benchmark's roofline is priced with):
 * [0] forward-DP wave-steps (one step = two DP columns of every flank row, summed over all waves)
 * [1] DP columns computed, including the columns column segments recompute   [2] alignments
 * [3] waves per alignment (column segments) of the last forward launch   [4] score tables per CU
 * [5] 1 = 24-bit tables, 0 = float32   [6] rows per lane   [7] Viterbi time steps. */
int strq_last_counters(const strq_ctx* ctx, double out[8]);
/* Launch geometry of the last forward-DP launch of the last batched call (which kernel instance ran; the parity
 * tests assert it, the benchmark names the kernel of its roofline with it):
 * [0] waves per alignment (column segments)   [1] score tables per CU   [2] WPE template argument of
 * align_forward_seg_kernel<R, S, PK, SEG, WPE> (0: the one-wave kernels ran)   [3] rows per lane R
 * [4] 1 = 24-bit tables   [5] overlap (columns) the pieces were cut with first   [6] the worst-case overlap
 * [7] forward launch groups of the last sub-batch. */
int strq_last_geometry(const strq_ctx* ctx, int32_t out[8]);
/* Viterbi launches of the flanked-model decode (scripts/STRique.py:603) of the last sub-batch of the last batched call:
 * [0] launches   [1] of them on the register-resident kernel (viterbi_g2_kernel: one launch serves repeat profiles of
 * either parity)   [2] on the lane-layout kernels   [3] on the general kernel (viterbi_csr_kernel). */
int strq_last_viterbi_launches(const strq_ctx* ctx, int32_t out[4]);
/* Flank alignments of the last batched call whose first forward round -- column segments cut with the short, adaptive
 * overlap, or the screen's windows -- did not reach the score that certifies it, and which therefore ran the second round over their
 * whole read with the worst-case overlap: [0] such alignments, [1] all alignments (two per read).  What a read that does not contain
 * its flank costs.  (Alignments the coarse screen's second look resolved with more windows are not in [0]: strq_last_screen_mode [5].) */
int strq_last_second_round(const strq_ctx* ctx, int64_t out[2]);
/* The upper-bound screen of the last batched call (csrc/screen_kernels.hip: an integer DP over the whole read whose last-row
 * values bound the float32 ones of src/align_raw.h:106-158 from above, so that the exact DP only runs over the column windows
 * that can hold the optimum): [0] ms in align_screen_kernel   [1] alignments screened   [2] of them with windows
 * [3] without (their whole read ran)   [4] columns inside the windows   [5] screen wave-steps (one step = two columns of
 * every flank row)   [6] scale (scores are rounded up to multiples of 1 / scale)   [7] candidate chunks of 128 columns. */
int strq_last_screen(const strq_ctx* ctx, double out[8]);
/* Which screen the last sub-batch of the last batched call ran: [0] 0 none, 1 the fine screen (align_screen_kernel: one DP row per flank
 * row, bound within m / scale of the exact last row), 2 the coarse one (align_screen3_kernel by default: three flank rows per DP row, both flanks
 * of a read per wave, candidates taken with a margin)   [1] / [2] sub-batches for which the coarse / the fine screen stays paused
 * (it did not pay on the last one it ran on)   [3] the coarse screen's candidate margin in score units (x 1.3 / 1.75 at three / six
 * rows per DP row)   [4] flank rows per DP row of the screen that ran (3: align_screen3_kernel, 1: align_screen1_kernel, 0: the one-flank
 * kernel)   [5] alignments of the last batched call that missed the first look's certificate and were resolved by the coarse screen's second look
 * (or belonged to an attempt that started over with the fine screen)   [6] LDS layout of the score tables in the two-flank kernels of that
 * screen: 1 the lane-major image (one 16-bit column per lane, no bank conflicts), 2 class rows (STRQ_SCREEN_LDS=rows, or an image that
 * would not fit: wide bands), 3 the level image of the coarse screen (one row of byte entries per level, STRQ_SCREEN_LDS=levels or the
 * default where the alignment parameters admit a byte scale and every read's image fits), 0 the one-flank kernel or no screen   [7] on the level
 * image, the scale the kernel rounds its byte entries at inside (6 for STRique's parameters; its chunk values are converted up to the scale of
 * strq_last_screen [6], in which everything behind the kernel works); 0 otherwise. */
int strq_last_screen_mode(const strq_ctx* ctx, int32_t out[8]);
/* The two sub-batches in flight, since the start of the last run call: [0] ms of HMM Viterbi launches whose rows were taken
 * [1] of them, ms that lay under the screen kernel of the sub-batch that followed   [2] ... under its whole alignment stage
 * (screen, exact pass, trace)   [3] sub-batches counted in [1], [2] (those whose rows were taken by the following sub-batch's run
 * call; a sub-batch nobody followed runs its Viterbi launches alone). */
int strq_last_overlap(const strq_ctx* ctx, double out[4]);

#ifdef __cplusplus
}
#endif
#endif
