// Anchored counting: which reads hold one flank only, and their windows for the HMM.  The flank geometry and the conditioning
// rows are on the device already (finalize_kernel, scan_kernels.h); the decode runs on the Viterbi kernels as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "anchored_kernels.h"

namespace strq {

// One thread per read.  m = min_score > 0; every comparison with a NaN score is false, so such a read is neither above nor below m.
__global__ void __launch_bounds__(128) anchored_classify_kernel(AnchoredClassifyArgs a)
{
    const int r = blockIdx.x * 128 + threadIdx.x;
    if (r >= a.n_reads) return;
    const ReadCond rc = a.rc[r];
    const ReadGeom g = a.geom[r];
    AnchoredClass c = {};
    if (rc.n > 0 && rc.status == COND_OK) {
        const double m = a.min_score;
        const bool pre = g.score_prefix >= m, suf = g.score_suffix >= m;
        if (pre && suf) {
            if (g.prefix_begin < g.suffix_end) { c.kind = ANCH_SPANNING; c.begin = g.prefix_begin; c.end = g.suffix_end; }
        } else if (pre && g.score_suffix < m) {
            // prefix_begin is a sample of the read (row_position), so the window is never empty
            if (g.prefix_begin >= 0 && g.prefix_begin < (int64_t)rc.n) { c.kind = ANCH_ENDS; c.begin = g.prefix_begin; c.end = rc.n; }
        } else if (suf && g.score_prefix < m) {
            if (g.suffix_end > 0 && g.suffix_end <= (int64_t)rc.n) { c.kind = ANCH_STARTS; c.begin = 0; c.end = g.suffix_end; }
        }
    }
    a.out[r] = c;
}

__global__ void __launch_bounds__(128) anchored_task_kernel(AnchoredTaskArgs a)
{
    const int k = blockIdx.x * 128 + threadIdx.x;
    if (k >= a.n_tasks) return;
    const int r = a.read[k];
    VitTask vt = {};
    vt.model = a.model[k];
    if (r >= 0 && r < a.n_reads) {
        const AnchoredClass c = a.cls[r];
        const ReadCond rc = a.rc[r];
        // the window once more against the read it is cut from: a task never leaves the read's samples
        const int open = (c.kind == ANCH_ENDS || c.kind == ANCH_STARTS) && c.begin >= 0 && c.begin < c.end && c.end <= (int64_t)rc.n;
        vt = window_task(open, c.begin, c.end, rc, a.model[k], a.flt, a.is_f64, a.ps);
    }
    a.vit[k] = vt;
}

// One thread per item.  The stretch is read off the marks exactly as anchored_record (detect_plan.h) reads it for the record, and
// checked once more against the window, the read and what the host reserved: a task never leaves the read's samples or its buffers.
__global__ void __launch_bounds__(128) anchored_mod_task_kernel(AnchoredModTaskArgs a)
{
    const int k = blockIdx.x * 128 + threadIdx.x;
    if (k >= a.n_items) return;
    const AnchoredModItem it = a.item[k];
    ModTask m = {};
    VitTask vt = {};
    m.out = it.out; m.is_f64 = a.is_f64;
    m.clip_lo = a.clip_lo; m.clip_hi = a.clip_hi; m.mod_lo = it.mod_lo; m.mod_hi = it.mod_hi;
    vt.model = it.model; vt.sig = it.out; vt.src_kind = VIT_SRC_F64; vt.bp = it.bp;
    if (it.read >= 0 && it.read < a.n_reads && it.res >= 0 && it.res < a.n_res) {
        const AnchoredClass c = a.cls[it.read];
        const ReadCond rc = a.rc[it.read];
        const VitResult v = a.res[it.res];
        const bool open = (c.kind == ANCH_ENDS || c.kind == ANCH_STARTS) && c.begin >= 0 && c.begin < c.end && c.end <= (int64_t)rc.n;
        const int64_t W = c.end - c.begin;
        const int64_t enter = v.dbg[0], leave = v.dbg[1] ? (int64_t)v.dbg[1] : W + 1;
        if (open && v.status == 0 && enter >= 1 && leave > enter && leave <= W + 1 && leave - enter <= it.cap) {
            const int64_t begin = c.begin + enter - 1, T = leave - enter;
            m.raw = static_cast<const char*>(a.raw) + (size_t)(rc.off + begin) * (a.is_f64 ? 8 : 2);
            m.T = T; vt.T = T;
            m.c1 = rc.r_c1; m.h1 = rc.r_h1; m.h2 = rc.h2; m.c2 = rc.c2;
        }
    }
    a.mod[k] = m;
    if (it.slot >= 0 && it.slot < a.n_items) a.vit[it.slot] = vt;
}

int launch_anchored_mod_tasks(hipStream_t s, const AnchoredModTaskArgs& a)
{
    if (a.n_items <= 0) return 0;
    hipLaunchKernelGGL(anchored_mod_task_kernel, dim3((a.n_items + 127) / 128), dim3(128), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_anchored_classify(hipStream_t s, const AnchoredClassifyArgs& a)
{
    if (a.n_reads <= 0) return 0;
    hipLaunchKernelGGL(anchored_classify_kernel, dim3((a.n_reads + 127) / 128), dim3(128), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_anchored_tasks(hipStream_t s, const AnchoredTaskArgs& a)
{
    if (a.n_tasks <= 0) return 0;
    hipLaunchKernelGGL(anchored_task_kernel, dim3((a.n_tasks + 127) / 128), dim3(128), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace strq
