// C ABI of the motif track (include/strique_hip.h: strq_motif_track; kernels: motif_kernels.hip; the rule: strique_amd/motifs.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/strique_hip.h"
#include "strq_ctx.h"
#include "detect_plan.h"
#include "motif_kernels.h"

using namespace strq;

namespace strq {

// The edge image of a loop model (HostModel::motif_dev), built if it is not there; STRQ_ERR_UNSUPPORTED (c->err says why) for a model
// that is no loop model.
int motif_model(strq_ctx* c, HostModel* hm)
{
    if (hm->motif_dev) return STRQ_OK;
    if (hm->motif_blob.reserve(motif_image_bytes()) != hipSuccess) { c->err = "out of device memory"; return STRQ_ERR_NOMEM; }
    std::vector<char> blob; std::string why;
    if (motif_build_image(hm->n_states, hm->silent_start, hm->start, hm->end, hm->in_ptr.data(), hm->in_src.data(), hm->in_logp.data(),
                          hm->emis_kind.data(), hm->emis_a.data(), hm->emis_b.data(), hm->emis_c.data(), hm->motif_blob.p, blob, why)) { c->err = why; return STRQ_ERR_UNSUPPORTED; }
    STRQ_HIP(c, hipMemcpy(hm->motif_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    hm->motif_dev = hm->motif_blob.as<MotifModel>();
    return STRQ_OK;
}

}  // namespace strq

extern "C" {

int strq_motif_track(strq_ctx* c, int32_t n_models, const int32_t* model_ids, int32_t segment, int64_t n_seq, const double* x, const int64_t* x_off,
                     int64_t seg_cap, double* V, int32_t* winners, int64_t* n_seg, int64_t* obs_won, int32_t* majority)
{
    STRQ_ENTER(c);
    if (n_models < 2 || n_models > MOTIF_MAX_CAND || !model_ids || n_seq < 0 || n_seq >= ((int64_t)1 << 31) || !x_off || x_off[0] != 0 || seg_cap < 0 ||
        !V || !winners || !n_seg || !obs_won || !majority) { c->err = "bad argument"; return STRQ_ERR_ARG; }
    if (segment < MOTIF_SEG_MIN || segment > MOTIF_SEG_MAX) { c->err = "bad argument (the segment length must lie between " + std::to_string(MOTIF_SEG_MIN) + " and " + std::to_string(MOTIF_SEG_MAX) + ")"; return STRQ_ERR_ARG; }
    const MotifModel* dev[MOTIF_MAX_CAND] = {nullptr, nullptr, nullptr, nullptr};
    for (int32_t j = 0; j < n_models; ++j) {
        if (model_ids[j] < 0 || model_ids[j] >= (int32_t)c->models.size() || !c->models[(size_t)model_ids[j]]) { c->err = "bad argument (no such model)"; return STRQ_ERR_ARG; }
        HostModel* hm = c->models[(size_t)model_ids[j]];
        if (const int rc = motif_model(c, hm)) return rc;
        dev[j] = hm->motif_dev;
    }
    if (n_seq == 0) return STRQ_OK;
    int64_t total_seg = 0;
    for (int64_t i = 0; i < n_seq; ++i) {
        const int64_t T = x_off[i + 1] - x_off[i];
        if (T < 1) { c->err = "bad argument (a window needs at least one observation, and offsets must not decrease)"; return STRQ_ERR_ARG; }
        n_seg[i] = T / segment > 1 ? T / segment : 1;
        total_seg += n_seg[i];
    }
    if (!x || total_seg > seg_cap) { c->err = "bad argument (the pools hold fewer segments than the windows have)"; return STRQ_ERR_ARG; }
    const int64_t tot = x_off[n_seq];
    const int run = motif_run_segments(segment);
    std::vector<MotifWindow> wv((size_t)n_seq); std::vector<MotifTask> tv;
    Carve lay;
    const size_t o_x = lay.add<double>((size_t)tot), o_V = lay.add<double>((size_t)total_seg * (size_t)n_models), o_win = lay.add<int32_t>((size_t)total_seg),
                 o_won = lay.add<int64_t>((size_t)n_seq * MOTIF_MAX_CAND), o_maj = lay.add<int32_t>((size_t)n_seq), o_w = lay.add<MotifWindow>((size_t)n_seq);
    int64_t seg_at = 0;
    for (int64_t i = 0; i < n_seq; ++i) {
        for (int64_t s = 0; s < n_seg[i]; s += run) {
            MotifTask t; t.window = (int32_t)i; t.seg_first = s; t.seg_count = (int32_t)(n_seg[i] - s < run ? n_seg[i] - s : run);
            tv.push_back(t);
        }
        seg_at += n_seg[i];
    }
    const size_t o_t = lay.add<MotifTask>(tv.size());
    DevBuf ws;
    STRQ_HIP(c, ws.reserve(lay.total() + 64));
    double* d_x = Carve::at<double>(ws.p, o_x); double* d_V = Carve::at<double>(ws.p, o_V); int32_t* d_win = Carve::at<int32_t>(ws.p, o_win);
    int64_t* d_won = Carve::at<int64_t>(ws.p, o_won); int32_t* d_maj = Carve::at<int32_t>(ws.p, o_maj);
    MotifWindow* d_w = Carve::at<MotifWindow>(ws.p, o_w); MotifTask* d_t = Carve::at<MotifTask>(ws.p, o_t);
    seg_at = 0;
    for (int64_t i = 0; i < n_seq; ++i) {
        MotifWindow& w = wv[(size_t)i]; std::memset(&w, 0, sizeof(w));
        w.obs.sig = d_x + x_off[i]; w.obs.T = x_off[i + 1] - x_off[i]; w.obs.src_kind = VIT_SRC_F64;
        for (int32_t j = 0; j < MOTIF_MAX_CAND; ++j) w.model[j] = dev[j];
        w.n_cand = n_models; w.segment = segment; w.n_seg = n_seg[i];
        w.V = d_V + (size_t)seg_at * (size_t)n_models; w.winner = d_win + seg_at;
        w.obs_won = d_won + (size_t)i * MOTIF_MAX_CAND; w.majority = d_maj + i;
        seg_at += n_seg[i];
    }
    hipStream_t st = c->stream;
    STRQ_HIP(c, hipMemcpyAsync(d_x, x, (size_t)tot * 8, hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_w, wv.data(), wv.size() * sizeof(MotifWindow), hipMemcpyHostToDevice, st));
    STRQ_HIP(c, hipMemcpyAsync(d_t, tv.data(), tv.size() * sizeof(MotifTask), hipMemcpyHostToDevice, st));
    if (launch_motif_track(st, d_w, (int)n_seq, d_t, (int64_t)tv.size(), c->n_cu)) { c->err = "motifs: launch failed"; return STRQ_ERR_DEVICE; }
    STRQ_HIP(c, hipMemcpyAsync(V, d_V, (size_t)total_seg * (size_t)n_models * 8, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(winners, d_win, (size_t)total_seg * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(obs_won, d_won, (size_t)n_seq * MOTIF_MAX_CAND * 8, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipMemcpyAsync(majority, d_maj, (size_t)n_seq * 4, hipMemcpyDeviceToHost, st));
    STRQ_HIP(c, hipStreamSynchronize(st));
    return STRQ_OK;
}

}  // extern "C"
