"""Cost of a scan (strq_scan_set) on bench.py's workload (BASELINE configs[2]: 50 kb reads, C9orf72): reads/s and ms per stage of
one resident batch as a plain detect (every read with its true target and strand) and as a scan over the four candidates of the
bundled repeat_config.tsv (c9orf72 +/-, fmr1 +/-) on the same reads and the same build; how many reads find their true candidate.
usage (GPU box): python tools/scan_probe.py [n_reads] [read_nt] [steps] [min_score]"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench  # noqa: E402
from strique_amd.counter import repeatCounter  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    min_score = float(sys.argv[4]) if len(sys.argv) > 4 else 5.0          # the value the tests use; a scan has no default
    pm, cfg = bench.load_inputs()
    sigs, strands, nreps = bench.make_batches_parallel(n, nt, 0, 16)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in ("c9orf72", "fmr1"):
        chrom, b, e, repeat, prefix, suffix = cfg["repeat"][name]
        rc.add_target(name, repeat, prefix, suffix)
    ctx = rc.ctx
    cands = rc.candidates()
    ids = [rc._classifier_for(t, s).target_id for t, s in cands]
    true_ids = [rc._classifier_for("c9orf72", s).target_id for s in strands]
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs])
    ctx.batch_upload(np.concatenate(sigs).astype(np.int16), off, true_ids)

    def leg(name, scanning):
        if scanning:
            ctx.scan_set(ids, min_score)
        try:
            ctx.batch_run(); rows = ctx.batch_fetch()          # warm-up: buffers grown once
            times, stage = [], []
            for _ in range(steps):
                t0 = time.time(); ctx.batch_run(); rows = ctx.batch_fetch(); times.append(time.time() - t0)
                stage.append(ctx.last_timing().copy())
            win = ctx.batch_fetch_scan() if scanning else None
            cnt = ctx.last_counters(); alignments = int(cnt[2])
            scr = ctx.last_screen()          # of the last sub-batch
        finally:
            if scanning:
                ctx.scan_clear()
        dt = float(np.median(times)); t = np.median(np.array(stage), axis=0)
        res = dict(leg=name, reads=n, read_nt=nt, step_ms=round(dt * 1e3, 1), reads_per_s=round(n / dt, 1), alignments=alignments,
                   cond_ms=round(float(t[5]), 1), tables_ms=round(float(t[0]), 1), forward_ms=round(float(t[1]), 1), trace_ms=round(float(t[2]), 1),
                   viterbi_ms=round(float(t[6]), 1), dp_columns=float(cnt[1]), wave_steps=float(cnt[0]),
                   last_sub_batch_screen={k: scr[k] for k in ("mode", "screened", "windowed", "whole_read", "window_columns", "coarse_pause", "fine_pause")})
        if win is not None:
            res.update(candidates=len(ids), min_score=min_score, winners=int((win >= 0).sum()),
                       true_winner=int(sum(int(w) >= 0 and ids[int(w)] == tid for w, tid in zip(win, true_ids))))
        print(json.dumps(res), flush=True)
        return rows, win

    rows_plain, _ = leg("detect", False)
    rows_scan, win = leg("scan", True)
    rows_after, _ = leg("detect_after_scan", False)
    assert rows_after.tobytes() == rows_plain.tobytes(), "a detect after a scan gives other rows"
    same = sum(int(w) >= 0 and ids[int(w)] == tid and a.tobytes() == b.tobytes() for w, tid, a, b in zip(win, true_ids, rows_plain, rows_scan))
    print(json.dumps(dict(rows_equal_to_detect=int(same), of_true_winners=int(sum(int(w) >= 0 and ids[int(w)] == tid for w, tid in zip(win, true_ids))))), flush=True)


if __name__ == "__main__":          # the reads are synthesised by spawned worker processes (bench.make_batches_parallel)
    main()
