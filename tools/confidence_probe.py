"""Cost of the count confidence (strq_set_confidence) on bench.py's workload (BASELINE configs[2]: 50 kb reads, C9orf72): reads/s of
one resident batch with confidence off and on, alternating in the same loop on the same build; the forward pass's GPU time, its
windows and its largest rescale exponent (strq_last_confidence).
usage (GPU box): python tools/confidence_probe.py [n_reads] [read_nt] [steps]"""
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
    pm, cfg = bench.load_inputs()
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    sigs, strands, nreps = bench.make_batches_parallel(n, nt, 0, 16)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", repeat, prefix, suffix)
    ctx = rc.ctx
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs[:n]])
    ctx.batch_upload(np.concatenate(sigs[:n]).astype(np.int16), off, [rc._classifier_for("c9orf72", s).target_id for s in strands[:n]])
    times = {False: [], True: []}; fwd_ms = []; rows = {}
    try:
        for on in (False, True):          # warm-up: buffers grown once, the forward image built
            ctx.set_confidence(on); ctx.batch_run(); ctx.batch_fetch()
        for _ in range(steps):
            for on in (False, True):
                ctx.set_confidence(on)
                t0 = time.time(); ctx.batch_run(); rows[on] = ctx.batch_fetch(); times[on].append(time.time() - t0)
                if on:
                    fwd_ms.append(ctx.last_confidence()["ms"])
        conf = ctx.batch_fetch_confidence()
        info = ctx.last_confidence()
    finally:
        ctx.set_confidence(False)
    assert np.array_equal(rows[False], rows[True]), "rows changed with confidence on"
    for on in (False, True):
        dt = float(np.median(times[on]))
        print(json.dumps(dict(leg="confidence_on" if on else "confidence_off", reads=n, step_ms=round(dt * 1e3, 1), reads_per_s=round(n / dt, 1),
                              all_step_ms=[round(t * 1e3, 1) for t in times[on]])), flush=True)
    dec = [c for c in conf if c is not None]
    sd = np.array([c[2] for c in dec]); gap = np.array([c[0] for c in dec]) - np.array([float(r["log_p"]) for r, c in zip(rows[True], conf) if c is not None])
    print(json.dumps(dict(forward_pass_ms=round(float(np.median(fwd_ms)), 1), windows=info["windows"], no_path=info["no_path"],
                          max_exponent=info["max_exponent"], decoded=len(dec), count_sd_median=float(np.median(sd)), count_sd_max=float(sd.max()),
                          log_lik_minus_log_p_min=float(gap.min()))), flush=True)


if __name__ == "__main__":          # the reads are synthesised by spawned worker processes (bench.make_batches_parallel)
    main()
