"""Cost of the second normalisation step (strq_set_renorm) on bench.py's workload (BASELINE configs[2]: C9orf72 reads of LEN nt): one
resident batch, run with the switch off and on alternating in one loop.  Prints reads/s of both, the pass's ms on the GPU per 4096
reads (strq_last_renorm) next to the conditioning time of the same runs (strq_last_timing), and how many reads were fitted / applied.
usage (GPU box): python tools/renorm_probe.py [N] [LEN] [STEPS] [min_share]"""
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
    m = float(sys.argv[4]) if len(sys.argv) > 4 else 0.4          # the switch has no default; the bench reads stay below it
    pm, cfg = bench.load_inputs()
    sigs, strands, nreps = bench.make_batches_parallel(n, nt, 0, 16)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", *cfg["repeat"]["c9orf72"][3:6])
    ctx = rc.ctx
    ids = [rc._classifier_for("c9orf72", s).target_id for s in strands]
    off = np.zeros(len(sigs) + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs])
    ctx.batch_upload(np.concatenate(sigs).astype(np.int16), off, ids)
    rc._ensure_renorm()
    res = {False: [], True: []}
    rows = {}
    for step in range(2 * (steps + 1)):          # off, on, off, on, ...: the first pair is the warm-up (buffers grown once)
        on = step % 2 == 1
        ctx.set_renorm(on, m)
        t0 = time.time(); ctx.batch_run(); got = ctx.batch_fetch(); dt = time.time() - t0
        t = ctx.last_timing().copy(); a = ctx.last_renorm()
        rows[on] = got
        if step >= 2:
            res[on].append((dt, float(t[5]), a))
    ctx.set_renorm(False)
    out = {}
    for on in (False, True):
        dts = [r[0] for r in res[on]]
        out["on" if on else "off"] = dict(step_ms=[round(x * 1e3, 1) for x in dts], reads_per_s=round(n / float(np.median(dts)), 1),
                                          conditioning_ms_per_4096=round(float(np.median([r[1] for r in res[on]])) * 4096 / n, 3), renorm=res[on][-1][2])
    out["renorm_ms_per_4096_reads"] = round(float(np.median([r[2]["ms"] for r in res[True]])) * 4096 / n, 3)
    out["reads"], out["read_nt"], out["min_share"] = n, nt, m
    out["rows_changed"] = int(np.sum(rows[True]["count"] != rows[False]["count"]))
    out["planted_count_recovered_off_on"] = [int(np.sum(rows[k]["count"] == np.asarray(nreps))) for k in (False, True)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":          # the reads are synthesised by spawned worker processes (bench.make_batches_parallel)
    main()
