"""Cost of anchored counting (strq_set_anchored) on bench.py's workload (BASELINE configs[2]: 50 kb reads, C9orf72): one resident
batch in which every fourth read is cut in the middle of its array (alternately keeping the part before and the part behind the
cut), run with the switch off and on alternating in one loop.  Prints reads/s of both, the pass's ms per anchored read next to the
flanked decode's ms per read of the same runs (strq_last_timing), the kernel shape the two models ran on, and the chain builder's
refusal text where it refused one.
usage (GPU box): python tools/anchored_probe.py [n_reads] [read_nt] [steps] [min_score]"""
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
    m = float(sys.argv[4]) if len(sys.argv) > 4 else 6.5          # the value the tests use; the switch has no default
    pm, cfg = bench.load_inputs()
    sigs, strands, nreps = bench.make_batches_parallel(n, nt, 0, 16)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", *cfg["repeat"]["c9orf72"][3:6])
    ctx = rc.ctx
    ids = [rc._classifier_for("c9orf72", s).target_id for s in strands]

    def upload(reads):
        off = np.zeros(len(reads) + 1, np.int64); off[1:] = np.cumsum([len(s) for s in reads])
        ctx.batch_upload(np.concatenate(reads).astype(np.int16), off, ids)

    # where the arrays are: the rows of the whole reads (offset = prefix_end, ticks = suffix_begin - prefix_end)
    upload(sigs); ctx.batch_run(); rows = ctx.batch_fetch()
    cut, want = 0, {}
    for i in range(0, n, 4):
        mid = int(rows["offset"][i] + rows["ticks"][i] // 2)
        if rows["count"][i] <= 0 or not 0 < mid < len(sigs[i]):
            continue
        keep_head = (i // 4) % 2 == 0
        sigs[i] = sigs[i][:mid] if keep_head else sigs[i][mid:]
        want[i] = 2 if keep_head else 3; cut += 1
    upload(sigs)
    rc._ensure_anchored()
    layouts = {"%d:%s" % (t, k): {"states": v["states"], "register_resident": v["positions_rc"] == 0, "refusal": v["positions_error"]}
               for t, md in rc.anchored_models.items() for k, v in md.items()}
    print(json.dumps(dict(models=layouts)), flush=True)
    res = {False: [], True: []}
    last = None
    for step in range(2 * (steps + 1)):          # off, on, off, on, ...: the first pair is the warm-up (buffers grown once)
        on = step % 2 == 1
        ctx.set_anchored(on, m)
        t0 = time.time(); ctx.batch_run(); got = ctx.batch_fetch(); dt = time.time() - t0
        t = ctx.last_timing().copy(); a = ctx.last_anchored()
        if on:
            last = ctx.batch_fetch_anchored()
        if step >= 2:
            res[on].append((dt, float(t[6]), a))
    ctx.set_anchored(False)
    out = {}
    for on in (False, True):
        dts = [r[0] for r in res[on]]; vit = [r[1] for r in res[on]]; a = res[on][-1][2]
        out["on" if on else "off"] = dict(step_ms=[round(x * 1e3, 1) for x in dts], reads_per_s=round(n / float(np.median(dts)), 1),
                                          flanked_viterbi_ms_per_read=round(float(np.median(vit)) / n, 5), anchored=a)
    a = res[True][-1][2]; anchored_reads = a["kinds"][2] + a["kinds"][3]
    out["pass_ms_per_anchored_read"] = round(float(np.median([r[2]["ms"] for r in res[True]])) / max(1, anchored_reads), 5)
    out["reads"], out["read_nt"], out["cut"], out["min_score"] = n, nt, cut, m
    out["cut_reads_classified_as_cut"] = int(sum(int(last["kind"][i]) == k for i, k in want.items()))
    dec = last[(last["kind"] >= 2) & (last["status"] == 0)]
    out["free_samples_percentiles_0_50_90_100"] = [int(x) for x in np.percentile(dec["free_samples"], [0, 50, 90, 100])] if len(dec) else []
    print(json.dumps(out), flush=True)


if __name__ == "__main__":          # the reads are synthesised by spawned worker processes (bench.make_batches_parallel)
    main()
