"""Cost of the methylation calls of anchored reads (strq_set_anchored_mod) on bench.py's workload (BASELINE configs[2]: 50 kb reads,
C9orf72) with a modification model: one resident batch in which every fourth read is cut in the middle of its array (alternately
keeping the part before and the part behind the cut), anchored counting on throughout, the switch off and on alternating in one
loop.  Prints ms per step of both, the pass's own ms (strq_last_anchored_mod), and the reads and units it called.
usage (GPU box): python tools/anchored_mod_probe.py [n_reads] [read_nt] [steps] [min_score]"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench  # noqa: E402
from strique_amd.counter import repeatCounter  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    m = float(sys.argv[4]) if len(sys.argv) > 4 else 6.5          # the value the tests use; the switch has no default
    pm, cfg = bench.load_inputs()
    t = np.load(os.path.join(R, "tests", "golden", "pore_tables.npz"))
    pm_mod = pore_model(table=(t["mod_kmer"], t["mod_mean"], t["mod_stdv"]))
    sigs, strands, nreps = bench.make_batches_parallel(n, nt, 0, 16)
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", *cfg["repeat"]["c9orf72"][3:6])
    ctx = rc.ctx
    ids = [rc._classifier_for("c9orf72", s).target_id for s in strands]

    def upload(reads):
        off = np.zeros(len(reads) + 1, np.int64); off[1:] = np.cumsum([len(s) for s in reads])
        ctx.batch_upload(np.concatenate(reads).astype(np.int16), off, ids)

    # where the arrays are: the rows of the whole reads (offset = prefix_end, ticks = suffix_begin - prefix_end)
    upload(sigs); ctx.batch_run(); rows = ctx.batch_fetch()
    cut = 0
    for i in range(0, n, 4):
        mid = int(rows["offset"][i] + rows["ticks"][i] // 2)
        if rows["count"][i] <= 0 or not 0 < mid < len(sigs[i]):
            continue
        sigs[i] = sigs[i][:mid] if (i // 4) % 2 == 0 else sigs[i][mid:]
        cut += 1
    upload(sigs)
    rc._ensure_anchored()
    ctx.set_anchored(True, m)
    res = {False: [], True: []}
    calls = None
    for step in range(2 * (steps + 1)):          # off, on, off, on, ...: the first pair is the warm-up (buffers grown once)
        on = step % 2 == 1
        ctx.set_anchored_mod(on)
        t0 = time.time(); ctx.batch_run(); ctx.batch_fetch(); dt = time.time() - t0
        a = ctx.last_anchored_mod(); b = ctx.last_anchored()
        if on:
            calls = ctx.batch_fetch_anchored_mod()
        if step >= 2:
            res[on].append((dt, a, b))
    ctx.set_anchored_mod(False); ctx.set_anchored(False)
    out = dict(reads=n, read_nt=nt, cut=cut, min_score=m)
    for on in (False, True):
        dts = [r[0] for r in res[on]]
        out["on" if on else "off"] = dict(step_ms=[round(x * 1e3, 1) for x in dts], median_step_ms=round(float(np.median(dts)) * 1e3, 1),
                                          anchored_pass_ms=round(float(np.median([r[2]["ms"] for r in res[on]])), 2))
    a = res[True][-1][1]
    out["pass_ms"] = round(float(np.median([r[1]["ms"] for r in res[True]])), 2)
    out["reads_called"], out["units_called"], out["launches"] = a["reads"], a["units"], a["launches"]
    pats = [c[0] for c in calls if c is not None and c[0] != "-"]
    out["share_of_1"] = round(sum(p.count("1") for p in pats) / max(1, sum(len(p) for p in pats)), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":          # the reads are synthesised by spawned worker processes (bench.make_batches_parallel)
    main()
