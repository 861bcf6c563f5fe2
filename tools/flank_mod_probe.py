"""Cost of the flank methylation calls (strq_set_flank_mod) on one GPU: one resident batch of n_reads synthetic C9orf72 reads of
read_nt bases (20 to 99 units) with a modification model, the switch off and on alternating in one loop on the same build.  Prints ms per step of
both, and the pass's own GPU milliseconds, launches, flanks decoded and groups scored from strq_last_flank_mod.
usage (GPU box): python tools/flank_mod_probe.py [n_reads] [read_nt] [steps]"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench  # noqa: E402
from strique_amd import synth  # noqa: E402
from strique_amd.counter import repeatCounter  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    pm, cfg = bench.load_inputs()
    t = np.load(os.path.join(R, "tests", "golden", "pore_tables.npz"))
    pm_mod = pore_model(table=(t["mod_kmer"], t["mod_mean"], t["mod_stdv"]))
    table = synth.KmerTable(pm)
    target = tuple(cfg["repeat"]["c9orf72"][3:6])
    made = [synth.make_read(table, 61, i, nt, target, 20 + i % 80) for i in range(n)]          # 20 to 99 units, either strand
    sigs = [m[0] for m in made]; strands = [m[1] for m in made]
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", *cfg["repeat"]["c9orf72"][3:6])
    ctx = rc.ctx
    ids = [rc._classifier_for("c9orf72", s).target_id for s in strands]
    off = np.zeros(len(sigs) + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs])
    ctx.batch_upload(np.concatenate(sigs).astype(np.int16), off, ids)
    rc._ensure_flank_mod()
    res = {False: [], True: []}
    for step in range(2 * (steps + 1)):          # off, on, off, on, ...: the first pair is the warm-up (buffers grown once)
        on = step % 2 == 1
        ctx.set_flank_mod(on)
        t0 = time.time(); ctx.batch_run(); ctx.batch_fetch(); dt = time.time() - t0
        if step >= 2:
            res[on].append((dt, ctx.last_flank_mod()))
    ctx.set_flank_mod(False)
    out = dict(reads=n, read_nt=nt)
    for on in (False, True):
        dts = [r[0] for r in res[on]]
        out["on" if on else "off"] = dict(step_ms=[round(x * 1e3, 1) for x in dts], median_step_ms=round(float(np.median(dts)) * 1e3, 1))
    a = res[True][-1][1]
    out["pass_ms"] = round(float(np.median([r[1]["ms"] for r in res[True]])), 2)
    out["flanks"], out["groups_scored"], out["launches"] = a["flanks"], a["groups"], a["launches"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
