"""Cost of the per-unit scores (strq_set_mod_llr) on bench.py's reads with the modification model (BASELINE configs[4]: 50 kb reads,
C9orf72, --mod_model): reads/s of one resident batch with the switch off and on, alternating in the same loop on the same build; the
scoring pass's GPU time, its units and launches (strq_last_mod_llr) beside the Viterbi time of the run (strq_last_timing).
usage (GPU box): python tools/mod_llr_probe.py [n_reads] [read_nt] [steps]"""
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
    pm, cfg = bench.load_inputs()
    t = np.load(os.path.join(R, "tests", "golden", "pore_tables.npz"))
    pmm = pore_model(table=(t["mod_kmer"], t["mod_mean"], t["mod_stdv"]))
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    sigs, strands, nreps = bench.make_batches_parallel(n, nt, 0, 16)
    rc = repeatCounter(pm, mod_model_file=pmm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", repeat, prefix, suffix)
    ctx = rc.ctx
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs[:n]])
    ctx.batch_upload(np.concatenate(sigs[:n]).astype(np.int16), off, [rc._classifier_for("c9orf72", s).target_id for s in strands[:n]])
    times = {False: [], True: []}; pass_ms = []; vit_ms = []; rows = {}; mods = {}
    try:
        for on in (False, True):          # warm-up: buffers grown once, the edge image built
            ctx.set_mod_llr(on); ctx.batch_run(); ctx.batch_fetch()
        for _ in range(steps):
            for on in (False, True):
                ctx.set_mod_llr(on)
                t0 = time.time(); ctx.batch_run(); rows[on] = ctx.batch_fetch(); times[on].append(time.time() - t0)
                mods[on] = ctx.batch_fetch_mod()
                if on:
                    pass_ms.append(ctx.last_mod_llr()["ms"]); vit_ms.append(float(ctx.last_timing()[6]))
        vs = ctx.batch_fetch_mod_llr()
        info = ctx.last_mod_llr()
    finally:
        ctx.set_mod_llr(False)
    assert np.array_equal(rows[False], rows[True]) and mods[False] == mods[True], "rows or patterns changed with the switch on"
    for on in (False, True):
        dt = float(np.median(times[on]))
        print(json.dumps(dict(leg="mod_llr_on" if on else "mod_llr_off", reads=n, step_ms=round(dt * 1e3, 1), reads_per_s=round(n / dt, 1),
                              all_step_ms=[round(x * 1e3, 1) for x in times[on]])), flush=True)
    llr = np.concatenate([v[:, 1] - v[:, 0] for v in vs if v is not None]) if any(v is not None for v in vs) else np.zeros(0)
    calls = "".join(m for m in mods[True] if m != "-")
    agree = int(np.sum((llr >= -1e-9) == (np.frombuffer(calls.encode(), np.uint8) == ord("1")))) if len(llr) else 0
    print(json.dumps(dict(llr_pass_ms=round(float(np.median(pass_ms)), 1), viterbi_ms=round(float(np.median(vit_ms)), 1), units=info["units"],
                          reads_with_units=info["reads"], launches=info["launches"], sign_agrees=agree, infinite=int(np.isinf(llr).sum()),
                          abs_llr_median=float(np.median(np.abs(llr))) if len(llr) else None)), flush=True)


if __name__ == "__main__":          # the reads are synthesised by spawned worker processes (bench.make_batches_parallel)
    main()
