"""Cost of the variant pass (strq_set_variants) on bench.py's reads (50 kb reads, C9orf72) with a modification model and one alt unit
(GGCCTC): reads/s of one resident batch with the switch off and on, alternating in the same loop on the same build, and -- for scale --
with the per-unit scores of the modification pass (strq_set_mod_llr) on instead; the variant pass's GPU time, passages and launches
(strq_last_variants) beside the scoring pass's (strq_last_mod_llr) and the Viterbi time of the run (strq_last_timing).
usage (GPU box): python tools/variants_probe.py [n_reads] [read_nt] [steps]"""
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

ALT = ["GGCCTC"]


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
    rc.add_target("c9orf72", repeat, prefix, suffix, alt_units=ALT)
    rc._ensure_variants()
    ctx = rc.ctx
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs[:n]])
    ctx.batch_upload(np.concatenate(sigs[:n]).astype(np.int16), off, [rc._classifier_for("c9orf72", s).target_id for s in strands[:n]])
    legs = ("off", "variants", "mod_llr")

    def switch(leg):
        ctx.set_variants(leg == "variants"); ctx.set_mod_llr(leg == "mod_llr")

    times = {leg: [] for leg in legs}; var_ms = []; llr_ms = []; vit_ms = []; rows = {}; mods = {}
    try:
        for leg in legs:          # warm-up: buffers grown once, the edge images built
            switch(leg); ctx.batch_run(); ctx.batch_fetch()
        for _ in range(steps):
            for leg in legs:
                switch(leg)
                t0 = time.time(); ctx.batch_run(); rows[leg] = ctx.batch_fetch(); times[leg].append(time.time() - t0)
                mods[leg] = ctx.batch_fetch_mod()
                if leg == "variants":
                    var_ms.append(ctx.last_variants()["ms"]); vit_ms.append(float(ctx.last_timing()[6]))
                    info = ctx.last_variants(); var = ctx.batch_fetch_variants()
                if leg == "mod_llr":
                    llr_ms.append(ctx.last_mod_llr()["ms"]); llr_info = ctx.last_mod_llr()
    finally:
        switch("off")
    for leg in legs[1:]:
        assert np.array_equal(rows["off"], rows[leg]) and mods["off"] == mods[leg], "rows or patterns changed with the switch on"
    for leg in legs:
        dt = float(np.median(times[leg]))
        print(json.dumps(dict(leg=leg, reads=n, step_ms=round(dt * 1e3, 1), reads_per_s=round(n / dt, 1),
                              all_step_ms=[round(x * 1e3, 1) for x in times[leg]])), flush=True)
    dec = [v for v in var if v is not None]
    diff = [v[0] - int(r["count"]) for v, r in zip(var, rows["variants"]) if v is not None]
    print(json.dumps(dict(variant_pass_ms=round(float(np.median(var_ms)), 1), mod_llr_pass_ms=round(float(np.median(llr_ms)), 1),
                          viterbi_ms=round(float(np.median(vit_ms)), 1), passages=info["passages"], reads_decoded=info["reads"], launches=info["launches"],
                          mod_llr_units=llr_info["units"], alt_calls=int(sum(int((v[1] > 0).sum()) for v in dec)),
                          count_v_minus_count={str(k): int(c) for k, c in zip(*np.unique(diff, return_counts=True))} if diff else {})), flush=True)


if __name__ == "__main__":          # the reads are synthesised by spawned worker processes (bench.make_batches_parallel)
    main()
