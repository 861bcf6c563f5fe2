"""Cost of the repeat-unit positions (strq_set_units) on bench.py's workload (BASELINE configs[2]: 50 kb reads, C9orf72): reads/s of
one resident batch with units off, with units on (unit records), and with units on through the back-pointer route
(STRQ_UNITS_BACKPOINTERS=1); the unit pass's GPU time and its largest record workspace (strq_last_units).
usage (GPU box): python tools/units_probe.py [n_reads] [read_nt] [steps] [bp_reads]
(bp_reads: reads of the back-pointer leg -- ~180 MB of back-pointers per read, pieces of STRQ_UNITS_WS_BYTES)"""
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
    n_bp = int(sys.argv[4]) if len(sys.argv) > 4 else 256
    pm, cfg = bench.load_inputs()
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    sigs, strands, nreps = bench.make_batches_parallel(n, nt, 0, 16)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", repeat, prefix, suffix)
    ctx = rc.ctx

    def leg(name, k, units, options=()):
        off = np.zeros(k + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs[:k]])
        ctx.batch_upload(np.concatenate(sigs[:k]).astype(np.int16), off, [rc._classifier_for("c9orf72", s).target_id for s in strands[:k]])
        for key, v in options:
            ctx.set_option(key, v)
        ctx.set_units(units)
        try:
            ctx.batch_run(); rows = ctx.batch_fetch()          # warm-up: buffers grown once
            times, unit_ms = [], []
            for _ in range(steps):
                t0 = time.time(); ctx.batch_run(); rows = ctx.batch_fetch(); times.append(time.time() - t0)
                unit_ms.append(ctx.last_units()["ms"] if units else 0.0)
            pos = ctx.batch_fetch_units() if units else None
            info = ctx.last_units() if units else {}
        finally:
            ctx.set_units(False)
            for key, _ in options:
                ctx.set_option(key, "")
        dt = float(np.median(times))
        res = dict(leg=name, reads=k, step_ms=round(dt * 1e3, 1), reads_per_s=round(k / dt, 1), unit_pass_ms=round(float(np.median(unit_ms)), 1),
                   record_bytes=info.get("ws_bytes", 0), windows=info.get("windows", 0), positions=info.get("positions", 0),
                   vit_ms=round(float(ctx.last_timing()[6]), 1))
        if pos is not None:
            res["decoded"] = sum(p is not None for p in pos)
            res["len_ok"] = sum(p is not None and len(p) == int(r["count"]) - rc._classifier_for("c9orf72", s).repeatHMM.count_bias
                                for p, r, s in zip(pos, rows, strands[:k]))
        print(json.dumps(res), flush=True)
        return rows, pos

    rows_off, _ = leg("units_off", n, False)
    rows_on, pos_on = leg("units_on", n, True)
    assert np.array_equal(rows_off, rows_on), "rows changed with units on"
    _, pos_bp = leg("units_backpointers", n_bp, True, (("STRQ_UNITS_BACKPOINTERS", "1"),))
    same = all((a is None and b_ is None) or (a is not None and b_ is not None and np.array_equal(a, b_)) for a, b_ in zip(pos_on[:n_bp], pos_bp))
    print(json.dumps(dict(record_route_equals_backpointers=bool(same), reads_compared=n_bp)), flush=True)


if __name__ == "__main__":          # the reads are synthesised by spawned worker processes (bench.make_batches_parallel)
    main()
