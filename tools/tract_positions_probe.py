"""Cost of the tract-position pass (strq_set_tract_positions) on reads of an HTT-like compound locus -- (CAG)n CAACAG (CCG)m between
the C9orf72 flanks of the bundled config, as tools/tracts_probe.py builds them: reads/s of one resident batch with the tract pass on
and the positions off and on, alternating in the same loop on the same build; the pass's GPU time, its windows, launches and peak
back-pointer bytes (strq_last_tract_positions), and whether every tract got count - bias positions.
usage (GPU box): python tools/tract_positions_probe.py [n_reads] [read_nt] [steps]"""
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

UNITS, LINKERS = ("CAG", "CCG"), ("CAACAG",)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    pm, cfg = bench.load_inputs()
    prefix, suffix = cfg["repeat"]["c9orf72"][4:6]
    table = synth.KmerTable(pm)
    rng = np.random.Generator(np.random.PCG64(2026))
    sigs, strands = [], []
    for i in range(n):
        p = (int(rng.integers(10, 60)), int(rng.integers(5, 20)))
        strand = "+-"[i % 2]
        array = "".join(u * k + l for u, k, l in zip(UNITS, p, LINKERS + ("",)))
        sigs.append(synth.make_signal(rng, table, synth.make_sequence(rng, nt, prefix, array, 1, suffix, strand), True, 0.0))
        strands.append(strand)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("htt_like", "CAG", prefix, suffix, tracts=(UNITS, LINKERS))
    rc._ensure_tracts()
    ctx = rc.ctx
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs])
    tids = [rc._classifier_for("htt_like", s).target_id for s in strands]
    ctx.batch_upload(np.concatenate(sigs).astype(np.int16), off, tids)
    times = {False: [], True: []}; pass_ms = []; rows = {}; recs = {}
    try:
        ctx.set_tracts(True)
        for on in (False, True):          # warm-up: buffers grown once
            ctx.set_tract_positions(on); ctx.batch_run(); ctx.batch_fetch()
        for _ in range(steps):
            for on in (False, True):
                ctx.set_tract_positions(on)
                t0 = time.time(); ctx.batch_run(); rows[on] = ctx.batch_fetch(); times[on].append(time.time() - t0)
                recs[on] = ctx.batch_fetch_tracts()
                if on:
                    pass_ms.append(ctx.last_tract_positions()["ms"])
        pos = ctx.batch_fetch_tract_positions()
        info = ctx.last_tract_positions()
    finally:
        ctx.set_tract_positions(False); ctx.set_tracts(False)
    assert np.array_equal(rows[False], rows[True]) and recs[False].tobytes() == recs[True].tobytes(), "rows or tract records changed with the positions on"
    for on in (False, True):
        dt = float(np.median(times[on]))
        print(json.dumps(dict(leg="positions_on" if on else "positions_off", reads=n, read_nt=nt, step_ms=round(dt * 1e3, 1), reads_per_s=round(n / dt, 1),
                              all_step_ms=[round(t * 1e3, 1) for t in times[on]])), flush=True)
    bias = {tid: rc.tract_models[tid][0].count_bias for tid in set(tids)}
    whole = sum(1 for t, (ps, p), tid in zip(recs[True], pos, tids)
                if int(t["status"]) == 0 and ps == 0 and all(len(p[j]) == int(t["count"][j]) - bias[tid][j] for j in range(int(t["n_tracts"]))))
    ms = float(np.median(pass_ms))
    print(json.dumps(dict(position_pass_ms=round(ms, 2), ms_per_window=round(ms / max(1, info["windows"]), 4), windows=info["windows"], launches=info["launches"],
                          bp_bytes=info["bp_bytes"], pos_status=np.bincount([ps for ps, _ in pos], minlength=3).tolist(), reads_with_all_positions=whole,
                          positions=int(sum(len(q) for ps, p in pos if p is not None for q in p)))), flush=True)


if __name__ == "__main__":
    main()
