"""Cost of the state-statistics pass (strq_set_state_stats) on c9orf72 reads: reads/s of one resident batch with the switch off and
on, alternating in the same loop on the same build; the pass's GPU time, its windows, launches and peak back-pointer bytes
(strq_last_state_stats), whether the rows changed, and how many reads got statistics.
usage (GPU box): python tools/state_stats_probe.py [n_reads] [read_nt] [steps]"""
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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    pm, cfg = bench.load_inputs()
    target = tuple(cfg["repeat"]["c9orf72"][3:6])
    table = synth.KmerTable(pm)
    rng = np.random.Generator(np.random.PCG64(2026))
    sigs, strands = [], []
    for i in range(n):
        strand = "+-"[i % 2]
        sigs.append(synth.make_read(table, 11, i, nt, target, int(rng.integers(10, 200)), strand=strand)[0])
        strands.append(strand)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", *target)
    ctx = rc.ctx
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs])
    tids = [rc._classifier_for("c9orf72", s).target_id for s in strands]
    ctx.batch_upload(np.concatenate(sigs).astype(np.int16), off, tids)
    times = {False: [], True: []}; pass_ms = []; rows = {}
    try:
        for on in (False, True):          # warm-up: buffers grown once
            ctx.set_state_stats(on); ctx.batch_run(); ctx.batch_fetch()
        for _ in range(steps):
            for on in (False, True):
                ctx.set_state_stats(on)
                t0 = time.time(); ctx.batch_run(); rows[on] = ctx.batch_fetch(); times[on].append(time.time() - t0)
                if on:
                    pass_ms.append(ctx.last_state_stats()["ms"])
        t0 = time.time(); status, stats = ctx.batch_fetch_state_stats(with_status=True); fetch_ms = (time.time() - t0) * 1e3
        info = ctx.last_state_stats()
    finally:
        ctx.set_state_stats(False)
    assert np.array_equal(rows[False], rows[True]), "rows changed with the statistics on"
    for on in (False, True):
        dt = float(np.median(times[on]))
        print(json.dumps(dict(leg="state_stats_on" if on else "state_stats_off", reads=n, read_nt=nt, step_ms=round(dt * 1e3, 1), reads_per_s=round(n / dt, 1),
                              all_step_ms=[round(t * 1e3, 1) for t in times[on]])), flush=True)
    ms = float(np.median(pass_ms))
    print(json.dumps(dict(state_stats_pass_ms=round(ms, 2), ms_per_window=round(ms / max(1, info["windows"]), 4), windows=info["windows"], launches=info["launches"],
                          bp_bytes=info["bp_bytes"], status=np.bincount(status, minlength=3).tolist(), fetch_ms=round(fetch_ms, 1),
                          observations=int(sum(int(s[0].sum()) for s in stats if s is not None)))), flush=True)


if __name__ == "__main__":
    main()
