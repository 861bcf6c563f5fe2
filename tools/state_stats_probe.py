"""Cost of the state-statistics pass (strq_set_state_stats) and of the state-posteriors pass (strq_set_state_posteriors) on c9orf72
reads: reads/s of one resident batch with both switches off, with the first on and with the second on, alternating in the same loop
on the same build; each pass's GPU time, its windows, launches and peak workspace bytes (strq_last_state_stats,
strq_last_state_posteriors), whether the rows changed, and how many reads got statistics.
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
    legs = ("off", "state_stats", "state_posteriors")
    times = {leg: [] for leg in legs}; pass_ms = {leg: [] for leg in legs[1:]}; rows = {}

    def switch(leg):
        ctx.set_state_stats(leg == "state_stats"); ctx.set_state_posteriors(leg == "state_posteriors")

    try:
        for leg in legs:          # warm-up: buffers grown once
            switch(leg); ctx.batch_run(); ctx.batch_fetch()
        for _ in range(steps):
            for leg in legs:
                switch(leg)
                t0 = time.time(); ctx.batch_run(); rows[leg] = ctx.batch_fetch(); times[leg].append(time.time() - t0)
                if leg == "state_stats":
                    pass_ms[leg].append(ctx.last_state_stats()["ms"])
                    if len(pass_ms[leg]) == steps:
                        t0 = time.time(); status, stats = ctx.batch_fetch_state_stats(with_status=True); fetch_ms = (time.time() - t0) * 1e3
                        info = ctx.last_state_stats()
                if leg == "state_posteriors":
                    pass_ms[leg].append(ctx.last_state_posteriors()["ms"])
                    if len(pass_ms[leg]) == steps:
                        t0 = time.time(); pstatus, pstats = ctx.batch_fetch_state_posteriors(with_status=True); pfetch_ms = (time.time() - t0) * 1e3
                        pinfo = ctx.last_state_posteriors()
    finally:
        switch("off")
    assert np.array_equal(rows["off"], rows["state_stats"]), "rows changed with the statistics on"
    assert np.array_equal(rows["off"], rows["state_posteriors"]), "rows changed with the posteriors on"
    for leg in legs:
        dt = float(np.median(times[leg]))
        print(json.dumps(dict(leg=leg if leg == "off" else leg + "_on", reads=n, read_nt=nt, step_ms=round(dt * 1e3, 1), reads_per_s=round(n / dt, 1),
                              all_step_ms=[round(t * 1e3, 1) for t in times[leg]])), flush=True)
    ms = float(np.median(pass_ms["state_stats"]))
    print(json.dumps(dict(state_stats_pass_ms=round(ms, 2), ms_per_window=round(ms / max(1, info["windows"]), 4), windows=info["windows"], launches=info["launches"],
                          bp_bytes=info["bp_bytes"], status=np.bincount(status, minlength=3).tolist(), fetch_ms=round(fetch_ms, 1),
                          observations=int(sum(int(s[0].sum()) for s in stats if s is not None)))), flush=True)
    ms = float(np.median(pass_ms["state_posteriors"]))
    obs = float(sum(float(s[0].sum()) for s in pstats if s is not None))
    print(json.dumps(dict(state_posteriors_pass_ms=round(ms, 2), ms_per_window=round(ms / max(1, pinfo["windows"]), 4), windows=pinfo["windows"],
                          launches=pinfo["launches"], ws_bytes=pinfo["ws_bytes"], status=np.bincount(pstatus, minlength=3).tolist(), fetch_ms=round(pfetch_ms, 1),
                          observations=int(round(obs)), ns_per_observation=round(ms * 1e6 / max(1.0, obs), 2))), flush=True)


if __name__ == "__main__":
    main()
