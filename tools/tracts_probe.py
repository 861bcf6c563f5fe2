"""Cost of the tract pass (strq_set_tracts) on reads of an HTT-like compound locus -- (CAG)n CAACAG (CCG)m between the C9orf72
flanks of the bundled config: reads/s of one resident batch with the switch off and on, alternating in the same loop on the same
build; the pass's GPU time, its windows and launches (strq_last_tracts), the kernel shape the compound models land on
(strq_debug_viterbi_plan), and how many reads got their planted counts back.
usage (GPU box): python tools/tracts_probe.py [n_reads] [read_nt] [steps]"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench  # noqa: E402
from strique_amd import ffi, synth, tracts  # noqa: E402
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
    sigs, strands, planted = [], [], []
    for i in range(n):
        p = (int(rng.integers(10, 60)), int(rng.integers(5, 20)))
        strand = "+-"[i % 2]
        array = "".join(u * k + l for u, k, l in zip(UNITS, p, LINKERS + ("",)))
        sigs.append(synth.make_signal(rng, table, synth.make_sequence(rng, nt, prefix, array, 1, suffix, strand), True, 0.0))
        strands.append(strand); planted.append(p)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("htt_like", "CAG", prefix, suffix, tracts=(UNITS, LINKERS))
    rc._ensure_tracts()
    ctx = rc.ctx
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs])
    ctx.batch_upload(np.concatenate(sigs).astype(np.int16), off, [rc._classifier_for("htt_like", s).target_id for s in strands])
    times = {False: [], True: []}; pass_ms = []; rows = {}
    try:
        for on in (False, True):          # warm-up: buffers grown once
            ctx.set_tracts(on); ctx.batch_run(); ctx.batch_fetch()
        for _ in range(steps):
            for on in (False, True):
                ctx.set_tracts(on)
                t0 = time.time(); ctx.batch_run(); rows[on] = ctx.batch_fetch(); times[on].append(time.time() - t0)
                if on:
                    pass_ms.append(ctx.last_tracts()["ms"])
        recs = ctx.batch_fetch_tracts()
        info = ctx.last_tracts()
    finally:
        ctx.set_tracts(False)
    assert np.array_equal(rows[False], rows[True]), "rows changed with tracts on"
    for on in (False, True):
        dt = float(np.median(times[on]))
        print(json.dumps(dict(leg="tracts_on" if on else "tracts_off", reads=n, read_nt=nt, step_ms=round(dt * 1e3, 1), reads_per_s=round(n / dt, 1),
                              all_step_ms=[round(t * 1e3, 1) for t in times[on]])), flush=True)
    exact = sum(1 for t, p, s in zip(recs, planted, strands)
                if int(t["status"]) == 0 and tracts.configured_order([int(c) for c in t["count"][:2]], s) == p)
    shapes = {s: ffi.debug_viterbi_plan(m.baked)["shape"] for _, (m, s) in rc.tract_models.items()}
    ms = float(np.median(pass_ms))
    print(json.dumps(dict(tract_pass_ms=round(ms, 2), ms_per_window=round(ms / max(1, info["windows"]), 4), windows=info["windows"], launches=info["launches"],
                          failed=info["failed"], status=np.bincount(recs["status"], minlength=4).tolist(), planted_recovered=exact,
                          window_samples_median=int(np.median([int(r["suffix_end"] - r["prefix_begin"]) for r in rows[True]])),
                          kernel_shape=shapes, states={s: m.baked.n_states for _, (m, s) in rc.tract_models.items()})), flush=True)


if __name__ == "__main__":
    main()
