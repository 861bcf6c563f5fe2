"""Cost of the motif pass (strq_set_motifs) on reads of an RFC1-like locus -- arrays of AAAAG, AAAGG or AAGGG, pure or changing over
once, between the C9orf72 flanks of the bundled config, the target configured with AAAAG: reads/s of one resident batch with the
switch off and on, alternating in the same loop on the same build; the pass's GPU time, its reads, segments, launches and majority
decodes (strq_last_motifs) beside the Viterbi time of the same run, and how many pure-array reads got their planted unit as majority.
usage (GPU box): python tools/motifs_probe.py [n_reads] [read_nt] [steps] [segment]"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench  # noqa: E402
from strique_amd import motifs, synth  # noqa: E402
from strique_amd.counter import repeatCounter  # noqa: E402

UNITS = ("AAAAG", "AAAGG", "AAGGG")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    segment = int(sys.argv[4]) if len(sys.argv) > 4 else motifs.SEGMENT
    pm, cfg = bench.load_inputs()
    prefix, suffix = cfg["repeat"]["c9orf72"][4:6]
    table = synth.KmerTable(pm)
    rng = np.random.Generator(np.random.PCG64(2026))
    sigs, strands, planted = [], [], []
    for i in range(n):
        a, b = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        strand = "+-"[i % 2]
        array = UNITS[a] * int(rng.integers(15, 60)) + (UNITS[b] * int(rng.integers(15, 60)) if i % 4 == 3 else "")
        sigs.append(synth.make_signal(rng, table, synth.make_sequence(rng, nt, prefix, array, 1, suffix, strand), True, 0.0))
        strands.append(strand); planted.append(a if i % 4 != 3 else None)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("rfc1_like", UNITS[0], prefix, suffix, motifs=list(UNITS[1:]))
    rc._ensure_motifs()
    ctx = rc.ctx
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs])
    ctx.batch_upload(np.concatenate(sigs).astype(np.int16), off, [rc._classifier_for("rfc1_like", s).target_id for s in strands])
    times = {False: [], True: []}; pass_ms = []; vit_ms = []; rows = {}
    try:
        for on in (False, True):          # warm-up: buffers grown once
            ctx.set_motifs(on, segment); ctx.batch_run(); ctx.batch_fetch()
        for _ in range(steps):
            for on in (False, True):
                ctx.set_motifs(on, segment)
                t0 = time.time(); ctx.batch_run(); rows[on] = ctx.batch_fetch(); times[on].append(time.time() - t0)
                if on:
                    pass_ms.append(ctx.last_motifs()["ms"]); vit_ms.append(float(ctx.last_timing()[6]))
        recs, _, _ = ctx.batch_fetch_motifs()
        info = ctx.last_motifs()
    finally:
        ctx.set_motifs(False)
    assert np.array_equal(rows[False], rows[True]), "rows changed with motifs on"
    for on in (False, True):
        dt = float(np.median(times[on]))
        print(json.dumps(dict(leg="motifs_on" if on else "motifs_off", reads=n, read_nt=nt, step_ms=round(dt * 1e3, 1), reads_per_s=round(n / dt, 1),
                              all_step_ms=[round(t * 1e3, 1) for t in times[on]])), flush=True)
    pure = [(r, p) for r, p in zip(recs, planted) if p is not None and int(r["status"]) == 0]
    ms = float(np.median(pass_ms))
    print(json.dumps(dict(motif_pass_ms=round(ms, 2), viterbi_ms_of_the_run=round(float(np.median(vit_ms)), 2), segment=segment, reads=info["reads"],
                          segments=info["segments"], launches=info["launches"], majority_decodes=info["decodes"],
                          status=np.bincount(recs["status"], minlength=2).tolist(), pure_arrays=len(pure),
                          majority_is_planted=sum(1 for r, p in pure if int(r["majority"]) == p),
                          stretch_samples_median=int(np.median([int(r["end"] - r["begin"]) for r in recs if int(r["status"]) == 0] or [0])))), flush=True)


if __name__ == "__main__":
    main()
