#!/usr/bin/env python3
"""Six benchmark steps (three batches of 4096 reads of 50 kb, each twice) through detect_batch: what the coarse screen's first look
left to the second (strq_last_screen_mode [5]), the whole-read second round, candidate chunks per alignment, the layout and scale
that ran -- and every row of every step, saved so that two libraries (STRQ_LIB) can be compared byte for byte:

    python3 tools/screen_six_steps.py --out a.npy;  STRQ_LIB=/other/libstrique_hip.so python3 tools/screen_six_steps.py --out b.npy
    python3 tools/screen_six_steps.py --compare a.npy b.npy
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default="")
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        x, y = np.load(a.compare[0]), np.load(a.compare[1])
        same = x.shape == y.shape and x.tobytes() == y.tobytes()
        print(json.dumps({"rows": int(x.shape[0]), "fields": int(x.shape[1]), "byte_equal": bool(same),
                          "rows_that_differ": int((x.view(np.uint64) != y.view(np.uint64)).any(axis=1).sum()) if x.shape == y.shape else None}))
        sys.exit(0 if same else 1)
    import bench
    from strique_amd.counter import repeatCounter
    pm, cfg = bench.load_inputs()
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    sigs, strands, _ = bench.make_batches_parallel(a.batches * a.reads, 50000, 0, a.workers)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", repeat, prefix, suffix)
    tot = dict(second_look=0, second_round=0, alignments=0, candidate_chunks=0.0, screened=0.0)
    rows, per_step = [], []
    for k in range(a.steps):
        lo = (k % a.batches) * a.reads
        got = rc.detect_batch([("c9orf72", s, st) for s, st in zip(sigs[lo:lo + a.reads], strands[lo:lo + a.reads])])
        s, sr = rc.ctx.last_screen(), rc.ctx.last_second_round()
        tot["second_look"] += s["second_look"]; tot["second_round"] += sr[0]; tot["alignments"] += sr[1]
        tot["candidate_chunks"] += s["candidate_chunks"]; tot["screened"] += s["screened"]
        per_step.append(dict(mode=s["mode"], layout=s["lds_layout"], scale=s["scale"], second_look=s["second_look"], second_round=sr[0]))
        rows += [[float(v) for v in g[:6]] for g in got]
    rc.ctx.close()
    tot["candidate_chunks_per_alignment"] = tot["candidate_chunks"] / max(1.0, tot["screened"])
    tot["second_look_share"] = tot["second_look"] / max(1.0, tot["screened"])
    print(json.dumps(dict(total=tot, steps=per_step)))
    if a.out:
        np.save(a.out, np.asarray(rows, np.float64))


if __name__ == "__main__":
    main()
