#!/usr/bin/env python3
"""Gate (b) of the coarse screen's level image: what a byte scale costs in looseness -- CPU only.

For benchmark reads (bench.make_batch, all five repeat counts) and both flank alignments of each, the merged-row recurrence of
the coarse screen (tests/screen_step_ref.py: --merge 3 and / or 6 flank rows per DP row) runs over the whole read at the scales given, and its chunk values go
through the first look's rule as screen_windows_kernel states it: threshold = best chunk value - margin - 2 slack, raised until
at most max_cand chunks and four windows remain; the certificate fails when the exact optimum (the oracle's align_overlap, which
is what the exact pass finds inside windows that hold it) stays below (threshold - m v + slack) / sc.  Not modelled: the pieces'
cold starts, the lane skew of a chunk's columns, and the grouped chunk maxima (at most 3 hh per value).
Per alignment the table also counts the chunks whose value reaches the exact optimum -- what the second look (threshold: the score the
first look found, minus the slack) hands to the exact pass when the certificate fails; --max-cand sweeps the first look's cap.

    python3 tools/screen_level_looseness.py --reads 40 --scales 512 6 --out profiles/screen_level_looseness.csv
    python3 tools/screen_level_looseness.py --reads 60 --scales 6 --merge 3 6 --out profiles/screen_class_rows_looseness.csv
"""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHUNK, MAX_CAND, MAX_WIN, MERGE_GAP = 128, 8, 4, 3072
MARGIN_UNITS, SLACK_UNITS = 384.0 * 1.3, 16          # strq_ctx::coarse_margin x 1.3 (merge 3 and 6 alike); screen_plan's float32 slack


def first_look(cv, sc, m, v, margin_units, max_cand=MAX_CAND):
    """(threshold, candidates) of screen_windows_kernel's first look on the chunk values cv."""
    margin, slack = int(round(margin_units * sc)), SLACK_UNITS * sc
    vmax = int(cv.max())
    theta = vmax - margin - 2 * slack
    order = np.sort(cv)[::-1]
    if (cv >= theta).sum() > max_cand:
        theta = int(order[max_cand - 1]) if order[max_cand - 1] > order[max_cand] else int(order[max_cand - 1]) + 1

    def windows(th):
        idx = np.flatnonzero(cv >= th)
        if len(idx) == 0:
            return 0
        lo, hi = idx * CHUNK + 1, idx * CHUNK + CHUNK
        return 1 + int((lo[1:] > hi[:-1] + MERGE_GAP).sum())
    if windows(theta) > MAX_WIN:
        a, b = theta, vmax
        while b - a > 1:
            mid = a + (b - a) // 2
            if windows(mid) > MAX_WIN:
                a = mid
            else:
                b = mid
        theta = b
    return theta, int((cv >= theta).sum())


def one_read(args):
    index, scales, read_nt, margins, merges, caps = args
    import bench
    from oracle import strique_oracle as orc
    import screen_step_ref as ref
    pm, cfg = bench.load_inputs()
    sigs, strands, nreps = bench.make_batch(pm, cfg, 1, read_nt, index)
    t = np.load(os.path.join(ROOT, "tests", "golden", "pore_tables.npz"))
    opm = orc.PoreModel(table=(t["base_kmer"], t["base_mean"], t["base_stdv"]))
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    tc = orc.classifier(repeat, prefix, suffix, strands[0], opm, None, cfg["HMM"])
    params = orc.align_params(cfg["align"])
    _, u8, morph, _ = orc.condition(np.asarray(sigs[0]), opm)
    n = len(morph)
    rows = []
    for flank in ("prefix_ext", "suffix_ext"):
        seg = tc[flank]
        classes, m = seg[::ref.SAMPLES], len(seg)
        exact = float(orc.align_overlap(morph, seg, params, want_idx=False)[0])
        for sc, merge in ((sc, merge) for sc in scales for merge in merges):
            hh, v = int(round(-float(params[1]) * sc)), int(round(-float(params[3]) * sc))
            T = ref.last_row(morph.astype(np.float32), classes, params, sc, hh, v, merge)
            dec = (T - np.arange(n + 1, dtype=np.int64) * hh)[1:]
            pad = (-n) % CHUNK
            cv = np.concatenate([dec, np.full(pad, dec.min())]).reshape(-1, CHUNK).max(axis=1)
            loose = (int(cv.max()) - m * v) / sc - exact
            # the second look's threshold with the exact optimum as the score found (strq_align_api.hip: floor(b1 sc) + m v - slack)
            reach = int((cv >= np.floor(exact * sc) + m * v - SLACK_UNITS * sc).sum())
            for mu in margins:
                for cap in caps:
                    theta, ncand = first_look(cv, sc, m, v, mu, cap)
                    lower = (theta - m * v + SLACK_UNITS * sc) / sc
                    rows.append((index, nreps[0], flank[:6], n, int(u8.min()), int(u8.max()), sc, mu, exact, loose, ncand, int(exact < lower), merge, cap, reach, len(cv)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=40)
    ap.add_argument("--read-nt", type=int, default=50000)
    ap.add_argument("--scales", type=int, nargs="+", default=[512, 6])
    ap.add_argument("--margins", type=float, nargs="+", default=[MARGIN_UNITS])
    ap.add_argument("--merge", type=int, nargs="+", default=[3], choices=(1, 2, 3, 6), help="flank rows per DP row")
    ap.add_argument("--max-cand", type=int, nargs="+", default=[MAX_CAND], help="candidate cap of the first look")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from oracle import strique_oracle as orc
    orc.lib()
    with Pool(a.workers) as pool:
        parts = pool.map(one_read, [(i, a.scales, a.read_nt, a.margins, a.merge, a.max_cand) for i in range(a.reads)], chunksize=1)
    rows = [r for p in parts for r in p]
    head = "read,repeats,flank,samples,level_min,level_max,scale,margin,exact,looseness,candidates,certificate_fails,merge,max_cand,chunks_reaching_exact,chunks"
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(head + "\n")
            for r in rows:
                fp.write(",".join("%.3f" % x if isinstance(x, float) else str(x) for x in r) + "\n")
    lv = np.array([r[5] - r[4] + 1 for r in rows])
    print("alignments %d, levels used per read %d .. %d" % (len(rows) // (len(a.scales) * len(a.margins) * len(a.merge) * len(a.max_cand)), lv.min(), lv.max()))
    for sc, merge, mu, cap in ((sc, merge, mu, cap) for sc in a.scales for merge in a.merge for mu in a.margins for cap in a.max_cand):
        sel = [r for r in rows if r[6] == sc and r[7] == mu and r[12] == merge and r[13] == cap]
        lo = np.array([r[9] for r in sel])
        q = np.percentile(lo, [0, 10, 50, 90, 100])
        failing = [r[14] for r in sel if r[11]]
        print("scale %4d merge %d margin %6.1f cap %2d: looseness min %.1f p10 %.1f median %.1f p90 %.1f max %.1f mean %.1f | certificate fails %.2f %% | candidates per alignment %.3f | chunks reaching the exact optimum per failing alignment %.1f of %.0f"
              % (sc, merge, mu, cap, q[0], q[1], q[2], q[3], q[4], lo.mean(), 100.0 * np.mean([r[11] for r in sel]), np.mean([r[10] for r in sel]),
                 np.mean(failing) if failing else 0.0, np.mean([r[15] for r in sel])))


if __name__ == "__main__":
    main()
