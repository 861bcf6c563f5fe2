"""Accuracy of anchored counting on noisy reads, with the CPU oracle alone (no GPU): EmpiricalNoise reads of C9orf72 and FMR1 on both
strands, cut at a random place inside the array (keeping the part before the cut: ends_in_repeat; or the part behind it:
starts_in_repeat), decoded with the reference models of tests/anchored_ref.py.  Prints the distribution of count - truth (truth:
the complete units the read holds) and of free_samples per kind, and how many reads each threshold misclassifies.
usage: python tools/anchored_accuracy.py [reads_per_kind] [thresholds, comma separated]"""
import collections
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import anchored_ref as ar  # noqa: E402
from oracle import strique_oracle as orc  # noqa: E402  (the checker is the subject here)
from strique_amd import synth  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402


def main():
    per_kind = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    thresholds = [float(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [5.0, 6.5]
    G = os.path.join(R, "tests", "golden")
    t = np.load(os.path.join(G, "pore_tables.npz")); cfg = json.load(open(os.path.join(G, "config.json")))
    table = synth.KmerTable(pore_model(table=(t["base_kmer"], t["base_mean"], t["base_stdv"])))
    opm = orc.PoreModel(table=(t["base_kmer"], t["base_mean"], t["base_stdv"]))
    params = orc.align_params(cfg["align"]); noise = synth.EmpiricalNoise()
    rng = np.random.default_rng(2026)
    jobs = []
    for kind in (ar.ENDS, ar.STARTS):
        for i in range(per_kind):
            name = ar.TARGETS[i % 2]; strand = "+-"[(i // 2) % 2]
            target = tuple(cfg["repeat"][name][3:6])
            r, _, _, pe, se = ar.strand_sequences(*target, strand)
            n = int(rng.integers(30, 120)); L = len(r)
            left, right = ar._backbone(rng, 1200), ar._backbone(rng, 1200)
            seq = left + pe + r * n + se + right
            a0 = len(left) + len(pe)
            pos = a0 + int(rng.integers(1, n * L))
            if kind == ar.ENDS:
                seq, truth = seq[:pos], (pos - a0) // L
            else:
                seq, truth = seq[pos:], (a0 + n * L - pos) // L
            sig = synth.make_signal(rng, table, seq.encode(), True, 0.0, noise)
            tc = orc.classifier(*target, strand, opm, None, cfg["HMM"])
            jobs.append((kind, name, strand, truth, sig, tc, ar.models(*target, strand, opm, cfg["HMM"])))
    orc.lib()
    for m in thresholds:
        with ThreadPoolExecutor(8) as ex:
            recs = list(ex.map(lambda j: ar.record(j[4], j[5], j[6], opm, params, m), jobs))
        for kind in (ar.ENDS, ar.STARTS):
            mine = [(j, rec, row) for j, (row, rec) in zip(jobs, recs) if j[0] == kind]
            ok = [(j, rec) for j, rec, _ in mine if rec[0] == kind and rec[1] == 0]
            diff = collections.Counter(rec[2] - j[3] for j, rec in ok)
            free = [rec[6] for _, rec in ok]
            present = [row[1] if kind == ar.ENDS else row[2] for _, _, row in mine]; absent = [row[2] if kind == ar.ENDS else row[1] for _, _, row in mine]
            print(json.dumps(dict(threshold=m, kind=("ends_in_repeat", "starts_in_repeat")[kind - 2], reads=len(mine), misclassified=len(mine) - len(ok),
                                  as_kind=dict(collections.Counter(rec[0] for _, rec, _ in mine)), count_minus_truth=dict(sorted(diff.items())),
                                  free_samples_percentiles_0_50_90_100=[int(x) for x in np.percentile(free, [0, 50, 90, 100])] if free else [],
                                  present_score_min_median=[round(float(np.min(present)), 2), round(float(np.median(present)), 2)],
                                  absent_score_median_max=[round(float(np.median(absent)), 2), round(float(np.max(absent)), 2)])), flush=True)


if __name__ == "__main__":
    main()
