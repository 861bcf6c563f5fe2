"""What calibration recovers, on the CPU: six 8 kb reads of a bundled target are made from a table whose repeat k-mers (both strands)
are shifted by U[-3, 3] pA, decoded with the shipped table, and the k-mer levels re-estimated from the reference state statistics
(tests/state_stats_ref.py: the oracle's Viterbi path on the product's baked model, strique_amd/calibrate.py's pool and estimate) for a
few rounds.  Two legs: clean reads (the SURVEY recipe), and reads with the bundled real read's noise (synth.EmpiricalNoise) -- that
noise has no systematic per-k-mer component, so the second leg is expected to show little gain.  Prints per round the table's error
against the planted table over the planted k-mers and count - planted of every read; no GPU.
usage: python tools/calibrate_accuracy.py [target] [rounds] [min_obs]"""
import json
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import state_stats_ref as ssr  # noqa: E402
from oracle import strique_oracle as orc  # noqa: E402  (the checker is the subject here)
from strique_amd import calibrate, synth  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "c9orf72"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    min_obs = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    tables = np.load(os.path.join(R, "tests", "golden", "pore_tables.npz"))
    cfg = json.load(open(os.path.join(R, "tests", "golden", "config.json")))
    target = tuple(cfg["repeat"][name][3:6])
    planted, shift = ssr.planted_table(tables, target[0])
    truth = pore_model(table=planted).model_dict
    ptable = synth.KmerTable(pore_model(table=planted))
    for leg, noise in (("clean", None), ("empirical_noise", synth.EmpiricalNoise())):
        reads = [(synth.make_read(ptable, 9, r, 8000, target, 40 + 10 * r, strand="+-"[r % 2], noise=noise)[0], "+-"[r % 2], 40 + 10 * r) for r in range(6)]
        means = np.array(tables["base_mean"], np.float64)
        for rnd in range(rounds + 1):
            table = (planted[0], means, planted[2])
            pm = pore_model(table=table)
            err = np.array([abs(pm.model_dict[k][0] - truth[k][0]) for k in shift])
            rows, records, _ = ssr.reference_records(orc, cfg, table, target, reads)
            worst = max(shift, key=lambda k: abs(pm.model_dict[k][0] - truth[k][0]))
            print(json.dumps(dict(leg=leg, target=name, round=rnd, kmers=len(shift), mean_abs_err=round(float(err.mean()), 3), max_abs_err=round(float(err.max()), 3),
                                  worst_kmer=worst, count_minus_planted=[int(r[0]) - u for r, (_, _, u) in zip(rows, reads)], reads_with_statistics=len(records))), flush=True)
            if rnd == rounds:
                break
            new_means, _ = calibrate.estimate(calibrate.pool(records), pm, min_obs)
            means = np.array([new_means.get(k, m) for k, m in zip(planted[0], means)])


if __name__ == "__main__":
    main()
