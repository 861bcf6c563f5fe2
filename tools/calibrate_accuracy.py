"""What calibration recovers, on the CPU: six 8 kb reads of a bundled target are made from a table whose repeat k-mers (both strands)
are shifted by U[-3, 3] pA, decoded with the shipped table, and the k-mer levels re-estimated from the reference state statistics
(tests/state_stats_ref.py: the oracle's Viterbi path on the product's baked model, strique_amd/calibrate.py's pool and estimate) for a
few rounds.  Two legs: clean reads (the SURVEY recipe), and reads with the bundled real read's noise (synth.EmpiricalNoise) -- that
noise has no systematic per-k-mer component, so the second leg is expected to show little gain.  Prints per round the table's error
against the planted table over the planted k-mers and count - planted of every read; no GPU.
--posterior: the same two legs with soft assignment -- the records are the state posteriors of the tests' restatement in float64
(tests/posterior_ref.py on the oracle's un-baked model of the strand, matched to the product's states by name), pooled by
calibrate.pool_posterior; min_obs then counts expected observations.
usage: python tools/calibrate_accuracy.py [--posterior] [target] [rounds] [min_obs]"""
import json
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import state_stats_ref as ssr  # noqa: E402
from posterior_ref import emitting_names, posterior_ref  # noqa: E402
from oracle import strique_oracle as orc  # noqa: E402  (the checker is the subject here)
from strique_amd import calibrate, hmm, synth  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402


def posterior_records(cfg, table, target, reads):
    """One round of the soft check on `table`: per read the oracle's row under that table and the record calibrate.pool_posterior
    takes.  Returns (rows, records), like ssr.reference_records."""
    pm = pore_model(table=table)
    opm = orc.PoreModel(table=table)
    repeat, prefix, suffix = target
    R_, P, S = repeat.upper(), prefix[-50:].upper(), suffix[:50].upper()
    models = {"+": hmm.FlankedRepeatModel(R_, P, S, pm, cfg["HMM"]), "-": hmm.FlankedRepeatModel(ssr.revcomp(R_), ssr.revcomp(S), ssr.revcomp(P), pm, cfg["HMM"])}
    tcs = {s: orc.classifier(repeat, prefix, suffix, s, opm, None, cfg["HMM"]) for s in "+-"}
    rows, records = [], []
    for sig, strand, _ in reads:
        row, x = ssr.oracle_window(orc, opm, cfg, tcs[strand], sig)
        rows.append(row)
        if x is None or row[0] <= 0:
            continue
        ll, status, w, wx, wxx = posterior_ref(tcs[strand]["hmm"], x, np.float64)
        if status:
            continue
        on, bn = emitting_names(tcs[strand]["hmm"]), emitting_names(models[strand].baked)
        idx = np.array([on.index(nm) for nm in bn])
        records.append((models[strand].state_kmers(), w[idx], wx[idx], wxx[idx]))
    return rows, records


def main():
    argv = [a for a in sys.argv[1:] if a != "--posterior"]
    posterior = len(argv) != len(sys.argv) - 1
    name = argv[0] if len(argv) > 0 else "c9orf72"
    rounds = int(argv[1]) if len(argv) > 1 else 3
    min_obs = int(argv[2]) if len(argv) > 2 else 200
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
            rows, records = posterior_records(cfg, table, target, reads) if posterior else ssr.reference_records(orc, cfg, table, target, reads)[:2]
            worst = max(shift, key=lambda k: abs(pm.model_dict[k][0] - truth[k][0]))
            print(json.dumps(dict(leg=leg + ("/posterior" if posterior else ""), target=name, round=rnd, kmers=len(shift), mean_abs_err=round(float(err.mean()), 3), max_abs_err=round(float(err.max()), 3),
                                  worst_kmer=worst, count_minus_planted=[int(r[0]) - u for r, (_, _, u) in zip(rows, reads)], reads_with_statistics=len(records))), flush=True)
            if rnd == rounds:
                break
            new_means, _ = calibrate.estimate(calibrate.pool_posterior(records) if posterior else calibrate.pool(records), pm, min_obs)
            means = np.array([new_means.get(k, m) for k, m in zip(planted[0], means)])


if __name__ == "__main__":
    main()
