"""What the second normalisation step (strique_amd/renorm.py) does to the count, with the CPU oracle alone (no GPU): reads of both
bundled targets on both strands, clean (synth.make_signal, realism 0) and with EmpiricalNoise(), at repeat shares from 0.02 to 0.95,
decoded as the code stands (oracle.detect) and with the rule applied whatever the fitted share (tests/renorm_ref.detect).  Prints per
read: share, fitted share, alpha, beta, and `count (score_prefix, score_suffix)` of both; then how many reads each min_share of
0.2 ... 0.7 leaves alone, by true share; then the read the reference bundles (tests/golden/bundled_read.npz).
usage: python tools/renorm_accuracy.py [shares, comma separated] [seed]"""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import renorm_ref as rr  # noqa: E402
from oracle import strique_oracle as orc  # noqa: E402  (the checker is the subject here)
from strique_amd import renorm, synth  # noqa: E402

UNGATED = 1e-9          # every fitted read with a share above 0 is folded


def plan(share, unit_len):
    """(units, backbone nt per side) of a read of about that repeat share: 8 k nt, longer where the flanks alone would exceed the rest."""
    total = max(8000.0, 700.0 / (1.0 - share))
    units = max(2, int(round(share * total / unit_len)))
    bb = max(200, int(round((units * unit_len / share - units * unit_len - 300) / 2)))
    return units, bb


def main():
    shares = [float(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [0.02, 0.04, 0.15, 0.3, 0.45, 0.57, 0.72, 0.87, 0.93, 0.95]
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    G = os.path.join(R, "tests", "golden")
    tables = np.load(os.path.join(G, "pore_tables.npz")); cfg = json.load(open(os.path.join(G, "config.json")))
    table, opm, params = rr.setup(tables, cfg)
    noise = synth.EmpiricalNoise()
    orc.lib()
    jobs = []
    for name in ("c9orf72", "fmr1"):
        target = tuple(cfg["repeat"][name][3:6])
        for strand in "+-":
            tc = orc.classifier(*target, strand, opm, None, cfg["HMM"])
            QA = rr.target_tables(opm, target[0], strand)
            for share in shares:
                units, bb = plan(share, len(target[0]))
                for noisy in (False, True):
                    mk = (lambda rng, t, s, i16, r, nz=noise if noisy else None: synth.make_signal(rng, t, s, i16, r, nz))
                    sig = rr.make_read(table, mk, target, strand, units, bb, seed)
                    true = units * len(target[0]) / (units * len(target[0]) + 300 + 2 * bb)
                    jobs.append((name, strand, noisy, units, round(true, 3), sig, tc, QA))

    def run(j):
        name, strand, noisy, units, true, sig, tc, QA = j
        plain = orc.detect(sig, tc, opm, params)[0]
        row, rec, _ = rr.detect(sig, tc, opm, params, QA, UNGATED)
        return plain, row, rec
    with ThreadPoolExecutor(8) as ex:
        done = list(ex.map(run, jobs))
    fmt = lambda r: "%d (%.2f, %.2f)" % (r[0], r[1], r[2])
    d = renorm.grid(opm.model_min, opm.model_max)[1]
    left_alone = {}
    for (name, strand, noisy, units, true, sig, tc, QA), (plain, row, rec) in zip(jobs, done):
        f = rec[1]["filtered"]
        w = float(renorm.W[f[2]]) if f else None
        print(json.dumps(dict(target=name, strand=strand, noise="empirical" if noisy else "clean", units=units, samples=len(sig), share=true,
                              fitted_share=w, alpha=f[0] / 64 if f else None, beta_pA=round(f[1] * d, 3) if f else None,
                              as_it_stands=fmt(plain), with_the_rule=fmt(row))), flush=True)
        for m in (0.2, 0.3, 0.4, 0.5, 0.6, 0.7):
            k = left_alone.setdefault(m, {})
            k.setdefault(true, [0, 0])
            k[true][0] += int(w is None or w < m); k[true][1] += 1
    for m, by in left_alone.items():
        print(json.dumps(dict(min_share=m, left_alone_of_reads_by_share={str(s): "%d/%d" % tuple(v) for s, v in sorted(by.items())})), flush=True)
    # the read the reference bundles: C9orf72, - strand
    z = np.load(os.path.join(G, "bundled_read.npz"))
    target = tuple(cfg["repeat"]["c9orf72"][3:6])
    tc = orc.classifier(*target, "-", opm, None, cfg["HMM"])
    QA = rr.target_tables(opm, target[0], "-")
    plain = orc.detect(z["signal"], tc, opm, params)[0]
    row, rec, _ = rr.detect(z["signal"], tc, opm, params, QA, UNGATED)
    f = rec[1]["filtered"]
    print(json.dumps(dict(read="bundled", samples=int(len(z["signal"])), fitted_share=float(renorm.W[f[2]]), alpha=f[0] / 64, beta_pA=round(f[1] * d, 3),
                          as_it_stands=fmt(plain), with_the_rule=fmt(row))), flush=True)


if __name__ == "__main__":
    main()
