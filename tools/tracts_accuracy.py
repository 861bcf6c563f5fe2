"""What the compound model (hmm.CompoundRepeatModel, strique_amd/tracts.py) makes of reads with planted tract counts, with the CPU
reference alone (tests/tract_ref.py: nets from the oracle's pieces, the oracle's detect() and Viterbi; no GPU): an HTT-like locus of
two 3-nt units and a CNBP-like one whose units differ in length, both strands, clean reads (synth.make_signal, realism 0) and reads
with EmpiricalNoise().  Prints per read the planted counts, the counts and count_j - planted_j, and the count of the one-unit model
beside them; then the table of count_j - planted_j per locus, noise and tract.
usage: python tools/tracts_accuracy.py [reads per cell] [seed]"""
import json
import os
import sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import tract_ref as tr  # noqa: E402
from oracle import strique_oracle as orc  # noqa: E402  (the checker is the subject here)
from strique_amd import synth  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402

FLANKED_REPEAT = {"htt_like": "CAG", "cnbp_like": "CCTG"}
RANGES = {"htt_like": ((8, 60), (5, 15)), "cnbp_like": ((5, 40), (4, 20), (5, 25))}


def main():
    per_cell = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    G = os.path.join(R, "tests", "golden")
    tables = np.load(os.path.join(G, "pore_tables.npz")); cfg = json.load(open(os.path.join(G, "config.json")))
    table_args = (tables["base_kmer"], tables["base_mean"], tables["base_stdv"])
    table = synth.KmerTable(pore_model(table=table_args)); opm = orc.PoreModel(table=table_args)
    params = orc.align_params(cfg["align"])
    prefix, suffix = cfg["repeat"]["c9orf72"][4].upper(), cfg["repeat"]["c9orf72"][5].upper()
    noise = synth.EmpiricalNoise()
    orc.lib()
    rng = np.random.Generator(np.random.PCG64(seed))
    jobs = []
    for name in sorted(tr.LOCI):
        units, linkers = tr.LOCI[name]
        for strand in "+-":
            tc = orc.classifier(FLANKED_REPEAT[name], prefix, suffix, strand, opm, None, cfg["HMM"])
            m = (tr.model(units, linkers, prefix[-50:], suffix[:50], strand, opm, cfg["HMM"]), strand)
            for noisy in (False, True):
                for _ in range(per_cell):
                    planted = tuple(int(rng.integers(lo, hi)) for lo, hi in RANGES[name])
                    seq = synth.make_sequence(rng, 8000, prefix, tr.array_of(units, linkers, planted), 1, suffix, strand)
                    sig = synth.make_signal(rng, table, seq, True, 0.0, noise if noisy else None)
                    jobs.append((name, strand, noisy, planted, sig, tc, m))
    with ThreadPoolExecutor(8) as ex:
        done = list(ex.map(lambda j: tr.record(j[4], j[5], j[6], opm, params), jobs))
    cells = {}
    for (name, strand, noisy, planted, sig, tc, m), (row, rec) in zip(jobs, done):
        err = None if rec is None else [c - p for c, p in zip(rec[0], planted)]
        print(json.dumps(dict(locus=name, strand=strand, noise="empirical" if noisy else "clean", planted=planted, counts=None if rec is None else list(rec[0]),
                              error=err, one_unit_count=row[0], scores=[round(row[1], 2), round(row[2], 2)])), flush=True)
        for j in range(len(planted)):
            cells.setdefault((name, "empirical" if noisy else "clean", j), []).append(None if err is None else err[j])
    print("locus\tnoise\ttract\treads\tnot_decoded\texact\twithin_1\twithin_2\tmedian\tmin\tmax\thistogram of count_j - planted_j")
    for (name, kind, j), errs in sorted(cells.items()):
        e = np.array([x for x in errs if x is not None])
        hist = " ".join("%+d:%d" % kv for kv in sorted(Counter(e.tolist()).items()))
        stats = ["-"] * 6 if not len(e) else [str(int((e == 0).sum())), str(int((abs(e) <= 1).sum())), str(int((abs(e) <= 2).sum())), "%g" % np.median(e), str(e.min()), str(e.max())]
        print("\t".join([name, kind, "%d (%s)" % (j, tr.LOCI[name][0][j]), str(len(errs)), str(len(errs) - len(e))] + stats + [hist]), flush=True)


if __name__ == "__main__":
    main()
