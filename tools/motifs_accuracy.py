"""What the motif track (strique_amd/motifs.py) makes of reads with a planted array, with the CPU reference alone (tests/motif_ref.py:
loop nets from the oracle's pieces, the oracle's detect() and Viterbi; no GPU): c9orf72's flanks around pure arrays of every candidate
and around mixed arrays, both strands, clean reads (synth.make_signal, realism 0) and reads with EmpiricalNoise().  Prints per read the
majority, the shares, the runs, the smallest per-observation margin and count_m beside the row's count; then per noise kind the segments
whose winner is the unit planted at their midpoint (the array's unit boundaries laid over the stretch in proportion to their bases).
usage: python tools/motifs_accuracy.py [segment]"""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import motif_ref as mr  # noqa: E402
from oracle import strique_oracle as orc  # noqa: E402  (the checker is the subject here)
from strique_amd import synth  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402

SETS = {"rfc1": ("AAAAG", "AAAGG", "AAGGG"), "fgf14": ("GAA", "GAAGGA"), "fame": ("TTTTA", "TTTCA")}
MIXED = {"rfc1": [((0, 30), (2, 30)), ((2, 25), (1, 25), (0, 25))], "fame": [((0, 40), (1, 40), (0, 40))], "fgf14": [((0, 50), (1, 30))]}


def planted_at(array, units, strand, frac):
    """The candidate planted at fraction `frac` of the stretch, in signal order."""
    spans = [(j, len(units[j]) * n) for j, n in array]
    if strand == '-':
        spans = spans[::-1]
    total = sum(n for _, n in spans)
    at = frac * total
    for j, n in spans:
        if at < n:
            return j
        at -= n
    return spans[-1][0]


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    G = os.path.join(R, "tests", "golden")
    tables = np.load(os.path.join(G, "pore_tables.npz")); cfg = json.load(open(os.path.join(G, "config.json")))
    table_args = (tables["base_kmer"], tables["base_mean"], tables["base_stdv"])
    table = synth.KmerTable(pore_model(table=table_args)); opm = orc.PoreModel(table=table_args)
    params = orc.align_params(cfg["align"])
    prefix, suffix = cfg["repeat"]["c9orf72"][4].upper(), cfg["repeat"]["c9orf72"][5].upper()
    noise = synth.EmpiricalNoise()
    orc.lib()
    cases = [(name, ((j, 40),)) for name in SETS for j in range(len(SETS[name]))] + [(name, a) for name in SETS for a in MIXED[name]]
    jobs = []
    for noisy in (False, True):
        i = 0
        for name, array in cases:
            for strand in "+-":
                i += 1
                rng = np.random.Generator(np.random.PCG64(9000 + i))
                units = SETS[name]
                seq = synth.make_sequence(rng, 8000, prefix, "".join(units[j] * n for j, n in array), 1, suffix, strand)
                sig = synth.make_signal(rng, table, seq, True, 0.0, noise=noise if noisy else None)
                jobs.append((noisy, name, array, strand, sig))
    with ThreadPoolExecutor(8) as ex:
        done = list(ex.map(lambda j: mr.record(j[4], SETS[j[1]][0], SETS[j[1]][1:], prefix, suffix, j[3], opm, params, cfg["HMM"], S), jobs))
    tally = {}
    for (noisy, name, array, strand, sig), (row, rec) in zip(jobs, done):
        kind = "empirical" if noisy else "clean"
        if rec is None:
            print(json.dumps(dict(noise=kind, locus=name, array=array, strand=strand, row_count=row[0], motifs=None)), flush=True)
            continue
        majority, shares, count_m, log_p_m, runs, win, V, bounds = rec
        T = bounds[-1][1]
        top = np.sort(V, axis=1)[:, ::-1]
        margin = (top[:, 0] - top[:, 1]) / np.array([e - b for b, e in bounds])
        want = [planted_at(array, SETS[name], strand, (b + e) / 2 / T) for b, e in bounds]
        hit = sum(1 for w, p in zip(win, want) if w == p)
        t = tally.setdefault(kind, [0, 0, np.inf, np.inf])
        t[0] += len(win); t[1] += hit; t[3] = min(t[3], float(margin.min()))
        if len(array) == 1:
            t[2] = min(t[2], float(margin.min()))
        print(json.dumps(dict(noise=kind, locus=name, array=[(SETS[name][j], n) for j, n in array], strand=strand, row_count=row[0], majority=SETS[name][majority],
                              shares=[round(s, 4) for s in shares], count_m=count_m, segments=len(win), planted_at_midpoint=hit,
                              min_margin=round(float(margin.min()), 3), runs=[(SETS[name][c], a, b) for c, a, b in runs])), flush=True)
    print("noise\tsegments\twinner_is_planted_unit\tmin_margin_pure_arrays\tmin_margin_all")
    for kind, (n, hit, m_pure, m_all) in sorted(tally.items()):
        print("%s\t%d\t%d\t%.3f\t%.3f" % (kind, n, hit, m_pure, m_all), flush=True)


if __name__ == "__main__":
    main()
