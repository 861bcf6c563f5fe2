"""How often the methylation call of an anchored read says what was planted -- CPU oracle only, no GPU: reads synthesised wholly from
the mCpG k-mer table or wholly from the base table, cut inside an array of 30 to 120 units (keeping the part before or the part
behind the cut), clean (the reference's generate_signal distribution) and with EmpiricalNoise(); the anchored record from
tests/anchored_ref.py, the call from tests/anchored_mod_ref.py.  Reports, per noise level, planted table and kind, the reads that
qualified and the share of their units called as planted.  A measurement: nothing asserts a tolerance on it.
usage: python tools/anchored_mod_accuracy.py [reads per cell] [min_score]"""
import json
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import anchored_mod_ref as amr  # noqa: E402
import anchored_ref as ar  # noqa: E402
from oracle import strique_oracle as orc  # noqa: E402
from strique_amd import synth  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402


def main():
    per_cell = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    m = float(sys.argv[2]) if len(sys.argv) > 2 else 6.5
    tables = np.load(os.path.join(R, "tests", "golden", "pore_tables.npz"))
    cfg = json.load(open(os.path.join(R, "tests", "golden", "config.json")))
    base = (tables["base_kmer"], tables["base_mean"], tables["base_stdv"]); mod = (tables["mod_kmer"], tables["mod_mean"], tables["mod_stdv"])
    made_from = {"base": synth.KmerTable(pore_model(table=base)), "mod": synth.KmerTable(pore_model(table=mod))}
    opm, opm_mod = orc.PoreModel(table=base), orc.PoreModel(table=mod)
    params = orc.align_params(cfg["align"])
    orc.lib()
    jobs = []
    empirical = synth.EmpiricalNoise()
    for name in ar.TARGETS:
        target = tuple(cfg["repeat"][name][3:6])
        for strand in "+-":
            tc = orc.classifier(*target, strand, opm, opm_mod, cfg["HMM"])
            mods = ar.models(*target, strand, opm, cfg["HMM"])
            r, _, _, pe, se = ar.strand_sequences(*target, strand)
            for noise_name in ("clean", "empirical"):
                for which in ("base", "mod"):
                    for kind in (ar.ENDS, ar.STARTS):
                        for k in range(per_cell):
                            rng = np.random.Generator(np.random.PCG64([len(jobs), 20261020]))
                            n_units = int(rng.integers(30, 121))
                            left, right = ar._backbone(rng, ar.FLANK_BACKBONE), ar._backbone(rng, ar.FLANK_BACKBONE)
                            a0 = len(left) + len(pe)
                            cut = a0 + int(rng.integers(5, n_units - 4)) * len(r) + int(rng.integers(0, len(r)))
                            seq = left + pe + r * n_units + se + right
                            seq = seq[:cut] if kind == ar.ENDS else seq[cut:]
                            noise = empirical if noise_name == "empirical" else None
                            sig = synth.make_signal(rng, made_from[which], seq.encode(), True, 0.0, noise)
                            jobs.append(dict(noise=noise_name, table=which, kind=kind, sig=sig, tc=tc, mods=mods))

    def work(j):
        _, rec = ar.record(j["sig"], j["tc"], j["mods"], opm, params, m)
        return rec, amr.call(j["sig"], rec, j["tc"], opm, llr=False)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as ex:
        done = list(ex.map(work, jobs))
    cells = {}
    for j, (rec, c) in zip(jobs, done):
        cell = cells.setdefault((j["noise"], j["table"], j["kind"]), dict(reads=0, kind_found=0, called=0, units=0, as_planted=0))
        cell["reads"] += 1
        cell["kind_found"] += rec[0] == j["kind"]
        if c is None or rec[0] != j["kind"] or c[0] == "-":
            continue
        cell["called"] += 1; cell["units"] += len(c[0]); cell["as_planted"] += c[0].count("1" if j["table"] == "mod" else "0")
    print("noise\tplanted\tkind\treads\tkind_found\tcalled\tunits\tas_planted\tshare")
    for (noise, table, kind), v in sorted(cells.items()):
        print("\t".join([noise, table, ("ends_in_repeat", "starts_in_repeat")[kind - 2], str(v["reads"]), str(v["kind_found"]), str(v["called"]), str(v["units"]),
                         str(v["as_planted"]), "%.4f" % (v["as_planted"] / v["units"]) if v["units"] else "-"]))


if __name__ == "__main__":
    main()
