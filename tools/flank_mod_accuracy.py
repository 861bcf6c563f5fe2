"""How often the flank methylation call of a CpG group says what was planted -- CPU oracle only, no GPU: reads of 6 kb with 10 to
30 units synthesised wholly from the mCpG k-mer table or wholly from the base table, on both bundled targets and HTT, both strands,
clean (the reference's generate_signal distribution) and with EmpiricalNoise(); the calls from tests/flank_mod_ref.py on the 150-nt
flanks.  Two stretches per flank: `whole`, the samples the alignment of the whole configured flank covers (what the tests use), and
`row`, the positions of the count row -- [prefix_begin, prefix_end) and [suffix_begin, suffix_end) -- which the flank trim has
moved to the inner 50 nt of the flank.  Reports, per noise level, stretch and planted table: the groups, the share per status, the
share of the scored groups whose ratio has the planted sign (llr > 0 on mCpG-table reads, llr < 0 on base-table reads) and the
median |llr|.  The segmentation comes from the base profile on either kind of read.  A measurement: nothing asserts a tolerance.
usage: python tools/flank_mod_accuracy.py [reads per cell]"""
import json
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import flank_mod_ref as fr  # noqa: E402
from oracle import strique_oracle as orc  # noqa: E402
from strique_amd import synth  # noqa: E402
from strique_amd.cli import parse_config  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402


def main():
    per_cell = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    golden = os.path.join(R, "tests", "golden")
    tables = np.load(os.path.join(golden, "pore_tables.npz"))
    cfg = json.load(open(os.path.join(golden, "config.json")))
    targets = {name: tuple(v[3:6]) for name, v in cfg["repeat"].items()}
    targets.update({name: tuple(v[3:6]) for name, v in parse_config(os.path.join(golden, "repeat_config_htt.tsv"))["repeat"].items()})
    base = (tables["base_kmer"], tables["base_mean"], tables["base_stdv"]); mod = (tables["mod_kmer"], tables["mod_mean"], tables["mod_stdv"])
    made_from = {"base": synth.KmerTable(pore_model(table=base)), "mod": synth.KmerTable(pore_model(table=mod))}
    opm, opm_mod = orc.PoreModel(table=base), orc.PoreModel(table=mod)
    params = orc.align_params(cfg["align"])
    orc.lib()
    empirical = synth.EmpiricalNoise()
    jobs = []
    for name, (repeat, prefix, suffix) in sorted(targets.items()):
        for strand in "+-":
            tc = orc.classifier(repeat, prefix, suffix, strand, opm, None, cfg["HMM"])
            pe, se = prefix.upper(), suffix.upper()
            if strand == "-":
                pe, se = orc.revcomp(se), orc.revcomp(pe)
            for noise_name in ("clean", "empirical"):
                for which in ("base", "mod"):
                    for k in range(per_cell):
                        rng = np.random.Generator(np.random.PCG64([len(jobs), 20261020]))
                        seq = synth.make_sequence(rng, 6000, prefix, repeat, int(rng.integers(10, 31)), suffix, strand)
                        sig = synth.make_signal(rng, made_from[which], seq, True, 0.0, empirical if noise_name == "empirical" else None)
                        jobs.append(dict(noise=noise_name, table=which, sig=sig, tc=tc, flanks=(pe, se)))

    def work(j):
        row, info = orc.detect(j["sig"], j["tc"], opm, params)
        whole = fr.flank_ranges(j["sig"], j["tc"], opm, params)
        rowpos = ((info["prefix_begin"], info["prefix_end"]), (info["suffix_begin"], info["suffix_end"]))
        out = {}
        for name, ranges in (("whole", whole), ("row", rowpos)):
            out[name] = [g for flank, (b, e) in zip(j["flanks"], ranges) if b < e
                         for g in fr.call(fr.stretch(j["sig"], opm, opm_mod, b, e), flank, opm, opm_mod, cfg["HMM"])]
        return out
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as ex:
        done = list(ex.map(work, jobs))
    cells = {}
    for j, res in zip(jobs, done):
        for stretch, groups in res.items():
            cell = cells.setdefault((j["noise"], stretch, j["table"]), dict(status=[0] * 5, llr=[]))
            for g in groups:
                cell["status"][g["status"]] += 1
                if g["status"] == fr.SCORED:
                    cell["llr"].append(g["v_mod"] - g["v_base"])
    print("noise\tstretch\tplanted\tgroups\tscored\tno_path\tedge\tskipped\ttoo_long\tas_planted\tmedian_abs_llr")
    for (noise, stretch, table), v in sorted(cells.items()):
        n = sum(v["status"]); llr = np.array(v["llr"])
        good = (llr > 0).mean() if table == "mod" else (llr < 0).mean()
        print("\t".join([noise, stretch, table, str(n)] + ["%.4f" % (s / n) for s in v["status"]] +
                        ["%.4f" % good if len(llr) else "-", "%.2f" % np.median(np.abs(llr[np.isfinite(llr)])) if np.isfinite(llr).any() else "-"]))


if __name__ == "__main__":
    main()
