"""Accuracy of the variant calls and of the corrected count, on the CPU oracle alone (tests/variant_ref.py: no GPU, nothing of the
product but the read synthesis): per target (FMR1 with AGG, C9orf72 with GGCCTC), strand and kind of read (clean synthetic,
EmpiricalNoise()) N reads of 3000 nt of background around prefix + 60 units + suffix with four units replaced by the alt unit
(strique_amd.synth.make_variant_read, seeds 1000 + r).  Prints one JSON line per (target, strand, kind): how far count and count_v
are from the truth, and per read the planted units called at their exact index / within two indices, and the extra calls.
usage: python tools/variants_accuracy.py [reads per target and kind, default 40]"""
import json
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import variant_ref  # noqa: E402
from oracle import strique_oracle as orc  # noqa: E402
from strique_amd import synth  # noqa: E402
from strique_amd.pore_model import pore_model  # noqa: E402

TRUTH = 60
PROBE = (("fmr1", "AGG"), ("c9orf72", "GGCCTC"))


def hist(values):
    return {str(int(k)): int(c) for k, c in zip(*np.unique(values, return_counts=True))}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    t = np.load(os.path.join(R, "tests", "golden", "pore_tables.npz"))
    table = (t["base_kmer"], t["base_mean"], t["base_stdv"])
    pm, opm = pore_model(table=table), orc.PoreModel(table=table)
    cfg = json.load(open(os.path.join(R, "tests", "golden", "config.json")))
    params = orc.align_params(cfg["align"])
    kt = synth.KmerTable(pm)
    for locus, alt in PROBE:
        target = tuple(cfg["repeat"][locus][3:6])
        for kind in ("clean", "empirical"):
            noise = synth.EmpiricalNoise() if kind == "empirical" else None
            count_d, countv_d, exact, near, extra, undecoded = [], [], 0, 0, 0, 0
            per_strand = n // 2
            for strand in "+-":
                tc = orc.classifier(*target, strand, opm, None, cfg["HMM"])
                vm = variant_ref.VariantModel(target[0], [alt], strand, opm, cfg["HMM"])
                for r in range(per_strand):
                    sig, planted = synth.make_variant_read(1000 + r, kt, target, TRUTH, alt, strand, noise=noise)
                    ref = variant_ref.reference(sig, tc, opm, params, vm)
                    if not ref["decoded"]:
                        undecoded += 1
                        continue
                    called = [i for i, _ in variant_ref.calls(ref)]
                    count_d.append(ref["row"][0] - TRUTH); countv_d.append(ref["count_v"] - TRUTH)
                    exact += sum(p in called for p in planted)
                    hit = [p for p in planted if any(abs(p - c) <= 2 for c in called)]
                    near += len(hit)
                    extra += max(0, len(called) - len(hit))
            reads = len(count_d)
            print(json.dumps(dict(target=locus, alt=alt, kind=kind, reads=reads, undecoded=undecoded, planted=4 * reads, called_exact=exact, called_within_2=near,
                                  extra_calls=extra, count_minus_truth=hist(count_d), count_v_minus_truth=hist(countv_d),
                                  mean_abs_count=round(float(np.mean(np.abs(count_d))), 2) if reads else None,
                                  mean_abs_count_v=round(float(np.mean(np.abs(countv_d))), 2) if reads else None)), flush=True)


if __name__ == "__main__":
    main()
