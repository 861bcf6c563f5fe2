"""Reference of the methylation calls of anchored reads for the tests, from the oracle alone: the anchored record of
tests/anchored_ref.py, then, on the raw-signal samples [begin, end) of that record, the oracle's mod_repeats (STRique.py:492-500) on
the minmax-normalised RAW signal, and the per-unit pairs (V_base, V_mod) through the masked-model Viterbi of tests/mod_llr_ref.py on
the unit bounds of that path.  Nothing of the product is imported here but the signal synthesis (the reads are inputs).

The reads: anchored_ref.make_case for both bundled targets, both strands and all seven cuts, each synthesised once from the base
k-mer table and once from the mCpG table -- 56 reads as int16; the C9orf72 ones also as float64 (28).  The cuts are the smallest
shapes at which this can go wrong: a stretch of zero units (in_prefix, one_base_in), one that ends mid-unit, one that ends right
behind a unit, a start three bases into the array."""
import numpy as np

import anchored_ref as ar
import mod_llr_ref
from oracle import strique_oracle as orc

SEED = 1              # chosen so that the oracle alone meets the preconditions of tests/test_anchored_mod_host.py on every read
M = ar.M
TABLES = ("base", "mod")
# the cuts that leave a stretch of many units inside the array ("mid-array"); start_in_first holds nearly the whole array
MID_CUTS = ("mid_unit", "behind_unit", "before_array_end", "start_mid")
_CASES = {}
_MASKS = {}


def qualifies(rec, has_mod_model=True):
    """The rule, restated: kind 2 / 3, status 0, begin < end, a target with a modification model."""
    return has_mod_model and rec[0] in (ar.ENDS, ar.STARTS) and rec[1] == 0 and rec[4] < rec[5]


def call(sig, rec, tc, opm, llr=True):
    """None, or (pattern, V (n, 2) float64 of (V_base, V_mod), x) of one read with anchored record `rec`; V has no rows when the
    pattern is '-'."""
    if not qualifies(rec, tc.get("mod") is not None):
        return None
    nrm = opm.normalize_minmax(np.asarray(sig).astype(np.float64))
    stretch = nrm[rec[4]:rec[5]]
    model = tc["mod"]
    pattern = orc.mod_repeats(model, tc["mod_range"], stretch)
    x = np.clip(stretch, tc["mod_range"][0], tc["mod_range"][1])
    if pattern == "-" or not llr:
        return pattern, np.zeros((0, 2)), x
    _, mpath, _ = orc.viterbi(model, x)
    bounds = mod_llr_ref.unit_bounds(model, mpath)
    assert len(bounds) == len(pattern)
    if id(model) not in _MASKS:
        _MASKS[id(model)] = (model, mod_llr_ref.masked(model, 0), mod_llr_ref.masked(model, 1))
    _, m_base, m_mod = _MASKS[id(model)]
    V = np.zeros((len(bounds), 2))
    for j, (u, w) in enumerate(bounds):
        V[j, 0] = orc.viterbi(m_base, x[u:w + 1], want_path=False)[0]
        V[j, 1] = orc.viterbi(m_mod, x[u:w + 1], want_path=False)[0]
    return pattern, V, x


def cases(tables, cfg, as_int16):
    """The shared reads and what the reference makes of them, computed once per process:
    [dict(target, strand, cut, table, sig, kind, complete, row, rec, call, tc)]; float64: the C9orf72 reads only."""
    if as_int16 in _CASES:
        return _CASES[as_int16]
    from concurrent.futures import ThreadPoolExecutor
    from strique_amd import synth
    from strique_amd.pore_model import pore_model
    base = (tables["base_kmer"], tables["base_mean"], tables["base_stdv"])
    mod = (tables["mod_kmer"], tables["mod_mean"], tables["mod_stdv"])
    made_from = {"base": synth.KmerTable(pore_model(table=base)), "mod": synth.KmerTable(pore_model(table=mod))}
    opm, opm_mod = orc.PoreModel(table=base), orc.PoreModel(table=mod)
    params = orc.align_params(cfg["align"])
    jobs = []
    for name in ar.TARGETS if as_int16 else ("c9orf72",):
        target = tuple(cfg["repeat"][name][3:6])
        for strand in "+-":
            tc = orc.classifier(*target, strand, opm, opm_mod, cfg["HMM"])
            mods = ar.models(*target, strand, opm, cfg["HMM"])
            for cut in ar.ENDS_CUTS + ar.STARTS_CUTS:
                for which in TABLES:
                    sig, kind, complete = ar.make_case(made_from[which], synth.make_signal, target, strand, cut, SEED, as_int16)
                    jobs.append(dict(target=name, strand=strand, cut=cut[0], table=which, sig=sig, kind=kind, complete=complete, tc=tc, mods=mods))
    orc.lib()

    def work(j):
        row, rec = ar.record(j["sig"], j["tc"], j["mods"], opm, params, M)
        return row, rec, call(j["sig"], rec, j["tc"], opm)
    with ThreadPoolExecutor(8) as ex:          # the oracle's DP and Viterbi are ctypes calls: they release the interpreter lock
        done = list(ex.map(work, jobs))
    for j, (row, rec, c) in zip(jobs, done):
        j.update(row=row, rec=rec, call=c)
        del j["mods"]
    _CASES[as_int16] = jobs
    return jobs
