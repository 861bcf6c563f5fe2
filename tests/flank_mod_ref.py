"""Reference of the flank methylation calls for the tests, from the oracle alone (strique_amd/flank_mod.py states the rule; it is
restated here, not imported): on one flank stretch x -- normalised and clipped as the modification pass takes its stretch --

  * oracle.viterbi with path on the UN-BAKED flank profile net (start -> s1 | s2 -> profile -> end, every silent state kept);
  * per CpG group the first and the last observation the path emits from a match or insert state of the group's columns, and from
    them status, u = first - 1, w = last + 1;
  * V_base / V_mod = oracle.viterbi of the un-baked site net (the dual model over the bases the group's columns spell, passed once)
    on x[u .. w] with the other branch masked out by tests/mod_llr_ref.masked.

Ties: two best segmentation paths of equal log-probability can hand an observation to either neighbour, and the un-baked net and a
baked model break such ties by different in-edge orders.  `call(..., alt=)` therefore decodes a second time on `alt` -- any object
with the oracle's array fields and a `column_of`, e.g. the arrays a product bakes -- and marks every group whose bounds differ
between the two (`tie`): such a group is compared with nothing.

Nothing of the product is imported here but the signal synthesis (the reads are inputs)."""
import re

import numpy as np

import mod_llr_ref
from oracle import hmm_oracle as ho
from oracle import strique_oracle as orc

SCORED, NO_PATH, EDGE, SKIPPED, TOO_LONG = 0, 1, 2, 3, 4
MAX_COLUMNS, MAX_GROUPS, MAX_STRETCH = 31, 64, 64
TIE_CAP = 0.02              # share of the (read, group) pairs of a parametrisation that may be excluded as ties

_MODELS = {}


def groups(flank, k):
    """[(sites, c0, c1)]: the CG dinucleotides of the flank, chained while two neighbours fit one k-mer, and the profile columns
    (k-mers, by their first base) that hold a whole CG of the chain."""
    n = len(flank) - k + 1
    out = []
    for m in re.finditer("(?=CG)", flank.upper()):
        c = m.start()
        if out and c + 2 - out[-1][0][-1] <= k:          # both dinucleotides inside one k-mer: c + 2 - c_prev <= k
            out[-1][0].append(c)
        else:
            out.append(([c], None, None))
    return [(tuple(s), max(0, s[0] + 2 - k), min(n - 1, s[-1])) for s, _, _ in out]


def profile_model(flank, pm, config=None):
    """The un-baked flank profile net, prepared, with column_of[state] from the state names (-1: no column)."""
    key = ("profile", flank, id(pm), repr(sorted((config or {}).items())))
    if key not in _MODELS:
        P = ho._merged(dict(skip=1 - 1e-4, seq_std_scale=1.0, seq_std_offset=0.0, e1_ratio=0.1), config if isinstance(config, dict) else None)
        prof = ho._Profile(flank, pm, P, "flank", False, P["seq_std_scale"], P["seq_std_offset"])
        net = ho.Net("flankprofile")
        at = net.unite(prof.net)
        net.edge(net.start, at(prof.s1), P["e1_ratio"]); net.edge(net.start, at(prof.s2), 1 - P["e1_ratio"])
        net.edge(at(prof.e1), net.end, 1); net.edge(at(prof.e2), net.end, 1)
        m = ho.prepare(net)
        m.column_of = np.full(m.n_states, -1, np.int64)
        for s in range(m.silent_start):
            m.column_of[s] = int(re.fullmatch(r"flank(\d+)[mi]", m.names[s]).group(1))
        _MODELS[key] = m
    return _MODELS[key]


def site_models(sequence, pm_base, pm_mod, config=None):
    """(dual net, masked to base, masked to mod) of one group: repeatModHMM's net over `sequence` itself, without the e0 -> s0
    edge, e0 -> end certain."""
    key = ("site", sequence, id(pm_base), id(pm_mod), repr(sorted((config or {}).items())))
    if key not in _MODELS:
        P = ho._merged(dict(rep_std_scale=1.5, rep_std_offset=0.0), config if isinstance(config, dict) else None)
        base = ho._Profile(sequence, pm_base, P, "base", True, P["rep_std_scale"], P["rep_std_offset"])
        mod = ho._Profile(sequence, pm_mod, P, "mod", True, P["rep_std_scale"] * pm_mod.scale2stdv(pm_base), P["rep_std_offset"])
        net = ho.Net("site")
        b = net.unite(base.net); m = net.unite(mod.net)
        lo = min(pm_base.model_min, pm_mod.model_min); hi = max(pm_base.model_max, pm_mod.model_max)
        s0 = net.node("s0", ho.UNIFORM, (lo, hi)); e0 = net.node("e0", ho.UNIFORM, (lo, hi))
        net.edge(net.start, s0, 1)
        for at, prof in ((b, base), (m, mod)):
            net.edge(s0, at(prof.s1), 0.25); net.edge(s0, at(prof.s2), 0.25)
        for at, prof in ((b, base), (m, mod)):
            net.edge(at(prof.e1), e0, 1); net.edge(at(prof.e2), e0, 1)
        net.edge(e0, net.end, 1)
        dual = ho.prepare(net)
        _MODELS[key] = (dual, mod_llr_ref.masked(dual, 0), mod_llr_ref.masked(dual, 1))
    return _MODELS[key]


def stretch(sig, pm_base, pm_mod, begin, end):
    """Raw samples [begin, end) as the modification pass normalises them: minmax on the RAW signal, then the clip to the range of
    both pore models."""
    nrm = pm_base.normalize_minmax(np.asarray(sig).astype(np.float64))
    return np.clip(nrm[begin:end], min(pm_base.model_min, pm_mod.model_min), max(pm_base.model_max, pm_mod.model_max))


def bounds(path, column_of, ranges):
    """[(status, u, w)] per (c0, c1); u = w = -1 unless scored."""
    if path is None:
        return [(NO_PATH, -1, -1)] * len(ranges)
    col = np.asarray(column_of)[np.asarray(path, np.int64)]
    out = []
    for c0, c1 in ranges:
        t = np.flatnonzero((col >= c0) & (col <= c1))
        if not len(t):
            out.append((SKIPPED, -1, -1))
        elif t[0] == 0 or t[-1] == len(col) - 1:
            out.append((EDGE, -1, -1))
        else:
            out.append((SCORED, int(t[0]) - 1, int(t[-1]) + 1))
    return out


def call(x, flank, pm_base, pm_mod, config=None, alt=None):
    """One dict per group of the flank: sites, c0, c1, n_columns, status, u, w, v_base, v_mod (NaN unless scored) and tie (with
    `alt`: the bounds under its in-edge order differ)."""
    k = pm_base.kmer
    gs = groups(flank, k)
    ranges = [(c0, c1) for _, c0, c1 in gs]
    if len(x) > MAX_STRETCH * len(flank):
        bs = [(TOO_LONG, -1, -1)] * len(gs)
        other = bs
    else:
        model = profile_model(flank, pm_base, config)
        bs = bounds(orc.viterbi(model, x)[1], model.column_of, ranges)
        other = bs if alt is None else bounds(orc.viterbi(alt, x)[1], alt.column_of, ranges)
    out = []
    for (s, c0, c1), (status, u, w), o in zip(gs, bs, other):
        v = [np.nan, np.nan]
        if status == SCORED:
            _, m_base, m_mod = site_models(flank[c0:c1 + k], pm_base, pm_mod, config)
            v = [orc.viterbi(m, x[u:w + 1], want_path=False)[0] for m in (m_base, m_mod)]
        out.append(dict(sites=s, c0=c0, c1=c1, n_columns=c1 - c0 + 1, status=status, u=u, w=w, v_base=v[0], v_mod=v[1],
                        tie=tuple(o) != (status, u, w)))
    return out


# ---- the shared reads ----------------------------------------------------------------------------------------------------------------
SEED = 1              # chosen so that the oracle alone keeps the ties of every parametrisation under TIE_CAP (tests/test_flank_mod_host.py)
TABLES = ("base", "mod")
_CASES = {}


def flank_ranges(sig, tc, opm, params):
    """((begin, end) of the strand's prefix flank, (begin, end) of its suffix flank) in raw samples: where the alignment of the
    whole configured flank -- no trim -- begins and ends."""
    _, _, morph, _ = orc.condition(np.asarray(sig), opm)
    _, pb, pe = orc.detect_range(morph, tc["prefix_ext"], params)
    _, sb, se = orc.detect_range(morph, tc["suffix_ext"], params)
    return (pb, pe), (sb, se)


def cases(tables, cfg, targets, names, as_int16, n_units=(12, 27)):
    """The shared reads and their stretches, computed once per process: per target of `names`, strand and pore table one read of
    6 kb with an array of n_units[...] units; [dict(target, strand, table, sig, flanks: [(which, flank as the strand reads it,
    begin, end, x)])]."""
    key = (tuple(names), as_int16)
    if key in _CASES:
        return _CASES[key]
    from strique_amd import synth
    from strique_amd.pore_model import pore_model
    base = (tables["base_kmer"], tables["base_mean"], tables["base_stdv"])
    mod = (tables["mod_kmer"], tables["mod_mean"], tables["mod_stdv"])
    made_from = {"base": synth.KmerTable(pore_model(table=base)), "mod": synth.KmerTable(pore_model(table=mod))}
    opm, opm_mod = orc.PoreModel(table=base), orc.PoreModel(table=mod)
    params = orc.align_params(cfg["align"])
    out = []
    for ti, name in enumerate(names):
        repeat, prefix, suffix = targets[name]
        for si, strand in enumerate("+-"):
            tc = orc.classifier(repeat, prefix, suffix, strand, opm, None, cfg["HMM"])
            pe, se = prefix.upper(), suffix.upper()
            if strand == "-":
                pe, se = orc.revcomp(se), orc.revcomp(pe)
            for wi, which in enumerate(TABLES):
                sig, _ = synth.make_read(made_from[which], 40 + SEED, 100 * ti + 10 * si + wi, 6000, (repeat, prefix, suffix),
                                         n_units[(si + wi) % 2], strand=strand, as_int16=as_int16)
                (pb, pend), (sb, send) = flank_ranges(sig, tc, opm, params)
                flanks = [(0, pe, pb, pend, stretch(sig, opm, opm_mod, pb, pend)), (1, se, sb, send, stretch(sig, opm, opm_mod, sb, send))]
                out.append(dict(target=name, strand=strand, table=which, sig=sig, flanks=flanks))
    _CASES[key] = (out, opm, opm_mod)
    return _CASES[key]


# ---- hand-written paths for the bounds (the plain-Python function and the kernel both run them) ---------------------------------------
# a toy profile of 4 columns: state 2 c = match of column c, 2 c + 1 = its insert, state 8 has no column
HAND_COLUMN_OF = [0, 0, 1, 1, 2, 2, 3, 3, -1]
HAND_PATHS = [
    # (path, ranges, expected)
    ([2], [(1, 1), (0, 0)], [(2, -1, -1), (3, -1, -1)]),                                          # T = 1: inside the group is the edge
    ([0, 0, 6, 6, 6], [(1, 2)], [(3, -1, -1)]),                                                   # never enters the group
    ([2, 2, 4, 6, 6], [(1, 2)], [(2, -1, -1)]),                                                   # inside from t = 0
    ([0, 0, 2, 4, 4], [(1, 2)], [(2, -1, -1)]),                                                   # stays to T - 1
    ([0, 0, 3, 3, 5, 6, 6], [(1, 2)], [(0, 1, 5)]),                                               # inserts only
    ([0, 2, 8, 4, 6, 6], [(1, 2), (3, 3), (0, 0)], [(0, 0, 4), (2, -1, -1), (2, -1, -1)]),        # a state without a column in between
    ([0, 2, 6, 6, 2, 6], [(1, 1)], [(0, 0, 5)]),                                                  # first and last, not a run
    (None, [(1, 2), (0, 0)], [(1, -1, -1), (1, -1, -1)]),                                         # no path
]
