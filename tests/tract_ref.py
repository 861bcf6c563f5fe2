"""Reference of tract counting for the tests.  Nothing of the product is imported here.

The compound net of a definition is built from the oracle's own pieces (oracle/hmm_oracle.py: _Profile, _Loop, Net, prepare --
un-baked graphs, as tests/anchored_ref.py builds its nets) from the rule restated below.  Two decodes of any model given as
arrays (a Prepared net, or the BakedHMM the GPU tests hand to both sides):

  reference A   orc.viterbi: the oracle's bit-exact log-probability and state path; the counts are read off the path.
  reference B   a float64 DP of its own that carries K counters along the winner of every state; the first of equal candidates
                in ascending source order wins (the contract tests/vit_mode_cases.py states for the count payload).

Also the shared cases: clean reads of two loci with planted (n_0 .. n_{K-1}), both strands, and what reference A makes of them."""
import math

import numpy as np

from oracle import hmm_oracle as ho
from oracle import strique_oracle as orc

_DEFAULTS = dict(skip=1 - 1e-4, seq_std_scale=1.0, rep_std_scale=1.0, seq_std_offset=0.0, rep_std_offset=0.0, e1_ratio=0.1)


# ---- the rule, restated ----------------------------------------------------------------------------------------------------------
def strand_definition(units, linkers, prefix, suffix, strand):
    """(units, linkers, prefix, suffix) as the strand reads them: '-' takes the reverse complements in reverse order, the flanks swap."""
    units = [u.upper() for u in units]; linkers = [l.upper() for l in linkers]; prefix = prefix.upper(); suffix = suffix.upper()
    if strand == '+':
        return units, linkers, prefix, suffix
    return ([orc.revcomp(u) for u in reversed(units)], [orc.revcomp(l) for l in reversed(linkers)], orc.revcomp(suffix), orc.revcomp(prefix))


def units_of(unit, kmer):
    return int(math.ceil(kmer / len(unit)))


def compound_net(units, linkers, prefix, suffix, pm, config=None):
    """start -> prefix + (U_0 u_0)[:-1] -> loop tract0 -> U_0 u_0 + L_0 + (U_1 u_1)[:-1] -> loop tract1 ... -> U_{K-1} u_{K-1} + suffix
    -> end.  Returns (Net, biases); the counted nodes of tract j are the two dummy states of loop j."""
    P = ho._merged(_DEFAULTS, config if isinstance(config, dict) else None)
    K = len(units)
    assert 2 <= K <= 3 and len(linkers) == K - 1
    u = [units_of(x, pm.kmer) for x in units]
    prof = lambda seq, tag: ho._Profile(seq, pm, P, tag, False, P["seq_std_scale"], P["seq_std_offset"])
    parts = [prof(prefix + (units[0] * u[0])[:-1], "prefix")]
    loops = []
    for j in range(K):
        loops.append(ho._Loop(units[j], pm, P, "tract%d" % j, P["rep_std_scale"], P["rep_std_offset"]))
        parts.append(loops[-1])
        if j < K - 1:
            parts.append(prof(units[j] * u[j] + linkers[j] + (units[j + 1] * u[j + 1])[:-1], "junction%d" % j))
    parts.append(prof(units[K - 1] * u[K - 1] + suffix, "suffix"))
    net = ho.Net("compound")
    at = [net.unite(p.net) for p in parts]
    net.edge(net.start, at[0](parts[0].s1), P["e1_ratio"]); net.edge(net.start, at[0](parts[0].s2), 1 - P["e1_ratio"])
    for i in range(len(parts) - 1):
        net.edge(at[i](parts[i].e1), at[i + 1](parts[i + 1].s1), 1); net.edge(at[i](parts[i].e2), at[i + 1](parts[i + 1].s2), 1)
    net.edge(at[-1](parts[-1].e1), net.end, 1); net.edge(at[-1](parts[-1].e2), net.end, 1)
    counted = []
    for p, a in zip(parts, at):
        if isinstance(p, ho._Loop):
            counted += [a(p.d1), a(p.d2)]
    net.counted = tuple(counted)
    return net, [2 * uj - 1 - l.repeat_offset for uj, l in zip(u, loops)]


def tract_of_names(names, silent_start):
    """Per state: the tract whose dummy state it is, from its name; -1 otherwise."""
    out = np.full(len(names), -1, np.int32)
    for i, n in enumerate(names[:silent_start]):
        if n.startswith("tract") and (n.endswith("dummy1") or n.endswith("dummy2")):
            out[i] = int(n[len("tract"):-len("dummy1")])
    return out


_MODELS = {}


def model(units, linkers, prefix, suffix, strand, pm, config=None):
    """{'net', 'prep', 'bias' (model order), 'tract_of', 'K'} of one strand of a definition, built once."""
    key = (tuple(units), tuple(linkers), prefix, suffix, strand, id(pm), repr(sorted((config or {}).items())))
    if key not in _MODELS:
        un, li, p, s = strand_definition(units, linkers, prefix, suffix, strand)
        net, bias = compound_net(un, li, p, s, pm, config)
        prep = ho.prepare(net)
        _MODELS[key] = {"net": net, "prep": prep, "bias": bias, "tract_of": tract_of_names(prep.names, prep.silent_start), "K": len(un)}
    return _MODELS[key]


# ---- reference A -----------------------------------------------------------------------------------------------------------------
def decode_a(m, tract_of, K, x):
    """(logp, counts[K] or zeros, status) -- status 0 ok, 1 no path -- from the oracle's path."""
    logp, path, _ = orc.viterbi(m, x)
    if path is None:
        return logp, [0] * K, 1
    t = np.asarray(tract_of)[np.asarray(path, np.int64)] if len(path) else np.zeros(0, np.int64)
    return logp, [int((t == j).sum()) for j in range(K)], 0


# ---- reference B -----------------------------------------------------------------------------------------------------------------
def decode_b(m, tract_of, K, x):
    """The same triple from a DP of its own."""
    n, ne = int(m.n_states), int(m.silent_start)
    NEG = -np.inf
    in_ptr = np.asarray(m.in_ptr); in_src = np.asarray(m.in_src); in_lp = np.asarray(m.in_logp, np.float64)
    ins = []
    for l in range(n):
        es = sorted(range(in_ptr[l], in_ptr[l + 1]), key=lambda e: int(in_src[e]))          # ascending source
        ins.append([(int(in_src[e]), float(in_lp[e])) for e in es])
    D = max(1, max(len(ins[l]) for l in range(ne)))
    E_src = np.full((ne, D), n, np.int64); E_lp = np.zeros((ne, D))
    for l in range(ne):
        for j, (k, lp) in enumerate(ins[l]):
            E_src[l, j] = k; E_lp[l, j] = lp
    add = np.zeros((ne, K), np.int64)
    for l in range(ne):
        if tract_of[l] >= 0:
            add[l, int(tract_of[l])] = 1
    kind = np.asarray(m.emis_kind); ea = np.asarray(m.emis_a, np.float64); eb = np.asarray(m.emis_b, np.float64); ec = np.asarray(m.emis_c, np.float64)
    rows = np.arange(ne)
    v = np.full(n + 1, NEG); c = np.zeros((n + 1, K), np.int64)

    def silent(pin):
        for l in range(ne, n):
            if pin and l == m.start:
                v[l] = 0.0; c[l] = 0
                continue
            best, arg = NEG, -1
            for k, lp in ins[l]:
                cand = v[k] + lp
                if cand > best:
                    best, arg = cand, k
            v[l] = best
            c[l] = c[arg] if arg >= 0 else 0

    silent(True)
    for xt in np.asarray(x, np.float64):
        cand = v[E_src] + E_lp
        win = np.argmax(cand, axis=1)          # the first of equal candidates
        best = cand[rows, win]; wsrc = E_src[rows, win]
        if xt != xt:
            em = np.zeros(ne)
        else:
            d = xt - ea
            with np.errstate(invalid="ignore", over="ignore"):
                en = ec - (d * d) * eb
            em = np.where(kind == 1, en, np.where((xt >= ea) & (xt <= eb), ec, NEG))
        nc = c[wsrc] + add
        v = np.concatenate([best + em, np.full(n - ne + 1, NEG)])
        c = np.concatenate([nc, np.zeros((n - ne + 1, K), np.int64)])
        silent(False)
    e = int(m.end)
    if not v[e] > NEG:
        return float(v[e]), [0] * K, 1
    return float(v[e]), [int(q) for q in c[e]], 0


# ---- the shared cases ------------------------------------------------------------------------------------------------------------
# name -> (units, linkers): an HTT-like locus of two 3-nt units with a linker, and one whose units differ in length
LOCI = {
    "htt_like": (("CAG", "CCG"), ("CAACAG",)),
    "cnbp_like": (("CCTG", "TCTG", "TG"), ("", "")),
}
# definitions the model test builds beside them: units of 2, 3, 4 and 6 nt, K = 2 and 3
MODEL_DEFINITIONS = dict(LOCI, mixed6=(("GGCCTG", "CAG"), ("",)), atxn8_like=(("CTA", "CTG"), ("",)), tg_ca=(("TG", "CA", "GGCCCC"), ("A", "")))
PLANTED = {"htt_like": ((12, 7), (5, 9)), "cnbp_like": ((9, 6, 11), (6, 10, 7))}
SAMPLES = 6
NOISE_SD = 1.0
SEED = 7


def clean_read(pm, units, linkers, prefix, suffix, strand, planted, seed):
    """The window of a read with the planted counts: the k-mer means of prefix | U_j x n_j, linkers | suffix as the strand reads
    them, SAMPLES observations each, with a little seeded Gaussian noise (NOISE_SD pA: a window of bare k-mer means is full of
    exact ties), clipped into the emission range."""
    un, li, p, s = strand_definition(units, linkers, prefix, suffix, strand)
    n = list(planted) if strand == '+' else list(reversed(planted))
    seq = p
    for j, u in enumerate(un):
        seq += u * n[j] + (li[j] if j < len(li) else "")
    seq += s
    rng = np.random.Generator(np.random.PCG64(seed))
    x = pm.template(seq, SAMPLES)
    x = x + rng.normal(0.0, NOISE_SD, len(x))
    return np.clip(x, pm.model_min + .5, pm.model_max - .5)


def configured(values, strand):
    return list(values) if strand == '+' else list(reversed(list(values)))


_CASES = {}


def cases(pm, prefix, suffix, config=None):
    """[(locus, strand, planted, x, model dict)] -- the shared clean reads, built once per process."""
    key = (id(pm), prefix, suffix)
    if key not in _CASES:
        out = []
        for name in sorted(LOCI):
            units, linkers = LOCI[name]
            for strand in "+-":
                m = model(units, linkers, prefix, suffix, strand, pm, config)
                for i, planted in enumerate(PLANTED[name]):
                    x = clean_read(pm, units, linkers, prefix, suffix, strand, planted, SEED + i)
                    out.append((name, strand, planted, x, m))
        _CASES[key] = out
    return _CASES[key]


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
def record(sig, tc, m, pm, params):
    """(row, record) of one read: the oracle's detect() row for the flanked classifier `tc`, and None or (counts in configured
    order, log_p) -- `m`: (model dict, strand) of the read's compound model, None for a target without tracts.  The rule: the gate
    passed, the read was normalised, the flanked decode found a path; then the compound net on the very window of that decode."""
    sig = np.asarray(sig)
    row, info = orc.detect(sig, tc, pm, params)
    if m is None:
        return row, None
    flt = orc.medfilt3(sig)
    normalised = np.isfinite(np.median(flt)) and orc.mad(flt) > 0
    b, e = info["prefix_begin"], info["suffix_end"]
    gate = b < e and row[1] > 0.0 and row[2] > 0.0
    if not (gate and normalised and row[3] != 0):
        return row, None
    model_, strand = m
    fltn = pm.normalize_minmax(flt.astype(np.float64))
    logp, visits, status = decode_a(model_["prep"], model_["tract_of"], model_["K"], fltn[b:e])
    if status:
        return row, None
    return row, (tuple(configured([v + q for v, q in zip(visits, model_["bias"])], strand)), logp)


def array_of(units, linkers, planted):
    """The repeat array of a compound locus on the + strand: U_0 x n_0 | L_0 | U_1 x n_1 ..."""
    out = ""
    for j, u in enumerate(units):
        out += u * planted[j] + (linkers[j] if j < len(linkers) else "")
    return out


# count_j - planted_j (configured order) of reference A on every shared case: recorded from the reference, which is
# deterministic -- this pins the model definition, it is no claim of accuracy
RECORDED_ERROR = {
    ("cnbp_like", "+", (9, 6, 11)): (0, 0, 0), ("cnbp_like", "+", (6, 10, 7)): (0, 0, 0),
    ("cnbp_like", "-", (9, 6, 11)): (0, 0, 0), ("cnbp_like", "-", (6, 10, 7)): (0, 0, 0),
    ("htt_like", "+", (12, 7)): (0, 0), ("htt_like", "+", (5, 9)): (0, 0),
    ("htt_like", "-", (12, 7)): (0, 0), ("htt_like", "-", (5, 9)): (0, 0),
}
