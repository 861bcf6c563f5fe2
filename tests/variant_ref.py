"""Test helper: the variant pass (alt-unit calls per passage, corrected count) from the CPU oracle alone.

Nothing is imported from the product.  For one read and one strand-specific oracle classifier (oracle.strique_oracle.classifier) plus
the un-baked variant net of that strand (variant_net, from oracle.hmm_oracle's Net / _Profile / tandem_unit / prepare, the way
mod_net builds the modification net):

  * oracle.detect gives the row and the window [prefix_begin, suffix_end);
  * the clipped repeat stretch x is rebuilt as tests/mod_llr_ref.py rebuilds it: the raw samples normalised to the pore model, those
    the flanked path emits from repeat states, clipped to [model_min, model_max].  The repeat section of a flanked model cannot be
    re-entered, so those samples are one contiguous run and observation t of x is raw sample first + t, first = prefix_begin + the
    first repeat emission -- reference() asserts it;
  * oracle.viterbi(net, x) gives the path whose maximal runs of non-hub emissions are the passages: passage j is emitted at
    x[u_j + 1 .. w_j - 1], x[u_j] by the hub s0 in front of it and x[w_j] by the hub e0 behind it; its branch is that of its states;
  * M_b, b = 0 .. NB - 1, are copies of the model with in_logp = -inf on every edge that has an emitting state of another branch at
    either end, and V_b(j) = oracle.viterbi(M_b, x[u_j : w_j + 1], want_path=False): the oracle's own arithmetic, unchanged.

pattern: '0' per base passage, '0' * m + str(b) per passage of alt branch b; count_v = len(pattern) + the classifier's count_bias;
end_j = first + w_j.
"""
import copy

import numpy as np

from oracle import hmm_oracle as ho
from oracle import strique_oracle as orc

HUBS = ("s0", "e0")


def context_units(repeat, K):
    return -(-(K - 1) // len(repeat))


def variant_net(repeat, alt_units, pm, config=None):
    """The un-baked variant net of one strand (`repeat`, `alt_units` as that strand reads them).  Returns (Net, m)."""
    P = ho._merged(dict(rep_std_scale=1.5, rep_std_offset=0.0, leave_repeat=.002, variant_prior=None), config if isinstance(config, dict) else None)
    K, L = pm.kmer, len(repeat)
    m = context_units(repeat, K)
    NB = 1 + len(alt_units)
    unit, _ = ho.tandem_unit(repeat, K)
    profs = [ho._Profile(unit, pm, P, "base", True, P["rep_std_scale"], P["rep_std_offset"])]
    for b, alt in enumerate(alt_units, 1):
        seq = (repeat * m + alt + repeat * K)[:(m + 1) * L + K - 1]
        profs.append(ho._Profile(seq, pm, P, "alt%d" % b, True, P["rep_std_scale"], P["rep_std_offset"]))
    p = P["variant_prior"]
    prior = [1.0 / NB] * NB if p is None else [1.0 - (NB - 1) * p] + [p] * (NB - 1)
    net = ho.Net("variant")
    ats = [net.unite(pr.net) for pr in profs]
    s0 = net.node("s0", ho.UNIFORM, (pm.model_min, pm.model_max)); e0 = net.node("e0", ho.UNIFORM, (pm.model_min, pm.model_max))
    net.edge(net.start, s0, 1)
    for at, prof, pr in zip(ats, profs, prior):
        net.edge(s0, at(prof.s1), pr / 2); net.edge(s0, at(prof.s2), pr / 2)
    for at, prof in zip(ats, profs):
        net.edge(at(prof.e1), e0, 1); net.edge(at(prof.e2), e0, 1)
    net.edge(e0, net.end, P["leave_repeat"]); net.edge(e0, s0, 1 - P["leave_repeat"])
    return net, m


def strand_units(repeat, alt_units, strand):
    """repeat and alt units as the given strand reads them."""
    r, alts = repeat.upper(), [a.upper() for a in alt_units]
    return (r, alts) if strand == "+" else (orc.revcomp(r), [orc.revcomp(a) for a in alts])


class VariantModel(object):
    """prepared net of one strand, its branches and its masked copies"""

    def __init__(self, repeat, alt_units, strand, pm, config=None):
        r, alts = strand_units(repeat, alt_units, strand)
        net, self.m = variant_net(r, alts, pm, config)
        self.net = net
        self.model = ho.prepare(net)
        self.nb = 1 + len(alts)
        self.range = (pm.model_min, pm.model_max)
        self.branch = branch_of(self.model)
        self.masked = [masked(self.model, self.branch, b) for b in range(self.nb)]


def branch_of(model):
    """Per state: 0 base, b alt branch b, -2 hub, -1 silent."""
    out = np.full(model.n_states, -1, np.int64)
    for l in range(model.n_states):
        n = model.names[l]
        if l < model.silent_start:
            out[l] = -2 if n in HUBS else (int(n[3]) if n.startswith("alt") else 0)
    return out


def masked(model, branch, keep):
    """The model without the other branches: every edge into or out of an emitting state of another branch at -inf.  (The silent
    s1 / s2 / e1 / e2 of a profile lead to and from its own emitting states only, so nothing passes through them either.)"""
    m = copy.copy(model)
    lp = np.array(model.in_logp, np.float64, copy=True)
    other = lambda s: branch[s] >= 0 and branch[s] != keep
    for l in range(model.n_states):
        for e in range(int(model.in_ptr[l]), int(model.in_ptr[l + 1])):
            if other(l) or other(int(model.in_src[e])):
                lp[e] = -np.inf
    m.in_logp = lp
    return m


def passages(branch, path):
    """[(u_j, w_j, branch_j)] of a path: the hub emissions around every maximal run of non-hub emissions."""
    out = []
    t, T = 0, len(path)
    while t < T:
        if branch[path[t]] == -2:
            t += 1
            continue
        t0 = t
        while t < T and branch[path[t]] != -2:
            t += 1
        bs = set(int(branch[s]) for s in path[t0:t])
        assert len(bs) == 1 and t0 >= 1 and t < T, "a passage lies in one branch, between two hub emissions"
        out.append((t0 - 1, t, bs.pop()))
    return out


def pattern_of(branches, m):
    return "".join("0" if b == 0 else "0" * m + str(b) for b in branches)


def reference(raw, tc, opm, params, vm):
    """dict(row, decoded, count_v, pattern, branch, end, bounds [(u, w)], V (n, NB) float64, x, first) for one read; decoded False (and
    nothing else filled in) when the gate failed or the flanked decode found no path.  window / mask as mod_llr_ref.reference gives
    them, for mod_llr_ref.stretch_is_unique."""
    raw = np.asarray(raw)
    row, info = orc.detect(raw, tc, opm, params)
    out = dict(row=row, decoded=False, count_v=0, pattern=None, branch=np.zeros(0, np.int8), end=np.zeros(0, np.int64), bounds=[],
               V=np.zeros((0, vm.nb)), x=None, first=None, window=None, mask=None)
    b, e = info["prefix_begin"], info["suffix_end"]
    if not (b < e and row[1] > 0.0 and row[2] > 0.0):
        return out
    _, _, _, fltn = orc.condition(raw, opm)
    _, path, _ = orc.viterbi(tc["hmm"], fltn[b:e])
    if path is None:
        return out
    mask = np.array(["repeat" in tc["hmm"].names[s] for s in path], bool)
    idx = np.flatnonzero(mask)
    out.update(window=fltn[b:e], mask=mask)
    if len(idx) == 0:
        return out
    # the repeat section cannot be re-entered: one contiguous run, so observation t of x is raw sample first + t
    assert np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx)))
    first = b + int(idx[0])
    nrm = opm.normalize_minmax(raw.astype(np.float64))
    x = np.clip(nrm[b:e][mask], vm.range[0], vm.range[1])
    assert np.array_equal(x, np.clip(nrm[first:first + len(x)], vm.range[0], vm.range[1]))
    _, vpath, _ = orc.viterbi(vm.model, x)
    if vpath is None:
        return out
    ps = passages(vm.branch, vpath)
    V = np.zeros((len(ps), vm.nb))
    for j, (u, w, _) in enumerate(ps):
        for c in range(vm.nb):
            V[j, c] = orc.viterbi(vm.masked[c], x[u:w + 1], want_path=False)[0]
    br = np.array([p[2] for p in ps], np.int8)
    pattern = pattern_of(br, vm.m)
    out.update(decoded=True, pattern=pattern, count_v=len(pattern) + tc["count_bias"], branch=br,
               end=np.array([first + p[1] for p in ps], np.int64), bounds=[(p[0], p[1]) for p in ps], V=V, x=x, first=first)
    return out


def calls(ref_or_pattern):
    """[(index in the pattern, alt number)] of the alt characters of a pattern."""
    pat = ref_or_pattern if isinstance(ref_or_pattern, str) else ref_or_pattern["pattern"]
    return [(i, int(ch)) for i, ch in enumerate(pat) if ch != "0"]
