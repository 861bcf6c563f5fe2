"""Test helper: the per-unit scores behind a modification pattern, from the CPU oracle alone.

Nothing is imported from the product.  For one read and one strand-specific oracle classifier (oracle.strique_oracle.classifier with a
modification pore model):

  * oracle.detect gives the row, the pattern string and the window [prefix_begin, suffix_end);
  * the clipped repeat stretch x is rebuilt the way detect builds it (STRique.py:605-609), and oracle.viterbi(tc['mod'], x) gives the
    path whose runs of non-hub states are the units: unit j is emitted at x[u_j + 1 .. w_j - 1], x[u_j] by the hub s0 in front of it
    and x[w_j] by the hub e0 behind it;
  * M_base / M_mod are copies of the dual model with in_logp = -inf on every edge that has an emitting state of the other branch at
    either end, and V_B(j) = oracle.viterbi(M_B, x[u_j : w_j + 1], want_path=False): the oracle's own arithmetic, unchanged.

llr_j = V_mod(j) - V_base(j).
"""
import copy

import numpy as np

from oracle import strique_oracle as orc

HUBS = ("s0", "e0")


def branch_of(model):
    """Per state: 0 base, 1 modified, 2 hub, -1 silent."""
    out = np.full(model.n_states, -1, np.int64)
    for l in range(model.silent_start):
        out[l] = 2 if model.names[l] in HUBS else (1 if "mod" in model.names[l] else 0)
    return out


def masked(model, keep):
    """The dual model without the other branch: edges into or out of its emitting states at -inf, arrays and order unchanged."""
    br = branch_of(model)
    other = 1 - keep
    m = copy.copy(model)
    lp = np.array(model.in_logp, np.float64, copy=True)
    for l in range(model.n_states):
        for e in range(int(model.in_ptr[l]), int(model.in_ptr[l + 1])):
            if br[l] == other or br[int(model.in_src[e])] == other:
                lp[e] = -np.inf
    m.in_logp = lp
    return m


def unit_bounds(model, path):
    """[(u_j, w_j)] of a path of the dual model: the hub emissions around every maximal run of non-hub emissions."""
    br = branch_of(model)
    hub = np.array([br[s] == 2 for s in path], bool)
    out = []
    t, T = 0, len(path)
    while t < T:
        if hub[t]:
            t += 1
            continue
        t0 = t
        while t < T and not hub[t]:
            t += 1
        out.append((t0 - 1, t))
    return out


_MASKS = {}


def reference(raw, tc, opm, params, opm_mod):
    """dict(row, pattern, x, bounds [(u, w)], V (n, 2) float64 of (V_base, V_mod); V has no rows when the pattern is '-'), plus
    window / mask: the observations of the flanked decode and which of them its path emits from repeat states (the stretch x is cut
    from) -- for stretch_is_unique."""
    raw = np.asarray(raw)
    row, info = orc.detect(raw, tc, opm, params, pm_mod=opm_mod)
    out = dict(row=row, pattern=row[6], x=None, bounds=[], V=np.zeros((0, 2)), window=None, mask=None)
    if row[6] == "-":
        return out
    b, e = info["prefix_begin"], info["suffix_end"]
    _, _, _, fltn = orc.condition(raw, opm)
    _, path, _ = orc.viterbi(tc["hmm"], fltn[b:e])
    mask = np.array(["repeat" in tc["hmm"].names[s] for s in path], bool)
    nrm = opm.normalize_minmax(raw.astype(np.float64))
    x = np.clip(nrm[b:e][mask], tc["mod_range"][0], tc["mod_range"][1])
    model = tc["mod"]
    _, mpath, _ = orc.viterbi(model, x)
    bounds = unit_bounds(model, mpath)
    if id(model) not in _MASKS:
        _MASKS[id(model)] = (model, masked(model, 0), masked(model, 1))
    _, m_base, m_mod = _MASKS[id(model)]
    V = np.zeros((len(bounds), 2))
    for j, (u, w) in enumerate(bounds):
        V[j, 0] = orc.viterbi(m_base, x[u:w + 1], want_path=False)[0]
        V[j, 1] = orc.viterbi(m_mod, x[u:w + 1], want_path=False)[0]
    out.update(x=x, bounds=bounds, V=V, window=fltn[b:e], mask=mask)
    return out


def stretch_is_unique(ref, flanked, repeat_tag=1):
    """The per-unit scores are defined on the repeat stretch of the flanked decode.  Where that decode has two best paths of equal
    log-probability (the last prefix state and the first repeat state share a k-mer, so a dwell can go to either), the stretch may
    begin a few observations earlier or later depending on the order a model lists its in-edges in -- the order differs between the
    un-baked graph of the oracle and the baked arrays of a product (`flanked`: any object with the oracle's array fields and a `tag`
    marking repeat states).  True when both orders mark the same stretch: only then is the reference the reference of that product."""
    if ref["mask"] is None:
        return True
    _, path, _ = orc.viterbi(flanked, ref["window"])
    return path is not None and np.array_equal(np.asarray(flanked.tag)[path] == repeat_tag, ref["mask"])
