"""Reference of the motif track for the tests.  Nothing of the product is imported here: the nets come from oracle/hmm_oracle.py
(un-baked graphs), the decodes from oracle/strique_oracle.py and numpy.

The rule, restated.  The loop model of a unit is the repeat section of the flanked net of that unit -- its emitting states, in the
order `prepare` gives them, with the edges among them as `prepare` leaves them (out-edges renormalised inside the flanked net) and
every hop through a silent state of the section resolved into one edge (log-probabilities added along the hop).  Every state is
entered from a start state with -log(n_emit) and reaches an end state with log-probability 0; the edges that leave the section
are dropped.  Arrays in the layout of hmm_oracle.Prepared: start is state n_emit, end is state n_emit + 1, in-edges by ascending
source.

A stretch of T observations has n_seg = max(1, T // S) segments: [i S, (i + 1) S) for i < n_seg - 1, the last one runs to T.
V[i][j] is the value of the end state of loop model j after the observations of segment i.  Two evaluations that must agree to
the bit: `score_a`, orc.viterbi on the arrays, and `score_b`, a plain numpy loop."""
import math

import numpy as np

from oracle import hmm_oracle as ho
from oracle import strique_oracle as orc

_FLANK = "GATTACAGATTACAGT"          # any flank: the repeat section does not depend on it


def revcomp(s):
    return orc.revcomp(s)


def key(unit):
    """Primitive root of the unit, at its lexicographically smallest rotation."""
    root = next(unit[:n] for n in range(1, len(unit) + 1) if len(unit) % n == 0 and unit[:n] * (len(unit) // n) == unit)
    return min(root[i:] + root[:i] for i in range(len(root)))


class Loop(object):
    """Arrays strq_oracle_viterbi consumes."""
    pass


_LOOPS = {}


def loop(unit, pm, config=None):
    """The loop model of `unit`, built once."""
    k = (unit, id(pm), repr(sorted((config or {}).items())))
    if k in _LOOPS:
        return _LOOPS[k]
    net, _, _ = ho.flanked_net(unit, _FLANK, _FLANK, pm, config)
    p = ho.prepare(net)
    ne_all = p.silent_start
    section = lambda s: p.names[s].startswith("repeat")
    emit = [s for s in range(ne_all) if section(s)]
    new = {old: i for i, old in enumerate(emit)}
    ne = len(emit)

    def sources(s):
        """(emitting source of the section, log-probability) of every way into state s, hops through the section's silent states resolved."""
        out = []
        for e in range(p.in_ptr[s], p.in_ptr[s + 1]):
            src, lp = int(p.in_src[e]), float(p.in_logp[e])
            if src < ne_all:
                if section(src):
                    out.append((src, lp))
            elif section(src):
                out += [(q, lq + lp) for q, lq in sources(src)]
        return out

    m = Loop()
    m.n_states, m.silent_start, m.start, m.end = ne + 2, ne, ne, ne + 1
    m.in_ptr = np.zeros(ne + 3, np.int32)
    src_all, lp_all = [], []
    for i, s in enumerate(emit):
        ins = sorted((new[q], lq) for q, lq in sources(s))
        assert len(set(q for q, _ in ins)) == len(ins), "parallel edges in a loop"
        src_all += [q for q, _ in ins] + [m.start]
        lp_all += [lq for _, lq in ins] + [-math.log(ne)]
        m.in_ptr[i + 1] = len(src_all)
    m.in_ptr[m.start + 1] = len(src_all)
    src_all += list(range(ne)); lp_all += [0.0] * ne
    m.in_ptr[m.end + 1] = len(src_all)
    m.in_src = np.array(src_all, np.int32); m.in_logp = np.array(lp_all, np.float64)
    m.emis_kind = np.asarray(p.emis_kind)[emit].copy()
    m.emis_a = np.asarray(p.emis_a)[emit].copy(); m.emis_b = np.asarray(p.emis_b)[emit].copy(); m.emis_c = np.asarray(p.emis_c)[emit].copy()
    m.count_inc = np.zeros(ne + 2, np.int32)
    m.names = [p.names[s] for s in emit] + ["loop-start", "loop-end"]
    m.tag = np.zeros(ne + 2, np.int32)
    _LOOPS[k] = m
    return m


def segments(T, S):
    n = max(1, T // S)
    return [(i * S, (i + 1) * S if i < n - 1 else T) for i in range(n)]


def score_a(m, x):
    """The end state's value from the oracle's Viterbi."""
    return orc.viterbi(m, x, want_path=False)[0]


def score_b(m, x):
    """The same from a numpy loop: the largest value over the emitting states after the last observation."""
    ne = int(m.silent_start)
    D = max(int(m.in_ptr[l + 1] - m.in_ptr[l]) for l in range(ne))
    E_src = np.full((ne, D), ne + 2, np.int64); E_lp = np.zeros((ne, D))
    for l in range(ne):
        for j, e in enumerate(range(m.in_ptr[l], m.in_ptr[l + 1])):
            E_src[l, j] = m.in_src[e]; E_lp[l, j] = m.in_logp[e]
    v = np.full(ne + 3, -np.inf); v[m.start] = 0.0          # (cell ne + 2: the source of padding edges)
    kind, ea, eb, ec = (np.asarray(a) for a in (m.emis_kind, m.emis_a, m.emis_b, m.emis_c))
    for xt in np.asarray(x, np.float64):
        best = (v[E_src] + E_lp).max(axis=1)
        if xt != xt:
            em = np.zeros(ne)
        else:
            d = xt - ea
            with np.errstate(invalid="ignore", over="ignore"):
                en = ec - (d * d) * eb
            em = np.where(kind == 1, en, np.where((xt >= ea) & (xt <= eb), ec, -np.inf))
        v = np.concatenate([best + em, np.full(3, -np.inf)])
    return float(v[:ne].max())


def track(models, x, S, score=score_a):
    """(V (n_seg, K), winners, obs_won, majority, bounds) of a stretch under the candidates' loop models."""
    x = np.asarray(x, np.float64)
    bounds = segments(len(x), S)
    V = np.array([[score(m, x[b:e]) for m in models] for b, e in bounds], np.float64)
    win = [int(np.argmax(row)) for row in V]          # the first of equal values
    obs_won = [0] * len(models)
    for w, (b, e) in zip(win, bounds):
        obs_won[w] += e - b
    majority = obs_won.index(max(obs_won))            # the first of equal counts
    return V, win, obs_won, majority, bounds


def record(sig, repeat, alternatives, prefix, suffix, strand, pm, params, config, S):
    """(row, record) of one read: the oracle's detect() row for the target's own unit, and None or (majority, shares, count_m,
    log_p_m, runs, winners, V, bounds).  The rule: the gate passed, the read was normalised, prefix_end < suffix_begin; then the
    track on the filtered, normalised signal between the two flanks; the count under the majority unit is the row's own for
    candidate 0 (None, None when the row has no decode), else the oracle's flanked decode of that unit on the row's window.
    alternatives None: a target without motifs."""
    sig = np.asarray(sig)
    tc = orc.classifier(repeat, prefix, suffix, strand, pm, None, config)
    row, info = orc.detect(sig, tc, pm, params)
    if alternatives is None:
        return row, None
    flt = orc.medfilt3(sig)
    normalised = np.isfinite(np.median(flt)) and orc.mad(flt) > 0
    b, e = info["prefix_begin"], info["suffix_end"]
    pe, sb = info["prefix_end"], info["suffix_begin"]
    if not (b < e and row[1] > 0.0 and row[2] > 0.0 and normalised and pe < sb):
        return row, None
    fltn = pm.normalize_minmax(flt.astype(np.float64))
    units = [repeat.upper()] + [u.upper() for u in alternatives]
    as_read = units if strand == '+' else [revcomp(u) for u in units]
    V, win, obs_won, majority, bounds = track([loop(u, pm, config) for u in as_read], fltn[pe:sb], S)
    T = sb - pe
    if majority == 0:
        count_m, log_p_m = (row[0], row[3]) if row[3] != 0 else (None, None)
    else:
        tm = orc.classifier(units[majority], prefix, suffix, strand, pm, None, config)
        logp, path, counted = orc.viterbi(tm['hmm'], fltn[b:e])
        count_m, log_p_m = (int(counted) + tm['count_bias'], logp) if path is not None else (None, None)
    return row, (majority, tuple(o / T for o in obs_won), count_m, log_p_m, runs(win, bounds, pe), win, V, bounds)


def runs(win, bounds, first_sample=0):
    """Maximal runs of equal winners: (candidate, first_sample, end_sample)."""
    out = []
    for w, (b, e) in zip(win, bounds):
        if out and out[-1][0] == w:
            out[-1] = (w, out[-1][1], first_sample + e)
        else:
            out.append((w, first_sample + b, first_sample + e))
    return out
