"""Test helper: the forward algorithm with the second-order expectation semiring, restated in numpy.

Independent of the product: nothing is imported from strique_amd, and the graph it runs on is the UN-BAKED one that
oracle.hmm_oracle.prepare() returns (CSR in-edges in graph order, emitting states first, silent states in topological order) --
or any object with the same fields.  What it computes, over all paths from `start` to `end` that emit the T observations of x:

    log_lik = log sum_paths P(path, x)                 pomegranate's HiddenMarkovModel.log_probability(x)
    mean    = E[v | x],   sd = sqrt(Var[v | x])        v = observations a path emits from states with count_inc != 0

Every state carries (log p, log r, log s) with p the mass of the paths that reach it, r = p E[v], s = p E[v^2]; an edge or an
emission adds its log-probability to all three; an emission from a counted state maps (p, r, s) -> (p, r + p, s + 2 r + p).
Moments are taken about zero (all three are non-negative, so log space can hold them).  A missing observation (NaN) has
probability 1 under every distribution; an observation outside a Uniform's support has probability 0 there.

Log space, parametrised by dtype: np.longdouble is the reference, np.float64 shows what a float64 implementation of the same
formulation loses.
"""
import numpy as np


def _lse(a, axis):
    """log sum exp along `axis`; -inf where every term is -inf."""
    m = a.max(axis=axis)
    ms = np.where(np.isfinite(m), m, a.dtype.type(0))
    with np.errstate(divide="ignore"):
        return ms + np.log(np.exp(a - np.expand_dims(ms, axis)).sum(axis=axis))


class _Plan(object):
    """In-edges of a group of states as padded arrays: src[k, j], lp[k, j] (-inf padding)."""

    def __init__(self, prep, states, dtype):
        deg = max([int(prep.in_ptr[l + 1] - prep.in_ptr[l]) for l in states] + [1])
        self.states = np.array(states, np.int64)
        self.src = np.zeros((len(states), deg), np.int64)
        self.lp = np.full((len(states), deg), -np.inf, dtype)
        for k, l in enumerate(states):
            a, b = int(prep.in_ptr[l]), int(prep.in_ptr[l + 1])
            self.src[k, :b - a] = prep.in_src[a:b]
            self.lp[k, :b - a] = np.asarray(prep.in_logp[a:b], dtype)

    def gather(self, L):
        return _lse(L[:, self.src] + self.lp[None, :, :], axis=2)          # [3, states]


def forward_ref(prep, x, dtype=np.longdouble):
    """(log_lik, mean, sd, status) of the window x; status 1 and (-inf, nan, nan) when no path emits it."""
    dt = np.dtype(dtype).type
    n, ne = int(prep.n_states), int(prep.silent_start)
    x = np.asarray(x, np.float64)
    emit = _Plan(prep, list(range(ne)), dtype)
    # silent states level by level: level = length of the longest chain of silent predecessors (they are in topological order)
    level = {}
    for l in range(ne, n):
        level[l] = max([level[int(k)] + 1 for k in prep.in_src[prep.in_ptr[l]:prep.in_ptr[l + 1]] if k >= ne] + [0])
    plans = [_Plan(prep, [l for l in range(ne, n) if level[l] == v], dtype) for v in range(max(level.values()) + 1)]
    kind = np.asarray(prep.emis_kind)
    ea, eb, ec = (np.asarray(a, dtype) for a in (prep.emis_a, prep.emis_b, prep.emis_c))
    counted = np.asarray(prep.count_inc[:ne]) != 0
    if np.any(np.asarray(prep.count_inc[ne:]) != 0):
        raise ValueError("counted silent states are outside the definition")
    ln2 = np.log(dt(2))
    NEG = dt(-np.inf)

    def silent(L, pin):
        for pl in plans:
            g = pl.gather(L)
            if pin:
                k = np.nonzero(pl.states == prep.start)[0]
                if len(k):
                    g[:, k[0]] = (dt(0), NEG, NEG)
            L[:, pl.states] = g

    L = np.full((3, n), NEG, dtype)
    silent(L, True)
    for t in range(len(x)):
        xt = dt(x[t])
        if np.isnan(x[t]):
            em = np.zeros(ne, dtype)
        else:
            d = xt - ea
            with np.errstate(invalid="ignore"):
                em = np.where(kind == 1, ec - d * d * eb, np.where((xt >= ea) & (xt <= eb), ec, NEG))
        new = emit.gather(L) + em[None, :]
        lp, lr, ls = new[0].copy(), new[1].copy(), new[2].copy()
        c = counted
        new[2, c] = _lse(np.stack([ls[c], ln2 + lr[c], lp[c]]), axis=0)
        new[1, c] = _lse(np.stack([lr[c], lp[c]]), axis=0)
        L = np.full((3, n), NEG, dtype)
        L[:, :ne] = new
        silent(L, False)
    lp, lr, ls = L[:, prep.end]
    if not np.isfinite(lp):
        return dt(-np.inf), dt(np.nan), dt(np.nan), 1
    mean = np.exp(lr - lp)
    var = np.exp(ls - lp) - mean * mean
    if not var > 0:
        var = dt(0)
    return lp, mean, np.sqrt(var), 0


def sample_window(prep, rng, T_max=10 ** 7, visits_exactly=None):
    """A window drawn from the model itself: a seeded random walk from `start` to `end` over the out-edges (their probabilities
    renormalised per state), every emitting state drawing one observation from its distribution.  Returns (x, visits).
    visits_exactly: the walk leaves a counted state by its likeliest edge (on round the loop) until it has emitted that many
    counted observations, then by its least likely one (out of the loop) -- for windows longer than a walk would ever get."""
    n = int(prep.n_states)
    outs = [[] for _ in range(n)]
    for l in range(n):
        for e in range(int(prep.in_ptr[l]), int(prep.in_ptr[l + 1])):
            outs[int(prep.in_src[e])].append((l, float(np.exp(prep.in_logp[e]))))
    x, visits, st = [], 0, int(prep.start)
    while st != prep.end and len(x) < T_max:
        dst = [b for b, _ in outs[st]]
        p = np.array([q for _, q in outs[st]])
        if visits_exactly is not None and st < prep.silent_start and prep.count_inc[st] != 0:
            st = int(dst[int(np.argmax(p)) if visits < visits_exactly else int(np.argmin(p))])
        else:
            st = int(dst[rng.choice(len(dst), p=p / p.sum())])
        if st < prep.silent_start:
            if prep.emis_kind[st] == 1:
                sigma = 1.0 / np.sqrt(2.0 * prep.emis_b[st])
                x.append(rng.normal(prep.emis_a[st], sigma))
            else:
                x.append(rng.uniform(prep.emis_a[st], prep.emis_b[st]))
            visits += int(prep.count_inc[st] != 0)
    return np.array(x, np.float64), visits
