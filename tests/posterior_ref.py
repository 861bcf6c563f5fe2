"""Test helper: per-state posterior occupancy of an observation window -- forward-backward in log space, restated in numpy.

Independent of the product: nothing is imported from strique_amd, and the graph it runs on is the UN-BAKED one that
oracle.hmm_oracle.prepare() returns (CSR in-edges in graph order, emitting states first, silent states in topological order, `names`)
-- or any object with the same fields.  What it computes, over all paths from `start` to `end` that emit the T observations of x:

    log_lik = log sum_paths P(path, x)
    gamma_t(s) = P(the path emits x_t from emitting state s | x) = alpha_t(s) beta_t(s) / P
    w[s] = sum_t gamma_t(s),   wx[s] = sum_t gamma_t(s) x_t,   wxx[s] = sum_t gamma_t(s) x_t^2      over the t whose x_t is a number

alpha_t(s): log mass of the paths that reach s having emitted x_1..t (x_t from s); beta_t(s): log mass of the paths from s to `end`
that emit x_t+1..T.  Silent states are resolved inside a time step, level by level (forwards by their longest chain of silent
predecessors, backwards by their longest chain of silent successors).  A missing observation (NaN) has probability 1 under every
distribution; an observation outside a Uniform's support has probability 0 there.

Log space, parametrised by dtype: np.longdouble is the reference R, np.float64 shows what a float64 restatement loses.
"""
import numpy as np


def _lse(a, axis):
    """log sum exp along `axis`, one term after the other; -inf where every term is -inf.  (One ufunc call: the silent states of a
    flanked net lie in long chains, a level each, so a time step is hundreds of small gathers.)"""
    return np.logaddexp.reduce(a, axis=axis)


class _Edges(object):
    """Edges of a group of states as padded arrays: other[k, j], lp[k, j] (-inf padding); gather(V) = lse_j(V[other] + lp)."""

    def __init__(self, states, lists, dtype):
        deg = max([len(lists[l]) for l in states] + [1])
        self.states = np.array(states, np.int64)
        self.other = np.zeros((len(states), deg), np.int64)
        self.lp = np.full((len(states), deg), -np.inf, dtype)
        for k, l in enumerate(states):
            for j, (o, p) in enumerate(lists[l]):
                self.other[k, j] = o
                self.lp[k, j] = p

    def gather(self, V):
        return _lse(V[self.other] + self.lp, axis=1)


def _levels(n, ne, lists, ascending):
    """Silent states grouped by the longest chain of silent neighbours in `lists` behind them: in-edges in ascending order of the
    states (they are in topological order), out-edges in descending order."""
    level = {}
    for l in (range(ne, n) if ascending else range(n - 1, ne - 1, -1)):
        level[l] = max([level[o] + 1 for o, _ in lists[l] if o >= ne] + [0])
    return [[l for l in range(ne, n) if level[l] == v] for v in range(max(level.values()) + 1)]


def emitting_names(prep):
    """Names of the emitting states; unique, so that two orders of the same states can be matched."""
    names = list(prep.names[:int(prep.silent_start)])
    assert len(set(names)) == len(names), "emitting state names are not unique"
    return names


def posterior_ref(prep, x, dtype=np.longdouble):
    """(log_lik, status, w, wx, wxx) of the window x: arrays of silent_start entries in `dtype`, in the order of prep's emitting
    states.  status 1, -inf and zero rows when no path emits the window."""
    dt = np.dtype(dtype).type
    n, ne = int(prep.n_states), int(prep.silent_start)
    start, end = int(prep.start), int(prep.end)
    x = np.asarray(x, np.float64)
    T = len(x)
    NEG = dt(-np.inf)
    ins = [[] for _ in range(n)]
    outs = [[] for _ in range(n)]
    for l in range(n):
        for e in range(int(prep.in_ptr[l]), int(prep.in_ptr[l + 1])):
            k, p = int(prep.in_src[e]), dt(prep.in_logp[e])
            ins[l].append((k, p)); outs[k].append((l, p))
    emit_in = _Edges(list(range(ne)), ins, dtype)
    emit_out = _Edges(list(range(ne)), outs, dtype)
    sil_in = [_Edges(g, ins, dtype) for g in _levels(n, ne, ins, True)]
    sil_out = [_Edges(g, outs, dtype) for g in _levels(n, ne, outs, False)]
    kind = np.asarray(prep.emis_kind)[:ne]
    ea, eb, ec = (np.asarray(a, dtype)[:ne] for a in (prep.emis_a, prep.emis_b, prep.emis_c))

    def emission(t):
        if np.isnan(x[t]):
            return np.zeros(ne, dtype)
        xt = dt(x[t])
        d = xt - ea
        with np.errstate(invalid="ignore"):
            return np.where(kind == 1, ec - d * d * eb, np.where((xt >= ea) & (xt <= eb), ec, NEG))

    # forward: alpha[t] over the emitting states for t = 1 .. T (row t - 1), the whole vector only for the step in hand
    alpha = np.full((T, ne), NEG, dtype)
    L = np.full(n, NEG, dtype)
    L[start] = dt(0)
    for pl in sil_in:
        g = pl.gather(L)
        L[pl.states] = np.where(pl.states == start, dt(0), g)
    for t in range(T):
        new = emit_in.gather(L) + emission(t)
        alpha[t] = new
        L = np.full(n, NEG, dtype)
        L[:ne] = new
        for pl in sil_in:
            L[pl.states] = pl.gather(L)
    log_lik = L[end]
    zeros = np.zeros(ne, dtype)
    if not np.isfinite(log_lik):
        return dt(-np.inf), 1, zeros, zeros.copy(), zeros.copy()
    # backward: V holds b_j(x_t+1) beta_t+1(j) in its emitting entries and beta_t in its silent ones
    w, wx, wxx = zeros.copy(), zeros.copy(), zeros.copy()
    beta = np.full(ne, NEG, dtype)
    for t in range(T, 0, -1):
        V = np.full(n, NEG, dtype)
        if t < T:
            V[:ne] = beta + emission(t)
        for pl in sil_out:
            g = pl.gather(V)
            V[pl.states] = np.where(pl.states == end, dt(0), g) if t == T else g
        beta = emit_out.gather(V)
        if not np.isnan(x[t - 1]):
            gamma = np.exp(alpha[t - 1] + beta - log_lik)
            xt = dt(x[t - 1])
            w += gamma; wx += gamma * xt; wxx += gamma * xt * xt
    return log_lik, 0, w, wx, wxx


def counted_occupancy(prep, w):
    """sum of w over the states with count_inc != 0: E[v | x] on a window without NaN."""
    c = np.asarray(prep.count_inc[:int(prep.silent_start)]) != 0
    return w[c].sum()


def brute_force(prep, x):
    """The same five quantities by enumerating every start -> end path that emits len(x) observations (plain Python floats, linear
    space): for toy graphs and T <= 5 only."""
    n, ne = int(prep.n_states), int(prep.silent_start)
    start, end = int(prep.start), int(prep.end)
    x = [float(v) for v in x]
    T = len(x)
    outs = [[] for _ in range(n)]
    for l in range(n):
        for e in range(int(prep.in_ptr[l]), int(prep.in_ptr[l + 1])):
            outs[int(prep.in_src[e])].append((l, float(np.exp(prep.in_logp[e]))))

    def dens(s, v):
        if v != v:
            return 1.0
        if prep.emis_kind[s] == 1:
            d = v - float(prep.emis_a[s])
            return float(np.exp(float(prep.emis_c[s]) - d * d * float(prep.emis_b[s])))
        return float(np.exp(float(prep.emis_c[s]))) if float(prep.emis_a[s]) <= v <= float(prep.emis_b[s]) else 0.0

    total = 0.0
    acc = [[0.0, 0.0, 0.0] for _ in range(ne)]
    stack = [(start, 0, 1.0, ())]
    while stack:
        st, t, p, emitted = stack.pop()
        if st == end and t == T:
            total += p
            for k, s in enumerate(emitted):
                if x[k] == x[k]:
                    acc[s][0] += p; acc[s][1] += p * x[k]; acc[s][2] += p * x[k] * x[k]
        for dst, q in outs[st]:
            if dst < ne:
                if t < T:
                    b = dens(dst, x[t])
                    if b > 0.0:
                        stack.append((dst, t + 1, p * q * b, emitted + (dst,)))
            else:
                stack.append((dst, t, p * q, emitted))
    if total == 0.0:
        return -np.inf, 1, np.zeros(ne), np.zeros(ne), np.zeros(ne)
    a = np.array(acc) / total
    return float(np.log(total)), 0, a[:, 0], a[:, 1], a[:, 2]
