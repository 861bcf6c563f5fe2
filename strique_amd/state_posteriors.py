"""The rule of the state posteriors (strq_set_state_posteriors, strq_forward_state_stats, posterior_kernels.hip): what ALL paths of a
model, weighted by their probability, assign to every emitting state -- the soft counterpart of strique_amd/state_stats.py, which
gives every observation wholly to the state of the best path.  Pure Python, no device.

A window x[0 .. T) is what the decode sees: normalised and clipped observations, NaN = missing, read through vit_observation.  The
model has `start` and `end`; its transition probabilities are those the forward pass uses -- exp(in_logp_sum) where bake() merged
parallel paths into one edge (strq_model_set_forward_logp), exp(in_logp) everywhere else.  Then

    P          = sum over all start -> end paths that emit the T observations of P(path, x)
    log_lik    = log P                                    the quantity strq_forward_batch reports
    gamma_t(s) = P(the path emits x_t from emitting state s | x)
                 a missing observation has emission probability 1 under every distribution; an observation outside a Uniform's
                 support has probability 0 there

and for every emitting state s in [0, silent_start) (baked order), summed over the t whose x_t is a number:

    w[s]   = sum_t gamma_t(s)            wx[s]  = sum_t gamma_t(s) x_t            wxx[s] = sum_t gamma_t(s) x_t^2

status 0: ok.  status 1: no path, P = 0 -- all rows are +0.0 and log_lik is -inf.  (The entry points add a status of their own for a
window whose workspace exceeds the budget: zero rows, log_lik valid.)

Identities (the tests use them):
    sum_s gamma_t(s) = 1 for every t, so  sum_s w[s]  is the number of observations that are numbers;
    on a window without NaN,  sum over the counted states of w[s] = E[v | x],  the visits_mean of strq_forward_batch with c0 = 0.

The results are float64 and NOT defined to the bit against a restatement: the kernels work in linear space with a power-of-two
rescale after every time step, this module and the tests' reference in log space, and the two round differently -- exactly as for
`count --confidence`.  On the GPU they are deterministic to the bit: one wave sums a window in an order fixed by the model image and
t; there are no floating-point atomics and no tree reduction, and nothing depends on the launch geometry, on which windows share a
launch or on how a batch was cut into pieces.
"""
import numpy as np


def _lse(a):
    m = a.max(axis=1)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return ms + np.log(np.exp(a - ms[:, None]).sum(axis=1))


class _Rows(object):
    """Padded edge rows of a group of states: gather(V) = log sum_j exp(V[other[k, j]] + lp[k, j])."""

    def __init__(self, states, lists):
        deg = max([len(lists[l]) for l in states] + [1])
        self.states = np.array(states, np.int64)
        self.other = np.zeros((len(states), deg), np.int64)
        self.lp = np.full((len(states), deg), -np.inf)
        for k, l in enumerate(states):
            for j, (o, p) in enumerate(lists[l]):
                self.other[k, j] = o; self.lp[k, j] = p

    def gather(self, V):
        return _lse(V[self.other] + self.lp)


def state_posteriors(baked, x):
    """(log_lik, status, w, wx, wxx) of one window under the rule above, float64 in log space: np.float64 arrays of silent_start
    entries.  `baked`: a hmm.BakedHMM, or any object with its graph fields."""
    n, ne, start, end = int(baked.n_states), int(baked.silent_start), int(baked.start), int(baked.end)
    lp_all = getattr(baked, "in_logp_sum", None)
    lp_all = baked.in_logp if lp_all is None else lp_all
    x = np.asarray(x, np.float64)
    T = len(x)
    ins = [[] for _ in range(n)]; outs = [[] for _ in range(n)]
    for l in range(n):
        for e in range(int(baked.in_ptr[l]), int(baked.in_ptr[l + 1])):
            ins[l].append((int(baked.in_src[e]), float(lp_all[e]))); outs[int(baked.in_src[e])].append((l, float(lp_all[e])))
    # silent states one at a time: forwards in topological order, backwards in the reverse order
    sil_in = [_Rows([l], ins) for l in range(ne, n)]
    sil_out = [_Rows([l], outs) for l in range(n - 1, ne - 1, -1)]
    e_in, e_out = _Rows(list(range(ne)), ins), _Rows(list(range(ne)), outs)
    kind = np.asarray(baked.emis_kind)[:ne]
    ea, eb, ec = (np.asarray(a, np.float64)[:ne] for a in (baked.emis_a, baked.emis_b, baked.emis_c))

    def emission(t):
        if np.isnan(x[t]):
            return np.zeros(ne)
        d = x[t] - ea
        return np.where(kind == 1, ec - d * d * eb, np.where((x[t] >= ea) & (x[t] <= eb), ec, -np.inf))

    alpha = np.full((T, ne), -np.inf)
    L = np.full(n, -np.inf)
    L[start] = 0.0
    for r in sil_in:
        if r.states[0] != start:
            L[r.states] = r.gather(L)
    for t in range(T):
        alpha[t] = e_in.gather(L) + emission(t)
        L = np.full(n, -np.inf)
        L[:ne] = alpha[t]
        for r in sil_in:
            L[r.states] = r.gather(L)
    log_lik = float(L[end])
    w, wx, wxx = np.zeros(ne), np.zeros(ne), np.zeros(ne)
    if not np.isfinite(log_lik):
        return -np.inf, 1, w, wx, wxx
    beta = np.full(ne, -np.inf)
    for t in range(T, 0, -1):
        V = np.full(n, -np.inf)
        if t < T:
            V[:ne] = beta + emission(t)
        for r in sil_out:
            V[r.states] = 0.0 if (t == T and r.states[0] == end) else r.gather(V)
        beta = e_out.gather(V)
        if not np.isnan(x[t - 1]):
            g = np.exp(alpha[t - 1] + beta - log_lik)
            w += g; wx += g * x[t - 1]; wxx += g * x[t - 1] * x[t - 1]
    return log_lik, 0, w, wx, wxx
