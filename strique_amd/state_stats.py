"""The rule of the state statistics (strq_set_state_stats, strq_viterbi_state_stats, state_stats_kernels.hip): what the best path of
a decode assigns to every emitting state.  Pure Python, no device: the kernel is held to this to the bit.

A window x[0 .. T) is what the decode sees: normalised and clipped observations, NaN = missing.  path[t] is the emitting state, in
baked order, of observation t on the best path -- the path of strq_viterbi, with its tie-breaks.  For every emitting state
s in [0, silent_start):

    n[s]      int64: the observations t with path[t] == s that are numbers (a NaN is neither counted nor summed)
    sum[s]    float64 from +0.0, the observations added one at a time in ascending t
    sumsq[s]  float64 from +0.0, their squares added one at a time in ascending t; a square is rounded to float64 before it is
              added (no fused multiply-add)

A state the path never visits has 0, +0.0, +0.0.  The order is part of the rule, so the three rows are defined to the bit: an
implementation cannot use floating-point atomics or a tree reduction.
"""
import numpy as np


def state_stats(x, path, n_emit):
    """(n, sum, sumsq) of one window under the rule above: np.int64, np.float64, np.float64 arrays of n_emit entries."""
    x = np.asarray(x, np.float64)
    if len(path) != len(x):
        raise ValueError("one state per observation")
    n = [0] * n_emit
    s1 = [0.0] * n_emit
    s2 = [0.0] * n_emit
    for v, s in zip(x.tolist(), np.asarray(path).tolist()):
        if not 0 <= s < n_emit:
            raise ValueError("state %d is no emitting state" % s)
        if v != v:
            continue
        n[s] += 1
        s1[s] = s1[s] + v          # Python floats are IEEE doubles: one rounding per operation
        q = v * v
        s2[s] = s2[s] + q
    return np.array(n, np.int64), np.array(s1, np.float64), np.array(s2, np.float64)


def mean_sd(n, s, q):
    """Mean and observed standard deviation of one accumulator triple (n > 0): sqrt(max(0, q / n - mean^2))."""
    mean = s / n
    return mean, max(0.0, q / n - mean * mean) ** 0.5
