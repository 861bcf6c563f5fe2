"""Reference of tract positions for the tests: where the counted emissions of every tract lie.  Nothing of the product is imported here.

The positions are read off orc.viterbi's state path with `tract_of`, as tests/tract_ref.py's decode_a reads off the counts: observation
t belongs to tract j when the path emits it from a state whose tract is j.  Model level: observation indices.  Pipeline: raw-signal
samples prefix_begin + t on the window of the tract decode, in configured order (tract_ref.configured)."""
import numpy as np

import tract_ref as tr
from oracle import strique_oracle as orc


def decode(m, tract_of, K, x):
    """(logp, counts[K], positions or None, status): status 0 ok, 1 no path; positions a list of K ascending int64 arrays."""
    logp, path, _ = orc.viterbi(m, x)
    if path is None:
        return logp, [0] * K, None, 1
    path = np.asarray(path, np.int64)
    assert len(path) == len(x)                                       # one emitting state per observation
    t = np.asarray(tract_of)[path] if len(path) else np.zeros(0, np.int64)
    pos = [np.nonzero(t == j)[0].astype(np.int64) for j in range(K)]
    return logp, [len(p) for p in pos], pos, 0


def window(sig, tc, pm, params):
    """(row, prefix_begin, x): the oracle's detect() row of the flanked classifier `tc`, and the window of the tract decode -- the
    normalised filtered signal over [prefix_begin, suffix_end) -- or None where the rule gives no tract record (tract_ref.record)."""
    sig = np.asarray(sig)
    row, info = orc.detect(sig, tc, pm, params)
    flt = orc.medfilt3(sig)
    normalised = np.isfinite(np.median(flt)) and orc.mad(flt) > 0
    b, e = info["prefix_begin"], info["suffix_end"]
    gate = b < e and row[1] > 0.0 and row[2] > 0.0
    if not (gate and normalised and row[3] != 0):
        return row, b, None
    return row, b, pm.normalize_minmax(flt.astype(np.float64))[b:e]


def record_on(model_arrays, tract_of, K, bias, strand, b, x):
    """None or (counts, log_p, positions), counts and positions in configured order, positions as raw-signal samples."""
    if x is None:
        return None
    logp, visits, pos, status = decode(model_arrays, tract_of, K, x)
    if status:
        return None
    return (tuple(tr.configured([v + q for v, q in zip(visits, bias)], strand)), logp, tuple(tr.configured([p + b for p in pos], strand)))


def record(sig, tc, m, pm, params):
    """(row, record) of one read on the reference's own un-baked net; m: (model dict of tract_ref.model, strand) or None."""
    row, b, x = window(sig, tc, pm, params)
    if m is None:
        return row, None
    model_, strand = m
    return row, record_on(model_["prep"], model_["tract_of"], model_["K"], model_["bias"], strand, b, x)


def same_positions(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)) for g, w in zip(got, want))
