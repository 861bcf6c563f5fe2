"""The rule of the second normalisation step (`repeatCounter.set_renorm(min_share)`, `count --renorm`, strq_set_renorm): scale and
shift of a read's normalised signals refitted against what the read is made of.  Pure numpy, no device: the GPU applies the same
rule in renorm_kernels.hip, and the tests compare the two bit for bit -- the fit is integer arithmetic throughout.

detect() maps a read into the pore model's domain with statistics of the whole read (medians of its 1 % / 99 % tails against those
of the model's k-mer means, scripts/STRique.py:150-180).  That assumes the read's k-mer composition looks like the model's.  A read
that is mostly repeat holds len(repeat) k-mers: its tails are their noise tails, the map is stretched and the flanks are not found.
Here the map of each signal is corrected by (alpha, beta) chosen to maximise the likelihood of its histogram under a mixture
w * (this target's repeat k-mers) + (1 - w) * (all k-mers), and the read keeps its maps when the fitted repeat share w is below
`min_share` (there is no default: below the threshold the fit costs a little flank score, above it it rescues the read --
README, "Renorm").

Not refitted: the 8-bit quantisation z * 24 + 127 with the read's own MAD.  One repeat per read.  Not available in a scan.
"""
import numpy as np

GRID = 1024                      # bins; the model range [model_min, model_max] covers bins 256 .. 767
HALF = 512                       # the pivot p is the centre of this bin
A_ONE = 64                       # alpha = a / A_ONE
A_MIN, A_MAX = 24, 104
B_MAX = 128                      # |b| <= a quarter of the model range, in bins
N_W = 15
W = np.array([round(0.07 * k, 2) for k in range(N_W)])      # 0 .. 0.98
P_FLOOR = 1e-9
Q_SCALE = 1024
Q_OUT = int(np.rint(Q_SCALE * np.log(P_FLOOR)))
# the schedule, part of the rule: a coarse grid over (a, b), every w; then every (a, b) within FINE_A / FINE_B of the coarse winner
COARSE_A, COARSE_B = 2, 4
FINE_A, FINE_B = 1, 3
SIGNALS = ('morph', 'filtered', 'raw')      # order of the per-signal entries of a record


def grid(model_min, model_max):
    """(lo, d, p): start of bin 0, bin width, pivot."""
    d = (model_max - model_min) / 512
    lo = model_min - 256 * d
    p = lo + (HALF + 0.5) * d
    return lo, d, p


def _mixture(centres, means, stdvs):
    out = np.zeros(len(centres))
    for m, s in zip(means, stdvs):
        out += np.exp(-0.5 * ((centres - m) / s) ** 2) / (s * np.sqrt(2 * np.pi))
    return out / len(means)


def repeat_kmers(repeat, k):
    """The len(repeat) k-mers of the tandem array of `repeat` (as the strand reads it)."""
    s = repeat * (k // len(repeat) + 2)
    return [s[i:i + k] for i in range(len(repeat))]


def tables(kmer_stats, k, model_min, model_max, repeat):
    """(Q int16 [N_W, GRID], A int32 [A_MAX + 1]) of one strand of a target.  kmer_stats: {k-mer: (mean, stdv)}; repeat: the unit as
    the strand reads it (reverse-complemented for '-')."""
    lo, d, _ = grid(model_min, model_max)
    centres = lo + (np.arange(GRID) + 0.5) * d
    rep = [kmer_stats[km] for km in repeat_kmers(repeat.upper(), k)]
    p_rep = _mixture(centres, [v[0] for v in rep], [v[1] for v in rep])
    allv = list(kmer_stats.values())
    p_bg = _mixture(centres, [v[0] for v in allv], [v[1] for v in allv])
    Q = np.rint(Q_SCALE * np.log(np.maximum(W[:, None] * p_rep[None, :] + (1 - W[:, None]) * p_bg[None, :], P_FLOOR)))
    if np.abs(Q).max() >= 2 ** 15:
        raise ValueError("renorm: score table outside int16")
    A = np.zeros(A_MAX + 1, np.int32)
    A[1:] = np.rint(Q_SCALE * np.log(np.arange(1, A_MAX + 1) / A_ONE)).astype(np.int32)
    return Q.astype(np.int16), A


def bins(x, c1, h1, h2, c2, lo, d):
    """Bin of every sample under its current, unclipped map; -1 outside the grid (or not a number)."""
    with np.errstate(all='ignore'):
        v = (np.asarray(x, np.float64) - c1) / h1 * h2 + c2
        t = np.floor((v - lo) / d)
    ok = (t >= 0) & (t < GRID)
    return np.where(ok, t, -1).astype(np.int64)


def histogram(x, c1, h1, h2, c2, lo, d):
    b = bins(x, c1, h1, h2, c2, lo, d)
    return np.bincount(b[b >= 0], minlength=GRID).astype(np.int64)


def _scores(h, Q, A, a_list, b_list):
    """S[a, b, w] (int64) over the given a and b."""
    nz = np.nonzero(h)[0]
    hv = h[nz].astype(np.int64)
    N = int(h.sum())
    Qp = np.concatenate([Q.astype(np.int64), np.full((N_W, 1), Q_OUT, np.int64)], axis=1)
    b_arr = np.asarray(b_list, np.int64)
    S = np.zeros((len(a_list), len(b_arr), N_W), np.int64)
    for k, a in enumerate(a_list):
        base = HALF + (a * (nz - HALF)) // A_ONE                  # floor division
        idx = base[None, :] + b_arr[:, None]
        idx = np.where((idx >= 0) & (idx < GRID), idx, GRID)
        S[k] = (Qp[:, idx] @ hv).T + N * int(A[a])
    return S


def _best(S, a_list, b_list):
    k = int(np.argmax(S))                                        # first maximum in C order: the smallest (a, b, w)
    ia, ib, iw = np.unravel_index(k, S.shape)
    return int(a_list[ia]), int(b_list[ib]), int(iw), int(S[ia, ib, iw])


def fit(h, Q, A):
    """(a, b, w, score) of a histogram, or None for an empty one."""
    h = np.asarray(h, np.int64)
    if h.sum() == 0:
        return None
    a_c = list(range(A_MIN, A_MAX + 1, COARSE_A)); b_c = list(range(-B_MAX, B_MAX + 1, COARSE_B))
    a0, b0, _, _ = _best(_scores(h, Q, A, a_c, b_c), a_c, b_c)
    a_f = list(range(max(A_MIN, a0 - FINE_A), min(A_MAX, a0 + FINE_A) + 1))
    b_f = list(range(max(-B_MAX, b0 - FINE_B), min(B_MAX, b0 + FINE_B) + 1))
    return _best(_scores(h, Q, A, a_f, b_f), a_f, b_f)


def fold(c1, h1, h2, c2, a, b, p, d):
    """(c1', h1') of a signal's map after the fit (a, b)."""
    alpha = a / A_ONE
    h1n = h1 / alpha
    t = alpha * (c2 - p)
    t = t + p
    t = t + b * d
    t = t - c2
    t = t * h1n
    t = t / h2
    return c1 - t, h1n


def level_values(m_c1, m_h1, h2, c2, clip_lo, clip_hi):
    """The 256 values of the morphology signal's levels under its map (float32, as the alignment takes them)."""
    v = (np.arange(256, dtype=np.float64) - m_c1) / m_h1
    v = v * h2 + c2
    return np.clip(v, clip_lo, clip_hi).astype(np.float32)


def apply(maps, signals, Q, A, model_min, model_max, min_share, status=0):
    """The whole rule for one read.  maps: {'morph': (c1, h1), 'filtered': ..., 'raw': ... or absent}, plus 'h2', 'c2'; signals: the
    samples of each (the 8-bit levels for 'morph').  Returns (new maps, record): record = (applied, {signal: None or (a, b, w, score)}).
    `min_share` in (0, 1)."""
    if not 0 < min_share < 1:
        raise ValueError("renorm: min_share must be inside (0, 1)")
    lo, d, p = grid(model_min, model_max)
    h2, c2 = maps['h2'], maps['c2']
    fits = {s: None for s in SIGNALS}
    out = dict(maps)
    if status != 0 or Q is None:
        return out, (0, fits)
    for s in SIGNALS:
        if s in signals and s in maps:
            c1, h1 = maps[s]
            fits[s] = fit(histogram(signals[s], c1, h1, h2, c2, lo, d), Q, A)
    f = fits['filtered']
    applied = int(f is not None and W[f[2]] >= min_share)
    if applied:
        for s in SIGNALS:
            if fits[s] is not None:
                out[s] = fold(maps[s][0], maps[s][1], h2, c2, fits[s][0], fits[s][1], p, d)
    return out, (applied, fits)


# ---------------------------------------------------------------------------------------------
# the side file of `count --renorm MIN_SHARE --renorm-out FILE`
# ---------------------------------------------------------------------------------------------
HEADER = ['ID', 'target', 'strand', 'applied'] + ['%s_%s' % (s, f) for s in SIGNALS for f in ('share', 'alpha', 'beta')]


def report(rec, d):
    """What the file says of one read, from the record (applied, {signal: None or (a, b, w, score)}) and the grid's bin width d:
    (applied, ((share, alpha, beta in pA) or None per signal, in the order of SIGNALS)); None for no record."""
    if rec is None:
        return None
    applied, fits = rec
    out = []
    for s in SIGNALS:
        f = fits.get(s)
        out.append(None if f is None else (float(W[f[2]]), f[0] / A_ONE, f[1] * d))
    return int(applied), tuple(out)


def pack(rep):
    """A report as it travels between ranks."""
    return ';'.join([str(int(rep[0]))] + ['-' if f is None else ','.join(repr(float(x)) for x in f) for f in rep[1]])


def unpack(text):
    f = text.split(';')
    return int(f[0]), tuple(None if c == '-' else tuple(float(x) for x in c.split(',')) for c in f[1:])


def format_row(read_id, target, strand, rep):
    """One row of the file.  rep: None (no fit was tried: not a read of a renorm run) or a report."""
    if rep is None:
        return '\t'.join([str(read_id), str(target), str(strand), '-'] + ['-'] * 9)
    vals = []
    for f in rep[1]:
        vals += ['-'] * 3 if f is None else [repr(float(x)) for x in f]
    return '\t'.join([str(read_id), str(target), str(strand), str(int(rep[0]))] + vals)


def parse(stream):
    """Rows of a --renorm-out file: [(ID, target, strand, report or None)]."""
    rows, seen_header = [], False
    for line in stream:
        if not line.strip():
            continue
        f = line.rstrip('\n').split('\t')
        if not seen_header:
            if f != HEADER:
                raise ValueError("not a --renorm-out file")
            seen_header = True
            continue
        if len(f) != len(HEADER):
            raise ValueError("renorm row of %s: %r" % (f[0], f[1:]))
        if f[3] == '-':
            rows.append((f[0], f[1], f[2], None))
            continue
        fits = []
        for k in range(len(SIGNALS)):
            c = f[4 + 3 * k: 7 + 3 * k]
            fits.append(None if c[0] == '-' else (float(c[0]), float(c[1]), float(c[2])))
        rows.append((f[0], f[1], f[2], (int(f[3]), tuple(fits))))
    return rows
