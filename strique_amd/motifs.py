"""The rule of the motif track (strq_motif_track, csrc/motif_kernels.hip): which repeat unit each stretch of a repeat array is made
of.  Pure Python and numpy, no device: stated once here, the model builder and the tests take it from this module.

`count` models a locus as prefix | one unit x n | suffix with the unit the config names.  For loci such as RFC1 (AAAAG, AAAGG or
AAGGG), FGF14 (GAA or GAAGGA) or the FAME loci (TTTTA with a TTTCA insertion) the question is which unit the array is made of.

Candidates.  Candidate 0 is the target's `repeat`; one to three alternatives follow, so K is 2 to 4.  All are given on the + strand
like `repeat`; on the - strand each is reverse-complemented (`strand_units`), and results stay in configured order.  Two candidates
with the same `key` -- the unit's primitive root, rotated to its lexicographically smallest rotation -- spell the same array and
are refused.

Loop model.  The emitting states of the repeat section of hmm.FlankedRepeatModel(unit, ...) -- after bake() the states with tag 1;
they do not depend on the flanks -- in baked order, with the log-probabilities bake() leaves on the edges among them (out-edge
normalisation and the spliced e1 / e2 -> dummy and dummy -> s1 / s2 hops included).  Every state can be entered with
-log(n_emit) and left with log-probability 0; the `leave_repeat` edges are dropped.  `loop_arrays` returns it in the field layout
of hmm.BakedHMM: start is state n_emit, end is state n_emit + 1.  A loop model has 2 * columns + 2 emitting states, columns =
len(extend_repeat(unit, k)[0]) - k + 1, and at most MAX_EMIT of them: units of up to 31 nt at k = 6.

Segments.  A stretch of T observations is cut into n_seg = max(1, T // S) segments of S observations; segment i < n_seg - 1 is
[i S, (i + 1) S), the last one runs to T -- so every segment has between S and 2 S - 1 observations, except the single segment of a
stretch shorter than S.  S = SEGMENT = 256 by default: a resolution chosen on synthetic reads (about seven 5-nt units at the
generator's dwell), not a tuned value.

Scores.  V[i][j] is the maximum, over the states, of the Viterbi value after the last observation of segment i under candidate j's
loop model: float64, best = max_e(v_prev[src_e] + in_logp[e]), v = best + log emission, a missing observation (NaN) has log
emission 0.  These are comparison scores, not likelihoods of complete models.  The winner of a segment is the candidate with the
largest V (the lowest index among equals), its margin (V_first - V_second) / length.  Per stretch, obs_won[j] is the number of
observations of the segments candidate j won, the majority the candidate with the most (the lowest index among equals),
share[j] = obs_won[j] / T, and the runs are the maximal runs of equal winners."""
import math
from collections import namedtuple

import numpy as np

from . import hmm

SEGMENT, SEGMENT_MIN, SEGMENT_MAX = 256, 32, 4096
MAX_ALTERNATIVES = 3
MAX_CANDIDATES = 1 + MAX_ALTERNATIVES
MAX_EMIT = 64

_COMPLEMENT = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}


def _revcomp(s):
    return "".join(_COMPLEMENT[b] for b in reversed(s))


def key(unit):
    """What array a unit spells: its primitive root (the shortest r with unit == r * n), rotated to its smallest rotation."""
    unit = str(unit).upper()
    root = unit
    for n in range(1, len(unit) + 1):
        if len(unit) % n == 0 and unit[:n] * (len(unit) // n) == unit:
            root = unit[:n]
            break
    return min(root[i:] + root[:i] for i in range(len(root))) if root else root


def n_emit(unit, kmer):
    """Emitting states of the loop model of `unit`: a match and an insert state per column, and the two dummy states."""
    return 2 * (len(hmm.extend_repeat(unit, kmer)[0]) - kmer + 1) + 2


def check(repeat, alternatives, kmer):
    """The candidates, upper-cased, as a tuple: `repeat` first, then the alternatives.  ValueError for: an empty unit, letters beyond
    ACGT, no alternative or more than MAX_ALTERNATIVES, a unit whose loop model has more than MAX_EMIT emitting states, two
    candidates with the same key.  kmer None: the limit on the states is left to a later call (a definition file is read before
    the pore model is)."""
    if isinstance(alternatives, str):
        alternatives = [alternatives]
    units = (str(repeat).upper(),) + tuple(str(u).upper() for u in alternatives)
    if not 1 <= len(units) - 1 <= MAX_ALTERNATIVES:
        raise ValueError("motifs: between 1 and %d alternative units per target, got %d" % (MAX_ALTERNATIVES, len(units) - 1))
    for u in units:
        if not u:
            raise ValueError("motifs: an empty unit")
        if set(u) - set("ACGT"):
            raise ValueError("motifs: unit %r: only the letters A, C, G, T" % u)
        if kmer is not None and n_emit(u, kmer) > MAX_EMIT:
            raise ValueError("motifs: unit %s (%d nt): its loop model has %d emitting states, at most %d are supported"
                             % (u, len(u), n_emit(u, kmer), MAX_EMIT))
    for i, u in enumerate(units):
        for v in units[:i]:
            if key(u) == key(v):
                raise ValueError("motifs: units %s and %s spell the same array (key %s)" % (v, u, key(u)))
    return units


def check_segment(segment):
    segment = int(segment)
    if not SEGMENT_MIN <= segment <= SEGMENT_MAX:
        raise ValueError("motifs: the segment length must lie between %d and %d, got %d" % (SEGMENT_MIN, SEGMENT_MAX, segment))
    return segment


def strand_units(units, strand):
    """The candidates as the signal of `strand` reads them, in configured order."""
    if strand == '+':
        return tuple(units)
    if strand == '-':
        return tuple(_revcomp(u) for u in units)
    raise ValueError("motifs: strand must be + or -")


def loop_arrays(baked):
    """The loop model of a baked FlankedRepeatModel as a hmm.BakedHMM (see the module text)."""
    emit = [s for s in range(baked.silent_start) if baked.tag[s] == 1]
    ne = len(emit)
    if not ne:
        raise ValueError("motifs: the model has no repeat section")
    new = {old: k for k, old in enumerate(emit)}
    start, end = ne, ne + 1
    enter = -math.log(ne)
    in_ptr = np.zeros(ne + 3, np.int32)
    in_src, in_logp = [], []
    for k, old in enumerate(emit):
        for e in range(baked.in_ptr[old], baked.in_ptr[old + 1]):
            src = int(baked.in_src[e])
            if src in new:                                  # sources ascend in the baked model, and so do their new numbers
                in_src.append(new[src]); in_logp.append(float(baked.in_logp[e]))
        in_src.append(start); in_logp.append(enter)
        in_ptr[k + 1] = len(in_src)
    in_ptr[start + 1] = len(in_src)                         # nothing enters start
    in_src += list(range(ne)); in_logp += [0.0] * ne
    in_ptr[end + 1] = len(in_src)
    pad = lambda a, dtype: np.concatenate([np.asarray(a, dtype)[emit], np.zeros(2, dtype)])
    return hmm.BakedHMM(ne + 2, ne, start, end, in_ptr, np.array(in_src, np.int32), np.array(in_logp, np.float64),
                        np.asarray(baked.emis_kind, np.int32)[emit], np.asarray(baked.emis_a, np.float64)[emit],
                        np.asarray(baked.emis_b, np.float64)[emit], np.asarray(baked.emis_c, np.float64)[emit],
                        pad(baked.count_inc, np.int32), pad(baked.tag, np.int32),
                        [baked.names[s] for s in emit] + ['loop-start', 'loop-end'], np.asarray(baked.orig_index, np.int32)[emit],
                        np.full(ne + 2, -1, np.int32), np.full(ne + 2, -1, np.int32))


_ANY_FLANK = "ACGTTGCATCAGGATC"          # the loop does not depend on the flanks: any flank that yields a profile will do


def loop_model(unit, pm, config=None):
    """The loop model of `unit` (as the strand reads it) under pore model `pm` and the HMM config."""
    return loop_arrays(hmm.FlankedRepeatModel(unit, _ANY_FLANK, _ANY_FLANK, pm, config).baked)


def segments(T, segment=SEGMENT):
    """[(begin, end)] of the segments of a stretch of T >= 1 observations."""
    T, S = int(T), int(segment)
    if T < 1:
        raise ValueError("motifs: a stretch holds at least one observation")
    n = max(1, T // S)
    return [(i * S, (i + 1) * S if i < n - 1 else T) for i in range(n)]


def winners(V):
    """Per segment the candidate with the largest V (the lowest index among equals): V of shape (n_seg, K)."""
    return np.argmax(np.asarray(V, np.float64), axis=1).astype(np.int32)


def margins(V, bounds):
    """Per segment (V_first - V_second) / length."""
    top = np.sort(np.asarray(V, np.float64), axis=1)[:, ::-1]
    with np.errstate(invalid="ignore"):
        return (top[:, 0] - top[:, 1]) / np.array([e - b for b, e in bounds], np.float64)


Summary = namedtuple("Summary", "obs_won majority shares")


def summary(win, bounds, n_cand):
    """obs_won[j], the majority and share[j] of a stretch from the winners of its segments."""
    obs_won = [0] * n_cand
    for w, (b, e) in zip(win, bounds):
        obs_won[int(w)] += e - b
    T = bounds[-1][1]
    majority = max(range(n_cand), key=lambda j: (obs_won[j], -j))
    return Summary(tuple(obs_won), majority, tuple(o / T for o in obs_won))


def runs(win, bounds, first_sample=0):
    """The maximal runs of equal winners as (candidate, first_sample, end_sample), in signal order; `first_sample`: the raw sample of
    the stretch's first observation."""
    out = []
    for w, (b, e) in zip(win, bounds):
        if out and out[-1][0] == int(w):
            out[-1] = (out[-1][0], out[-1][1], first_sample + e)
        else:
            out.append((int(w), first_sample + b, first_sample + e))
    return out


# ---- the definition file (`count --motif-units`) ----------------------------------------------------------------------------------
def parse_definitions(stream, repeats):
    """{target: alternatives} of a definition file: one line per target, `target<TAB>U1[,U2[,U3]]`.  Lines that start with # and
    blank lines are skipped.  repeats: {target: (repeat, k-mer length or None)} of the configured targets.  ValueError for a malformed line,
    a duplicate, an unknown target and anything `check` rejects."""
    out = {}
    for no, line in enumerate(stream, 1):
        text = line.rstrip('\r\n')
        if not text.strip() or text.lstrip().startswith('#'):
            continue
        f = text.split('\t')
        if len(f) != 2 or not f[0].strip():
            raise ValueError("motif definitions, line %d: expected target<TAB>U1[,U2[,U3]]" % no)
        name = f[0].strip()
        if name in out:
            raise ValueError("motif definitions, line %d: target %s is defined twice" % (no, name))
        if name not in repeats:
            raise ValueError("motif definitions, line %d: unknown target %s" % (no, name))
        try:
            out[name] = check(repeats[name][0], [u.strip() for u in f[1].split(',')], repeats[name][1])[1:]
        except ValueError as e:
            raise ValueError("motif definitions, line %d (%s): %s" % (no, name, e))
    return out


# ---- the side file (one row per count row) ---------------------------------------------------------------------------------------
HEADER = ['ID', 'target', 'strand', 'count', 'n_segments', 'majority_unit', 'shares', 'count_m', 'log_p_m', 'runs']
Row = namedtuple("Row", "units n_segments majority shares count_m log_p_m runs")


def format_row(read_id, target, strand, count, rec):
    """One row.  count: the count of the count row; rec: None (not scored, or a target without motifs) or a Row -- the candidates
    as configured, the segments, the majority candidate, the shares in configured order (written with four decimals), the count
    and log-probability under the majority unit (None: no decode; log_p_m written with repr) and the runs as (candidate,
    first_sample, end_sample), written `unit:first-end`.  Lists joined by commas, '-' for a field without a value."""
    head = [str(read_id), str(target), str(strand), str(int(count))]
    if rec is None:
        return '\t'.join(head + ['-'] * 6)
    units = rec.units
    return '\t'.join(head + [str(int(rec.n_segments)), units[rec.majority], ','.join('%.4f' % s for s in rec.shares),
                             '-' if rec.count_m is None else str(int(rec.count_m)), '-' if rec.log_p_m is None else repr(float(rec.log_p_m)),
                             ','.join('%s:%d-%d' % (units[c], a, b) for c, a, b in rec.runs)])


def parse(stream):
    """Rows of the side file: [(ID, target, strand, count, None or (n_segments, majority unit, shares as written, count_m or None,
    log_p_m or None, runs as (unit, first_sample, end_sample)))]."""
    rows, seen_header = [], False
    for line in stream:
        if not line.strip():
            continue
        f = line.rstrip('\n').split('\t')
        if not seen_header:
            if f != HEADER:
                raise ValueError("not a --motifs file")
            seen_header = True
            continue
        if len(f) != len(HEADER):
            raise ValueError("motifs row of %s: %r" % (f[0], f[1:]))
        if f[4] == '-':
            if f[5:] != ['-'] * 5:
                raise ValueError("motifs row of %s: %r" % (f[0], f[1:]))
            rec = None
        else:
            runs = []
            for item in f[9].split(','):
                unit, span = item.split(':')
                a, b = span.split('-')
                runs.append((unit, int(a), int(b)))
            rec = (int(f[4]), f[5], tuple(float(s) for s in f[6].split(',')), None if f[7] == '-' else int(f[7]),
                   None if f[8] == '-' else float(f[8]), runs)
        rows.append((f[0], f[1], f[2], int(f[3]), rec))
    return rows
