"""The rule of a scan (`repeatCounter.scan_batch`, `count --scan`, strq_scan_batch_reads): which of several candidates --
a candidate is one strand of one target -- a read spans, judged from the flank alignments detect() makes anyway
(scripts/STRique.py:590-601).  Pure Python, no device: the GPU applies the same rule in scan_select_kernel
(strique_amd/csrc/scan_kernels.hip), and the tests compare the two.
"""

# There is no default min_score.  Measured with the CPU oracle over clean, empirical-noise and target-free reads of 5 to 50 kb and
# the bundled real read ("Scan"), the keys of wrong candidates and of true candidates overlap on the empirical-noise
# reads, so no threshold is right for everybody: the caller names one (`count --scan-scores` writes what it is chosen from).


def key(score_prefix, score_suffix):
    """min(score_prefix, score_suffix) as the kernel takes it (eligible() keeps a NaN out before it is compared)."""
    return score_prefix if score_prefix < score_suffix else score_suffix


def eligible(scores, geometry, min_score):
    """scores: (score_prefix, score_suffix); geometry: (prefix_begin, prefix_end, suffix_begin, suffix_end)."""
    # both scores against min_score, which is key >= min_score for numbers and False for a NaN in either place
    return geometry[0] < geometry[3] and scores[0] >= min_score and scores[1] >= min_score


def select(scores, geometry, min_score):
    """Position of the winner in the candidate list, or -1.

    scores[c] = (score_prefix, score_suffix) and geometry[c] = (prefix_begin, prefix_end, suffix_begin, suffix_end) of
    candidate c, as detect() computes them for the read with that candidate.  A candidate is eligible when
    prefix_begin < suffix_end and min(score_prefix, score_suffix) >= min_score; the eligible candidate with the largest
    minimum wins, the lowest position on a tie.  min_score must be above 0, so that an eligible candidate always passes
    the gate of STRique.py:603."""
    if not min_score > 0:
        raise ValueError("scan: min_score must be above 0")
    if len(scores) != len(geometry):
        raise ValueError("scan: one geometry per candidate")
    winner, best = -1, 0.0
    for c, (sc, geo) in enumerate(zip(scores, geometry)):
        if not eligible(sc, geo, min_score):
            continue
        k = key(sc[0], sc[1])
        if winner < 0 or k > best:
            winner, best = c, k
    return winner


SCORES_HEADER = ['ID', 'winner_target', 'winner_strand']


def scores_header(candidates):
    """Header of the `count --scan-scores` file: two columns per candidate, named after it."""
    cols = list(SCORES_HEADER)
    for name, strand in candidates:
        cols += ["%s%s:score_prefix" % (name, strand), "%s%s:score_suffix" % (name, strand)]
    return cols


def format_scores(read_id, winner, scores):
    """One row of the `count --scan-scores` file.  winner: (target, strand) or None; scores: (score_prefix, score_suffix) per candidate."""
    cols = [str(read_id)] + ([winner[0], winner[1]] if winner else ['-', '-'])
    for sp, ss in scores:
        cols += [repr(float(sp)), repr(float(ss))]
    return '\t'.join(cols)


def parse_scores(stream):
    """(candidates, rows) of a `count --scan-scores` file: candidates = [(target, strand)], rows = [(ID, winner or None,
    [(score_prefix, score_suffix)] per candidate)] in file order."""
    candidates, rows = None, []
    for line in stream:
        f = line.rstrip('\n').split('\t')
        if not line.strip():
            continue
        if candidates is None:
            if f[:3] != SCORES_HEADER or (len(f) - 3) % 2:
                raise ValueError("not a --scan-scores file")
            candidates = [(c[:-len(":score_prefix")][:-1], c[:-len(":score_prefix")][-1]) for c in f[3::2]]
            continue
        if len(f) != 3 + 2 * len(candidates):
            raise ValueError("scores row of %s: %d columns" % (f[0], len(f)))
        vals = [float(x) for x in f[3:]]
        rows.append((f[0], None if f[1] == '-' else (f[1], f[2]), list(zip(vals[0::2], vals[1::2]))))
    return candidates or [], rows
