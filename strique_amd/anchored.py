"""The rule of anchored counting (`repeatCounter.detect(..., anchored=m)`, `count --anchored`, strq_set_anchored): which reads
hold one flank only, and which stretch of them is decoded with which model.  Pure Python, no device: the GPU applies the same
rule in anchored_classify_kernel (strique_amd/csrc/anchored_kernels.hip), and the tests compare the two.

A read that breaks off inside the repeat, or starts inside it, has one flank.  The other flank alignment of detect()
(scripts/STRique.py:598-601) lands somewhere at a low normalised score, the gate of STRique.py:602 opens all the same and the
flanked HMM is decoded between two positions of which one means nothing.  Here such a read is decoded from its one flank to
its end (or from its start to its one flank) with a model whose missing flank profile is a single free state
(hmm.AnchoredRepeatModel); the count is a lower bound on the allele up to the decode's own error.
"""

# There is no default for the threshold `m`: like the scan's min_score (strique_amd/scan.py) it separates the score of a flank
# that is there from one that is not, and those overlap on noisy reads, so the caller names it.

NONE, SPANNING, ENDS_IN_REPEAT, STARTS_IN_REPEAT = 0, 1, 2, 3
KIND_NAMES = ('none', 'spanning', 'ends_in_repeat', 'starts_in_repeat')


def classify(status, n, score_prefix, score_suffix, prefix_begin, suffix_end, m):
    """(kind, window begin, window end) of one read.

    status, n: the read's conditioning status (0 = it could be normalised) and its length in samples; the scores and positions
    are the ones detect() reports for the strand-specific classifier.  The kinds name what the signal does, so they need no
    strand to be read.  Comparisons with a NaN are false: a NaN score is neither above nor below `m`, the read is `none`."""
    if not m > 0:
        raise ValueError("anchored: the score threshold must be above 0")
    if status != 0 or n <= 0:
        return NONE, 0, 0
    if score_prefix >= m and score_suffix >= m:
        return (SPANNING, prefix_begin, suffix_end) if prefix_begin < suffix_end else (NONE, 0, 0)
    # (the positions of an alignment are samples of the read; a window that would not lie inside it is never decoded)
    if score_prefix >= m and score_suffix < m:
        return (ENDS_IN_REPEAT, prefix_begin, n) if 0 <= prefix_begin < n else (NONE, 0, 0)
    if score_suffix >= m and score_prefix < m:
        return (STARTS_IN_REPEAT, 0, suffix_end) if 0 < suffix_end <= n else (NONE, 0, 0)
    return NONE, 0, 0


def free_samples(kind, T, first_tagged, last_tagged):
    """Observations the free state emitted, from the bounds of the stretch of the window (T observations) that was decoded into
    repeat states: behind it for a read that ends in the repeat, in front of it for one that starts there."""
    if kind == ENDS_IN_REPEAT:
        return T - 1 - last_tagged
    if kind == STARTS_IN_REPEAT:
        return first_tagged
    raise ValueError("anchored: no free state for kind %r" % (kind,))


HEADER = ['ID', 'target', 'strand', 'kind', 'count', 'log_p', 'begin', 'end', 'free_samples']


def format_row(read_id, target, strand, rec):
    """One row of the `count --anchored` file.  rec: None (the rule was not applied: no count row's worth of a read), or
    (kind, status, count, log_p, begin, end, free_samples); '-' where there is no decode."""
    if rec is None:
        return '\t'.join([str(read_id), str(target), str(strand), KIND_NAMES[NONE]] + ['-'] * 5)
    kind, status, count, log_p, begin, end, free = rec
    if kind in (ENDS_IN_REPEAT, STARTS_IN_REPEAT) and status == 0:
        vals = [str(int(count)), repr(float(log_p)), str(int(begin)), str(int(end)), str(int(free))]
    else:
        vals = ['-'] * 5
    return '\t'.join([str(read_id), str(target), str(strand), KIND_NAMES[int(kind)]] + vals)


def parse(stream):
    """Rows of a `count --anchored` file: [(ID, target, strand, kind name, None or (count, log_p, begin, end, free_samples))]."""
    rows, seen_header = [], False
    for line in stream:
        if not line.strip():
            continue
        f = line.rstrip('\n').split('\t')
        if not seen_header:
            if f != HEADER:
                raise ValueError("not a --anchored file")
            seen_header = True
            continue
        if len(f) != len(HEADER) or f[3] not in KIND_NAMES:
            raise ValueError("anchored row of %s: %r" % (f[0], f[1:]))
        dec = None if f[4] == '-' else (int(f[4]), float(f[5]), int(f[6]), int(f[7]), int(f[8]))
        rows.append((f[0], f[1], f[2], f[3], dec))
    return rows


# ---- methylation calls of anchored reads (`count --anchored-mod`, strq_set_anchored_mod) -----------------------------------------
# With --mod_model the reference (and the count row) call mCpG on spanning reads only (scripts/STRique.py:605-609).  A read gets an
# anchored methylation call when
#   * its anchored record has kind 2 or 3 and status 0,
#   * begin < end (which status 0 implies), and
#   * its target has a modification model;
# with nrm = normalize2model(raw, 'minmax') of the RAW signal, as the modification pass of a spanning read takes it, the call is
#   pattern = mod_repeats(mod_model, mod_range, nrm[begin:end])     one character per unit the best path of the dual model passes,
#                                                                   '-' when that decode has no path,
# and with the per-unit switch on (V_base(j), V_mod(j)) per character, defined on this stretch exactly as README "Methylation
# calls: per-unit log-likelihood ratio" defines them on the stretch of a spanning read.  Spanning reads (their row has the pattern),
# kinds 0 / 1, records of status 1 / 2 and targets without a modification model get nothing.  len(pattern) is not tied to the
# record's count: the reference ties the two for spanning reads no more than this does.

def gets_mod_call(rec, has_mod_model):
    """The rule above on one record (kind, status, count, log_p, begin, end, free_samples), or None."""
    if rec is None or not has_mod_model:
        return False
    kind, status, _, _, begin, end, _ = rec
    return kind in (ENDS_IN_REPEAT, STARTS_IN_REPEAT) and status == 0 and begin < end


MOD_HEADER = ['ID', 'target', 'strand', 'kind', 'count', 'mod_pattern', 'n_units', 'llr']


def format_mod_row(read_id, target, strand, rec, call):
    """One row of the `count --anchored-mod` file.  rec: the anchored record or None, as format_row takes it; call: None, or
    (pattern, ratios) -- ratios: None (no --mod-llr, or no units) or V_mod - V_base per character of the pattern, written with four
    decimals and joined by commas.  '-' for every field without a value."""
    kind = KIND_NAMES[NONE] if rec is None else KIND_NAMES[int(rec[0])]
    count = str(int(rec[2])) if rec is not None and rec[0] in (ENDS_IN_REPEAT, STARTS_IN_REPEAT) and rec[1] == 0 else '-'
    if call is None:
        vals = ['-', '-', '-']
    else:
        pattern, llr = call
        units = 0 if pattern == '-' else len(pattern)
        ratios = [] if llr is None else [float(x) for x in llr]
        if ratios and len(ratios) != units:
            raise ValueError("anchored-mod row of %s: %d ratios for %d units" % (read_id, len(ratios), units))
        vals = [pattern if pattern else '-', str(units), ','.join('%.4f' % x for x in ratios) if ratios else '-']
    return '\t'.join([str(read_id), str(target), str(strand), kind, count] + vals)


def parse_mod(stream):
    """Rows of a `count --anchored-mod` file: [(ID, target, strand, kind name, count or None, None or (pattern, n_units, ratios
    or None))] in file order; a call whose pattern has no units reads back as ('-', 0, None)."""
    rows, seen_header = [], False
    for line in stream:
        if not line.strip():
            continue
        f = line.rstrip('\n').split('\t')
        if not seen_header:
            if f != MOD_HEADER:
                raise ValueError("not a --anchored-mod file")
            seen_header = True
            continue
        if len(f) != len(MOD_HEADER) or f[3] not in KIND_NAMES:
            raise ValueError("anchored-mod row of %s: %r" % (f[0], f[1:]))
        call = None
        if f[6] != '-':
            ratios = None if f[7] == '-' else [float(x) for x in f[7].split(',')]
            if ratios is not None and len(ratios) != int(f[6]):
                raise ValueError("anchored-mod row of %s: %d ratios, n_units = %s" % (f[0], len(ratios), f[6]))
            call = (f[5], int(f[6]), ratios)
        elif f[5] != '-' or f[7] != '-':
            raise ValueError("anchored-mod row of %s: %r" % (f[0], f[1:]))
        rows.append((f[0], f[1], f[2], f[3], None if f[4] == '-' else int(f[4]), call))
    return rows
