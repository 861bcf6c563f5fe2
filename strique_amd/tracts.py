"""The rule of tract counting (`hmm.CompoundRepeatModel`, strq_model_set_tracts / strq_viterbi_tracts): what a compound
definition of a repeat locus is, how it reads on the other strand, what a tract's count is, and the two files that go with it
(the definitions, and one row of counts per read).  Pure Python, no device: stated once here, the model builder and the tests
take it from this module.

`count` models a locus as prefix | one unit x n | suffix.  A compound locus is a fixed sequence of K = 2 or 3 tracts, each a
unit of its own repeated n_j times, with K - 1 linkers (possibly empty) between them:

    prefix | U_0 x n_0 | L_0 | U_1 x n_1 [| L_1 | U_2 x n_2] | suffix         HTT: (CAG)n CAACAG (CCG)m

All sequences are given on the + strand, like `repeat`.  The model has one repeat loop per tract; with k the pore model's
k-mer length and u_j = ceil(k / len(U_j)), the profile in front of loop j ends with u_j units of U_j less one base and the
profile behind it starts with u_j units -- exactly the flanks of the one-unit model -- so

    count_j = visits_j + bias_j,    bias_j = 2 u_j - 1 - repeat_offset_j

where visits_j is the number of emissions of the two dummy states of loop j on the best path and repeat_offset_j the whole
extra units the padded unit profile holds (hmm.extend_repeat).  Every loop is passed at least once, so a tract shorter than
bias_j + 1 units cannot be represented (`min_units`): such a read decodes as one that has bias_j + 1.
"""
import math

MIN_TRACTS, MAX_TRACTS = 2, 3

_COMPLEMENT = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}


def _revcomp(s):
    return "".join(_COMPLEMENT[b] for b in reversed(s))


def check(units, linkers):
    """(units, linkers) upper-cased, as tuples.  ValueError for: K outside 2..3, a number of linkers other than K - 1, letters
    beyond ACGT, an empty unit, two adjacent equal units with an empty linker between them (one tract, not two)."""
    if isinstance(units, str) or isinstance(linkers, str):
        raise ValueError("tracts: units and linkers are sequences of strings")
    units = tuple(str(u).upper() for u in units)
    linkers = tuple(str(l).upper() for l in linkers)
    if not MIN_TRACTS <= len(units) <= MAX_TRACTS:
        raise ValueError("tracts: between %d and %d units per target, got %d" % (MIN_TRACTS, MAX_TRACTS, len(units)))
    if len(linkers) != len(units) - 1:
        raise ValueError("tracts: %d units need %d linkers, got %d" % (len(units), len(units) - 1, len(linkers)))
    for u in units:
        if not u:
            raise ValueError("tracts: an empty unit")
        if set(u) - set("ACGT"):
            raise ValueError("tracts: unit %r: only the letters A, C, G, T" % u)
    for l in linkers:
        if set(l) - set("ACGT"):
            raise ValueError("tracts: linker %r: only the letters A, C, G, T" % l)
    for j, l in enumerate(linkers):
        if not l and units[j] == units[j + 1]:
            raise ValueError("tracts: units %d and %d are both %s with nothing between them: that is one tract" % (j, j + 1, units[j]))
    return units, linkers


def strand_definition(units, linkers, strand):
    """The definition as the signal of `strand` reads it: on '-' the reverse complements in reverse order (prefix and suffix
    swap the same way, repeatCounter._classifier).  Tract j of the '-' model is tract K - 1 - j as configured: `configured_order`."""
    units, linkers = check(units, linkers)
    if strand == '+':
        return units, linkers
    if strand == '-':
        return tuple(_revcomp(u) for u in reversed(units)), tuple(_revcomp(l) for l in reversed(linkers))
    raise ValueError("tracts: strand must be + or -")


def configured_order(values, strand):
    """Per-tract values in model order of `strand` -> in the order the definition was configured in."""
    return tuple(values) if strand == '+' else tuple(reversed(tuple(values)))


def flank_units(unit, kmer):
    """u: whole units of `unit` a flanking profile holds."""
    return int(math.ceil(kmer / len(unit)))


def repeat_offset(unit, kmer):
    """Whole extra units in the padded unit profile of a loop (hmm.extend_repeat restated: the rule is stated here once more so
    that this module stands alone)."""
    if len(unit) >= kmer:
        return 0
    ext = kmer - 1 + (len(unit) - 1) - ((kmer - 1) % len(unit))
    return int((len(unit) + ext) / len(unit)) - 1


def bias(unit, kmer):
    return 2 * flank_units(unit, kmer) - 1 - repeat_offset(unit, kmer)


def min_units(unit, kmer):
    """The shortest tract of `unit` the model can represent."""
    return bias(unit, kmer) + 1


def sections(units, linkers, prefix, suffix, kmer):
    """The profile sequences and loop units of the model, in order: [('profile', name, sequence) | ('loop', name, unit)]."""
    units, linkers = check(units, linkers)
    K = len(units)
    u = [flank_units(x, kmer) for x in units]
    out = [('profile', 'prefix', prefix + (units[0] * u[0])[:-1])]
    for j in range(K):
        out.append(('loop', 'tract%d' % j, units[j]))
        if j < K - 1:
            out.append(('profile', 'junction%d' % j, units[j] * u[j] + linkers[j] + (units[j + 1] * u[j + 1])[:-1]))
    out.append(('profile', 'suffix', units[K - 1] * u[K - 1] + suffix))
    return out


# ---- the definition file (`count --tract-units`) ---------------------------------------------------------------------------------
def parse_definitions(stream, targets=None):
    """{target: (units, linkers)} of a definition file: one line per target, `target<TAB>U0,U1[,U2][<TAB>L0[,L1]]`; `-` or a
    missing third column means empty linkers, a single `-` inside the list one empty linker.  Lines that start with # and blank
    lines are skipped.  ValueError for a malformed line, a duplicate, a target not in `targets` (when given) and anything
    `check` rejects."""
    out = {}
    for no, line in enumerate(stream, 1):
        text = line.rstrip('\r\n')
        if not text.strip() or text.lstrip().startswith('#'):
            continue
        f = text.split('\t')
        if len(f) not in (2, 3) or not f[0].strip():
            raise ValueError("tract definitions, line %d: expected target<TAB>units[<TAB>linkers]" % no)
        name = f[0].strip()
        if name in out:
            raise ValueError("tract definitions, line %d: target %s is defined twice" % (no, name))
        if targets is not None and name not in targets:
            raise ValueError("tract definitions, line %d: unknown target %s" % (no, name))
        units = [u.strip() for u in f[1].split(',')]
        col = f[2].strip() if len(f) == 3 else '-'
        if col in ('-', ''):
            linkers = [''] * (len(units) - 1)
        else:
            linkers = ['' if l.strip() == '-' else l.strip() for l in col.split(',')]
        try:
            out[name] = check(units, linkers)
        except ValueError as e:
            raise ValueError("tract definitions, line %d (%s): %s" % (no, name, e))
    return out


# ---- the side file (one row per count row) ---------------------------------------------------------------------------------------
HEADER = ['ID', 'target', 'strand', 'count', 'n_tracts', 'tract_counts', 'tract_log_p']


def format_row(read_id, target, strand, count, rec):
    """One row.  count: the count of the count row; rec: None (not decoded, or a target without tracts) or (counts in configured
    order, log_p).  Counts joined by commas, log_p written with repr, '-' for a field without a value."""
    head = [str(read_id), str(target), str(strand), str(int(count))]
    if rec is None:
        return '\t'.join(head + ['-', '-', '-'])
    counts, log_p = rec
    return '\t'.join(head + [str(len(counts)), ','.join(str(int(c)) for c in counts), repr(float(log_p))])


def parse(stream):
    """Rows of the side file: [(ID, target, strand, count, None or (counts tuple, log_p))]."""
    rows, seen_header = [], False
    for line in stream:
        if not line.strip():
            continue
        f = line.rstrip('\n').split('\t')
        if not seen_header:
            if f != HEADER:
                raise ValueError("not a --tracts file")
            seen_header = True
            continue
        if len(f) != len(HEADER):
            raise ValueError("tracts row of %s: %r" % (f[0], f[1:]))
        if f[4] == '-':
            if f[5] != '-' or f[6] != '-':
                raise ValueError("tracts row of %s: %r" % (f[0], f[1:]))
            rec = None
        else:
            counts = tuple(int(c) for c in f[5].split(','))
            if len(counts) != int(f[4]):
                raise ValueError("tracts row of %s: %d counts, n_tracts = %s" % (f[0], len(counts), f[4]))
            rec = (counts, float(f[6]))
        rows.append((f[0], f[1], f[2], int(f[3]), rec))
    return rows


# ---- where the units of a tract lie (`count --tract-positions`) ------------------------------------------------------------------
# The rule.  A read gets positions exactly when its tract record has status 0.  With the window [prefix_begin, suffix_end) of the
# filtered signal under the read's conditioning record -- the window of the tract decode -- position prefix_begin + t belongs to tract
# j when the best path of the compound model emits observation t from one of the two dummy states of loop j.  Per tract the positions
# ascend and there are count_j - bias_j of them: the visits, no bias applied (the bias units sit in the neighbouring profiles and have
# no position).  Tracts come back in configured order on both strands (`configured_order`: on '-' the tract that is first in the
# signal is configured last).  The span of a tract is (first position, last position).
POS_HEADER = ['ID', 'target', 'strand', 'count', 'n_tracts', 'tract_counts', 'tract_spans', 'tract_positions']


def spans(positions):
    """(first, last) per tract, None for a tract without positions."""
    return tuple((int(p[0]), int(p[-1])) if len(p) else None for p in positions)


def format_positions_row(read_id, target, strand, count, rec):
    """One row.  rec: None (no tract record) or (counts, log_p, positions) in configured order, positions None (back-pointers over
    the budget) or one ascending sequence per tract.  Spans `first-last` per tract joined by commas; positions joined by commas
    within a tract and ';' between tracts; '-' for a field without a value and for a tract without positions."""
    head = [str(read_id), str(target), str(strand), str(int(count))]
    if rec is None:
        return '\t'.join(head + ['-', '-', '-', '-'])
    counts, positions = rec[0], rec[2]
    fields = [str(len(counts)), ','.join(str(int(c)) for c in counts)]
    if positions is None:
        return '\t'.join(head + fields + ['-', '-'])
    if len(positions) != len(counts):
        raise ValueError("tract positions of %s: %d tracts, %d position lists" % (read_id, len(counts), len(positions)))
    fields.append(','.join('-' if s is None else '%d-%d' % s for s in spans(positions)))
    fields.append(';'.join(','.join(str(int(x)) for x in p) if len(p) else '-' for p in positions))
    return '\t'.join(head + fields)


def parse_positions(stream):
    """Rows of the positions file: [(ID, target, strand, count, None or (counts tuple, spans or None, positions or None))] -- spans a
    tuple of (first, last) or None per tract, positions a tuple of tuples of int."""
    rows, seen_header = [], False
    for line in stream:
        if not line.strip():
            continue
        f = line.rstrip('\n').split('\t')
        if not seen_header:
            if f != POS_HEADER:
                raise ValueError("not a --tract-positions file")
            seen_header = True
            continue
        if len(f) != len(POS_HEADER):
            raise ValueError("tract positions row of %s: %r" % (f[0], f[1:]))
        if f[4] == '-':
            if f[5:] != ['-', '-', '-']:
                raise ValueError("tract positions row of %s: %r" % (f[0], f[1:]))
            rec = None
        else:
            counts = tuple(int(c) for c in f[5].split(','))
            if len(counts) != int(f[4]):
                raise ValueError("tract positions row of %s: %d counts, n_tracts = %s" % (f[0], len(counts), f[4]))
            if f[6] == '-' and f[7] == '-':
                rec = (counts, None, None)
            else:
                sp = tuple(None if s == '-' else tuple(int(v) for v in s.split('-')) for s in f[6].split(','))
                pos = tuple(() if p == '-' else tuple(int(v) for v in p.split(',')) for p in f[7].split(';'))
                if len(sp) != len(counts) or len(pos) != len(counts) or spans(pos) != sp:
                    raise ValueError("tract positions row of %s: spans and positions disagree" % f[0])
                rec = (counts, sp, pos)
        rows.append((f[0], f[1], f[2], int(f[3]), rec))
    return rows
