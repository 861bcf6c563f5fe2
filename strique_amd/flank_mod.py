"""The rule of the flank methylation calls: mCpG log-likelihood ratios for the CpG sites of the configured flanks.  Pure Python, no
device: the GPU applies the bounds part of it in flank_mod_bounds_kernel (strique_amd/csrc/flank_mod_kernels.hip), and the tests
compare the two.

Everything here is in the coordinates of the flank AS THE STRAND READS IT -- what add_target hands the classifier of that strand
after its +/- swap and reverse complement; `configured()` maps back to the configured (+ strand) flank.  k = pm.kmer,
L = len(flank), n = L - k + 1 profile columns.

  sites    every c with flank[c:c+2] == "CG"
  groups   consecutive sites with c2 - c1 <= k - 2 share a k-mer and form one group; the mCpG table assumes every CpG of a k-mer
           methylated, so a group is called as a whole.  Its columns are [c_first - k + 2, c_last] clipped to [0, n): the k-mers
           that hold a whole CG of the group
  stretch  the raw samples the alignment of the WHOLE configured flank covers: from the sample flank row 0 of the alignment sits on to
           the sample its last row sits on (`__detect_range__`, scripts/STRique.py:538-548, without pre_trim / post_trim).  The
           prefix flank is scored on [whole prefix begin, prefix_end), the suffix flank on [suffix_begin, whole suffix end).  The
           row's prefix_begin and suffix_end are NOT these ends: they are taken `trim` rows further in (STRique.py:598-599) and bound
           the inner 50 nt of a 150-nt flank.  The pipeline keeps both (finalize_kernel; strq_batch_fetch_flank_ranges hands the
           whole ones out).  The samples are normalised from the raw signal and clipped as the modification pass takes its stretch.
           A read qualifies when its gate passed, it could be conditioned and its target has a modification model; a flank of it
           is called where begin < end.  A stretch of more than 64 L observations is not decoded (`too_long`)
  segmentation
           one Viterbi decode of the stretch with hmm.FlankProfileModel; `first` / `last` are the first and the last observation
           the best path emits from a match or insert state of the group's columns
  scores   u = first - 1, w = last + 1; V_base, V_mod are the Viterbi log-probabilities of hmm.SiteModModel over the group's
           columns on x[u .. w] with the other branch removed (as mod_llr_kernels.h evaluates them); llr = V_mod - V_base
"""
from collections import namedtuple

MAX_GROUP_COLUMNS = 31        # LLR_MAX_EMIT = 128 = 2 hubs + 4 * 31 (mod_llr_kernels.h)
MAX_GROUPS = 64               # one lane of flank_mod_bounds_kernel per group
MAX_STRETCH = 64              # observations per flank base beyond which a stretch is not decoded

SCORED, NO_PATH, EDGE, SKIPPED, TOO_LONG = 0, 1, 2, 3, 4
STATUS_NAMES = ('scored', 'no_path', 'edge', 'skipped', 'too_long')

PREFIX, SUFFIX = 0, 1
FLANK_LETTERS = ('p', 's')

class Group(namedtuple("Group", "sites c0 c1")):
    """One CpG group: its sites ascending, its profile columns c0 .. c1 inclusive."""
    __slots__ = ()

    @property
    def n_columns(self):
        return self.c1 - self.c0 + 1

    @property
    def n_sites(self):
        return len(self.sites)


def sites(flank):
    flank = flank.upper()
    return [c for c in range(len(flank) - 1) if flank[c:c + 2] == "CG"]


def groups(flank, k):
    """The groups of a flank in ascending order (no limits applied: see check)."""
    n = len(flank) - k + 1
    if n < 1:
        raise ValueError("flank-mod: a flank of %d nt has no %d-mer" % (len(flank), k))
    runs = []
    for c in sites(flank):
        if runs and c - runs[-1][-1] <= k - 2:
            runs[-1].append(c)
        else:
            runs.append([c])
    return [Group(tuple(r), max(0, r[0] - k + 2), min(n - 1, r[-1])) for r in runs]


def check(flank, k, what="flank"):
    """groups(flank, k), or ValueError with the message of the refusal: a group beyond MAX_GROUP_COLUMNS columns, more than
    MAX_GROUPS groups."""
    gs = groups(flank, k)
    for g in gs:
        if g.n_columns > MAX_GROUP_COLUMNS:
            raise ValueError("flank-mod: the CpG group at %d of the %s spans %d profile columns, at most %d are scored (a dual model of "
                             "128 emitting states)" % (g.sites[0], what, g.n_columns, MAX_GROUP_COLUMNS))
    if len(gs) > MAX_GROUPS:
        raise ValueError("flank-mod: the %s holds %d CpG groups, at most %d are called" % (what, len(gs), MAX_GROUPS))
    return gs


def site_sequence(flank, group, k):
    """The bases the columns of a group spell: the sequence of its hmm.SiteModModel."""
    return flank[group.c0:group.c1 + k]


def configured(which, group, flank_len, strand):
    """(flank, pos) of a group of the strand's flank `which` (PREFIX / SUFFIX) in the configured (+ strand) flanks: CG is its own
    reverse complement, so a site at c of the - strand is the configured flank's C at L - 2 - c, and the - strand's prefix is the
    configured suffix.  pos is the group's first C in the configured string."""
    if strand == '+':
        return which, group.sites[0]
    if strand != '-':
        raise ValueError("strand must be + or -")
    return 1 - which, flank_len - 2 - group.sites[-1]


def too_long(T, flank_len):
    return T > MAX_STRETCH * flank_len


def bounds(path, column_of, ranges):
    """[(status, u, w)] per (c0, c1) of `ranges`, from the emitting-state path of the segmentation decode (None: no path) and the
    model's column_of: SCORED with u = first - 1, w = last + 1; EDGE when `first` is the stretch's first observation or `last` its
    last, so that a hub has nothing to emit; SKIPPED when the path emits nothing from the columns.  u = w = -1 unless SCORED."""
    if path is None:
        return [(NO_PATH, -1, -1)] * len(ranges)
    T = len(path)
    cols = [int(column_of[int(s)]) for s in path]
    out = []
    for c0, c1 in ranges:
        hit = [t for t, c in enumerate(cols) if c0 <= c <= c1]
        if not hit:
            out.append((SKIPPED, -1, -1))
        elif hit[0] == 0 or hit[-1] == T - 1:
            out.append((EDGE, -1, -1))
        else:
            out.append((SCORED, hit[0] - 1, hit[-1] + 1))
    return out


# ---- the side file -----------------------------------------------------------------------------------------------------------------
HEADER = ['ID', 'target', 'strand', 'count', 'n_groups', 'calls']


def format_row(read_id, target, strand, count, calls):
    """One row.  calls: None (the read has no flank calls) or [(flank, pos, n_sites, llr)] -- flank PREFIX / SUFFIX as configured, llr
    None or NaN for a group without a score."""
    if not calls:
        return '\t'.join([str(read_id), str(target), str(strand), str(count), '0', '-'])
    f = []
    for flank, pos, n_sites, llr in calls:
        scored = llr is not None and llr == llr
        f.append('%s:%d:%d:%s' % (FLANK_LETTERS[int(flank)], int(pos), int(n_sites), ('%.4f' % float(llr)) if scored else '-'))
    return '\t'.join([str(read_id), str(target), str(strand), str(count), str(len(calls)), ','.join(f)])


def parse(stream):
    """Rows of the side file: [(ID, target, strand, count, [(flank, pos, n_sites, llr or None)])] in file order."""
    rows, seen_header = [], False
    for line in stream:
        if not line.strip():
            continue
        f = line.rstrip('\n').split('\t')
        if not seen_header:
            if f != HEADER:
                raise ValueError("not a --flank-mod file")
            seen_header = True
            continue
        if len(f) != len(HEADER):
            raise ValueError("flank-mod row of %s: %r" % (f[0], f[1:]))
        calls = []
        if f[5] != '-':
            for item in f[5].split(','):
                p = item.split(':')
                if len(p) != 4 or p[0] not in FLANK_LETTERS:
                    raise ValueError("flank-mod row of %s: call %r" % (f[0], item))
                calls.append((FLANK_LETTERS.index(p[0]), int(p[1]), int(p[2]), None if p[3] == '-' else float(p[3])))
        if len(calls) != int(f[4]):
            raise ValueError("flank-mod row of %s: %d calls, n_groups = %s" % (f[0], len(calls), f[4]))
        rows.append((f[0], f[1], f[2], f[3], calls))
    return rows
