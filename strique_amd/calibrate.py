"""Calibration: k-mer levels re-estimated from the state statistics of the best path (segmental / Viterbi re-estimation).

Every match state of the flanked model stands for one k-mer (hmm.FlankedRepeatModel.state_kmers), so the mean of the observations the
best path assigns to it (strique_amd/state_stats.py) estimates that k-mer's level in the model's own domain, on the windows `count`
decodes.  The rule, said once:

    pool      per k-mer, over all reads and all match states that carry it (both strands: a model of the - strand carries the k-mers
              of the reverse-complemented locus, which is what the pore table lists):  N = sum of n,  S and Q = math.fsum of the
              per-(read, state) sums and sums of squares -- exactly rounded, so that the pool does not depend on the order of the
              reads, on batching or on how the device split a batch
    estimate  the new mean of a k-mer is S / N where N >= min_obs, otherwise the table's value stays; the observed standard
              deviation sqrt(max(0, Q / N - mean^2)) is reported and never written into the table
    table     every k-mer of the input table in input order, `kmer<TAB>mean<TAB>stdv` with repr floats: untouched k-mers round-trip
              exactly through pore_model

Limits: means only (no stdv fitting); only the k-mers of the configured loci; the decode clips observations to
[model_min + .5, model_max - .5], which biases levels at the edge of the range; hard assignment -- two neighbouring k-mers with
nearly equal levels share their error.
"""
import math

STATS_HEADER = ['kmer', 'n_reads', 'n_obs', 'mean', 'sd', 'table_mean', 'table_stdv', 'delta', 'updated']


def pool(records):
    """records: per read (state_kmers, n, sum, sumsq) -- state_kmers as hmm.FlankedRepeatModel.state_kmers() gives them (or any
    sequence of (section, kind, kmer)), the three rows of that read's statistics.  Returns {kmer: (n_reads, N, S, Q)} sorted by
    k-mer; a k-mer without a counted observation does not appear."""
    parts = {}
    for what, n, s, q in records:
        if not (len(what) == len(n) == len(s) == len(q)):
            raise ValueError("one statistics entry per emitting state")
        seen = set()
        for (section, kind, kmer), ni, si, qi in zip(what, n, s, q):
            if kmer is None or int(ni) == 0:
                continue
            p = parts.setdefault(kmer, [0, 0, [], []])
            if kmer not in seen:
                seen.add(kmer); p[0] += 1
            p[1] += int(ni); p[2].append(float(si)); p[3].append(float(qi))
    return {k: (parts[k][0], parts[k][1], math.fsum(parts[k][2]), math.fsum(parts[k][3])) for k in sorted(parts)}


def estimate(pooled, pm, min_obs):
    """(new_means, rows): new_means {kmer: mean} of the k-mers with at least min_obs observations, rows one tuple per pooled k-mer
    in STATS_HEADER order (sorted by k-mer)."""
    if min_obs < 1:
        raise ValueError("min_obs must be at least 1")
    new_means, rows = {}, []
    for kmer, (n_reads, N, S, Q) in pooled.items():
        if kmer not in pm.model_dict:
            raise KeyError("k-mer %s is not in the pore model" % kmer)
        t_mean, t_stdv = pm.model_dict[kmer]
        mean = S / N
        sd = math.sqrt(max(0.0, Q / N - mean * mean))
        updated = N >= min_obs
        if updated:
            new_means[kmer] = mean
        rows.append((kmer, n_reads, N, mean, sd, t_mean, t_stdv, mean - t_mean, 1 if updated else 0))
    return new_means, rows


def write_model(path, pm, new_means):
    """The table of `pm` with the means of `new_means` in place: every k-mer in input order, kmer<TAB>mean<TAB>stdv."""
    with open(path, 'w') as fp:
        for kmer, (mean, stdv) in pm.model_dict.items():
            fp.write("%s\t%r\t%r\n" % (kmer, float(new_means.get(kmer, mean)), float(stdv)))


def format_row(row):
    kmer, n_reads, n_obs, mean, sd, t_mean, t_stdv, delta, updated = row
    return "\t".join([kmer, str(int(n_reads)), str(int(n_obs))] + [repr(float(v)) for v in (mean, sd, t_mean, t_stdv, delta)] + [str(int(updated))])


def format(rows):
    """The text of a --stats file: header and one line per row."""
    return "".join(line + "\n" for line in ["\t".join(STATS_HEADER)] + [format_row(r) for r in rows])


def parse(text):
    """Rows of a --stats file as format() wrote them (exact inverse)."""
    lines = text.splitlines()
    if not lines or lines[0].split("\t") != STATS_HEADER:
        raise ValueError("not a calibrate --stats file")
    rows = []
    for line in lines[1:]:
        c = line.split("\t")
        if len(c) != len(STATS_HEADER):
            raise ValueError("bad --stats row: %r" % line)
        rows.append((c[0], int(c[1]), int(c[2]), float(c[3]), float(c[4]), float(c[5]), float(c[6]), float(c[7]), int(c[8])))
    return rows
