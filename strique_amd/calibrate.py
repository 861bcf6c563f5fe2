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

Soft assignment (`calibrate --posterior`): the same estimator over the state posteriors (strique_amd/state_posteriors.py) -- the EM
(Baum-Welch) step where the rule above is segmental k-means.  Every observation is shared among the states in proportion to the
posterior probability that the state emitted it:

    pool_posterior  per k-mer  W = math.fsum of w,  S and Q = math.fsum of wx and wxx over the per-(read, state) rows of the states
                    that carry it; a read counts in n_reads where that k-mer's states together hold at least one expected
                    observation (sum of w >= 1)
    estimate        unchanged, on the float W: the new mean is S / W where W >= min_obs
    --stats         the third column is `exp_obs` (a repr float) instead of `n_obs`
"""
import math

STATS_HEADER = ['kmer', 'n_reads', 'n_obs', 'mean', 'sd', 'table_mean', 'table_stdv', 'delta', 'updated']
STATS_HEADER_POSTERIOR = STATS_HEADER[:2] + ['exp_obs'] + STATS_HEADER[3:]


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


def pool_posterior(records):
    """records: per read (state_kmers, w, wx, wxx) -- the three rows of that read's state posteriors (the soft counterpart of pool's
    records).  Returns {kmer: (n_reads, W, S, Q)} sorted by k-mer, W, S, Q the math.fsum over the per-(read, state) rows of the states
    that carry the k-mer: exactly rounded, so independent of the order of the reads.  n_reads: the reads in which those states
    together hold at least one expected observation.  A k-mer whose W is 0 does not appear."""
    parts = {}
    for what, w, wx, wxx in records:
        if not (len(what) == len(w) == len(wx) == len(wxx)):
            raise ValueError("one statistics entry per emitting state")
        mine = {}
        for (section, kind, kmer), wi, si, qi in zip(what, w, wx, wxx):
            if kmer is None:
                continue
            p = parts.setdefault(kmer, [0, [], [], []])
            p[1].append(float(wi)); p[2].append(float(si)); p[3].append(float(qi))
            mine.setdefault(kmer, []).append(float(wi))
        for kmer, ws in mine.items():
            if math.fsum(ws) >= 1.0:
                parts[kmer][0] += 1
    out = {}
    for k in sorted(parts):
        W = math.fsum(parts[k][1])
        if W > 0.0:
            out[k] = (parts[k][0], W, math.fsum(parts[k][2]), math.fsum(parts[k][3]))
    return out


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


def format_row(row, posterior=False):
    kmer, n_reads, n_obs, mean, sd, t_mean, t_stdv, delta, updated = row
    obs = repr(float(n_obs)) if posterior else str(int(n_obs))
    return "\t".join([kmer, str(int(n_reads)), obs] + [repr(float(v)) for v in (mean, sd, t_mean, t_stdv, delta)] + [str(int(updated))])


def format(rows, posterior=False):
    """The text of a --stats file: header and one line per row.  posterior: the third column is the expected number of observations,
    a repr float under the header `exp_obs`."""
    header = STATS_HEADER_POSTERIOR if posterior else STATS_HEADER
    return "".join(line + "\n" for line in ["\t".join(header)] + [format_row(r, posterior) for r in rows])


def parse(text):
    """Rows of a --stats file as format() wrote them, either header (exact inverse: the third column is an int under `n_obs`, a
    float under `exp_obs`)."""
    lines = text.splitlines()
    if not lines or lines[0].split("\t") not in (STATS_HEADER, STATS_HEADER_POSTERIOR):
        raise ValueError("not a calibrate --stats file")
    obs = float if lines[0].split("\t") == STATS_HEADER_POSTERIOR else int
    rows = []
    for line in lines[1:]:
        c = line.split("\t")
        if len(c) != len(STATS_HEADER):
            raise ValueError("bad --stats row: %r" % line)
        rows.append((c[0], int(c[1]), obs(c[2]), float(c[3]), float(c[4]), float(c[5]), float(c[6]), float(c[7]), int(c[8])))
    return rows
