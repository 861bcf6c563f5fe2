"""Case lists of tests/test_gpu_conditioning.py, and a plain restatement of which path of strique_amd/csrc/cond_kernels.hip a
read takes.  No GPU, no library: tests/test_cond_cases_host.py counts the classes these lists reach, so that a change of the
lists (or of the kernels' tiling) that stops reaching one of them fails on the host.

A batch is a list of reads that goes to the device in one call.  The reads of a batch sit back to back in one buffer, so the
alignment phase `a0` of a read (samples between the 16-byte boundary in front of it and its first sample) is fixed by the summed
lengths of the reads in front of it -- and by the residue of the buffer's base, which the lists do not assume: every edge length
occurs behind prefixes of every residue 0..7.

Tags of a case:
  degenerate   MAD = 0 or no order statistics at all: the levels are undefined and are not compared.  These are the constant
               reads, the read with a NaN, the empty reads -- and the reads of one and two samples, whose median-filtered
               signal is constant whatever the samples are (med(0, a, 0) = 0; med(0, a, b) = med(a, b, 0)).
  empty_tails  MAD > 0, but no level lies strictly below the 1st / above the 99th percentile of the 8-bit signal: the reference's
               medians of nothing are NaN and so is every level value.  Levels are compared; values compare equal as NaN.
"""
import warnings
from collections import namedtuple

import numpy as np

# The five numbers of strique_amd/csrc/cond_kernels.hip this module restates (its #defines of the same names):
COND_TILE = 2048          # samples of one quant_morph_kernel workgroup
COND_HALO = 16            # context on each side of such a tile
HIST_TILE = 16384         # samples of one medfilt_hist16(_vec)_kernel / hist16_kernel workgroup
HIST_WIN = 4096           # values of the LDS histogram window, anchored at the tile minimum
HSTAT_LDS_BINS = 14336    # widest occupied bin range hist_stats_kernel stages in LDS

Case = namedtuple("Case", "name signal tags")
Batch = namedtuple("Batch", "name dtype cases sub")          # sub: STRQ_SUBBATCH_READS of the run (0: the whole batch is one sub-batch)

TINY = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31)
SEAMS = tuple(COND_TILE * k + d for k in (1, 2, 3) for d in (-17, -16, -15, -1, 0, 1, 15, 16, 17))
# the smallest read with an interior tile has 2 * COND_TILE + COND_HALO - a0 samples: 4105 (a0 = 7) ... 4112 (a0 = 0)
FIRST_INTERIOR = tuple(range(2 * COND_TILE + COND_HALO - 8, 2 * COND_TILE + COND_HALO + 1))
LAST_TILE = tuple(COND_TILE + d for d in range(1, 17))          # a last tile of 1..16 samples (+ a0)
HIST_SEAMS = (16383, 16384, 16385, 16391, 16392, 32768, 32769)
LONG_READ = 300007
# The last stage of the closing is an 8-wide erosion, so the lowest level of the 8-bit signal holds eight samples or more (five at a
# reflecting border): in a read this short that is more than one percent, the 1st percentile IS the lowest level and nothing lies
# strictly below it -- such reads have empty tails whatever their samples are.
MIN_TAILS = 400


def steps(rng, n, lo=350.0, hi=650.0, noise=6.0, dwell=9):
    """A nanopore-like signal: levels held for a few samples each (at least three), plus noise.  Reads of more than
    MIN_TAILS samples also hold one ten-sample level below and one above all others: wide enough to survive the 1 x 8 opening and
    closing, short enough to lie beyond the 1st / 99th percentile, so that both tails of the 8-bit signal are occupied."""
    nseg = n // 3 + 2
    d = rng.geometric(1.0 / dwell, nseg) + 2
    x = np.repeat(rng.uniform(lo, hi, nseg), d)[:n]
    if n > MIN_TAILS:
        a, b = rng.choice(np.arange(20, n - 30, 16), 2, replace=False)
        x[a:a + 10] = lo - 0.15 * (hi - lo); x[b:b + 10] = hi + 0.15 * (hi - lo)
    return x + rng.normal(0.0, noise, n)


def as_i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _tags(n, *more):
    return frozenset(more) | (frozenset(["degenerate"]) if n <= 2 else frozenset()) | (frozenset(["empty_tails"]) if 3 <= n <= MIN_TAILS else frozenset())


def spiked(x):
    """First and last sample far above the rest: the zero pad of medfilt makes the filter drop them (med(0, spike, x1) = x1),
    a neighbouring read's spike in the pad's place would not be dropped (med(spike', spike, x1) = min of the spikes)."""
    if len(x) >= 2:
        x = x.copy()
        x[0] = 30000 + (int(abs(x[1])) % 2000)
        x[-1] = 29000 + (int(abs(x[-2])) % 2000)
    return x


def edge_block(rng, dtype, lengths, at, residue, tag):
    """Reads of `lengths` behind one filler read, which makes the number of samples in front of them `residue` mod 8 (`at`
    samples lie in front of the filler)."""
    out = []
    fill = 40 + (residue - at - 40) % 8
    sig = steps(rng, fill)
    out.append(Case("%s/filler%d" % (tag, fill), spiked(as_i16(sig) if dtype == np.int16 else sig * 0.25), _tags(fill)))
    for n in lengths:
        sig = steps(rng, n)
        if dtype == np.int16:
            sig = spiked(as_i16(sig))
        else:
            sig = spiked(sig * 0.2317 - 40.0)          # fractional parts, negative values
        out.append(Case("%s/n%d" % (tag, n), sig, _tags(n)))
    return out


def int16_edges():
    """Every tile-edge length behind every prefix residue, one batch.  Lengths sum to a multiple of 8 in no block, so the blocks
    are kept apart by their fillers alone."""
    rng = np.random.default_rng(20261016)
    lengths = TINY + SEAMS + FIRST_INTERIOR + LAST_TILE + (HIST_TILE - 1,)
    lengths = tuple(sorted(set(lengths), key=lambda n: (n * 2654435761) % 4093))          # neighbours of unlike lengths
    cases = []
    for r in range(8):
        at = sum(len(c.signal) for c in cases)
        cases += edge_block(rng, np.int16, lengths, at, r, "r%d" % r)
        if r == 3:
            # an empty read and a one-sample read between two long ones
            cases.append(Case("r3/empty", np.zeros(0, np.int16), frozenset(["degenerate"])))
            cases.append(Case("r3/one", np.array([777], np.int16), frozenset(["degenerate"])))
    return Batch("int16_edges", np.int16, cases, 0)


def int16_leak():
    """Reads of negative samples between reads of positive ones, all with edge samples far above the rest: the zero pad makes the
    median at the edge of a negative read 0 and drops the edge sample of a positive one; the neighbour's edge sample in the pad's
    place (+20000 next to -500, +30000 next to +500) would change both."""
    rng = np.random.default_rng(77)
    cases = []
    for k in range(24):
        n = 4200 + 11 * k + k % 8 if k % 3 else 150 + k
        x = as_i16(steps(rng, n))
        if k % 2:
            x = (-x).astype(np.int16)
            x[0] = 20000 + k; x[-1] = 21000 + k
        else:
            x[0] = 30000 + k; x[-1] = 29000 + k
        cases.append(Case("leak%d/n%d" % (k, n), x, _tags(n)))
    return Batch("int16_leak", np.int16, cases, 0)


def int16_ranges():
    """Value ranges and read lengths beyond one histogram tile."""
    rng = np.random.default_rng(4242)
    cases = []
    for n in HIST_SEAMS + (LONG_READ,):
        cases.append(Case("hist/n%d" % n, as_i16(steps(rng, n)), frozenset()))
    x = as_i16(steps(rng, 9000))
    for at, v in ((1000, -32768), (3000, 32767), (5000, -32768), (7001, 32767)):
        x[at:at + 4] = v                                           # plateaus survive the filter
    cases.append(Case("range/extremes", x, frozenset()))
    x = steps(rng, 20000); x[9000:] += 6000.0
    x = as_i16(x)
    for at in rng.integers(100, 19900, 40):
        x[at:at + 3] = 9000 + int(at) % 5000                       # far above the tile minimum
    cases.append(Case("range/step6000", x, frozenset(["empty_tails"])))
    cases.append(Case("range/x40", as_i16((steps(rng, 24000, 300.0, 700.0) - 500.0) * 40.0), frozenset()))
    for bins in (HSTAT_LDS_BINS, HSTAT_LDS_BINS + 1):
        x = np.clip(as_i16((steps(rng, 18000) - 500.0) * 40.0), -7000, -7000 + bins - 1).astype(np.int16)      # the two planted levels land on the bounds
        x[2000:2004] = -7000; x[12000:12004] = -7000 + bins - 1
        cases.append(Case("range/bins%d" % bins, x, frozenset()))
    cases.append(Case("range/two_valued", np.where((np.arange(6000) // 5) % 2, 400, 600).astype(np.int16), frozenset(["empty_tails"])))
    cases.append(Case("range/constant", np.full(5000, 500, np.int16), frozenset(["degenerate"])))
    return Batch("int16_ranges", np.int16, cases, 0)


def near_integer_levels(rng, reps=4):
    """A float64 read whose z * 24 + 127 lies within an ulp or two of an integer at every sample: plateaus of twelve samples at
    m + (k - 127) * c, the k symmetric about 127 with mean |k - 127| = 24, so that the median is m and the MAD 24 c."""
    a = np.repeat(np.arange(49), 2 * reps); s = np.tile(np.repeat([1, -1], reps), 49)
    k = 127 + (a * s)[rng.permutation(len(a))]
    return 90.3 + (np.repeat(k, 12) - 127) * 0.37


def float64_edges():
    rng = np.random.default_rng(31337)
    lengths = tuple(sorted(set(TINY + SEAMS + (2 * COND_TILE + COND_HALO - 1, 2 * COND_TILE + COND_HALO) + LAST_TILE[:3]), key=lambda n: (n * 40503) % 4093))
    cases = edge_block(rng, np.float64, lengths, 0, 0, "f0")
    for r in range(1, 8):
        # interior tiles behind every residue: the 8-byte level store holds only when the read starts at a multiple of 8
        at = sum(len(c.signal) for c in cases)
        cases += edge_block(rng, np.float64, (2 * COND_TILE + COND_HALO + r,), at, r, "f%d" % r)
        cases += edge_block(rng, np.float64, (3 * COND_TILE + 17,), at + len(cases[-2].signal) + len(cases[-1].signal), r, "g%d" % r)
    cases.append(Case("f/near_integer", near_integer_levels(rng), frozenset()))
    cases.append(Case("f/negative", -np.abs(steps(rng, 5000)) * 0.37, frozenset()))
    x = steps(rng, 4500) * 0.25; x[2222] = np.nan
    cases.append(Case("f/nan", x, frozenset()))                       # a lone NaN: the median of three drops it
    x = steps(rng, 4400) * 0.25; x[1000:1002] = np.nan
    cases.append(Case("f/nan_pair", x, frozenset(["degenerate"])))    # two in a row stay, every statistic is NaN
    cases.append(Case("f/empty", np.zeros(0), frozenset(["degenerate"])))
    cases.append(Case("f/constant", np.full(4200, 88.25), frozenset(["degenerate"])))
    cases.append(Case("f/hist_seam", steps(rng, HIST_TILE + 1) * 0.25, frozenset()))
    return Batch("float64_edges", np.float64, cases, 0)


def sub_batch_cases(dtype, residue, per=6):
    """2 * `per` reads for STRQ_SUBBATCH_READS = per: the first sub-batch holds `residue` samples more than a multiple of 8, the
    last one the reads that are compared (an empty and a one-sample read between long ones among them)."""
    rng = np.random.default_rng(900 + residue + (0 if dtype == np.int16 else 50))
    conv = (lambda x: spiked(as_i16(x))) if dtype == np.int16 else (lambda x: spiked(x * 0.2317 - 40.0))
    first = [Case("sb%d/pre%d" % (residue, i), conv(steps(rng, 48 + (residue if i == 0 else 0))), _tags(48)) for i in range(per)]
    last = [Case("sb%d/n%d" % (residue, n), conv(steps(rng, n)), _tags(n)) for n in (3 * COND_TILE + 17, 0, 1, 2 * COND_TILE + COND_HALO + 1, COND_TILE + 2, 17)]
    assert len(last) == per
    return Batch("sub_batch_r%d_%s" % (residue, np.dtype(dtype).name), dtype, first + last, per)


def two_part_cases():
    """More than 1024 reads from a host buffer: the library conditions such a sub-batch in two upload parts (the second half of
    the reads with the kernels' read tables starting in the middle of the sub-batch)."""
    rng = np.random.default_rng(1024)
    cases = []
    for i in range(1100):
        if i % 100 == 57:
            n = 2 * COND_TILE + COND_HALO + 30 + i % 8
        elif i % 100 == 58:
            n = COND_TILE + 1 + i % 16
        else:
            n = 24 + (i * 7) % 41
        cases.append(Case("part/%d/n%d" % (i, n), spiked(as_i16(steps(rng, n))), _tags(n)))
    return Batch("two_parts", np.int16, cases, 0)


def all_batches():
    out = [int16_edges(), int16_leak(), int16_ranges(), float64_edges(), two_part_cases()]
    for r in range(8):
        out.append(sub_batch_cases(np.int16, r))
    for r in range(2):
        out.append(sub_batch_cases(np.float64, r))
    return out


def offsets(batch):
    off = np.zeros(len(batch.cases) + 1, np.int64)
    off[1:] = np.cumsum([len(c.signal) for c in batch.cases])
    return off


def compared(batch):
    """(index in the batch, index in the last sub-batch, samples of the batch in front of the read, samples of the last sub-batch
    in front of it) of the reads the test hooks can see: those of the last sub-batch."""
    off = offsets(batch)
    first = 0 if not batch.sub else (len(batch.cases) - 1) // batch.sub * batch.sub
    return [(i, i - first, int(off[i]), int(off[i] - off[first])) for i in range(first, len(batch.cases))]


def phase(batch, at, rel, base=0):
    """The `a0` classify() wants: int16 -- samples between the 16-byte boundary in front of the read and its first sample, for a
    batch buffer that starts `base` samples behind such a boundary; float64 -- the read's offset in the level stream of its
    sub-batch mod 8 (that stream starts on an 8-byte boundary)."""
    return (base + at) % 8 if batch.dtype == np.int16 else rel % 8


# ---------------------------------------------------------------------------------------------------------------------------
# expected values: numpy restatements, nothing from the library
def tails(x):
    """Centre and half-width of the reference's 'minmax' map (STRique.py:152-160)."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if len(x) == 0 or np.isnan(x).any():
            return np.nan, np.nan
        q_lo, q_hi = np.percentile(x, [1, 99])
        m_lo = np.median(x[x < q_lo]); m_hi = np.median(x[x > q_hi])
        return m_lo + (m_hi - m_lo) / 2, (m_hi - m_lo) / 2


Expected = namedtuple("Expected", "flt med mad u8 morph f_tails m_tails r_tails ok")


def expected(orc, opm, case):
    """What the oracle says about one read.  u8 / morph are None where the levels are undefined (MAD = 0, NaN, empty)."""
    s = case.signal
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flt = orc.medfilt3(s)
        if len(s) == 0:
            return Expected(flt, np.nan, np.nan, None, None, (np.nan, np.nan), (np.nan, np.nan), (np.nan, np.nan), False)
        med = np.median(flt); mad = orc.mad(flt)
        f_t = tails(flt.astype(np.float64)); r_t = tails(np.asarray(s, np.float64))
        if not mad > 0:
            return Expected(flt, med, mad, None, None, f_t, (np.nan, np.nan), r_t, False)
        _, u8, morph, _ = orc.condition(s, opm)
        m_t = tails(u8.astype(np.float64))
        ok = bool(np.isfinite(f_t[0]) and f_t[1] > 0 and np.isfinite(m_t[0]) and m_t[1] > 0)
        return Expected(flt, med, mad, u8, morph, f_t, m_t, r_t, ok)


# ---------------------------------------------------------------------------------------------------------------------------
# which path a read takes: the dispatch conditions of cond_kernels.hip in plain Python
def classify(case, dtype, a0, exp):
    """Names of the classes read `case` belongs to when it starts `a0` samples behind a 16-byte boundary (int16) / when `a0`
    reads' worth of samples mod 8 lie in front of it (float64: its tiles start at the read, `a0` decides only whether
    the 8-byte level store of an interior tile is aligned)."""
    n = len(case.signal)
    kind = "i16" if dtype == np.int16 else "f64"
    out = set()
    if exp.u8 is None:
        out.add("%s/mad0_or_undefined" % kind)
        if n and exp.mad == 0:
            out.add("%s/mad0" % kind)
    if n == 0:
        return out
    t_a0 = a0 if dtype == np.int16 else 0
    interior = 0; last = None
    for b in range((n + 7 + COND_TILE - 1) // COND_TILE + 1):
        t0 = b * COND_TILE - t_a0
        if t0 >= n:
            break
        lo = t0 - COND_HALO
        if lo >= 0 and lo + COND_TILE + 2 * COND_HALO <= n:
            interior += 1
        last = n - max(t0, 0)
    if exp.u8 is not None:          # quant_morph_kernel returns at once when MAD = 0
        out.add("%s/interior" % kind if interior else "%s/no_interior" % kind)
        if interior:
            out.add("%s/interior/a0=%d" % (kind, a0))
            if dtype != np.int16:
                out.add("f64/interior/store_%s" % ("aligned" if a0 == 0 else "unaligned"))
        if last <= 16:
            out.add("%s/last_tile=%d" % (kind, last))
        if not np.isfinite(exp.m_tails[0]):
            out.add("%s/empty_tails" % kind)
    if dtype == np.int16:
        if a0 > 0 and (n + a0) % 8 != 0 and n + a0 > 16:
            out.add("i16/partial_first_and_last_vector/a0=%d" % a0)
        if (n + a0 + HIST_TILE - 1) // HIST_TILE > 1:
            out.add("i16/hist_tiles>1")
        flt = exp.flt.astype(np.int64)
        for h in range((n + a0 + HIST_TILE - 1) // HIST_TILE):
            seg = flt[max(0, h * HIST_TILE - a0):h * HIST_TILE - a0 + HIST_TILE]
            if len(seg) and seg.max() - seg.min() >= HIST_WIN:
                out.add("i16/span>=HIST_WIN")
        nb = int(flt.max() - flt.min()) + 1
        out.add("i16/range>LDS" if nb > HSTAT_LDS_BINS else "i16/range<=LDS")
        if nb in (HSTAT_LDS_BINS, HSTAT_LDS_BINS + 1):
            out.add("i16/range=%d" % nb)
    elif n > HIST_TILE:
        out.add("f64/n>HIST_TILE")
    return out


def required_classes():
    req = set()
    for kind in ("i16", "f64"):
        req |= {"%s/interior" % kind, "%s/no_interior" % kind, "%s/empty_tails" % kind, "%s/mad0" % kind}
        req |= {"%s/last_tile=%d" % (kind, k) for k in range(1, 17)} if kind == "i16" else {"f64/last_tile=%d" % k for k in (1, 2, 3, 15, 16)}
    req |= {"i16/interior/a0=%d" % a for a in range(8)} | {"i16/partial_first_and_last_vector/a0=%d" % a for a in range(1, 8)}
    req |= {"f64/interior/store_aligned", "f64/interior/store_unaligned"}
    req |= {"i16/hist_tiles>1", "i16/span>=HIST_WIN", "i16/range>LDS", "i16/range<=LDS",
            "i16/range=%d" % HSTAT_LDS_BINS, "i16/range=%d" % (HSTAT_LDS_BINS + 1)}
    return req
