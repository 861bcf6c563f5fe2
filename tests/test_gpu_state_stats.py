"""State statistics on the GPU (strq_viterbi_state_stats, strq_set_state_stats, repeatCounter.state_stats_batch, `calibrate`) against
tests/state_stats_ref.py: the path of the oracle's Viterbi on the product's baked arrays and the rule as a plain loop.  n, sum and
sumsq are compared bit for bit; there is no tolerance anywhere."""
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import state_stats_ref as ssr
from conftest import oracle_map

pytestmark = pytest.mark.gpu

FRONTS = (1, 63, 64, 65, 128, 129)
NAMES = ("c9orf72", "fmr1")


def _flanked(pm, cfg, name, strand):
    from strique_amd import hmm
    repeat, prefix, suffix = cfg["repeat"][name][3:6]
    R, P, S = repeat.upper(), prefix[-50:].upper(), suffix[:50].upper()
    if strand == "-":
        R, P, S = ssr.revcomp(R), ssr.revcomp(S), ssr.revcomp(P)
    return hmm.FlankedRepeatModel(R, P, S, pm, cfg["HMM"])


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    return ffi.Context(0)


@pytest.fixture(scope="module")
def items(pm, cfg):
    """Reads of 3.5 to 8 kb with 4 to 60 units: per target and strand three reads, one of them with float64 samples; the last
    c9orf72 + read is by far the longest window (60 units against at most 12)."""
    from strique_amd import synth
    table = synth.KmerTable(pm)
    out = []
    k = 0
    for name in NAMES:
        target = tuple(cfg["repeat"][name][3:6])
        for strand in "+-":
            for j, (nt, units) in enumerate(((3500, 4 + k % 3), (5000, 7 + k % 3), (8000, 60 if (name, strand) == ("c9orf72", "+") else 10 + k % 3))):
                sig = synth.make_read(table, 9, 4100 + k, nt, target, units, strand=strand, as_int16=(k % 3 != 1))[0]
                out.append((name, sig, strand)); k += 1
    return out


@pytest.fixture(scope="module")
def windows(items, pm, cfg, orc, opm):
    """Per read of `items`: (row, x or None) of the oracle, and per (target, strand) the product's flanked model.  Computed once."""
    from conftest import oracle_tc
    targets = {n: tuple(cfg["repeat"][n][3:6]) for n in NAMES}
    tcs = {(n, s): oracle_tc(orc, opm, targets, n, s, cfg["HMM"]) for n in NAMES for s in "+-"}
    wins = oracle_map(lambda it: ssr.oracle_window(orc, opm, cfg, tcs[(it[0], it[2])], it[1]), items)
    models = {(n, s): _flanked(pm, cfg, n, s) for n in NAMES for s in "+-"}
    return wins, models


@pytest.fixture(scope="module")
def expected(items, windows, orc):
    """The reference statistics of every read of `items` (None without a window or a path).  Computed once, never changed."""
    wins, models = windows
    def one(job):
        it, (row, x) = job
        if x is None:
            return None
        ref = ssr.reference(orc, models[(it[0], it[2])].baked, x)
        return None if ref[2] else ref
    return oracle_map(one, list(zip(items, wins)))


def _check(ctx, orc, mid, baked, xs, want_status=None):
    """viterbi_state_stats of the windows against the reference and against viterbi_batch; returns (status, n, sum, sumsq)."""
    logp, counted, status, n, s, q = ctx.viterbi_state_stats(mid, xs)
    assert n.dtype == np.int64 and s.dtype == q.dtype == np.float64 and n.shape == s.shape == q.shape == (len(xs), baked.silent_start)
    blogp, bcounted, bstatus, _ = ctx.viterbi_batch(mid, xs, False)
    assert np.array_equal(ssr.bits(logp), ssr.bits(np.asarray(blogp, np.float64))) and np.array_equal(counted, bcounted)
    refs = oracle_map(lambda x: ssr.reference(orc, baked, x), xs)
    for i, (x, ref) in enumerate(zip(xs, refs)):
        assert status[i] == ref[2] == bstatus[i] if want_status is None else status[i] == want_status[i], (i, len(x), status[i])
        if ref[2] == 0:
            assert np.float64(logp[i]).tobytes() == np.float64(ref[0]).tobytes() and counted[i] == ref[1], (i, len(x))
        if status[i] == 0:
            assert ssr.same_rows((n[i], s[i], q[i]), ref[3:]), (i, len(x))
            assert int(n[i].sum()) == len(x) - int(np.isnan(x).sum())
        else:
            assert not n[i].any() and not ssr.bits(s[i]).any() and not ssr.bits(q[i]).any(), (i, len(x))          # zero rows, +0.0 bits
    return status, n, s, q


# ---- model level -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strand", [(n, s) for n in NAMES for s in "+-"])
def test_flanked_models_whole_windows_and_fronts(ctx, orc, items, windows, name, strand):
    """Whole windows of the three reads of the target and strand, and T = 1 .. 129 cut from the front of one (most fronts have no
    path: status 1, zero rows); the statistics of visited and of never visited states, logp and counted as viterbi_batch."""
    wins, models = windows
    m = models[(name, strand)]
    whole = [np.ascontiguousarray(x) for it, (row, x) in zip(items, wins) if (it[0], it[2]) == (name, strand) and x is not None]
    assert len(whole) == 3
    xs = whole + [whole[1][:T].copy() for T in FRONTS]
    mid = ctx.model_create(m.baked)
    status, n, s, q = _check(ctx, orc, mid, m.baked, xs)
    assert status[:3].tolist() == [0, 0, 0]
    unvisited = n[0] == 0
    assert unvisited.any() and not ssr.bits(s[0])[unvisited].any() and not ssr.bits(q[0])[unvisited].any()


def test_all_whole_windows_in_one_call(ctx, orc, windows):
    """Twelve windows of one model's kernel shape in one call (one model: the c9orf72 + strand decodes them all, whatever they hold)."""
    wins, models = windows
    m = models[("c9orf72", "+")]
    xs = [np.ascontiguousarray(x) for _, x in wins if x is not None]
    assert len(xs) >= 8
    _check(ctx, orc, ctx.model_create(m.baked), m.baked, xs)


def _tiny_model():
    """Two Normal states and a Uniform one, every one reachable from start and leading to end: a path exists at T = 1."""
    from strique_amd import hmm
    g = hmm.Graph()
    a = g.add_state("a", hmm.NORMAL, (80.0, 2.0)); b = g.add_state("b", hmm.NORMAL, (100.0, 3.0)); u = g.add_state("u", hmm.UNIFORM, (40.0, 160.0))
    for s, p in ((a, .5), (b, .3), (u, .2)):
        g.add_transition(g.start, s, p)
    for s in (a, b, u):
        for t, p in ((a, .3), (b, .3), (u, .2)):
            g.add_transition(s, t, p if s != t else p + .1)
        g.add_transition(s, g.end, .1)
    return hmm.bake(g, count_states=(b,))


def test_tiny_model_has_paths_at_every_length(ctx, orc):
    baked = _tiny_model()
    rng = np.random.default_rng(11)
    xs = []
    for T in FRONTS + (300,):
        level = np.repeat(rng.choice([80.0, 100.0, 130.0], T // 7 + 1), 7)[:T]
        xs.append(level + rng.normal(0, 1.5, T))
    status, n, s, q = _check(ctx, orc, ctx.model_create(baked), baked, xs)
    assert not status.any() and [int(r.sum()) for r in n] == [len(x) for x in xs]


def test_a_state_that_emits_300_observations_in_a_row(ctx, orc, windows, items):
    """A stretch of 320 observations at the level of one repeat match state, with full-mantissa noise, spliced into a window where the
    path is in that state: it crosses five round boundaries of the kernel, so any regrouping of the sum shows in the last bits."""
    wins, models = windows
    m = models[("c9orf72", "+")]
    x = next(np.ascontiguousarray(x) for it, (row, x) in zip(items, wins) if (it[0], it[2]) == ("c9orf72", "+") and x is not None)
    _, path, _ = orc.viterbi(m.baked, x)
    what = m.state_kmers()
    t = next(t for t in range(len(path) // 2, len(path)) if what[path[t]][:2] == ("repeat", "match"))
    s = int(path[t])
    rng = np.random.default_rng(5)
    stretch = m.baked.emis_a[s] + rng.normal(0, 0.4, 320) * (1 + rng.random(320) * 2.0 ** -30)
    x2 = np.concatenate([x[:t], stretch, x[t:]])
    _, path2, _ = orc.viterbi(m.baked, x2)
    runs = np.flatnonzero(np.diff(path2) != 0)
    longest = int(np.diff(np.concatenate([[-1], runs, [len(path2) - 1]])).max())
    assert longest >= 300 and np.bincount(path2, minlength=m.baked.silent_start)[s] >= 300
    status, n, _, _ = _check(ctx, orc, ctx.model_create(m.baked), m.baked, [x2, x2[:t + 200], x2[3:]])
    assert status[0] == 0 and n[0][s] >= 300


def test_missing_observations_are_skipped(ctx, orc, windows, items):
    wins, models = windows
    m = models[("fmr1", "-")]
    x = next(np.ascontiguousarray(x) for it, (row, x) in zip(items, wins) if (it[0], it[2]) == ("fmr1", "-") and x is not None).copy()
    rng = np.random.default_rng(8)
    x[rng.choice(len(x), len(x) // 25, replace=False)] = np.nan
    x[64:70] = np.nan          # a run of them across the start of a round
    status, n, s, q = _check(ctx, orc, ctx.model_create(m.baked), m.baked, [x])
    assert status[0] == 0 and int(n[0].sum()) == len(x) - int(np.isnan(x).sum()) < len(x)
    assert not np.isnan(s[0]).any() and not np.isnan(q[0]).any()


def test_a_model_beyond_the_lane_layouts(ctx, orc, pm, cfg):
    """A 70 nt repeat unit: more than 512 emitting states, the general kernel, a row with more than 512 entries."""
    from strique_amd import ffi, hmm
    rng = np.random.default_rng(31337)
    nt = lambda n: "".join(rng.choice(list("ACGT"), n))
    unit, prefix, suffix = nt(70), nt(50), nt(50)
    m = hmm.FlankedRepeatModel(unit, prefix, suffix, pm, cfg["HMM"])
    assert m.baked.silent_start > 512 and ffi.debug_viterbi_plan(m.baked)["csr"] == 1
    xs = []
    for units in (3, 5):
        sig = pm.generate_signal(prefix + unit * units + suffix, samples=0, noise=True, rng=rng)
        xs.append(np.clip(sig, pm.model_min + .5, pm.model_max - .5))
    xs.append(xs[0][:65].copy())
    status, n, s, q = _check(ctx, orc, ctx.model_create(m.baked), m.baked, xs)
    assert status[:2].tolist() == [0, 0] and n.shape[1] == m.baked.silent_start


def test_budget_three_pieces_and_one_window_over_it(ctx, orc, windows, items):
    """STRQ_STATE_STATS_WS_BYTES at twice the back-pointers of the largest ordinary window: the five ordinary windows go in three
    pieces, the 60-unit window exceeds the budget alone -- status 4, zero rows, logp and counted valid; the others are unchanged."""
    wins, models = windows
    m = models[("c9orf72", "+")]
    xs = [np.ascontiguousarray(x) for it, (row, x) in zip(items, wins) if it[0] == "c9orf72" and x is not None]
    assert len(xs) == 6
    size = lambda x: ((len(x) + 1) * m.baked.n_states * 2 + 15) & ~15
    order = sorted(range(6), key=lambda i: len(xs[i]))
    long = order[-1]
    budget = 2 * size(xs[order[-2]])
    assert size(xs[long]) > budget and 3 * size(xs[order[0]]) > budget          # at most two windows per piece: 2 + 2 + 1
    mid = ctx.model_create(m.baked)
    base = ctx.viterbi_state_stats(mid, xs)
    assert not base[2].any()
    ctx.set_option("STRQ_STATE_STATS_WS_BYTES", str(budget))
    try:
        want = [4 if i == long else 0 for i in range(6)]
        status, n, s, q = _check(ctx, orc, mid, m.baked, xs, want_status=want)
    finally:
        ctx.set_option("STRQ_STATE_STATS_WS_BYTES", "")
    assert status.tolist() == want
    for i in range(6):
        if i != long:
            assert ssr.same_rows((n[i], s[i], q[i]), (base[3][i], base[4][i], base[5][i]))


# ---- pipeline ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counter(pm, cfg):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in NAMES:
        rc.add_target(name, *cfg["repeat"][name][3:6])
    return rc


def _same_stats(got, want):
    return (got is None) == (want is None) and (got is None or ssr.same_rows(got, want[3:]))


def test_state_stats_batch_equals_the_reference(counter, items, windows, expected):
    """Twelve reads over both targets, both strands, int16 and float64 samples (both affine sources): the rows are detect()'s, the
    statistics those of the oracle's window and path."""
    wins, models = windows
    assert {np.asarray(sig).dtype for _, sig, _ in items} == {np.dtype(np.int16), np.dtype(np.float64)}
    got = counter.state_stats_batch(items)
    assert sum(w is not None for w in expected) >= 8
    for it, (row, stats), (orow, x), want in zip(items, got, wins, expected):
        assert tuple(row[:6]) == tuple(orow[:6]), (it[0], it[2])
        assert _same_stats(stats, want), (it[0], it[2])
        if stats is not None:
            tc = counter.targets[it[0]][0 if it[2] == "+" else 1]
            assert len(stats[0]) == tc.repeatHMM.baked.silent_start == len(tc.repeatHMM.state_kmers())
            assert int(stats[0].sum()) == len(x)
    assert [r for r, _ in got] == counter.detect_batch(items)
    # the switch is off again, and the product's models are the ones the reference used
    assert counter.ctx.last_state_stats()["windows"] == 0
    for (n, s), m in models.items():
        assert counter.targets[n][0 if s == "+" else 1].repeatHMM.baked.names == m.baked.names


def test_rows_do_not_change_and_other_passes_run_beside_it(counter, items, expected):
    ints = [(it, w) for it, w in zip(items, expected) if np.asarray(it[1]).dtype == np.int16]
    its = [it for it, _ in ints]
    off = counter.detect_batch(its, units=True, confidence=True)
    counter.ctx.set_state_stats(True)
    try:
        on = counter.detect_batch(its, units=True, confidence=True)
        stats = counter.ctx.batch_fetch_state_stats()
        info = counter.ctx.last_state_stats()
    finally:
        counter.ctx.set_state_stats(False)
    assert len(on) == len(off) and [r for r, _, _ in on] == [r for r, _, _ in off] == counter.detect_batch(its)
    for (_, u1, c1), (_, u0, c0) in zip(on, off):
        assert (u1 is None) == (u0 is None) and (u1 is None or np.array_equal(u1, u0)) and c1 == c0
    assert all(_same_stats(g, w) for g, (_, w) in zip(stats, ints))
    assert info["windows"] == sum(w is not None for _, w in ints) and info["launches"] >= 3 and info["bp_bytes"] > 0 and info["ms"] > 0


def test_reads_without_a_decode_have_none(counter, items):
    rng = np.random.default_rng(3)
    bad = [("c9orf72", np.full(5000, 300, np.int16), "+"),                           # constant: not conditioned
           ("c9orf72", rng.integers(200, 800, 6000).astype(np.int16), "-")]          # no flank: the gate fails
    good = [it for it in items if np.asarray(it[1]).dtype == np.int16][:2]
    got = counter.state_stats_batch(bad[:1] + good + bad[1:])
    assert got[0][1] is None and got[0][0][0] == 0 and got[1][1] is not None and got[2][1] is not None
    assert got[3][1] is None or got[3][0][0] != 0
    assert [r for r, _ in got] == counter.detect_batch(bad[:1] + good + bad[1:])


def test_budget_in_the_pipeline(counter, items, expected):
    """STRQ_STATE_STATS_WS_BYTES small: several pieces, and the one read whose back-pointers exceed it alone has status 2."""
    pick = [(it, w) for it, w in zip(items, expected) if it[0] == "c9orf72" and w is not None and np.asarray(it[1]).dtype == np.int16]
    its = [it for it, _ in pick]
    assert len(its) >= 4
    counter.state_stats_batch(its)
    whole = counter.ctx.last_state_stats()
    n_states = counter.targets["c9orf72"][0].repeatHMM.baked.n_states
    T = sorted(int(w[3].sum()) for _, w in pick)
    budget = 2 * (((T[-2] + 1) * n_states * 2 + 15) & ~15)
    assert ((T[-1] + 1) * n_states * 2) > budget
    counter.ctx.set_option("STRQ_STATE_STATS_WS_BYTES", str(budget))
    try:
        got = counter.state_stats_batch(its)
        info = counter.ctx.last_state_stats()
        status, stats = counter.ctx.batch_fetch_state_stats(with_status=True)
    finally:
        counter.ctx.set_option("STRQ_STATE_STATS_WS_BYTES", "")
    longest = max(range(len(pick)), key=lambda i: int(pick[i][1][3].sum()))
    assert status.tolist() == [2 if i == longest else 0 for i in range(len(pick))]
    assert info["launches"] > whole["launches"] and info["bp_bytes"] <= budget < whole["bp_bytes"]
    for i, ((row, st), (_, w)) in enumerate(zip(got, pick)):
        assert (st is None and stats[i] is None) if i == longest else (_same_stats(st, w) and _same_stats(stats[i], w))


def test_fetch_refuses_after_a_run_without_the_switch(counter, items):
    from strique_amd import ffi
    counter.detect_batch(items[:2])
    assert counter.ctx.last_state_stats() == {"ms": 0.0, "windows": 0, "launches": 0, "bp_bytes": 0.0}
    with pytest.raises(ffi.StriqueHipError, match=r"the last batch ran without state statistics \(strq_set_state_stats\)"):
        counter.ctx.batch_fetch_state_stats()


# ---- calibrate ---------------------------------------------------------------------------------------------------------------------
def test_calibrate_end_to_end(workdir, tables, cfg, orc):
    """The six planted-shift c9orf72 reads of the CPU check through `calibrate`: --out and --stats equal, byte for byte, what
    calibrate.py makes of the reference statistics."""
    import h5write
    from strique_amd import calibrate, cli
    from strique_amd.pore_model import pore_model
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    target = (repeat, prefix, suffix)
    planted, _ = ssr.planted_table(tables, repeat)
    reads = ssr.planted_reads(planted, target)
    named, sam = [], ["@HD\tVN:1.0"]
    for i, (sig, strand, _) in enumerate(reads):
        rid = "%08d-0000-4000-8000-%012d" % (i, i)
        named.append((rid, sig))
        sam.append("\t".join([rid, "16" if strand == "-" else "0", chrom, str(b - 3000), "60", "12S6000M5S", "*", "0", "0", "ACGT", "*"]))
    bulk = workdir / "bulk"; bulk.mkdir()
    (bulk / "batch_0.fast5").write_bytes(h5write.multi_read_fast5(named))
    buf = io.StringIO()
    with redirect_stdout(buf):
        cli.main(["index", str(bulk)])
    (bulk / "reads.fofn").write_text(buf.getvalue())
    (workdir / "aln.sam").write_text("\n".join(sam) + "\n")
    out, stats = workdir / "new.model", workdir / "stats.tsv"
    cli.main(["calibrate", str(bulk / "reads.fofn"), str(workdir / "r9_4_450bps.model"), str(workdir / "repeat_config.tsv"), "--config", str(workdir / "STRique.json"),
              "--algn", str(workdir / "aln.sam"), "--out", str(out), "--stats", str(stats), "--min-score", "3.0", "--min-obs", "200", "--batch", "4"])
    pm0 = pore_model(str(workdir / "r9_4_450bps.model"))
    shipped = (planted[0], np.array(tables["base_mean"], np.float64), planted[2])
    rows, records, _ = ssr.reference_records(orc, cfg, shipped, target, reads)
    assert len(records) == 6 and all(r[1] >= 3.0 and r[2] >= 3.0 for r in rows)
    means, srows = calibrate.estimate(calibrate.pool(records), pm0, 200)
    want = workdir / "want.model"
    calibrate.write_model(str(want), pm0, means)
    assert len(means) >= 6 and out.read_bytes() == want.read_bytes()
    assert stats.read_bytes() == calibrate.format(srows).encode()


from test_cli_end_to_end import workdir  # noqa: E402,F401  (model, config and repeat files in a temporary directory)
