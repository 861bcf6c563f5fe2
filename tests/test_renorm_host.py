"""The second normalisation step without a GPU: the rule (strique_amd/renorm.py) on the reads detect() loses as it stands, its gate,
its tie and edge cases against a plain restatement (tests/renorm_ref.py), and the `count --renorm` plumbing with a stubbed counter."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import renorm_ref as rr
from conftest import ROOT
from test_mod_llr_host import FakeCounter, OneRank


def _bytes(row):
    return tuple(np.float64(x).tobytes() if isinstance(x, float) else x for x in row)


@pytest.fixture(scope="module")
def lost(tables, cfg):
    return rr.run_specs(rr.LOST, tables, cfg, plain=True)


# ---- the rule on reads ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(rr.LOST)))
def test_rule_recovers_the_planted_count_where_detect_does_not(lost, cfg, k):
    spec, sig, row, rec, st, plain_row = lost[k]
    assert abs(rr.share_of(spec, cfg) - 0.87) < 0.01
    print(spec[0], "as it stands", plain_row[:3], "with the rule", row[:3], rec)
    assert plain_row[0] != spec[3]                               # the oracle's detect() as it stands does not find the planted count
    assert rec[0] == 1 and row[0] == spec[3]                     # ... the rule does, exactly
    f = rec[1]['filtered']
    assert rr.renorm.W[f[2]] >= 0.77 and f[0] < 64               # the map was stretched: alpha below 1
    assert rec[1]['raw'] is None and rec[1]['morph'] is not None


def test_reference_without_the_rule_is_the_oracle(tables, cfg, orc):
    """tests/renorm_ref.detect restates the oracle's detect(): with the rule left out the rows are equal to the bit."""
    _, opm, params = rr.setup(tables, cfg)
    for spec in (rr.READS[0], rr.READS[6]):
        tc = orc.classifier(*cfg["repeat"][spec[1]][3:6], spec[2], opm, None, cfg["HMM"])
        sig = rr.signal_of(spec, tables, cfg)
        assert _bytes(rr.detect(sig, tc, opm, params)[0]) == _bytes(orc.detect(sig, tc, opm, params)[0])


def test_read_below_min_share_is_byte_equal_to_the_ungated_oracle(tables, cfg, orc):
    _, opm, params = rr.setup(tables, cfg)
    specs = [s for s in rr.READS if s[6] == 0.04][:2]
    for (spec, sig, row, rec, st) in rr.run_specs(specs, tables, cfg):
        assert abs(rr.share_of(spec, cfg) - 0.04) < 0.005
        tc = orc.classifier(*cfg["repeat"][spec[1]][3:6], spec[2], opm, None, cfg["HMM"])
        f = rec[1]['filtered']
        assert rec[0] == 0 and f is not None and rr.renorm.W[f[2]] < rr.MIN_SHARE          # fitted, and left alone by the gate
        assert _bytes(row) == _bytes(orc.detect(sig, tc, opm, params)[0])
        maps, _, _, _, _ = rr.condition(sig, opm)
        assert st["maps"] == maps


def test_fitted_share_follows_the_true_share(tables, cfg):
    """Within two steps of the rule's share grid (0.07 each, rounded up): the flanks and the backbone hold repeat-like k-mers too, and
    the share of the samples is not the share of the bases."""
    for (spec, sig, row, rec, st) in rr.run_specs([s for s in rr.READS if s[5]], tables, cfg):
        w = rr.renorm.W[rec[1]['filtered'][2]]
        print(spec[0], "share", round(rr.share_of(spec, cfg), 3), "fitted", w, rec[1]['filtered'][:2], row[:3])
        assert abs(w - rr.share_of(spec, cfg)) <= 0.15
        if spec[6] > 0.5:
            assert rec[0] == 1 and row[0] == spec[3]


# ---- tie and edge cases of the rule ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qa(tables, cfg):
    _, opm, _ = rr.setup(tables, cfg)
    return {(name, strand): rr.target_tables(opm, cfg["repeat"][name][3], strand) for name in ("c9orf72", "fmr1") for strand in "+-"}, opm


def test_tables(qa):
    tabs, opm = qa
    rn = rr.renorm
    lo, d, p = rn.grid(opm.model_min, opm.model_max)
    assert lo + 256 * d == pytest.approx(opm.model_min) and lo + 768 * d == pytest.approx(opm.model_max) and p == pytest.approx(lo + 512.5 * d)
    assert len(rn.W) == 15 and rn.W[0] == 0 and rn.W[-1] == 0.98
    for (name, strand), (Q, A) in tabs.items():
        assert Q.dtype == np.int16 and Q.shape == (15, 1024) and A.dtype == np.int32 and A[64] == 0
        assert Q.min() >= rn.Q_OUT and np.array_equal(Q[0], tabs[("fmr1", "+")][0][0])          # w = 0: the background alone, whatever the target
        assert A[24] == int(np.rint(1024 * np.log(24 / 64))) and A[104] == int(np.rint(1024 * np.log(104 / 64)))
    # the - strand reads the reverse complement: other k-mers, another table
    assert not np.array_equal(tabs[("c9orf72", "+")][0][14], tabs[("c9orf72", "-")][0][14])
    assert rn.repeat_kmers("GGCCCC", 6) == ["GGCCCC", "GCCCCG", "CCCCGG", "CCCGGC", "CCGGCC", "CGGCCC"]
    assert rn.repeat_kmers("CGG", 6) == ["CGGCGG", "GGCGGC", "GCGGCG"]


@pytest.mark.parametrize("case", ["one_bin", "one_bin_low", "two_bins", "edge_bins", "single_sample", "flat"])
def test_fit_equals_the_plain_restatement(qa, case):
    """All samples in one bin (many (a, b) reach the same cell: the tie rule decides), bins at the rim of the grid (every scaled bin
    falls outside), a single sample, a flat histogram."""
    tabs, _ = qa
    Q, A = tabs[("c9orf72", "+")]
    h = np.zeros(1024, np.int64)
    if case == "one_bin":
        h[512] = 5000
    elif case == "one_bin_low":
        h[300] = 77
    elif case == "two_bins":
        h[400] = 10; h[640] = 10
    elif case == "edge_bins":
        h[0] = 3; h[1023] = 3
    elif case == "single_sample":
        h[700] = 1
    else:
        h[256:768:16] = 1
    got = rr.renorm.fit(h, Q, A)
    want = rr.ref_fit(h, Q, A)
    print(case, got)
    assert got == want
    if case == "one_bin":
        # the pivot bin does not move with a: every a scores the same cell, the smallest a of the best A[a] + Q wins -- A grows with a,
        # so the best a is the largest, and b the smallest shift that reaches the best cell
        assert got[0] == rr.renorm.A_MAX


def test_empty_histogram_and_degenerate_reads_are_not_fitted(qa, tables, cfg):
    tabs, opm = qa
    Q, A = tabs[("fmr1", "-")]
    assert rr.renorm.fit(np.zeros(1024, np.int64), Q, A) is None
    # a constant read: no MAD, no map
    maps, signals, status, med, mad = rr.condition(np.full(5000, 417, np.int16), opm)
    assert status == 1
    out, rec = rr.renorm.apply(maps, signals, Q, A, opm.model_min, opm.model_max, 0.3, status)
    assert rec == (0, {'morph': None, 'filtered': None, 'raw': None}) and out == maps
    # a target without tables
    maps, signals, status, _, _ = rr.condition(rr.signal_of(rr.READS[0], tables, cfg)[:5000], opm)
    assert status == 0
    assert rr.renorm.apply(maps, signals, None, None, opm.model_min, opm.model_max, 0.3, status)[1][0] == 0
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            rr.renorm.apply(maps, signals, Q, A, opm.model_min, opm.model_max, bad, status)


def test_short_read_and_samples_outside_the_grid(qa, tables, cfg):
    tabs, opm = qa
    rn = rr.renorm
    spec = rr.READS[0]
    Q, A = tabs[(spec[1], spec[2])]
    sig = rr.signal_of(spec, tables, cfg)
    lo, d, p = rn.grid(opm.model_min, opm.model_max)
    # fewer than 64 samples: the 1 % tails of the morphology signal are empty (its minimum is a plateau of 8 samples and more), the
    # read has no 'minmax' map and is not fitted; a histogram of NaN maps is empty anyway
    for n in (40, 63):
        short = sig[5000:5000 + n]
        maps, signals, status, _, _ = rr.condition(short, opm)
        assert status == 1 and rn.histogram(signals['morph'], *maps['morph'], maps['h2'], maps['c2'], lo, d).sum() == 0
        out, rec = rn.apply(maps, signals, Q, A, opm.model_min, opm.model_max, 0.3, status)
        assert rec == (0, {'morph': None, 'filtered': None, 'raw': None})
    # a short read that can be conditioned: the fit is that of the plain restatement
    maps, signals, status, _, _ = rr.condition(sig[5000:8000], opm)
    h = rn.histogram(signals['filtered'], *maps['filtered'], maps['h2'], maps['c2'], lo, d)
    assert status == 0 and 0 < h.sum() <= 3000
    assert rn.apply(maps, signals, Q, A, opm.model_min, opm.model_max, 0.3, status)[1][1]['filtered'] == rr.ref_fit(h, Q, A)
    # samples far outside the grid are dropped from the histogram, and the fit is that of the samples inside it
    wild = rr.with_outliers(sig)
    maps, signals, status, _, _ = rr.condition(wild, opm)
    hw = rn.histogram(signals['filtered'], *maps['filtered'], maps['h2'], maps['c2'], lo, d)
    assert status == 0 and hw.sum() == len(wild) - 180
    b = rn.bins(np.array([np.nan, np.inf, -np.inf, 1e300]), 0.0, 1.0, maps['h2'], maps['c2'], lo, d)
    assert list(b) == [-1, -1, -1, -1]


def test_fold_is_the_map_composed_with_the_fit(qa):
    """x -> alpha * (map(x) - p) + p + b * d equals the folded map, up to rounding."""
    _, opm = qa
    rn = rr.renorm
    lo, d, p = rn.grid(opm.model_min, opm.model_max)
    c1, h1, h2, c2 = 512.25, 101.5, 20.125, 88.5
    x = np.linspace(300, 700, 41)
    for a, b in ((24, -128), (64, 0), (50, 5), (104, 128)):
        c1n, h1n = rn.fold(c1, h1, h2, c2, a, b, p, d)
        want = (a / 64) * (((x - c1) / h1 * h2 + c2) - p) + p + b * d
        assert np.allclose((x - c1n) / h1n * h2 + c2, want, rtol=0, atol=1e-9)
    assert rn.fold(c1, h1, h2, c2, 64, 0, p, d)[1] == h1


# ---- command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,needle", [
    (["--renorm", "0"], "inside (0, 1)"),
    (["--renorm", "1"], "inside (0, 1)"),
    (["--renorm", "-0.2"], "inside (0, 1)"),
    (["--renorm", "nan"], "inside (0, 1)"),
    (["--renorm-out", "r.tsv"], "needs --renorm"),
    (["--renorm", "0.4", "--scan", "--scan-min-score", "5"], "--scan"),
])
def test_argument_errors(capsys, argv, needle):
    from strique_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.count(["reads.fofn", "r9.model", "repeats.tsv"] + argv)
    assert e.value.code == 2 and needle in capsys.readouterr().err


REPORTS = [None, (0, (None, None, None)), (0, ((0.07, 1.03125, 0.3125), (0.07, 1.0, 0.0), None)),
           (1, ((0.91, 0.703125, -1.25), (0.91, 0.78125, 0.7568359375), (0.84, 0.8125, 1.1)))]


def test_format_parse_round_trip():
    from strique_amd import renorm as rn
    assert rn.HEADER[:4] == ["ID", "target", "strand", "applied"] and len(rn.HEADER) == 13
    text = "\t".join(rn.HEADER) + "\n" + "".join(rn.format_row("read%d" % i, "fmr1", "+-"[i % 2], r) + "\n" for i, r in enumerate(REPORTS))
    rows = rn.parse(io.StringIO(text))
    assert rows == [("read%d" % i, "fmr1", "+-"[i % 2], r) for i, r in enumerate(REPORTS)]
    assert text.splitlines()[1].split("\t")[3:] == ["-"] * 10 and text.splitlines()[2].split("\t")[3:] == ["0"] + ["-"] * 9
    for r in REPORTS[1:]:
        assert rn.unpack(rn.pack(r)) == r
    assert rn.report((1, {'morph': (45, -8, 13, -5), 'filtered': (50, 5, 13, -7), 'raw': None}), 0.25) == (1, ((0.91, 45 / 64, -2.0), (0.91, 50 / 64, 1.25), None))
    assert rn.report(None, 0.25) is None
    with pytest.raises(ValueError):
        rn.parse(io.StringIO("ID\tx\n"))
    with pytest.raises(ValueError):
        rn.parse(io.StringIO("\t".join(rn.HEADER) + "\nr\tt\t+\t1\t-\n"))


def test_blob_carries_the_report():
    from strique_amd import cli
    assert "renorm" in [o.name for o in cli.OUTPUTS] and cli.Merged(None, None, None, None, None).renorm is None
    assert cli.Detected((0,), None, None, None).renorm is None
    on = cli.outputs_on(units=True, renorm=True)
    assert [o.name for o in on] == ["units", "renorm"]
    for rep in REPORTS:
        blob = cli.pack_blob(on, "fmr1", "-", "-", dict(units=np.array([5, 9]), renorm=rep))
        assert blob.count("\t") == 2 + len(cli.OUTPUTS)
        t, s, m, got = cli.unpack_blob(on, blob)
        assert (t, s, m) == ("fmr1", "-", "-") and got["units"] == [5, 9] and got["renorm"] == rep
    off = cli.outputs_on(units=True)
    assert cli.unpack_blob(off, cli.pack_blob(off, "fmr1", "-", "-", dict(renorm=REPORTS[3])))[3]["renorm"] is None


class RenormCounter(FakeCounter):
    """FakeCounter with the switch: with it on, reads of an even length are 'applied' and their count changes; the record depends on
    the inputs only."""
    renorm_bin_width = 0.25

    def __init__(self):
        self.renorm = None
        self.switched = []

    def set_renorm(self, min_share):
        self.switched.append(min_share)
        self.renorm = min_share

    def detect_batch(self, items, units=False, confidence=False, mod_llr=False, records=False):
        from strique_amd.counter import Detected
        plain = FakeCounter.detect_batch(self, items, units=units, confidence=confidence, mod_llr=mod_llr)
        if self.renorm is None:
            assert not records
            return plain
        assert records
        out = []
        for (t, raw, s), res in zip(items, plain):
            any_extra = units or confidence or mod_llr
            rest = iter(res[1:]) if any_extra else iter(())
            row = res[0] if any_extra else res
            applied = int(len(raw) % 2 == 0)
            fits = {'morph': (40 + len(raw) % 30, len(raw) % 9 - 4, 13, -len(raw)), 'filtered': (41 + len(raw) % 30, 3, 12 if applied else 1, -2 * len(raw)),
                    'raw': None if len(raw) % 3 else (64, 0, 0, -1)}
            if len(raw) % 5 == 0:
                applied, fits = 0, {'morph': None, 'filtered': None, 'raw': None}
            if applied:
                row = (row[0] + 1000,) + tuple(row[1:])
            out.append(Detected(row, next(rest) if units else None, next(rest) if confidence else None, next(rest) if mod_llr else None, None, None, (applied, fits)))
        return out

    def detect(self, t, raw, s, units=False, confidence=False, mod_llr=False, records=False):
        return self.detect_batch([(t, raw, s)], units=units, confidence=confidence, mod_llr=mod_llr, records=records)[0]


def _sam(n=23):
    lines = ["@HD\tVN:1.0"]
    for i in range(n):
        chrom, pos = ("chr9", 27570000) if i % 3 else ("chrX", 146990000)
        lines.append("\t".join(["read%d" % i, "16" if i % 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))
    return lines


@pytest.mark.parametrize("units", [False, True])
def test_count_rows_with_a_stubbed_counter(cfg, units):
    """The side file next to the count rows, single process and through the gather's blob; without the switch every file is
    byte-identical to a counter that never heard of it; the switch belongs to the run."""
    from strique_amd import cli, renorm as rn
    loci = {}
    for name, (chrom, b, e, *_r) in cfg["repeat"].items():
        loci.setdefault(chrom, []).append((name, b, e))
    lines = _sam()
    get_raw = lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))
    log = cli.Log("error")

    def run(counter, **more):
        f = {k: io.StringIO() for k in ("rows", "units")}
        cli.run_count(iter(lines), loci, get_raw, counter, log, 4, 0, 1, f["rows"], units=units, units_out=f["units"] if units else None, **more)
        return f
    plain = run(FakeCounter())
    off = run(RenormCounter())
    assert plain["rows"].getvalue() == off["rows"].getvalue() and plain["units"].getvalue() == off["units"].getvalue()
    side = io.StringIO()
    c = RenormCounter()
    on = run(c, renorm=0.4, renorm_out=side)
    assert c.switched == [0.4, None] and c.renorm is None
    nofile = run(RenormCounter(), renorm=0.4)
    assert on["rows"].getvalue() == nofile["rows"].getvalue() != plain["rows"].getvalue()
    strip = lambda text_: [l.split("\t")[:3] + l.split("\t")[4:] for l in text_.splitlines()]          # (the units file repeats the count)
    assert on["units"].getvalue() == nofile["units"].getvalue() and strip(on["units"].getvalue()) == strip(plain["units"].getvalue())
    rows = rn.parse(io.StringIO(side.getvalue()))
    count_rows = [l.split("\t") for l in on["rows"].getvalue().splitlines()[1:]]
    plain_rows = [l.split("\t") for l in plain["rows"].getvalue().splitlines()[1:]]
    assert len(rows) == 23 and [(r[0], r[1], r[2]) for r in rows] == [tuple(cr[:3]) for cr in count_rows]
    for r, cr, pr in zip(rows, count_rows, plain_rows):
        applied, fits = r[3]
        assert int(cr[3]) == int(pr[3]) + 1000 * applied and cr[4:] == pr[4:]
        assert (fits[1] is None) == (fits[0] is None) and (fits[1] is None or fits[1][0] == (0.84 if applied else 0.07))
    assert {r[3][0] for r in rows} == {0, 1} and any(r[3][1][2] is None for r in rows) and any(r[3][1][1] is None for r in rows)
    # two ranks, one gather: the same bytes
    stats = {}
    parts = [cli.run_count(iter(lines), loci, get_raw, RenormCounter(), log, 4, rank, 2, stats=stats if rank == 0 else {}, units=units, renorm=0.4) for rank in (0, 1)]
    merged = cli.gather_rows(parts[1] + parts[0], stats["items"], OneRank, units=units, renorm=True)
    text = lambda rows_, header: (lambda b: (cli.write_rows(b, rows_, header=header), b.getvalue())[1])(io.StringIO())
    assert text(merged.rows, True) == on["rows"].getvalue()
    assert text(merged.renorm, rn.HEADER) == side.getvalue()
    if units:
        assert text(merged.units, cli.UNITS_HEADER) == on["units"].getvalue()
    for bad in (dict(renorm=0.4, scan={"min_score": 5.0, "candidates": [("c9orf72", "+")], "scores": False}), dict(renorm=1.5)):
        with pytest.raises(ValueError):
            cli.run_count(["read1"], {}, get_raw, RenormCounter(), log, 4, 0, 1, io.StringIO(), **bad)


def test_counter_switch_without_a_device():
    """set_renorm validates its argument and leaves detect's keywords alone (no context is touched before a run)."""
    import inspect
    from strique_amd.counter import repeatCounter
    rc = repeatCounter.__new__(repeatCounter)
    rc.renorm = None
    for bad in (0, 1, -1, 2.5, float("nan")):
        with pytest.raises(ValueError):
            rc.set_renorm(bad)
    rc.set_renorm(0.45); assert rc.renorm == 0.45
    rc.set_renorm(None); assert rc.renorm is None
    rc.set_renorm(0.3); rc.set_renorm(False); assert rc.renorm is None
    assert "renorm" not in inspect.signature(repeatCounter.detect).parameters
    assert "renorm" not in inspect.signature(repeatCounter.detect_batch).parameters
    rc.renorm = 0.3
    with pytest.raises(ValueError):
        rc.scan_batch([np.arange(10)], min_score=5.0)


GLOO_WORKER = r'''
import io, json, os, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
from strique_amd import cli, dist as sdist, renorm as rn
from test_renorm_host import RenormCounter, _sam
rank, world, local = sdist.init_process_group(backend="gloo")
cfg = json.load(open(os.path.join(%r, "tests", "golden", "config.json")))
loci = {}
for name, (chrom, b, e, *_r) in cfg["repeat"].items():
    loci.setdefault(chrom, []).append((name, b, e))
lines = _sam(37)
get_raw = lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))
log = cli.Log("error")
stats = {}
mine = cli.run_count(iter(lines), loci, get_raw, RenormCounter(), log, 5, rank, world, stats=stats, renorm=0.4)
merged = cli.gather_rows(mine, stats["items"], sdist, renorm=True)            # the run's one collective carries the reports too
if rank == 0:
    one, side = io.StringIO(), io.StringIO()
    cli.run_count(iter(lines), loci, get_raw, RenormCounter(), log, 5, 0, 1, one, renorm=0.4, renorm_out=side)
    buf = io.StringIO(); cli.write_rows(buf, merged.rows)
    sbuf = io.StringIO(); cli.write_rows(sbuf, merged.renorm, header=rn.HEADER)
    assert buf.getvalue() == one.getvalue() and sbuf.getvalue() == side.getvalue()
    assert len(rn.parse(io.StringIO(sbuf.getvalue()))) == 37
    print("RENORM_GATHER_OK")
else:
    assert merged.rows is None and merged.renorm is None
import torch.distributed as dist
dist.barrier(); dist.destroy_process_group()
''' % (ROOT, ROOT, ROOT)


def test_two_rank_gloo_gather(tmp_path):
    script = tmp_path / "renorm_worker.py"
    script.write_text(GLOO_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29557", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "RENORM_GATHER_OK" in outs[0]
