"""Scan on the GPU (strq_scan_batch_reads, repeatCounter.scan_batch, `count --scan`): scores, winners and the winners' rows
against the oracle scan -- oracle.detect's geometry for every candidate, then strique_amd.scan.select -- and against the plain
detect path, on every route through the pipeline."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, oracle_map, oracle_tc
from test_scan_host import CANDIDATES, MIN_SCORE, bundled_read, oracle_scan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def counter(pm, cfg, targets):
    """The two bundled targets: four candidates."""
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in ("c9orf72", "fmr1"):
        rc.add_target(name, *targets[name])
    assert rc.candidates() == CANDIDATES
    return rc


def parity_reads(pm, targets):
    """[(true (target, strand) or None, signal)]: 24 synthetic reads over both targets and strands -- clean and empirical noise,
    int16 and four float64 --, the bundled real read, two reads of pure random sequence."""
    from strique_amd import synth
    table = synth.KmerTable(pm)
    noise = synth.EmpiricalNoise()
    out = []
    for c, (name, strand) in enumerate(CANDIDATES):
        for k in range(3):
            nt = 5000 + 700 * k
            out.append(((name, strand), synth.make_read(table, 32, 10 * c + k, nt, targets[name], 12 + 20 * k, strand=strand, as_int16=k != 2)[0]))
            out.append(((name, strand), synth.make_read(table, 33, 10 * c + k, nt, targets[name], 12 + 20 * k, strand=strand, noise=noise)[0]))
    name, strand, sig = bundled_read()
    out.append(((name, strand), sig))
    rng = np.random.default_rng(77)
    for nt in (5000, 7000):
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, nt)].tobytes()
        out.append((None, synth.make_signal(rng, table, seq)))
    return out


@pytest.fixture(scope="module")
def reads(pm, targets):
    return parity_reads(pm, targets)


@pytest.fixture(scope="module")
def expected(reads, cfg, orc, opm, targets):
    """(scores, geometry) of every read and candidate from the oracle."""
    return oracle_scan(orc, opm, cfg, targets, [sig for _, sig in reads])


def test_scan_equals_the_oracle_scan(counter, reads, expected, cfg, orc, opm, targets):
    """Every score of every candidate bit for bit, every winner equal to select() over the oracle's values, every winner's row
    equal to the oracle's detect() for that candidate.  No read is left out."""
    from strique_amd.scan import select
    sigs = [sig for _, sig in reads]
    got, scores = counter.scan_batch(sigs, min_score=MIN_SCORE, scores=True)
    assert len(got) == len(reads) == 27 and scores.shape == (27, 4, 2)
    want_win = [select(sc, geo, MIN_SCORE) for sc, geo in expected]
    for i, ((truth, sig), (sc, geo)) in enumerate(zip(reads, expected)):
        print(i, truth, sig.dtype, len(sig), "oracle", ["%.3f/%.3f" % s for s in sc], "winner", want_win[i])
        assert [tuple(x) for x in scores[i]] == [tuple(x) for x in sc], (i, truth)
        assert (CANDIDATES.index(got[i][:2]) if got[i] is not None else -1) == want_win[i], (i, truth, got[i])
    winners = [(i, CANDIDATES[w]) for i, w in enumerate(want_win) if w >= 0]
    rows = oracle_map(lambda iw: orc.detect(sigs[iw[0]], oracle_tc(orc, opm, targets, iw[1][0], iw[1][1], cfg["HMM"]), opm, orc.align_params(cfg["align"]))[0], winners)
    for (i, cand), want in zip(winners, rows):
        assert got[i][:2] == cand and tuple(got[i][2]) == tuple(want), (i, cand, got[i], want)
    # what the reads were made for: the clean reads and the real read find their target and strand
    for i, (truth, sig) in enumerate(reads):
        if truth is None:
            assert got[i] is None, (i, got[i])
    assert sum(got[i] is not None and got[i][:2] == truth for i, (truth, _) in enumerate(reads) if truth) >= 20


def test_rows_equal_the_plain_detect_path(counter, reads, pm, pm_mod, cfg, targets):
    sigs = [sig for _, sig in reads]
    got = counter.scan_batch(sigs, min_score=MIN_SCORE, units=True)
    items = [(g[0], sig, g[1]) for g, sig in zip(got, sigs) if g is not None]
    assert len(items) >= 20
    plain = counter.detect_batch(items, units=True)
    for g, (row, pos) in zip([g for g in got if g is not None], plain):
        assert g[2][0] == row, (g, row)
        assert (g[2][1] is None) == (pos is None) and (pos is None or np.array_equal(g[2][1], pos))
    # a target with a modification model: the pattern of the winner
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in ("c9orf72", "fmr1"):
        rc.add_target(name, *targets[name])
    repeat, prefix, suffix = targets["c9orf72"]
    rng = np.random.default_rng(12)
    backbone = "".join(rng.choice(list("ACTG"), 2000))
    msigs = []
    for n, model in ((40, pm), (40, pm_mod), (25, pm_mod)):
        sig = model.generate_signal(backbone[:1000] + prefix + repeat * n + suffix + backbone[-1000:], samples=8, noise=True, rng=rng)
        msigs += [sig, np.round(sig * (8192 / 1400.0) - 10).astype(np.int16)]
    mgot = rc.scan_batch(msigs, min_score=MIN_SCORE)
    assert all(g is not None and g[:2] == ("c9orf72", "+") for g in mgot), mgot
    assert [g[2] for g in mgot] == rc.detect_batch([("c9orf72", s, "+") for s in msigs])
    assert all(set(g[2][6]) <= set("01") and len(g[2][6]) > 10 for g in mgot)


def _raw_scan(ctx, sigs, ids):
    """(rows, winners, scores) as bytes, int16 and float64 reads as two device batches."""
    out = []
    for dt in (np.int16, np.float64):
        part = [s for s in sigs if s.dtype == dt]
        rows, win, sc = ctx.scan_batch_reads(part, ids, MIN_SCORE, scores=True)
        out.append((rows.tobytes(), win.tobytes(), sc.tobytes()))
    return out


def test_every_route_gives_the_same_scan(counter, reads, expected):
    from strique_amd import ffi
    sigs = [sig for _, sig in reads]
    ids = [counter._classifier_for(t, s).target_id for t, s in CANDIDATES]
    base = _raw_scan(counter.ctx, sigs, ids)
    # the raw rows: the four positions of every winner (int16 and float64 reads) are the oracle's for that candidate
    n_win = 0
    for dt, (rows, win, _) in zip((np.int16, np.float64), base):
        rows = np.frombuffer(rows, ffi.RESULT_DTYPE); win = np.frombuffer(win, np.int32)
        exp = [e for (_, sig), e in zip(reads, expected) if sig.dtype == dt]
        assert len(rows) == len(win) == len(exp)
        for r, w, (_, geo) in zip(rows, win, exp):
            if w >= 0:
                assert (int(r["prefix_begin"]), int(r["prefix_end"]), int(r["suffix_begin"]), int(r["suffix_end"])) == tuple(geo[int(w)])
                n_win += 1
    assert n_win >= 20
    for key, value in (("STRQ_SERIAL", "1"), ("STRQ_SCREEN_MODE", "fine"), ("STRQ_NO_SCREEN", "1"), ("STRQ_SUBBATCH_READS", "5")):
        counter.ctx.set_option(key, value)
        try:
            got = _raw_scan(counter.ctx, sigs, ids)
        finally:
            counter.ctx.set_option(key, "")
        assert got == base, key


def test_work_done_and_resident_form(counter, reads, expected):
    """2 * n_cand alignments per read; only the winners' windows are decoded; the resident form gives the same rows."""
    sigs = [sig for _, sig in reads if sig.dtype == np.int16]
    ids = [counter._classifier_for(t, s).target_id for t, s in CANDIDATES]
    ctx = counter.ctx
    rows, win, sc = ctx.scan_batch_reads(sigs, ids, MIN_SCORE, scores=True)
    cnt = ctx.last_counters()
    assert cnt[2] == 2 * len(ids) * len(sigs)
    decoded = [r for r, w in zip(rows, win) if w >= 0]
    assert 0 < len(decoded) < len(sigs)
    # strq_last_counters[7]: observations handed to the Viterbi launches -- the winners' windows and nothing else
    assert cnt[7] == sum(int(r["suffix_end"] - r["prefix_begin"]) for r in decoded)
    # the four positions of every winner's row are the oracle's for that candidate
    exp = [e for (_, sig), e in zip(reads, expected) if sig.dtype == np.int16]
    for r, w, (_, geo) in zip(rows, win, exp):
        if w >= 0:
            assert (int(r["prefix_begin"]), int(r["prefix_end"]), int(r["suffix_begin"]), int(r["suffix_end"])) == tuple(geo[int(w)])
            assert int(r["offset"]) == geo[int(w)][1] and int(r["ticks"]) == max(geo[int(w)][2] - geo[int(w)][1], 0)
    assert all(r.tobytes() == np.zeros(1, rows.dtype)[0].tobytes() for r, w in zip(rows, win) if w < 0)
    # resident: upload with any target id, scan set, run, fetch
    off = np.zeros(len(sigs) + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sigs])
    ctx.batch_upload(np.concatenate(sigs), off, [ids[3]] * len(sigs))
    ctx.scan_set(ids, MIN_SCORE)
    try:
        ctx.batch_run()
        assert ctx.last_counters()[2] == 2 * len(ids) * len(sigs)
        rwin, rsc = ctx.batch_fetch_scan(scores=True)
        assert ctx.batch_fetch().tobytes() == rows.tobytes() and rwin.tobytes() == win.tobytes() and rsc.tobytes() == sc.tobytes()
        ctx.batch_run_range(2, 9)
        assert ctx.batch_fetch_range(2, 9).tobytes() == rows[2:9].tobytes()
        # like the rows, winners and scores of reads outside the range stay those of the run that covered them
        rwin, rsc = ctx.batch_fetch_scan(scores=True)
        assert ctx.batch_fetch().tobytes() == rows.tobytes() and rwin.tobytes() == win.tobytes() and rsc.tobytes() == sc.tobytes()
    finally:
        ctx.scan_clear()
    # the same resident batch without the scan set: a plain detect with the targets given at upload
    ctx.batch_run()
    plain = ctx.batch_fetch()
    want = ctx.detect_batch_reads(sigs, [ids[3]] * len(sigs))
    assert plain.tobytes() == want.tobytes()
    with pytest.raises(Exception):
        ctx.batch_fetch_scan()


def test_bad_arguments(counter, reads):
    from strique_amd import ffi
    sigs = [reads[0][1]]
    ids = [counter._classifier_for(t, s).target_id for t, s in CANDIDATES]
    for cand, ms in (([], 5.0), ([ids[0], 9999], 5.0), ([-1], 5.0), (ids, 0.0), (ids, -3.0), (ids, float("nan"))):
        with pytest.raises(ffi.StriqueHipError) as e:
            counter.ctx.scan_batch_reads(sigs, cand, ms)
        assert e.value.code == ffi.STRQ_ERR_ARG
        with pytest.raises(ffi.StriqueHipError) as e:
            counter.ctx.scan_set(cand, ms)
        assert e.value.code == ffi.STRQ_ERR_ARG
    # no default threshold
    with pytest.raises(ValueError):
        counter.scan_batch(sigs)
    with pytest.raises(ValueError):
        counter.scan_batch(sigs, min_score=0)
    # degenerate, featureless, tiny and empty reads: no winner, and the batch goes through
    bad = [np.full(5000, 300, np.int16), np.random.default_rng(3).integers(200, 800, 6000).astype(np.int16),
           np.array([300, 310, 305], np.int16), np.zeros(0, np.int16)]
    got = counter.scan_batch(bad + sigs, min_score=MIN_SCORE)
    assert got[:4] == [None] * 4 and got[4] is not None


def test_detect_and_scan_on_one_context(counter, reads):
    sigs = [sig for _, sig in reads][:8]
    items = [(t[0], sig, t[1]) for t, sig in reads[:8]]
    from strique_amd.counter import repeatCounter
    scan_alone = counter.scan_batch(sigs, min_score=MIN_SCORE)
    detect_alone = counter.detect_batch(items)
    assert counter.scan_batch(sigs, min_score=MIN_SCORE) == scan_alone          # a scan after a plain detect
    assert counter.detect_batch(items) == detect_alone                          # a plain detect after a scan
    assert counter.detect_batch(items[::-1]) == detect_alone[::-1]
    assert counter.scan_batch(sigs[::-1], min_score=MIN_SCORE) == scan_alone[::-1]


def test_count_scan_on_the_bundled_read(workdir):
    """`count --scan` on tests/golden/c9orf72.fast5: the one TSV row is byte-equal to the row `count` writes with the bundled
    SAM; two ranks write the same files."""
    from strique_amd import cli, scan
    from test_cli_end_to_end import _index
    fofn = workdir / "data" / "reads.fofn"
    fofn.write_text(_index(workdir))
    base = [str(fofn), str(workdir / "r9_4_450bps.model"), str(workdir / "repeat_config.tsv"), "--config", str(workdir / "STRique.json")]
    plain, scanned, scores = workdir / "plain.tsv", workdir / "scan.tsv", workdir / "scores.tsv"
    cli.main(["count"] + base + ["--algn", str(workdir / "data" / "c9orf72.sam"), "--out", str(plain)])
    cli.main(["count"] + base + ["--scan", "--scan-min-score", str(MIN_SCORE), "--scan-scores", str(scores), "--out", str(scanned)])
    assert len(plain.read_text().splitlines()) == 2
    assert scanned.read_bytes() == plain.read_bytes()
    cands, rows = scan.parse_scores(open(scores))
    assert cands == CANDIDATES and len(rows) == 1
    rid, target, strand = plain.read_text().splitlines()[1].split("\t")[:3]
    assert rows[0][0] == rid and rows[0][1] == (target, strand) == ("c9orf72", "-")
    sp, ss = plain.read_text().splitlines()[1].split("\t")[4:6]
    assert (repr(rows[0][2][1][0]), repr(rows[0][2][1][1])) == (sp, ss)
    two, scores2 = workdir / "two.tsv", workdir / "scores2.tsv"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29551", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "STRique.py"), "count"] + base + [
        "--scan", "--scan-min-score", str(MIN_SCORE), "--scan-scores", str(scores2), "--out", str(two), "--backend", "gloo", "--share-device"]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert two.read_bytes() == plain.read_bytes() and scores2.read_bytes() == scores.read_bytes()


from test_cli_end_to_end import workdir  # noqa: E402,F401  (the bundled fast5 / SAM / model files in a temporary directory)
