"""Scan on the host: the rule (strique_amd.scan.select), the oracle scan -- the oracle's detect() geometry for every candidate,
then select -- on reads whose target and strand are known, and the surface of `count --scan`."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, oracle_map, oracle_tc

# the four candidates of the bundled repeat_config.tsv, in add_target order, '+' before '-'
CANDIDATES = [("c9orf72", "+"), ("c9orf72", "-"), ("fmr1", "+"), ("fmr1", "-")]
MIN_SCORE = 5.0


def oracle_candidates(orc, opm, cfg, tcs, sig):
    """(scores, geometry) of one read for the oracle classifiers `tcs`: detect()'s conditioning and its two __detect_range__
    calls per candidate (oracle/strique_oracle.py: detect, lines 283-287) -- the conditioning once, it does not depend on the
    candidate."""
    morph = orc.condition(np.asarray(sig), opm)[2]
    params = orc.align_params(cfg["align"])
    scores, geometry = [], []
    for tc in tcs:
        sp, pb, pe = orc.detect_range(morph, tc["prefix_ext"], params, pre_trim=len(tc["prefix_ext"]) - len(tc["prefix"]))
        ss, sb, se = orc.detect_range(morph, tc["suffix_ext"], params, post_trim=len(tc["suffix_ext"]) - len(tc["suffix"]))
        scores.append((sp, ss)); geometry.append((pb, pe, sb, se))
    return scores, geometry


def oracle_scan(orc, opm, cfg, targets, sigs, candidates=CANDIDATES):
    """[(scores, geometry)] per read, on a few threads (the oracle's DP releases the interpreter lock)."""
    tcs = [oracle_tc(orc, opm, targets, n, s, cfg["HMM"]) for n, s in candidates]
    return oracle_map(lambda sig: oracle_candidates(orc, opm, cfg, tcs, sig), sigs)


def table_reads(pm, targets):
    """The three clean reads of the kind the threshold table of DESIGN.md starts from: 8000 nt, 30 repeats."""
    from strique_amd import synth
    table = synth.KmerTable(pm)
    out = []
    for k, (name, strand) in enumerate((("c9orf72", "+"), ("c9orf72", "-"), ("fmr1", "+"))):
        out.append((name, strand, synth.make_read(table, 31, k, 8000, targets[name], 30, strand=strand)[0]))
    return out


def bundled_read():
    z = np.load(os.path.join(GOLDEN, "bundled_read.npz"))
    return "c9orf72", "-", z["signal"]


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def test_select_rule():
    from strique_amd.scan import select
    geo = (100, 900, 5000, 5800)
    assert select([(9.0, 7.0), (3.0, 3.5)], [geo, geo], 5.0) == 0
    assert select([(3.0, 3.5), (9.0, 7.0)], [geo, geo], 5.0) == 1
    # the key is the smaller of the two scores
    assert select([(20.0, 5.5), (6.0, 6.0)], [geo, geo], 5.0) == 1
    # a tie goes to the lower position
    assert select([(4.0, 4.0), (7.0, 8.0), (8.0, 7.0), (7.0, 7.0)], [geo] * 4, 5.0) == 1
    # prefix_begin >= suffix_end: not eligible whatever the scores
    assert select([(50.0, 50.0), (6.0, 6.0)], [(5800, 6000, 50, 100), geo], 5.0) == 1
    assert select([(50.0, 50.0)], [(700, 900, 650, 700)], 5.0) == -1
    # a key exactly equal to min_score is eligible, the next float below is not
    assert select([(5.0, 9.0)], [geo], 5.0) == 0
    assert select([(np.nextafter(5.0, 0.0), 9.0)], [geo], 5.0) == -1
    # no winner; NaN is never eligible; no candidates
    assert select([(4.9, 9.0), (9.0, 0.0)], [geo, geo], 5.0) == -1
    assert select([(float("nan"), 9.0), (9.0, float("nan"))], [geo, geo], 5.0) == -1
    assert select([], [], 5.0) == -1
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            select([(9.0, 9.0)], [geo], bad)


# ---- the oracle scan ---------------------------------------------------------------------------------------------------------
def test_oracle_scan_finds_target_and_strand(pm, cfg, orc, opm, targets):
    """The winner is the true (target, strand) on clean reads at min_score 5.0, and the winner's scores are those of the oracle's
    detect() for that candidate.  The same on the bundled real read: none of its three wrong candidates is eligible at 5.0 (the
    largest of their keys is 3.71: DESIGN.md, "Scan")."""
    from strique_amd.scan import key, select
    reads = table_reads(pm, targets) + [bundled_read()]
    got = oracle_scan(orc, opm, cfg, targets, [sig for _, _, sig in reads])
    for (name, strand, sig), (scores, geometry) in zip(reads, got):
        true = CANDIDATES.index((name, strand))
        keys = [key(*s) for s in scores]
        print(name, strand, len(sig), ["%.3f/%.3f" % s for s in scores], geometry)
        assert max(range(len(keys)), key=lambda c: keys[c]) == true
        assert select(scores, geometry, MIN_SCORE) == true, (name, strand, scores)
        res, info = orc.detect(sig, oracle_tc(orc, opm, targets, name, strand, cfg["HMM"]), opm, orc.align_params(cfg["align"]))
        assert (res[1], res[2]) == scores[true]
        assert (info["prefix_begin"], info["prefix_end"], info["suffix_begin"], info["suffix_end"]) == geometry[true]
        assert res[0] > 0


# ---- the surface -------------------------------------------------------------------------------------------------------------
def _count_args(tmp_path):
    for name in ("reads.fofn", "model"):
        (tmp_path / name).write_text("")
    tsv = tmp_path / "repeat_config.tsv"
    tsv.write_text("chr\tbegin\tend\tname\trepeat\tprefix\tsuffix\n")
    return [str(tmp_path / "reads.fofn"), str(tmp_path / "model"), str(tsv)]


def test_scan_and_algn_exclude_each_other(tmp_path, capsys):
    from strique_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["count"] + _count_args(tmp_path) + ["--scan", "--algn", "x"])
    assert e.value.code == 2 and "--scan" in capsys.readouterr().err
    # the scan options need --scan
    with pytest.raises(SystemExit) as e:
        cli.main(["count"] + _count_args(tmp_path) + ["--scan-scores", "s.tsv"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        cli.main(["count"] + _count_args(tmp_path) + ["--scan", "--scan-min-score", "0"])
    assert e.value.code == 2
    # no default threshold: --scan alone is an error that names the option
    with pytest.raises(SystemExit) as e:
        cli.main(["count"] + _count_args(tmp_path) + ["--scan"])
    assert e.value.code == 2 and "--scan-min-score" in capsys.readouterr().err


def test_scan_scores_file_round_trips():
    import io
    from strique_amd import scan
    cands = CANDIDATES
    rows = [("read-1", ("c9orf72", "-"), [(3.25, 2.0), (6.3155927807600545, 6.031860427335506), (0.0, 3.9), (1e-3, 4.07)]),
            ("read-2", None, [(3.0, 2.0), (0.1 + 0.2, 1.0 / 3.0), (0.0, 0.0), (2.5, 4.0)])]
    text = "\t".join(scan.scores_header(cands)) + "\n" + "".join(scan.format_scores(*r) + "\n" for r in rows)
    assert text.splitlines()[0].split("\t")[:5] == ["ID", "winner_target", "winner_strand", "c9orf72+:score_prefix", "c9orf72+:score_suffix"]
    got_cands, got_rows = scan.parse_scores(io.StringIO(text))
    assert got_cands == cands and got_rows == rows          # repr(): every float64 comes back bit for bit
    with pytest.raises(ValueError):
        scan.parse_scores(io.StringIO("ID\ttarget\n"))


def test_scan_symbols_are_declared():
    from strique_amd import ffi, scan
    header = open(os.path.join(ROOT, "include", "strique_hip.h")).read()
    for name in ("strq_scan_batch_reads", "strq_scan_set", "strq_scan_clear", "strq_batch_fetch_scan"):
        assert "int %s(" % name in header and name in ffi.SCAN_SYMBOLS
    for name in ("scan_batch_reads", "scan_set", "scan_clear", "batch_fetch_scan"):
        assert callable(getattr(ffi.Context, name))
    from strique_amd.counter import repeatCounter
    assert callable(repeatCounter.scan_batch) and callable(scan.select)
    assert not hasattr(scan, "DEFAULT_MIN_SCORE")          # wrong and true keys overlap on noisy reads: DESIGN.md, "Scan"
