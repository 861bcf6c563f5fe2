"""What `count` and run_count refuse, without a GPU: every argument error of count() with its full text, the keywords run_count takes,
the counter switch a run turns on and off again, and the two tables -- the outputs of the CLI and the passes of the counter --
naming the same things."""
import io

import numpy as np
import pytest

from test_anchored_mod_host import AnchoredModCounter

MOD = ["--mod_model", "m.model"]
SCAN = ["--scan", "--scan-min-score", "5"]
ANCHORED = ["--anchored", "a.tsv", "--anchored-min-score", "6.5"]
ALIGNED = "pass runs on reads whose target and strand an alignment gives"
BOTH_FLANKS = "a scan takes a read for a target when it finds both flanks"

ERRORS = [
    (SCAN + ["--confidence", "c.tsv"], "--confidence cannot be combined with --scan: the forward " + ALIGNED),
    (["--mod-llr", "l.tsv"], "--mod-llr needs --mod_model: the ratios belong to the calls of the modification model"),
    (MOD + SCAN + ["--mod-llr", "l.tsv"], "--mod-llr cannot be combined with --scan: the scoring " + ALIGNED),
    (["--variants", "v.tsv"], "--variants needs --alt-units FILE: the units to tell from the repeat unit"),
    (SCAN + ["--alt-units", "alt.tsv", "--variants", "v.tsv"], "--variants cannot be combined with --scan: the variant " + ALIGNED),
    (["--tracts", "t.tsv"], "--tract-units FILE and --tracts FILE need each other: the definitions, and where the counts go"),
    (["--tract-units", "u.tsv"], "--tract-units FILE and --tracts FILE need each other: the definitions, and where the counts go"),
    (SCAN + ["--tract-units", "u.tsv", "--tracts", "t.tsv"], "--tracts cannot be combined with --scan: the tract " + ALIGNED),
    (SCAN + ["--algn", "reads.sam"], "--scan takes the target and strand of a read from its signal: it cannot be combined with --algn"),
    (["--scan-scores", "s.tsv"], "--scan-min-score and --scan-scores need --scan"),
    (["--scan-min-score", "5"], "--scan-min-score and --scan-scores need --scan"),
    (["--scan"], "--scan needs --scan-min-score X: the scores of wrong and of true candidates overlap on noisy reads, so there is no default "
                 "(a first run with a high X and --scan-scores FILE shows what to choose from)"),
    (["--scan", "--scan-min-score", "0"], "--scan-min-score must be above 0"),
    (["--scan", "--scan-min-score", "-3"], "--scan-min-score must be above 0"),
    (SCAN + ANCHORED, "--anchored cannot be combined with --scan: " + BOTH_FLANKS),
    (["--anchored", "a.tsv"], "--anchored needs --anchored-min-score X: the scores of a flank that is there and of one that is not overlap on noisy reads, "
                              "so there is no default"),
    (["--anchored-min-score", "6.5"], "--anchored-min-score needs --anchored FILE"),
    (["--anchored", "a.tsv", "--anchored-min-score", "0"], "--anchored-min-score must be above 0"),
    (MOD + ["--anchored-mod", "b.tsv"], "--anchored-mod needs --anchored FILE --anchored-min-score X: the calls are made on the reads anchored counting finds"),
    (ANCHORED + ["--anchored-mod", "b.tsv"], "--anchored-mod needs --mod_model: the calls are those of the modification model"),
    (MOD + SCAN + ANCHORED + ["--anchored-mod", "b.tsv"], "--anchored-mod cannot be combined with --scan: " + BOTH_FLANKS),
    (["--flank-mod", "f.tsv"], "--flank-mod needs --mod_model: the calls compare the modification model's k-mer table with the base table"),
    (MOD + SCAN + ["--flank-mod", "f.tsv"], "--flank-mod cannot be combined with --scan: the flank " + ALIGNED),
    (["--renorm", "0"], "--renorm MIN_SHARE must be inside (0, 1)"),
    (["--renorm", "1"], "--renorm MIN_SHARE must be inside (0, 1)"),
    (["--renorm-out", "r.tsv"], "--renorm-out needs --renorm MIN_SHARE"),
    (SCAN + ["--renorm", "0.4"], "--renorm cannot be combined with --scan: the fit needs the target of a read, which a scan finds with the maps as they are"),
]

# Two mistakes in one command line: the checks of single arguments come first, in the order they are written in; then, output by
# output in the order of OUTPUTS, --mod_model before --scan.  Before the checks moved into OUTPUTS they stood output by output in the
# order the arguments were added in, so five command lines here (and the anchored_mod / scan line above, whose message nothing could
# reach) named their other mistake then: --confidence, --confidence, --anchored with --scan, --tracts, --variants in the order below.
PRECEDENCE = [
    (SCAN + ["--confidence", "c.tsv", "--algn", "reads.sam"], "--scan takes the target and strand of a read from its signal: it cannot be combined with --algn"),
    (["--scan", "--confidence", "c.tsv"], ERRORS[11][1]),                                        # --scan needs --scan-min-score X
    (SCAN + ["--anchored", "a.tsv"], ERRORS[15][1]),                                             # --anchored needs --anchored-min-score X
    (SCAN + ["--variants", "v.tsv"], "--variants needs --alt-units FILE: the units to tell from the repeat unit"),
    (SCAN + ["--anchored-mod", "b.tsv"], ERRORS[18][1]),                                         # --anchored-mod needs --anchored FILE ...
    (SCAN + ["--mod-llr", "l.tsv"], "--mod-llr needs --mod_model: the ratios belong to the calls of the modification model"),
    (SCAN + ["--flank-mod", "f.tsv", "--confidence", "c.tsv"], "--confidence cannot be combined with --scan: the forward " + ALIGNED),
    (MOD + SCAN + ["--tract-units", "u.tsv", "--tracts", "t.tsv", "--flank-mod", "f.tsv"], "--flank-mod cannot be combined with --scan: the flank " + ALIGNED),
    (SCAN + ["--renorm", "0.4", "--alt-units", "alt.tsv", "--variants", "v.tsv"], ERRORS[-1][1]),   # renorm stands in front of variants
]


def test_the_precedence_cases_name_what_they_mean():
    assert ERRORS[11][1].startswith("--scan needs --scan-min-score X") and ERRORS[15][1].startswith("--anchored needs --anchored-min-score X")
    assert ERRORS[18][1].startswith("--anchored-mod needs --anchored FILE") and ERRORS[-1][1].startswith("--renorm cannot be combined with --scan")
    assert len({m for _, m in ERRORS}) == 23                         # every parser.error of count() is reached


@pytest.mark.parametrize("argv,message", ERRORS + PRECEDENCE, ids=[" ".join(a) for a, _ in ERRORS + PRECEDENCE])
def test_argument_errors(capsys, argv, message):
    """Every parser.error of count(): exit status 2 and the whole message, before any file is looked at."""
    from strique_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.count(["reads.fofn", "r9.model", "repeats.tsv"] + argv)
    assert e.value.code == 2
    assert capsys.readouterr().err.endswith(": error: " + message + "\n")


def _input(cfg):
    loci = {}
    for name, (chrom, b, e, *_r) in cfg["repeat"].items():
        loci.setdefault(chrom, []).append((name, b, e))
    lines = ["@HD\tVN:1.0"]
    for i in range(9):
        chrom, pos = ("chr9", 27570000) if i % 3 else ("chrX", 146990000)
        lines.append("\t".join(["read%d" % i, "16" if i % 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))
    return lines, loci, lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))


class SwitchLog(AnchoredModCounter):
    def __init__(self):
        AnchoredModCounter.__init__(self)
        self.switched = []

    def set_anchored_mod(self, on):
        self.switched.append(on)
        AnchoredModCounter.set_anchored_mod(self, on)


def test_run_count_releases_the_anchored_mod_switch(cfg):
    """The switch belongs to the run, like those of variants, renorm, tracts and flank_mod: a later detect_batch on the same counter
    without anchored= must not meet it."""
    from strique_amd import cli
    lines, loci, get_raw = _input(cfg)
    c = SwitchLog()
    side = io.StringIO()
    cli.run_count(iter(lines), loci, get_raw, c, cli.Log("error"), 4, 0, 1, io.StringIO(), anchored=6.5, anchored_mod=True, anchored_mod_out=side)
    assert len(side.getvalue().splitlines()) == 1 + 9
    assert c.switched == [True, False]
    assert c.on is False


def test_run_count_takes_no_unknown_keyword(cfg):
    from strique_amd import cli
    lines, loci, get_raw = _input(cfg)
    for bad in (dict(no_such_out=1), dict(scores=True), dict(units=True, unit_out=io.StringIO())):
        c = SwitchLog()
        with pytest.raises(TypeError):
            cli.run_count(iter(lines), loci, get_raw, c, cli.Log("error"), 4, 0, 1, io.StringIO(), **bad)
        assert c.switched == []
    with pytest.raises(TypeError):
        cli.gather_rows([], [], None, no_such=True)


def test_what_asks_for_an_output(cfg):
    """By truth -- 0 and '' ask for nothing -- but for the outputs whose value says more than yes: an empty {target: alt units} asks
    for variants (and is refused in a scan), and a renorm share of 0.0 is looked at (and refused)."""
    from strique_amd import cli
    lines, loci, get_raw = _input(cfg)
    scan = {"min_score": 5.0, "candidates": [("c9orf72", "+")], "scores": False}
    run = lambda counter, **kw: cli.run_count(iter(lines), loci, get_raw, counter, cli.Log("error"), 4, 0, 1, io.StringIO(), **kw)
    c = SwitchLog()
    stats = {}
    run(c, units=0, confidence="", mod_llr=None, anchored_mod=0, tracts=0, flank_mod="", stats=stats)          # SwitchLog has no set_tracts, no set_flank_mod
    assert c.switched == [] and len(stats["unit_rows"]) == len(stats["tract_rows"]) == len(stats["anchored_mod_rows"]) == 0
    with pytest.raises(ValueError, match="^variants cannot be combined with a scan$"):
        cli.run_count(["read1"], {}, get_raw, SwitchLog(), cli.Log("error"), 4, 0, 1, io.StringIO(), variants={}, scan=scan)
    with pytest.raises(ValueError, match="^the renorm share threshold must be inside"):
        run(SwitchLog(), renorm=0.0)
    with pytest.raises(ValueError, match="^anchored methylation calls need anchored counting$"):
        run(SwitchLog(), anchored_mod=True)


def test_outputs_name_the_passes_of_the_counter():
    """Every output but the scan's score rows is a pass of the counter: same names, and a Detected field behind each."""
    from strique_amd import cli, counter
    passes = {p.name: p for p in counter.PASSES}
    assert [o.name for o in cli.OUTPUTS if o.name not in passes] == ["scores"]
    assert sorted(passes) == sorted(o.name for o in cli.OUTPUTS if o.name != "scores")
    assert sorted(p.field for p in counter.PASSES) == sorted(counter.Detected._fields[1:])
    for o in cli.OUTPUTS:
        if o.name in passes:
            # a keyword of detect_batch is asked for as a keyword, a switch of the counter through its set_ method
            assert (o.ask == "keyword") == passes[o.name].keyword and (o.ask == "switch") == (not passes[o.name].keyword)
            assert callable(getattr(counter.repeatCounter, "set_" + o.name, None)) == (o.ask == "switch")
            assert o.level == passes[o.name].level
