"""Methylation calls of anchored reads without a GPU: the row format of `count --anchored-mod`, the CLI's argument errors, the rule
"which reads get a call", the CPU preconditions on the very reads the GPU test uses (tests/test_gpu_anchored_mod.py) -- the seed
of tests/anchored_mod_ref.py was chosen so that the oracle alone meets them -- and the plumbing with a stubbed counter."""
import io

import numpy as np
import pytest

import anchored_mod_ref as amr
import anchored_ref as ar
from test_anchored_host import AnchoredCounter
from test_mod_llr_host import OneRank

REC = (2, 0, 42, -4229.255537715763, 10137, 12060, 25)
# (record, call): every kind, every status, a pattern without a path, one without units, ratios with an infinity
ROWS = [(REC, ("0110", np.array([-1.25, 3.5, float("inf"), -0.00004]))), (REC, ("0110", None)), ((3, 0, 7, -1.5, 0, 300, 2), ("-", None)),
        ((3, 0, 7, -1.5, 0, 300, 2), ("", None)), ((2, 1, 0, 0.0, 0, 0, 0), None), ((3, 2, 0, 0.0, 0, 0, 0), None), ((1, 0, 0, 0.0, 0, 0, 0), None),
        ((0, 0, 0, 0.0, 0, 0, 0), None), (None, None)]


def test_format_parse_round_trip():
    from strique_amd import anchored as an
    assert an.MOD_HEADER == ["ID", "target", "strand", "kind", "count", "mod_pattern", "n_units", "llr"]
    text = "\t".join(an.MOD_HEADER) + "\n" + "".join(an.format_mod_row("read%d" % i, "fmr1", "+-"[i % 2], r, c) + "\n" for i, (r, c) in enumerate(ROWS))
    lines = text.splitlines()
    assert lines[1].split("\t")[3:] == ["ends_in_repeat", "42", "0110", "4", "-1.2500,3.5000,inf,-0.0000"]
    assert lines[2].split("\t")[3:] == ["ends_in_repeat", "42", "0110", "4", "-"]
    rows = an.parse_mod(io.StringIO(text))
    assert len(rows) == len(ROWS)
    for i, ((rec, call), (rid, target, strand, kind, count, got)) in enumerate(zip(ROWS, rows)):
        assert (rid, target, strand) == ("read%d" % i, "fmr1", "+-"[i % 2])
        assert kind == an.KIND_NAMES[0 if rec is None else rec[0]]
        assert count == (rec[2] if rec is not None and rec[0] in (2, 3) and rec[1] == 0 else None)
        if call is None:
            assert got is None and lines[1 + i].split("\t")[5:] == ["-"] * 3          # every field without a value is '-'
        elif call[0] in ("-", ""):
            assert got == ("-", 0, None)
        else:
            assert got[0] == call[0] and got[1] == len(call[0])
            assert got[2] is None if call[1] is None else got[2] == [float("%.4f" % x) for x in call[1]]
    with pytest.raises(ValueError):
        an.parse_mod(io.StringIO("\t".join(an.HEADER) + "\n"))                          # the --anchored file is another file
    with pytest.raises(ValueError):
        an.parse_mod(io.StringIO("\t".join(an.MOD_HEADER) + "\nr\tt\t+\tends_in_repeat\t3\t010\t3\t0.5,0.5\n"))
    with pytest.raises(ValueError):
        an.format_mod_row("r", "t", "+", REC, ("010", [0.5]))


def test_rule():
    from strique_amd import anchored as an
    ok = (2, 0, 5, -1.0, 10, 20, 3)
    assert an.gets_mod_call(ok, True) and an.gets_mod_call((3,) + ok[1:], True)
    assert not an.gets_mod_call(ok, False)                                              # a target without a modification model
    assert not an.gets_mod_call((1, 0, 0, 0.0, 0, 0, 0), True)                          # spanning: the row has the pattern
    assert not an.gets_mod_call((0, 0, 0, 0.0, 0, 0, 0), True)
    assert not an.gets_mod_call((2, 1, 0, 0.0, 0, 0, 0), True) and not an.gets_mod_call((3, 2, 0, 0.0, 0, 0, 0), True)
    assert not an.gets_mod_call((2, 0, 0, -1.0, 10, 10, 0), True)                       # begin < end
    assert not an.gets_mod_call(None, True)
    for kind in range(4):
        for status in range(3):
            for b, e in ((0, 0), (5, 9), (9, 5)):
                for has in (True, False):
                    rec = (kind, status, 1, -1.0, b, e, 0)
                    assert an.gets_mod_call(rec, has) == amr.qualifies(rec, has), (rec, has)


# ---- preconditions on the shared reads (conditions, not measurements: the seed was chosen so that the oracle meets them) ---------
def test_cpu_preconditions_on_the_shared_reads(tables, cfg):
    got = amr.cases(tables, cfg, True)
    assert len(got) == 2 * 2 * 7 * 2
    ones = {"base": [0, 0], "mod": [0, 0]}
    for c in got:
        what = (c["target"], c["strand"], c["cut"], c["table"], c["rec"])
        assert (c["call"] is not None) == amr.qualifies(c["rec"]), what
        if c["call"] is not None:
            pattern, V, x = c["call"]
            assert set(pattern) <= set("01") or pattern == "-", what
            assert V.shape == ((0 if pattern == "-" else len(pattern)), 2), what
        if c["cut"] in amr.MID_CUTS:
            assert amr.qualifies(c["rec"]) and c["rec"][0] == c["kind"], what
            pattern = c["call"][0]
            assert pattern != "-" and len(pattern) > 0, what
            ones[c["table"]][0] += pattern.count("1"); ones[c["table"]][1] += len(pattern)
    # a sanity condition on the inputs, not a claim about the product
    print("share of '1' by table:", {k: v[0] / v[1] for k, v in ones.items()})
    assert ones["mod"][0] / ones["mod"][1] > ones["base"][0] / ones["base"][1]
    # every case the rule turns away is among the shared reads or the GPU test's mixed batch; here: kind 0
    assert sum(1 for c in got if c["call"] is None) >= 1 and sum(1 for c in got if c["call"] is not None) >= 50
    # zero-unit stretches are there
    assert any(c["cut"] in ("in_prefix", "one_base_in") and c["call"] is not None and len(c["call"][0]) <= 1 for c in got)


def test_boundary_tie_stays_within_the_exemption(pm, tables, cfg):
    """The k-mer tie at the repeat boundary: where the anchored decode has two best paths, the order a model lists its in-edges in
    decides where the stretch begins, and that order differs between the oracle's un-baked graph and baked arrays.  Decoding the
    shared reads with the oracle's Viterbi on the baked arrays of the product's models (no GPU involved) tells how many of the 56
    reads are affected: the GPU test may exempt the first unit of at most 2."""
    from strique_amd import hmm
    from oracle import strique_oracle as orc
    from conftest import oracle_map
    opm = orc.PoreModel(table=(tables["base_kmer"], tables["base_mean"], tables["base_stdv"]))
    params = orc.align_params(cfg["align"])
    decoded = [c for c in amr.cases(tables, cfg, True) if c["rec"][0] in (ar.ENDS, ar.STARTS) and c["rec"][1] == 0]
    baked = {}
    for c in decoded:
        key = (c["target"], c["strand"], c["rec"][0])
        if key not in baked:
            r, p, s, _, _ = ar.strand_sequences(*cfg["repeat"][c["target"]][3:6], c["strand"])
            baked[key] = hmm.AnchoredRepeatModel("ends_in_repeat" if key[2] == ar.ENDS else "starts_in_repeat", r, p, s, pm, cfg["HMM"]).baked

    def stretch(c):
        """[begin, end) of the read's repeat section as the baked arrays decode its window"""
        sig = np.asarray(c["sig"])
        _, info = orc.detect(sig, c["tc"], opm, params)
        w0, w1 = (info["prefix_begin"], len(sig)) if c["rec"][0] == ar.ENDS else (0, info["suffix_end"])
        b = baked[(c["target"], c["strand"], c["rec"][0])]
        fltn = opm.normalize_minmax(orc.medfilt3(sig).astype(np.float64))
        _, path, _ = orc.viterbi(b, fltn[w0:w1])
        assert path is not None
        tagged = np.flatnonzero(np.asarray(b.tag)[path] == 1)
        return w0 + int(tagged[0]), w0 + int(tagged[-1]) + 1
    got = oracle_map(stretch, decoded)
    moved = [(c["target"], c["strand"], c["cut"], c["table"], g, c["rec"][4:6]) for c, g in zip(decoded, got) if tuple(g) != tuple(c["rec"][4:6])]
    print("reads whose stretch depends on the in-edge order:", moved)
    assert len(decoded) >= 50 and len(moved) <= 2


# ---- blob, run_count, CLI ----------------------------------------------------------------------------------------------------------
def test_blob_carries_record_and_call():
    from strique_amd import cli
    names = [o.name for o in cli.OUTPUTS]
    assert "anchored_mod" in names and names[-1] == "anchored" and cli.Merged(None, None, None, None, None).anchored_mod is None
    assert cli.Detected((0,), None, None, None).anchored_mod is None
    on = cli.outputs_on(anchored=True, anchored_mod=True)
    assert [o.name for o in on] == ["anchored_mod", "anchored"]
    for rec, call in ROWS:
        blob = cli.pack_blob(on, "fmr1", "-", "-", dict(anchored=rec, anchored_mod=(rec, call)))
        assert blob.count("\t") == 2 + len(cli.OUTPUTS)
        got = cli.unpack_blob(on, blob)[3]
        assert got["anchored"] == rec
        grec, gcall = got["anchored_mod"] or (None, None)
        assert grec == rec and (gcall is None) == (call is None)
        if call is not None:
            assert gcall[0] == call[0]
            assert gcall[1] is None if call[1] is None else np.array(gcall[1]).tobytes() == np.asarray(call[1], np.float64).tobytes()
    off = cli.outputs_on(anchored=True)
    assert cli.unpack_blob(off, cli.pack_blob(off, "fmr1", "-", "-", dict(anchored_mod=ROWS[0])))[3]["anchored_mod"] is None


class AnchoredModCounter(AnchoredCounter):
    """AnchoredCounter that also answers set_anchored_mod: the call depends on the inputs only."""

    def __init__(self):
        self.on = False

    def set_anchored_mod(self, on):
        self.on = bool(on)

    def detect_batch(self, items, mod_llr=False, **kw):
        out = AnchoredCounter.detect_batch(self, items, mod_llr=mod_llr, **kw)
        if not self.on:
            return out
        got = []
        for (t, raw, s), d in zip(items, out):
            call = None
            if d.anchored[0] in (2, 3) and d.anchored[1] == 0:
                n = len(raw) % 4
                call = ("01"[len(raw) % 2] * n if len(raw) % 9 else "-", (np.arange(n) / 3.0 - 0.5) if mod_llr and n and len(raw) % 9 else None)
            got.append(d._replace(anchored_mod=call))
        return got

    def detect(self, t, raw, s, **kw):
        return self.detect_batch([(t, raw, s)], **kw)[0]


@pytest.mark.parametrize("mod_llr", [False, True])
def test_count_rows_with_a_stubbed_counter(cfg, mod_llr):
    """FILE2 next to the count rows: one row per count row, single process and through the blob of the gather; the count TSV, the
    anchored file and the ratio file byte-identical with and without the switch."""
    from strique_amd import anchored as an, cli
    loci = {}
    for name, (chrom, b, e, *_r) in cfg["repeat"].items():
        loci.setdefault(chrom, []).append((name, b, e))
    lines = ["@HD\tVN:1.0"]
    for i in range(23):
        chrom, pos = ("chr9", 27570000) if i % 3 else ("chrX", 146990000)
        lines.append("\t".join(["read%d" % i, "16" if i % 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))
    get_raw = lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))
    log = cli.Log("error")

    def run(counter, **more):
        f = {k: io.StringIO() for k in ("rows", "mod_llr", "anchored", "anchored_mod")}
        cli.run_count(iter(lines), loci, get_raw, counter, log, 4, 0, 1, f["rows"], mod_llr=mod_llr, llr_out=f["mod_llr"] if mod_llr else None,
                      anchored=6.5, anchored_out=f["anchored"], **more)
        return {k: v.getvalue() for k, v in f.items()}
    off = run(AnchoredModCounter())
    on = run(AnchoredModCounter(), anchored_mod=True, anchored_mod_out=None)
    with_file = io.StringIO()
    full = run(AnchoredModCounter(), anchored_mod=True, anchored_mod_out=with_file)
    for name in ("rows", "mod_llr", "anchored"):
        assert off[name] == on[name] == full[name], name
    rows = an.parse_mod(io.StringIO(with_file.getvalue()))
    count_rows = [l.split("\t") for l in off["rows"].splitlines()[1:]]
    anch_rows = an.parse(io.StringIO(off["anchored"]))
    assert [(r[0], r[1], r[2]) for r in rows] == [tuple(c[:3]) for c in count_rows] and len(rows) == 23
    assert [(r[3], r[4]) for r in rows] == [(a[3], None if a[4] is None else a[4][0]) for a in anch_rows]
    assert any(r[5] is not None and r[5][2] is not None for r in rows) == mod_llr and any(r[5] is not None for r in rows) and any(r[5] is None for r in rows)
    assert all(r[5] is None for r in rows if r[3] in ("none", "spanning"))
    # two ranks, one gather: the same bytes
    stats = {}
    parts = [cli.run_count(iter(lines), loci, get_raw, AnchoredModCounter(), log, 4, rank, 2, stats=stats if rank == 0 else {}, anchored=6.5, anchored_mod=True,
                           mod_llr=mod_llr) for rank in (0, 1)]
    merged = cli.gather_rows(parts[1] + parts[0], stats["items"], OneRank, anchored=True, anchored_mod=True, mod_llr=mod_llr)
    text = lambda rows_, header: (lambda b: (cli.write_rows(b, rows_, header=header), b.getvalue())[1])(io.StringIO())
    assert text(merged.rows, True) == off["rows"]
    assert text(merged.anchored, an.HEADER) == off["anchored"]
    assert text(merged.anchored_mod, an.MOD_HEADER) == with_file.getvalue()
    with pytest.raises(ValueError):
        cli.run_count(iter(lines), loci, get_raw, AnchoredModCounter(), log, 4, 0, 1, io.StringIO(), anchored_mod=True)


def test_the_counter_switch():
    """anchored_mod is a switch of the counter (set_anchored_mod), like set_variants: detect and detect_batch keep the keywords
    every stand-in counter of run_count answers; without a modification model, and without anchored=m, it is an error."""
    import inspect
    from strique_amd.counter import Detected, repeatCounter
    assert "anchored_mod" in Detected._fields and callable(repeatCounter.set_anchored_mod)
    assert "anchored_mod" not in inspect.signature(repeatCounter.detect).parameters

    class NoDevice(repeatCounter):
        def __init__(self, with_mod):
            self.pm = object(); self.pm_mod = object() if with_mod else self.pm
            self.anchored_mod = False; self.variants = False; self.renorm = None
    with pytest.raises(ValueError) as e:
        NoDevice(False).set_anchored_mod(True)
    assert "modification model" in str(e.value)
    c = NoDevice(True)
    c.set_anchored_mod(True)
    with pytest.raises(ValueError) as e:
        c.detect_batch([], anchored=None)
    assert "anchored=m" in str(e.value)


@pytest.mark.parametrize("argv,needle", [
    (["--mod_model", "m.model", "--anchored-mod", "b.tsv"], "needs --anchored"),
    (["--anchored", "a.tsv", "--anchored-min-score", "6.5", "--anchored-mod", "b.tsv"], "--mod_model"),
    (["--mod_model", "m.model", "--anchored", "a.tsv", "--anchored-min-score", "6.5", "--anchored-mod", "b.tsv", "--scan", "--scan-min-score", "5"], "--scan"),
])
def test_argument_errors(capsys, argv, needle):
    from strique_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.count(["reads.fofn", "r9.model", "repeats.tsv"] + argv)
    assert e.value.code == 2
    assert needle in capsys.readouterr().err
