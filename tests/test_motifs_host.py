"""The rule of the motif track on the host (strique_amd/motifs.py) against tests/motif_ref.py: the refusals, the key, both strands,
the loop models to the bit, segment bounds, ties and runs; the library exports the entry; the definition file, the side file's round
trip, the refusals of the command line, the gather through a stand-in counter and the counter's switch through a recording context.
No GPU."""
import ctypes
import math
import os

import numpy as np
import pytest

import motif_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNITS = ["A", "GAA", "AAGGG", "GAAGGA", "ACGTTGCATCAGGATCCATGGTACCAGTTAC"]          # 1, 3, 5, 6 and 31 nt


def test_check_refuses():
    from strique_amd import motifs
    assert motifs.check("aaaag", ["aaagg", "AAGGG"], 6) == ("AAAAG", "AAAGG", "AAGGG")
    assert motifs.check("GAA", "GAAGGA", 6) == ("GAA", "GAAGGA")
    for repeat, alts, word in (("AAAAG", [""], "empty"), ("", ["AAGGG"], "empty"), ("AAAAG", ["AANGG"], "letters"),
                               ("AAAAG", ["AAAGG", "AAGGG", "AGGGG", "GGGGG"], "between 1 and 3"), ("AAAAG", [], "between 1 and 3"),
                               ("AAAAG", [UNITS[-1] + "A"], "emitting states"), ("AAAAG", ["AAAGA"], "same array"),
                               ("GAA", ["GAAGAA"], "same array"), ("AAAAG", ["AAAGG", "GGAAA"], "same array")):
        with pytest.raises(ValueError, match=word):
            motifs.check(repeat, alts, 6)
    assert len(UNITS[-1]) == 31 and motifs.n_emit(UNITS[-1], 6) == 64 and motifs.n_emit(UNITS[-1] + "A", 6) == 66
    for S in (31, 4097, 0):
        with pytest.raises(ValueError, match="segment"):
            motifs.check_segment(S)
    assert motifs.check_segment(32) == 32 and motifs.check_segment(4096) == 4096


def test_key_rotations_and_powers():
    from strique_amd import motifs
    assert motifs.key("AAAAG") == "AAAAG" and motifs.key("AGAAA") == "AAAAG" and motifs.key("GAAAA") == "AAAAG"
    assert motifs.key("GAAGAA") == "AAG" and motifs.key("GAA") == "AAG" and motifs.key("AAAA") == "A"
    assert motifs.key("GAAGGA") == "AAGGAG" and motifs.key("gaagga") == "AAGGAG"
    for u in UNITS + ["TTTCA", "CAGCAG", "ACAC"]:
        assert motifs.key(u) == mr.key(u)
        assert motifs.key(u[2:] + u[:2]) == motifs.key(u) == motifs.key(u * 3)


def test_strands():
    from strique_amd import motifs
    units = ("AAAAG", "AAAGG", "AAGGG")
    assert motifs.strand_units(units, '+') == units
    assert motifs.strand_units(units, '-') == ("CTTTT", "CCTTT", "CCCTT") == tuple(mr.revcomp(u) for u in units)
    with pytest.raises(ValueError):
        motifs.strand_units(units, '?')


def _same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("strand", "+-")
def test_loop_arrays_equal_the_reference(pm, opm, cfg, unit, strand):
    from strique_amd import hmm, motifs
    u = motifs.strand_units((unit,), strand)[0]
    prefix, suffix = (s.upper() for s in cfg["repeat"]["c9orf72"][4:6])
    got = motifs.loop_arrays(hmm.FlankedRepeatModel(u, prefix[-50:], suffix[:50], pm, cfg["HMM"]).baked)
    want = mr.loop(u, opm, cfg["HMM"])
    assert got.silent_start == want.silent_start == motifs.n_emit(u, pm.kmer)
    assert (got.n_states, got.start, got.end) == (want.n_states, want.start, want.end) == (got.silent_start + 2, got.silent_start, got.silent_start + 1)
    assert np.array_equal(got.in_ptr, want.in_ptr) and np.array_equal(got.in_src, want.in_src) and _same_bits(got.in_logp, want.in_logp)
    assert np.array_equal(got.emis_kind, want.emis_kind)
    assert _same_bits(got.emis_a, want.emis_a) and _same_bits(got.emis_b, want.emis_b) and _same_bits(got.emis_c, want.emis_c)
    assert got.names[:got.silent_start] == want.names[:want.silent_start]
    ne = got.silent_start
    assert max(int(got.in_ptr[l + 1] - got.in_ptr[l]) for l in range(ne)) - 1 <= 7          # in-edges from emitting states: the image holds 8
    assert all(got.in_src[got.in_ptr[l + 1] - 1] == got.start and got.in_logp[got.in_ptr[l + 1] - 1] == -math.log(ne) for l in range(ne))
    # the loop does not depend on the flanks
    again = motifs.loop_model(u, pm, cfg["HMM"])
    assert np.array_equal(again.in_src, got.in_src) and _same_bits(again.in_logp, got.in_logp) and _same_bits(again.emis_c, got.emis_c)


def test_the_two_evaluations_agree(opm, cfg):
    rng = np.random.Generator(np.random.PCG64(5))
    for unit in ("A", "GAA", "AAGGG"):
        m = mr.loop(unit, opm, cfg["HMM"])
        for T in (1, 2, 65):
            x = rng.uniform(opm.model_min + 1, opm.model_max - 1, T)
            if T == 65:
                x[[3, 40]] = np.nan
            assert _same_bits(mr.score_a(m, x), mr.score_b(m, x)), (unit, T)
        assert _same_bits(mr.score_a(m, np.full(4, np.nan)), mr.score_b(m, np.full(4, np.nan)))


def test_segment_bounds():
    from strique_amd import motifs
    S = 64
    want = {1: [(0, 1)], S - 1: [(0, S - 1)], S: [(0, S)], S + 1: [(0, S + 1)], 2 * S - 1: [(0, 2 * S - 1)], 2 * S: [(0, S), (S, 2 * S)],
            3 * S + 5: [(0, S), (S, 2 * S), (2 * S, 3 * S + 5)]}
    for T, bounds in want.items():
        assert motifs.segments(T, S) == bounds == mr.segments(T, S), T
    with pytest.raises(ValueError):
        motifs.segments(0, S)
    assert motifs.segments(1000)[-1] == (512, 1000) and len(motifs.segments(1000)) == 3


def test_winner_and_majority_ties_and_runs():
    from strique_amd import motifs
    V = np.array([[-5.0, -5.0, -7.0], [-9.0, -3.0, -3.0], [-np.inf, -np.inf, -np.inf], [-4.0, -8.0, -1.0]])
    win = motifs.winners(V)
    assert list(win) == [0, 1, 0, 2]
    bounds = [(0, 10), (10, 20), (20, 30), (30, 45)]
    m = motifs.margins(V, bounds)
    assert m[0] == 0.0 and m[3] == 3.0 / 15
    s = motifs.summary(win, bounds, 3)
    assert s.obs_won == (20, 10, 15) and s.majority == 0 and s.shares == (20 / 45, 10 / 45, 15 / 45)
    assert motifs.summary([1, 0], [(0, 10), (10, 20)], 2).majority == 0          # a tie goes to the lowest index
    assert motifs.summary([1, 0], [(0, 10), (10, 21)], 2).majority == 0 and motifs.summary([1, 0], [(0, 10), (10, 19)], 2).majority == 1
    assert motifs.runs([0, 0, 1, 1, 0], [(0, 4), (4, 8), (8, 12), (12, 16), (16, 23)], 100) == [(0, 100, 108), (1, 108, 116), (0, 116, 123)]
    assert motifs.runs(win, bounds) == mr.runs([int(w) for w in win], bounds) == [(0, 0, 10), (1, 10, 20), (0, 20, 30), (2, 30, 45)]


def test_library_exports_the_entry_and_refuses_a_null_context():
    from strique_amd import ffi
    lib = ctypes.CDLL(ffi.LIB_PATH)
    assert lib.strq_motif_track(None, ctypes.c_int32(2), None, ctypes.c_int32(64), ctypes.c_int64(0), None, None, ctypes.c_int64(0),
                                None, None, None, None, None) == ffi.STRQ_ERR_ARG
    assert "strq_motif_track" in open(os.path.join(ROOT, "include", "strique_hip.h")).read()


# ---- the definition file, the side file, the command line, the gather -------------------------------------------------------------
def test_definitions_file():
    import io
    from strique_amd import motifs
    repeats = {"rfc1": ("AAAAG", 6), "fgf14": ("GAA", 6)}
    text = "# loci\n\nrfc1\tAAAGG, aaggg\nfgf14\tGAAGGA\n"
    assert motifs.parse_definitions(io.StringIO(text), repeats) == {"rfc1": ("AAAGG", "AAGGG"), "fgf14": ("GAAGGA",)}
    for bad, word in (("nope\tAAAGG\n", "unknown target"), ("rfc1\tAAAGG\nrfc1\tAAGGG\n", "defined twice"), ("rfc1\n", "expected target"),
                      ("rfc1\tAAAGG\textra\n", "expected target"), ("rfc1\tAAAGA\n", "same array"), ("rfc1\tA,C,G,T\n", "between 1 and 3"),
                      ("rfc1\tAANGG\n", "letters"), ("rfc1\t" + UNITS[-1] + "A\n", "emitting states")):
        with pytest.raises(ValueError, match=word):
            motifs.parse_definitions(io.StringIO(bad), repeats)
    # without a k-mer length the limit on the states is left to add_target
    assert motifs.parse_definitions(io.StringIO("rfc1\t" + UNITS[-1] + "A\n"), {"rfc1": ("AAAAG", None)}) == {"rfc1": (UNITS[-1] + "A",)}


ROWS = [
    ("r1", "rfc1", "+", 3, ("AAAAG", "AAAGG", "AAGGG"), 5, 2, (0.0, 1.0 / 3, 2.0 / 3), 22, -4039.544817646358, [(1, 100, 612), (2, 612, 1636)]),
    ("r2", "fgf14", "-", 40, ("GAA", "GAAGGA"), 1, 0, (1.0, 0.0), None, None, [(0, 7, 90)]),
]


def test_format_row_and_parse_round_trip():
    import io
    from strique_amd import motifs
    lines = ['\t'.join(motifs.HEADER)]
    for rid, target, strand, count, units, n_seg, maj, shares, count_m, log_p_m, runs in ROWS:
        lines.append(motifs.format_row(rid, target, strand, count, motifs.Row(units, n_seg, maj, shares, count_m, log_p_m, runs)))
    lines.append(motifs.format_row("r3", "plain", "+", 20, None))
    assert lines[1] == "r1\trfc1\t+\t3\t5\tAAGGG\t0.0000,0.3333,0.6667\t22\t-4039.544817646358\tAAAGG:100-612,AAGGG:612-1636"
    assert lines[2] == "r2\tfgf14\t-\t40\t1\tGAA\t1.0000,0.0000\t-\t-\tGAA:7-90"
    assert lines[3] == "r3\tplain\t+\t20" + "\t-" * 6
    got = motifs.parse(io.StringIO("\n".join(lines) + "\n"))
    assert got[0] == ("r1", "rfc1", "+", 3, (5, "AAGGG", (0.0, 0.3333, 0.6667), 22, -4039.544817646358, [("AAAGG", 100, 612), ("AAGGG", 612, 1636)]))
    assert got[1] == ("r2", "fgf14", "-", 40, (1, "GAA", (1.0, 0.0), None, None, [("GAA", 7, 90)])) and got[2] == ("r3", "plain", "+", 20, None)
    with pytest.raises(ValueError):
        motifs.parse(io.StringIO("ID\tother\n"))
    with pytest.raises(ValueError):
        motifs.parse(io.StringIO("\n".join(lines[:1] + ["r1\trfc1\t+\t3\t-\tAAGGG\t-\t-\t-\t-"]) + "\n"))


def test_cli_refusals(tmp_path, capsys):
    from strique_amd import cli
    (tmp_path / "defs.tsv").write_text("c9orf72\tGGCCCC\n")
    base = ["count", str(tmp_path / "none.fofn"), str(tmp_path / "none.model"), ROOT + "/tests/golden/repeat_config_htt.tsv"]
    d, o = ["--motif-units", str(tmp_path / "defs.tsv")], ["--motifs", str(tmp_path / "m.tsv")]
    for bad, word in ((d, "need each other"), (o, "need each other"), (["--motif-segment", "64"], "--motif-segment N needs"),
                      (d + o + ["--motif-segment", "16"], "between 32 and 4096"), (d + o + ["--scan", "--scan-min-score", "5"], "cannot be combined with --scan")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + bad)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad
    # the definition file: an unknown target, a duplicate line, what check refuses -- before any device is touched
    config = tmp_path / "config.tsv"
    config.write_text("chr\tbegin\tend\tname\trepeat\tprefix\tsuffix\nchrA\t100\t200\trfc1\tAAAAG\t" + "ACGT" * 40 + "\t" + "TGCA" * 40 + "\n")
    base[3] = str(config)
    for text in ("nope\tAAAGG\n", "rfc1\tAAAGG\nrfc1\tAAGGG\n", "rfc1\tAAAGA\n", "rfc1\tAANGG\n", "# nothing\n"):
        (tmp_path / "defs.tsv").write_text(text)
        with pytest.raises(SystemExit) as e:
            cli.main(base + d + o)
        assert e.value.code == 1, text
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--motif-units", str(tmp_path / "missing.tsv")] + o)
    assert e.value.code == 1


class MotifCounter(object):
    """Stands in for the GPU engine with the motif switch: rows and records depend on the inputs only."""
    motif_units = {"c9orf72": ("GGCCCC", "GGCCTG"), "fmr1": ("CGG", "AGG", "CCG")}

    def __init__(self):
        from test_mod_llr_host import FakeCounter
        self.inner, self.motifs, self.motif_records, self.log = FakeCounter(), None, None, []

    def set_motifs(self, on, segment=256):
        self.log.append((bool(on), segment if on else None))
        self.motifs = segment if on else None

    def detect_batch(self, items, **kw):
        self.motif_records = None
        if self.motifs is not None:
            self.motif_records = []
            for t, raw, s in items:
                K, n = len(self.motif_units[t]), len(raw)
                if n % 4 == 0:
                    self.motif_records.append(None)
                    continue
                maj = n % K
                shares = tuple((1.0 / 3 if j == maj else (2.0 / 3) / (K - 1)) for j in range(K))
                win = np.array([maj, (maj + 1) % K], np.int32)
                self.motif_records.append((maj, shares, None if n % 7 == 0 else n % 50, None if n % 7 == 0 else -1.0 / n,
                                           [(maj, int(raw[0]), int(raw[0]) + self.motifs), ((maj + 1) % K, int(raw[0]) + self.motifs, int(raw[0]) + 3 * self.motifs)],
                                           win, np.zeros((2, K))))
        return self.inner.detect_batch(items, **kw)

    def detect(self, t, raw, s, **kw):
        return self.detect_batch([(t, raw, s)], **kw)[0]


def test_the_gather_carries_the_motif_rows(cfg):
    """Two ranks write the bytes one process writes; the count rows and the unit rows do not depend on the flag; the blob has one field
    more only when the output is on."""
    import io
    from test_mod_llr_host import FakeCounter, OneRank
    from strique_amd import cli, motifs
    loci = {}
    for name, (chrom, b, e, *_r) in cfg["repeat"].items():
        loci.setdefault(chrom, []).append((name, b, e))
    lines = ["@HD\tVN:1.0"]
    for i in range(23):
        chrom, pos = ("chr9", 27570000) if i % 3 else ("chrX", 146990000)
        lines.append("\t".join(["read%d" % i, "16" if i % 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))
    get_raw = lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))
    log = cli.Log("error")
    text = lambda rows, header=True: (lambda buf: (cli.write_rows(buf, rows, header=header), buf.getvalue())[1])(io.StringIO())
    plain, uplain = io.StringIO(), io.StringIO()
    cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, plain, units=True, units_out=uplain)
    one, uone, mone, rc = io.StringIO(), io.StringIO(), io.StringIO(), MotifCounter()
    cli.run_count(iter(lines), loci, get_raw, rc, log, 4, 0, 1, one, units=True, units_out=uone, motifs=64, motifs_out=mone)
    assert one.getvalue() == plain.getvalue() and uone.getvalue() == uplain.getvalue()
    assert rc.log == [(True, 64), (False, None)] and rc.motifs is None          # the switch belongs to the run
    rows = motifs.parse(io.StringIO(mone.getvalue()))
    count_rows = plain.getvalue().splitlines()[1:]
    assert len(rows) == len(count_rows) == 23 and any(r[4] is None for r in rows) and any(r[4] is not None and r[4][3] is None for r in rows)
    for r, line in zip(rows, count_rows):
        f = line.split("\t")
        assert r[:4] == (f[0], f[1], f[2], int(f[3]))
        if r[4] is not None:
            assert r[4][1] in MotifCounter.motif_units[r[1]] and [u for u, _, _ in r[4][5]][0] == r[4][1]
    stats = {}
    parts = [cli.run_count(iter(lines), loci, get_raw, MotifCounter(), log, 4, rank, 2, stats=stats if rank == 0 else {}, units=True, motifs=64) for rank in (0, 1)]
    merged = cli.gather_rows(parts[1] + parts[0], stats["items"], OneRank, units=True, motifs=64)
    assert text(merged.rows) == plain.getvalue() and text(merged.units, cli.UNITS_HEADER) == uplain.getvalue()
    assert text(merged.riders["motifs"], motifs.HEADER) == mone.getvalue()
    # the blob: a field of its own at the end, only when the output is on; floats travel bit for bit
    on = cli.outputs_on(units=True, motifs=64)
    v = motifs.Row(("AAAAG", "AAGGG"), 3, 1, (0.1 + 0.2, 1.0 / 3), 17, -1234.5678901234567, [(1, 5, 9), (0, 9, 30)])
    blob = cli.pack_blob(on, "rfc1", "+", "-", dict(units=np.array([1, 2]), motifs=v))
    assert blob.count("\t") == 3 + len(cli.OUTPUTS) and cli.unpack_blob(on, blob)[3]["motifs"] == v
    assert cli.unpack_blob(on, cli.pack_blob(on, "rfc1", "+", "-", dict(motifs=None)))[3]["motifs"] is None
    off = cli.outputs_on(units=True)
    assert cli.pack_blob(off, "rfc1", "+", "-", dict(motifs=v)).count("\t") == 2 + len(cli.OUTPUTS)
    with pytest.raises(ValueError, match="motifs cannot be combined with a scan"):
        cli.run_count(["read1"], {}, get_raw, MotifCounter(), log, 4, 0, 1, io.StringIO(), motifs=64,
                      scan={"min_score": 5.0, "candidates": [("c9orf72", "+")], "scores": False})


def test_the_counter_switch_without_a_device(pm, pm_mod, cfg):
    """set_motifs through the recording stand-in context of the pass tests: the context is asked only while the switch is on, behind
    the passes, and told off again; Detected and the tuples of detect_batch stay as they are."""
    from test_counter_passes_host import RecordingContext, read
    from strique_amd import ffi
    from strique_amd.counter import Detected, repeatCounter

    class Ctx(RecordingContext):
        def set_motifs(self, on, segment=256):
            self.log.append(("set_motifs", bool(on)) + ((segment,) if on else ()))

        def batch_fetch_motifs(self):
            self.log.append("batch_fetch_motifs")
            rec = np.zeros(len(self.lengths), ffi.MOTIFS_DTYPE)
            rec["status"] = 1
            rec[0] = (0, 2, 2, 1, 0, 100, 228, (64, 64, 0, 0), 9, 0, -7.5)
            return rec, [np.zeros((2, 2))] + [np.zeros((0, 0))] * (len(rec) - 1), [np.array([0, 1], np.int32)] + [np.zeros(0, np.int32)] * (len(rec) - 1)

    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], context=Ctx())
    repeat, prefix, suffix = cfg["repeat"]["c9orf72"][3:6]
    with pytest.raises(ValueError):
        rc.set_motifs(True)                                      # no target with motifs
    rc.add_target("c9orf72", repeat, prefix, suffix, motifs=["GGCCTG"])
    items = [("c9orf72", read(11), "+"), ("c9orf72", read(12), "-")]
    assert rc.detect_batch(items, records=True)[0] == Detected(rc.detect_batch(items)[0], None, None, None) and rc.motif_records is None
    assert not [e for e in rc.ctx.log if "motifs" in str(e)]     # off: the context never hears of it
    with pytest.raises(ValueError):
        rc.set_motifs(True, 16)
    rc.set_motifs(True, 64)
    del rc.ctx.log[:]
    rows = rc.detect_batch(items)
    assert [type(r) for r in rows] == [tuple, tuple] and len(rows[0]) == 7
    names = [e if isinstance(e, str) else e[0] for e in rc.ctx.log]
    assert rc.ctx.log[0] == ("set_motifs", True, 64) and names[1] == "detect_batch_reads" and "batch_fetch_motifs" in names
    assert names.index("batch_fetch_motifs") < names.index("set_motifs", 1) and ("set_motifs", False) in rc.ctx.log
    first, second = rc.motif_records
    assert second is None and first[:4] == (1, (0.5, 0.5), 9, -7.5) and first[4] == [(0, 100, 164), (1, 164, 228)]
    with pytest.raises(ValueError):
        rc.scan_batch([read(11)], min_score=5.0)
    rc.set_motifs(False)
    assert rc.motifs is None
