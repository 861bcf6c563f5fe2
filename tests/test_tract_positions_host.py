"""Tract positions without a GPU: the positions file, the refusals of `count`, the rows through a stubbed counter and through the
gather blob, the header against the library's exports, the reference's positions on the shared clean reads, and the tie guard of
the reads tests/test_gpu_tract_positions.py decodes (the un-baked net and the baked model give the same positions for every one)."""
import io
import os
import re

import numpy as np
import pytest

import tract_pos_cases as tpc
import tract_pos_ref as tpr
import tract_ref as tr
from test_mod_llr_host import FakeCounter, OneRank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("strq_set_tract_positions", "strq_batch_fetch_tract_positions", "strq_last_tract_positions", "strq_viterbi_tract_positions")


# ---- the file ----------------------------------------------------------------------------------------------------------------------
def test_positions_file_round_trip():
    from strique_amd import tracts
    assert tracts.POS_HEADER == ["ID", "target", "strand", "count", "n_tracts", "tract_counts", "tract_spans", "tract_positions"]
    a = lambda *v: np.array(v, np.int64)
    recs = [("r1", "htt", "+", 19, ((12, 7), -2319.5, (a(100, 130, 161), a(400, 409)))),
            ("r2", "cnbp", "-", 0, None),                                                   # no tract record
            ("r3", "cnbp", "-", 13, ((6, 10, 7), -1.0, (a(5), a(), a(7, 8)))),              # a tract without positions
            ("r4", "htt", "+", 36, ((30, 4), -3.0, None)),                                  # pos_status 2
            ("r5", "htt", "-", 3, ((2, 1), -3.0, (a(), a())))]
    lines = [tracts.format_positions_row(*r) for r in recs]
    assert lines[0] == "r1\thtt\t+\t19\t2\t12,7\t100-161,400-409\t100,130,161;400,409"
    assert lines[1] == "r2\tcnbp\t-\t0\t-\t-\t-\t-"
    assert lines[2] == "r3\tcnbp\t-\t13\t3\t6,10,7\t5-5,-,7-8\t5;-;7,8"
    assert lines[3] == "r4\thtt\t+\t36\t2\t30,4\t-\t-"
    assert lines[4] == "r5\thtt\t-\t3\t2\t2,1\t-,-\t-;-"
    back = tracts.parse_positions(io.StringIO("\t".join(tracts.POS_HEADER) + "\n" + "\n".join(lines) + "\n"))
    assert [b[:4] for b in back] == [r[:4] for r in recs]
    assert back[1][4] is None and back[3][4] == ((30, 4), None, None)
    assert back[0][4] == ((12, 7), ((100, 161), (400, 409)), ((100, 130, 161), (400, 409)))
    assert back[2][4] == ((6, 10, 7), ((5, 5), None, (7, 8)), ((5,), (), (7, 8)))
    assert back[4][4] == ((2, 1), (None, None), ((), ()))
    assert tracts.spans(recs[0][4][2]) == ((100, 161), (400, 409))
    head = "\t".join(tracts.POS_HEADER) + "\n"
    for bad in ("x\ty\n", head + "r\tt\t+\t3\t2\t1,2,3\t-\t-\n", head + "r\tt\t+\t3\t-\t1\t-\t-\n", head + "r\tt\t+\t3\n",
                head + "r\tt\t+\t3\t2\t1,2\t5-6,7-7\t5,6;8\n", head + "r\tt\t+\t3\t2\t1,2\t5-6\t5,6;7\n"):
        with pytest.raises(ValueError):
            tracts.parse_positions(io.StringIO(bad))
    with pytest.raises(ValueError):
        tracts.format_positions_row("r", "t", "+", 3, ((1, 2), -1.0, (a(1),)))               # two tracts, one list


# ---- count: refusals, rows, gather -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,message", [
    (["--tract-positions", "p.tsv"], "--tract-positions FILE needs --tract-units FILE --tracts FILE: the positions are those of the tract counts"),
    # (the older check of the two flags it needs comes first, as the arguments' checks stand in the order they were written in)
    (["--tract-positions", "p.tsv", "--tract-units", "d.tsv"], "--tract-units FILE and --tracts FILE need each other: the definitions, and where the counts go"),
    (["--tract-positions", "p.tsv", "--tract-units", "d.tsv", "--tracts", "t.tsv", "--scan", "--scan-min-score", "5"], None),
])
def test_count_refusals(capsys, tmp_path, extra, message):
    from strique_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["count", str(tmp_path / "reads.fofn"), str(tmp_path / "m.model"), str(tmp_path / "repeat.tsv")] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    if message is None:
        assert "cannot be combined with --scan" in err
    else:
        assert err.endswith(": error: " + message + "\n")


class PositionsCounter(FakeCounter):
    """FakeCounter with the tract switch and its positions keyword: records that depend on the inputs only."""
    tracts = positions = False

    def set_tracts(self, on, positions=False):
        self.tracts, self.positions = bool(on), bool(on and positions)

    def detect_batch(self, items, units=False, confidence=False, mod_llr=False, records=False):
        from strique_amd import cli
        rows = FakeCounter.detect_batch(self, items, units=units, confidence=confidence, mod_llr=mod_llr)
        if not records:
            return rows
        out = []
        for (t, raw, s), res in zip(items, rows):
            d = cli.as_detected(res, units, confidence, mod_llr)
            k = len(raw) % 4
            rec = None
            if k and self.tracts:
                K = 2 + k % 2
                rec = (tuple(int(raw[0]) + j for j in range(K)), -1.0 / len(raw) - len(t))
                if self.positions:
                    # k == 3: back-pointers over the budget; else tract j holds j positions (tract 0 none)
                    rec += (None if k == 3 else tuple(np.arange(j, dtype=np.int64) * 7 + int(raw[0]) + 100 * j for j in range(K)),)
            out.append(d._replace(tracts=rec))
        return out

    def detect(self, t, raw, s, **kw):
        return self.detect_batch([(t, raw, s)], **kw)[0]


def _input(cfg):
    loci = {}
    for name, (chrom, b, e, *_r) in cfg["repeat"].items():
        loci.setdefault(chrom, []).append((name, b, e))
    lines = ["@HD\tVN:1.0"]
    for i in range(23):
        chrom, pos = ("chr9", 27570000) if i % 3 else ("chrX", 146990000)
        lines.append("\t".join(["read%d" % i, "16" if i % 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))
    return lines, loci, lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))


def test_rows_and_gather_with_a_stubbed_counter(cfg):
    """One positions row per count row; the count rows and the tract rows byte-identical with and without the positions; the same
    rows out of the gather's blob, which has no field of its own for them."""
    from strique_amd import cli, tracts
    lines, loci, get_raw = _input(cfg)
    log = cli.Log("error")
    plain, tplain = io.StringIO(), io.StringIO()
    cli.run_count(iter(lines), loci, get_raw, PositionsCounter(), log, 4, 0, 1, plain, tracts=True, tracts_out=tplain)
    counter = PositionsCounter()
    one, tone, pone, st = io.StringIO(), io.StringIO(), io.StringIO(), {}
    cli.run_count(iter(lines), loci, get_raw, counter, log, 4, 0, 1, one, stats=st, tracts=True, tracts_out=tone, tract_positions=True, tract_positions_out=pone)
    assert counter.tracts is False and counter.positions is False          # the switch belongs to the run
    assert one.getvalue() == plain.getvalue() and tone.getvalue() == tplain.getvalue()
    rows = tracts.parse_positions(io.StringIO(pone.getvalue()))
    trows = tracts.parse(io.StringIO(tone.getvalue()))
    assert len(rows) == len(trows) == len(st["tract_position_rows"]) == 23
    for r, t in zip(rows, trows):
        assert r[:4] == t[:4] and (r[4] is None) == (t[4] is None) and (r[4] is None or r[4][0] == t[4][0])
    assert any(r[4] is None for r in rows) and any(r[4] and r[4][2] is None for r in rows)
    assert any(r[4] and r[4][2] and r[4][2][0] == () and len(r[4][2][-1]) > 0 for r in rows)
    # several ranks: the positions travel in the tracts field of the blob
    names = [o.name for o in cli.OUTPUTS]
    assert "tract_positions" not in names and [o.name for o in cli.RIDERS] == ["tract_positions"] and cli.RIDERS[0].rides == ("tracts", "positions")
    on = cli.outputs_on(tracts=True, tract_positions=True)
    for v in (((12, 7), -2319.51263745851, (np.array([3, 9], np.int64), np.zeros(0, np.int64))), ((9, 6, 11), -1.5, None), ((1, 2), -0.5), None):
        blob = cli.pack_blob(on, "htt", "+", "-", dict(tracts=v))
        assert blob.count("\t") == 2 + len(cli.OUTPUTS)
        back = cli.unpack_blob(on, blob)[3]["tracts"]
        assert (back is None) == (v is None)
        if v is not None:
            assert back[:2] == v[:2] and len(back) == len(v)
            assert len(v) == 2 or (back[2] is None) == (v[2] is None)
            assert len(v) == 2 or v[2] is None or tpr.same_positions(back[2], v[2])
    st2 = {}
    kw = dict(tracts=True, tract_positions=True)
    mine = cli.run_count(iter(lines), loci, get_raw, PositionsCounter(), log, 4, 0, 2, stats=st2, **kw)
    other = cli.run_count(iter(lines), loci, get_raw, PositionsCounter(), log, 4, 1, 2, stats={}, **kw)
    got = cli.gather_rows(mine + other, st2["items"], OneRank, **kw)
    buf = io.StringIO(); cli.write_rows(buf, got.rows)
    tbuf = io.StringIO(); cli.write_rows(tbuf, got.tracts, header=tracts.HEADER)
    pbuf = io.StringIO(); cli.write_rows(pbuf, got.riders["tract_positions"], header=tracts.POS_HEADER)
    assert buf.getvalue() == plain.getvalue() and tbuf.getvalue() == tplain.getvalue() and pbuf.getvalue() == pone.getvalue()
    assert cli.gather_rows(mine + other, st2["items"], OneRank, tracts=True).riders == {}
    # the refusals of run_count: without the tract counts, and in a scan
    with pytest.raises(ValueError, match="^tract positions need the tract counts$"):
        cli.run_count(iter(lines), loci, get_raw, PositionsCounter(), log, 4, tract_positions=True)
    with pytest.raises(ValueError):
        cli.run_count(["r"], loci, get_raw, PositionsCounter(), log, 4, scan={"min_score": 5.0, "candidates": [], "scores": False}, **kw)


def test_counter_switch_and_element():
    """set_tracts(on, positions): the context's switch rides on the tracts switch, the element has three parts in configured order,
    None for pos_status 2; with positions off no call reaches the context and the element is as it was."""
    from test_counter_passes_host import RecordingContext, _struct, make_counter
    import json
    from strique_amd import ffi
    from strique_amd.pore_model import pore_model
    golden = os.path.join(ROOT, "tests", "golden")
    t = np.load(os.path.join(golden, "pore_tables.npz"))
    pm = pore_model(table=(t["base_kmer"], t["base_mean"], t["base_stdv"])); pm_mod = pore_model(table=(t["mod_kmer"], t["mod_mean"], t["mod_stdv"]))
    cfg = json.load(open(os.path.join(golden, "config.json")))

    class Ctx(RecordingContext):
        def set_tract_positions(self, on):
            self.log.append(("set_tract_positions", bool(on)))

        def batch_fetch_tract_positions(self):
            self.log.append("batch_fetch_tract_positions")
            a = lambda *v: np.array(v, np.int64)
            canned = {11: (0, (a(1, 2), a(5), a(9, 10, 11))), 12: (2, None)}
            return [canned.get(n, (1, None)) for n in self.lengths]

    rc = make_counter(pm, pm_mod, cfg)
    rc.ctx = ctx = Ctx()
    ctx.canned = {"tracts": {11: _struct(ffi.TRACTS_DTYPE, status=0, n_tracts=3, count=[4, 5, 6], log_p=-33.25),
                             12: _struct(ffi.TRACTS_DTYPE, status=0, n_tracts=2, count=[8, 9, 0], log_p=-2.5)}}
    rc.tract_models = {tc.target_id: (None, s) for tc, s in zip(rc.targets["c9orf72"], "+-")}
    rc._ensure_tracts = lambda: None
    items = [("c9orf72", np.zeros(11, np.int16), "-"), ("c9orf72", np.zeros(12, np.int16), "+"), ("c9orf72", np.zeros(13, np.int16), "+")]
    rc.set_tracts(True, positions=True)
    a, b, c = rc.detect_batch(items, records=True)
    assert a.tracts[:2] == ((6, 5, 4), -33.25) and [p.tolist() for p in a.tracts[2]] == [[9, 10, 11], [5], [1, 2]]      # the - strand: configured order
    assert b.tracts == ((8, 9), -2.5, None) and c.tracts is None
    log = ctx.log
    assert log.index(("set_tracts", True)) < log.index(("set_tract_positions", True)) < log.index("batch_fetch_tracts")
    assert log.index("batch_fetch_tract_positions") < log.index(("set_tract_positions", False))
    del ctx.log[:]
    rc.set_tracts(True)
    assert [d.tracts for d in rc.detect_batch(items, records=True)] == [((6, 5, 4), -33.25), ((8, 9), -2.5), None]
    assert not any("tract_positions" in (e if isinstance(e, str) else e[0]) for e in ctx.log)
    rc.set_tracts(False, positions=True)
    assert rc.tracts is False and rc.tract_positions is False


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_and_exports_agree_on_the_new_symbols():
    import ctypes
    from strique_amd import build, ffi
    header = open(os.path.join(ROOT, "include", "strique_hip.h")).read()
    declared = set(re.findall(r"\b(strq_[a-z_0-9]+)\s*\(", header))
    handle = ctypes.CDLL(build.LIB)
    for name in NEW_SYMBOLS:
        assert name in declared and getattr(handle, name) is not None
    for method in ("set_tract_positions", "batch_fetch_tract_positions", "last_tract_positions", "viterbi_tract_positions"):
        assert callable(getattr(ffi.Context, method))
    assert "strq_abi_version" in declared


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _flanks(cfg):
    prefix, suffix = cfg["repeat"]["c9orf72"][4:6]
    return prefix[-50:].upper(), suffix[:50].upper()


def test_reference_positions_on_the_shared_cases(opm, cfg):
    """count_j - bias_j positions per tract, ascending, and the tracts do not interleave in the signal."""
    prefix, suffix = _flanks(cfg)
    for name, strand, planted, x, m in tr.cases(opm, prefix, suffix, cfg["HMM"]):
        logp, counts, pos, status = tpr.decode(m["prep"], m["tract_of"], m["K"], x)
        a = tr.decode_a(m["prep"], m["tract_of"], m["K"], x)
        assert status == 0 and (a[0], a[1], a[2]) == (logp, counts, 0)
        want = [c - q for c, q in zip(tr.configured([p + e for p, e in zip(planted, tr.RECORDED_ERROR[(name, strand, planted)])], strand), m["bias"])]
        assert [len(p) for p in pos] == want == counts, (name, strand, planted)
        for j, p in enumerate(pos):
            assert len(p) > 0 and (np.diff(p) > 0).all() and p[0] >= 0 and p[-1] < len(x)
            assert j == 0 or pos[j - 1][-1] < p[0], (name, strand, planted, j)          # model order is signal order


def test_tie_guard_of_the_pipeline_reads(pm, opm, orc, cfg):
    """For every read the GPU pipeline test uses: the oracle's path on the un-baked net and its path on the baked model the product
    builds give the same record -- counts, log-probability bits and positions (README, 'One limit of what the tests pin': the two
    may break a tie between equal paths differently, and the kernels follow the baked arrays).  No read is left out."""
    from strique_amd import hmm, tracts
    prefix, suffix = tpc.full_flanks(cfg)
    n = 0
    for (target, sig, strand), row, rec, (b, x), m in tpc.pipeline(pm, opm, orc, cfg):
        if m is None:
            continue
        units, linkers = tr.LOCI[target]
        un, li = tracts.strand_definition(units, linkers, strand)
        p, s = (prefix[-50:], suffix[:50]) if strand == '+' else (tr.orc.revcomp(suffix[:50]), tr.orc.revcomp(prefix[-50:]))
        cm = hmm.CompoundRepeatModel(un, li, p, s, pm, cfg["HMM"])
        baked = tpr.record_on(cm.baked, cm.tract_of, cm.n_tracts, list(cm.count_bias), strand, b, x)
        assert (baked is None) == (rec is None), (target, strand)
        if rec is None:
            continue
        n += 1
        assert baked[0] == rec[0] and np.float64(baked[1]).tobytes() == np.float64(rec[1]).tobytes(), (target, strand, baked[:2], rec[:2])
        assert tpr.same_positions(baked[2], rec[2]), (target, strand)
        for c, q, pos in zip(rec[0], tracts.configured_order(m[0]["bias"], strand), rec[2]):
            assert len(pos) == c - q and (np.diff(pos) > 0).all()
    assert n == sum(1 for r in tpc.PIPELINE_READS if r[3] == "read")


# ---- plot --------------------------------------------------------------------------------------------------------------------------
def test_plot_marks_the_tract_positions(tmp_path):
    """`plot --tract-positions pos.tsv`: the figure changes, and every Axes carries per tract the positions inside its range."""
    from contextlib import redirect_stdout
    import h5write
    from matplotlib.figure import Figure
    from strique_amd import cli, plotting, tracts
    rng = np.random.default_rng(5)
    rid = "bbbbbbbb-0002-4000-8000-000000000000"
    sig = rng.integers(200, 900, 6000).astype(np.int16)
    tree = {"attrs": {"file_version": "2.0"}, "groups": {"read_" + rid: {"groups": {
        "Raw": {"attrs": {"read_id": rid, "duration": len(sig), "read_number": 1, "start_time": 1, "median_before": 200.0},
                "datasets": {"Signal": (sig, {})}},
        "channel_id": {"attrs": {"channel_number": "1", "digitisation": 8192.0, "offset": 10.0, "range": 1400.5, "sampling_rate": 4000.0}}}}}}
    src = tmp_path / "src"; src.mkdir()
    (src / "batch.fast5").write_bytes(h5write.write_tree(tree))
    buf = io.StringIO()
    with redirect_stdout(buf):
        cli.main(["index", str(src)])
    (src / "reads.fofn").write_text(buf.getvalue())
    counts = tmp_path / "counts.tsv"
    counts.write_text("\t".join(cli.HEADER) + "\n" + "\t".join([rid, "htt", "+", "5", "6.5", "6.1", "-1234.5", "1000", "2500", "-"]) + "\n")
    pos = (np.array([1010, 1500, 2000], np.int64), np.array([2600, 3450], np.int64))
    pfile = tmp_path / "pos.tsv"
    pfile.write_text("\t".join(tracts.POS_HEADER) + "\n" + tracts.format_positions_row(rid, "htt", "+", 5, ((5, 4), -1.0, pos)) + "\n")
    args = [str(src / "reads.fofn"), "--counts", str(counts), "--width", "6", "--height", "4"]
    plain = cli.plot(args + ["--output", str(tmp_path / "p0")])
    marked = cli.plot(args + ["--output", str(tmp_path / "p1"), "--tract-positions", str(pfile)])
    assert len(plain) == len(marked) == 1 and open(plain[0], "rb").read() != open(marked[0], "rb").read()
    row = next(iter(plotting.parse_counts(open(counts))))
    axes = plotting.draw(Figure(figsize=(6, 4)), sig, row, zoom=500, tract_positions=pos)
    assert [p.tolist() for p in axes["overview"].strique_tract_positions] == [p.tolist() for p in pos]
    lo, hi = plotting.Windows(len(sig), row.offset, row.ticks, 0.1, 500).left
    assert [p.tolist() for p in axes["left"].strique_tract_positions] == [[u for u in p.tolist() if lo <= u < hi] for p in pos]
    assert all(hasattr(ax, "strique_tract_positions") for ax in axes.values())
    assert not hasattr(plotting.draw(Figure(figsize=(6, 4)), sig, row, zoom=500)["overview"], "strique_tract_positions")
