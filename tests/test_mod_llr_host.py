"""count --mod-llr without a GPU: the ABI, the reference's own properties, the command line."""
import io
import os

import numpy as np
import pytest

import mod_llr_ref
from conftest import oracle_tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_the_entries_and_keeps_its_version():
    from strique_amd import ffi
    lib = ffi.load_library()
    assert lib.strq_abi_version() == 13
    for name in ("strq_set_mod_llr", "strq_batch_fetch_mod_llr", "strq_last_mod_llr"):
        getattr(lib, name)
    header = open(os.path.join(ROOT, "include", "strique_hip.h")).read()
    for name in ("strq_set_mod_llr", "strq_batch_fetch_mod_llr"):
        at = header.index("int %s(" % name)
        assert "STRique.py:492-500" in header[header.rindex("/*", 0, at):at]
    assert ffi.Context.set_mod_llr and ffi.Context.batch_fetch_mod_llr


@pytest.fixture(scope="module")
def refs(pm, pm_mod, cfg, orc, opm, opm_mod, targets):
    """Three 5 kb reads on C9orf72 with 12, 24 and 40 units (the repeat loop sees one unit fewer than planted): from the modified
    table, from the base table, and a '-' strand one."""
    from strique_amd import synth
    params = orc.align_params(cfg["align"])
    out = []
    for k, (table, strand, nrep) in enumerate(((pm_mod, "+", 13), (pm, "+", 25), (pm_mod, "-", 41))):
        sig = synth.make_read(synth.KmerTable(table), 31, k, 5000, targets["c9orf72"], nrep, strand=strand)[0]
        tc = oracle_tc(orc, opm, targets, "c9orf72", strand, cfg["HMM"], opm_mod)
        out.append(mod_llr_ref.reference(sig, tc, opm, params, opm_mod))
    return out


def test_reference_units_are_the_characters_of_the_pattern(refs):
    for ref in refs:
        assert set(ref["pattern"]) <= set("01") and 12 <= len(ref["pattern"]) <= 40, ref["pattern"]
        assert len(ref["bounds"]) == len(ref["pattern"]) == len(ref["V"])
        assert ref["bounds"][0][0] == 0 and ref["bounds"][-1][1] == len(ref["x"]) - 1
        for (u0, w0), (u1, w1) in zip(ref["bounds"], ref["bounds"][1:]):
            assert u1 == w0 + 1 and w0 >= u0 + 2


def test_reference_llr_has_the_sign_of_the_call(refs):
    """With the segmentation fixed the units are independent, so the branch the joint decode called is never the worse one.  Slack:
    the joint decode accumulates from t = 0, a unit score from u_j -- values of 10^2 .. 10^3 over ~50 steps, rounding ~1e-11."""
    seen = set()
    for ref in refs:
        llr = ref["V"][:, 1] - ref["V"][:, 0]
        assert not np.isnan(llr).any()
        for ch, v in zip(ref["pattern"], llr):
            assert v >= -1e-9 if ch == "1" else v <= 1e-9, (ch, v)
            seen.add(ch)
    assert seen == set("01")


# ---- command line ---------------------------------------------------------------------------------------------------------------
def test_mod_llr_needs_a_mod_model_and_excludes_scan(capsys):
    from strique_amd import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(["count", "reads.fofn", "model", "repeats.tsv", "--mod-llr", "llr.tsv"])
    assert ei.value.code == 2 and "--mod-llr needs --mod_model" in capsys.readouterr().err
    with pytest.raises(SystemExit) as ei:
        cli.main(["count", "reads.fofn", "model", "repeats.tsv", "--mod_model", "m", "--scan", "--scan-min-score", "5", "--mod-llr", "llr.tsv"])
    assert ei.value.code == 2 and "--mod-llr cannot be combined with --scan" in capsys.readouterr().err


def test_row_format_round_trip():
    from strique_amd import cli
    row = cli.format_mod_llr("r1", "c9orf72", "+", 12, "011", np.array([-3.14159, np.inf, -np.inf]))
    assert row == "r1\tc9orf72\t+\t12\t011\t3\t-3.1416,inf,-inf"
    assert cli.format_mod_llr("r2", "t", "-", 0, "-", None) == "r2\tt\t-\t0\t-\t0\t-"
    text = "\t".join(cli.MODLLR_HEADER) + "\n" + row + "\n" + cli.format_mod_llr("r2", "t", "-", 0, "-", None) + "\n"
    assert cli.parse_mod_llr(io.StringIO(text)) == [("r1", "c9orf72", "+", 12, "011", [-3.1416, np.inf, -np.inf]), ("r2", "t", "-", 0, "-", [])]
    assert cli.MODLLR_HEADER == ["ID", "target", "strand", "count", "mod_pattern", "n_units", "llr"]


class FakeCounter(object):
    """Stands in for the GPU engine: everything depends on the inputs only."""

    def detect_batch(self, items, units=False, confidence=False, mod_llr=False):
        out = []
        for t, raw, s in items:
            n = len(raw) % 5
            row = (len(raw) % 97, 1.5, 2.5, -3.0 * len(t), int(raw[0]), 7, "01"[len(raw) % 2] * n if n else "-")
            pos = None if n == 0 else np.arange(n, dtype=np.int64) * 13 + int(raw[0])
            conf = None if n == 0 else (-3.0 * len(t) + 1.0 / len(raw), 0.1 / 3, 1.0 / (1 + int(raw[0])))
            llr = None if n == 0 else np.arange(n) / 7.0 - (np.inf if len(raw) % 11 == 0 else 0.25)
            extra = ((pos,) if units else ()) + ((conf,) if confidence else ()) + ((llr,) if mod_llr else ())
            out.append((row,) + extra if extra else row)
        return out

    def detect(self, t, raw, s, **kw):
        return self.detect_batch([(t, raw, s)], **kw)[0]


class OneRank(object):
    """dist.gather_results of a single rank."""

    @staticmethod
    def gather_results(rec, idx, n_items, mods):
        full = np.zeros(n_items, rec.dtype); full[idx] = rec
        full_mods = [""] * n_items
        for i, m in zip(idx, mods):
            full_mods[int(i)] = m
        return full, full_mods


@pytest.mark.parametrize("units,confidence", [(False, False), (True, False), (False, True), (True, True)])
def test_count_rows_with_a_stubbed_counter(cfg, units, confidence):
    """The ratio rows next to the count rows: single process, and through the blob of the gather; count, unit and confidence rows
    byte-identical to a run without the flag."""
    from strique_amd import cli
    loci = {}
    for name, (chrom, b, e, *_r) in cfg["repeat"].items():
        loci.setdefault(chrom, []).append((name, b, e))
    lines = ["@HD\tVN:1.0"]
    for i in range(23):
        chrom, pos = ("chr9", 27570000) if i % 3 else ("chrX", 146990000)
        lines.append("\t".join(["read%d" % i, "16" if i % 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))
    get_raw = lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))
    log = cli.Log("error")
    kw = dict(units=units, confidence=confidence)
    plain, uplain, cplain = io.StringIO(), io.StringIO(), io.StringIO()
    cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, plain, units_out=uplain if units else None, conf_out=cplain if confidence else None, **kw)
    one, uone, cone, lone, st = io.StringIO(), io.StringIO(), io.StringIO(), io.StringIO(), {}
    cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, one, stats=st, units_out=uone if units else None,
                  conf_out=cone if confidence else None, mod_llr=True, llr_out=lone, **kw)
    assert one.getvalue() == plain.getvalue() and uone.getvalue() == uplain.getvalue() and cone.getvalue() == cplain.getvalue()
    rows = cli.parse_mod_llr(io.StringIO(lone.getvalue()))
    counts = [l.split("\t") for l in one.getvalue().splitlines()[1:]]
    assert len(rows) == len(counts) == 23
    for r, c in zip(rows, counts):
        assert list(r[:3]) == c[:3] and str(r[3]) == c[3] and r[4] == c[9]
        assert len(r[5]) == (0 if r[4] == "-" else len(r[4]))
    assert any(v == -np.inf for r in rows for v in r[5]) and any(not r[5] for r in rows)
    # several ranks: the same rows out of the gather's blob
    st2 = {}
    mine = cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 2, stats=st2, mod_llr=True, **kw)
    other = cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 1, 2, stats={}, mod_llr=True, **kw)
    got = cli.gather_rows(mine + other, st2["items"], OneRank, mod_llr=True, **kw)
    merged, munits, mconf, mllr = got.rows, got.units, got.confidence, got.mod_llr
    buf = io.StringIO(); cli.write_rows(buf, merged)
    lbuf = io.StringIO(); cli.write_rows(lbuf, mllr, header=cli.MODLLR_HEADER)
    assert buf.getvalue() == plain.getvalue() and lbuf.getvalue() == lone.getvalue()
    assert (munits is None) == (not units) and (mconf is None) == (not confidence)
    if units:
        ubuf = io.StringIO(); cli.write_rows(ubuf, munits, header=cli.UNITS_HEADER)
        assert ubuf.getvalue() == uplain.getvalue()
    if confidence:
        cbuf = io.StringIO(); cli.write_rows(cbuf, mconf, header=cli.CONF_HEADER)
        assert cbuf.getvalue() == cplain.getvalue()
