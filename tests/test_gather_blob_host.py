"""The blob that carries a read's optional outputs between ranks (cli.pack_blob / cli.unpack_blob) and the gather built on it
(cli.gather_rows): every combination of the optional outputs gives, out of two ranks, the bytes a single process writes."""
import io
import itertools

import numpy as np
import pytest

from test_mod_llr_host import FakeCounter, OneRank

COMBOS = list(itertools.product((False, True), repeat=3))          # units, confidence, mod_llr

# (target, strand, modification pattern, {output: value}): a decoded read with a pattern, ratios that are infinite, an undecoded
# read, a decoded read without pattern or units, and floats that str() would not carry
READS = [
    ("c9orf72", "+", "0110", dict(units=np.array([101, 230, 377, 512], np.int64), confidence=(-1234.5678901234567, 0.1 + 0.2, 1e-300),
                                  mod_llr=np.array([-3.5, np.inf, -np.inf, 1.0 / 3]))),
    ("c9orf72", "-", "-", dict(units=None, confidence=None, mod_llr=None)),
    ("fmr1", "-", "-", dict(units=np.zeros(0, np.int64), confidence=(-0.0, 5e-324, 2.0 ** 70), mod_llr=np.zeros(0))),
    ("htt", "+", "1", dict(units=np.array([2 ** 40], np.int64), confidence=(float(np.nextafter(1.0, 2.0)), 1.0, 0.0), mod_llr=np.array([-np.inf]))),
]
SCORES = [(12.5, 0.1 + 0.7), (1.0 / 3, -0.0), (np.nextafter(8.0, 9.0), 1e-17), (0.0, 7.25)]


def _bits(values):
    return np.ascontiguousarray(values, np.float64).view(np.uint64).tolist()


def _check_values(on, got, want):
    names = {o.name for o in on}
    for name in ("units", "confidence", "mod_llr", "scores"):
        w = want.get(name) if name in names else None
        if w is None or len(w) == 0:          # absent, not asked for, or empty: nothing travels
            assert got[name] is None, (name, got[name])
        elif name == "units":
            assert got[name] == [int(x) for x in w] and all(type(x) is int for x in got[name])
        else:
            assert _bits(got[name]) == _bits(w), (name, got[name], w)          # bit for bit: repr() of a float reads back exactly


@pytest.mark.parametrize("units,confidence,mod_llr", COMBOS)
def test_blob_round_trips(units, confidence, mod_llr):
    from strique_amd import cli
    on = cli.outputs_on(units=units, confidence=confidence, mod_llr=mod_llr)
    assert [o.name for o in on] == [n for n, f in (("units", units), ("confidence", confidence), ("mod_llr", mod_llr)) if f]
    for target, strand, mod, values in READS:
        blob = cli.pack_blob(on, target, strand, mod, values)
        assert blob.count("\t") == 2 + len(cli.OUTPUTS)          # a fixed number of fields, whatever is on
        t, s, m, got = cli.unpack_blob(on, blob)
        assert (t, s, m) == (target, strand, mod)
        _check_values(on, got, values)


@pytest.mark.parametrize("units", [False, True])
def test_blob_round_trips_for_a_scan(units):
    from strique_amd import cli
    on = cli.outputs_on(units=units, scores=True)
    for target, strand, mod, values in READS:
        values = dict(values, scores=SCORES)
        t, s, m, got = cli.unpack_blob(on, cli.pack_blob(on, target, strand, mod, values))
        assert (t, s, m) == (target, strand, mod)
        _check_values(on, got, values)
        assert got["scores"] == [tuple(float(x) for x in pair) for pair in SCORES]
    # a read without a winner: no target, no strand, no row -- the scores still travel
    t, s, m, got = cli.unpack_blob(on, cli.pack_blob(on, None, None, "-", dict(scores=SCORES)))
    assert (t, s, m) == ("-", "-", "-") and got["units"] is None
    _check_values(on, got, dict(scores=SCORES))


def _sam(cfg):
    loci = {}
    for name, (chrom, b, e, *_r) in cfg["repeat"].items():
        loci.setdefault(chrom, []).append((name, b, e))
    lines = ["@HD\tVN:1.0"]
    for i in range(23):
        chrom, pos = ("chr9", 27570000) if i % 3 else ("chrX", 146990000)
        lines.append("\t".join(["read%d" % i, "16" if i % 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))
    return loci, lines


def _text(rows, header=True):
    from strique_amd import cli
    buf = io.StringIO(); cli.write_rows(buf, rows, header=header)
    return buf.getvalue()


@pytest.mark.parametrize("units,confidence,mod_llr", COMBOS)
def test_two_ranks_write_the_bytes_of_one_process(cfg, units, confidence, mod_llr):
    from strique_amd import cli
    loci, lines = _sam(cfg)
    get_raw = lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))          # lengths with len % 5 == 0 (undecoded) and len % 11 == 0 (-inf)
    log = cli.Log("error")
    kw = dict(units=units, confidence=confidence, mod_llr=mod_llr)
    files = {name: io.StringIO() for name in ("rows", "units", "confidence", "mod_llr")}
    cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, files["rows"], units_out=files["units"] if units else None,
                  conf_out=files["confidence"] if confidence else None, llr_out=files["mod_llr"] if mod_llr else None, **kw)
    stats = {}
    parts = [cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, rank, 2, stats=stats if rank == 0 else {}, **kw) for rank in (0, 1)]
    assert parts[0] and parts[1]
    merged = cli.gather_rows(parts[1] + parts[0], stats["items"], OneRank, **kw)
    assert isinstance(merged, cli.Merged) and merged.scores is None
    assert _text(merged.rows) == files["rows"].getvalue() and len(merged.rows) == 23
    for name, header, flag in (("units", cli.UNITS_HEADER, units), ("confidence", cli.CONF_HEADER, confidence), ("mod_llr", cli.MODLLR_HEADER, mod_llr)):
        got = getattr(merged, name)
        assert (got is None) == (not flag), name
        if flag:
            assert _text(got, header) == files[name].getvalue() and len(got) == 23, name

    class OtherRank(object):          # off rank 0 the gather returns nothing
        gather_results = staticmethod(lambda rec, idx, n_items, mods: (None, None))
    assert cli.gather_rows(parts[1], stats["items"], OtherRank, **kw) == cli.Merged(None, None, None, None, None)


class ScanCounter(object):
    """FakeCounter for a scan: the winner, if any, and the scores depend on the read only."""
    CANDS = [("c9orf72", "+"), ("c9orf72", "-"), ("fmr1", "+"), ("fmr1", "-")]

    def scan_batch(self, signals, min_score=None, units=False, scores=False):
        out, sc = [], np.zeros((len(signals), len(self.CANDS), 2))
        for i, raw in enumerate(signals):
            sc[i] = (np.arange(8).reshape(4, 2) + len(raw)) / 7.0
            if len(raw) % 3 == 0:
                out.append(None)
                continue
            row = FakeCounter().detect_batch([("t", raw, "+")], units=units)[0]
            out.append(self.CANDS[len(raw) % 4] + (row,))
        return out, sc


@pytest.mark.parametrize("units", [False, True])
def test_two_ranks_write_the_bytes_of_one_process_for_a_scan(units):
    from strique_amd import cli, scan as scan_mod
    scan = {"min_score": 5.0, "candidates": ScanCounter.CANDS, "scores": True}
    ids = ["read%d" % i for i in range(17)]
    get_raw = lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))
    log = cli.Log("error")
    files = {name: io.StringIO() for name in ("rows", "units", "scores")}
    cli.run_count(list(ids), {}, get_raw, ScanCounter(), log, 4, 0, 1, files["rows"], units=units, units_out=files["units"] if units else None,
                  scan=scan, scores_out=files["scores"])
    assert len(files["scores"].getvalue().splitlines()) == 1 + len(ids) > len(files["rows"].getvalue().splitlines()) > 1
    stats = {}
    parts = [cli.run_count(list(ids), {}, get_raw, ScanCounter(), log, 4, rank, 2, stats=stats if rank == 0 else {}, units=units, scan=scan) for rank in (0, 1)]
    merged = cli.gather_rows(parts[0] + parts[1], stats["items"], OneRank, units=units, scan=scan)
    assert merged.confidence is None and merged.mod_llr is None and (merged.units is None) == (not units)
    assert _text(merged.rows) == files["rows"].getvalue()
    assert _text(merged.scores, scan_mod.scores_header(scan["candidates"])) == files["scores"].getvalue()
    if units:
        assert _text(merged.units, cli.UNITS_HEADER) == files["units"].getvalue()
