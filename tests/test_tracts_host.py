"""Tract counting without a GPU: the compound model against nets built from the oracle's pieces (tests/tract_ref.py), the biases,
the rule's checks and the two files, the gather blob and the `count --tracts` plumbing with a stubbed counter, and the two
references on the shared clean reads (tests/test_gpu_tracts.py holds the kernels against them)."""
import io
import math

import numpy as np
import pytest

import tract_ref as tr
from test_anchored_host import _check_hints, _net_edges, _Pm
from test_mod_llr_host import FakeCounter, OneRank


def _flanks(cfg):
    prefix, suffix = cfg["repeat"]["c9orf72"][4:6]
    return prefix[-50:].upper(), suffix[:50].upper()


def _product_model(pm, cfg, name, strand):
    from strique_amd import hmm, tracts
    prefix, suffix = _flanks(cfg)
    units, linkers = tr.MODEL_DEFINITIONS[name]
    un, li = tracts.strand_definition(units, linkers, strand)
    p, s = (prefix, suffix) if strand == '+' else (tr.orc.revcomp(suffix), tr.orc.revcomp(prefix))
    return hmm.CompoundRepeatModel(un, li, p, s, pm, cfg["HMM"])


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tr.MODEL_DEFINITIONS))
@pytest.mark.parametrize("strand", "+-")
def test_baked_model_equals_the_reference_net(pm, opm, cfg, name, strand):
    prefix, suffix = _flanks(cfg)
    units, linkers = tr.MODEL_DEFINITIONS[name]
    got = _product_model(pm, cfg, name, strand)
    ref = tr.model(units, linkers, prefix, suffix, strand, opm, cfg["HMM"])
    b, prep = got.baked, ref["prep"]
    K = len(units)
    assert got.n_tracts == K == ref["K"] and list(got.count_bias) == ref["bias"]
    ne = b.silent_start
    # emitting states: names and emissions, in the same (name) order
    assert list(b.names[:ne]) == list(prep.names[:prep.silent_start])
    for f in ("emis_kind", "emis_a", "emis_b", "emis_c"):
        assert np.array_equal(getattr(b, f), getattr(prep, f)), f
    # counted states: the two dummy states of every loop, each with its tract
    want_counted = ["tract%ddummy%d" % (j, k) for j in range(K) for k in (1, 2)]
    assert [b.names[i] for i in range(b.n_states) if b.count_inc[i]] == [prep.names[i] for i in range(prep.n_states) if prep.count_inc[i]] == want_counted
    assert np.array_equal(got.tract_of[:ne], ref["tract_of"][:ne]) and (got.tract_of[ne:] == -1).all()
    assert [b.names[i] for i in np.nonzero(got.tract_of >= 0)[0]] == want_counted
    # in-edges: every edge of the baked model is an edge of the net (spliced silent states contracted), with the same bits
    label = lambda i: "start" if i == b.start else ("end" if i == b.end else b.names[i])
    have = {}
    for d in range(b.n_states):
        for e in range(b.in_ptr[d], b.in_ptr[d + 1]):
            have[(label(int(b.in_src[e])), label(d))] = float(b.in_logp[e])
    want = _net_edges(ref["net"], prep, set(b.names[ne:]))
    assert have.keys() == want.keys()
    assert all(np.float64(have[key]).tobytes() == np.float64(want[key]).tobytes() for key in want)
    # the sections: K loops, K + 1 profiles with delete states, in the order of the rule
    assert sorted({n[:-len("dummy1")] for n in want_counted}) == ["tract%d" % j for j in range(K)]
    assert {n.rstrip("0123456789dmi") for n in b.names if n not in ("start", "end") and not n.startswith("tract")} <= {"prefix", "suffix"} | {"junction%d" % j for j in range(K - 1)} | {"junction"}
    if (np.asarray(b.hint_slot)[:ne] >= 0).all():
        _check_hints(b)
    assert b.pos_kind is None          # no register-resident image: it has one loop


def test_strand_definition_and_order():
    from strique_amd import tracts
    units, linkers = tr.LOCI["htt_like"]
    assert tracts.strand_definition(units, linkers, '+') == (units, linkers)
    assert tracts.strand_definition(units, linkers, '-') == (("CGG", "CTG"), ("CTGTTG",))
    assert tracts.strand_definition(*tr.LOCI["cnbp_like"], '-') == (("CA", "CAGA", "CAGG"), ("", ""))
    assert tracts.configured_order([1, 2, 3], '+') == (1, 2, 3) and tracts.configured_order([1, 2, 3], '-') == (3, 2, 1)
    for name, (u, l) in tr.MODEL_DEFINITIONS.items():
        for strand in "+-":
            mine = tracts.strand_definition(u, l, strand)
            ref = tr.strand_definition(u, l, "A", "C", strand)
            assert list(mine[0]) == ref[0] and list(mine[1]) == ref[1]
    with pytest.raises(ValueError):
        tracts.strand_definition(units, linkers, '.')


@pytest.mark.parametrize("k", [5, 6, 9])
def test_biases_for_unit_lengths_1_to_12(k):
    """Per tract the flanked model's bias: 2 u - 1 - repeat_offset, whatever the neighbours are."""
    from strique_amd import hmm, tracts
    rng = np.random.default_rng(40 + k)
    nt = lambda n: "".join(rng.choice(list("ACGT"), n))
    prefix, suffix = nt(50), nt(50)
    for L in range(1, 13):
        a, b_, c = nt(L), nt(13 - L), nt(L)
        m = hmm.CompoundRepeatModel((a, b_, c), ("", "ACG"), prefix, suffix, _Pm(k))
        for j, u in enumerate((a, b_, c)):
            flanked = hmm.FlankedRepeatModel(u, prefix, suffix, _Pm(k))
            assert m.count_bias[j] == flanked.count_bias == tracts.bias(u, k) == int(math.ceil(k / len(u)))
            assert m.repeat_offset[j] == flanked.repeat_offset == tracts.repeat_offset(u, k)
            assert tracts.min_units(u, k) == m.count_bias[j] + 1
        net, bias = tr.compound_net([a, b_, c], ["", "ACG"], prefix, suffix, _RefPm(k))
        assert bias == list(m.count_bias)


class _RefPm(object):
    """The oracle-side twin of test_anchored_host._Pm: a k-mer table of any k."""

    def __init__(self, k):
        self.kmer, self.table, self.model_min, self.model_max = k, _Pm(k).model_dict, 50.0, 150.0


# ---- the rule's checks and the files -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("units,linkers", [
    (("CAG",), ()), (("A", "C", "G", "T"), ("", "", "")),                              # K outside 2..3
    (("CAG", "CCG"), ()), (("CAG", "CCG"), ("A", "C")), (("CAG", "CCG", "CTG"), ("A",)),      # a wrong number of linkers
    (("CAG", "CNG"), ("",)), (("CAG", "CCG"), ("A-C",)), (("CAG", "ccx"), ("",)),      # letters beyond ACGT
    (("CAG", ""), ("",)),                                                              # an empty unit
    (("CAG", "CAG"), ("",)), (("CCG", "cag", "CAG"), ("A", "")),                       # adjacent equal units, nothing between them
    ("CAG", ("",)),                                                                    # a string where a list belongs
])
def test_check_rejects(units, linkers):
    from strique_amd import hmm, tracts
    with pytest.raises(ValueError):
        tracts.check(units, linkers)
    if not isinstance(units, str):
        with pytest.raises(ValueError):
            hmm.CompoundRepeatModel(units, linkers, "ACGT" * 13, "TGCA" * 13, _Pm(6))


def test_check_accepts_and_upper_cases():
    from strique_amd import tracts
    assert tracts.check(["cag", "CCG"], ["caacag"]) == (("CAG", "CCG"), ("CAACAG",))
    assert tracts.check(("CAG", "CAG"), ("T",)) == (("CAG", "CAG"), ("T",))          # equal units with a linker between them: two tracts
    assert tracts.check(("CCTG", "TCTG", "TG"), ("", "")) == tr.LOCI["cnbp_like"]


def test_definition_file():
    from strique_amd import tracts
    text = "# compound loci\n\nhtt\tCAG,CCG\tCAACAG\ncnbp\tcctg,TCTG,TG\t-\natxn8\tCTA,CTG\nmix\tCAG,CCG,CAG\t-,T\n"
    got = tracts.parse_definitions(io.StringIO(text), {"htt", "cnbp", "atxn8", "mix", "other"})
    assert got == {"htt": (("CAG", "CCG"), ("CAACAG",)), "cnbp": (("CCTG", "TCTG", "TG"), ("", "")), "atxn8": (("CTA", "CTG"), ("",)),
                   "mix": (("CAG", "CCG", "CAG"), ("", "T"))}
    assert tracts.parse_definitions(io.StringIO(text)) == got          # without a set of targets nothing is unknown
    for bad, why in (("nope\tCAG,CCG\n", "unknown target"), ("htt\tCAG,CCG\nhtt\tCAG,CTG\n", "twice"), ("htt\n", "expected"), ("htt\tCAG,CCG\tA\tB\n", "expected"),
                     ("htt\tCAG\n", "between 2 and 3"), ("htt\tCAG,CCG\tA,C\n", "linkers"), ("htt\tCAG,CXG\n", "letters"), ("htt\tCAG,,CCG\n", "empty unit"),
                     ("htt\tCAG,CAG\t-\n", "one tract"), ("\tCAG,CCG\n", "expected")):
        with pytest.raises(ValueError) as e:
            tracts.parse_definitions(io.StringIO(bad), {"htt"})
        assert why in str(e.value), (bad, str(e.value))


def test_side_file_round_trip():
    from strique_amd import tracts
    recs = [("r1", "htt", "+", 19, ((12, 7), -2319.51263745851)), ("r2", "cnbp", "-", 0, None), ("r3", "cnbp", "-", 13, ((6, 10, 7), -1e-300)),
            ("r4", "htt", "+", 36, ((30, 4), float(np.nextafter(-3051.9, 0))))]
    text = "\t".join(tracts.HEADER) + "\n" + "".join(tracts.format_row(*r) + "\n" for r in recs)
    assert tracts.HEADER == ["ID", "target", "strand", "count", "n_tracts", "tract_counts", "tract_log_p"]
    assert text.splitlines()[1] == "r1\thtt\t+\t19\t2\t12,7\t-2319.51263745851" and text.splitlines()[2] == "r2\tcnbp\t-\t0\t-\t-\t-"
    back = tracts.parse(io.StringIO(text))
    assert back == recs and all(np.float64(a[4][1]).tobytes() == np.float64(b[4][1]).tobytes() for a, b in zip(back, recs) if b[4])
    for bad in ("x\ty\n", "\t".join(tracts.HEADER) + "\nr\tt\t+\t3\t2\t1,2,3\t-1.0\n", "\t".join(tracts.HEADER) + "\nr\tt\t+\t3\t-\t1\t-\n",
                "\t".join(tracts.HEADER) + "\nr\tt\t+\t3\n"):
        with pytest.raises(ValueError):
            tracts.parse(io.StringIO(bad))


# ---- gather, Detected, Merged ------------------------------------------------------------------------------------------------------
def test_output_table_and_compatibility():
    from strique_amd import cli
    from strique_amd.counter import Detected, repeatCounter
    names = [o.name for o in cli.OUTPUTS]
    assert "tracts" in names and names.index("tracts") < names.index("anchored") and names[-1] == "anchored" and cli.Merged._fields[-1] == "anchored"
    assert cli.Merged(None, None, None, None, None).tracts is None          # callers that name five values keep working
    assert Detected._fields[-1] == "tracts" and Detected((0,), None, None, None).tracts is None
    assert Detected((0,), 1, 2, 3, 4, 5, 6, 7).anchored_mod == 7          # the eight positional fields stay where they were
    assert callable(repeatCounter.set_tracts)
    on = cli.outputs_on(tracts=True)
    for v in (((12, 7), -2319.51263745851), ((9, 6, 11), float(np.nextafter(-1.0, 0))), None):
        blob = cli.pack_blob(on, "htt", "+", "-", dict(tracts=v))
        assert blob.count("\t") == 2 + len(cli.OUTPUTS)
        t, s, mod, values = cli.unpack_blob(on, blob)
        assert (t, s, mod) == ("htt", "+", "-") and values["tracts"] == v
        assert v is not None or blob.split("\t")[3 + names.index("tracts")] == "-"          # an absent value is '-'
        assert all(values[n] is None for n in names if n != "tracts")
    # not asked for: '-' whatever the value
    assert cli.pack_blob([], "htt", "+", "-", dict(tracts=((1, 2), -1.0))).split("\t")[3:] == ["-"] * len(cli.OUTPUTS)


class TractCounter(FakeCounter):
    """FakeCounter with the switch of the tract pass: records with a tract value that depends on the inputs only."""
    tracts = False

    def set_tracts(self, on):
        self.tracts = bool(on)

    def detect_batch(self, items, units=False, confidence=False, mod_llr=False, records=False):
        from strique_amd.counter import Detected
        rows = FakeCounter.detect_batch(self, items, units=units, confidence=confidence, mod_llr=mod_llr)
        if not records:
            return rows
        from strique_amd import cli
        out = []
        for (t, raw, s), res in zip(items, rows):
            d = cli.as_detected(res, units, confidence, mod_llr)
            k = len(raw) % 4
            rec = None if (k == 0 or not self.tracts) else (tuple(int(raw[0]) + j for j in range(2 + k % 2)), -1.0 / len(raw) - len(t))
            out.append(d._replace(tracts=rec))
        return out

    def detect(self, t, raw, s, **kw):
        return self.detect_batch([(t, raw, s)], **kw)[0]


@pytest.mark.parametrize("units", [False, True])
def test_count_rows_with_a_stubbed_counter(cfg, units):
    """The tract rows next to the count rows: single process, and through the blob of the gather; count and unit rows byte-identical
    to a run without the flag."""
    from strique_amd import cli, tracts
    loci = {}
    for name, (chrom, b, e, *_r) in cfg["repeat"].items():
        loci.setdefault(chrom, []).append((name, b, e))
    lines = ["@HD\tVN:1.0"]
    for i in range(23):
        chrom, pos = ("chr9", 27570000) if i % 3 else ("chrX", 146990000)
        lines.append("\t".join(["read%d" % i, "16" if i % 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))
    get_raw = lambda q: np.arange(100 + int(q[4:]), 300 + 2 * int(q[4:]))
    log = cli.Log("error")
    plain, uplain = io.StringIO(), io.StringIO()
    cli.run_count(iter(lines), loci, get_raw, TractCounter(), log, 4, 0, 1, plain, units=units, units_out=uplain if units else None)
    counter = TractCounter()
    one, uone, tone, st = io.StringIO(), io.StringIO(), io.StringIO(), {}
    cli.run_count(iter(lines), loci, get_raw, counter, log, 4, 0, 1, one, stats=st, units=units, units_out=uone if units else None, tracts=True, tracts_out=tone)
    assert counter.tracts is False          # the switch belongs to the run
    assert one.getvalue() == plain.getvalue() and uone.getvalue() == uplain.getvalue()
    rows = tracts.parse(io.StringIO(tone.getvalue()))
    counts = [l.split("\t") for l in one.getvalue().splitlines()[1:]]
    assert len(rows) == len(counts) == len(st["tract_rows"]) == 23
    for r, c in zip(rows, counts):
        assert list(r[:3]) == c[:3] and str(r[3]) == c[3]
    assert any(r[4] is None for r in rows) and {len(r[4][0]) for r in rows if r[4]} == {2, 3}
    # several ranks: the same rows out of the gather's blob
    st2 = {}
    mine = cli.run_count(iter(lines), loci, get_raw, TractCounter(), log, 4, 0, 2, stats=st2, units=units, tracts=True)
    other = cli.run_count(iter(lines), loci, get_raw, TractCounter(), log, 4, 1, 2, stats={}, units=units, tracts=True)
    got = cli.gather_rows(mine + other, st2["items"], OneRank, units=units, tracts=True)
    buf = io.StringIO(); cli.write_rows(buf, got.rows)
    tbuf = io.StringIO(); cli.write_rows(tbuf, got.tracts, header=tracts.HEADER)
    assert buf.getvalue() == plain.getvalue() and tbuf.getvalue() == tone.getvalue()
    assert (got.units is None) == (not units) and got.anchored is None and got.variants is None
    assert cli.gather_rows(mine + other, st2["items"], OneRank, units=units).tracts is None
    with pytest.raises(ValueError):
        cli.run_count(["r"], loci, get_raw, TractCounter(), log, 4, tracts=True, scan={"min_score": 5.0, "candidates": [], "scores": False})


def test_count_flags_need_each_other(tmp_path):
    from strique_amd import cli
    base = ["count", str(tmp_path / "reads.fofn"), str(tmp_path / "m.model"), str(tmp_path / "repeat.tsv")]
    for extra in (["--tracts", "t.tsv"], ["--tract-units", "d.tsv"],
                  ["--tracts", "t.tsv", "--tract-units", "d.tsv", "--scan", "--scan-min-score", "5"]):
        with pytest.raises(SystemExit):
            cli.main(base + extra)


# ---- the references ---------------------------------------------------------------------------------------------------------------
def test_references_agree_on_the_shared_cases(opm, cfg):
    prefix, suffix = _flanks(cfg)
    shared = tr.cases(opm, prefix, suffix, cfg["HMM"])
    assert len(shared) == len(tr.RECORDED_ERROR) == 8 and {c[1] for c in shared} == {"+", "-"} and {c[4]["K"] for c in shared} == {2, 3}
    for name, strand, planted, x, m in shared:
        a = tr.decode_a(m["prep"], m["tract_of"], m["K"], x)
        b = tr.decode_b(m["prep"], m["tract_of"], m["K"], x)
        assert a[2] == 0 and a[1:] == b[1:] and np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes(), (name, strand, planted, a, b)
        counts = tr.configured([v + q for v, q in zip(a[1], m["bias"])], strand)
        # recorded from the reference (it is deterministic): this pins the model definition, it is no claim of accuracy
        assert tuple(c - p for c, p in zip(counts, planted)) == tr.RECORDED_ERROR[(name, strand, planted)], (name, strand, planted, counts)
        # a window shorter than any path
        assert tr.decode_a(m["prep"], m["tract_of"], m["K"], x[:2])[2] == 1 and tr.decode_b(m["prep"], m["tract_of"], m["K"], x[:2])[2] == 1


def test_baked_model_decodes_like_the_net(pm, opm, cfg):
    """bake() only splices certain silent states: the baked arrays give the net's bits and counts on the shared reads."""
    prefix, suffix = _flanks(cfg)
    for name, strand, planted, x, m in tr.cases(opm, prefix, suffix, cfg["HMM"]):
        cm = _product_model(pm, cfg, name, strand)
        a = tr.decode_a(m["prep"], m["tract_of"], m["K"], x)
        b = tr.decode_a(cm.baked, cm.tract_of, cm.n_tracts, x)
        assert a[1:] == b[1:] and np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes(), (name, strand, planted)
