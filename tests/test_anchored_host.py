"""Anchored counting without a GPU: the two models against nets built from the oracle's pieces (tests/anchored_ref.py), their count
biases, the rule, the CPU preconditions on the very reads the GPU tests use (tests/test_gpu_anchored.py), and the `count --anchored`
plumbing with a stubbed counter."""
import io
import math

import numpy as np
import pytest

import anchored_ref as ar
from test_mod_llr_host import FakeCounter, OneRank


# ---- models ---------------------------------------------------------------------------------------------------------------------
def _net_edges(net, prep, keep):
    """In-edges {(source name, target name): log-probability} of a prepared net with every silent state outside `keep` spliced out
    -- such a state must have one certain out-edge, as the states bake() splices have."""
    n = prep.n_states
    out_of = {}
    for b in range(n):
        for e in range(prep.in_ptr[b], prep.in_ptr[b + 1]):
            out_of.setdefault(int(prep.in_src[e]), []).append((b, float(prep.in_logp[e])))
    kept = lambda i: i < prep.silent_start or i in (prep.start, prep.end) or prep.names[i] in keep

    def target(b):
        while not kept(b):
            assert len(out_of[b]) == 1 and out_of[b][0][1] == 0.0, prep.names[b]
            b = out_of[b][0][0]
        return b
    label = lambda i: "start" if i == prep.start else ("end" if i == prep.end else prep.names[i])
    edges = {}
    for a, outs in out_of.items():
        if not kept(a):
            continue
        for b, lp in outs:
            key = (label(a), label(target(b)))
            edges[key] = max(lp, edges.get(key, -math.inf))
    return edges


@pytest.mark.parametrize("name", ar.TARGETS)
@pytest.mark.parametrize("strand", "+-")
@pytest.mark.parametrize("kind", ["ends_in_repeat", "starts_in_repeat"])
def test_baked_models_equal_the_reference_nets(pm, opm, cfg, name, strand, kind):
    from strique_amd import hmm
    target = tuple(cfg["repeat"][name][3:6])
    r, p, s, _, _ = ar.strand_sequences(*target, strand)
    got = hmm.AnchoredRepeatModel(kind, r, p, s, pm, cfg["HMM"])
    b = got.baked
    k = ar.ENDS if kind == "ends_in_repeat" else ar.STARTS
    ref = ar.models(*target, strand, opm, cfg["HMM"])
    prep, bias = ref[k]
    assert got.count_bias == bias
    ne = b.silent_start
    # emitting states: names and emissions, in the same (name) order
    assert list(b.names[:ne]) == list(prep.names[:prep.silent_start])
    for f in ("emis_kind", "emis_a", "emis_b", "emis_c"):
        assert np.array_equal(getattr(b, f), getattr(prep, f)), f
    # counted states and the tag
    assert [b.names[i] for i in range(b.n_states) if b.count_inc[i]] == [prep.names[i] for i in range(prep.n_states) if prep.count_inc[i]] == ["repeatdummy1", "repeatdummy2"]
    assert [bool(t) for t in b.tag] == ["repeat" in n for n in b.names]
    # in-edges: every edge of the baked model is an edge of the net (spliced states contracted), with the same bits
    label = lambda i: "start" if i == b.start else ("end" if i == b.end else b.names[i])
    have = {}
    for d in range(b.n_states):
        for e in range(b.in_ptr[d], b.in_ptr[d + 1]):
            have[(label(int(b.in_src[e])), label(d))] = float(b.in_logp[e])
    want = _net_edges(ref["nets"][k], prep, set(b.names[ne:]))
    assert have.keys() == want.keys()
    assert all(np.float64(have[key]).tobytes() == np.float64(want[key]).tobytes() for key in want)
    # the free state: a self-loop, at least one observation, nothing else new; no in-degree above the flanked model's
    free = "tail" if k == ar.ENDS else "head"
    assert have[(free, free)] == math.log(0.999)
    flanked = hmm.FlankedRepeatModel(r, p, s, pm, cfg["HMM"]).baked
    assert max(np.diff(b.in_ptr)) <= max(np.diff(flanked.in_ptr))
    assert b.in_ptr[b.end + 1] - b.in_ptr[b.end] == (1 if k == ar.ENDS else flanked.in_ptr[flanked.end + 1] - flanked.in_ptr[flanked.end])
    _check_hints(b)
    assert b.pos_kind is not None


def _check_hints(b):
    """The layout hints of a baked model are what strq_model_create takes: every emitting state in a lane of its own, in a slot the
    model has (64 states per slot)."""
    ne = b.silent_start
    slots, lanes = np.asarray(b.hint_slot)[:ne], np.asarray(b.hint_lane)[:ne]
    assert (slots >= 0).all() and (slots < (ne + 63) // 64).all() and (lanes >= 0).all() and (lanes < 64).all()
    assert len({(int(x), int(y)) for x, y in zip(slots, lanes)}) == ne


class _AnyKmer(dict):
    """A k-mer table of any k: levels from a hash of the k-mer."""

    def __missing__(self, kmer):
        h = sum((i + 1) * ord(c) for i, c in enumerate(kmer))
        self[kmer] = (70.0 + (h * 37) % 60, 1.0 + (h % 5) * 0.25)
        return self[kmer]


class _Pm(object):
    def __init__(self, k):
        self.kmer, self.model_dict, self.model_min, self.model_max = k, _AnyKmer(), 50.0, 150.0


@pytest.mark.parametrize("k", [5, 6, 9])
def test_count_biases_for_unit_lengths_1_to_12(k):
    from strique_amd import hmm
    rng = np.random.default_rng(k)
    nt = lambda n: "".join(rng.choice(list("ACGT"), n))
    for L in range(1, 13):
        repeat, prefix, suffix = nt(L), nt(50), nt(50)
        units = int(math.ceil(k / L))
        flanked = hmm.FlankedRepeatModel(repeat, prefix, suffix, _Pm(k))
        assert flanked.count_bias == units
        ends = hmm.AnchoredRepeatModel("ends_in_repeat", repeat, prefix, suffix, _Pm(k))
        starts = hmm.AnchoredRepeatModel("starts_in_repeat", repeat, prefix, suffix, _Pm(k))
        assert ends.count_bias == flanked.count_bias - units - 1 == -1
        assert starts.count_bias == flanked.count_bias - 1 == units - 1
    with pytest.raises(ValueError):
        hmm.AnchoredRepeatModel("spanning", "CAG", nt(50), nt(50), _Pm(6))


def test_layout_hints_wherever_the_flanked_model_has_them():
    """A target whose flanked model runs on a lane layout must not lose it with these models: the free state needs a lane more,
    and where the flanked layout fills all 64 lanes of its slots it goes to a third slot."""
    from strique_amd import hmm
    rng = np.random.default_rng(64)
    nt = lambda n: "".join(rng.choice(list("ACGT"), n))
    full = 0
    for L in range(1, 13):
        for flank in (40, 50, 51, 52, 53, 54, 55, 56):
            repeat, prefix, suffix = nt(L), nt(flank), nt(flank)
            flanked = hmm.FlankedRepeatModel(repeat, prefix, suffix, _Pm(6)).graph.layout
            P = flank + int(math.ceil(6 / L)) * L - 1 - 5
            R = len(hmm.extend_repeat(repeat, 6)[0]) - 5
            for kind in hmm.ANCHORED_KINDS:
                m = hmm.AnchoredRepeatModel(kind, repeat, prefix, suffix, _Pm(6))
                if flanked:
                    assert m.graph.layout, (L, flank, kind)
                if m.graph.layout:
                    _check_hints(m.baked)
                    full += kind == "ends_in_repeat" and P + R == 63
    assert full >= 1          # the edge itself was among them: 64 lanes taken, the free state in the third slot


# ---- rule -----------------------------------------------------------------------------------------------------------------------
def test_rule():
    from strique_amd import anchored as an
    m, n = 6.5, 1000
    up = float(np.nextafter(m, 10.0)); down = float(np.nextafter(m, 0.0))
    cl = lambda sp, ss, pb=100, se=900, status=0, n_=n, m_=m: an.classify(status, n_, sp, ss, pb, se, m_)
    assert cl(9.0, 9.0) == (an.SPANNING, 100, 900)
    assert cl(m, m) == (an.SPANNING, 100, 900)                    # equality at m: found
    assert cl(m, down) == (an.ENDS_IN_REPEAT, 100, n)
    assert cl(down, m) == (an.STARTS_IN_REPEAT, 0, 900)
    assert cl(up, 3.0) == (an.ENDS_IN_REPEAT, 100, n) and cl(down, 3.0) == (an.NONE, 0, 0)
    assert cl(9.0, 9.0, pb=900, se=100) == (an.NONE, 0, 0)          # both found, wrong order
    assert cl(9.0, 9.0, pb=500, se=500) == (an.NONE, 0, 0)
    nan = float("nan")
    for sp, ss in ((nan, 9.0), (9.0, nan), (nan, nan), (nan, 1.0), (1.0, nan)):
        assert cl(sp, ss) == (an.NONE, 0, 0)
    assert cl(9.0, 1.0, status=1) == (an.NONE, 0, 0)                # a read that could not be normalised
    assert cl(9.0, 1.0, n_=0) == (an.NONE, 0, 0)
    assert cl(0.0, 0.0) == (an.NONE, 0, 0) and cl(-1.0, 9.0) == (an.STARTS_IN_REPEAT, 0, 900)
    assert cl(9.0, 1.0, pb=n) == (an.NONE, 0, 0) and cl(1.0, 9.0, se=0) == (an.NONE, 0, 0) and cl(1.0, 9.0, se=n) == (an.STARTS_IN_REPEAT, 0, n)
    for bad in (0.0, -1.0, nan):
        with pytest.raises(ValueError):
            cl(9.0, 9.0, m_=bad)
    # the same rule as the reference helper states it, on a grid
    vals = [nan, -1.0, 0.0, 3.0, down, m, up, 9.0]
    for sp in vals:
        for ss in vals:
            for pb, se in ((100, 900), (900, 100), (0, n), (-1, n + 1)):
                for status in (0, 1):
                    assert cl(sp, ss, pb, se, status) == ar.classify(status, n, sp, ss, pb, se, m), (sp, ss, pb, se, status)
    assert an.free_samples(an.ENDS_IN_REPEAT, 100, 10, 89) == 10 and an.free_samples(an.STARTS_IN_REPEAT, 100, 10, 89) == 10
    assert (an.NONE, an.SPANNING, an.ENDS_IN_REPEAT, an.STARTS_IN_REPEAT) == (ar.NONE, ar.SPANNING, ar.ENDS, ar.STARTS) == (0, 1, 2, 3)


# ---- preconditions on the shared reads (conditions, not measurements: the seed was chosen so that the oracle meets them) ---------
@pytest.mark.parametrize("as_int16", [True, False])
def test_cpu_preconditions_on_the_shared_reads(tables, cfg, as_int16):
    got = ar.cases(tables, cfg, as_int16)
    assert len(got) == 4 * 7
    for name, strand, cut, sig, kind, complete, row, rec in got:
        what = (name, strand, cut, row, rec)
        assert 9000 <= len(sig) <= 13500, what
        present, absent = (row[1], row[2]) if kind == ar.ENDS else (row[2], row[1])
        assert present >= 7.5 and absent <= 5.5, what
        assert rec[0] == kind and rec[1] == 0, what
        lo = complete - 2 if kind == ar.ENDS else complete - 1
        assert lo <= rec[2] <= complete, what
        assert 0 <= rec[6] <= 64, what
        assert 0 <= rec[4] < rec[5] <= len(sig), what


# ---- file format, blob, CLI ----------------------------------------------------------------------------------------------------
RECORDS = [(2, 0, 42, -4229.255537715763, 10137, 12060, 25), (3, 0, 0, -0.1 - 0.2, 0, 1, 0), (2, 1, 0, 0.0, 0, 0, 0), (3, 2, 0, 0.0, 0, 0, 0),
           (1, 0, 0, 0.0, 0, 0, 0), (0, 0, 0, 0.0, 0, 0, 0), None]


def test_format_parse_round_trip():
    from strique_amd import anchored as an
    text = "\t".join(an.HEADER) + "\n" + "".join(an.format_row("read%d" % i, "c9orf72", "+-"[i % 2], r) + "\n" for i, r in enumerate(RECORDS))
    rows = an.parse(io.StringIO(text))
    assert len(rows) == len(RECORDS)
    for i, (r, (rid, target, strand, kind, dec)) in enumerate(zip(RECORDS, rows)):
        assert (rid, target, strand) == ("read%d" % i, "c9orf72", "+-"[i % 2])
        assert kind == an.KIND_NAMES[0 if r is None else r[0]]
        if r is not None and r[0] in (2, 3) and r[1] == 0:
            assert dec == (r[2], r[3], r[4], r[5], r[6]) and np.float64(dec[1]).tobytes() == np.float64(r[3]).tobytes()
        else:
            assert dec is None and text.splitlines()[1 + i].split("\t")[4:] == ["-"] * 5
    with pytest.raises(ValueError):
        an.parse(io.StringIO("ID\tx\n"))
    with pytest.raises(ValueError):
        an.parse(io.StringIO("\t".join(an.HEADER) + "\nr\tt\t+\tsideways\t-\t-\t-\t-\t-\n"))


def test_blob_carries_the_record():
    from strique_amd import cli
    assert [o.name for o in cli.OUTPUTS][-1] == "anchored" and cli.Merged._fields[-1] == "anchored"
    assert cli.Merged(None, None, None, None, None).anchored is None          # callers that name five values keep working
    assert cli.Detected((0,), None, None, None).anchored is None
    on = cli.outputs_on(units=True, anchored=True)
    assert [o.name for o in on] == ["units", "anchored"]
    for rec in RECORDS:
        blob = cli.pack_blob(on, "fmr1", "-", "-", dict(units=np.array([5, 9]), anchored=rec))
        assert blob.count("\t") == 2 + len(cli.OUTPUTS)
        t, s, m, got = cli.unpack_blob(on, blob)
        assert (t, s, m) == ("fmr1", "-", "-") and got["units"] == [5, 9]
        assert got["anchored"] == rec and (rec is None or np.float64(got["anchored"][3]).tobytes() == np.float64(rec[3]).tobytes())
    off = cli.outputs_on(units=True)
    assert cli.unpack_blob(off, cli.pack_blob(off, "fmr1", "-", "-", dict(anchored=RECORDS[0])))[3]["anchored"] is None


class AnchoredCounter(FakeCounter):
    """FakeCounter that also answers anchored=..., records=True: the record depends on the inputs only."""
    asked = None

    def detect_batch(self, items, units=False, confidence=False, mod_llr=False, anchored=None, records=False):
        from strique_amd.counter import Detected
        plain = FakeCounter.detect_batch(self, items, units=units, confidence=confidence, mod_llr=mod_llr)
        if anchored is None:
            assert not records
            return plain
        assert records
        type(self).asked = anchored
        out = []
        for (t, raw, s), res in zip(items, plain):
            rest = iter(res[1:]) if (units or confidence or mod_llr) else iter(())
            row = res[0] if (units or confidence or mod_llr) else res
            k = len(raw) % 4
            rec = (k, len(raw) % 3 == 0 and k >= 2, len(raw) % 50, -1.0 / len(raw), int(raw[0]), int(raw[0]) + 100, len(raw) % 7) if k else (0, 0, 0, 0.0, 0, 0, 0)
            rec = tuple(int(x) if i != 3 else float(x) for i, x in enumerate(rec))
            out.append(Detected(row, next(rest) if units else None, next(rest) if confidence else None, next(rest) if mod_llr else None, rec))
        return out


    def detect(self, t, raw, s, units=False, confidence=False, mod_llr=False, anchored=None, records=False):
        return self.detect_batch([(t, raw, s)], units=units, confidence=confidence, mod_llr=mod_llr, anchored=anchored, records=records)[0]


class BatchesFail(AnchoredCounter):
    """Every batch of more than one read is rejected; read13 fails on its own too."""

    def detect_batch(self, items, **kw):
        if len(items) > 1 or len(items[0][1]) == 200 + 2 * 13 - 13:
            raise RuntimeError("bad batch")
        return AnchoredCounter.detect_batch(self, items, **kw)


def test_the_counters_detect_takes_what_run_count_passes():
    """run_count retries a rejected batch read by read through counter.detect(t, raw, s, **extras): the product's detect must
    take every keyword its detect_batch takes."""
    import inspect
    from strique_amd.counter import repeatCounter
    batch = set(inspect.signature(repeatCounter.detect_batch).parameters) - {"self", "items"}
    one = set(inspect.signature(repeatCounter.detect).parameters) - {"self", "target_name", "raw_signal", "strand"}
    assert batch == one and {"anchored", "records"} <= one
    assert set(inspect.signature(AnchoredCounter.detect).parameters) - {"self", "t", "raw", "s"} == one


@pytest.mark.parametrize("units,confidence", [(False, False), (True, True)])
def test_a_rejected_batch_keeps_its_good_reads(cfg, units, confidence):
    """A batch the counter rejects is retried read by read: with the switch on, the count rows, the side files and the anchored
    file still carry every read but the one that fails on its own -- the bytes of a run whose batches go through, less that read."""
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

    def run(counter):
        f = {k: io.StringIO() for k in ("rows", "units", "confidence", "anchored")}
        stats = {}
        cli.run_count(iter(lines), loci, get_raw, counter, lambda *a, **k: None, 4, 0, 1, f["rows"], stats=stats, units=units, confidence=confidence,
                      units_out=f["units"] if units else None, conf_out=f["confidence"] if confidence else None, anchored=6.5, anchored_out=f["anchored"])
        return {k: v.getvalue() for k, v in f.items()}, stats
    good, st0 = run(AnchoredCounter())
    got, st1 = run(BatchesFail())
    assert st0["failed"] == 0 and st1["failed"] == 1
    for name in ("rows", "anchored") + (("units",) if units else ()) + (("confidence",) if confidence else ()):
        want = [l for l in good[name].splitlines() if not l.startswith("read13\t")]
        assert len(want) == 23 and got[name].splitlines() == want, name


@pytest.mark.parametrize("units,confidence", [(False, False), (True, True)])
def test_count_rows_with_a_stubbed_counter(cfg, units, confidence):
    """The anchored rows next to the count rows: single process, and through the blob of the gather; the count TSV and the other
    side files byte-identical to a run without the switch."""
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
    kw = dict(units=units, confidence=confidence)

    def run(counter, **more):
        f = {k: io.StringIO() for k in ("rows", "units", "confidence", "anchored")}
        cli.run_count(iter(lines), loci, get_raw, counter, log, 4, 0, 1, f["rows"], units_out=f["units"] if units else None,
                      conf_out=f["confidence"] if confidence else None, **kw, **more)
        return f
    plain = run(FakeCounter())
    files = run(AnchoredCounter(), anchored=6.5, anchored_out=None)
    with_file = io.StringIO()
    on = run(AnchoredCounter(), anchored=6.5, anchored_out=with_file)
    assert AnchoredCounter.asked == 6.5
    for name in ("rows", "units", "confidence"):
        assert plain[name].getvalue() == files[name].getvalue() == on[name].getvalue(), name
    assert len(plain["rows"].getvalue().splitlines()) == 24
    rows = an.parse(io.StringIO(with_file.getvalue()))
    count_rows = [l.split("\t") for l in plain["rows"].getvalue().splitlines()[1:]]
    assert [(r[0], r[1], r[2]) for r in rows] == [tuple(c[:3]) for c in count_rows]
    assert {r[3] for r in rows} == set(an.KIND_NAMES) and any(r[4] is None and r[3] == "ends_in_repeat" for r in rows)
    # two ranks, one gather: the same bytes
    stats = {}
    parts = [cli.run_count(iter(lines), loci, get_raw, AnchoredCounter(), log, 4, rank, 2, stats=stats if rank == 0 else {}, anchored=6.5, **kw) for rank in (0, 1)]
    merged = cli.gather_rows(parts[1] + parts[0], stats["items"], OneRank, anchored=True, **kw)
    text = lambda rows_, header: (lambda b: (cli.write_rows(b, rows_, header=header), b.getvalue())[1])(io.StringIO())
    assert text(merged.rows, True) == plain["rows"].getvalue()
    assert text(merged.anchored, an.HEADER) == with_file.getvalue()
    if units:
        assert text(merged.units, cli.UNITS_HEADER) == plain["units"].getvalue()
    with pytest.raises(ValueError):
        cli.run_count(["read1"], {}, get_raw, AnchoredCounter(), log, 4, 0, 1, io.StringIO(), anchored=6.5,
                      scan={"min_score": 5.0, "candidates": [("c9orf72", "+")], "scores": False})


@pytest.mark.parametrize("argv,needle", [
    (["--anchored", "a.tsv"], "--anchored-min-score"),
    (["--anchored-min-score", "6.5"], "needs --anchored"),
    (["--anchored", "a.tsv", "--anchored-min-score", "0"], "above 0"),
    (["--anchored", "a.tsv", "--anchored-min-score", "-2"], "above 0"),
    (["--anchored", "a.tsv", "--anchored-min-score", "6.5", "--scan", "--scan-min-score", "5"], "--scan"),
])
def test_argument_errors(capsys, argv, needle):
    from strique_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.count(["reads.fofn", "r9.model", "repeats.tsv"] + argv)
    assert e.value.code == 2 and needle in capsys.readouterr().err
