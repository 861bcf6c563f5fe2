"""Flank methylation calls through the detect pipeline (strq_set_flank_mod, repeatCounter.set_flank_mod) against
tests/flank_mod_ref.py: the reads of tests/test_gpu_flank_mod_models.py -- C9orf72 and HTT with their 150-nt flanks, both strands,
base-table and mCpG-table reads, int16 for both targets and float64 for C9orf72.  flank, pos, n_sites, n_columns, status, begin and
end are compared exactly, v_base and v_mod to the bit; ties as in the model-level test (at most 2 % of the pairs).  Then: a read
whose gate fails and a target without a modification model (None), sub-batches and three pieces of back-pointers against the
single-piece run, and the rows and the other passes' outputs with the switch on and off."""
import numpy as np
import pytest

import flank_mod_ref as fr

pytestmark = pytest.mark.gpu
NAMES = ("c9orf72", "htt")


class _Arrays(object):
    def __init__(self, model):
        self.__dict__.update(model.baked._asdict()); self.column_of = model.column_of


@pytest.fixture(scope="module")
def counter(pm, pm_mod, cfg, targets):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in NAMES:
        rc.add_target(name, *targets[name])
    return rc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _run(counter, items, on=True, **kw):
    """(Detected records, structured records per read or None, strq_last_flank_mod) of one batch."""
    counter.set_flank_mod(on)
    try:
        got = counter.detect_batch(items, records=True, **kw)
        recs = counter.ctx.batch_fetch_flank_mod() if on else None
        return got, recs, counter.ctx.last_flank_mod()
    finally:
        counter.set_flank_mod(False)


def _frozen(recs):
    return [None if r is None else r.tobytes() for r in recs]


def _configured(which, sites, L, strand):
    return (which, sites[0]) if strand == "+" else (1 - which, L - 2 - sites[-1])


@pytest.mark.parametrize("names,as_int16", [(NAMES, True), (("c9orf72",), False)])
def test_records_equal_the_reference(counter, pm, tables, cfg, targets, names, as_int16):
    from strique_amd import hmm
    cases, opm, opm_mod = fr.cases(tables, cfg, targets, names, as_int16)
    items = [(c["target"], c["sig"], c["strand"]) for c in cases]
    got, recs, last = _run(counter, items)
    print("flank-mod pass:", last)
    pairs = ties = scored = 0
    for c, d, rec in zip(cases, got, recs):
        what = (c["target"], c["strand"], c["table"])
        assert rec is not None and d.flank_mod is not None, what
        want = []
        for which, flank, b, e, x in c["flanks"]:
            ref = fr.call(x, flank, opm, opm_mod, cfg["HMM"], alt=_Arrays(hmm.FlankProfileModel(flank, pm, cfg["HMM"])))
            for r in ref:
                cf, pos = _configured(which, r["sites"], len(flank), c["strand"])
                s = r["status"] == fr.SCORED
                want.append((r["tie"], (cf, pos, len(r["sites"]), r["n_columns"], r["status"], b + r["u"] if s else -1, b + r["w"] if s else -1), (r["v_base"], r["v_mod"])))
        assert len(rec) == len(want) == len(d.flank_mod), (what, len(rec), len(want))
        for g, t, (tie, fields, v) in zip(rec, d.flank_mod, want):
            pairs += 1
            assert (int(g["flank"]), int(g["pos"]), int(g["n_sites"]), int(g["n_columns"])) == fields[:4], (what, g, fields)
            if tie:
                ties += 1
                continue
            assert (int(g["status"]), int(g["begin"]), int(g["end"])) == fields[4:], (what, g, fields)
            assert _bits([g["v_base"], g["v_mod"]]) == _bits(v), (what, g, v)
            assert t[:7] == fields and _bits(t[7]) == _bits(g["v_mod"] - g["v_base"]), (what, t)
            scored += fields[4] == fr.SCORED
    assert ties <= fr.TIE_CAP * pairs and scored >= 0.75 * pairs
    assert last["flanks"] == 2 * len(cases) and last["groups"] >= scored and last["launches"] >= 5 and last["ms"] > 0
    # the switch off: the same rows, nothing launched, nothing to fetch
    off, _, last0 = _run(counter, items, on=False)
    assert last0 == {"ms": 0.0, "flanks": 0, "groups": 0, "launches": 0}
    assert [d.row for d in off] == [d.row for d in got] and all(d.flank_mod is None for d in off)
    from strique_amd import ffi
    with pytest.raises(ffi.StriqueHipError) as e:
        counter.ctx.batch_fetch_flank_mod()
    assert e.value.code == ffi.STRQ_ERR_ARG and "strq_set_flank_mod" in str(e.value)


def test_sub_batches_and_pieces(counter, tables, cfg, targets):
    cases, _, _ = fr.cases(tables, cfg, targets, NAMES, True)
    items = [(c["target"], c["sig"], c["strand"]) for c in cases]
    _, one, last1 = _run(counter, items)
    ctx = counter.ctx
    # a flank's back-pointers are ~1 MB: a cap of a third of the total cuts three pieces and more
    per_flank = 1200 * 437 * 2
    try:
        ctx.set_option("STRQ_FLANK_MOD_WS_BYTES", str(per_flank * len(items) * 2 // 3))
        _, pieces, last3 = _run(counter, items)
        ctx.set_option("STRQ_FLANK_MOD_WS_BYTES", None)
        ctx.set_option("STRQ_SUBBATCH_READS", "3")
        _, subs, lasts = _run(counter, items)
    finally:
        ctx.set_option("STRQ_FLANK_MOD_WS_BYTES", None); ctx.set_option("STRQ_SUBBATCH_READS", None)
    assert _frozen(pieces) == _frozen(one) and _frozen(subs) == _frozen(one)
    assert last3["launches"] >= last1["launches"] + 2 * 4 and lasts["launches"] > last1["launches"]
    assert last3["flanks"] == lasts["flanks"] == last1["flanks"] and last3["groups"] == lasts["groups"] == last1["groups"]


def test_gate_and_targets_without_models(counter, pm, pm_mod, cfg, targets, tables):
    from strique_amd import synth
    from strique_amd.counter import repeatCounter
    cases, _, _ = fr.cases(tables, cfg, targets, NAMES, True)
    good = cases[0]
    # suffix in front of the prefix: the gate fails
    repeat, prefix, suffix = targets["c9orf72"]
    rng = np.random.default_rng(9)
    back = "".join(rng.choice(list("ACGT"), 2400))
    swapped = synth.make_signal(rng, synth.KmerTable(pm_mod), (back[:800] + suffix + back[800:1600] + prefix + back[1600:]).encode())
    got, recs, last = _run(counter, [(good["target"], good["sig"], good["strand"]), ("c9orf72", swapped, "+")])
    assert got[1].row[0] == 0 and recs[1] is None and got[1].flank_mod is None and recs[0] is not None and last["flanks"] == 2
    # a counter without a modification model has no switch; a scan refuses the pass
    plain = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], context=counter.ctx)
    with pytest.raises(ValueError, match="modification model"):
        plain.set_flank_mod(True)
    # ... and a target of the context without the models gives None while the switch is on
    plain.add_target("bare", *targets["c9orf72"])
    ctx = counter.ctx
    ctx.set_flank_mod(True)
    try:
        plain.detect_batch([("bare", good["sig"], good["strand"])])
        assert ctx.last_flank_mod()["flanks"] == 0 and ctx.batch_fetch_flank_mod() == [None]
    finally:
        ctx.set_flank_mod(False)


def test_other_passes_are_untouched(counter, tables, cfg, targets):
    """units, confidence and per-unit scores with the flank switch on and off: rows and every other fetch byte-equal; the flank
    records equal with the other switches on and off."""
    cases, _, _ = fr.cases(tables, cfg, targets, NAMES, True)
    items = [(c["target"], c["sig"], c["strand"]) for c in cases]
    kw = dict(units=True, confidence=True, mod_llr=True)
    on, recs_on, _ = _run(counter, items, **kw)
    off, _, _ = _run(counter, items, on=False, **kw)
    _, alone, _ = _run(counter, items)

    def frozen(ds):
        return [(d.row[:3], _bits(d.row[3]), d.row[4:], None if d.units is None else _bits(d.units), None if d.conf is None else _bits(d.conf),
                 None if d.llr is None else _bits(d.llr)) for d in ds]
    assert frozen(on) == frozen(off) and any(d.llr is not None for d in on)
    assert _frozen(recs_on) == _frozen(alone)


def _want(c, pm, opm, opm_mod, cfg):
    """[(tie, (flank, pos, n_sites, n_columns, status, begin, end), (v_base, v_mod))] of one case of flank_mod_ref.cases."""
    from strique_amd import hmm
    want = []
    for which, flank, b, e, x in c["flanks"]:
        for r in fr.call(x, flank, opm, opm_mod, cfg["HMM"], alt=_Arrays(hmm.FlankProfileModel(flank, pm, cfg["HMM"]))):
            cf, pos = _configured(which, r["sites"], len(flank), c["strand"])
            s = r["status"] == fr.SCORED
            want.append((r["tie"], (cf, pos, len(r["sites"]), r["n_columns"], r["status"], b + r["u"] if s else -1, b + r["w"] if s else -1), (r["v_base"], r["v_mod"])))
    return want


def test_too_long_stretches_are_not_decoded(counter, tables, cfg, targets):
    """The pass's own too_long branch, reached with the test option STRQ_FLANK_MOD_MAX_STRETCH (observations per flank base, the
    rule's 64): at 8 a 150-nt flank of more than 1200 observations gets too_long records and is neither sized nor decoded; every
    other flank of the batch has the records of the plain run."""
    cases, _, _ = fr.cases(tables, cfg, targets, NAMES, True)
    items = [(c["target"], c["sig"], c["strand"]) for c in cases]
    _, plain, last = _run(counter, items)
    long_ = [[e - b > 8 * len(flank) for _, flank, b, e, _ in c["flanks"]] for c in cases]
    n_long = sum(sum(f) for f in long_)
    assert 1 <= n_long < len(cases), long_
    ctx = counter.ctx
    try:
        ctx.set_option("STRQ_FLANK_MOD_MAX_STRETCH", "8")
        _, capped, lastc = _run(counter, items)
    finally:
        ctx.set_option("STRQ_FLANK_MOD_MAX_STRETCH", None)
    assert lastc["flanks"] == last["flanks"] - n_long and lastc["groups"] < last["groups"]
    for c, a, b, fl in zip(cases, plain, capped, long_):
        n0 = len(fr.groups(c["flanks"][0][1], 6))
        for part, is_long in ((slice(0, n0), fl[0]), (slice(n0, None), fl[1])):
            if not is_long:
                assert a[part].tobytes() == b[part].tobytes()
                continue
            for g, h in zip(a[part], b[part]):
                assert (int(h["status"]), int(h["begin"]), int(h["end"])) == (fr.TOO_LONG, -1, -1) and np.isnan(h["v_base"]) and np.isnan(h["v_mod"])
                assert [int(h[k]) for k in ("flank", "pos", "n_sites", "n_columns")] == [int(g[k]) for k in ("flank", "pos", "n_sites", "n_columns")]


def test_edge_and_skipped_through_the_pipeline(pm, pm_mod, cfg, targets, orc, opm, opm_mod):
    """A constructed target whose prefix starts with CG and whose suffix ends with it, and a read that breaks off three bases before
    the end of the suffix: the first group of the prefix is `edge`, the last group of the suffix -- its one k-mer is not in the read
    -- is `skipped`; both get score tasks without a passage on the device, and every record equals the reference."""
    from strique_amd import synth
    from strique_amd.counter import repeatCounter
    repeat, prefix, suffix = targets["c9orf72"]
    suffix2 = suffix[:-2] + "CG"
    assert prefix.upper().startswith("CG")
    rng = np.random.Generator(np.random.PCG64(7101))
    back = "".join(rng.choice(list("ACGT"), 2500))
    sig = synth.make_signal(rng, synth.KmerTable(pm), (back + prefix + repeat * 15 + suffix2[:-3]).upper().encode(), True, 0.0)
    tc = orc.classifier(repeat, prefix, suffix2, "+", opm, None, cfg["HMM"])
    (pb, pe), (sb, se) = fr.flank_ranges(sig, tc, opm, orc.align_params(cfg["align"]))
    case = dict(strand="+", flanks=[(0, prefix.upper(), pb, pe, fr.stretch(sig, opm, opm_mod, pb, pe)), (1, suffix2.upper(), sb, se, fr.stretch(sig, opm, opm_mod, sb, se))])
    want = _want(case, pm, opm, opm_mod, cfg)
    assert not any(t for t, _, _ in want) and want[0][1][4] == fr.EDGE and want[-1][1][4] == fr.SKIPPED and want[-1][1][:2] == (1, len(suffix2) - 2)
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("cgends", repeat, prefix, suffix2)
    got, recs, last = _run(rc, [("cgends", sig, "+")])
    rc.ctx.close()
    assert got[0].row[0] == 15 and len(recs[0]) == len(want)
    for g, (_, fields, v) in zip(recs[0], want):
        assert tuple(int(g[k]) for k in ("flank", "pos", "n_sites", "n_columns", "status", "begin", "end")) == fields, (g, fields)
        assert _bits([g["v_base"], g["v_mod"]]) == _bits(v)
    assert last["groups"] == sum(1 for _, f, _ in want if f[4] == fr.SCORED)


def test_count_flank_mod_end_to_end(tmp_path, pm, tables, cfg, targets):
    """`count --mod_model M --flank-mod FILE` from files: FILE is the host formatter applied to the reference and parses; the count
    TSV is byte-equal to a run without the option."""
    import io
    import json
    from contextlib import redirect_stdout
    import h5write
    from strique_amd import cli, flank_mod
    cases, opm, opm_mod = fr.cases(tables, cfg, targets, ("c9orf72",), True)
    for key, name in (("base", "base.model"), ("mod", "mod.model")):
        with open(tmp_path / name, "w") as fp:
            for k, m, s in zip(tables[key + "_kmer"], tables[key + "_mean"], tables[key + "_stdv"]):
                fp.write("%s\t%s\t%s\t1\n" % (k.decode() if isinstance(k, bytes) else str(k), repr(float(m)), repr(float(s))))
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    (tmp_path / "repeats.tsv").write_text("chr\tbegin\tend\tname\trepeat\tprefix\tsuffix\n" + "\t".join([chrom, str(b), str(e), "c9orf72", repeat, prefix, suffix]) + "\n")
    (tmp_path / "STRique.json").write_text(json.dumps({"align": cfg["align"], "HMM": cfg["HMM"]}))
    reads, sam = [], ["@HD\tVN:1.0"]
    for i, c in enumerate(cases):
        rid = "%08d-0000-4000-8000-%012d" % (i, i)
        reads.append((rid, c["sig"]))
        sam.append("\t".join([rid, "16" if c["strand"] == "-" else "0", chrom, str(b - 3000), "60", "12S6000M5S", "*", "0", "0", "ACGT", "*"]))
    data = tmp_path / "data"; data.mkdir()
    (data / "batch_0.fast5").write_bytes(h5write.multi_read_fast5(reads))
    buf = io.StringIO()
    with redirect_stdout(buf):
        cli.main(["index", str(data)])
    (data / "reads.fofn").write_text(buf.getvalue())
    (tmp_path / "aln.sam").write_text("\n".join(sam) + "\n")
    argv = ["count", str(data / "reads.fofn"), str(tmp_path / "base.model"), str(tmp_path / "repeats.tsv"), "--config", str(tmp_path / "STRique.json"),
            "--algn", str(tmp_path / "aln.sam"), "--mod_model", str(tmp_path / "mod.model")]
    cli.main(argv + ["--out", str(tmp_path / "plain.tsv")])
    cli.main(argv + ["--out", str(tmp_path / "with.tsv"), "--flank-mod", str(tmp_path / "f.tsv")])
    assert (tmp_path / "plain.tsv").read_bytes() == (tmp_path / "with.tsv").read_bytes()
    counts = [line.split("\t")[3] for line in (tmp_path / "plain.tsv").read_text().splitlines()[1:]]
    want = ["\t".join(flank_mod.HEADER)]
    for (rid, _), c, n in zip(reads, cases, counts):
        calls = [(f[0], f[1], f[2], v[1] - v[0] if f[4] == fr.SCORED else None) for tie, f, v in _want(c, pm, opm, opm_mod, cfg)]
        want.append(flank_mod.format_row(rid, "c9orf72", c["strand"], n, calls))
    assert (tmp_path / "f.tsv").read_text().splitlines() == want
    rows = flank_mod.parse(open(tmp_path / "f.tsv"))
    assert len(rows) == len(cases) and all(len(r[4]) in (20, 20) and any(x[3] is not None for x in r[4]) for r in rows)
