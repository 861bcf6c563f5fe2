"""Methylation calls of anchored reads on the GPU (strq_set_anchored_mod, repeatCounter.set_anchored_mod, anchored_mod_task_kernel)
against tests/anchored_mod_ref.py at m = 6.5: the reads of tests/test_anchored_mod_host.py, pattern strings byte for byte and
(V_base, V_mod) bit for bit on every read that qualifies, everything else untouched.

The k-mer tie at the repeat boundary (README, last paragraph of the mod-llr section): a read whose anchored record differs from the
reference's in `begin` alone is compared on everything except its first unit; at most 2 of the 56 reads may need that
(tests/test_anchored_mod_host.py::test_boundary_tie_stays_within_the_exemption finds none for the seed in use)."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest

import anchored_mod_ref as amr
import anchored_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def counter(pm, pm_mod, cfg):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in ar.TARGETS:
        rc.add_target(name, *cfg["repeat"][name][3:6])
    return rc


def _run(counter, items, amod=True, llr=True, **kw):
    """(Detected records, (pattern, (n, 2) pairs or None) or None per read, strq_last_anchored_mod) of one batch."""
    counter.set_anchored_mod(amod)
    try:
        got = counter.detect_batch(items, anchored=amr.M, mod_llr=llr, records=True, **kw)
        pairs = counter.ctx.batch_fetch_anchored_mod() if amod else None
        return got, pairs, counter.ctx.last_anchored_mod()
    finally:
        counter.set_anchored_mod(False)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _frozen(got, pairs):
    """Everything a run hands out, as bytes and tuples: for 'the same bytes come out'."""
    out = []
    for d, p in zip(got, pairs):
        out.append((d.row[:3], _bits(d.row[3]), d.row[4:], d.anchored[:3], _bits(d.anchored[3]), d.anchored[4:], None if d.llr is None else _bits(d.llr),
                    None if d.units is None else _bits(d.units), None if d.conf is None else _bits(d.conf),
                    None if p is None else (p[0], None if p[1] is None else _bits(p[1]))))
    return out


def _check(got, pairs, cases, llr=True):
    """Records against the reference first (as tests/test_gpu_anchored.py does), then the calls.  Returns the qualifying reads."""
    exempt, n_called = [], 0
    for d, p, c in zip(got, pairs, cases):
        what = (c["target"], c["strand"], c["cut"], c["table"])
        rec, ref = c["rec"], c["call"]
        assert tuple(d.row[:6]) == tuple(c["row"][:6]), (what, d.row, c["row"])
        same = tuple(d.anchored[:3]) == tuple(rec[:3]) and tuple(d.anchored[4:]) == tuple(rec[4:]) and _bits(d.anchored[3]) == _bits(rec[3])
        tie = not same and tuple(d.anchored[:2]) == tuple(rec[:2]) and d.anchored[5] == rec[5] and d.anchored[4] != rec[4] and ref is not None
        assert same or tie, (what, d.anchored, rec)
        if ref is None:
            assert p is None and d.anchored_mod is None, (what, p)
            continue
        n_called += 1
        assert p is not None, what
        pattern, V = p
        skip = 1 if tie else 0
        if tie:
            exempt.append(what)
        assert pattern[skip:] == ref[0][skip:] and (tie or len(pattern) == len(ref[0])), (what, pattern, ref[0])
        if llr and ref[0] != "-" and len(ref[0]):
            assert V is not None and V.shape == ref[1].shape, (what, V, ref[1])
            assert _bits(V[skip:]) == _bits(ref[1][skip:]), (what, V, ref[1])
            assert d.anchored_mod[0] == pattern and _bits(d.anchored_mod[1]) == _bits(V[:, 1] - V[:, 0])
        else:
            assert V is None and d.anchored_mod == (pattern, None), (what, V)
    assert len(exempt) <= 2, exempt
    return n_called


@pytest.mark.parametrize("as_int16", [True, False])
def test_calls_equal_the_reference(counter, tables, cfg, as_int16):
    cases = amr.cases(tables, cfg, as_int16)
    assert len(cases) == (56 if as_int16 else 28)
    items = [(c["target"], c["sig"], c["strand"]) for c in cases]
    assert all(sig.dtype == (np.int16 if as_int16 else np.float64) for _, sig, _ in items)
    got, pairs, last = _run(counter, items)
    print("anchored-mod pass:", last, counter.ctx.last_anchored())
    n_called = _check(got, pairs, cases)
    assert n_called == sum(1 for c in cases if amr.qualifies(c["rec"])) >= (50 if as_int16 else 25)
    assert last["reads"] == n_called and last["launches"] >= 5 and last["ms"] > 0
    assert last["units"] == sum(len(p[0]) for p in pairs if p is not None and p[0] != "-")
    # without the per-unit switch: the same patterns, no pairs
    got1, pairs1, last1 = _run(counter, items, llr=False)
    _check(got1, pairs1, cases, llr=False)
    assert [p and p[0] for p in pairs1] == [p and p[0] for p in pairs] and last1["launches"] < last["launches"]
    # the switch off: records, rows, patterns of the rows and their scores byte-equal, nothing launched, nothing to fetch
    off, _, last0 = _run(counter, items, amod=False)
    assert last0 == {"ms": 0.0, "reads": 0, "units": 0, "launches": 0}
    assert _frozen(off, [None] * len(off)) == _frozen(got, [None] * len(got))
    assert all(d.anchored_mod is None for d in off)
    from strique_amd import ffi
    with pytest.raises(ffi.StriqueHipError) as e:
        counter.ctx.batch_fetch_anchored_mod()
    assert e.value.code == ffi.STRQ_ERR_ARG
    # the element detect_batch documents: directly behind the anchored one
    counter.set_anchored_mod(True)
    try:
        pub = counter.detect_batch(items[:6], anchored=amr.M)
    finally:
        counter.set_anchored_mod(False)
    for (row_, an_, am_), d in zip(pub, got):
        assert row_ == d.row and (am_ is None) == (d.anchored_mod is None) and (am_ is None or am_ == (d.anchored_mod[0], None))


@pytest.fixture(scope="module")
def mixed(counter, tables, cfg, pm):
    """The 56 shared reads, and spanning reads and reads without a flank beside them (kinds 1 and 0: no call)."""
    from strique_amd import synth
    table = synth.KmerTable(pm)
    cases = amr.cases(tables, cfg, True)
    items = [(c["target"], c["sig"], c["strand"]) for c in cases]
    rng = np.random.default_rng(78)
    for k, name in enumerate(ar.TARGETS):
        target = tuple(cfg["repeat"][name][3:6])
        items.append((name, synth.make_read(table, 12, k, 3000, target, 20, strand="+-"[k])[0], "+-"[k]))
        items.append((name, synth.make_signal(rng, table, ar._backbone(rng, 1500).encode(), True, 0.0), "+-"[k]))
    return cases, items


def test_the_same_bytes_whatever_the_route(counter, mixed):
    cases, items = mixed
    base, pairs, last = _run(counter, items)
    n_called = _check(base[:len(cases)], pairs[:len(cases)], cases)
    assert last["reads"] == n_called
    for d, p in zip(base[len(cases):], pairs[len(cases):]):
        assert d.anchored[0] in (0, 1) and p is None and d.anchored_mod is None          # spanning (the row has the pattern) or none
    assert any(d.anchored[0] == 1 and d.row[6] != "-" for d in base[len(cases):])
    want = _frozen(base, pairs)
    ctx = counter.ctx
    for key, value in (("STRQ_SERIAL", "1"), ("STRQ_SUBBATCH_READS", "3"), ("STRQ_MOD_BACKPOINTERS", "1"), ("STRQ_VIT_NO_G2", "1")):
        try:
            ctx.set_option(key, value)
            got, gp, gl = _run(counter, items)
        finally:
            ctx.set_option(key, None)
        assert _frozen(got, gp) == want, key
        assert gl["reads"] == n_called, key
    # units and confidence beside it: the same calls, and their own outputs as without it
    both, bp, _ = _run(counter, items, units=True, confidence=True)
    alone, _, _ = _run(counter, items, amod=False, units=True, confidence=True)
    strip = lambda rows: [r[:7] + r[9:] for r in rows]
    assert strip(_frozen(both, bp)) == strip(want)
    assert [r[7:9] for r in _frozen(both, bp)] == [r[7:9] for r in _frozen(alone, [None] * len(alone))]
    assert any(d.units is not None for d in both)


def test_refusals_before_any_launch(counter, pm, cfg, tables):
    from strique_amd import ffi
    from strique_amd.counter import repeatCounter
    c = amr.cases(tables, cfg, True)[4]
    sig = np.ascontiguousarray(c["sig"])
    ctx = counter.ctx
    tid = counter._classifier_for(c["target"], c["strand"]).target_id
    counter._ensure_anchored()
    # anchored counting off
    try:
        ctx.set_anchored_mod(True)
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.detect_batch_reads([sig], [tid])
        assert e.value.code == ffi.STRQ_ERR_ARG and "needs anchored counting" in str(e.value)
        # a scan
        ctx.set_anchored(True, amr.M)
        ctx.batch_upload(sig, [0, len(sig)], [tid])
        ctx.scan_set([tid], 5.0)
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.batch_run()
        assert e.value.code == ffi.STRQ_ERR_ARG and "scan" in str(e.value)
    finally:
        ctx.scan_clear(); ctx.set_anchored_mod(False); ctx.set_anchored(False)
    for bad in (2, -1):
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx._check(ctx._lib.strq_set_anchored_mod(ctx._h, bad))
        assert e.value.code == ffi.STRQ_ERR_ARG
    # the context is usable after the refusals
    got, pairs, last = _run(counter, [(c["target"], c["sig"], c["strand"])])
    _check(got, pairs, [c])
    assert last["reads"] == 1
    # a target without a modification model: no call, nothing launched for it
    plain = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    plain.add_target(c["target"], *cfg["repeat"][c["target"]][3:6])
    with pytest.raises(ValueError):
        plain.set_anchored_mod(True)
    plain._ensure_anchored()
    ptid = plain._classifier_for(c["target"], c["strand"]).target_id
    try:
        plain.ctx.set_anchored(True, amr.M); plain.ctx.set_anchored_mod(True)
        plain.ctx.detect_batch_reads([sig], [ptid])
        assert plain.ctx.batch_fetch_anchored_mod() == [None]
        assert plain.ctx.batch_fetch_anchored()[0]["kind"] == c["rec"][0]
        assert plain.ctx.last_anchored_mod() == {"ms": 0.0, "reads": 0, "units": 0, "launches": 0}
    finally:
        plain.ctx.set_anchored_mod(False); plain.ctx.set_anchored(False)


def test_count_anchored_mod_end_to_end(tmp_path, tables, cfg):
    """`count --mod_model M --anchored FILE --anchored-min-score 6.5 --anchored-mod FILE2 --mod-llr FILE3` from files: FILE2 is the
    host formatter applied to the reference; the count TSV and the other side files are byte-equal to a run without the switch."""
    import h5write
    from strique_amd import anchored as an, cli
    cases = [c for c in amr.cases(tables, cfg, True) if c["target"] == "c9orf72" and c["cut"] in ("in_prefix", "mid_unit", "start_mid")]
    assert len(cases) == 12 and any(c["call"] is None for c in cases)
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
            "--algn", str(tmp_path / "aln.sam"), "--mod_model", str(tmp_path / "mod.model"), "--anchored-min-score", "6.5"]
    cli.main(argv + ["--out", str(tmp_path / "plain.tsv"), "--anchored", str(tmp_path / "a0.tsv"), "--mod-llr", str(tmp_path / "l0.tsv")])
    cli.main(argv + ["--out", str(tmp_path / "with.tsv"), "--anchored", str(tmp_path / "a1.tsv"), "--mod-llr", str(tmp_path / "l1.tsv"),
                     "--anchored-mod", str(tmp_path / "m1.tsv")])
    for x, y in (("plain.tsv", "with.tsv"), ("a0.tsv", "a1.tsv"), ("l0.tsv", "l1.tsv")):
        assert (tmp_path / x).read_bytes() == (tmp_path / y).read_bytes(), x
    want = ["\t".join(an.MOD_HEADER)]
    for (rid, _), c in zip(reads, cases):
        call = None if c["call"] is None else (c["call"][0], c["call"][1][:, 1] - c["call"][1][:, 0] if len(c["call"][1]) else None)
        want.append(an.format_mod_row(rid, "c9orf72", c["strand"], c["rec"], call))
    assert (tmp_path / "m1.tsv").read_text().splitlines() == want
    assert len(an.parse_mod(open(tmp_path / "m1.tsv"))) == 12
