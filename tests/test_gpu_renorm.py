"""The second normalisation step on the GPU (strq_set_renorm, repeatCounter.set_renorm, renorm_kernels.hip) against the rule
(strique_amd/renorm.py) and the reference built on it (tests/renorm_ref.py): fit records, conditioning scalars and level values after
the fold bit for bit, rows equal to the reference, the read detect() loses as it stands, and nothing launched with the switch off."""
import numpy as np
import pytest

import renorm_ref as rr

pytestmark = pytest.mark.gpu

SCALARS = ("med", "mad", "f_c1", "f_h1", "m_c1", "m_h1", "r_c1", "r_h1", "h2", "c2")


def _counter(pm, cfg, pm_mod=None, names=("c9orf72", "fmr1")):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in names:
        rc.add_target(name, *cfg["repeat"][name][3:6])
    return rc


@pytest.fixture(scope="module")
def counter(pm, cfg):
    return _counter(pm, cfg)


@pytest.fixture(scope="module")
def shared(tables, cfg):
    """[(spec, signal, row, record, state)] of the reference for the shared reads, computed once."""
    return rr.run_specs(rr.READS, tables, cfg)


def _record(r):
    """A fetched strq_renorm as the rule's record."""
    return int(r["applied"]), {s: (int(f["a"]), int(f["b"]), int(f["w"]), int(f["score"])) if f["fitted"] else None for s, f in zip(rr.renorm.SIGNALS, r["fit"])}


def _bits(x):
    return np.asarray(x, np.float64).tobytes()


def _same_row(got, want, what):
    assert tuple(got[:3]) == tuple(want[:3]) and tuple(got[4:]) == tuple(want[4:]), (what, got, want)
    assert _bits(got[3]) == _bits(want[3]), (what, got, want)


@pytest.mark.parametrize("name,strand", [("c9orf72", "+"), ("fmr1", "-")])
def test_fit_kernel_equals_the_rule_on_histograms(counter, qa_tables, name, strand):
    """The fit kernel alone: all samples in one bin (ties), bins at the rim (every scaled bin outside the grid), an empty histogram,
    a single sample, counters near 2^31 (the int64 accumulation), flat and random histograms."""
    counter._ensure_renorm()
    tid = counter._classifier_for(name, strand).target_id
    Q, A = qa_tables[(name, strand)]
    rng = np.random.default_rng(5)
    hs = []
    for bins_, v in (([512], 5000), ([300], 77), ([400, 640], 10), ([0, 1023], 3), ([700], 1), ([], 0), ([333], 2 ** 31 - 1), (list(range(256, 768, 16)), 1)):
        h = np.zeros(1024, np.uint32); h[bins_] = v; hs.append(h)
    hs.append(rng.integers(0, 50, 1024).astype(np.uint32))
    hs.append((rng.integers(0, 2, 1024) * rng.integers(1, 2 ** 31 - 1, 1024)).astype(np.uint32))
    sparse = np.zeros(1024, np.uint32); sparse[rng.integers(0, 1024, 40)] = rng.integers(1, 10 ** 5, 40); hs.append(sparse)
    while len(hs) % 3:
        hs.append(np.zeros(1024, np.uint32))
    for k in range(0, len(hs), 3):
        got = _record(counter.ctx.debug_renorm_fit(tid, np.stack(hs[k:k + 3])))
        for s, h in zip(rr.renorm.SIGNALS, hs[k:k + 3]):
            assert got[1][s] == rr.renorm.fit(h.astype(np.int64), Q, A), (k, s)


@pytest.fixture(scope="module")
def qa_tables(tables, cfg):
    _, opm, _ = rr.setup(tables, cfg)
    return {(name, strand): rr.target_tables(opm, cfg["repeat"][name][3], strand) for name in ("c9orf72", "fmr1") for strand in "+-"}


@pytest.mark.parametrize("as_int16", [True, False])
def test_fit_records_and_conditioning_after_the_fold(counter, shared, tables, cfg, qa_tables, as_int16):
    """Records, conditioning scalars and level values, bit for bit: the shared reads of one element type (both targets and strands in
    one batch) and the edge reads -- constant, fewer than 64 samples, samples outside the grid."""
    _, opm, _ = rr.setup(tables, cfg)
    rn = rr.renorm
    want = []      # (name, signal, target id, record, maps or None, level values or None)
    for spec, sig, row, rec, st in shared:
        if spec[5] == as_int16:
            want.append((spec[0], sig, counter._classifier_for(spec[1], spec[2]).target_id, rec, st["maps"], st["level_val"]))
    base = rr.signal_of(rr.READS[0] if as_int16 else rr.READS[6], tables, cfg)
    spec0 = rr.READS[0] if as_int16 else rr.READS[6]
    tid0 = counter._classifier_for(spec0[1], spec0[2]).target_id
    edge = [("constant", np.full(5000, 417, base.dtype)), ("short", base[5000:5040].copy())]
    if as_int16:
        edge.append(("outliers", rr.with_outliers(base)))
    for name, sig in edge:
        maps, signals, status, _, _ = rr.condition(sig, opm)
        out, rec = rn.apply(maps, signals, *qa_tables[(spec0[1], spec0[2])], opm.model_min, opm.model_max, rr.MIN_SHARE, status)
        lv = rn.level_values(*out["morph"], out["h2"], out["c2"], opm.model_min + .5, opm.model_max - .5) if status == 0 else None
        want.append((name, sig, tid0, rec, out if status == 0 else None, lv))
    assert [w[3][0] for w in want if w[0] in ("constant", "short")] == [0, 0]
    ctx = counter.ctx
    counter._ensure_renorm()
    try:
        ctx.set_renorm(True, rr.MIN_SHARE)
        ctx.detect_batch_reads([np.ascontiguousarray(w[1]) for w in want], [w[2] for w in want])
        recs = ctx.batch_fetch_renorm()
        last = ctx.last_renorm()
        cond = [ctx.debug_conditioning(i, len(w[1])) for i, w in enumerate(want)]
    finally:
        ctx.set_renorm(False)
    print("renorm pass:", last, [(w[0], _record(r)) for w, r in zip(want, recs)])
    for (name, sig, tid, rec, maps, lv), r, (levels, lval, sc) in zip(want, recs, cond):
        assert _record(r) == rec, (name, _record(r), rec)
        if maps is None:
            continue
        got = dict(zip(SCALARS, sc))
        for s, (c, h) in (("filtered", ("f_c1", "f_h1")), ("morph", ("m_c1", "m_h1"))):
            assert _bits(got[c]) == _bits(maps[s][0]) and _bits(got[h]) == _bits(maps[s][1]), (name, s, got, maps)
        assert _bits(got["h2"]) == _bits(maps["h2"]) and _bits(got["c2"]) == _bits(maps["c2"])
        assert np.asarray(lval, np.float32).tobytes() == lv.tobytes(), name
    n_fit = sum(1 for w in want if w[3][1]["filtered"] is not None)
    assert last["fitted"] == n_fit and last["applied"] == sum(w[3][0] for w in want) and last["launches"] >= 4 and last["ms"] > 0
    assert {0, 1} <= {w[3][0] for w in want}                        # the gate went both ways


def test_rows_equal_the_reference(counter, shared):
    """The full tuple of every shared read (int16 and float64, both targets, shares 0.04 / 0.72 / 0.93), the records beside them,
    small sub-batches in pipelined and in serial order, and the unit and anchored passes behind the corrected maps."""
    items = [(spec[1], sig, spec[2]) for spec, sig, row, rec, st in shared]
    ctx = counter.ctx
    counter.set_renorm(rr.MIN_SHARE)
    try:
        base = counter.detect_batch(items, records=True)
        for d, (spec, sig, row, rec, st) in zip(base, shared):
            _same_row(d.row, row, spec[0])
            assert d.renorm == rec, (spec[0], d.renorm, rec)
            if spec[6] > 0.5:
                assert d.row[0] == spec[3] and d.renorm[0] == 1
        assert counter.detect_batch(items) == [d.row for d in base]          # the tuple itself, without records
        try:
            ctx.set_option("STRQ_SUBBATCH_READS", "2")
            small = counter.detect_batch(items, records=True)
            ctx.set_option("STRQ_SERIAL", "1")
            serial = counter.detect_batch(items, records=True)
        finally:
            ctx.set_option("STRQ_SERIAL", None); ctx.set_option("STRQ_SUBBATCH_READS", None)
        for other in (small, serial):
            assert [(d.row, d.renorm) for d in other] == [(d.row, d.renorm) for d in base]
            assert all(_bits(a.row[3]) == _bits(b.row[3]) for a, b in zip(other, base))
        # units on one read, anchored counting on another: their rows are the reference's, the passes ran on the corrected maps
        k = next(i for i, s in enumerate(shared) if s[0][0] == "fm_p_072_i")
        u = counter.detect_batch([items[k]], units=True, records=True)[0]
        _same_row(u.row, shared[k][2], "units")
        assert u.units is not None and len(u.units) > 0.9 * shared[k][0][3]
        j = next(i for i, s in enumerate(shared) if s[0][0] == "c9_m_072_i")
        a = counter.detect_batch([items[j]], anchored=6.5, records=True)[0]
        _same_row(a.row, shared[j][2], "anchored")
        assert a.anchored[0] == 1 and a.renorm == shared[j][3]
    finally:
        counter.set_renorm(None)


@pytest.mark.parametrize("k", [1, 7])
def test_rows_with_a_modification_model(pm, pm_mod, opm_mod, cfg, tables, k):
    """A target with a modification model: the raw signal is fitted too, and the pattern is the reference's.  An int16 read (its raw
    histogram is re-binned) and a float64 read (its raw signal is streamed)."""
    spec = rr.READS[k]
    assert spec[5] == (k == 1)
    (_, sig, row, rec, st), = rr.run_specs([spec], tables, cfg, opm_mod=opm_mod)
    assert rec[1]["raw"] is not None and rec[0] == 1 and row[6] != "-"
    rc = _counter(pm, cfg, pm_mod, names=("c9orf72",))
    rc.set_renorm(rr.MIN_SHARE)
    d = rc.detect_batch([(spec[1], sig, spec[2])], records=True)[0]
    _same_row(d.row, row, "mod")
    assert d.row[6] == row[6] and d.renorm == rec
    sc = dict(zip(SCALARS, rc.ctx.debug_conditioning(0, len(sig))[2]))
    assert _bits(sc["r_c1"]) == _bits(st["maps"]["raw"][0]) and _bits(sc["r_h1"]) == _bits(st["maps"]["raw"][1])


@pytest.mark.parametrize("k", [0, 3])
def test_the_read_detect_loses_reports_its_planted_count(counter, tables, cfg, k):
    """Share 0.87: the planted count with the switch on, something else with it off."""
    spec = rr.LOST[k]
    sig = rr.signal_of(spec, tables, cfg)
    off = counter.detect(spec[1], sig, spec[2])
    counter.set_renorm(rr.MIN_SHARE)
    try:
        on = counter.detect(spec[1], sig, spec[2], records=True)
    finally:
        counter.set_renorm(None)
    print(spec[0], "off", off[:3], "on", on.row[:3], on.renorm)
    assert on.row[0] == spec[3] and on.renorm[0] == 1
    assert off[0] != spec[3]


def test_switch_off_and_refusals(counter, pm, cfg, shared):
    from strique_amd import ffi
    items = [(spec[1], sig, spec[2]) for spec, sig, row, rec, st in shared[:4]]
    ctx = counter.ctx
    counter.set_renorm(rr.MIN_SHARE)
    try:
        on = counter.detect_batch(items)
    finally:
        counter.set_renorm(None)
    off = counter.detect_batch(items)
    assert ctx.last_renorm() == {"ms": 0.0, "fitted": 0, "applied": 0, "launches": 0}
    with pytest.raises(ffi.StriqueHipError) as e:
        ctx.batch_fetch_renorm()                                 # the last run call ran with the switch off
    assert e.value.code == ffi.STRQ_ERR_ARG
    # a context that never heard of the feature: the same bytes
    fresh = _counter(pm, cfg)
    never = fresh.detect_batch(items)
    assert never == off and all(_bits(a[3]) == _bits(b[3]) for a, b in zip(never, off))
    assert fresh._renorm_done == set() and fresh.ctx.last_renorm()["launches"] == 0
    assert on != off                                             # (the switch does change rows: that is the point)
    for bad in (0.0, 1.0, -0.3, 1.5, float("nan")):
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.set_renorm(True, bad)
        assert e.value.code == ffi.STRQ_ERR_ARG and "(0, 1)" in str(e.value)
    # a target without tables: the run call fails before any launch, a run without the switch goes through
    tid = fresh._classifier_for(items[0][0], items[0][2]).target_id
    try:
        fresh.ctx.set_renorm(True, 0.4)
        with pytest.raises(ffi.StriqueHipError) as e:
            fresh.ctx.detect_batch_reads([np.ascontiguousarray(items[0][1])], [tid])
        assert e.value.code == ffi.STRQ_ERR_ARG and "tables" in str(e.value)
        assert fresh.ctx.last_renorm()["launches"] == 0
    finally:
        fresh.ctx.set_renorm(False)
    assert fresh.detect_batch(items[:1]) == never[:1]
    # not with a scan
    ids = [counter._classifier_for(t, st).target_id for t, st in counter.candidates()]
    try:
        ctx.scan_set(ids, 5.0)
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.set_renorm(True, 0.4)
        assert e.value.code == ffi.STRQ_ERR_ARG and "scan" in str(e.value)
    finally:
        ctx.scan_clear(); ctx.set_renorm(False)
    counter.set_renorm(0.4)
    try:
        with pytest.raises(ValueError):
            counter.scan_batch([items[0][1]], min_score=5.0)
    finally:
        counter.set_renorm(None)
    assert counter.detect_batch(items) == off


def test_tables_are_replaced_and_a_second_grid_is_refused(pm, cfg, qa_tables, shared):
    """strq_target_set_renorm again on a target replaces its tables (the same records afterwards); a grid that differs from the one
    another target's tables were registered with is refused and changes nothing; with no other tables held the grid may change."""
    from strique_amd import ffi
    rc = _counter(pm, cfg)
    rc._ensure_renorm()
    spec, sig, row, rec, st = shared[1]
    item = [(spec[1], sig, spec[2])]
    tid = rc._classifier_for(spec[1], spec[2]).target_id
    Q, A = qa_tables[(spec[1], spec[2])]
    rc.set_renorm(rr.MIN_SHARE)
    first = rc.detect_batch(item, records=True)[0]
    assert first.renorm == rec
    for _ in range(3):
        rc.ctx.target_set_renorm(tid, Q, A, pm.model_min, pm.model_max)
    with pytest.raises(ffi.StriqueHipError) as e:
        rc.ctx.target_set_renorm(tid, Q, A, pm.model_min, pm.model_max + 1.0)
    assert e.value.code == ffi.STRQ_ERR_ARG and "grid" in str(e.value)
    again = rc.detect_batch(item, records=True)[0]
    assert again.renorm == rec and again.row == first.row
    one = _counter(pm, cfg, names=(spec[1],))
    tids = [one._classifier_for(spec[1], s).target_id for s in "+-"]
    one.ctx.target_set_renorm(tids[0], Q, A, pm.model_min, pm.model_max)
    one.ctx.target_set_renorm(tids[0], Q, A, pm.model_min, pm.model_max + 1.0)          # the only tables of the context: its grid follows
    with pytest.raises(ffi.StriqueHipError):
        one.ctx.target_set_renorm(tids[1], Q, A, pm.model_min, pm.model_max)


def test_count_renorm_on_the_bundled_read(workdir):
    """`count --renorm` on tests/golden/c9orf72.{fast5,sam}: the real read fits a share of 0.07 and is left alone by the gate, so the
    count TSV is byte-identical to a run without the flag; the side file has one row per count row with the fit.  With the gate
    below the fitted share the row changes (the real read does not survive the fit: README, "Renorm")."""
    from strique_amd import cli, renorm as rn
    from test_cli_end_to_end import _index
    fofn = workdir / "data" / "reads.fofn"
    fofn.write_text(_index(workdir))
    base = [str(fofn), str(workdir / "r9_4_450bps.model"), str(workdir / "repeat_config.tsv"),
            "--config", str(workdir / "STRique.json"), "--algn", str(workdir / "data" / "c9orf72.sam")]
    plain, gated, side, forced, side2 = (workdir / n for n in ("plain.tsv", "gated.tsv", "renorm.tsv", "forced.tsv", "renorm2.tsv"))
    cli.main(["count"] + base + ["--out", str(plain)])
    cli.main(["count"] + base + ["--out", str(gated), "--renorm", "0.4", "--renorm-out", str(side)])
    assert gated.read_bytes() == plain.read_bytes()
    rows = plain.read_text().splitlines()[1:]
    srows = rn.parse(open(side))
    assert len(srows) == len(rows) == 1 and srows[0][:3] == tuple(rows[0].split("\t")[:3])
    applied, fits = srows[0][3]
    assert applied == 0 and fits[0] is not None and fits[1] is not None and fits[2] is None
    assert fits[1][0] == 0.07 and fits[1][1] == 65 / 64                # the fit tools/renorm_accuracy.py reports for this read
    cli.main(["count"] + base + ["--out", str(forced), "--renorm", "0.05", "--renorm-out", str(side2)])
    assert rn.parse(open(side2))[0][3][0] == 1 and rn.parse(open(side2))[0][3][1] == fits
    assert forced.read_bytes() != plain.read_bytes()


from test_cli_end_to_end import workdir  # noqa: E402,F401  (the bundled fast5 / SAM / model files in a temporary directory)
