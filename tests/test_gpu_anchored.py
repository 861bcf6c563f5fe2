"""Anchored counting on the GPU (strq_set_anchored, repeatCounter.detect_batch(..., anchored=m), anchored_kernels.hip) against
tests/anchored_ref.py: the reads of tests/test_anchored_host.py::test_cpu_preconditions_on_the_shared_reads, every field of every
record bit for bit, rows untouched."""
import numpy as np
import pytest

import anchored_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def counter(pm, cfg):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in ar.TARGETS:
        rc.add_target(name, *cfg["repeat"][name][3:6])
    return rc


def _same(got, want, what):
    """An anchored record against the reference's, log_p bit for bit."""
    assert tuple(got[:3]) == tuple(want[:3]) and tuple(got[4:]) == tuple(want[4:]), (what, got, want)
    assert np.float64(got[3]).tobytes() == np.float64(want[3]).tobytes(), (what, got, want)


def _same_row(got, want, what):
    assert tuple(got[:6]) == tuple(want[:6]), (what, got, want)


@pytest.fixture(scope="module")
def mixed(pm, opm, orc, cfg, tables):
    """Both targets and all four kinds in one batch: a few of the shared reads, spanning reads and reads without a target.
    [(item, row, record)] with the reference's row and record."""
    from strique_amd import synth
    table = synth.KmerTable(pm)
    params = orc.align_params(cfg["align"])
    shared = ar.cases(tables, cfg, True)
    out = [((n, sig, s), row, rec) for n, s, cut, sig, kind, complete, row, rec in shared if cut in ("mid_unit", "start_mid", "one_base_in")]
    rng = np.random.default_rng(77)
    k = 0
    for name in ar.TARGETS:
        target = tuple(cfg["repeat"][name][3:6])
        for strand in "+-":
            tc = orc.classifier(*target, strand, opm, None, cfg["HMM"])
            mods = ar.models(*target, strand, opm, cfg["HMM"])
            span = synth.make_read(table, 11, k, 3000, target, 20, strand=strand)[0]
            blank = synth.make_signal(rng, table, ar._backbone(rng, 1500).encode(), True, 0.0)
            k += 1
            for sig in (span, blank):
                row, rec = ar.record(sig, tc, mods, opm, params, ar.M)
                out.append(((name, sig, strand), row, rec))
    assert {rec[0] for _, _, rec in out} == {0, 1, 2, 3}
    return out


@pytest.mark.parametrize("as_int16", [True, False])
def test_records_equal_the_reference(counter, tables, cfg, as_int16):
    shared = ar.cases(tables, cfg, as_int16)
    items = [(n, sig, s) for n, s, cut, sig, kind, complete, row, rec in shared]
    assert all(sig.dtype == (np.int16 if as_int16 else np.float64) for _, sig, _ in items)
    got = counter.detect_batch(items, anchored=ar.M, records=True)
    last = counter.ctx.last_anchored()
    print("anchored pass:", last, {t: {k: (v["states"], v["positions_rc"]) for k, v in m.items()} for t, m in counter.anchored_models.items()})
    for d, (n, s, cut, sig, kind, complete, row, rec) in zip(got, shared):
        _same_row(d.row, row, (n, s, cut))
        _same(d.anchored, rec, (n, s, cut))
        assert d.anchored[0] == kind and d.units is None and d.conf is None
    assert last["kinds"] == (0, 0, 20, 8) and last["launches"] >= 4 and last["ms"] > 0
    # which kernel the two models run on is reported: every window on a lane layout or on the register-resident kernel, none on the general one
    assert last["register_resident"] + last["lane_layout"] == 28
    # rows are byte-equal to a run with the switch off, and nothing is launched then
    plain = counter.detect_batch(items)
    assert plain == [d.row for d in got]
    off = counter.ctx.last_anchored()
    assert off["launches"] == 0 and off["kinds"] == (0, 0, 0, 0) and off["ms"] == 0
    # the element detect_batch documents
    pub = counter.detect_batch(items[:8], anchored=ar.M)
    for (row_, el), d in zip(pub, got):
        assert row_ == d.row and el == (("ends_in_repeat", "starts_in_repeat")[d.anchored[0] - 2],) + tuple(d.anchored[2:])


def test_records_on_the_lane_layout(counter, tables, cfg):
    """The same records with the register-resident kernel switched off (STRQ_VIT_NO_G2): the models run on the lane layout their
    hints describe, none on the general kernel."""
    shared = ar.cases(tables, cfg, True)
    items = [(n, sig, s) for n, s, cut, sig, kind, complete, row, rec in shared]
    ctx = counter.ctx
    try:
        ctx.set_option("STRQ_VIT_NO_G2", "1")
        got = counter.detect_batch(items, anchored=ar.M, records=True)
        last = ctx.last_anchored()
    finally:
        ctx.set_option("STRQ_VIT_NO_G2", None)
    assert last["lane_layout"] == 28 and last["register_resident"] == 0
    for d, (n, s, cut, sig, kind, complete, row, rec) in zip(got, shared):
        _same_row(d.row, row, (n, s, cut))
        _same(d.anchored, rec, (n, s, cut))
    # detect() hands out the same record
    one = counter.detect(items[2][0], items[2][1], items[2][2], anchored=ar.M, records=True)
    _same(one.anchored, shared[2][7], "detect")


def test_threshold_at_a_reads_own_score(counter, tables, cfg):
    shared = ar.cases(tables, cfg, True)
    for pick, own in (("before_array_end", 1), ("start_mid", 2)):
        n, s, cut, sig, kind, complete, row, rec = next(c for c in shared if c[2] == pick and c[0] == "c9orf72" and c[1] == "+")
        m = row[own]                                             # the present flank's own score: found at m, not found right above it
        at = counter.detect_batch([(n, sig, s)], anchored=m, records=True)[0]
        above = counter.detect_batch([(n, sig, s)], anchored=float(np.nextafter(m, np.inf)), records=True)[0]
        _same(at.anchored, rec, (pick, m))
        assert above.anchored == (0, 0, 0, 0.0, 0, 0, 0) and above.row == at.row
        # a threshold at the absent flank's score (or below) finds both: the positions decide between spanning and none
        low = counter.detect_batch([(n, sig, s)], anchored=min(row[1], row[2]), records=True)[0]
        assert low.anchored[0] in (0, 1) and low.anchored[1:] == (0, 0, 0.0, 0, 0, 0)


def test_mixed_batch_sub_batches_and_other_passes(counter, mixed):
    items = [it for it, _, _ in mixed]
    base = counter.detect_batch(items, anchored=ar.M, records=True)
    for d, (it, row, rec) in zip(base, mixed):
        _same_row(d.row, row, it[0] + it[2])
        _same(d.anchored, rec, it[0] + it[2])
    ctx = counter.ctx
    try:
        ctx.set_option("STRQ_SERIAL", "1")
        serial = counter.detect_batch(items, anchored=ar.M, records=True)
        ctx.set_option("STRQ_SERIAL", None)
        ctx.set_option("STRQ_SUBBATCH_READS", "3")
        small = counter.detect_batch(items, anchored=ar.M, records=True)
        assert ctx.last_anchored()["kinds"] == tuple(sum(1 for _, _, rec in mixed if rec[0] == k) for k in range(4))
    finally:
        ctx.set_option("STRQ_SERIAL", None); ctx.set_option("STRQ_SUBBATCH_READS", None)
    assert serial == base and small == base
    for a, b in zip(serial + small, base + base):
        assert np.float64(a.anchored[3]).tobytes() == np.float64(b.anchored[3]).tobytes()
    # units and confidence beside it: the same records, and their own outputs as without it
    both = counter.detect_batch(items, units=True, confidence=True, anchored=ar.M, records=True)
    alone = counter.detect_batch(items, units=True, confidence=True, records=True)
    assert [d.anchored for d in both] == [d.anchored for d in base] and [d.row for d in both] == [d.row for d in base]
    assert all(d.anchored is None for d in alone)
    for x, y in zip(both, alone):
        assert (x.units is None) == (y.units is None) and (x.units is None or np.array_equal(x.units, y.units))
        assert (x.conf is None) == (y.conf is None) and (x.conf is None or np.array(x.conf).tobytes() == np.array(y.conf).tobytes())


def test_switch_off_and_refusals(counter, pm, cfg, tables):
    from strique_amd import ffi
    from strique_amd.counter import repeatCounter
    n, s, cut, sig, *_ = ar.cases(tables, cfg, True)[2]
    ctx = counter.ctx
    before = counter.detect_batch([(n, sig, s)])
    assert ctx.last_anchored()["launches"] == 0
    with pytest.raises(ffi.StriqueHipError) as e:
        ctx.batch_fetch_anchored()                               # the last run call ran with the switch off
    assert e.value.code == ffi.STRQ_ERR_ARG
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.set_anchored(True, bad)
        assert e.value.code == ffi.STRQ_ERR_ARG and "above 0" in str(e.value)
        with pytest.raises(ValueError):
            counter.detect_batch([(n, sig, s)], anchored=bad)
    # a target without the two models: the run call fails, a run without the switch goes through
    fresh = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    fresh.add_target("c9orf72", *cfg["repeat"]["c9orf72"][3:6])
    want = fresh.detect_batch([("c9orf72", sig, "+")])
    assert fresh.anchored_models == {}                           # a counter that never asked has registered nothing
    tid = fresh._classifier_for("c9orf72", "+").target_id
    try:
        fresh.ctx.set_anchored(True, ar.M)
        with pytest.raises(ffi.StriqueHipError) as e:
            fresh.ctx.detect_batch_reads([np.ascontiguousarray(sig)], [tid])
        assert e.value.code == ffi.STRQ_ERR_ARG and "without anchored models" in str(e.value)
    finally:
        fresh.ctx.set_anchored(False)
    assert fresh.detect_batch([("c9orf72", sig, "+")]) == want
    # a scan with the switch on
    ids = [counter._classifier_for(t, st).target_id for t, st in counter.candidates()]
    counter._ensure_anchored()
    try:
        ctx.set_anchored(True, ar.M)
        ctx.batch_upload(np.ascontiguousarray(sig), [0, len(sig)], [ids[0]])
        ctx.scan_set(ids, 5.0)
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.batch_run()
        assert e.value.code == ffi.STRQ_ERR_ARG and "scan" in str(e.value)
    finally:
        ctx.scan_clear(); ctx.set_anchored(False)
    # the context is usable after the refusals, with the switch off
    assert counter.detect_batch([(n, sig, s)]) == before
    assert ctx.last_anchored()["launches"] == 0
    with pytest.raises(ffi.StriqueHipError):
        ctx.batch_fetch_anchored()
