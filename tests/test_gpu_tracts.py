"""Tract decodes on the GPU (strq_model_set_tracts, strq_viterbi_tracts) against the two references of tests/tract_ref.py: the
log-probability has the oracle's bits, the counts of every tract and the status are equal.  Every comparison is exact.

Model level: the random baked models of tests/vit_mode_cases.py with their counted emitting states spread over two or three tracts
-- every lane row in both single-stage forms and the general kernel -- and the compound models of the product on the shared clean
reads; the shape that ran is the one strq_debug_viterbi_plan planned.  Field isolation: a window of 2^21 - 1 observations whose
three counters are exact, and one of 2^21 that is not decoded.  Pipeline (strq_set_tracts, repeatCounter.set_tracts): synthetic reads
of both loci and strands, a read whose gate fails and one of a target without tracts, across sub-batches -- records equal the
reference's, rows, units and confidence byte-equal with the switch on and off; the refusals; one `count --tract-units --tracts` run
from written fast5 files."""
import math

import numpy as np
import pytest

import tract_ref as tr
import vit_mode_cases as vc

pytestmark = pytest.mark.gpu

GENERATED = ["row%d_%s" % (row, v) for row in range(8) for v in ("ss", "multi")] + ["general"]


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    return ffi.Context(0)


@pytest.fixture(scope="module")
def all_cases(pm, pm_mod, cfg):
    return vc.cases(pm, pm_mod, cfg)


def spread(bk, K):
    """tract_of of a baked model: its counted emitting states (count_inc 1) dealt to K tracts in turn, everything else -1."""
    out = np.full(bk.n_states, -1, np.int32)
    counted = [l for l in range(bk.silent_start) if bk.count_inc[l] == 1]
    assert len(counted) >= 2
    for i, l in enumerate(counted):
        out[l] = i % K
    return out


def windows_of(case):
    """T = 1 and 2, about 40 and about 300 observations, a window with missing observations, an all-NaN window and one no
    distribution gives a finite probability (no path)."""
    w = dict(case.windows)
    return [("T1", w["T1"]), ("T2", w["T2"]), ("T41", w["T333"][:41]), ("T300", w["T333"][:300]), ("nan7", w["nan7"]), ("allnan", w["allnan"]),
            ("nopath", w["nopath"])]


def check(bk, tract_of, K, labels, xs, got, what):
    logp, counts, status = got
    for i, (label, x) in enumerate(zip(labels, xs)):
        a = tr.decode_a(bk, tract_of, K, x)
        b = tr.decode_b(bk, tract_of, K, x)
        assert a[1:] == b[1:] and np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes(), what + (label, a, b)          # (the references agree)
        w = what + (label, float(logp[i]), [int(v) for v in counts[i]], int(status[i]), a)
        assert int(status[i]) == a[2], w
        assert [int(v) for v in counts[i]] == a[1] + [0] * (3 - K), w
        if a[2] == 0:
            assert np.float64(logp[i]).tobytes() == np.float64(a[0]).tobytes(), w
        else:
            assert logp[i] == -np.inf, w


@pytest.mark.parametrize("name", GENERATED)
def test_generated_models_against_both_references(ctx, all_cases, name):
    from strique_amd import ffi
    c = all_cases[name]
    bk = c.baked
    K = 3 if int((np.asarray(bk.count_inc)[:bk.silent_start] == 1).sum()) >= 3 else 2          # (the rows with unit records have two counted states)
    tract_of = spread(bk, K)
    mid = ctx.model_create(bk)
    ctx.model_set_tracts(mid, K, tract_of)
    plan = ffi.debug_viterbi_plan(bk)
    assert plan["shape"] == (vc.SHAPE_CSR if c.row == vc.SHAPE_CSR else c.row | (vc.SHAPE_SS if c.ss else 0)), (name, plan)
    labels = [l for l, _ in windows_of(c)]; xs = [x for _, x in windows_of(c)]
    got = ctx.viterbi_tracts(mid, xs)
    assert ctx.debug_tract_shape() == plan["shape"], (name, ctx.debug_tract_shape(), plan["shape"])
    check(bk, tract_of, K, labels, xs, got, (name,))
    # the count decode of the same model is what it was: the tract increments are an array of their own
    _, counted, _, _ = ctx.viterbi_batch(mid, xs)
    for x, n in zip(xs, counted):
        assert int(n) == tr.orc.viterbi(bk, x)[2], name
    # ragged batch: every window alone gives the bits it gave in the batch
    for i, x in enumerate(xs):
        one = ctx.viterbi_tracts(mid, [x])
        assert np.float64(one[0][0]).tobytes() == np.float64(got[0][i]).tobytes() and np.array_equal(one[1][0], got[1][i]) and one[2][0] == got[2][i], (name, labels[i])


def _flanks(cfg):
    prefix, suffix = cfg["repeat"]["c9orf72"][4:6]
    return prefix[-50:].upper(), suffix[:50].upper()


@pytest.mark.parametrize("locus", sorted(tr.LOCI))
@pytest.mark.parametrize("strand", "+-")
def test_compound_models_on_the_shared_reads(ctx, pm, opm, cfg, locus, strand):
    """The product's compound model, baked, on the clean reads: the GPU against both references on the baked arrays, and against
    the reference net's own decode (same bits: bake() only splices certain silent states)."""
    from strique_amd import ffi, hmm, tracts
    prefix, suffix = _flanks(cfg)
    units, linkers = tr.LOCI[locus]
    un, li = tracts.strand_definition(units, linkers, strand)
    p, s = (prefix, suffix) if strand == '+' else (tr.orc.revcomp(suffix), tr.orc.revcomp(prefix))
    cm = hmm.CompoundRepeatModel(un, li, p, s, pm, cfg["HMM"])
    mid = ctx.model_create(cm.baked)
    ctx.model_set_tracts(mid, cm.n_tracts, cm.tract_of)
    plan = ffi.debug_viterbi_plan(cm.baked)
    mine = [c for c in tr.cases(opm, prefix, suffix, cfg["HMM"]) if c[0] == locus and c[1] == strand]
    xs = [c[3] for c in mine]
    # a window shorter than any path (every path emits in both flanks and in every loop), and the clean reads
    xs = [xs[0][:1], xs[0][:2]] + xs
    labels = ["short1", "short2"] + ["planted%r" % (c[2],) for c in mine]
    got = ctx.viterbi_tracts(mid, xs)
    assert ctx.debug_tract_shape() == plan["shape"] and plan["shape"] >= 0
    assert [int(v) for v in got[2][:2]] == [1, 1]
    check(cm.baked, cm.tract_of, cm.n_tracts, labels, xs, got, (locus, strand))
    for i, (_, _, planted, x, m) in enumerate(mine, 2):
        ref = tr.decode_a(m["prep"], m["tract_of"], m["K"], x)
        assert np.float64(got[0][i]).tobytes() == np.float64(ref[0]).tobytes() and [int(v) for v in got[1][i][:m["K"]]] == ref[1]
        counts = tracts.configured_order([int(v) + b for v, b in zip(got[1][i], cm.count_bias)], strand)
        assert tuple(c - q for c, q in zip(counts, planted)) == tr.RECORDED_ERROR[(locus, strand, planted)]


def test_set_tracts_rejects_what_it_must(ctx, all_cases):
    from strique_amd import ffi
    bk = all_cases["row1_ss"].baked          # counted silent states among its count_inc
    mid = ctx.model_create(bk)
    with pytest.raises(ffi.StriqueHipError):
        ctx.viterbi_tracts(mid, [np.zeros(3)])          # no tracts set
    good = spread(bk, 2)
    for bad_k in (0, 4):
        with pytest.raises(ffi.StriqueHipError):
            ctx.model_set_tracts(mid, bad_k, good)
    t = good.copy(); t[np.nonzero(good == 1)[0][0]] = 2          # a tract beyond n_tracts
    with pytest.raises(ffi.StriqueHipError):
        ctx.model_set_tracts(mid, 2, t)
    t = good.copy(); t[int(np.nonzero(np.asarray(bk.count_inc)[:bk.silent_start] == 0)[0][0])] = 0          # an emitting state that is not counted
    with pytest.raises(ffi.StriqueHipError):
        ctx.model_set_tracts(mid, 2, t)
    t = good.copy(); t[bk.n_states - 2] = 0          # a silent state
    with pytest.raises(ffi.StriqueHipError):
        ctx.model_set_tracts(mid, 2, t)
    ctx.model_set_tracts(mid, 2, good)


# ---- field isolation -------------------------------------------------------------------------------------------------------------
LEVELS = (70.0, 130.0, 100.0)


def isolation_model(variant):
    """Three counted emitting states in a row, one per tract, each a Normal emission with a self-loop (tests/vit_mode_cases.py's
    boundary model with all three counted); "csr": nine more in-edges on the last state, so that only the general kernel takes it."""
    extra = 9 if variant == "csr" else 0
    ne = 3 + extra; n = ne + 4; start = ne; s1, s2 = ne + 1, ne + 2; end = n - 1
    ins = [set() for _ in range(n)]
    ins[0] = {0, start}; ins[1] = {0, 1}; ins[2] = {1, 2} | set(range(3, ne))
    for k in range(3, ne):
        ins[k] = {k}
    ins[s1] = {start}; ins[s2] = {s1, 2}; ins[end] = {s2, 2}
    lps = {(k, l): math.log(0.5) for l in range(n) for k in ins[l]}
    mu = np.concatenate([LEVELS, np.full(extra, 40.0)]); sigma = np.full(ne, 2.0)
    inc = np.zeros(n, np.int32); inc[:3] = 1
    bk = vc._baked(n, ne, start, end, ins, lps, np.ones(ne, np.int32), mu, 1.0 / (2 * sigma ** 2), -np.log(sigma * 2.50662827463), inc, np.zeros(n, np.int32))
    tract_of = np.full(n, -1, np.int32); tract_of[:3] = (0, 1, 2)
    return bk, tract_of


def isolation_window(T, n2):
    """All but a few observations in the counted state of tract 0, then of tract 1 -- more than 2^20 in the first, so that its
    counter uses its top bit -- and n2 in that of tract 2."""
    n0 = (1 << 20) + 5
    x = np.full(T, LEVELS[1]); x[:n0] = LEVELS[0]; x[T - n2:] = LEVELS[2]
    return x, [n0, T - n0 - n2, n2]


@pytest.mark.parametrize("variant", ["lane", "csr"])
def test_field_isolation_at_the_window_limit(ctx, variant):
    from strique_amd import ffi
    bk, tract_of = isolation_model(variant)
    plan = ffi.debug_viterbi_plan(bk)
    assert (plan["shape"] == vc.SHAPE_CSR) == (variant == "csr")
    mid = ctx.model_create(bk)
    ctx.model_set_tracts(mid, 3, tract_of)
    T = (1 << 21) - 1
    x, want = isolation_window(T, 3)
    assert sum(want) == T and want[0] >= 1 << 20 and want[1] > 0
    # a short window beside it: the long one's counters do not leak into a neighbour of the batch
    short, want_short = np.array([LEVELS[0]] * 4 + [LEVELS[1]] * 2 + [LEVELS[2]]), [4, 2, 1]
    if variant == "csr":
        # the general kernel takes a workgroup barrier per level of silent states: two million time steps are ten seconds there.
        # Its payload arithmetic is the lane kernels' (one 64-bit addition); here only the limit itself
        logp, counts, status = ctx.viterbi_tracts(mid, [np.append(x, LEVELS[2]), short])
        assert ctx.debug_tract_shape() == plan["shape"]
        assert [int(s) for s in status] == [2, 0] and not counts[0].any() and [int(v) for v in counts[1]] == want_short
        return
    logp, counts, status = ctx.viterbi_tracts(mid, [short, x])
    assert ctx.debug_tract_shape() == plan["shape"]
    assert [int(s) for s in status] == [0, 0]
    assert [int(v) for v in counts[0]] == want_short and [int(v) for v in counts[1]] == want, (counts, want)
    a = tr.decode_a(bk, tract_of, 3, x)          # the oracle's path over the whole window
    assert a[1] == want and a[2] == 0 and np.float64(logp[1]).tobytes() == np.float64(a[0]).tobytes()
    # one observation more: not decoded
    logp, counts, status = ctx.viterbi_tracts(mid, [np.append(x, LEVELS[2]), short])
    assert [int(s) for s in status] == [2, 0] and not counts[0].any() and [int(v) for v in counts[1]] == want_short


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
# (target, strand, planted or None, what): both loci, both strands, K = 2 and 3; a read whose gate fails (its flanks in the wrong
# order) and a read of a target without tracts
PIPELINE_READS = [
    ("htt_like", "+", (12, 7), "read"), ("htt_like", "-", (5, 9), "read"), ("cnbp_like", "+", (9, 6, 11), "read"), ("cnbp_like", "-", (6, 10, 7), "read"),
    ("htt_like", "+", (30, 4), "read"), ("cnbp_like", "-", (15, 3, 8), "read"), ("htt_like", "+", (8, 8), "swapped"), ("plain", "+", None, "plain"),
    ("htt_like", "-", (21, 16), "read"),
]
FLANKED_REPEAT = {"htt_like": "CAG", "cnbp_like": "CCTG"}


def _full_flanks(cfg):
    return cfg["repeat"]["c9orf72"][4].upper(), cfg["repeat"]["c9orf72"][5].upper()


def pipeline_signal(table, cfg, i, target, strand, planted, what):
    from strique_amd import synth
    prefix, suffix = _full_flanks(cfg)
    rng = np.random.Generator(np.random.PCG64(4100 + i))
    total = 6000 + 450 * i
    if what == "plain":
        seq = synth.make_sequence(rng, total, prefix, cfg["repeat"]["c9orf72"][3], 20, suffix, strand)
    else:
        array = tr.array_of(*tr.LOCI[target], planted)
        # the whole array as `repeat`, once; "swapped": the suffix in front of the prefix, so that the gate fails
        seq = synth.make_sequence(rng, total, suffix, array, 1, prefix, strand) if what == "swapped" else synth.make_sequence(rng, total, prefix, array, 1, suffix, strand)
    return synth.make_signal(rng, table, seq, True, 0.0)


@pytest.fixture(scope="module")
def counter(pm, cfg):
    from strique_amd.counter import repeatCounter
    prefix, suffix = _full_flanks(cfg)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in sorted(tr.LOCI):
        rc.add_target(name, FLANKED_REPEAT[name], prefix, suffix, tracts=tr.LOCI[name])
    rc.add_target("plain", cfg["repeat"]["c9orf72"][3], prefix, suffix)
    return rc


@pytest.fixture(scope="module")
def pipeline(pm, opm, orc, cfg):
    """[(item, row, record)]: the reads and what the reference makes of them, computed once."""
    from conftest import oracle_map
    from strique_amd import synth
    table = synth.KmerTable(pm)
    prefix, suffix = _full_flanks(cfg)
    params = orc.align_params(cfg["align"])
    jobs = []
    for i, (target, strand, planted, what) in enumerate(PIPELINE_READS):
        sig = pipeline_signal(table, cfg, i, target, strand, planted, what)
        repeat = cfg["repeat"]["c9orf72"][3] if target == "plain" else FLANKED_REPEAT[target]
        tc = orc.classifier(repeat, prefix, suffix, strand, opm, None, cfg["HMM"])
        m = None if target == "plain" else (tr.model(*tr.LOCI[target], prefix[-50:], suffix[:50], strand, opm, cfg["HMM"]), strand)
        jobs.append(((target, sig, strand), tc, m))
    done = oracle_map(lambda j: tr.record(j[0][1], j[1], j[2], opm, params), jobs)
    out = [(j[0], row, rec) for j, (row, rec) in zip(jobs, done)]
    # the cases are what they claim: the swapped read fails the gate, the plain read is decoded, every other read has a record
    for (target, strand, planted, what), (_, row, rec) in zip(PIPELINE_READS, out):
        assert (rec is not None) == (what == "read"), (target, strand, what, row)
        assert (row[3] == 0) == (what == "swapped"), (target, strand, what, row)
    return out


def _same_record(got, want, what):
    assert (got is None) == (want is None), (what, got, want)
    if want is not None:
        assert tuple(got[0]) == tuple(want[0]) and np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (what, got, want)


def test_pipeline_records_equal_the_reference(counter, pipeline):
    from strique_amd import ffi
    items = [it for it, _, _ in pipeline]
    ctx = counter.ctx
    off = counter.detect_batch(items, units=True, confidence=True, records=True)
    assert ctx.last_tracts() == {"ms": 0.0, "windows": 0, "launches": 0, "failed": 0} and all(d.tracts is None for d in off)
    with pytest.raises(ffi.StriqueHipError) as e:
        ctx.batch_fetch_tracts()                                 # the last run call ran with the switch off
    assert e.value.code == ffi.STRQ_ERR_ARG
    counter.set_tracts(True)
    try:
        on = counter.detect_batch(items, units=True, confidence=True, records=True)
        last = ctx.last_tracts()
        print("tract pass:", last, {t: (m.baked.n_states, ffi.debug_viterbi_plan(m.baked)["shape"]) for t, (m, _) in counter.tract_models.items()})
        n_dec = sum(1 for _, _, rec in pipeline if rec is not None)
        assert last["windows"] == n_dec and last["failed"] == 0 and last["launches"] >= 2 and last["ms"] > 0
        for d, (it, row, rec), plan in zip(on, pipeline, PIPELINE_READS):
            assert tuple(d.row[:6]) == tuple(row[:6]), (plan, d.row, row)
            _same_record(d.tracts, rec, plan)
            if plan[3] == "read":
                print(plan, "tracts", d.tracts[0], "flanked count", d.row[0])
        # rows, units and confidence: byte-equal with the switch on and off
        for x, y in zip(on, off):
            assert x.row == y.row and np.float64(x.row[3]).tobytes() == np.float64(y.row[3]).tobytes()
            assert (x.units is None) == (y.units is None) and (x.units is None or np.array_equal(x.units, y.units))
            assert (x.conf is None) == (y.conf is None) and (x.conf is None or np.array(x.conf).tobytes() == np.array(y.conf).tobytes())
        # across sub-batches, and serially
        try:
            ctx.set_option("STRQ_SUBBATCH_READS", "2")
            small = counter.detect_batch(items, records=True)
            assert ctx.last_tracts()["windows"] == n_dec
            ctx.set_option("STRQ_SUBBATCH_READS", None); ctx.set_option("STRQ_SERIAL", "1")
            serial = counter.detect_batch(items, records=True)
        finally:
            ctx.set_option("STRQ_SERIAL", None); ctx.set_option("STRQ_SUBBATCH_READS", None)
        for a, b, c, plan in zip(small, serial, on, PIPELINE_READS):
            assert a.row == c.row and b.row == c.row
            _same_record(a.tracts, c.tracts, plan); _same_record(b.tracts, c.tracts, plan)
        # the element detect_batch and detect document: last, behind the others
        pub = counter.detect_batch(items[:4], units=True)
        for (row_, pos, el), d in zip(pub, on):
            assert row_ == d.row and np.array_equal(pos, d.units)
            _same_record(el, d.tracts, "detect_batch")
        one = counter.detect(*items[2])
        assert one[0] == on[2].row
        _same_record(one[1], on[2].tracts, "detect")
        # through ffi.Context: records in model order, status per read
        tids = [counter._classifier_for(t, s).target_id for t, _, s in items]
        ctx.set_tracts(True)
        ctx.detect_batch_reads([np.ascontiguousarray(sig) for _, sig, _ in items], tids)
        raw = ctx.batch_fetch_tracts()
        from strique_amd import tracts
        for t, d, plan in zip(raw, on, PIPELINE_READS):
            assert int(t["status"]) == (0 if d.tracts is not None else 1), (plan, t)
            if d.tracts is not None:
                assert int(t["n_tracts"]) == len(d.tracts[0]) and float(t["log_p"]) == d.tracts[1]
                assert tracts.configured_order([int(c) for c in t["count"][:int(t["n_tracts"])]], plan[1]) == tuple(d.tracts[0])
            else:
                assert int(t["n_tracts"]) == 0 and not t["count"].any() and float(t["log_p"]) == 0.0
    finally:
        ctx.set_tracts(False)
        counter.set_tracts(False)
    # and off again: nothing is launched
    again = counter.detect_batch(items, records=True)
    assert [d.row for d in again] == [d.row for d in off] and ctx.last_tracts()["launches"] == 0


def test_refusals(counter, pm, cfg, pipeline):
    from strique_amd import ffi
    from strique_amd.counter import repeatCounter
    ctx = counter.ctx
    fresh = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    fresh.add_target("c9orf72", *cfg["repeat"]["c9orf72"][3:6])
    with pytest.raises(ValueError):
        fresh.set_tracts(True)                                   # no target with tracts
    assert fresh.tract_models == {}
    with pytest.raises(ValueError):
        fresh.add_target("bad", "CAG", *_full_flanks(cfg), tracts=(("CAG", "CAG"), ("",)))
    # a model without tracts, another number of tracts, an unknown target
    counter._ensure_tracts()
    tid = counter._classifier_for("htt_like", "+").target_id
    plain_model = counter._classifier_for("plain", "+").repeatHMM.model_id
    m = counter.tract_models[tid][0]
    for args in ((tid, plain_model, 2, (0, 0)), (tid, m.model_id, 3, (0, 0, 0)), (10 ** 6, m.model_id, 2, (0, 0))):
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.target_set_tracts(*args)
        assert e.value.code == ffi.STRQ_ERR_ARG
    # a scan with the switch on, through the counter and through the context
    counter.set_tracts(True)
    try:
        with pytest.raises(ValueError):
            counter.scan_batch([pipeline[0][0][1]], min_score=5.0)
    finally:
        counter.set_tracts(False)
    ids = [counter._classifier_for(t, st).target_id for t, st in counter.candidates()]
    sig = np.ascontiguousarray(pipeline[0][0][1])
    try:
        ctx.set_tracts(True)
        ctx.batch_upload(sig, [0, len(sig)], [ids[0]])
        ctx.scan_set(ids, 5.0)
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.batch_run()
        assert e.value.code == ffi.STRQ_ERR_ARG and "scan" in str(e.value)
    finally:
        ctx.scan_clear(); ctx.set_tracts(False)
    # taken away: the target's reads report nothing, and the definition comes back on the next use
    ctx.target_set_tracts(tid, -1)
    del counter.tract_models[tid]
    counter.set_tracts(True)
    try:
        d = counter.detect_batch([pipeline[0][0]], records=True)[0]
        _same_record(d.tracts, pipeline[0][2], "registered again")
    finally:
        counter.set_tracts(False)


def test_count_command_with_tracts(tmp_path, tables, cfg, pipeline):
    """`count ... --tract-units defs.tsv --tracts out.tsv` from written fast5 files: the count TSV is byte-identical to a run without
    the flags, the side file parses back to the reference's records."""
    import io
    import json
    from contextlib import redirect_stdout
    import h5write
    from strique_amd import cli, tracts
    prefix, suffix = _full_flanks(cfg)
    with open(tmp_path / "r9_4_450bps.model", "w") as fp:
        for k, mu, sd in zip(tables["base_kmer"], tables["base_mean"], tables["base_stdv"]):
            fp.write("%s\t%s\t%s\t1\n" % (k.decode() if isinstance(k, bytes) else str(k), repr(float(mu)), repr(float(sd))))
    loci = {"htt_like": ("chrA", 50000, 50100), "cnbp_like": ("chrB", 70000, 70100), "plain": ("chrC", 90000, 90100)}
    with open(tmp_path / "repeat_config.tsv", "w") as fp:
        fp.write("chr\tbegin\tend\tname\trepeat\tprefix\tsuffix\n")
        for name, (chrom, b, e) in loci.items():
            fp.write("\t".join([chrom, str(b), str(e), name, FLANKED_REPEAT.get(name, cfg["repeat"]["c9orf72"][3]), prefix, suffix]) + "\n")
    with open(tmp_path / "STRique.json", "w") as fp:
        json.dump({"align": cfg["align"], "HMM": cfg["HMM"]}, fp)
    with open(tmp_path / "defs.tsv", "w") as fp:
        fp.write("# compound loci\n\nhtt_like\tCAG,CCG\tCAACAG\ncnbp_like\tCCTG,TCTG,TG\t-\n")
    reads, sam = [], ["@HD\tVN:1.0"]
    for i, ((target, sig, strand), row, rec) in enumerate(pipeline):
        rid = "%08d-2222-4000-8000-%012d" % (i, i)
        reads.append((rid, sig))
        chrom, b, e = loci[target]
        sam.append("\t".join([rid, "16" if strand == "-" else "0", chrom, str(b - 3000), "60", "12S6000M5S", "*", "0", "0", "ACGT", "*"]))
    bulk = tmp_path / "bulk"; bulk.mkdir()
    (bulk / "batch_0.fast5").write_bytes(h5write.multi_read_fast5(reads))
    buf = io.StringIO()
    with redirect_stdout(buf):
        cli.main(["index", str(bulk)])
    (bulk / "reads.fofn").write_text(buf.getvalue())
    (tmp_path / "aln.sam").write_text("\n".join(sam) + "\n")
    base = ["count", str(bulk / "reads.fofn"), str(tmp_path / "r9_4_450bps.model"), str(tmp_path / "repeat_config.tsv"),
            "--config", str(tmp_path / "STRique.json"), "--algn", str(tmp_path / "aln.sam"), "--batch", "4"]
    cli.main(base + ["--out", str(tmp_path / "plain.tsv")])
    cli.main(base + ["--out", str(tmp_path / "with.tsv"), "--tract-units", str(tmp_path / "defs.tsv"), "--tracts", str(tmp_path / "tracts.tsv")])
    assert (tmp_path / "with.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    count_rows = (tmp_path / "plain.tsv").read_text().splitlines()[1:]
    with open(tmp_path / "tracts.tsv") as fp:
        rows = tracts.parse(fp)
    assert len(rows) == len(count_rows) == len(pipeline)
    for got, line, (rid, _), ((target, _, strand), row, rec) in zip(rows, count_rows, reads, pipeline):
        assert got[:3] == (rid, target, strand) and got[3] == row[0] == int(line.split("\t")[3])
        _same_record(got[4], rec, rid)
    # each of the two flags needs the other, and neither goes with --scan
    for bad in (["--tracts", str(tmp_path / "t.tsv")], ["--tract-units", str(tmp_path / "defs.tsv")]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
