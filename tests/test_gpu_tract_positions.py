"""Tract positions on the GPU (strq_viterbi_tract_positions, strq_set_tract_positions) against tests/tract_pos_ref.py: the positions
of every tract equal the ones read off the oracle's path, the log-probability has the bits of strq_viterbi_tracts and the counts are
equal.  Every comparison is exact.

Model level: the random baked models of tests/vit_mode_cases.py with their counted emitting states dealt to two or three tracts --
the states of different tracts then interleave along a path, which real loci never do -- on every lane row in both single-stage forms
and the general kernel, windows at the edges of the ballot rounds, and the pieces of the back-pointer budget.  Pipeline: the nine
reads of tests/tract_pos_cases.py across sub-batches of two, through detect, detect_batch, ffi.Context and `count --tract-positions`."""
import numpy as np
import pytest

import tract_pos_cases as tpc
import tract_pos_ref as tpr
import tract_ref as tr
import vit_mode_cases as vc

pytestmark = pytest.mark.gpu

GENERATED = ["row%d_%s" % (row, v) for row in range(8) for v in ("ss", "multi")] + ["general"]
ROUND_EDGES = (41, 63, 64, 65, 128, 129, 300)
OVER_BUDGET = 4          # status of strq_viterbi_tract_positions: counts valid, back-pointers over the budget


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
    """1 and 2 observations, the lengths around the ballot rounds of 64, a window with missing observations, an all-NaN window and
    one without a path."""
    w = dict(case.windows)
    return ([("T1", w["T1"]), ("T2", w["T2"])] + [("T%d" % T, w["T333"][:T]) for T in ROUND_EDGES] +
            [("nan7", w["nan7"]), ("allnan", w["allnan"]), ("nopath", w["nopath"])])


def tracts_of(bk):
    return 3 if int((np.asarray(bk.count_inc)[:bk.silent_start] == 1).sum()) >= 3 else 2          # (the rows with unit records have two counted states)


def bp_bytes(bk, T):
    return (((T + 1) * bk.n_states * 2) + 15) & ~15


NO_INTERLEAVE = {"row6_ss"}          # the reference's paths on this model visit its counted states a few times only, tract after tract


def interleaved(ref):
    """Two tracts of a decoded window whose position ranges overlap."""
    p = [q for q in ref[2] if len(q)] if ref[3] == 0 else []
    return any(a is not b and b[0] < a[-1] and a[0] < b[-1] for a in p for b in p)


def check_window(got, i, ref, K, what):
    logp, counts, status, pos = got
    rl, rc, rp, rs = ref
    w = what + (float(logp[i]), [int(v) for v in counts[i]], int(status[i]), rl, rc, rs)
    assert int(status[i]) == rs, w
    assert [int(v) for v in counts[i]] == rc + [0] * (3 - K), w
    if rs == 0:
        assert np.float64(logp[i]).tobytes() == np.float64(rl).tobytes(), w
        assert tpr.same_positions(pos[i][:K], rp), w + ([p.tolist() for p in pos[i]], [p.tolist() for p in rp])
        assert all(len(p) == 0 for p in pos[i][K:]), w
        for p, n in zip(pos[i][:K], rc):
            assert len(p) == n and (np.diff(p) > 0).all()
    else:
        assert logp[i] == -np.inf and all(len(p) == 0 for p in pos[i]), w          # no path: empty positions, and no flag (the call returned)


@pytest.mark.parametrize("name", GENERATED)
def test_generated_models_against_the_reference(ctx, all_cases, name):
    from strique_amd import ffi
    c = all_cases[name]
    bk = c.baked
    K = tracts_of(bk)
    tract_of = spread(bk, K)
    mid = ctx.model_create(bk)
    ctx.model_set_tracts(mid, K, tract_of)
    plan = ffi.debug_viterbi_plan(bk)
    assert plan["shape"] == (vc.SHAPE_CSR if c.row == vc.SHAPE_CSR else c.row | (vc.SHAPE_SS if c.ss else 0)), (name, plan)
    labels = [l for l, _ in windows_of(c)]; xs = [x for _, x in windows_of(c)]
    refs = [tpr.decode(bk, tract_of, K, x) for x in xs]
    # the cases are what they claim: a window without a path, a decoded window whose path has no counted emission of one tract,
    # and paths on which the tracts interleave
    assert refs[labels.index("nopath")][3] == 1
    assert any(r[3] == 0 and min(r[1]) == 0 for r in refs), name
    assert any(interleaved(r) for r in refs) == (name not in NO_INTERLEAVE), name
    got = ctx.viterbi_tract_positions(mid, xs)
    assert ctx.debug_tract_shape() == plan["shape"], (name, ctx.debug_tract_shape(), plan["shape"])
    for i, label in enumerate(labels):
        check_window(got, i, refs[i], K, (name, label))
    # the count side is strq_viterbi_tracts, bit for bit
    logp, counts, status = ctx.viterbi_tracts(mid, xs)
    assert np.asarray(logp).tobytes() == np.asarray(got[0]).tobytes() and np.array_equal(counts, got[1]) and np.array_equal(status, got[2]), name
    # ragged batch: every window alone gives what it gave in the batch
    for i, x in enumerate(xs):
        one = ctx.viterbi_tract_positions(mid, [x])
        assert np.float64(one[0][0]).tobytes() == np.float64(got[0][i]).tobytes() and np.array_equal(one[1][0], got[1][i]) and one[2][0] == got[2][i], (name, labels[i])
        assert tpr.same_positions(one[3][0], got[3][i]), (name, labels[i])


@pytest.mark.parametrize("name", ["row0_multi", "row4_ss", "general"])
def test_pieces_of_the_back_pointer_budget(ctx, all_cases, name):
    """Four windows of 63 .. 66 observations: a budget that holds one of them per piece, one that holds two, and the default give the
    same result; a budget below the smallest window gives no positions and the counts as they are."""
    c = all_cases[name]
    bk = c.baked
    K = tracts_of(bk)
    tract_of = spread(bk, K)
    mid = ctx.model_create(bk)
    ctx.model_set_tracts(mid, K, tract_of)
    base = dict(c.windows)["T333"]
    xs = [base[:T] for T in (64, 65, 63, 66)]
    refs = [tpr.decode(bk, tract_of, K, x) for x in xs]
    assert all(r[3] == 0 for r in refs)
    one, two = bp_bytes(bk, 66), 2 * bp_bytes(bk, 66)
    assert bp_bytes(bk, 63) + bp_bytes(bk, 64) > one and bp_bytes(bk, 63) + bp_bytes(bk, 64) + bp_bytes(bk, 65) > two
    whole = ctx.viterbi_tract_positions(mid, xs)
    for i in range(len(xs)):
        check_window(whole, i, refs[i], K, (name, "whole", i))
    try:
        for budget in (one, two):
            ctx.set_option("STRQ_TRACT_POS_WS_BYTES", str(budget))
            got = ctx.viterbi_tract_positions(mid, xs)
            for i in range(len(xs)):
                check_window(got, i, refs[i], K, (name, budget, i))
        ctx.set_option("STRQ_TRACT_POS_WS_BYTES", str(bp_bytes(bk, 63) - 16))
        logp, counts, status, pos = ctx.viterbi_tract_positions(mid, xs)
        assert [int(s) for s in status] == [OVER_BUDGET] * 4
        assert np.asarray(logp).tobytes() == np.asarray(whole[0]).tobytes() and np.array_equal(counts, whole[1])
        assert all(len(p) == 0 for ps in pos for p in ps)
    finally:
        ctx.set_option("STRQ_TRACT_POS_WS_BYTES", None)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counter(pm, cfg):
    from strique_amd.counter import repeatCounter
    prefix, suffix = tpc.full_flanks(cfg)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in sorted(tr.LOCI):
        rc.add_target(name, tpc.FLANKED_REPEAT[name], prefix, suffix, tracts=tr.LOCI[name])
    rc.add_target("plain", cfg["repeat"]["c9orf72"][3], prefix, suffix)
    return rc


@pytest.fixture(scope="module")
def pipeline(pm, opm, orc, cfg):
    return tpc.pipeline(pm, opm, orc, cfg)


def _same_record(got, want, what):
    """(counts, log_p, positions) of the product against the reference's: counts, log-probability bits, positions tract by tract."""
    assert (got is None) == (want is None), (what, got, want)
    if want is not None:
        assert tuple(got[0]) == tuple(want[0]) and np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (what, got[:2], want[:2])
        assert got[2] is not None and tpr.same_positions(got[2], want[2]), (what, [np.asarray(p).tolist() for p in got[2]], [p.tolist() for p in want[2]])


def test_pipeline_positions_equal_the_reference(counter, pipeline):
    from strique_amd import ffi, tracts
    items = [p[0] for p in pipeline]
    ctx = counter.ctx
    n_dec = sum(1 for p in pipeline if p[2] is not None)
    counter.set_tracts(True)
    try:
        off = counter.detect_batch(items, units=True, confidence=True, records=True)
        assert ctx.last_tract_positions() == {"ms": 0.0, "windows": 0, "launches": 0, "bp_bytes": 0.0}
        assert all(d.tracts is None or len(d.tracts) == 2 for d in off)
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.batch_fetch_tract_positions()                        # the last run call ran with the switch off
        assert e.value.code == ffi.STRQ_ERR_ARG
        counter.set_tracts(True, positions=True)
        try:
            ctx.set_option("STRQ_SUBBATCH_READS", "2")
            on = counter.detect_batch(items, units=True, confidence=True, records=True)
            last = ctx.last_tract_positions()
        finally:
            ctx.set_option("STRQ_SUBBATCH_READS", None)
        print("tract-position pass:", last)
        assert last["windows"] == n_dec and last["launches"] >= 3 and last["ms"] > 0 and last["bp_bytes"] > 0
        for d, (it, row, rec, _, _), plan in zip(on, pipeline, tpc.PIPELINE_READS):
            assert tuple(d.row[:6]) == tuple(row[:6]), (plan, d.row, row)
            _same_record(d.tracts, rec, plan)
            if rec is not None:
                print(plan, "counts", d.tracts[0], "spans", tracts.spans(d.tracts[2]))
        # rows, tract records, units and confidence: byte-equal with the switch on and off
        for x, y in zip(on, off):
            assert x.row == y.row and np.float64(x.row[3]).tobytes() == np.float64(y.row[3]).tobytes()
            assert (x.tracts is None) == (y.tracts is None)
            assert x.tracts is None or (x.tracts[0] == y.tracts[0] and np.float64(x.tracts[1]).tobytes() == np.float64(y.tracts[1]).tobytes())
            assert (x.units is None) == (y.units is None) and (x.units is None or np.array_equal(x.units, y.units))
            assert (x.conf is None) == (y.conf is None) and (x.conf is None or np.array(x.conf).tobytes() == np.array(y.conf).tobytes())
        # one sub-batch, detect_batch's tuple and detect agree with the records
        pub = counter.detect_batch(items[:4], units=True)
        for (row_, pos, el), d in zip(pub, on):
            assert row_ == d.row and np.array_equal(pos, d.units)
            _same_record(el, d.tracts, "detect_batch")
        one = counter.detect(*items[2])
        assert one[0] == on[2].row
        _same_record(one[1], on[2].tracts, "detect")
        # a budget no window fits: no positions, the counts stay
        try:
            ctx.set_option("STRQ_TRACT_POS_WS_BYTES", "4096")
            none = counter.detect_batch(items, records=True)
            assert ctx.last_tract_positions()["windows"] == 0
        finally:
            ctx.set_option("STRQ_TRACT_POS_WS_BYTES", None)
        for x, y in zip(none, on):
            assert (x.tracts is None) == (y.tracts is None) and (x.tracts is None or (x.tracts[:2] == y.tracts[:2] and x.tracts[2] is None))
    finally:
        counter.set_tracts(False)
    # through ffi.Context: positions in model order, a status per read; the switch without set_tracts is refused
    tids = [counter._classifier_for(t, s).target_id for t, _, s in items]
    sigs = [np.ascontiguousarray(sig) for _, sig, _ in items]
    try:
        ctx.set_tract_positions(True)
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.detect_batch_reads(sigs, tids)
        assert e.value.code == ffi.STRQ_ERR_ARG and "strq_set_tracts" in str(e.value)
        ctx.set_tracts(True)
        ctx.detect_batch_reads(sigs, tids)
        raw = ctx.batch_fetch_tract_positions()
        recs = ctx.batch_fetch_tracts()
        for (ps, pos), t, d, plan in zip(raw, recs, on, tpc.PIPELINE_READS):
            assert ps == (0 if d.tracts is not None else 1) and (pos is None) == (d.tracts is None), (plan, ps)
            if d.tracts is not None:
                k = int(t["n_tracts"])
                assert tpr.same_positions(tracts.configured_order(pos[:k], plan[1]), d.tracts[2]) and all(len(p) == 0 for p in pos[k:]), plan
    finally:
        ctx.set_tract_positions(False); ctx.set_tracts(False)
    again = counter.detect_batch(items, records=True)
    assert [d.row for d in again] == [d.row for d in off] and ctx.last_tract_positions()["launches"] == 0 and all(d.tracts is None for d in again)


def test_count_command_with_tract_positions(tmp_path, tables, cfg, pipeline):
    """`count ... --tract-units defs.tsv --tracts out.tsv --tract-positions pos.tsv` from written fast5 files: the count TSV and the
    tracts file are byte-identical to a run without the flag, the positions file parses back to the reference's records, one row
    per count row."""
    import io
    import json
    from contextlib import redirect_stdout
    import h5write
    from strique_amd import cli, tracts
    prefix, suffix = tpc.full_flanks(cfg)
    with open(tmp_path / "r9_4_450bps.model", "w") as fp:
        for k, mu, sd in zip(tables["base_kmer"], tables["base_mean"], tables["base_stdv"]):
            fp.write("%s\t%s\t%s\t1\n" % (k.decode() if isinstance(k, bytes) else str(k), repr(float(mu)), repr(float(sd))))
    loci = {"htt_like": ("chrA", 50000, 50100), "cnbp_like": ("chrB", 70000, 70100), "plain": ("chrC", 90000, 90100)}
    with open(tmp_path / "repeat_config.tsv", "w") as fp:
        fp.write("chr\tbegin\tend\tname\trepeat\tprefix\tsuffix\n")
        for name, (chrom, b, e) in loci.items():
            fp.write("\t".join([chrom, str(b), str(e), name, tpc.FLANKED_REPEAT.get(name, cfg["repeat"]["c9orf72"][3]), prefix, suffix]) + "\n")
    with open(tmp_path / "STRique.json", "w") as fp:
        json.dump({"align": cfg["align"], "HMM": cfg["HMM"]}, fp)
    with open(tmp_path / "defs.tsv", "w") as fp:
        fp.write("htt_like\tCAG,CCG\tCAACAG\ncnbp_like\tCCTG,TCTG,TG\t-\n")
    reads, sam = [], ["@HD\tVN:1.0"]
    for i, ((target, sig, strand), row, rec, _, _) in enumerate(pipeline):
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
            "--config", str(tmp_path / "STRique.json"), "--algn", str(tmp_path / "aln.sam"), "--batch", "4", "--tract-units", str(tmp_path / "defs.tsv")]
    cli.main(base + ["--out", str(tmp_path / "plain.tsv"), "--tracts", str(tmp_path / "tracts0.tsv")])
    cli.main(base + ["--out", str(tmp_path / "with.tsv"), "--tracts", str(tmp_path / "tracts1.tsv"), "--tract-positions", str(tmp_path / "pos.tsv")])
    assert (tmp_path / "with.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    assert (tmp_path / "tracts1.tsv").read_bytes() == (tmp_path / "tracts0.tsv").read_bytes()
    count_rows = (tmp_path / "plain.tsv").read_text().splitlines()[1:]
    with open(tmp_path / "pos.tsv") as fp:
        rows = tracts.parse_positions(fp)
    assert len(rows) == len(count_rows) == len(pipeline)
    for got, line, (rid, _), ((target, _, strand), row, rec, _, _) in zip(rows, count_rows, reads, pipeline):
        assert got[:3] == (rid, target, strand) and got[3] == row[0] == int(line.split("\t")[3])
        assert (got[4] is None) == (rec is None), rid
        if rec is not None:
            counts, sp, pos = got[4]
            assert counts == tuple(rec[0]) and tpr.same_positions(pos, rec[2]) and sp == tuple((int(p[0]), int(p[-1])) for p in rec[2]), rid
