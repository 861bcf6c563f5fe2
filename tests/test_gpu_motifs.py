"""The motif track on the GPU (strq_motif_track, csrc/motif_kernels.hip) against tests/motif_ref.py.  Every comparison is exact: V has
the reference's bits, winners, observations won and majority are equal.

Model level: K = 2, 3 and 4 candidates with units of 1, 3, 5, 6 and 31 nt; windows at every length around the segment length S = 64
(1, 63, 64, 65, 127, 128, 129, 300), one long enough for several waves (1000: 15 segments, four tasks), one with a few missing
observations and one all-NaN; every window alone and the windows in reverse order give the bits they gave in the batch; other
segment lengths (32: eight segments per wave, 256: one); the refusals.

Pipeline (strq_set_motifs, repeatCounter.motifs_batch / set_motifs): clean synthetic reads of two loci on both strands -- pure arrays of
every candidate, two mixed arrays, a read whose gate fails and one of a target without motifs -- against the reference's records,
count under the majority unit included; rows, units and confidence byte-equal with the switch on and off, across sub-batches and
serially; the refusals; one `count --motif-units --motifs` run from written fast5 files, read back with motifs.parse."""
import numpy as np
import pytest

import motif_ref as mr
from conftest import oracle_map

pytestmark = pytest.mark.gpu

S = 64
U31 = "ACGTTGCATCAGGATCCATGGTACCAGTTAC"
SETS = {"K2": ("GAA", "GAAGGA"), "K3": ("AAAAG", "AAAGG", "AAGGG"), "K4": ("A", "GAA", "AAGGG", U31)}
LENGTHS = (1, 63, 64, 65, 127, 128, 129, 300, 1000)


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    return ffi.Context(0)


def _signal(opm, rng, array, T):
    """T observations of the k-mer means of `array` (six each) with a little seeded noise, clipped into the emission range."""
    while (len(array) - opm.kmer + 1) * 6 < T:
        array += array
    x = opm.template(array, 6)[:T] + rng.normal(0.0, 1.0, T)
    return np.clip(x, opm.model_min + .5, opm.model_max - .5)


def windows_of(opm, units, seed):
    """[(label, x)]: the lengths around S on arrays of the candidates in turn, a change-over in the long one, missing observations."""
    rng = np.random.Generator(np.random.PCG64(seed))
    K = len(units)
    out = []
    for i, T in enumerate(LENGTHS):
        array = units[i % K] * (240 // len(units[i % K]) + 1)
        if T == 1000:
            array = units[0] * (100 // len(units[0]) + 1) + units[K - 1] * (100 // len(units[K - 1]) + 1)
        out.append(("T%d" % T, _signal(opm, rng, array, T)))
    x = _signal(opm, rng, units[1] * 60, 200)
    x[[0, 63, 64, 100, 199]] = np.nan
    out.append(("nan5", x))
    out.append(("allnan", np.full(130, np.nan)))
    return out


@pytest.fixture(scope="module")
def shared(opm, cfg):
    """name -> (units, reference loop models, windows, reference track of every window at S): computed once."""
    out = {}
    for seed, (name, units) in enumerate(sorted(SETS.items())):
        models = [mr.loop(u, opm, cfg["HMM"]) for u in units]
        wins = windows_of(opm, units, 11 + seed)
        ref = oracle_map(lambda w: mr.track(models, w[1], S), wins)
        out[name] = (units, models, wins, ref)
    return out


def _register(ctx, pm, cfg, units):
    from strique_amd import motifs
    return [ctx.model_create(motifs.loop_model(u, pm, cfg["HMM"])) for u in units]


def _equal(got, want, what):
    V, win, won, maj = got
    rV, rwin, rwon, rmaj, _ = want
    assert V.shape == rV.shape, what
    assert V.tobytes() == rV.tobytes(), what + (V, rV)
    assert [int(w) for w in win] == rwin and [int(o) for o in won] == rwon and maj == rmaj, what + (win, rwin, won, rwon, maj, rmaj)


@pytest.mark.parametrize("name", sorted(SETS))
def test_track_against_the_reference(ctx, pm, cfg, shared, name):
    units, models, wins, ref = shared[name]
    ids = _register(ctx, pm, cfg, units)
    xs = [x for _, x in wins]
    got = ctx.motif_track(ids, xs, S)
    assert len(got) == len(xs)
    for (label, x), g, r in zip(wins, got, ref):
        assert len(g[0]) == max(1, len(x) // S)
        _equal(g, r, (name, label))
    # the winners mean something: a clean array of one candidate is won by it, segment by segment
    for i, (label, x) in enumerate(wins[3:8], 3):
        assert set(int(w) for w in got[i][1]) == {i % len(units)}, (name, label, got[i][1])
    # every window alone gives the bits it gave in the batch
    for (label, x), g in zip(wins, got):
        one = ctx.motif_track(ids, [x], S)[0]
        assert one[0].tobytes() == g[0].tobytes() and np.array_equal(one[1], g[1]) and np.array_equal(one[2], g[2]) and one[3] == g[3], (name, label)
    # ... and so do the windows in reverse order
    back = ctx.motif_track(ids, xs[::-1], S)[::-1]
    for (label, x), g, b in zip(wins, got, back):
        assert b[0].tobytes() == g[0].tobytes() and np.array_equal(b[1], g[1]) and np.array_equal(b[2], g[2]) and b[3] == g[3], (name, label)


@pytest.mark.parametrize("segment", (32, 256))
def test_other_segment_lengths(ctx, pm, cfg, shared, segment):
    units, models, wins, _ = shared["K3"]
    ids = _register(ctx, pm, cfg, units)
    pick = [w for w in wins if w[0] in ("T1", "T300", "T1000", "nan5")]
    got = ctx.motif_track(ids, [x for _, x in pick], segment)
    ref = oracle_map(lambda w: mr.track(models, w[1], segment), pick)
    for (label, x), g, r in zip(pick, got, ref):
        _equal(g, r, (segment, label))
    # the second evaluation of the reference has the same bits
    rb = mr.track(models, pick[1][1], segment, score=mr.score_b)
    assert rb[0].tobytes() == ref[1][0].tobytes()


def test_refusals(ctx, pm, cfg):
    from strique_amd import ffi, hmm, motifs
    ids = _register(ctx, pm, cfg, SETS["K2"])
    x = [np.zeros(70) + 90.0]
    for bad in (31, 4097):
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.motif_track(ids, x, bad)
        assert e.value.code == ffi.STRQ_ERR_ARG
    for bad_ids in (ids[:1], ids + ids + ids[:1], [ids[0], 10 ** 6]):
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.motif_track(bad_ids, x, S)
        assert e.value.code == ffi.STRQ_ERR_ARG
    with pytest.raises(ValueError):
        ctx.motif_track(ids, [np.zeros(0)], S)
    prefix, suffix = (s.upper() for s in cfg["repeat"]["c9orf72"][4:6])
    flanked = ctx.model_create(hmm.FlankedRepeatModel("GAA", prefix[-50:], suffix[:50], pm, cfg["HMM"]).baked)
    with pytest.raises(ffi.StriqueHipError) as e:
        ctx.motif_track([ids[0], flanked], x, S)
    assert e.value.code == ffi.STRQ_ERR_UNSUPPORTED and "motifs" in str(e.value)
    assert ctx.motif_track(ids, [], S) == []


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
# Clean synthetic reads of 8 000 nt: c9orf72's flanks around an array given whole, once.  (target, array as (candidate, units) runs,
# what) x strands: pure arrays of every candidate, two mixed arrays, a read whose gate fails (its flanks in the wrong order) and a
# read of a target without motifs.
TARGETS = {"rfc1": ("AAAAG", ("AAAGG", "AAGGG")), "fgf14": ("GAA", ("GAAGGA",))}
CASES = [("rfc1", ((0, 40),), "read"), ("rfc1", ((1, 40),), "read"), ("rfc1", ((2, 40),), "read"), ("fgf14", ((0, 40),), "read"), ("fgf14", ((1, 40),), "read"),
         ("rfc1", ((0, 30), (2, 30)), "read"), ("fgf14", ((0, 50), (1, 30)), "read")]
PIPELINE_READS = [c + (s,) for c in CASES for s in "+-"] + [("rfc1", ((0, 40),), "swapped", "+"), ("plain", None, "plain", "+")]
SEGMENT = 256


def _full_flanks(cfg):
    return cfg["repeat"]["c9orf72"][4].upper(), cfg["repeat"]["c9orf72"][5].upper()


def _units(target):
    return (TARGETS[target][0],) + TARGETS[target][1]


def pipeline_signal(table, cfg, i, target, array, what, strand):
    from strique_amd import synth
    prefix, suffix = _full_flanks(cfg)
    rng = np.random.Generator(np.random.PCG64(9000 + i))
    if what == "plain":
        seq = synth.make_sequence(rng, 8000, prefix, cfg["repeat"]["c9orf72"][3], 20, suffix, strand)
    else:
        text = "".join(_units(target)[j] * n for j, n in array)
        seq = synth.make_sequence(rng, 8000, suffix, text, 1, prefix, strand) if what == "swapped" else synth.make_sequence(rng, 8000, prefix, text, 1, suffix, strand)
    return synth.make_signal(rng, table, seq, True, 0.0, noise=None)


@pytest.fixture(scope="module")
def counter(pm, cfg):
    from strique_amd.counter import repeatCounter
    prefix, suffix = _full_flanks(cfg)
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name, (repeat, alts) in sorted(TARGETS.items()):
        rc.add_target(name, repeat, prefix, suffix, motifs=list(alts))
    rc.add_target("plain", cfg["repeat"]["c9orf72"][3], prefix, suffix)
    return rc


@pytest.fixture(scope="module")
def pipeline(pm, opm, orc, cfg):
    """[(item, row, record)]: the reads and what the reference makes of them, computed once."""
    from strique_amd import synth
    table = synth.KmerTable(pm)
    prefix, suffix = _full_flanks(cfg)
    params = orc.align_params(cfg["align"])
    jobs = []
    for i, (target, array, what, strand) in enumerate(PIPELINE_READS, 1):
        sig = pipeline_signal(table, cfg, i, target, array, what, strand)
        repeat, alts = TARGETS[target] if target in TARGETS else (cfg["repeat"]["c9orf72"][3], None)
        jobs.append(((target, sig, strand), repeat, alts))
    done = oracle_map(lambda j: mr.record(j[0][1], j[1], j[2], prefix, suffix, j[0][2], opm, params, cfg["HMM"], SEGMENT), jobs)
    out = [(j[0], row, rec) for j, (row, rec) in zip(jobs, done)]
    # the cases are what they claim: the swapped read fails the gate, the plain read has a row and no record, every other read has a
    # record; and on every clean pure-array read every segment's winner is the planted unit
    for (target, array, what, strand), (_, row, rec) in zip(PIPELINE_READS, out):
        assert (rec is not None) == (what == "read"), (target, strand, what, row)
        assert (row[3] == 0) == (what == "swapped"), (target, strand, what, row)
        if what == "read" and len(array) == 1:
            assert set(rec[5]) == {array[0][0]} and rec[0] == array[0][0], (target, array, strand, rec[5])
    return out


def _same_record(got, want, what):
    assert (got is None) == (want is None), (what, got, want)
    if want is None:
        return
    majority, shares, count_m, log_p_m, runs, win, V = got
    assert majority == want[0] and tuple(shares) == tuple(want[1]) and runs == want[4], (what, got[:5], want[:5])
    assert [int(w) for w in win] == want[5] and np.asarray(V).tobytes() == want[6].tobytes() and np.asarray(V).shape == want[6].shape, (what, win, want[5])
    assert count_m == want[2] and (log_p_m is None) == (want[3] is None), (what, count_m, log_p_m, want[2], want[3])
    if want[3] is not None:
        assert np.float64(log_p_m).tobytes() == np.float64(want[3]).tobytes(), (what, log_p_m, want[3])


def test_pipeline_records_equal_the_reference(counter, pipeline):
    from strique_amd import ffi
    items = [it for it, _, _ in pipeline]
    ctx = counter.ctx
    off = counter.detect_batch(items, units=True, confidence=True, records=True)
    assert ctx.last_motifs() == {"ms": 0.0, "reads": 0, "segments": 0, "launches": 0, "decodes": 0}
    with pytest.raises(ffi.StriqueHipError) as e:
        ctx.batch_fetch_motifs()                                 # the last run call ran with the switch off
    assert e.value.code == ffi.STRQ_ERR_ARG
    on = counter.motifs_batch(items, SEGMENT)
    last = ctx.last_motifs()
    print("motif pass:", last)
    scored = [rec for _, _, rec in pipeline if rec is not None]
    assert last["reads"] == len(scored) and last["segments"] == sum(len(r[5]) for r in scored) and last["ms"] > 0
    assert last["decodes"] == sum(1 for r in scored if r[0] != 0) and last["launches"] >= 2 + (2 if last["decodes"] else 0)
    for (row_, rec_), (it, row, rec), plan in zip(on, pipeline, PIPELINE_READS):
        assert tuple(row_[:6]) == tuple(row[:6]), (plan[:1] + plan[2:], row_, row)
        _same_record(rec_, rec, plan)
        if rec is not None:
            print(plan, "majority", rec_[0], "shares", ["%.4f" % s for s in rec_[1]], "count_m", rec_[2], "row count", row_[0], "runs", rec_[4])
    # rows, units and confidence: byte-equal with the switch on and off
    try:
        ctx.set_motifs(True, SEGMENT)
        with_switch = counter.detect_batch(items, units=True, confidence=True, records=True)
        assert ctx.last_motifs()["reads"] == len(scored)
    finally:
        ctx.set_motifs(False)
    for x, y, (row_, _) in zip(with_switch, off, on):
        assert x.row == y.row == row_ and np.float64(x.row[3]).tobytes() == np.float64(y.row[3]).tobytes()
        assert (x.units is None) == (y.units is None) and (x.units is None or np.array_equal(x.units, y.units))
        assert (x.conf is None) == (y.conf is None) and (x.conf is None or np.array(x.conf).tobytes() == np.array(y.conf).tobytes())
    # across sub-batches, and serially
    try:
        ctx.set_option("STRQ_SUBBATCH_READS", "2")
        small = counter.motifs_batch(items, SEGMENT)
        assert ctx.last_motifs()["reads"] == len(scored)
        ctx.set_option("STRQ_SUBBATCH_READS", None); ctx.set_option("STRQ_SERIAL", "1")
        serial = counter.motifs_batch(items, SEGMENT)
    finally:
        ctx.set_option("STRQ_SERIAL", None); ctx.set_option("STRQ_SUBBATCH_READS", None)
    for a, b, (_, row, rec), plan in zip(small, serial, pipeline, PIPELINE_READS):
        assert a[0] == b[0] and tuple(a[0][:6]) == tuple(row[:6])
        _same_record(a[1], rec, plan); _same_record(b[1], rec, plan)
    # and off again: nothing is launched
    again = counter.detect_batch(items, records=True)
    assert [d.row for d in again] == [d.row for d in off] and ctx.last_motifs()["launches"] == 0


def test_another_segment_length_in_the_pipeline(counter, pipeline, opm, orc, cfg):
    prefix, suffix = _full_flanks(cfg)
    pick = [k for k, plan in enumerate(PIPELINE_READS) if plan[0] == "fgf14" and len(plan[1]) == 2]
    got = counter.motifs_batch([pipeline[k][0] for k in pick], 64)
    for k, (row_, rec_) in zip(pick, got):
        (target, sig, strand), row, _ = pipeline[k]
        _, want = mr.record(sig, TARGETS[target][0], TARGETS[target][1], prefix, suffix, strand, opm, orc.align_params(cfg["align"]), cfg["HMM"], 64)
        _same_record(rec_, want, (PIPELINE_READS[k], 64))


def test_pipeline_refusals(counter, pm, cfg, pipeline):
    from strique_amd import ffi
    from strique_amd.counter import repeatCounter
    ctx = counter.ctx
    fresh = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    fresh.add_target("c9orf72", *cfg["repeat"]["c9orf72"][3:6])
    with pytest.raises(ValueError):
        fresh.motifs_batch([pipeline[0][0]])                     # no target with motifs
    with pytest.raises(ValueError):
        fresh.add_target("bad", "AAAAG", *_full_flanks(cfg), motifs=["AAAGA"])
    with pytest.raises(ValueError):
        counter.motifs_batch([pipeline[0][0]], 16)
    for bad in (31, 4097):
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.set_motifs(True, bad)
        assert e.value.code == ffi.STRQ_ERR_ARG
    # a candidate that is no loop model, an unknown target
    counter._ensure_motifs()
    tid = counter._classifier_for("rfc1", "+").target_id
    made = counter.motif_models[tid]
    plain_model = counter._classifier_for("plain", "+").repeatHMM.model_id
    with pytest.raises(ffi.StriqueHipError) as e:
        ctx.target_set_motifs(tid, [made[0][1], plain_model], [0, made[1][2]], [0, 0])
    assert e.value.code == ffi.STRQ_ERR_UNSUPPORTED
    with pytest.raises(ffi.StriqueHipError) as e:
        ctx.target_set_motifs(10 ** 6, [m[1] for m in made], [max(m[2], 0) for m in made], [m[3] for m in made])
    assert e.value.code == ffi.STRQ_ERR_ARG
    # a scan with the switch on
    ids = [counter._classifier_for(t, st).target_id for t, st in counter.candidates()]
    sig = np.ascontiguousarray(pipeline[0][0][1])
    try:
        ctx.set_motifs(True, SEGMENT)
        ctx.batch_upload(sig, [0, len(sig)], [ids[0]])
        ctx.scan_set(ids, 5.0)
        with pytest.raises(ffi.StriqueHipError) as e:
            ctx.batch_run()
        assert e.value.code == ffi.STRQ_ERR_ARG and "scan" in str(e.value)
    finally:
        ctx.scan_clear(); ctx.set_motifs(False)
    # the refused call left the target as it was
    row_, rec_ = counter.motifs_batch([pipeline[0][0]], SEGMENT)[0]
    _same_record(rec_, pipeline[0][2], "after the refusals")


def test_the_counter_switch(counter, pipeline):
    """set_motifs: detect_batch keeps the records of its last call beside the rows it has always returned."""
    items = [it for it, _, _ in pipeline]
    plain = counter.detect_batch(items, units=True)
    assert counter.motif_records is None
    counter.set_motifs(True, SEGMENT)
    try:
        got = counter.detect_batch(items, units=True)
        recs = counter.motif_records
    finally:
        counter.set_motifs(False)
    assert len(recs) == len(items)
    for (row_, pos_), (row, pos), rec_, (_, _, rec), plan in zip(got, plain, recs, pipeline, PIPELINE_READS):
        assert row_ == row and (pos is None) == (pos_ is None) and (pos is None or np.array_equal(pos, pos_))
        _same_record(rec_, rec, plan)
    assert counter.ctx.last_motifs()["reads"] == sum(1 for _, _, rec in pipeline if rec is not None)
    counter.detect_batch(items[:2])
    assert counter.motif_records is None and counter.ctx.last_motifs()["launches"] == 0


def test_count_command_with_motifs(tmp_path, tables, cfg, pipeline):
    """`count ... --motif-units defs.tsv --motifs out.tsv` from written fast5 files: the count TSV is byte-identical to a run without
    the flags, the side file parses back to the reference's records."""
    import io
    import json
    from contextlib import redirect_stdout
    import h5write
    from strique_amd import cli, motifs
    prefix, suffix = _full_flanks(cfg)
    with open(tmp_path / "r9_4_450bps.model", "w") as fp:
        for k, mu, sd in zip(tables["base_kmer"], tables["base_mean"], tables["base_stdv"]):
            fp.write("%s\t%s\t%s\t1\n" % (k.decode() if isinstance(k, bytes) else str(k), repr(float(mu)), repr(float(sd))))
    loci = {"rfc1": ("chrA", 50000, 50100), "fgf14": ("chrB", 70000, 70100), "plain": ("chrC", 90000, 90100)}
    with open(tmp_path / "repeat_config.tsv", "w") as fp:
        fp.write("chr\tbegin\tend\tname\trepeat\tprefix\tsuffix\n")
        for name, (chrom, b, e) in loci.items():
            fp.write("\t".join([chrom, str(b), str(e), name, TARGETS[name][0] if name in TARGETS else cfg["repeat"]["c9orf72"][3], prefix, suffix]) + "\n")
    with open(tmp_path / "STRique.json", "w") as fp:
        json.dump({"align": cfg["align"], "HMM": cfg["HMM"]}, fp)
    with open(tmp_path / "defs.tsv", "w") as fp:
        fp.write("# loci whose array may be another unit\n\nrfc1\tAAAGG,AAGGG\nfgf14\tGAAGGA\n")
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
            "--config", str(tmp_path / "STRique.json"), "--algn", str(tmp_path / "aln.sam"), "--batch", "5"]
    cli.main(base + ["--out", str(tmp_path / "plain.tsv")])
    cli.main(base + ["--out", str(tmp_path / "with.tsv"), "--motif-units", str(tmp_path / "defs.tsv"), "--motifs", str(tmp_path / "motifs.tsv")])
    assert (tmp_path / "with.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    count_rows = (tmp_path / "plain.tsv").read_text().splitlines()[1:]
    with open(tmp_path / "motifs.tsv") as fp:
        rows = motifs.parse(fp)
    assert len(rows) == len(count_rows) == len(pipeline)
    for got, line, (rid, _), ((target, _, strand), row, rec) in zip(rows, count_rows, reads, pipeline):
        assert got[:3] == (rid, target, strand) and got[3] == row[0] == int(line.split("\t")[3])
        assert (got[4] is None) == (rec is None), rid
        if rec is not None:
            units = _units(target)
            n_seg, unit, shares, count_m, log_p_m, runs = got[4]
            assert n_seg == len(rec[5]) and unit == units[rec[0]] and shares == tuple(float("%.4f" % s) for s in rec[1]), (rid, got[4], rec[:5])
            assert count_m == rec[2] and log_p_m == rec[3] and runs == [(units[c], a, b) for c, a, b in rec[4]], (rid, got[4], rec[:5])
