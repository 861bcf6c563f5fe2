"""strq_set_mod_llr on the GPU against tests/mod_llr_ref.py: every (V_base, V_mod) bit-equal to the oracle's Viterbi on the masked
dual model, rows and pattern strings exactly those of a run with the switch off."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import mod_llr_ref
from conftest import oracle_tc

pytestmark = pytest.mark.gpu

_CACHE = {}


def _ref(key, sig, tc, opm, params, opm_mod):
    """The reference of one read, computed once per session and never changed."""
    if key not in _CACHE:
        _CACHE[key] = mod_llr_ref.reference(sig, tc, opm, params, opm_mod)
    return _CACHE[key]


def _same_bits(got, want):
    got = np.ascontiguousarray(got, np.float64); want = np.ascontiguousarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def _counter(pm, pm_mod, cfg):
    from strique_amd.counter import repeatCounter
    return repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)


def _scores(rc, items):
    """(rows, [(n, 2) array or None]) of one batch with the switch on, through the context."""
    tcs = [rc._classifier_for(t, s) for t, _, s in items]
    rc.ctx.set_mod_llr(True)
    try:
        res = rc.ctx.detect_batch_reads([np.ascontiguousarray(r) for _, r, _ in items], [tc.target_id for tc in tcs])
        return res, rc.ctx.batch_fetch_mod(), rc.ctx.batch_fetch_mod_llr()
    finally:
        rc.ctx.set_mod_llr(False)


def _check_against_reference(rc, items, refs):
    # precondition, on the CPU: the flanked decode of every read marks one stretch whichever order its in-edges are listed in
    # (mod_llr_ref.stretch_is_unique) -- an exact tie there moves the start of the stretch, and with it the first unit
    for (name, _, strand), ref in zip(items, refs):
        assert mod_llr_ref.stretch_is_unique(ref, rc._classifier_for(name, strand).repeatHMM.baked), (name, strand)
    plain = rc.detect_batch(items)
    with_llr = rc.detect_batch(items, mod_llr=True)
    _, mods, vs = _scores(rc, items)
    for k, ref in enumerate(refs):
        assert tuple(plain[k]) == tuple(ref["row"]), (k, plain[k], ref["row"])
        assert tuple(with_llr[k][0]) == tuple(plain[k]) and mods[k] == ref["pattern"]
        n = 0 if ref["pattern"] == "-" else len(ref["pattern"])
        if n == 0:
            assert vs[k] is None and with_llr[k][1] is None
            continue
        assert vs[k].shape == (n, 2) and _same_bits(vs[k], ref["V"]), (k, vs[k], ref["V"])
        assert _same_bits(with_llr[k][1], ref["V"][:, 1] - ref["V"][:, 0])
    return vs


@pytest.fixture(scope="module")
def six(pm, pm_mod, cfg, orc, opm, opm_mod, targets):
    """Six reads on C9orf72: three from the base table and three from the mCpG one, both strands; [:3] int16, [3:] float64."""
    from strique_amd import synth
    params = orc.align_params(cfg["align"])
    plan = [(pm, "+", 3000, 5, True), (pm_mod, "-", 4500, 23, True), (pm_mod, "+", 6000, 60, True),
            (pm_mod, "-", 3500, 11, False), (pm, "-", 5000, 37, False), (pm, "+", 4000, 17, False)]
    items, refs = [], []
    for k, (table, strand, nt, nrep, as_int) in enumerate(plan):
        sig = synth.make_read(synth.KmerTable(table), 41, k, nt, targets["c9orf72"], nrep, strand=strand, as_int16=as_int)[0]
        items.append(("c9orf72", sig, strand))
        refs.append(_ref(("six", k), sig, oracle_tc(orc, opm, targets, "c9orf72", strand, cfg["HMM"], opm_mod), opm, params, opm_mod))
    return items, refs


@pytest.fixture(scope="module")
def mod_counter(pm, pm_mod, cfg, targets):
    rc = _counter(pm, pm_mod, cfg)
    rc.add_target("c9orf72", *targets["c9orf72"])
    yield rc
    rc.ctx.close()


def test_six_reads_bit_equal_the_reference(mod_counter, six):
    items, refs = six
    vs = []
    for part in (slice(0, 3), slice(3, 6)):          # an int16 batch and a float64 one
        vs += _check_against_reference(mod_counter, items[part], refs[part])
    llr = np.concatenate([v[:, 1] - v[:, 0] for v in vs])
    assert (llr > 0).any() and (llr < 0).any()
    for ref, v in zip(refs, vs):          # the branch the joint decode called is never the worse one (slack: see test_mod_llr_host)
        for ch, x in zip(ref["pattern"], v[:, 1] - v[:, 0]):
            assert x >= -1e-9 if ch == "1" else x <= 1e-9


def test_edges_one_unit_failed_gate_no_mod_model_missing_values(pm, pm_mod, cfg, orc, opm, opm_mod, targets):
    from strique_amd import synth
    from strique_amd.counter import repeatCounter
    params = orc.align_params(cfg["align"])
    rc = _counter(pm, pm_mod, cfg)
    rc.add_target("c9orf72", *targets["c9orf72"])
    tc = lambda strand: oracle_tc(orc, opm, targets, "c9orf72", strand, cfg["HMM"], opm_mod)
    table = synth.KmerTable(pm_mod)
    # the fewest repeats that still leave the dual model a unit
    one = synth.make_read(table, 43, 0, 3000, targets["c9orf72"], 2, strand="+")[0]
    ref_one = _ref(("edge", "one"), one, tc("+"), opm, params, opm_mod)
    assert len(ref_one["pattern"]) == 1 and ref_one["pattern"] != "-"
    # suffix in front of the prefix: the gate fails, pattern '-'
    repeat, prefix, suffix = targets["c9orf72"]
    rng = np.random.default_rng(9)
    back = "".join(rng.choice(list("ACGT"), 2400))
    swapped = synth.make_signal(rng, table, (back[:800] + suffix + back[800:1600] + prefix + back[1600:]).encode())
    ref_swapped = _ref(("edge", "swapped"), swapped, tc("+"), opm, params, opm_mod)
    assert ref_swapped["pattern"] == "-" and ref_swapped["row"][0] == 0
    # a read whose filtered signal normalises to NaNs (test_filtered_signal_without_tails_is_decoded_as_missing_values): the flanked
    # decode sees missing values, the dual model the finite raw normalisation of the stretch it marks
    s = synth.make_read(synth.KmerTable(pm), 9, 4242, 6000, targets["c9orf72"], 20, strand="+")[0].copy()
    floor, ceil_ = int(s.min()) - 40, int(s.max()) + 40
    rng = np.random.default_rng(5)
    for pos in rng.choice(np.arange(10, len(s) - 10, 12), size=len(s) // 100, replace=False):
        s[pos:pos + 3] = floor
    for pos in rng.choice(np.arange(16, len(s) - 10, 12), size=len(s) // 100, replace=False):
        s[pos:pos + 3] = ceil_
    assert np.isnan(orc.condition(s, opm)[3]).all()
    ref_nan = _ref(("edge", "nan"), s, tc("+"), opm, params, opm_mod)
    assert ref_nan["pattern"] != "-" and len(ref_nan["V"]) == len(ref_nan["pattern"]) >= 1
    items = [("c9orf72", one, "+"), ("c9orf72", swapped, "+"), ("c9orf72", s, "+")]
    _check_against_reference(rc, items, [ref_one, ref_swapped, ref_nan])
    # a target without a modification model in the same batch (a second counter on the same context, no mod model)
    plain = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], context=rc.ctx)
    plain.add_target("fmr1", *targets["fmr1"])
    fm = synth.make_read(synth.KmerTable(pm), 43, 7, 3500, targets["fmr1"], 20, strand="-")[0]
    ids = [rc._classifier_for("c9orf72", "+").target_id, plain._classifier_for("fmr1", "-").target_id, rc._classifier_for("c9orf72", "+").target_id]
    rc.ctx.set_mod_llr(True)
    res = rc.ctx.detect_batch_reads([one, fm, s], ids)
    mods, vs = rc.ctx.batch_fetch_mod(), rc.ctx.batch_fetch_mod_llr()
    rc.ctx.set_mod_llr(False)
    assert int(res[1]["count"]) > 0 and mods[1] == "-" and vs[1] is None
    assert _same_bits(vs[0], ref_one["V"]) and _same_bits(vs[2], ref_nan["V"])
    rc.ctx.close()


def _unit_target(length, seed):
    rng = np.random.default_rng(seed)
    unit = "".join(rng.choice(list("ACGT"), length))
    unit = unit[:1] + "CG" + unit[3:] if length >= 3 else unit
    return unit, "".join(rng.choice(list("ACGT"), 150)), "".join(rng.choice(list("ACGT"), 150))


@pytest.mark.parametrize("length", [3, 7, 15, 16, 31])
def test_lane_count_edges(pm, pm_mod, cfg, orc, opm, opm_mod, length):
    """Dual models of 4 L + 2 emitting states: 14 and 30 (two units per wave), 62 (one state per lane), 66 (just over: two states per
    lane), 126 (the largest covered).  (Read indices: the first ones whose flanked decode has no tie at the entry of the repeat
    section, see _check_against_reference; the 7-nt unit shares a k-mer with its prefix and ties on two reads in three.)"""
    from strique_amd import hmm, synth
    target = _unit_target(length, 100 + length)
    assert hmm.RepeatModModel(target[0], pm, pm_mod, cfg["HMM"]).baked.silent_start == 4 * length + 2
    rc = _counter(pm, pm_mod, cfg)
    rc.add_target("t", *target)
    params = orc.align_params(cfg["align"])
    items, refs = [], []
    for k, (table, strand) in enumerate(((pm_mod, "+"), (pm, "-"))):
        nrep = max(8, 120 // length) + 3 * k
        idx = 10 * length + k + (2 if (length, k) == (7, 1) else 0)
        sig = synth.make_read(synth.KmerTable(table), 47, idx, 3000 + nrep * length, target, nrep, strand=strand)[0]
        items.append(("t", sig, strand))
        refs.append(_ref(("lanes", length, k), sig, orc.classifier(*target, strand, opm, opm_mod, cfg["HMM"]), opm, params, opm_mod))
        assert 3 <= len(refs[-1]["pattern"]) <= 60 and refs[-1]["pattern"] != "-"
    _check_against_reference(rc, items, refs)
    rc.ctx.close()


def test_a_32_nt_unit_is_refused_with_a_message(pm, pm_mod, cfg):
    from strique_amd.ffi import StriqueHipError, STRQ_ERR_UNSUPPORTED
    big, small = _unit_target(32, 132), _unit_target(7, 107)
    # the switch goes on after the target
    rc = _counter(pm, pm_mod, cfg)
    rc.add_target("small", *small)
    rc.ctx.set_mod_llr(True); rc.ctx.set_mod_llr(False)
    rc.add_target("big", *big)
    with pytest.raises(StriqueHipError) as ei:
        rc.ctx.set_mod_llr(True)
    assert ei.value.code == STRQ_ERR_UNSUPPORTED and "at most 128 emitting states" in str(ei.value) and "130" in str(ei.value)
    assert rc.ctx.last_mod_llr()["launches"] == 0
    rc.ctx.close()
    # the target comes with the switch on
    rc = _counter(pm, pm_mod, cfg)
    rc.add_target("small", *small)
    rc.ctx.set_mod_llr(True)
    with pytest.raises(StriqueHipError) as ei:
        rc.add_target("big", *big)
    assert ei.value.code == STRQ_ERR_UNSUPPORTED and "at most 128 emitting states" in str(ei.value)
    rc.ctx.close()


def test_routes_and_scheduling_give_the_same_bytes(pm, pm_mod, cfg, targets, six):
    items, refs = six
    items = items[:3] + items[:3][::-1]
    want = refs[:3] + refs[:3][::-1]

    def run(options, **kw):
        rc = _counter(pm, pm_mod, cfg)
        rc.add_target("c9orf72", *targets["c9orf72"])
        for k, v in options.items():
            rc.ctx.set_option(k, v)
        got = rc.detect_batch(items, **kw)
        rc.ctx.close()
        return got

    base = run({}, mod_llr=True)
    for g, ref in zip(base, want):
        assert tuple(g[0]) == tuple(ref["row"]) and _same_bits(g[1], ref["V"][:, 1] - ref["V"][:, 0])
    same = lambda a, b: len(a) == len(b) and all(tuple(x[0]) == tuple(y[0]) and _same_bits(x[-1], y[-1]) for x, y in zip(a, b))
    assert same(base, run({}, mod_llr=True))                                     # two runs
    assert same(base, run({"STRQ_MOD_BACKPOINTERS": "1"}, mod_llr=True))         # bounds from the traced path
    assert same(base, run({"STRQ_SERIAL": "1"}, mod_llr=True))
    assert same(base, run({"STRQ_SUBBATCH_READS": "2"}, mod_llr=True))
    # with unit positions and confidence: every element equals the one of a run that asks for it alone
    allthree = run({}, units=True, confidence=True, mod_llr=True)
    units, conf = run({}, units=True), run({}, confidence=True)
    for a, u, c, b in zip(allthree, units, conf, base):
        assert len(a) == 4 and tuple(a[0]) == tuple(u[0]) == tuple(c[0]) == tuple(b[0])
        assert np.array_equal(a[1], u[1]) and a[2] == c[1] and _same_bits(a[3], b[1])


def test_all_outputs_share_one_read_back_and_one_grouping(pm, pm_mod, cfg, targets):
    """Units, confidence and mod_llr together, in sub-batches of 3 (two in flight, the last one harvested by the fetch) and serially:
    every element equals, bit for bit, the one of a run that asks for that output alone in one sub-batch.  The batch is the smallest
    at which the decoded windows the passes share and the launch grouping can go wrong: two targets in different Viterbi kernel
    shapes, interleaved (the task position of a read is not its index), and a read in the middle that fails the gate (the decoded
    list skips a position).  C9orf72 decodes on the register-resident kernel, as every bundled target does; the 12-nt unit of
    test_gpu_units.py has no such layout and takes a lane-layout shape."""
    from strique_amd import synth
    from strique_amd.ffi import StriqueHipError
    from test_gpu_units import CUSTOM
    both = {"c9orf72": targets["c9orf72"], "units_dodeca": CUSTOM["units_dodeca"]}
    rc = _counter(pm, pm_mod, cfg)
    for name, target in both.items():
        rc.add_target(name, *target)
    plan = [("c9orf72", "+", 3000, 9), ("units_dodeca", "-", 4500, 14), ("c9orf72", "-", 5200, 31), None,
            ("units_dodeca", "+", 6000, 22), ("c9orf72", "+", 3600, 17), ("units_dodeca", "-", 3300, 6)]
    items = []
    for k, p in enumerate(plan):
        if p is None:          # pure noise: no flank, the gate fails
            items.append(("c9orf72", np.random.default_rng(3).integers(200, 800, 4000).astype(np.int16), "-"))
            continue
        name, strand, nt, nrep = p
        table = synth.KmerTable(pm_mod if k % 2 else pm)
        items.append((name, synth.make_read(table, 53, k, nt, both[name], nrep, strand=strand, as_int16=True)[0], strand))
    bad = plan.index(None)

    def run(options, **kw):
        for k, v in options.items():
            rc.ctx.set_option(k, v)
        try:
            return rc.detect_batch(items, **kw)
        finally:
            for k in options:
                rc.ctx.set_option(k, "")

    units = run({}, units=True)
    assert rc.ctx.last_viterbi_launches()["launches"] == 2          # one sub-batch, two kernel shapes
    conf, llr = run({}, confidence=True), run({}, mod_llr=True)
    rows = [u[0] for u in units]
    assert rows[bad][0] == 0 and units[bad][1] is None and conf[bad][1] is None and llr[bad][1] is None
    assert sum(u[1] is not None and len(u[1]) > 0 for u in units) == len(items) - 1
    assert all(c[1] is not None for k, c in enumerate(conf) if k != bad) and sum(v[1] is not None for v in llr) >= len(items) - 2
    for options in ({"STRQ_SUBBATCH_READS": "3"}, {"STRQ_SERIAL": "1"}):
        got = run(options, units=True, confidence=True, mod_llr=True)
        assert len(got) == len(items)
        for k, (a, u, c, v) in enumerate(zip(got, units, conf, llr)):
            assert len(a) == 4 and tuple(a[0]) == tuple(u[0]) == tuple(c[0]) == tuple(v[0]), (options, k)
            for x, y in ((a[1], u[1]), (a[2], c[1]), (a[3], v[1])):
                assert (x is None) == (y is None), (options, k)
                assert x is None or _same_bits(x, y), (options, k, x, y)
        assert got[bad][1:] == (None, None, None)
    # the switches are off again: a plain run gives the plain rows, and its batch holds no unit positions
    assert run({}) == rows
    with pytest.raises(StriqueHipError, match="ran without unit positions"):
        rc.ctx.batch_fetch_units()
    rc.ctx.close()


def test_switch_off_launches_nothing_and_returns_no_units(mod_counter, six):
    items, refs = six
    ctx = mod_counter.ctx
    plain = mod_counter.detect_batch(items[:3])
    assert all(v is None for v in ctx.batch_fetch_mod_llr())
    assert ctx.last_mod_llr() == {"ms": 0.0, "units": 0, "reads": 0, "launches": 0}
    _, mods, vs = _scores(mod_counter, items[:3])
    st = ctx.last_mod_llr()
    assert st["launches"] == 2 and st["reads"] == 3 and st["units"] == sum(len(m) for m in mods) == sum(len(v) for v in vs)
    assert [p[6] for p in plain] == mods
    again = mod_counter.detect_batch(items[:3])          # off again: the scores of the earlier run are gone
    assert again == plain and all(v is None for v in ctx.batch_fetch_mod_llr()) and ctx.last_mod_llr()["launches"] == 0


def test_count_mod_llr_end_to_end(tmp_path, tables, pm, pm_mod, cfg, six):
    """`count --mod_model M --mod-llr FILE` on two fast5 reads: the file is written, the count TSV is byte-equal to a run without."""
    import h5write
    from strique_amd import cli
    items, refs = six
    for key, name in (("base", "base.model"), ("mod", "mod.model")):
        with open(tmp_path / name, "w") as fp:
            for k, m, s in zip(tables[key + "_kmer"], tables[key + "_mean"], tables[key + "_stdv"]):
                fp.write("%s\t%s\t%s\t1\n" % (k.decode() if isinstance(k, bytes) else str(k), repr(float(m)), repr(float(s))))
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    (tmp_path / "repeats.tsv").write_text("chr\tbegin\tend\tname\trepeat\tprefix\tsuffix\n" + "\t".join([chrom, str(b), str(e), "c9orf72", repeat, prefix, suffix]) + "\n")
    (tmp_path / "STRique.json").write_text(json.dumps({"align": cfg["align"], "HMM": cfg["HMM"]}))
    reads, sam = [], ["@HD\tVN:1.0"]
    for i in (0, 1):
        rid = "%08d-0000-4000-8000-%012d" % (i, i)
        reads.append((rid, items[i][1]))
        sam.append("\t".join([rid, "16" if items[i][2] == "-" else "0", chrom, str(b - 3000), "60", "12S6000M5S", "*", "0", "0", "ACGT", "*"]))
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
    cli.main(argv + ["--out", str(tmp_path / "with.tsv"), "--mod-llr", str(tmp_path / "llr.tsv")])
    assert (tmp_path / "with.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    rows = cli.parse_mod_llr(open(tmp_path / "llr.tsv"))
    assert open(tmp_path / "llr.tsv").readline().rstrip("\n").split("\t") == cli.MODLLR_HEADER
    assert len(rows) == 2
    for row, ref, (rid, _) in zip(rows, refs, reads):
        assert row[:5] == (rid, "c9orf72", "+" if ref is refs[0] else "-", ref["row"][0], ref["pattern"])
        assert row[5] == [float("%.4f" % x) for x in ref["V"][:, 1] - ref["V"][:, 0]]
