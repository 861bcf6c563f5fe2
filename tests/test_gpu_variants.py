"""strq_set_variants on the GPU against tests/variant_ref.py: passages, branches, raw samples, count_v and every score V_b bit-equal
to the CPU oracle's decode of the un-baked variant net and its Viterbi on the masked copies; rows and every other output exactly
those of a run with the switch off."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest

import mod_llr_ref
import variant_ref

pytestmark = pytest.mark.gpu

# three models: 26 emitting states (two passages per wave), 62 (one state per lane), 86 (two states per lane)
MODELS = {
    "fmr1_1": ("fmr1", ["AGG"]),
    "fmr1_3": ("fmr1", ["AGG", "CAG", "CGA"]),
    "c9_3": ("c9orf72", ["GGCCTC", "GGACCC", "AGCCCC"]),
}
SEED_BASE = 5000          # reads of a model: seeds SEED_BASE + 100 * (its position in MODELS) + candidate index
DODECA = ("ACGTTGCAAGTC", ["ACGTTGCAAGTA", "ACGTTGCATGTC", "TCGTTGCAAGTC"])          # 12-nt unit, three alts: 2 + 24 + 2 * 3 * 2 * 12 = 170 states

_CACHE = {}


def _same_bits(got, want):
    got = np.ascontiguousarray(got, np.float64); want = np.ascontiguousarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def _read(pm, targets, model, k, n_units=None):
    """Candidate read k of a model: ~20 k samples, 30 to 60 units, four of them one of the model's alt units; strands alternate."""
    from strique_amd import synth
    locus, alts = MODELS[model]
    strand = "+-"[k % 2]
    n = n_units or 30 + (7 * k + 11 * list(MODELS).index(model)) % 31
    base = tuple(int(x) for x in np.linspace(3, n - 8, 4))
    seed = SEED_BASE + 100 * list(MODELS).index(model) + k
    sig, planted = synth.make_variant_read(seed, synth.KmerTable(pm), targets[locus], n, alts[k % len(alts)], strand, flank_nt=1200, base_positions=base)
    return sig, strand, planted


def _oracle(orc, opm, cfg, targets, model, strand):
    key = ("tc", model, strand)
    if key not in _CACHE:
        locus, alts = MODELS[model]
        _CACHE[key] = (orc.classifier(*targets[locus], strand, opm, None, cfg["HMM"]),
                       variant_ref.VariantModel(targets[locus][0], alts, strand, opm, cfg["HMM"]))
    return _CACHE[key]


def _ref(key, sig, orc, opm, cfg, targets, model, strand):
    """The reference of one read, computed once per session and never changed."""
    if key not in _CACHE:
        tc, vm = _oracle(orc, opm, cfg, targets, model, strand)
        _CACHE[key] = variant_ref.reference(sig, tc, opm, orc.align_params(cfg["align"]), vm)
    return _CACHE[key]


def _counter(pm, cfg, targets, models=MODELS, pm_mod=None, context=None):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0, context=context)
    for name, (locus, alts) in models.items():
        rc.add_target(name, *targets[locus], alt_units=alts)
    return rc


def _with_variants(rc, items, **kw):
    """detect_batch with the counter's variant switch on for this call."""
    rc.set_variants(True)
    try:
        return rc.detect_batch(items, **kw)
    finally:
        rc.set_variants(False)


@pytest.fixture(scope="module")
def reads(pm, cfg, orc, opm, targets, counter):
    """Per model the first six candidate reads whose repeat stretch is unique on the CPU (mod_llr_ref.stretch_is_unique: the reason is
    in the README under mod-llr), with their references; at least four of the first six candidates qualify."""
    out = {}
    for model in MODELS:
        flanked = {strand: counter._classifier_for(model, strand).repeatHMM.baked for strand in "+-"}
        items, refs, ok = [], [], []
        for k in range(10):
            sig, strand, planted = _read(pm, targets, model, k)
            ref = _ref(("read", model, k), sig, orc, opm, cfg, targets, model, strand)
            unique = ref["decoded"] and mod_llr_ref.stretch_is_unique(ref, flanked[strand])
            if k < 6:
                ok.append(unique)
            if unique and len(items) < 6:
                items.append((model, sig, strand)); refs.append(ref)
            if k >= 5 and len(items) == 6:
                break
        assert sum(ok) >= 4 and len(items) == 6, (model, ok)
        out[model] = (items, refs)
    return out


@pytest.fixture(scope="module")
def counter(pm, cfg, targets):
    rc = _counter(pm, cfg, targets)
    yield rc
    rc.ctx.close()


def _check(got, ref):
    """The variants element of a detect_batch result against its reference."""
    if not ref["decoded"]:
        assert got is None
        return
    count_v, pattern, branch, end, V = got
    assert count_v == ref["count_v"] and pattern == ref["pattern"]
    assert branch.dtype == np.int8 and np.array_equal(branch, ref["branch"])
    assert end.dtype == np.int64 and np.array_equal(end, ref["end"])
    assert V.dtype == np.float64 and _same_bits(V, ref["V"]), (V, ref["V"])
    # the branch the joint decode called is never worse than the repeat unit's (slack: two sums of the same terms in another order)
    for j, b in enumerate(branch):
        assert V[j, b] - V[j, 0] >= -1e-9


@pytest.mark.parametrize("model", list(MODELS))
def test_six_reads_bit_equal_the_reference(counter, reads, model):
    items, refs = reads[model]
    assert {s for _, _, s in items} == {"+", "-"}
    plain = counter.detect_batch(items)
    got = _with_variants(counter, items)
    n_alt = 0
    for g, p, ref in zip(got, plain, refs):
        assert tuple(g[0]) == tuple(p) == tuple(ref["row"])
        _check(g[1], ref)
        assert g[1][4].shape == (len(ref["branch"]), 1 + len(MODELS[model][1]))
        n_alt += int((g[1][2] > 0).sum())
    assert n_alt >= 6          # the planted units are there to be found
    st = counter.ctx.last_variants()
    assert st["reads"] == 6 and st["passages"] == sum(len(r["branch"]) for r in refs) and st["launches"] == 3 and st["ms"] > 0          # count pass, write pass, one scoring launch


def test_three_models_in_one_batch(counter, reads):
    items = [reads[m][0][k] for k in (0, 1) for m in MODELS]
    refs = [reads[m][1][k] for k in (0, 1) for m in MODELS]
    for g, ref in zip(_with_variants(counter, items), refs):
        _check(g[1], ref)
    assert counter.ctx.last_variants()["launches"] == 2 + 3          # the two bounds passes, one scoring launch per (states per lane, branches)


def test_edges_one_passage_failed_gate_target_without_model(pm, cfg, orc, opm, targets):
    from strique_amd import synth
    rc = _counter(pm, cfg, targets, {"c9_3": MODELS["c9_3"]})
    rc.add_target("plain_fmr1", *targets["fmr1"])          # no alt units: no variant model
    # the fewest units that still leave the variant model a passage
    one = synth.make_variant_read(7, synth.KmerTable(pm), targets["c9orf72"], 2, "GGCCTC", "+", flank_nt=1200, base_positions=())[0]
    ref_one = _ref(("edge", "one"), one, orc, opm, cfg, targets, "c9_3", "+")
    assert ref_one["decoded"] and len(ref_one["branch"]) == 1
    # suffix in front of the prefix: the gate fails
    repeat, prefix, suffix = targets["c9orf72"]
    rng = np.random.default_rng(9)
    back = "".join(rng.choice(list("ACGT"), 2400))
    swapped = synth.make_signal(rng, synth.KmerTable(pm), (back[:800] + suffix + back[800:1600] + prefix + back[1600:]).encode())
    ref_swapped = _ref(("edge", "swapped"), swapped, orc, opm, cfg, targets, "c9_3", "+")
    assert not ref_swapped["decoded"] and ref_swapped["row"][0] == 0
    fm = synth.make_read(synth.KmerTable(pm), 43, 7, 3500, targets["fmr1"], 20, strand="-")[0]
    items = [("c9_3", one, "+"), ("plain_fmr1", fm, "-"), ("c9_3", swapped, "+"), ("c9_3", one, "+")]
    got = _with_variants(rc, items)
    assert got[1][0][0] > 0 and got[1][1] is None and got[2][1] is None and tuple(got[2][0]) == tuple(ref_swapped["row"])
    for k in (0, 3):
        assert tuple(got[k][0]) == tuple(ref_one["row"])
        _check(got[k][1], ref_one)
    assert rc.ctx.last_variants()["reads"] == 2
    # a counter without alt units has nothing to ask for
    from strique_amd.counter import repeatCounter
    bare = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], context=rc.ctx)
    bare.add_target("x", *targets["fmr1"])
    with pytest.raises(ValueError, match="alt_units"):
        bare.set_variants(True)
    rc.ctx.close()


def test_modification_model_and_variant_model_side_by_side(pm, pm_mod, cfg, targets, reads):
    """A target with both dual models: pattern and mod-llr bytes are those of a run without variants, the variants those of a counter
    without a modification model."""
    items = [("c9_3", sig, strand) for _, sig, strand in reads["c9_3"][0][:3]]
    refs = reads["c9_3"][1][:3]
    rc = _counter(pm, cfg, targets, {"c9_3": MODELS["c9_3"]}, pm_mod=pm_mod)
    without = rc.detect_batch(items, mod_llr=True)
    both = _with_variants(rc, items, mod_llr=True)
    for w, b, ref in zip(without, both, refs):
        assert tuple(w[0]) == tuple(b[0]) and w[0][6] != "-" and tuple(w[0][:6]) == tuple(ref["row"][:6])
        assert _same_bits(w[1], b[1])
        _check(b[2], ref)
    assert rc.ctx.last_mod_llr()["launches"] == 2 and rc.ctx.last_variants()["launches"] == 3
    rc.ctx.close()


def test_a_model_above_128_states_is_refused_with_a_message(pm, cfg, targets, reads):
    from strique_amd import hmm
    from strique_amd.ffi import StriqueHipError, STRQ_ERR_UNSUPPORTED
    rng = np.random.default_rng(12)
    flank = lambda: "".join(rng.choice(list("ACGT"), 150))
    assert hmm.RepeatVariantModel(DODECA[0], DODECA[1], pm, cfg["HMM"]).baked.silent_start == 170
    rc = _counter(pm, cfg, targets, {"fmr1_1": MODELS["fmr1_1"]})
    items, refs = reads["fmr1_1"]
    rc.add_target("dodeca", DODECA[0], flank(), flank(), alt_units=DODECA[1])
    with pytest.raises(StriqueHipError) as ei:
        _with_variants(rc, items[:1])
    assert ei.value.code == STRQ_ERR_UNSUPPORTED and "at most 128 emitting states" in str(ei.value) and "170" in str(ei.value)
    assert rc.ctx.last_variants()["launches"] == 0
    # the target was left alone (no variant model), the switch is off again, and the other target's model is registered
    assert tuple(rc.detect_batch(items[:1])[0]) == tuple(refs[0]["row"])
    tid = rc._classifier_for("dodeca", "+").target_id
    assert tid not in rc.variant_models and rc._classifier_for("fmr1_1", "+").target_id in rc.variant_models
    # the refusal is said once: the counter goes on with the targets that have a model, the refused one reports None
    assert "170" in rc.variant_refused[tid]
    again = _with_variants(rc, items[:1])
    _check(again[0][1], refs[0])
    # a model whose tags describe fewer alt branches than the call says is refused too, and the target keeps what it had
    ftid = rc._classifier_for("fmr1_1", items[0][2]).target_id
    fm = rc.variant_models[ftid]
    with pytest.raises(StriqueHipError) as ei:
        rc.ctx.target_set_variants(ftid, fm.model_id, fm.model_min, fm.model_max, 2, fm.context_units)
    assert ei.value.code == STRQ_ERR_UNSUPPORTED and "fewer than 2 alt branches" in str(ei.value)
    rc.ctx.set_variants(True)
    try:
        rc.ctx.detect_batch_reads([np.ascontiguousarray(items[0][1])], [rc._classifier_for("fmr1_1", items[0][2]).target_id])
        got = rc.ctx.batch_fetch_variants()[0]
    finally:
        rc.ctx.set_variants(False)
    assert got[0] == refs[0]["count_v"] and np.array_equal(got[1], refs[0]["branch"]) and _same_bits(got[3], refs[0]["V"])
    rc.ctx.close()


def test_routes_and_scheduling_give_the_same_bytes(pm, cfg, targets, reads):
    items = [reads[m][0][k] for m in MODELS for k in (0, 1)] + [reads["fmr1_1"][0][2]]
    want = [reads[m][1][k] for m in MODELS for k in (0, 1)] + [reads["fmr1_1"][1][2]]

    def run(options):
        rc = _counter(pm, cfg, targets)
        for k, v in options.items():
            rc.ctx.set_option(k, v)
        got = _with_variants(rc, items)
        launches = rc.ctx.last_variants()["launches"]
        rc.ctx.close()
        return got, launches

    for options in ({}, {"STRQ_MOD_BACKPOINTERS": "1"}, {"STRQ_SERIAL": "1"}, {"STRQ_SUBBATCH_READS": "2"}, {"STRQ_VIT_NO_G2": "1"}):
        got, launches = run(options)
        for g, ref in zip(got, want):
            assert tuple(g[0]) == tuple(ref["row"]), options
            _check(g[1], ref)
        # which route ran: the hub records need two bounds launches, the traced paths a traceback launch in front of them (one
        # sub-batch, three scoring launches) -- all three models are on the HUB shapes by default
        if "STRQ_SUBBATCH_READS" not in options:
            assert launches == (3 if "STRQ_MOD_BACKPOINTERS" in options else 2) + 3, (options, launches)


def test_switch_off_launches_nothing_and_rows_are_the_same(counter, reads):
    from strique_amd.ffi import StriqueHipError
    items, refs = reads["fmr1_3"]
    ctx = counter.ctx
    ids = [counter._classifier_for(t, s).target_id for t, _, s in items]
    sigs = [np.ascontiguousarray(r) for _, r, _ in items]
    off = ctx.detect_batch_reads(sigs, ids).copy()
    assert ctx.last_variants() == {"launches": 0, "passages": 0, "ms": 0.0, "reads": 0}
    with pytest.raises(StriqueHipError, match="ran without variants"):
        ctx.batch_fetch_variants()
    ctx.set_variants(True)
    on = ctx.detect_batch_reads(sigs, ids).copy()
    ctx.set_variants(False)
    assert ctx.last_variants()["launches"] == 3
    assert on.tobytes() == off.tobytes()
    again = ctx.detect_batch_reads(sigs, ids).copy()
    assert again.tobytes() == off.tobytes() and ctx.last_variants()["launches"] == 0


def test_count_variants_end_to_end(tmp_path, tables, pm, cfg, reads):
    """`count --alt-units FILE --variants OUT` on two fast5 reads: the file is written, the count TSV is byte-equal to a run without."""
    import h5write
    from strique_amd import cli
    items, refs = reads["fmr1_3"]
    with open(tmp_path / "base.model", "w") as fp:
        for k, m, s in zip(tables["base_kmer"], tables["base_mean"], tables["base_stdv"]):
            fp.write("%s\t%s\t%s\t1\n" % (k.decode() if isinstance(k, bytes) else str(k), repr(float(m)), repr(float(s))))
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["fmr1"]
    (tmp_path / "repeats.tsv").write_text("chr\tbegin\tend\tname\trepeat\tprefix\tsuffix\n" + "\t".join([chrom, str(b), str(e), "fmr1", repeat, prefix, suffix]) + "\n")
    (tmp_path / "alts.tsv").write_text("# interruptions\n\nfmr1\t" + ",".join(MODELS["fmr1_3"][1]).lower() + "\n")
    (tmp_path / "STRique.json").write_text(json.dumps({"align": cfg["align"], "HMM": cfg["HMM"]}))
    rd, sam = [], ["@HD\tVN:1.0"]
    for i in (0, 1):
        rid = "%08d-0000-4000-8000-%012d" % (i, i)
        rd.append((rid, items[i][1]))
        sam.append("\t".join([rid, "16" if items[i][2] == "-" else "0", chrom, str(b - 1500), "60", "12S3000M5S", "*", "0", "0", "ACGT", "*"]))
    data = tmp_path / "data"; data.mkdir()
    (data / "batch_0.fast5").write_bytes(h5write.multi_read_fast5(rd))
    buf = io.StringIO()
    with redirect_stdout(buf):
        cli.main(["index", str(data)])
    (data / "reads.fofn").write_text(buf.getvalue())
    (tmp_path / "aln.sam").write_text("\n".join(sam) + "\n")
    argv = ["count", str(data / "reads.fofn"), str(tmp_path / "base.model"), str(tmp_path / "repeats.tsv"), "--config", str(tmp_path / "STRique.json"),
            "--algn", str(tmp_path / "aln.sam")]
    cli.main(argv + ["--out", str(tmp_path / "plain.tsv")])
    cli.main(argv + ["--out", str(tmp_path / "with.tsv"), "--alt-units", str(tmp_path / "alts.tsv"), "--variants", str(tmp_path / "var.tsv")])
    assert (tmp_path / "with.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    assert open(tmp_path / "var.tsv").readline().rstrip("\n").split("\t") == cli.VARIANTS_HEADER
    rows = cli.parse_variants(open(tmp_path / "var.tsv"))
    assert len(rows) == 2
    for row, ref, (rid, _), item in zip(rows, refs, rd, items):
        assert row[:7] == (rid, "fmr1", item[2], ref["row"][0], ref["count_v"], len(ref["branch"]), ref["pattern"])
        want = [(i, MODELS["fmr1_3"][1][b - 1]) for i, b in variant_ref.calls(ref)]
        assert [(c[0], c[1]) for c in row[7]] == want and len(want) >= 1
        alt = [j for j, bb in enumerate(ref["branch"]) if bb]
        assert [c[2] for c in row[7]] == [int(ref["end"][j]) for j in alt]
        assert [c[3] for c in row[7]] == [float("%.4f" % (ref["V"][j, 1:].max() - ref["V"][j, 0])) for j in alt]
