"""All the optional passes behind the count decode in one run call (units, confidence, mod-llr, variants, anchored, anchored-mod,
tracts) against the runs with one switch on at a time: five reads in three sub-batches of at most two, so that both slots are used
twice and every pass of a sub-batch runs between the passes of its neighbours.  Every per-read output of the combined run has the
bits of the run where its switch was on alone, and every counter of strq_last_* (all entries but the milliseconds) is equal.
Renorm is not part of it: it changes the rows."""
import numpy as np
import pytest

import anchored_ref as ar
import tract_ref as tr

pytestmark = pytest.mark.gpu

ALT = "GGCCTG"
TRACTS = (("GGCCCC", ALT), ("",))
SWITCHES = ("units", "confidence", "mod_llr", "variants", "anchored", "anchored_mod", "tracts")
# the runs beside the combined one: every switch alone (anchored-mod hangs on the anchored records), and anchored-mod with the
# per-unit scores, whose pairs and launches it reports itself
ALONE = {"units": ("units",), "confidence": ("confidence",), "mod_llr": ("mod_llr",), "variants": ("variants",), "anchored": ("anchored",),
         "anchored_mod": ("anchored", "anchored_mod"), "tracts": ("tracts",), "anchored_mod_llr": ("anchored", "anchored_mod", "mod_llr")}


@pytest.fixture(scope="module")
def counter(pm, pm_mod, cfg):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9", *cfg["repeat"]["c9orf72"][3:6], alt_units=[ALT], tracts=TRACTS)
    yield rc
    rc.ctx.close()


@pytest.fixture(scope="module")
def items(pm, cfg):
    """Two spanning reads (a compound array on +, planted alt units on -), one read that ends in the repeat, one that starts in
    it, and one whose flanks stand in the wrong order (its gate fails); a spanning and an anchored read share a sub-batch."""
    from strique_amd import synth
    table = synth.KmerTable(pm)
    target = tuple(cfg["repeat"]["c9orf72"][3:6])
    repeat, prefix, suffix = target
    rng = np.random.Generator(np.random.PCG64(9100))
    span_plus = synth.make_signal(rng, table, synth.make_sequence(rng, 2600, prefix, tr.array_of(*TRACTS, (18, 7)), 1, suffix, "+"), True, 0.0)
    span_minus, _ = synth.make_variant_read(9101, table, target, 30, ALT, "-", flank_nt=1000, base_positions=(4, 11, 18, 24))
    ends, _, _ = ar.make_case(table, synth.make_signal, target, "+", ar.ENDS_CUTS[2], 9102)
    starts, _, _ = ar.make_case(table, synth.make_signal, target, "-", ar.STARTS_CUTS[0], 9103)
    swapped = synth.make_signal(rng, table, synth.make_sequence(rng, 2600, suffix, repeat, 20, prefix, "+"), True, 0.0)
    out = [("c9", span_plus, "+"), ("c9", ends, "+"), ("c9", span_minus, "-"), ("c9", starts, "-"), ("c9", swapped, "+")]
    assert all(sig.dtype == np.int16 and 2000 < len(sig) < 30000 for _, sig, _ in out)
    return out


def _bits(a):
    return None if a is None else (np.asarray(a).dtype.str, np.asarray(a).shape, np.ascontiguousarray(a).tobytes())


def _fields(rec):
    """A structured array field by field (the padding of a record is nobody's output)."""
    return [(name, rec[name].tobytes()) for name in rec.dtype.names if name != "pad_"]


def _counters(last):
    return {k: v for k, v in last.items() if k != "ms"}


def _run(counter, items, on):
    """One run call with the switches `on`: {output: per-read bytes} and {pass: strq_last_* without the milliseconds}."""
    ctx = counter.ctx
    counter.set_variants("variants" in on); counter.set_anchored_mod("anchored_mod" in on); counter.set_tracts("tracts" in on)
    try:
        ctx.set_option("STRQ_SUBBATCH_READS", "2")
        counter.detect_batch(items, units="units" in on, confidence="confidence" in on, mod_llr="mod_llr" in on,
                             anchored=ar.M if "anchored" in on else None, records=True)
    finally:
        ctx.set_option("STRQ_SUBBATCH_READS", None)
        counter.set_variants(False); counter.set_anchored_mod(False); counter.set_tracts(False)
    # (the switches are off again; what the last run call produced stays fetchable)
    out = {"rows": _fields(ctx.batch_fetch()), "mod": ctx.batch_fetch_mod()}
    if "units" in on:
        out["units"] = [_bits(u) for u in ctx.batch_fetch_units()]
    if "confidence" in on:
        out["confidence"] = [None if c is None else np.array(c).tobytes() for c in ctx.batch_fetch_confidence()]
    if "mod_llr" in on:
        out["mod_llr"] = [_bits(v) for v in ctx.batch_fetch_mod_llr()]
    if "variants" in on:
        out["variants"] = [None if v is None else (v[0],) + tuple(_bits(a) for a in v[1:]) for v in ctx.batch_fetch_variants()]
    if "anchored" in on:
        out["anchored"] = _fields(ctx.batch_fetch_anchored())
    if "anchored_mod" in on:
        out["anchored_mod"] = [None if p is None else (p[0], _bits(p[1])) for p in ctx.batch_fetch_anchored_mod()]
    if "tracts" in on:
        out["tracts"] = _fields(ctx.batch_fetch_tracts())
    last = {"units": ctx.last_units(), "confidence": ctx.last_confidence(), "mod_llr": ctx.last_mod_llr(), "variants": ctx.last_variants(),
            "anchored": ctx.last_anchored(), "anchored_mod": ctx.last_anchored_mod(), "tracts": ctx.last_tracts()}
    return out, {k: _counters(v) for k, v in last.items()}


@pytest.fixture(scope="module")
def runs(counter, items):
    out = {"all": _run(counter, items, SWITCHES)}
    for name, on in ALONE.items():
        out[name] = _run(counter, items, on)
    return out


def test_the_reads_exercise_every_pass(runs):
    """The combined run is no empty comparison: every pass had reads, over three sub-batches."""
    out, last = runs["all"]
    print("combined run:", last)
    rows = dict(out["rows"])
    count = np.frombuffer(rows["count"], np.int32)
    assert count[0] > 0 and count[2] > 0 and count[4] == 0          # the spanning reads are decoded, the swapped one is not
    assert out["units"][0] is not None and out["units"][2] is not None and out["units"][4] is None
    assert out["confidence"][0] is not None and out["confidence"][2] is not None
    assert out["mod"][0] != "-" and out["mod_llr"][0] is not None
    assert out["variants"][0] is not None and out["variants"][2] is not None and out["variants"][1] is None
    kind = np.frombuffer(dict(out["anchored"])["kind"], np.int32)
    assert [int(k) for k in kind[:4]] == [1, 2, 1, 3], kind
    assert out["anchored_mod"][1] is not None and out["anchored_mod"][3] is not None and out["anchored_mod"][0] is None
    assert out["anchored_mod"][1][1] is not None          # (with the per-unit scores on: pairs)
    status = np.frombuffer(dict(out["tracts"])["status"], np.int32)
    assert status[0] == 0 and status[2] == 0 and status[1] == 1 and status[4] == 1, status
    assert last["units"]["windows"] == 2 and last["confidence"]["windows"] == 2 and last["variants"]["reads"] == 2
    assert last["anchored"]["kinds"] == (1, 2, 1, 1) and last["anchored_mod"]["reads"] == 2 and last["tracts"]["windows"] == 2
    assert all(last[k]["launches"] > 0 for k in ("mod_llr", "variants", "anchored", "anchored_mod", "tracts"))


@pytest.mark.parametrize("name", sorted(ALONE))
def test_combined_run_equals_the_switch_alone(runs, name):
    both, both_last = runs["all"]
    alone, alone_last = runs[name]
    # rows and patterns do not depend on the switches
    assert alone["rows"] == both["rows"] and alone["mod"] == both["mod"]
    if name == "anchored_mod":
        # without the per-unit scores: the patterns alone; the pass's launches count the scoring launches of the combined run,
        # so its counters are compared in the run with exactly those three switches on
        assert [p and p[0] for p in alone["anchored_mod"]] == [p and p[0] for p in both["anchored_mod"]]
        assert all(p is None or p[1] is None for p in alone["anchored_mod"])
        assert {k: v for k, v in alone_last[name].items() if k != "launches"} == {k: v for k, v in both_last[name].items() if k != "launches"}
        return
    if name == "anchored_mod_llr":
        assert alone["anchored_mod"] == both["anchored_mod"] and alone["anchored"] == both["anchored"]
        assert alone_last["anchored_mod"] == both_last["anchored_mod"] and alone_last["anchored"] == both_last["anchored"]
        return
    assert alone[name] == both[name]
    assert alone_last[name] == both_last[name], (name, alone_last[name], both_last[name])
    # a pass that was off ran nothing
    for other in SWITCHES:
        if other not in ALONE[name]:
            assert not any(v if not isinstance(v, tuple) else any(v) for v in alone_last[other].values()), (name, other, alone_last[other])
