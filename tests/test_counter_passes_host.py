"""The optional passes of repeatCounter without a GPU: a recording stand-in context logs every switch, run and fetch call and hands
out canned records, so that the switch sequence, the legacy tuple, the Detected records, the mixed batch and the ValueErrors of
detect_batch / scan_batch / set_* are pinned by literal values."""
import re

import numpy as np
import pytest

from strique_amd import ffi
from strique_amd.counter import Detected, repeatCounter

# the order the switches go on in
PASSES = ("anchored", "anchored_mod", "units", "confidence", "mod_llr", "variants", "renorm", "tracts", "flank_mod")
KEYWORDS = ("units", "confidence", "mod_llr")


def _struct(dtype, **fields):
    rec = np.zeros((), dtype)
    for k, v in fields.items():
        rec[k] = v
    return rec[()]


# what a fetch hands out for a read nobody canned a record for
DEFAULTS = {"mod": "-", "units": None, "confidence": None, "mod_llr": None, "variants": None, "anchored_mod": None, "flank_mod": None,
            "anchored": _struct(ffi.ANCHORED_DTYPE), "renorm": _struct(ffi.RENORM_DTYPE), "tracts": _struct(ffi.TRACTS_DTYPE, status=1)}


class RecordingContext(object):
    """Stands in for ffi.Context: ids from model_create / target_add, zero rows (count = the read's length, so that a row names its
    read) from the run calls, canned records ({fetch name: {read length: record}}) from the fetches, every call of interest in `log`."""
    last_positions_rc = 0
    last_positions_error = ""

    def __init__(self):
        self.log = []
        self.canned = {}
        self.fail = None
        self.ids = 0
        self.lengths = []

    def _id(self, *a, **kw):
        self.ids += 1
        return self.ids

    model_create = target_add = _id

    def __getattr__(self, name):
        if name.startswith(("set_align_params", "set_pore_stats", "target_set_", "model_set_")):
            return lambda *a, **kw: None
        raise AttributeError(name)

    def _rows(self, arrs):
        self.lengths = [len(a) for a in arrs]
        out = np.zeros(len(arrs), ffi.RESULT_DTYPE)
        out["count"] = self.lengths
        out["log_p"] = -1.5
        return out

    def detect_batch_reads(self, arrs, tids):
        self.log.append(("detect_batch_reads", str(arrs[0].dtype), tuple(int(t) for t in tids)))
        if self.fail == "detect_batch_reads":
            raise RuntimeError("the run failed")
        return self._rows(arrs)

    def scan_batch_reads(self, arrs, cand_ids, min_score, scores=False):
        self.log.append(("scan_batch_reads", tuple(int(c) for c in cand_ids), min_score))
        return self._rows(arrs), np.zeros(len(arrs), np.int32), np.zeros((len(arrs), len(cand_ids), 2))


def _switch(name):
    def switch(self, on, level=None):
        self.log.append((name, True) + (() if level is None else (level,)) if on else (name, False))
        if on and self.fail == name:
            raise ffi.StriqueHipError(ffi.STRQ_ERR_UNSUPPORTED, "refused")
    return switch


def _fetch(name):
    def fetch(self):
        self.log.append("batch_fetch_" + name)
        return [self.canned.get(name, {}).get(n, DEFAULTS[name]) for n in self.lengths]
    return fetch


for _p in PASSES:
    setattr(RecordingContext, "set_" + _p, _switch("set_" + _p))
for _f in DEFAULTS:
    setattr(RecordingContext, "batch_fetch_" + _f, _fetch(_f))


def make_counter(pm, pm_mod, cfg):
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], context=RecordingContext())
    repeat, prefix, suffix = cfg["repeat"]["c9orf72"][3:6]
    rc.add_target("c9orf72", repeat, prefix, suffix, alt_units=["GGCCTG"], tracts=(("GGCCCC", "GGCCTG"), ("",)))
    return rc


@pytest.fixture()
def rc(pm, pm_mod, cfg):
    return make_counter(pm, pm_mod, cfg)


def ask(rc, names, anchored=6.5, renorm=0.4):
    """The counter's switches of `names` on; the keywords of detect_batch for the rest of them."""
    kw = {}
    for n in names:
        if n in KEYWORDS:
            kw[n] = True
        elif n == "anchored":
            kw[n] = anchored
        elif n == "renorm":
            rc.set_renorm(renorm)
        else:
            getattr(rc, "set_" + n)(True)
    return kw


def read(n, dtype=np.int16):
    return np.zeros(n, dtype)


def expected_on(names, anchored=6.5, renorm=0.4):
    return [("set_" + p, True) + ((anchored,) if p == "anchored" else (renorm,) if p == "renorm" else ()) for p in PASSES if p in names]


def check_bracket(log, names, run="detect_batch_reads", with_mod=True):
    """One run of `log`: exactly the switches of `names` on, in order, then the run call, then exactly their fetches, then every
    switch off.  Returns the run call's entry."""
    at = [i for i, e in enumerate(log) if isinstance(e, tuple) and e[0] == run]
    assert len(at) == 1, log
    assert log[:at[0]] == expected_on(names)
    rest = log[at[0] + 1:]
    fetches = [e for e in rest if isinstance(e, str)]
    assert sorted(fetches) == sorted(["batch_fetch_" + p for p in names] + (["batch_fetch_mod"] if with_mod else []))
    offs = rest[len(fetches):]
    assert rest[:len(fetches)] == fetches                           # no switch goes off before the last fetch
    assert sorted(offs) == sorted(("set_" + p, False) for p in PASSES)
    return log[at[0]]


ALONE = [("anchored",), ("anchored", "anchored_mod"), ("units",), ("confidence",), ("mod_llr",), ("variants",), ("renorm",), ("tracts",), ("flank_mod",)]


@pytest.mark.parametrize("names", ALONE + [(), PASSES], ids=lambda n: "+".join(n) or "none")
def test_switch_sequence(rc, names):
    kw = ask(rc, names)
    plus = rc.targets["c9orf72"][0].target_id
    rc.detect_batch([("c9orf72", read(11), "+"), ("c9orf72", read(12), "+")], **kw)
    assert check_bracket(rc.ctx.log, names) == ("detect_batch_reads", "int16", (plus, plus))


def test_no_mod_fetch_without_a_modification_model(pm, cfg):
    rc = make_counter(pm, None, cfg)
    rc.detect_batch([("c9orf72", read(11), "+")], units=True)
    check_bracket(rc.ctx.log, ("units",), with_mod=False)


def test_switches_go_off_when_the_run_raises(rc):
    kw = ask(rc, PASSES)
    rc.ctx.fail = "detect_batch_reads"
    with pytest.raises(RuntimeError, match="the run failed"):
        rc.detect_batch([("c9orf72", read(11), "+")], **kw)
    log = rc.ctx.log
    assert log[:len(PASSES)] == expected_on(PASSES) and log[len(PASSES)][0] == "detect_batch_reads"
    assert sorted(log[len(PASSES) + 1:]) == sorted(("set_" + p, False) for p in PASSES)


def test_switches_go_off_when_mod_llr_is_refused(rc):
    kw = ask(rc, PASSES)
    rc.ctx.fail = "set_mod_llr"
    with pytest.raises(ffi.StriqueHipError):
        rc.detect_batch([("c9orf72", read(11), "+")], **kw)
    log = rc.ctx.log
    # the switches in front of mod_llr went on, mod_llr was tried, nothing ran, and every switch was turned off
    assert log[:5] == [("set_anchored", True, 6.5), ("set_anchored_mod", True), ("set_units", True), ("set_confidence", True), ("set_mod_llr", True)]
    assert sorted(log[5:]) == sorted(("set_" + p, False) for p in PASSES)


def test_scan_switches_units_only(rc):
    plus, minus = (tc.target_id for tc in rc.targets["c9orf72"])
    got = rc.scan_batch([read(11)], min_score=5.0, units=True)
    assert check_bracket(rc.ctx.log, ("units",), run="scan_batch_reads") == ("scan_batch_reads", (plus, minus), 5.0)
    assert got == [("c9orf72", "+", ((11, 0.0, 0.0, -1.5, 0, 0, "-"), None))]
    del rc.ctx.log[:]
    assert rc.scan_batch([read(11)], min_score=5.0) == [("c9orf72", "+", (11, 0.0, 0.0, -1.5, 0, 0, "-"))]
    check_bracket(rc.ctx.log, (), run="scan_batch_reads")


# ---- canned records and what the counter makes of them ---------------------------------------------------------------------------
def row(n, mod="-"):
    return (n, 0.0, 0.0, -1.5, 0, 0, mod)


def _fit(a, b, w, fitted, score):
    return (a, b, w, fitted, score)


def can_everything(ctx):
    """Reads of 11 and 12 samples with a record of every pass; a read of 13 samples keeps the defaults."""
    ctx.canned = {
        "mod": {11: "01", 12: "1"},
        "units": {11: np.array([3, 7], np.int64)},
        "confidence": {11: (-10.5, 4.25, 0.5)},
        "mod_llr": {11: np.array([[1.0, 3.5], [2.0, -1.0]])},
        "anchored": {11: _struct(ffi.ANCHORED_DTYPE, kind=2, status=0, count=7, log_p=-12.5, begin=100, end=400, free_samples=5),
                     12: _struct(ffi.ANCHORED_DTYPE, kind=3, status=1),
                     14: _struct(ffi.ANCHORED_DTYPE, kind=1)},
        "anchored_mod": {11: ("01", np.array([[0.5, 1.5], [2.0, 1.0]])), 12: ("10", None)},
        # one base passage and one passage through the alt unit; V as the fetch hands it out, [n_passages, n_branches]
        "variants": {11: (5, np.array([0, 1], np.int8), np.array([40, 90], np.int64), np.array([-1.0, -5.0, -7.0, -2.0]))},
        "renorm": {11: _struct(ffi.RENORM_DTYPE, applied=1, fit=[_fit(40, -2, 13, 1, -77), _fit(41, 3, 12, 1, -99), _fit(9, 9, 9, 0, 9)])},
        "tracts": {11: _struct(ffi.TRACTS_DTYPE, status=0, n_tracts=3, count=[4, 5, 6], log_p=-33.25),
                   12: _struct(ffi.TRACTS_DTYPE, status=0, n_tracts=2, count=[8, 9, 77], log_p=-2.5)},
        "flank_mod": {11: np.array([(1, 17, 2, 9, 0, 0, 50, 80, -20.0, -18.5), (0, 3, 1, 6, 2, 0, -1, -1, 0.0, 0.0)], ffi.FLANK_MOD_DTYPE)},
    }


def test_records(rc):
    """records=True: every field of Detected holds the converted value of the canned record."""
    kw = ask(rc, PASSES)
    can_everything(rc.ctx)
    plus, minus = (tc.target_id for tc in rc.targets["c9orf72"])
    got =rc.detect_batch([("c9orf72", read(11), "-"), ("c9orf72", read(12), "+"), ("c9orf72", read(13), "+")], records=True, **kw)
    m = rc.variant_models[minus]
    assert (m.context_units, m.n_branches) == (1, 2)
    a, b, c = got
    assert all(type(d) is Detected for d in got)
    assert Detected._fields == ("row", "units", "conf", "llr", "anchored", "variants", "renorm", "anchored_mod", "flank_mod", "tracts")
    # the read of 11 samples, on the - strand
    assert a.row == row(11, "01")
    assert a.units.tolist() == [3, 7] and a.units.dtype == np.int64
    assert a.conf == (-10.5, 4.25, 0.5)
    assert a.llr.tolist() == [2.5, -3.0]
    assert a.anchored == (2, 0, 7, -12.5, 100, 400, 5) and [type(x) for x in a.anchored] == [int, int, int, float, int, int, int]
    assert a.anchored_mod[0] == "01" and a.anchored_mod[1].tolist() == [1.0, -1.0]
    count_v, pattern, branch, end, V = a.variants
    assert (count_v, pattern) == (5, "0" + "0" * 1 + "1") and pattern == "0" + "0" * m.context_units + "1"
    assert branch.tolist() == [0, 1] and end.tolist() == [40, 90]
    assert V.shape == (2, m.n_branches) and V.tolist() == [[-1.0, -5.0], [-7.0, -2.0]]
    assert a.renorm == (1, {"morph": (40, -2, 13, -77), "filtered": (41, 3, 12, -99), "raw": None})
    assert a.tracts == ((6, 5, 4), -33.25)                          # three tracts on the - strand: back in the configured order
    assert a.flank_mod == [(1, 17, 2, 9, 0, 50, 80, 1.5), (0, 3, 1, 6, 2, -1, -1, 0.0)]
    assert [type(x) for x in a.flank_mod[0]] == [int] * 7 + [float]
    # the read of 12 samples, on the + strand: a call without score pairs, a two-tract record, nothing else
    assert b.row == row(12, "1")
    assert b.anchored == (3, 1, 0, 0.0, 0, 0, 0)
    assert b.anchored_mod == ("10", None)
    assert b.tracts == ((8, 9), -2.5)
    assert (b.units, b.conf, b.llr, b.variants, b.flank_mod) == (None,) * 5
    assert b.renorm == (0, {"morph": None, "filtered": None, "raw": None})
    # the read of 13 samples: no record anywhere; a tract record of status 1 is None
    assert c == Detected(row(13), None, None, None, (0, 0, 0, 0.0, 0, 0, 0), None, (0, {"morph": None, "filtered": None, "raw": None}), None, None, None)
    assert [e for e in rc.ctx.log if isinstance(e, tuple) and e[0] == "detect_batch_reads"] == [("detect_batch_reads", "int16", (minus, plus, plus))]


def test_records_hold_none_for_what_was_not_asked(rc):
    can_everything(rc.ctx)
    got = rc.detect_batch([("c9orf72", read(11), "+")], units=True, records=True)[0]
    assert got.row == row(11, "01") and got.units.tolist() == [3, 7]
    assert got[2:] == (None,) * 8
    assert rc.detect_batch([("c9orf72", read(11), "+")], records=True) == [Detected(row(11, "01"), None, None, None)]


def test_legacy_tuple(rc):
    """Without records: (row, units, conf, llr, anchored, anchored_mod, variants, tracts, flank_mod), restricted to what was asked;
    renorm is never in it; the bare row when nothing was asked."""
    can_everything(rc.ctx)
    items = [("c9orf72", read(11), "+")]
    assert rc.detect_batch(items) == [row(11, "01")]
    assert rc.detect("c9orf72", read(11), "+") == row(11, "01")
    rc.set_renorm(0.4)
    assert rc.detect_batch(items) == [row(11, "01")]                 # renorm is reported in Detected only
    kw = ask(rc, PASSES)
    got = rc.detect_batch(items, **kw)[0]
    assert len(got) == 9 and got[0] == row(11, "01")
    assert got[1].tolist() == [3, 7]
    assert got[2] == (-10.5, 4.25, 0.5)
    assert got[3].tolist() == [2.5, -3.0]
    assert got[4] == ("ends_in_repeat", 7, -12.5, 100, 400, 5)
    assert got[5][0] == "01" and got[5][1].tolist() == [1.0, -1.0]
    assert got[6][:2] == (5, "001")
    assert got[7] == ((4, 5, 6), -33.25)
    assert got[8] == [(1, 17, 2, 9, 0, 50, 80, 1.5), (0, 3, 1, 6, 2, -1, -1, 0.0)]
    for p in ("anchored_mod", "variants", "tracts", "flank_mod"):
        getattr(rc, "set_" + p)(False)
    rc.set_renorm(None)
    # subsets keep the order
    got = rc.detect_batch(items, confidence=True, anchored=6.5)[0]
    assert got == (row(11, "01"), (-10.5, 4.25, 0.5), ("ends_in_repeat", 7, -12.5, 100, 400, 5))
    rc.set_tracts(True); rc.set_variants(True)
    got = rc.detect_batch(items, units=True)[0]
    assert len(got) == 4 and got[1].tolist() == [3, 7] and got[2][:2] == (5, "001") and got[3] == ((4, 5, 6), -33.25)
    rc.set_variants(False); rc.set_flank_mod(True)
    got = rc.detect_batch(items, mod_llr=True)[0]
    assert len(got) == 4 and got[1].tolist() == [2.5, -3.0] and got[2] == ((4, 5, 6), -33.25) and got[3][0] == (1, 17, 2, 9, 0, 50, 80, 1.5)


def test_legacy_anchored_element(rc):
    """None for kinds 0 and 1, (name, count, log_p, begin, end, free_samples) for kinds 2 and 3 -- whatever the status."""
    can_everything(rc.ctx)
    got = rc.detect_batch([("c9orf72", read(n), "+") for n in (13, 14, 11, 12)], anchored=6.5)
    assert got == [(row(13), None), (row(14), None), (row(11, "01"), ("ends_in_repeat", 7, -12.5, 100, 400, 5)),
                   (row(12, "1"), ("starts_in_repeat", 0, 0.0, 0, 0, 0))]


def test_mixed_batch(rc):
    """One int16 and one float64 read: two device batches, each bracketed by the switches, the results in input order."""
    can_everything(rc.ctx)
    rc.set_tracts(True)
    plus, minus = (tc.target_id for tc in rc.targets["c9orf72"])
    items = [("c9orf72", np.full(12, 0.5), "-"), ("c9orf72", read(11), "+"), ("c9orf72", np.full(13, 40000, np.int32), "+")]
    got = rc.detect_batch(items, units=True, records=True)
    assert [d.row for d in got] == [row(12, "1"), row(11, "01"), row(13)]
    assert [d.tracts for d in got] == [((9, 8), -2.5), ((4, 5, 6), -33.25), None]
    assert got[1].units.tolist() == [3, 7] and got[0].units is None
    log = rc.ctx.log
    first, half = [i for i, e in enumerate(log) if e == ("set_units", True)]          # each batch begins with its first switch
    assert first == 0
    assert check_bracket(log[:half], ("units", "tracts")) == ("detect_batch_reads", "int16", (plus,))
    assert check_bracket(log[half:], ("units", "tracts")) == ("detect_batch_reads", "float64", (minus, plus))


# ---- ValueErrors -------------------------------------------------------------------------------------------------------------------
def raises(text):
    return pytest.raises(ValueError, match="^" + re.escape(text) + "$")


def test_validation(rc, pm, cfg):
    items = [("c9orf72", read(11), "+")]
    bare = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], context=RecordingContext())
    repeat, prefix, suffix = cfg["repeat"]["c9orf72"][3:6]
    bare.add_target("c9orf72", repeat, prefix, suffix)
    with raises("RepeatCounter: mod_llr needs a modification model."):
        bare.detect_batch(items, mod_llr=True)
    for bad in (0, -1.0, float("nan")):
        with raises("RepeatCounter: the anchored score threshold must be above 0."):
            rc.detect_batch(items, anchored=bad)
    rc.set_anchored_mod(True)
    with raises("RepeatCounter: anchored_mod needs anchored=m (the calls hang on the anchored records)."):
        rc.detect_batch(items)
    rc.set_anchored_mod(False)
    with raises("RepeatCounter: Target with name fmr1 not defined."):
        rc.detect_batch([("fmr1", read(11), "+")])
    with raises("RepeatCounter: Strand must be + or -."):
        rc.detect_batch([("c9orf72", read(11), "*")])
    with raises("RepeatCounter: Target with name c9orf72 already defined."):
        rc.add_target("c9orf72", repeat, prefix, suffix)
    assert rc.ctx.log == [] and bare.ctx.log == []                   # nothing was switched or run
    # the switches
    with raises("RepeatCounter: tracts needs a target added with tracts=(units, linkers)."):
        bare.set_tracts(True)
    with raises("RepeatCounter: variants needs a target added with alt_units."):
        bare.set_variants(True)
    with raises("RepeatCounter: flank_mod needs a modification model."):
        bare.set_flank_mod(True)
    with raises("RepeatCounter: anchored_mod needs a modification model."):
        bare.set_anchored_mod(True)
    for bad in (0, 1, -0.5, 2.5, float("nan")):
        with raises("RepeatCounter: the renorm share threshold must be inside (0, 1)."):
            rc.set_renorm(bad)
    for p in ("tracts", "variants", "flank_mod", "anchored_mod"):
        getattr(bare, "set_" + p)(False)                             # off is always fine
    # scan_batch
    with raises("RepeatCounter: scan_batch needs min_score (there is no default: see README, 'Scan')."):
        rc.scan_batch([read(11)])
    for bad in (0, -2.0):
        with raises("RepeatCounter: min_score must be above 0."):
            rc.scan_batch([read(11)], min_score=bad)
    with raises("RepeatCounter: Target with name fmr1 not defined."):
        rc.scan_batch([read(11)], targets=["fmr1"], min_score=5.0)
    with raises("RepeatCounter: no targets to scan for."):
        rc.scan_batch([read(11)], targets=[], min_score=5.0)
    rc.set_renorm(0.4)
    with raises("RepeatCounter: renorm is not available in a scan (set_renorm(None) first)."):
        rc.scan_batch([read(11)], min_score=5.0)
    rc.set_renorm(None); rc.set_tracts(True)
    with raises("RepeatCounter: tracts are not available in a scan (set_tracts(False) first)."):
        rc.scan_batch([read(11)], min_score=5.0)
    assert rc.ctx.log == []
