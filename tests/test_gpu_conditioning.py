"""The conditioning kernels (strique_amd/csrc/cond_kernels.hip) against the CPU oracle, bit for bit and over whole reads: the
median-filtered signal (strq_debug_filtered), the 8-bit morphology levels, their values and the scalars (strq_debug_conditioning)
-- at tile, vector and histogram seams, behind prefixes of every residue mod 8, over value ranges that leave the LDS windows, on
the vector and the scalar int16 route, for the last of several sub-batches and for a sub-batch conditioned in two upload parts.

The case lists and the statement of which kernel path a read takes are in tests/cond_cases.py; tests/test_cond_cases_host.py
proves on the host that the lists reach every path.  Rows are not asserted here: most of these reads fail the gate."""
from collections import Counter

import numpy as np
import pytest

import cond_cases as cc

pytestmark = pytest.mark.gpu

_EXPECTED = {}
_SEEN = Counter()          # class -> reads compared (classes as for a batch buffer on a 16-byte boundary)
_RAN = set()


def _expected(orc, opm, batch):
    if batch.name not in _EXPECTED:
        from conftest import oracle_map
        _EXPECTED[batch.name] = oracle_map(lambda c: cc.expected(orc, opm, c), batch.cases)
    return _EXPECTED[batch.name]


def _batch(name):
    return [b for b in cc.all_batches() if b.name == name][0]


@pytest.fixture(scope="module")
def mod_counter(pm, pm_mod, cfg, targets):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", *targets["c9orf72"])
    return rc


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _run_and_compare(counter, orc, opm, batch, options=(), mod=False):
    ctx = counter.ctx
    exp = _expected(orc, opm, batch)
    tid = counter._classifier_for("c9orf72", "+").target_id
    flat = np.concatenate([c.signal for c in batch.cases]).astype(batch.dtype, copy=False)
    options = tuple(options) + ((("STRQ_SUBBATCH_READS", str(batch.sub)),) if batch.sub else ())
    for k, v in options:
        ctx.set_option(k, v)
    try:
        rows = ctx.detect_batch(flat, cc.offsets(batch), [tid] * len(batch.cases))
    finally:
        for k, _ in options:
            ctx.set_option(k, None)
    first = not any(k == batch.name for k, _, _ in _RAN)
    _RAN.add((batch.name, options, mod))
    for i, j, at, rel in cc.compared(batch):
        c, e = batch.cases[i], exp[i]
        s, n, what = c.signal, len(c.signal), (batch.name, c.name, options)
        if first:
            _SEEN.update(cc.classify(c, batch.dtype, cc.phase(batch, at, rel), e))
        # int16: also the raw signal's tails decide the status of a read with a modification model
        ok = e.ok and (not mod or batch.dtype != np.int16 or bool(np.isfinite(e.r_tails[0]) and e.r_tails[1] > 0))
        assert rows["status"][i] == (0 if ok else 1), what
        flt = ctx.debug_filtered(j, n, batch.dtype)
        assert flt.dtype == e.flt.dtype == s.dtype and len(flt) == n, what
        bad = np.flatnonzero(~((flt == e.flt) | ((flt != flt) & (e.flt != e.flt))))
        assert len(bad) == 0, what + ("filtered", n, bad[:8], flt[bad[:8]], e.flt[bad[:8]])
        if n >= 2 and not np.isnan(s[[0, 1, -2, -1]].astype(np.float64)).any():
            # the zero pad at both ends, stated on its own: a neighbouring read's sample in its place gives another median
            assert flt[0] == sorted([0, s[0], s[1]])[1] and flt[-1] == sorted([s[-2], s[-1], 0])[1], what
        if n == 0:
            continue
        lv, lval, sc = ctx.debug_conditioning(j, n)
        assert _same(sc[0:2], [e.med, e.mad]), what + (sc[0:2], e.med, e.mad)
        assert _same(sc[2:4], e.f_tails), what + (sc[2:4], e.f_tails)
        if mod:
            assert _same(sc[6:8], e.r_tails), what + (sc[6:8], e.r_tails)
        if e.u8 is None:
            assert "degenerate" in c.tags, what
            continue
        bad = np.flatnonzero(lv != e.u8)
        assert len(bad) == 0, what + ("levels", n, cc.phase(batch, at, rel), bad[:8], lv[bad[:8]], e.u8[bad[:8]])
        uq, at_first = np.unique(e.u8, return_index=True)
        assert np.array_equal(lval[uq], e.morph[at_first].astype(np.float32), equal_nan=True), what
        assert _same(sc[4:6], e.m_tails), what + (sc[4:6], e.m_tails)


ROUTES = {"vector": (), "scalar": (("STRQ_COND_SCALAR", "1"),)}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", ["int16_edges", "int16_leak", "int16_ranges"])
def test_int16_reads(gpu_counter, orc, opm, name, route):
    """Both int16 routes against the oracle (and so against each other): 16-byte loads with masked partial vectors, and the
    scalar kernel."""
    _run_and_compare(gpu_counter, orc, opm, _batch(name), ROUTES[route])


@pytest.mark.parametrize("name", ["int16_ranges", "float64_edges"])
def test_raw_signal_statistics_of_the_modification_route(mod_counter, orc, opm, name):
    _run_and_compare(mod_counter, orc, opm, _batch(name), mod=True)


def test_float64_reads(gpu_counter, orc, opm):
    _run_and_compare(gpu_counter, orc, opm, _batch("float64_edges"))


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("residue", range(8))
def test_last_sub_batch_int16(gpu_counter, orc, opm, residue, route):
    """The last sub-batch starts `residue` samples behind a multiple of 8: its filtered signal and its levels are shifted inside
    their buffers by that phase."""
    _run_and_compare(gpu_counter, orc, opm, _batch("sub_batch_r%d_int16" % residue), ROUTES[route])


@pytest.mark.parametrize("residue", range(2))
def test_last_sub_batch_float64(gpu_counter, orc, opm, residue):
    _run_and_compare(gpu_counter, orc, opm, _batch("sub_batch_r%d_float64" % residue))


@pytest.mark.parametrize("threads", ["0", "3"])
def test_sub_batch_conditioned_in_two_upload_parts(gpu_counter, orc, opm, threads):
    """1100 reads from a host buffer: the library uploads and conditions a sub-batch of 1024 reads or more in two parts (the
    second with its read table starting in the middle of the sub-batch), through the pageable path and through staging threads."""
    _run_and_compare(gpu_counter, orc, opm, _batch("two_parts"), (("STRQ_UPLOAD_THREADS", threads),))


def test_every_class_was_compared():
    """One line per class of tests/cond_cases.py with the number of reads compared (first run of every batch)."""
    for cls in sorted(_SEEN):
        print("conditioning class %-48s %5d reads" % (cls, _SEEN[cls]))
    if {k for k, _, _ in _RAN} >= {b.name for b in cc.all_batches()}:          # the whole module ran
        missing = sorted(cc.required_classes() - set(_SEEN))
        assert not missing, missing
